"""GPU tests of the cubed-sphere put (ghx_cs_put_create, k_put_cs) and of the cubed-sphere bulk
object built on it (structured.cubed_sphere.make_bulk_communication_object): halos copied field
to field, rotated and negated on the way, with no buffer. Every field is compared bit for bit with
the expectation expanded from the recorded reference fixture (tests/cs_cases.py)."""
import ctypes

import numpy as np
import pytest

from tests import cs_cases
from tests.cs_cases import ArenaField, DomainField, dense_strides, from_device, to_device
from tests.cs_put_cases import (K_FAST, X_FAST, Y_FAST, Z_FAST, Field, Puts, cs_item,
                                emulated_ranks, field_desc, value_kind)

pytestmark = pytest.mark.gpu

REFERENCE_FIELDS = [("float64", 1, False, X_FAST), ("float32", 3, True, X_FAST)]
# tests/test_gpu_cs_self.py's TYPES
TYPES = [("float64", 1, False), ("float32", 3, True), ("float64", 3, True), ("int32", 3, True),
         ("int64", 3, True)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ghex_amd
    ghex_amd.native_library()


def _one_rank(cfg, specs):
    """All domains of `cfg` on one rank (world 1: no epochs, no IPC mapping) with one field per
    spec (dtype, nc, vector, layout) and domain, spec-major, all added to one cubed-sphere bulk
    object: (bulk object, [(DomainField, base, layout)])."""
    import ghex_amd
    from ghex_amd.structured import cubed_sphere as CS
    cube = CS.Cube(cfg["edge_size"], cfg["levels"])
    ctx = ghex_amd.make_context()
    dds = [CS.DomainDescriptor(cube, d["tile"], *d["x"], *d["y"]) for d in cfg["domains"]]
    pc = CS.make_pattern(ctx, CS.HaloGenerator(cfg["halos"]), dds)
    bco = CS.make_bulk_communication_object(ctx)
    fields = []
    for dtype, nc, vector, layout in specs:
        for di, dd in enumerate(dds):
            df = DomainField(cfg, di, dtype, nc, vector, special=vector)
            base, logical = to_device(df.initial(), layout, dtype)
            bco.add_field(pc(CS.FieldDescriptor(dd, logical, df.offsets, df.extents, nc, vector)))
            fields.append((df, base, layout))
    return bco, fields


def _check(fields, what=None):
    for df, base, layout in fields:
        got, exp = from_device(base, layout, df.dtype), df.expected()
        assert np.array_equal(got, exp), (what, df.di, str(df.dtype), np.argwhere(got != exp)[:5])


def _put_info(h):
    from ghex_amd import _ghx
    p, r, x = (ctypes.c_int32(-1) for _ in range(3))
    _ghx.call("ghx_cs_put_info", h, ctypes.byref(p), ctypes.byref(r), ctypes.byref(x))
    return dict(pair_tiles=p.value, records=r.value, x_tiles=x.value)


def _message_bytes(cfg, specs):
    """The bytes of every message of one exchange, from the fixture's intersections."""
    cells = 0
    for dom in cfg["domains"]:
        for b in dom["boxes"]:
            for x in b["x"]:
                cells += int(np.prod([x[4 + d] - x[1 + d] + 1 for d in range(3)]))
    return sum(cells * nc * cs_cases.elem_size(dtype) for dtype, nc, _, _ in specs)


@pytest.mark.parametrize("layout", [X_FAST, Y_FAST, Z_FAST, K_FAST], ids="xyzk")
def test_one_rank_layouts_and_types(layout):
    """c = 6, halos (1, 2, 0, 3), six domains, five fields per domain in one exchange; the
    integer vectors carry the cells where a negation by halves fails."""
    cfg = cs_cases.config(6)
    specs = [t + (layout,) for t in TYPES]
    bco, fields = _one_rank(cfg, specs)
    bco.exchange().wait()
    _check(fields, layout)
    assert bco._ep is None and bco._co is None
    assert bco.bytes_per_exchange() == _message_bytes(cfg, specs)


def test_reference_geometry_takes_one_launch_per_put_plan():
    """c = 10, 24 domains, halo 2, a scalar f64 and a 3-vector f32 per domain, x stride-1: 48
    fields, 336 messages in several put plans (put_chunks). One launch per plan — k_put_cs for a
    plan with put tile records, k_put for one without —, no buffer anywhere, the message bytes
    moved once."""
    import torch
    from ghex_amd import _ghx
    cfg = cs_cases.config(10)
    bco, fields = _one_rank(cfg, REFERENCE_FIELDS)
    bco.init()
    assert len(fields) == 48 and len(bco._puts) > 1
    before = torch.cuda.memory_allocated()
    ms, n = (ctypes.c_float * 64)(), ctypes.c_int32()
    _ghx.call("ghx_launch_timing", 1)
    try:
        bco.exchange().wait()
        _ghx.call("ghx_launch_timing_read", ms, 64, ctypes.byref(n))
    finally:
        _ghx.call("ghx_launch_timing", 0)
    _check(fields)
    assert n.value == len(bco._puts)
    infos = [_put_info(h) for h, *_ in bco._puts]
    # every plan is one launch of its pair tiles and put tiles together
    assert all(i["pair_tiles"] + i["x_tiles"] > 0 for i in infos)
    assert sum(i["records"] for i in infos) > 0
    assert torch.cuda.memory_allocated() == before and bco._co is None  # no send / recv buffers
    assert bco.bytes_per_exchange() == _message_bytes(cfg, REFERENCE_FIELDS)


def test_long_edge_boxes():
    """c = 70, 5 levels, halo 3, f64: each edge box spans several tiles and its rows are longer
    than a wave."""
    cfg = cs_cases.config(70)
    bco, fields = _one_rank(cfg, [("float64", 1, False, X_FAST)])
    bco.exchange().wait()
    _check(fields)
    infos = [_put_info(h) for h, *_ in bco._puts]
    assert sum(i["x_tiles"] for i in infos) > sum(i["records"] for i in infos) > 0


# ---------------------------------------------------------------------------------------------
# the byte-wide path, through the C ABI with raw pointers
# ---------------------------------------------------------------------------------------------
def _arena_puts(dtype, nc, layout, src_shift=0, dst_shift=0, pad=None, odd_domain=0):
    """The six-domain cube on one emulated rank with every field in a byte arena, read from one
    set of arenas and written into another: every source base is src_shift bytes off, every
    destination base dst_shift bytes off, and domain `odd_domain`'s field (both of its arenas)
    is pitched with `pad`. Whole arenas are compared, guard bytes and padding included: the
    destinations with the expectation, the sources with what they held."""
    import torch
    cfg = cs_cases.config(6)
    elem = cs_cases.elem_size(dtype)
    (mine, dds, pc), = emulated_ranks(cfg, lambda i, dom: 0)
    bis, srcs, dsts, dptr = [], [], [], []
    for i, dd in zip(mine, dds):
        df = DomainField(cfg, i, dtype, nc, True, special=True)
        strides = dense_strides(df.shape, layout, elem, pad if i == odd_domain else None)
        sa, da = ArenaField(df, strides, src_shift), ArenaField(df, strides, dst_shift)
        assert sa.layout() == layout
        sdev = torch.from_numpy(sa.arena(df.initial())).cuda()
        ddev = torch.from_numpy(da.arena(df.initial())).cuda()
        assert sdev.data_ptr() % 256 == 0 and ddev.data_ptr() % 256 == 0
        desc = field_desc(df.shape, df.offsets + (0,), layout, elem, strides)
        item = cs_item(cfg, cfg["domains"][i], True, value_kind(dtype, True))
        bis.append(pc(Field(desc, item, dd.domain_id(), sdev.data_ptr() + sa.base)))
        srcs.append((sa, sdev))
        dsts.append((da, ddev))
        dptr.append(ddev.data_ptr() + da.base)
    puts = Puts([bis], dst_ptrs=[dptr])
    try:
        info = puts.info()
        assert info["records"] > 0
        puts.execute(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        puts.close()
    for (sa, sdev), (da, ddev) in zip(srcs, dsts):
        a, exp = ddev.cpu().numpy(), da.arena(da.df.expected())
        assert np.array_equal(a, exp), (da.df.di, np.flatnonzero(a != exp)[:8] - da.base)
        assert np.array_equal(sdev.cpu().numpy(), sa.arena(sa.df.initial())), sa.df.di
    return bis


@pytest.mark.parametrize("dtype,nc", [("float32", 3), ("int64", 2)])
@pytest.mark.parametrize("layout", [X_FAST, Z_FAST], ids="xz")
@pytest.mark.parametrize("what", ["aligned", "source", "destination", "stride"])
def test_one_misaligned_side_takes_the_bytewise_path(what, layout, dtype, nc):
    """One byte off, each alone: every source base, every destination base, or one stride of one
    domain's field (the second-fastest dim pitched by a byte). Vector fields, so the negation runs
    between byte-wise loads and stores. "aligned" is the same set-up with nothing shifted."""
    order = cs_cases.layout_order(layout)
    kw = dict(aligned={}, source=dict(src_shift=1), destination=dict(dst_shift=1),
              stride=dict(pad={order[-2]: 1}))[what]
    bis = _arena_puts(dtype, nc, layout, **kw)
    elem = cs_cases.elem_size(dtype)
    odd = [s for s in bis[0].field.desc.byte_strides if s % elem]
    assert bool(odd) == (what == "stride")


# ---------------------------------------------------------------------------------------------
# tuning, emulated ranks, graph capture
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", [{"x_tile_elems": 32}, {"x_tile_elems": 48},
                                   {"x_tile_elems": 4096}, {"grid_cap": 1}, {"grid_cap": 7}],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_tile_sizes_and_fewer_workgroups_than_tiles(knobs):
    """x_tile_elems is read when the put is planned, grid_cap at the launch: one workgroup (or
    seven) walks pair tiles and put tiles grid-stride. c = 6, an f64 scalar and an f32 3-vector."""
    from ghex_amd import _ghx
    cfg = cs_cases.config(6)

    def tiles(bco):
        infos = [_put_info(h) for h, *_ in bco._puts]
        return sum(i["pair_tiles"] for i in infos), sum(i["x_tiles"] for i in infos)
    default, _ = _one_rank(cfg, REFERENCE_FIELDS)
    default.init()
    try:
        for k, v in knobs.items():
            _ghx.call("ghx_tune", k.encode(), v)
        bco, fields = _one_rank(cfg, REFERENCE_FIELDS)
        bco.exchange().wait()
        _check(fields, knobs)
        (dp, dx), (p, x) = tiles(default), tiles(bco)
        assert p == dp > 0
        want = knobs.get("x_tile_elems", 256)
        # smaller tiles: more of them; larger ones: no more (this geometry's boxes are small)
        assert x > dx if want < 256 else x <= dx if want > 256 else x == dx
        if "grid_cap" in knobs:
            assert all(i["pair_tiles"] + i["x_tiles"] > knobs["grid_cap"]
                       for i in (_put_info(h) for h, *_ in bco._puts))
    finally:
        _ghx.call("ghx_tune", b"reset", 0)


def test_six_emulated_ranks_put_into_each_others_fields():
    """One tile per rank, c = 6, halos (1, 2, 0, 3), two fields of different layout per rank (an
    f32 2-vector x stride-1, an f64 scalar y stride-1). Every rank plans as the bulk object does
    (field_records without IPC export -> put_messages -> put_entries -> ghx_cs_put_create); the
    target pointers are the other ranks' tensors; all plans run on one stream."""
    import torch
    from ghex_amd.structured import cubed_sphere as CS
    cfg = cs_cases.config(6)
    bis_all, fields = [], []
    for mine, dds, pc in emulated_ranks(cfg, lambda i, dom: i):
        bis = []
        (i,), (dd,) = mine, dds
        for dtype, nc, vector, layout in (("float32", 2, True, X_FAST), ("float64", 1, False, Y_FAST)):
            df = DomainField(cfg, i, dtype, nc, vector)
            base, logical = to_device(df.initial(), layout, dtype)
            bis.append(pc(CS.FieldDescriptor(dd, logical, df.offsets, df.extents, nc, vector)))
            fields.append((df, base, layout))
        bis_all.append(bis)
    puts = Puts(bis_all)
    try:
        assert len(puts.plans) == 6 and all(puts.plans)
        assert puts.info()["bytes"] == _message_bytes(cfg, [("float32", 2, True, X_FAST),
                                                            ("float64", 1, False, Y_FAST)])
        puts.execute(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        puts.close()
    _check(fields)


def _expected_with_interior_flip(df, flip):
    """df.expected() when every interior cell of every domain has `flip` XORed into its bits
    (applied before a vector component's negation, as the exchange sees it)."""
    u = cs_cases.uint_of(df.dtype)
    a = df.initial()
    own = a != df.sentinel
    a[own] ^= u(flip)
    for b in df.dom["boxes"]:
        xs, ys, _ = df.box_values(b)
        saved, df.vector = df.vector, False
        _, _, plain = df.box_values(b)
        df.vector = saved
        bits = plain ^ u(flip)
        if df.vector:
            for comp in (0, 1):
                if comp < df.nc and b["sign"][comp] < 0:
                    bits[..., comp] = cs_cases.negate_bits(bits[..., comp], df.dtype)
        a[xs[0] + df.h:xs[-1] + df.h + 1, ys[0] + df.h:ys[-1] + df.h + 1] = bits
    return a


def test_exchange_replayed_from_a_linear_capture():
    """The one-rank c = 6 exchange (no epochs: one linear chain of put launches) captured into a
    graph; two replays with changed interiors."""
    import torch
    bco, fields = _one_rank(cs_cases.config(6), REFERENCE_FIELDS)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bco.exchange().wait()  # set-up and a warm run, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bco.exchange()
    for flip in (0x1, 0x2):
        # new interiors (low mantissa bits flipped), stale halos from the run before
        for df, base, layout in fields:
            a = from_device(base, layout, df.dtype).copy()
            first = df.initial()
            own = first != df.sentinel
            a[own] = first[own] ^ cs_cases.uint_of(df.dtype)(flip)
            order = cs_cases.layout_order(layout)
            base.copy_(torch.from_numpy(np.ascontiguousarray(a.transpose(order))
                                        .view(np.dtype(df.dtype))))
        g.replay()
        torch.cuda.synchronize()
        for df, base, layout in fields:
            exp = _expected_with_interior_flip(df, flip)
            got = from_device(base, layout, df.dtype)
            assert np.array_equal(got, exp), (df.di, str(df.dtype), flip)
