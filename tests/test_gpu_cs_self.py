"""GPU tests of the fused cubed-sphere self exchange (ghx_cs_exchange_self, k_self_cs): a whole
cube on one rank exchanged in ONE launch that packs, rotates and negates. Every field is compared
bit for bit with the expectation expanded from the recorded reference fixture (tests/cs_cases.py),
every send buffer with the buffer the plain three-launch path packs from identical fields."""
import ctypes

import numpy as np
import pytest

from tests import cs_cases
from tests.cs_cases import ArenaField, DomainField, dense_strides, from_device, to_device
from tests.gpu_util import FakeContext, emulated_exchange

pytestmark = pytest.mark.gpu

X_FAST, Y_FAST, Z_FAST, K_FAST = (3, 2, 1, 0), (2, 3, 1, 0), (1, 2, 3, 0), (0, 1, 2, 3)
REFERENCE_FIELDS = [("float64", 1, False, X_FAST), ("float32", 3, True, X_FAST)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ghex_amd
    ghex_amd.native_library()


def _one_rank(cfg, specs, **co_options):
    """All domains of `cfg` on one rank with one field per spec (dtype, nc, vector, layout) and
    domain, spec-major: (communication object, buffer infos, [(DomainField, base, layout)])."""
    import ghex_amd
    from ghex_amd.structured import cubed_sphere as CS
    cube = CS.Cube(cfg["edge_size"], cfg["levels"])
    ctx = ghex_amd.make_context()
    dds = [CS.DomainDescriptor(cube, d["tile"], *d["x"], *d["y"]) for d in cfg["domains"]]
    pc = CS.make_pattern(ctx, CS.HaloGenerator(cfg["halos"]), dds)
    bis, fields = [], []
    for dtype, nc, vector, layout in specs:
        for di, dd in enumerate(dds):
            df = DomainField(cfg, di, dtype, nc, vector, special=vector)
            base, logical = to_device(df.initial(), layout, dtype)
            bis.append(pc(CS.FieldDescriptor(dd, logical, df.offsets, df.extents, nc, vector)))
            fields.append((df, base, layout))
    return CS.make_communication_object(ctx, **co_options), bis, fields


def _check(fields, what=None):
    for df, base, layout in fields:
        got, exp = from_device(base, layout, df.dtype), df.expected()
        assert np.array_equal(got, exp), (what, df.di, str(df.dtype), np.argwhere(got != exp)[:5])


def _send_buffers(co, bis, fields):
    plan = co.plan(bis)
    send, _ = co.buffers(plan, fields[0][1].device)
    return [t[:x["size"]].cpu().numpy() for t, x in zip(send, plan.send)]


def _launches(co, bis):
    """The kernel launches of one exchange (ghx_launch_timing counts them on this thread)."""
    from ghex_amd import _ghx
    ms, n = (ctypes.c_float * 64)(), ctypes.c_int32()
    _ghx.call("ghx_launch_timing", 1)
    try:
        co.exchange(bis).wait()
        _ghx.call("ghx_launch_timing_read", ms, 64, ctypes.byref(n))
    finally:
        _ghx.call("ghx_launch_timing", 0)
    return n.value


def _fused_and_plain(cfg, specs, what=None):
    """One fused exchange and one plain exchange of identical fields: fields against the
    fixture, send buffers against each other. Returns the launch counts (fused, plain)."""
    co, bis, fields = _one_rank(cfg, specs, fuse_rotated=True)
    assert co.cs_self(co.plan(bis)) and not co.all_self(co.plan(bis))
    plain, pbis, pfields = _one_rank(cfg, specs, fuse_self=False)
    assert not plain.fuse_rotated
    counts = _launches(co, bis), _launches(plain, pbis)
    _check(fields, what)
    _check(pfields, what)
    got, exp = _send_buffers(co, bis, fields), _send_buffers(plain, pbis, pfields)
    assert len(got) == len(exp) > 0
    for i, (g, e) in enumerate(zip(got, exp)):
        assert np.array_equal(g, e), (what, i, np.flatnonzero(g != e)[:8])
    return counts


def test_reference_geometry_in_one_launch():
    """c = 10, 24 domains, halo 2 (test_cubed_sphere_exchange.cpp:945-955), a scalar f64 and a
    3-vector f32 per domain, x stride-1: one launch. The plain object takes at least three; with
    this geometry's 168 domain-pair buffers its pack, unpack and transformed plans each run in
    several launch groups of 64 buffer slots, so it takes more (the count is printed)."""
    fused, plain = _fused_and_plain(cs_cases.config(10), REFERENCE_FIELDS)
    print("launches: fused", fused, "plain", plain)
    assert fused == 1
    assert plain >= 3


def test_six_domains_take_one_launch_where_the_plain_object_takes_three():
    """One domain per tile (18 buffers: no launch groups): pack, ordinary unpack and k_unpack_x
    on the plain object, k_self_cs alone on the fused one."""
    specs = [("float64", 1, False, X_FAST), ("float32", 3, True, X_FAST)]
    assert _fused_and_plain(cs_cases.config(6), specs) == (1, 3)


TYPES = [("float64", 1, False), ("float32", 3, True), ("float64", 3, True), ("int32", 3, True),
         ("int64", 3, True)]


@pytest.mark.parametrize("layout", [X_FAST, Y_FAST, Z_FAST, K_FAST], ids="xyzk")
def test_layouts_and_types(layout):
    """c = 6, halos (1, 2, 0, 3), five fields per domain in one exchange; the integer vectors
    carry the cells where a negation by halves fails (0, the minimum, -1, words with a zero or
    all-ones low half)."""
    _fused_and_plain(cs_cases.config(6), [t + (layout,) for t in TYPES], layout)


def test_long_edge_boxes():
    """c = 70, 5 levels, halo 3, f64: each edge box spans several tiles and its rows are longer
    than a wave."""
    fused, _ = _fused_and_plain(cs_cases.config(70), [("float64", 1, False, X_FAST)])
    assert fused == 1


# ---------------------------------------------------------------------------------------------
# the byte-wide path, through the C ABI with raw pointers
# ---------------------------------------------------------------------------------------------
BUF_GUARD = 64


def _field_desc(af):
    from ghex_amd import _ghx
    df, layout = af.df, af.layout()
    fd = _ghx.FieldDesc()
    fd.dim, fd.elem_size = 4, af.elem
    for d in range(4):
        fd.layout[d] = layout[d]
        fd.byte_strides[d] = af.strides[d]
        fd.offsets[d] = df.offsets[d] if d < 3 else 0
        fd.extents[d] = df.shape[d]
    fd.num_components, fd.has_components = df.nc, 1
    return fd


def _cs_item(df):
    from ghex_amd import _ghx
    cs = _ghx.CsItem()
    cs.tile, cs.first_x, cs.first_y = df.dom["tile"], df.dom["x"][0], df.dom["y"][0]
    cs.edge_size = df.c
    cs.is_vector = 1 if df.vector else 0
    cs.value_kind = {"f": 1, "i": 2}.get(cs_cases.elem_kind(df.dtype), 0) if df.vector else 0
    return cs


def _arena_exchange(dtype, nc, layout, field_shift=0, buf_shift=0, pad=None, odd_domain=0):
    """The six-domain cube with every field in a byte arena; domain `odd_domain`'s field alone
    is shifted by field_shift bytes or pitched with `pad`, every buffer starts buf_shift bytes
    into its allocation. One ghx_cs_exchange_self; whole arenas and whole buffer allocations are
    compared (the buffers with what ghx_exchange_pack then packs from the same fields)."""
    import torch
    import ghex_amd
    from ghex_amd import _ghx
    from ghex_amd.communication_object import _ExchangePlan
    from ghex_amd.structured import cubed_sphere as CS
    cfg = cs_cases.config(6)
    cube = CS.Cube(cfg["edge_size"], cfg["levels"])
    dds = [CS.DomainDescriptor(cube, d["tile"], *d["x"], *d["y"]) for d in cfg["domains"]]
    pc = CS.make_pattern(ghex_amd.make_context(), CS.HaloGenerator(cfg["halos"]), dds)
    elem = cs_cases.elem_size(dtype)
    afs, devs, items, cs_items = [], [], [], []
    for di, dd in enumerate(dds):
        df = DomainField(cfg, di, dtype, nc, True, special=True)
        odd = di == odd_domain
        af = ArenaField(df, dense_strides(df.shape, layout, elem, pad if odd else None),
                        field_shift if odd else 0)
        assert af.layout() == layout
        dev = torch.from_numpy(af.arena(df.initial())).cuda()
        assert dev.data_ptr() % 256 == 0
        it = _ghx.ExchangeItem()
        it.pattern, it.local_index = pc.handle, pc.local_index(dd.domain_id())
        it.kind, it.field, it.align, it.tag_offset = 0, _field_desc(af), elem, 0
        afs.append(af)
        devs.append(dev)
        items.append(it)
        cs_items.append(_cs_item(df))
    plan = _ExchangePlan(items, cs_items)
    fus = ctypes.c_int32()
    _ghx.call("ghx_cs_self_info", plan.h, ctypes.byref(fus), None, None, None)
    assert fus.value == 1, _ghx.lib().ghx_last_error()

    def buffers():
        out = [torch.full((BUF_GUARD + buf_shift + x["size"] + BUF_GUARD,), 0x5A, dtype=torch.uint8,
                          device="cuda") for x in plan.send]
        assert all(t.data_ptr() % 256 == 0 for t in out)
        return out, _ghx.ptr_array([t.data_ptr() + BUF_GUARD + buf_shift for t in out])
    fp = _ghx.ptr_array([dev.data_ptr() + af.base for dev, af in zip(devs, afs)])
    s = torch.cuda.current_stream().cuda_stream
    got, gp = buffers()
    _ghx.call("ghx_cs_exchange_self", plan.h, fp, len(items), gp, len(got), s)
    torch.cuda.synchronize()
    for af, dev in zip(afs, devs):
        a, exp = dev.cpu().numpy(), af.arena(af.df.expected())
        assert np.array_equal(a, exp), (af.df.di, np.flatnonzero(a != exp)[:8] - af.base)
    exp, ep = buffers()  # the interiors are as they were: the ordinary pack gives the message
    _ghx.call("ghx_exchange_pack", plan.h, fp, len(items), ep, len(exp), s)
    torch.cuda.synchronize()
    for i, (g, e) in enumerate(zip(got, exp)):
        g, e = g.cpu().numpy(), e.cpu().numpy()
        assert np.array_equal(g, e), (i, np.flatnonzero(g != e)[:8] - BUF_GUARD - buf_shift)
    return items


@pytest.mark.parametrize("dtype,nc", [("float32", 3), ("int64", 2)])
@pytest.mark.parametrize("layout", [X_FAST, Z_FAST], ids="xz")
@pytest.mark.parametrize("what", ["aligned", "field", "buffer", "stride"])
def test_one_misaligned_side_takes_the_bytewise_path(what, layout, dtype, nc):
    """One byte off, each alone: one domain's field (the source of the tiles its neighbours
    receive, the destination of its own: each side alone in those tiles), every buffer, or one
    stride of one domain's field (the second-fastest dim pitched by a byte). Vector fields, so the
    negation runs between byte-wise loads and stores. "aligned" is the same set-up with nothing
    shifted."""
    order = cs_cases.layout_order(layout)
    kw = dict(aligned={}, field=dict(field_shift=1), buffer=dict(buf_shift=1),
              stride=dict(pad={order[-2]: 1}))[what]
    items = _arena_exchange(dtype, nc, layout, **kw)
    elem = cs_cases.elem_size(dtype)
    odd = [s for s in items[0].field.byte_strides if s % elem]
    assert bool(odd) == (what == "stride")


# ---------------------------------------------------------------------------------------------
# tuning, graph capture, fallback
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", [{"x_tile_elems": 32}, {"x_tile_elems": 48},
                                   {"x_tile_elems": 4096}, {"grid_cap": 1}, {"grid_cap": 7},
                                   {"grid_cap": 7, "x_tile_elems": 32}],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
@pytest.mark.parametrize("edge", [10, 70])
def test_tile_sizes_and_fewer_workgroups_than_tiles(edge, knobs):
    """x_tile_elems is read when the exchange is planned, grid_cap at the launch: one workgroup
    (or seven) walks pair tiles and self tiles grid-stride."""
    from ghex_amd import _ghx
    specs = REFERENCE_FIELDS if edge == 10 else [("float64", 1, False, X_FAST)]
    try:
        for k, v in knobs.items():
            _ghx.call("ghx_tune", k.encode(), v)
        fused, _ = _fused_and_plain(cs_cases.config(edge), specs, knobs)
        assert fused == 1
    finally:
        _ghx.call("ghx_tune", b"reset", 0)


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


def test_fused_exchange_replayed_from_a_linear_capture():
    """One fused exchange of the 24-domain geometry captured on one stream without branches; two
    replays with changed interiors."""
    import torch
    from ghex_amd import _ghx
    co, bis, fields = _one_rank(cs_cases.config(10), REFERENCE_FIELDS, fuse_rotated=True)
    # plain float cells only: the flips below must not turn a cell into the sentinel
    plan = co.plan(bis)
    assert co.cs_self(plan)
    send, _ = co.buffers(plan, fields[0][1].device)
    L = _ghx.lib()
    fp = _ghx.ptr_array([bi.field.data_ptr() for bi in bis])
    sp = _ghx.ptr_array([t.data_ptr() for t in send])

    def step(s):
        _ghx.check(L.ghx_cs_exchange_self(plan.h, fp, len(bis), sp, len(send), s), "cs self")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(side.cuda_stream)  # warm, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(torch.cuda.current_stream().cuda_stream)
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


def test_six_emulated_ranks_fall_back():
    """One tile per rank under fuse_rotated=True: every message has a peer, nothing is fusable,
    and the exchange is today's."""
    from ghex_amd.structured import cubed_sphere as CS
    cfg = cs_cases.config(6)
    cube = CS.Cube(cfg["edge_size"], cfg["levels"])
    table = [[(cube.edge_size, cube.levels, d["tile"], *d["x"], *d["y"])] for d in cfg["domains"]]
    cos, bis_all, fields = [], [], []
    for r, dom in enumerate(cfg["domains"]):
        ctx = FakeContext(r, 6, table)
        dd = CS.DomainDescriptor(cube, dom["tile"], *dom["x"], *dom["y"])
        pc = CS.make_pattern(ctx, CS.HaloGenerator(cfg["halos"]), [dd])
        bis = []
        for dtype, nc, vector, layout in (("float32", 2, True, X_FAST), ("float64", 1, False, Y_FAST)):
            df = DomainField(cfg, r, dtype, nc, vector)
            base, logical = to_device(df.initial(), layout, dtype)
            bis.append(pc(CS.FieldDescriptor(dd, logical, df.offsets, df.extents, nc, vector)))
            fields.append((df, base, layout))
        co = CS.make_communication_object(ctx, fuse_rotated=True)
        assert not co.cs_self(co.plan(bis))
        cos.append(co)
        bis_all.append(bis)
    emulated_exchange(cos, bis_all)
    _check(fields)
