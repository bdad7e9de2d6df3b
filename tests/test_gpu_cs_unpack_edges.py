"""GPU tests of the transformed cubed-sphere unpack (k_unpack_x) where its first tests do not
reach: every element width (1, 2, 4, 8, 16 bytes), 64-bit integer negation, the byte-wise path of
misaligned buffers, fields and strides, tile sizes other than the default (several loop trips per
tile, many evened tiles), fewer workgroups than tiles, 12-byte elements (the signed-stride
ordinary segments) and one exchange of mixed widths in more field slots than one launch takes.

Every expectation is a bit pattern expanded cell by cell from the recorded reference fixture
(tests/golden/cubed_sphere_case.json through tests/cs_cases.py) and compared with np.array_equal:
whole fields, or whole byte arenas with their guards and padding."""
import ctypes
import math

import numpy as np
import pytest

from tests import cs_cases
from tests.cs_cases import (ArenaField, DomainField, buffer_to_device, dense_strides, from_device,
                            to_device)

pytestmark = pytest.mark.gpu

X_FAST, Y_FAST, Z_FAST = (3, 2, 1, 0), (2, 3, 1, 0), (1, 2, 3, 0)
LAYOUT_ID = {X_FAST: "x", Y_FAST: "y", Z_FAST: "z"}
# every distinct transform: tile 0's domains 0 (-x, -y) and 3 (+x, +y), likewise tile 1's 4 and 7
DOMAINS = (0, 3, 4, 7)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ghex_amd
    ghex_amd.native_library()


def _tune(**knobs):
    from ghex_amd import _ghx
    for k, v in knobs.items():
        _ghx.call("ghx_tune", k.encode(), v)


def _reset():
    from ghex_amd import _ghx
    _ghx.call("ghx_tune", b"reset", 0)


def _info(h):
    from ghex_amd import _ghx
    n, t, r, b = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64()
    _ghx.call("ghx_cs_plan_info", h, ctypes.byref(n), ctypes.byref(b), ctypes.byref(t),
              ctypes.byref(r))
    return dict(records=n.value, bytes=b.value, tiles=t.value, rotated=r.value)


class _Pattern:
    """All domains of a configuration on one rank."""

    def __init__(self, cfg):
        import ghex_amd
        from ghex_amd.structured import cubed_sphere as CS
        self.cfg = cfg
        self.cube = CS.Cube(cfg["edge_size"], cfg["levels"])
        self.ctx = ghex_amd.make_context()
        self.dds = [CS.DomainDescriptor(self.cube, d["tile"], *d["x"], *d["y"])
                    for d in cfg["domains"]]
        self.pc = CS.make_pattern(self.ctx, CS.HaloGenerator(cfg["halos"]), self.dds)

    def info_of_one_field(self, di, desc, cs_item, align):
        """ghx_cs_plan_info of the exchange of domain di's field alone."""
        from ghex_amd import _ghx
        from ghex_amd.communication_object import _ExchangePlan
        it = _ghx.ExchangeItem()
        it.pattern = self.pc.handle
        it.local_index = self.pc.local_index(self.dds[di].domain_id())
        it.kind, it.field, it.align, it.tag_offset = 0, desc, align, 0
        plan = _ExchangePlan([it], [cs_item])  # owns the exchange: alive while it is read
        return _info(plan.h)


@pytest.fixture(scope="module")
def pattern10():
    return _Pattern(cs_cases.config(10))


# ---------------------------------------------------------------------------------------------
# B. widths and value kinds
# ---------------------------------------------------------------------------------------------
SCALARS = [("uint8", 1), ("uint8", 3), ("int16", 1), ("float16", 1), ("bfloat16", 1),
           ("complex64", 1), ("complex128", 1)]
VECTORS = [("int64", 3), ("float32", 3), ("int64", 1)]
ONE_FIELD = ([(d, nc, False, lay) for d, nc in SCALARS for lay in (X_FAST, Y_FAST)] +
             [(d, nc, True, lay) for d, nc in VECTORS for lay in (X_FAST, Y_FAST, Z_FAST)])


@pytest.mark.parametrize("dtype,nc,vector,layout", ONE_FIELD,
                         ids=[f"{d}x{nc}{'v' if v else ''}-{LAYOUT_ID[lay]}"
                              for d, nc, v, lay in ONE_FIELD])
def test_unpack_of_one_field_by_width_and_kind(pattern10, dtype, nc, vector, layout):
    """Element sizes 1, 2, 8 (opaque) and 16 as scalars, and vectors whose integer cells include
    0, the minimum, -1 and words with a zero or all-ones low half (tests/cs_cases.py). The
    x- and y-stride-1 cases must be planned as transformed records, whatever the type."""
    from ghex_amd.structured import cubed_sphere as CS
    import torch
    cfg = pattern10.cfg
    for di in DOMAINS:
        df = DomainField(cfg, di, dtype, nc, vector, special=vector)
        boxes = df.dom["boxes"]
        base, logical = to_device(df.initial(), layout, dtype)
        fd = CS.FieldDescriptor(pattern10.dds[di], logical, df.offsets, df.extents, nc, vector)
        assert fd.desc.elem_size == cs_cases.elem_size(dtype)
        if layout != Z_FAST:
            info = pattern10.info_of_one_field(di, fd.desc, fd.cs_item, fd.align)
            assert info["records"] > 0 and info["records"] == info["rotated"], info
        buf = buffer_to_device(df.buffer(boxes, layout), dtype)
        fd.unpack(buf, df.spaces(boxes))
        torch.cuda.synchronize()
        got, exp = from_device(base, layout, dtype), df.expected(boxes)
        assert np.array_equal(got, exp), (di, np.argwhere(got != exp)[:5])


def _one_rank(cfg, specs, **co_options):
    """All domains of `cfg` on one rank with one field per spec (dtype, nc, vector, layout) and
    domain, spec-major: (communication object, buffer infos, [(DomainField, base, layout)])."""
    from ghex_amd.structured import cubed_sphere as CS
    pat = _Pattern(cfg)
    bis, fields = [], []
    for dtype, nc, vector, layout in specs:
        for di, dd in enumerate(pat.dds):
            df = DomainField(cfg, di, dtype, nc, vector, special=vector)
            base, logical = to_device(df.initial(), layout, dtype)
            bis.append(pat.pc(CS.FieldDescriptor(dd, logical, df.offsets, df.extents, nc, vector)))
            fields.append((df, base, layout))
    return CS.make_communication_object(pat.ctx, **co_options), bis, fields


def _check(fields, what=None):
    for df, base, layout in fields:
        got, exp = from_device(base, layout, df.dtype), df.expected()
        assert np.array_equal(got, exp), (what, df.di, str(df.dtype), np.argwhere(got != exp)[:5])


MIXED = [("uint8", 3, False), ("int16", 1, False), ("float32", 3, True), ("int64", 3, True),
         ("complex128", 1, False)]


@pytest.mark.parametrize("layout", [X_FAST, Y_FAST], ids="xy")
def test_exchange_of_mixed_widths_in_several_launch_groups(layout):
    """Five fields of five element sizes per domain, 24 domains on one rank: 120 field slots, so
    the transformed plan runs as several launches with slot maps, its tile records differ in
    element size, and the buffers pad between fields (a 1-byte field of 3 components before a
    2-byte one, 8-byte before 16-byte)."""
    from ghex_amd import _ghx
    co, bis, fields = _one_rank(cs_cases.config(10), [s + (layout,) for s in MIXED])
    assert len(bis) == 120 > _ghx.MAX_SLOTS
    plan = co.plan(bis)
    info = _info(plan.h)
    assert info["records"] > 0 and info["records"] == info["rotated"]
    assert info["bytes"] == sum(sum(_record_elements(cs_cases.config(10), nc)) *
                                cs_cases.elem_size(d) for d, nc, _ in MIXED)
    co.exchange(bis).wait()
    _check(fields)


# ---------------------------------------------------------------------------------------------
# C. tiling and grid
# ---------------------------------------------------------------------------------------------
def _record_elements(cfg, nc):
    """Elements of every rotated receive space of every domain of cfg (one field of nc
    components each): the recorded intersections of the boxes whose image turns x into y."""
    out = []
    for dom in cfg["domains"]:
        for b in dom["boxes"]:
            if b["t"] == dom["tile"] or b["img"][2] != b["img"][0]:
                continue  # own tile, or a step in x moves x': a translation
            for x in b["x"]:
                out.append(math.prod(x[4 + k] - x[1 + k] + 1 for k in range(3)) * nc)
    return out


TILING = {70: [("float64", 1, False, X_FAST)], 10: [("float32", 3, True, X_FAST)]}


@pytest.mark.parametrize("edge", [70, 10])
def test_tile_sizes_other_than_the_default(edge):
    """x_tile_elems 32, 48 and 4096 next to the default 256, each with a communication object of
    its own so that the plan is cut under the knob (ghx_cs_unpack's cached plan would keep the
    first tiling). c = 70: 1,050-element edge boxes, one tile of five loop trips at 4096 and many
    evened tiles at 32. The tile counts prove the knob took effect."""
    cfg, specs = cs_cases.config(edge), TILING[edge]
    elements = _record_elements(cfg, specs[0][1])
    seen = {}
    try:
        for T in (256, 32, 48, 4096):
            _tune(x_tile_elems=T)
            co, bis, fields = _one_rank(cfg, specs)
            seen[T] = info = _info(co.plan(bis).h)
            assert info["tiles"] >= sum(-(-e // T) for e in elements), (T, info)
            assert info["records"] == len(elements) == info["rotated"]
            assert info["bytes"] == sum(elements) * cs_cases.elem_size(specs[0][0])
            co.exchange(bis).wait()
            _check(fields, f"x_tile_elems={T}")
    finally:
        _reset()
    assert seen[32]["tiles"] > seen[48]["tiles"] > seen[256]["tiles"] >= seen[4096]["tiles"]
    if max(elements) > 256:
        assert seen[256]["tiles"] > seen[4096]["tiles"]
        assert seen[4096]["tiles"] == len(elements)  # 1,050 elements: one tile, several trips
    else:
        # c = 10: no record has more than 256 elements, one tile each from 256 on
        assert seen[256]["tiles"] == seen[4096]["tiles"] == len(elements)
    assert edge != 70 or max(elements) > 1024


@pytest.mark.parametrize("knobs", [{"grid_cap": 1}, {"grid_cap": 7},
                                   {"grid_cap": 1, "x_tile_elems": 32},
                                   {"grid_cap": 7, "x_tile_elems": 32}],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_fewer_workgroups_than_tiles(knobs):
    """grid_cap: k_unpack_x walks its tiles grid-stride (1: one workgroup takes them all)."""
    specs = [("float64", 1, False, X_FAST), ("float32", 3, True, X_FAST)]
    try:
        _tune(**knobs)
        co, bis, fields = _one_rank(cs_cases.config(10), specs)
        info = _info(co.plan(bis).h)
        assert info["tiles"] >= 96  # 48 records per field: many more tiles than workgroups
        co.exchange(bis).wait()
        _check(fields)
    finally:
        _reset()


# ---------------------------------------------------------------------------------------------
# D, E. raw pointers: the byte-wise path and elements that are no power of two
# ---------------------------------------------------------------------------------------------
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


def _boxes(spaces, lo, hi):
    from ghex_amd import _ghx
    arr = (_ghx.Box * len(spaces))()
    for i, sp in enumerate(spaces):
        for d in range(3):
            arr[i].first[d], arr[i].last[d] = sp[lo][d], sp[hi][d]
    return arr


BUF_GUARD = 64


def _unpack_in_arena(df, layout, field_shift=0, buf_shift=0, pad=None):
    """ghx_cs_unpack of all of df's boxes with raw pointers: the field in an arena at GUARD +
    field_shift with `pad` pitch bytes, the buffer at an allocation + buf_shift. Compares the
    whole arena and the whole buffer allocation. Returns (field descriptor, item)."""
    import torch
    from ghex_amd import _ghx
    elem = cs_cases.elem_size(df.dtype)
    af = ArenaField(df, dense_strides(df.shape, layout, elem, pad), field_shift)
    assert af.layout() == layout
    boxes = df.dom["boxes"]
    spaces = df.spaces(boxes)
    dev = torch.from_numpy(af.arena(df.initial())).cuda()
    msg = cs_cases.as_bytes(df.buffer(boxes, layout), df.dtype).ravel()
    host_buf = np.full(BUF_GUARD + buf_shift + msg.size + BUF_GUARD, 0x5A, dtype=np.uint8)
    host_buf[BUF_GUARD + buf_shift:BUF_GUARD + buf_shift + msg.size] = msg
    buf = torch.from_numpy(host_buf).cuda()
    assert dev.data_ptr() % 256 == 0 and buf.data_ptr() % 256 == 0
    fd, cs = _field_desc(af), _cs_item(df)
    _ghx.call("ghx_cs_unpack", ctypes.byref(fd), ctypes.byref(cs), dev.data_ptr() + af.base,
              buf.data_ptr() + BUF_GUARD + buf_shift, _boxes(spaces, 0, 1), _boxes(spaces, 2, 3),
              _ghx.i32_array([sp[4] for sp in spaces]), len(spaces),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got, exp = dev.cpu().numpy(), af.arena(df.expected(boxes))
    assert np.array_equal(got, exp), (df.di, layout, np.flatnonzero(got != exp)[:8] - af.base)
    assert np.array_equal(buf.cpu().numpy(), host_buf)
    return fd, cs


BY_SIZE = {2: ("int16", 1), 4: ("float32", 2), 8: ("float64", 2), 16: ("complex128", 1)}
ARENA_CASES = [(6, 0), (6, 1), (10, 0)]


def _misalignments(elem):
    half = elem // 2
    shifts = [1] if half == 1 else [1, half]
    return ([("buffer", s) for s in shifts] + [("field", s) for s in shifts] + [("pitch", half)])


@pytest.mark.parametrize("elem,what,by", [(e, w, b) for e in BY_SIZE for w, b in _misalignments(e)],
                         ids=lambda v: str(v))
def test_one_misaligned_side_takes_the_bytewise_path(elem, what, by):
    """The buffer pointer, the field pointer, or one stride alone is no multiple of the element
    size (the other two are): k_unpack_x must load and store byte by byte. Everything else in the
    arena — guards, pitch padding, the bytes around the shifted message — must stay."""
    dtype, nc = BY_SIZE[elem]
    for edge, di in ARENA_CASES:
        df = DomainField(cs_cases.config(edge), di, dtype, nc, False)
        for layout in (X_FAST, Y_FAST):
            order = cs_cases.layout_order(layout)
            kw = dict(buffer=dict(buf_shift=by), field=dict(field_shift=by),
                      pitch=dict(pad={order[-2]: by}))[what]  # pitch: the second-fastest dim
            fd, _ = _unpack_in_arena(df, layout, **kw)
            odd = [s for s in fd.byte_strides if s % elem]
            assert bool(odd) == (what == "pitch")


@pytest.mark.parametrize("layout", [X_FAST, Y_FAST, Z_FAST], ids="xyz")
@pytest.mark.parametrize("dtype", ["float32", "int64"])
def test_negation_on_the_bytewise_path(dtype, layout):
    """3-vectors with the field pointer one byte off: the sign-bit flip and the two's-complement
    negation between byte-wise loads and stores."""
    for edge, di in ARENA_CASES:
        df = DomainField(cs_cases.config(edge), di, dtype, 3, True, special=True)
        _unpack_in_arena(df, layout, field_shift=1)


@pytest.mark.parametrize("layout", [X_FAST, Y_FAST], ids="xy")
def test_twelve_byte_elements_ride_the_ordinary_launch(pattern10, layout):
    """A 12-byte scalar whose stride-1 axis the rotation moves is no case for k_unpack_x: it is
    planned as element-sized rows of an ordinary segment with up to four outer dims and signed
    strides. The field pointer is 4-byte aligned only."""
    for di in DOMAINS:
        df = DomainField(pattern10.cfg, di, "raw12", 1, False)
        fd, cs = _unpack_in_arena(df, layout, field_shift=4)
        info = pattern10.info_of_one_field(di, fd, cs, 4)
        assert info["records"] == 0 and info["tiles"] == 0 and info["rotated"] > 0, info
