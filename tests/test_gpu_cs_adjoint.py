"""GPU tests of the cubed-sphere adjoint exchange: the rotating reverse pack (k_pack_x behind
ghx_cs_pack_rotated and ghx_cs_exchange_adjoint_pack) and the whole adjoint (reverse pack, transport
with the roles swapped, k_accum_s) through CommunicationObject(adjoint_rotated=True).

Every expectation is expanded cell by cell from the recorded reference fixture
(tests/golden/cubed_sphere_case.json through tests/cs_cases.py and tests/cs_adjoint_cases.py) and
compared with np.array_equal: whole buffers with their guards, whole fields with their halos, corner
squares and padding, or whole byte arenas. The sums are taken over values for which they are exact
in any order (tests/cs_adjoint_cases.py)."""
import ctypes

import numpy as np
import pytest

from tests import cs_adjoint_cases as adj
from tests import cs_cases
from tests.cs_cases import ArenaField, DomainField, dense_strides, from_device, to_device
from tests.gpu_util import FakeContext, emulated_exchange

pytestmark = pytest.mark.gpu

X_FAST, Y_FAST, Z_FAST, K_FAST = (3, 2, 1, 0), (2, 3, 1, 0), (1, 2, 3, 0), (0, 1, 2, 3)
LAYOUT_ID = {X_FAST: "x", Y_FAST: "y", Z_FAST: "z", K_FAST: "k"}
# every distinct transform: tile 0's domains 0 (-x, -y) and 3 (+x, +y), likewise tile 1's 4 and 7
DOMAINS = (0, 3, 4, 7)
GUARD = 64


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


class _Pattern:
    """The domains of a configuration that rank `rank` of `world` holds (one tile per rank when
    world is 6, everything when it is 1), with their indices in the configuration."""

    def __init__(self, cfg, rank=0, world=1):
        from ghex_amd.structured import cubed_sphere as CS
        self.cfg = cfg
        cube = CS.Cube(cfg["edge_size"], cfg["levels"])
        rank_of = (lambda d: 0) if world == 1 else (lambda d: d["tile"])
        table = [[(cube.edge_size, cube.levels, d["tile"], *d["x"], *d["y"])
                  for d in cfg["domains"] if rank_of(d) == r] for r in range(world)]
        self.ctx = FakeContext(rank, world, table)
        self.mine = [i for i, d in enumerate(cfg["domains"]) if rank_of(d) == rank]
        self.dds = {i: CS.DomainDescriptor(cube, cfg["domains"][i]["tile"], *cfg["domains"][i]["x"],
                                           *cfg["domains"][i]["y"]) for i in self.mine}
        self.pc = CS.make_pattern(self.ctx, CS.HaloGenerator(cfg["halos"]), list(self.dds.values()))


@pytest.fixture(scope="module")
def pattern10():
    return _Pattern(cs_cases.config(10))


# ---------------------------------------------------------------------------------------------
# 1. ghx_cs_pack_rotated on one field
# ---------------------------------------------------------------------------------------------
ONE_FIELD = [("float64", 1, False), ("float32", 3, True), ("int32", 2, True), ("int64", 3, True),
             ("int16", 1, False), ("complex128", 1, False)]


def _expected_bytes(df, bits, boxes, layout):
    return cs_cases.as_bytes(adj.rotated_buffer(df, bits, boxes, layout), df.dtype).ravel()


def _pack_rotated(pat, di, df, bits, layout, boxes=None):
    """pack_rotated of df's boxes from the device copy of `bits` into a guarded buffer; checks the
    whole buffer allocation and that the field is unchanged. Returns the message on the device."""
    import torch
    from ghex_amd.structured import cubed_sphere as CS
    boxes = df.dom["boxes"] if boxes is None else boxes
    base, logical = to_device(bits, layout, df.dtype)
    fd = CS.FieldDescriptor(pat.dds[di], logical, df.offsets, df.extents, df.nc, df.vector)
    want = _expected_bytes(df, bits, boxes, layout)
    buf = torch.full((GUARD + want.size + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    fd.pack_rotated(buf[GUARD:], df.spaces(boxes))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == 0x5A).all() and (got[GUARD + want.size:] == 0x5A).all()
    msg = got[GUARD:GUARD + want.size]
    assert np.array_equal(msg, want), (df.di, layout, np.flatnonzero(msg != want)[:8])
    assert np.array_equal(from_device(base, layout, df.dtype), bits)
    return fd, buf[GUARD:GUARD + want.size]


@pytest.mark.parametrize("layout", [X_FAST, Y_FAST, Z_FAST, K_FAST], ids="xyzk")
@pytest.mark.parametrize("dtype,nc,vector", ONE_FIELD, ids=[f"{d}x{n}{'v' if v else ''}" for d, n, v in ONE_FIELD])
def test_pack_rotated_of_one_field(pattern10, dtype, nc, vector, layout):
    """Every width (2, 4, 8, 16 B), both negations with their special bit patterns (NaN payloads,
    -0.0, the integer minimum, words with a zero low half), every layout, every transform."""
    for di in DOMAINS:
        df = DomainField(pattern10.cfg, di, dtype, nc, vector, special=vector)
        _pack_rotated(pattern10, di, df, adj.full_bits(df), layout)


@pytest.mark.parametrize("layout", [X_FAST, Y_FAST], ids="xy")
@pytest.mark.parametrize("dtype,nc,vector", [("float32", 3, True), ("int64", 3, True), ("int16", 1, False)],
                         ids=["float32x3v", "int64x3v", "int16"])
def test_unpack_of_pack_rotated_restores_the_receive_boxes(pattern10, dtype, nc, vector, layout):
    import torch
    for di in DOMAINS:
        df = DomainField(pattern10.cfg, di, dtype, nc, vector, special=vector)
        bits = adj.full_bits(df)
        fd, msg = _pack_rotated(pattern10, di, df, bits, layout)
        blank = np.full_like(bits, df.sentinel)
        base, logical = to_device(blank, layout, dtype)
        from ghex_amd.structured import cubed_sphere as CS
        fd2 = CS.FieldDescriptor(pattern10.dds[di], logical, df.offsets, df.extents, nc, vector)
        fd2.unpack(msg, df.spaces(df.dom["boxes"]))
        torch.cuda.synchronize()
        want = blank.copy()
        for b in df.dom["boxes"]:
            sl = adj._local_slice(df, b)
            want[sl] = bits[sl]
        assert np.array_equal(from_device(base, layout, dtype), want), di


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


def _pack_in_arena(df, layout, field_shift=0, buf_shift=0, pad=None):
    """ghx_cs_pack_rotated of all of df's boxes with raw pointers: the field in an arena at GUARD +
    field_shift with `pad` pitch bytes, the buffer at an allocation + buf_shift. Compares the whole
    buffer allocation and the whole arena (unchanged: guards, padding and the field itself)."""
    import torch
    from ghex_amd import _ghx
    elem = cs_cases.elem_size(df.dtype)
    af = ArenaField(df, dense_strides(df.shape, layout, elem, pad), field_shift)
    assert af.layout() == layout
    boxes = df.dom["boxes"]
    spaces = df.spaces(boxes)
    bits = adj.full_bits(df)
    arena = af.arena(bits)
    dev = torch.from_numpy(arena).cuda()
    msg = _expected_bytes(df, bits, boxes, layout)
    want = np.full(GUARD + buf_shift + msg.size + GUARD, 0x5A, dtype=np.uint8)
    buf = torch.from_numpy(want.copy()).cuda()
    want[GUARD + buf_shift:GUARD + buf_shift + msg.size] = msg
    assert dev.data_ptr() % 256 == 0 and buf.data_ptr() % 256 == 0
    fd, cs = _field_desc(af), _cs_item(df)
    _ghx.call("ghx_cs_pack_rotated", ctypes.byref(fd), ctypes.byref(cs), dev.data_ptr() + af.base,
              buf.data_ptr() + GUARD + buf_shift, _boxes(spaces, 0, 1), _boxes(spaces, 2, 3),
              _ghx.i32_array([sp[4] for sp in spaces]), len(spaces),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got, want), (df.di, layout, np.flatnonzero(got != want)[:8] - GUARD - buf_shift)
    assert np.array_equal(dev.cpu().numpy(), arena)


ARENA_CASES = [(6, 0), (6, 1), (10, 0)]
ARENA_TYPES = [("float64", 2, False), ("float32", 3, True), ("int64", 3, True), ("complex128", 1, False)]


@pytest.mark.parametrize("what,by", [("buffer", 1), ("buffer", 2), ("buffer", 4), ("field", 1),
                                     ("field", 2), ("field", 4), ("pitch", 2), ("none", 0)],
                         ids=lambda v: str(v))
def test_pack_rotated_in_an_arena_with_one_side_shifted(what, by):
    """Guard bands, and the field pointer, the buffer pointer or a pitch alone shifted by 1, 2 or
    4 B: whatever is then no multiple of the element size takes the byte-wide path."""
    for dtype, nc, vector in ARENA_TYPES:
        for edge, di in ARENA_CASES:
            df = DomainField(cs_cases.config(edge), di, dtype, nc, vector, special=vector)
            for layout in (X_FAST, Y_FAST):
                order = cs_cases.layout_order(layout)
                kw = dict(buffer=dict(buf_shift=by), field=dict(field_shift=by),
                          pitch=dict(pad={order[-2]: by}), none={})[what]
                _pack_in_arena(df, layout, **kw)


def test_pack_rotated_of_long_rows_in_several_tiles_and_few_workgroups():
    """c = 70: edge boxes of 8,400 B (1,050 fp64 elements, rows longer than a wave) over several
    tiles at x_tile_elems 64 and the default, with grid_cap 1, 3 and the default. One domain per
    combination, so that each plan is cut under its knobs (the call's plan is cached)."""
    pat = _Pattern(cs_cases.config(70))
    combos = [(t, g) for t in (64, 0) for g in (1, 3, 0)]
    try:
        for di, (t, g) in enumerate(combos):
            _reset()
            _tune(**({"x_tile_elems": t} if t else {}), **({"grid_cap": g} if g else {}))
            df = DomainField(pat.cfg, di, "float64", 1, False)
            assert max((b["l"][3] - b["l"][0] + 1) * (b["l"][4] - b["l"][1] + 1) for b in df.dom["boxes"]) \
                * pat.cfg["levels"] == 1050
            _pack_rotated(pat, di, df, adj.full_bits(df), X_FAST)
            dv = DomainField(pat.cfg, di, "float32", 3, True)
            _pack_rotated(pat, di, dv, adj.full_bits(dv), Y_FAST)
    finally:
        _reset()


# ---------------------------------------------------------------------------------------------
# 2. the adjoint of whole configurations
# ---------------------------------------------------------------------------------------------
def _load(base, layout, values):
    import torch
    order = cs_cases.layout_order(layout)
    base.copy_(torch.from_numpy(np.ascontiguousarray(values.transpose(order))))


class _World:
    """A configuration on one rank or on six emulated ranks: one field per spec (dtype, nc, vector,
    layout) and domain, the communication objects made with adjoint_rotated=True, and the state
    of every field as values."""

    def __init__(self, cfg, specs, world, values_of):
        from ghex_amd.structured import cubed_sphere as CS
        self.cfg, self.specs, self.world = cfg, specs, world
        self.cos, self.bis, self.f = [], [], {}
        for r in range(world):
            pat = _Pattern(cfg, r, world)
            bis = []
            for si, (dtype, nc, vector, layout) in enumerate(specs):
                for di in pat.mine:
                    df = DomainField(cfg, di, dtype, nc, vector)
                    vals = values_of(df, si)
                    base, logical = to_device(adj.bits_of(vals), layout, dtype)
                    bis.append(pat.pc(CS.FieldDescriptor(pat.dds[di], logical, df.offsets, df.extents,
                                                         nc, vector)))
                    self.f[(si, di)] = [df, base, layout, vals]
            self.cos.append(CS.make_communication_object(pat.ctx, adjoint_rotated=True))
            self.bis.append(bis)
        self.n_dom = len(cfg["domains"])

    def load(self, values_of):
        import torch
        for (si, di), f in self.f.items():
            f[3] = values_of(f[0], si)
            _load(f[1], f[2], f[3])
        torch.cuda.synchronize()

    def adjoint(self, zero_halos=True):
        import torch
        if self.world == 1:
            self.cos[0].adjoint_exchange(self.bis[0], zero_halos=zero_halos).wait()
        else:
            from tests.test_gpu_uaccum import emulated_adjoint
            assert emulated_adjoint(self.cos, self.bis, zero_halos=zero_halos) > 0
        torch.cuda.synchronize()

    def forward(self):
        import torch
        if self.world == 1:
            self.cos[0].exchange(self.bis[0]).wait()
        else:
            emulated_exchange(self.cos, self.bis)
        torch.cuda.synchronize()

    def state(self, si):
        out = []
        for di in range(self.n_dom):
            df, base, layout, vals = self.f[(si, di)]
            out.append(from_device(base, layout, df.dtype).view(vals.dtype))
        return out

    def dfs(self, si):
        return [self.f[(si, di)][0] for di in range(self.n_dom)]

    def values(self, si):
        return [self.f[(si, di)][3] for di in range(self.n_dom)]

    def check_adjoint(self, zero_halos, what=None):
        for si in range(len(self.specs)):
            want = adj.numpy_adjoint(self.cfg, self.dfs(si), self.values(si), zero_halos)
            for di, (g, w) in enumerate(zip(self.state(si), want)):
                assert np.array_equal(adj.bits_of(g), adj.bits_of(w)), \
                    (what, si, di, np.argwhere(adj.bits_of(g) != adj.bits_of(w))[:5])


FLOATS = [("float64", 1, False, X_FAST), ("float32", 3, True, X_FAST)]
INTS = [("int32", 2, True, X_FAST), ("int64", 3, True, Y_FAST)]
WORLDS = [(6, 1), (70, 1), (10, 6), (8, 6)]


def _small(df, si):
    return adj.small_values(df, si)


@pytest.mark.parametrize("zero_halos", [True, False], ids=["zero", "keep"])
@pytest.mark.parametrize("edge,world", WORLDS, ids=[f"c{e}-{w}rank" for e, w in WORLDS])
def test_adjoint_of_a_scalar_and_a_vector_field(edge, world, zero_halos):
    """Every cell of every field against the NumPy adjoint: owned cells with their sums, receive
    boxes zeroed or kept, the cube-corner squares and the padding untouched."""
    w = _World(cs_cases.config(edge), FLOATS, world, _small)
    w.adjoint(zero_halos)
    w.check_adjoint(zero_halos)


@pytest.mark.parametrize("edge,world", [(6, 1), (10, 6)], ids=["c6-1rank", "c10-6rank"])
def test_adjoint_of_integer_vectors_wraps(edge, world):
    w = _World(cs_cases.config(edge), INTS, world, lambda df, si: adj.wrapping_values(df, si))
    w.adjoint(True)
    w.check_adjoint(True)


def test_adjoint_with_other_layouts_on_one_rank():
    """y-, z- and k-fastest fields in one exchange: the z- and k-fastest spaces ride the ordinary
    reverse pack with signed strides, the y-fastest ones k_pack_x."""
    specs = [("float32", 3, True, Y_FAST), ("float64", 1, False, Z_FAST), ("float64", 2, True, K_FAST)]
    w = _World(cs_cases.config(6), specs, 1, _small)
    w.adjoint(True)
    w.check_adjoint(True)


# ---------------------------------------------------------------------------------------------
# 3. transpose identity against the shipped forward path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge,world", [(6, 1), (10, 6)], ids=["c6-1rank", "c10-6rank"])
def test_transpose_identity_with_the_forward_exchange(edge, world):
    """<E x, y> == <x, E^T y> exactly for integer-valued x and y over whole fields (halos, corner
    squares and padding included: E is the identity there), E = exchange() of the same objects."""
    specs = [("float64", 3, True, X_FAST)]
    w = _World(cs_cases.config(edge), specs, world, lambda df, si: adj.small_values(df, 1))
    y = [adj.small_values(df, 2) for df in w.dfs(0)]
    x = w.values(0)
    w.forward()
    lhs = sum(float((ex * yy).sum()) for ex, yy in zip(w.state(0), y))
    w.load(lambda df, si: adj.small_values(df, 2))
    w.adjoint(True)
    rhs = sum(float((xx * ey).sum()) for xx, ey in zip(x, w.state(0)))
    assert lhs == rhs and abs(lhs) < 2.0 ** 53
    # and E changed something: the identity is no tautology
    assert any(not np.array_equal(a, b) for a, b in zip(w.state(0), y))


# ---------------------------------------------------------------------------------------------
# 4. reproducibility
# ---------------------------------------------------------------------------------------------
def test_order_sensitive_sums_are_reproducible():
    """f32 values whose sum depends on its order: identical bits across two runs and across
    grid_cap 1 / 3 / default, two tile_bytes and two x_tile_elems (each with objects of its own, so
    that the plans are cut under the knobs)."""
    specs = [("float32", 1, False, X_FAST), ("float32", 3, True, Y_FAST)]
    vals = lambda df, si: adj.order_sensitive_values(df, si)  # noqa: E731
    first = None
    try:
        for knobs in ({}, {}, {"grid_cap": 1}, {"grid_cap": 3}, {"tile_bytes": 1024}, {"tile_bytes": 4096},
                      {"x_tile_elems": 32}, {"x_tile_elems": 4096}):
            _reset()
            _tune(**knobs)
            w = _World(cs_cases.config(6), specs, 1, vals)
            w.adjoint(True)
            got = [adj.bits_of(a).copy() for si in range(2) for a in w.state(si)]
            if first is None:
                first = got
                # the corners were summed: the result differs from the input on owned cells
                assert any(not np.array_equal(g, adj.bits_of(v))
                           for g, v in zip(got, w.values(0) + w.values(1)))
            for a, b in zip(first, got):
                assert np.array_equal(a, b), knobs
    finally:
        _reset()


# ---------------------------------------------------------------------------------------------
# 5. graph capture
# ---------------------------------------------------------------------------------------------
def test_adjoint_replayed_from_a_capture():
    import torch
    w = _World(cs_cases.config(6), FLOATS, 1, _small)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        w.cos[0].adjoint_exchange(w.bis[0]).wait()  # set-up and a warm run, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    w.check_adjoint(True, "warm")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        w.cos[0].adjoint_pack_only(w.bis[0], stream=torch.cuda.current_stream())
        w.cos[0].adjoint_accumulate_only(w.bis[0], zero_halos=True, stream=torch.cuda.current_stream())
    for salt in (3, 5):
        w.load(lambda df, si: adj.small_values(df, si + salt))
        g.replay()
        torch.cuda.synchronize()
        w.check_adjoint(True, salt)


# ---------------------------------------------------------------------------------------------
# 6. the Python refusals that need a device
# ---------------------------------------------------------------------------------------------
def test_python_refusals_with_device_fields(pattern10):
    import torch
    from ghex_amd import _ghx
    from ghex_amd.structured import cubed_sphere as CS
    cfg, di = pattern10.cfg, 0
    df = DomainField(cfg, di, "float32", 1, False)
    base, logical = to_device(df.initial(), X_FAST, "float32")
    fd = CS.FieldDescriptor(pattern10.dds[di], logical, df.offsets, df.extents, 1, False)
    assert fd.dtype_code() == _ghx.DT_F32
    for name, code in (("float64", _ghx.DT_F64), ("int32", _ghx.DT_I32), ("int64", _ghx.DT_I64)):
        d2 = DomainField(cfg, di, name, 1, False)
        _, lg = to_device(d2.initial(), X_FAST, name)
        assert CS.FieldDescriptor(pattern10.dds[di], lg, d2.offsets, d2.extents, 1, False).dtype_code() == code
    bi = pattern10.pc(fd)
    # without the option: refused as before, with or without adjoint_boxes
    with pytest.raises(ValueError, match="unstructured fields only"):
        CS.make_communication_object(pattern10.ctx).adjoint_exchange([bi])
    with pytest.raises(ValueError, match="cubed-sphere"):
        CS.make_communication_object(pattern10.ctx, adjoint_boxes=True).adjoint_exchange([bi])
    # a dtype the accumulate does not sum
    dh = DomainField(cfg, di, "float16", 1, False)
    _, lh = to_device(dh.initial(), X_FAST, "float16")
    fh = CS.FieldDescriptor(pattern10.dds[di], lh, dh.offsets, dh.extents, 1, False)
    co = CS.make_communication_object(pattern10.ctx, adjoint_rotated=True)
    with pytest.raises(TypeError, match=r"adjoint exchange: dtype torch.float16 is not supported"):
        co.adjoint_exchange([pattern10.pc(fh)])
    # the whole 24-domain cube on one rank: more buffers than the accumulate launch has slots
    bis = []
    for i in pattern10.mine:
        d = DomainField(cfg, i, "float32", 1, False)
        _, lg = to_device(d.initial(), X_FAST, "float32")
        bis.append(pattern10.pc(CS.FieldDescriptor(pattern10.dds[i], lg, d.offsets, d.extents, 1, False)))
    with pytest.raises(_ghx.GhxError, match="at most 64 field and 64 buffer slots"):
        co.adjoint_exchange(bis)
    assert torch.cuda.is_available()
