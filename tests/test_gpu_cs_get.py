"""GPU tests of the fused cubed-sphere adjoint (k_accum_get_x behind
ghx_cs_exchange_adjoint_self_accumulate) through
make_communication_object(adjoint_rotated=True, fuse_adjoint_rotated=True).

Every expectation is expanded cell by cell from the recorded reference fixture
(tests/golden/cubed_sphere_case.json through tests/cs_cases.py and tests/cs_adjoint_cases.py) or is
the unfused path's result on equal inputs, and every comparison is np.array_equal on bit patterns:
whole local arrays with their halos, corner squares and padding, or whole byte arenas with their
guards."""
import ctypes

import numpy as np
import pytest

from tests import cs_adjoint_cases as adj
from tests import cs_cases
from tests.cs_cases import ArenaField, DomainField, dense_strides, from_device, to_device
from tests.gpu_util import FakeContext, emulated_exchange

pytestmark = pytest.mark.gpu

X_FAST, Y_FAST, Z_FAST, K_FAST = (3, 2, 1, 0), (2, 3, 1, 0), (1, 2, 3, 0), (0, 1, 2, 3)
FLOATS = [("float64", 1, False, X_FAST), ("float32", 3, True, X_FAST)]
INTS = [("int32", 2, True, X_FAST), ("int64", 3, True, X_FAST)]
OTHER_LAYOUTS = [("float32", 3, True, Y_FAST), ("float64", 1, False, Z_FAST), ("float64", 2, True, K_FAST),
                 ("float32", 3, True, Z_FAST)]
ORDER = [("float32", 1, False, X_FAST), ("float32", 3, True, Y_FAST)]
RANK_OF = {"one": lambda d: 0, "two": lambda d: d["tile"] // 3, "six": lambda d: d["tile"]}
FUSED = dict(adjoint_rotated=True, fuse_adjoint_rotated=True)
PLAIN = dict(adjoint_rotated=True)


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


def _load(base, layout, values):
    import torch
    order = cs_cases.layout_order(layout)
    base.copy_(torch.from_numpy(np.ascontiguousarray(values.transpose(order))))


class _World:
    """A configuration on one rank, on two emulated ranks (tiles 0-2 and 3-5) or on six (one tile
    each): one field per spec (dtype, nc, vector, layout) and domain, one communication object per
    rank made with `options`, and the state of every field as values."""

    def __init__(self, cfg, specs, placement, values_of, options):
        from ghex_amd.structured import cubed_sphere as CS
        self.cfg, self.specs = cfg, specs
        rank_of = RANK_OF[placement]
        self.world = 1 + max(rank_of(d) for d in cfg["domains"])
        cube = CS.Cube(cfg["edge_size"], cfg["levels"])
        table = [[(cube.edge_size, cube.levels, d["tile"], *d["x"], *d["y"]) for d in cfg["domains"] if rank_of(d) == r]
                 for r in range(self.world)]
        self.cos, self.bis, self.f = [], [], {}
        for r in range(self.world):
            ctx = FakeContext(r, self.world, table)
            mine = [i for i, d in enumerate(cfg["domains"]) if rank_of(d) == r]
            dds = {i: CS.DomainDescriptor(cube, cfg["domains"][i]["tile"], *cfg["domains"][i]["x"],
                                          *cfg["domains"][i]["y"]) for i in mine}
            pc = CS.make_pattern(ctx, CS.HaloGenerator(cfg["halos"]), list(dds.values()))
            bis = []
            for si, (dtype, nc, vector, layout) in enumerate(specs):
                for di in mine:
                    df = DomainField(cfg, di, dtype, nc, vector)
                    vals = values_of(df, si)
                    base, logical = to_device(adj.bits_of(vals), layout, dtype)
                    bis.append(pc(CS.FieldDescriptor(dds[di], logical, df.offsets, df.extents, nc, vector)))
                    self.f[(si, di)] = [df, base, layout, vals]
            self.cos.append(CS.make_communication_object(ctx, **options))
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

    def forms(self):
        """ghx_cs_exchange_adjoint_self_info's form of every rank's plan."""
        from ghex_amd import _ghx
        out = []
        for co, bis in zip(self.cos, self.bis):
            f = ctypes.c_int32(-1)
            _ghx.call("ghx_cs_exchange_adjoint_self_info", co.plan(bis).h, ctypes.byref(f), None, None, None, None)
            out.append(f.value)
        return out

    def state(self, si):
        out = []
        for di in range(self.n_dom):
            df, base, layout, vals = self.f[(si, di)]
            out.append(from_device(base, layout, df.dtype).view(vals.dtype))
        return out

    def bits(self):
        return [adj.bits_of(a).copy() for si in range(len(self.specs)) for a in self.state(si)]

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


def _small(df, si):
    return adj.small_values(df, si)


# ---------------------------------------------------------------------------------------------
# 1. whole fields against the NumPy adjoint
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_halos", [True, False], ids=["zero", "keep"])
@pytest.mark.parametrize("edge", [6, 70, 8, 10])
def test_fused_adjoint_of_a_cube_on_one_rank(edge, zero_halos):
    """Every cell of every field: owned cells with their sums, receive boxes zeroed or kept, the
    cube-corner squares and the padding untouched. c = 10 is the 24-domain cube (48 fields, 168
    buffers) that the unfused adjoint refuses for its slots."""
    w = _World(cs_cases.config(edge), FLOATS, "one", _small, FUSED)
    w.adjoint(zero_halos)
    assert w.forms() == [1]
    w.check_adjoint(zero_halos)


def test_fused_adjoint_of_integer_vectors_wraps():
    w = _World(cs_cases.config(6), INTS, "one", lambda df, si: adj.wrapping_values(df, si), FUSED)
    w.adjoint(True)
    w.check_adjoint(True)


def test_fused_adjoint_with_other_layouts():
    """y-, z- and k-fastest fields in one exchange: element rows under the y-fastest transforms,
    vector rows along z, and the k-fastest f64 x 2 vector whose components differ in sign."""
    w = _World(cs_cases.config(6), OTHER_LAYOUTS, "one", _small, FUSED)
    w.adjoint(True)
    assert w.forms() == [1]
    w.check_adjoint(True)
    w.load(lambda df, si: adj.small_values(df, si + 3))
    w.adjoint(False)
    w.check_adjoint(False)


# ---------------------------------------------------------------------------------------------
# 2. bits against the unfused path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge,placement", [(6, "one"), (8, "six")], ids=["c6-1rank", "c8-6ranks"])
def test_order_sensitive_bits_equal_the_unfused_path(edge, placement):
    """f32 values whose sum depends on its order: the fused and the unfused object on equal inputs,
    under the default knobs, grid_cap 1 / 3 and tile_bytes 1024 / 4096, with fresh objects each (the
    plans are cut under the knobs). c = 8 over six ranks runs mixed forms on every rank."""
    cfg = cs_cases.config(edge)
    vals = lambda df, si: adj.order_sensitive_values(df, si)  # noqa: E731
    first = None
    try:
        for knobs in ({}, {"grid_cap": 1}, {"grid_cap": 3}, {"tile_bytes": 1024}, {"tile_bytes": 4096}):
            _reset()
            _tune(**knobs)
            fused = _World(cfg, ORDER, placement, vals, FUSED)
            plain = _World(cfg, ORDER, placement, vals, PLAIN)
            fused.adjoint(True)
            plain.adjoint(True)
            assert fused.forms() == ([1] if placement == "one" else [2] * 6) and set(plain.forms()) == {0}
            got, want = fused.bits(), plain.bits()
            for a, b in zip(got, want):
                assert np.array_equal(a, b), knobs
            if first is None:
                first = got
                before = [adj.bits_of(v) for si in range(len(ORDER)) for v in fused.values(si)]
                assert any(not np.array_equal(g, v) for g, v in zip(got, before))
            for a, b in zip(first, got):
                assert np.array_equal(a, b), knobs
    finally:
        _reset()


def test_self_buffers_are_not_touched():
    """Form 1: every byte of the object's send and receive buffers keeps the sentinel."""
    import torch
    w = _World(cs_cases.config(6), FLOATS, "one", _small, FUSED)
    co, bis = w.cos[0], w.bis[0]
    plan = co._adjoint_plan(bis)
    send, recv = co.buffers(plan, bis[0].field.device)
    assert len(send) == len(recv) == 18
    for t in send + recv:
        t.fill_(cs_cases.SENTINEL_BYTE)
    torch.cuda.synchronize()
    w.adjoint(True)
    w.check_adjoint(True)
    for t in send + recv:
        assert bool((t == cs_cases.SENTINEL_BYTE).all())


# ---------------------------------------------------------------------------------------------
# 3. mixed forms against the NumPy adjoint
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_halos", [True, False], ids=["zero", "keep"])
@pytest.mark.parametrize("edge,placement", [(6, "two"), (10, "six")], ids=["c6-2ranks", "c10-6ranks"])
def test_mixed_forms_on_emulated_ranks(edge, placement, zero_halos):
    """Two ranks at c = 6: rotated self messages beside rotated peer messages. Six ranks at c = 10:
    four domains per rank, in-tile self messages, every cross-tile message a peer's."""
    w = _World(cs_cases.config(edge), FLOATS, placement, _small, FUSED)
    w.adjoint(zero_halos)
    assert set(w.forms()) == {2}
    w.check_adjoint(zero_halos)


# ---------------------------------------------------------------------------------------------
# 4. misaligned field pointers, whole arenas
# ---------------------------------------------------------------------------------------------
def _arena_run(specs, shifts, zero_halos=True):
    """The c = 6 cube on one rank through the C calls, every field in a byte arena of its own at
    GUARD + shift. Returns (return code of the accumulate, arenas after, arenas before, arenas
    expected from the NumPy adjoint)."""
    import torch
    from ghex_amd import _ghx
    from tests import cs_get_cases as G
    cfg = cs_cases.config(6)
    host = [(layout, cs_cases.elem_size(dt), nc, int(vec), {"f": 1, "i": 2}[np.dtype(dt).kind])
            for dt, nc, vec, layout in specs]
    ex = G.Exchange(_ghx, cfg, host)
    try:
        assert ex.create() == 0, ex.error()
        n_dom = len(cfg["domains"])
        afs, devs, before, want = [], [], [], []
        for si, (dt, nc, vec, layout) in enumerate(specs):
            dfs = [DomainField(cfg, di, dt, nc, vec) for di in range(n_dom)]
            vals = [adj.small_values(df, si) for df in dfs]
            exp = adj.numpy_adjoint(cfg, dfs, vals, zero_halos)
            for di, df in enumerate(dfs):
                assert ex.domains[si * n_dom + di] == di
                af = ArenaField(df, dense_strides(df.shape, layout, cs_cases.elem_size(dt)), shifts[si])
                afs.append(af)
                before.append(af.arena(adj.bits_of(vals[di])))
                want.append(af.arena(adj.bits_of(exp[di])))
                devs.append(torch.from_numpy(before[-1]).cuda())
                assert devs[-1].data_ptr() % 256 == 0
        fptrs = _ghx.ptr_array([d.data_ptr() + af.base for d, af in zip(devs, afs)])
        n = ex.buffers(0)
        none = _ghx.ptr_array([0] * n)
        s = torch.cuda.current_stream().cuda_stream
        _ghx.call("ghx_cs_exchange_adjoint_self_pack", ex.h, fptrs, len(devs), none, n, s)
        rc = _ghx.lib().ghx_cs_exchange_adjoint_self_accumulate(ex.h, fptrs, len(devs), none, n,
                                                                1 if zero_halos else 0, s)
        err = ex.error()
        torch.cuda.synchronize()
        return rc, err, [d.cpu().numpy() for d in devs], before, want
    finally:
        ex.close()


@pytest.mark.parametrize("zero_halos", [True, False], ids=["zero", "keep"])
def test_field_bases_shifted_by_one_element(zero_halos):
    """An f64 x 2 vector z-fastest (16-byte vectors planned) at 8 B past a 256-byte boundary and an
    f32 3-vector x-fastest at 4 B: the launch narrows its vectors; whole arenas with their guards."""
    specs = [("float64", 2, True, Z_FAST), ("float32", 3, True, X_FAST), ("float32", 3, True, Z_FAST)]
    rc, err, got, before, want = _arena_run(specs, [8, 4, 4], zero_halos)
    assert rc == 0, err
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (k, np.flatnonzero(g != w)[:8])
    assert any(not np.array_equal(g, b) for g, b in zip(got, before))


def test_f64_fields_shifted_by_four_bytes_are_refused_untouched():
    """4 B under f64 fields is no multiple of the element: the accumulate refuses the pointers, as
    the unfused accumulate does, before anything is launched; every arena keeps every byte."""
    rc, err, got, before, _ = _arena_run([("float64", 1, False, X_FAST)], [4])
    assert rc == -1 and "a field pointer is not aligned to its element" in err
    for g, b in zip(got, before):
        assert np.array_equal(g, b)


# ---------------------------------------------------------------------------------------------
# 5. transpose identity, graph replay, the Python refusal
# ---------------------------------------------------------------------------------------------
def test_transpose_identity_with_the_fused_forward_exchange():
    """<E x, y> == <x, E^T y> exactly for integer-valued x and y over whole fields, E the
    fuse_rotated=True forward exchange of the same object."""
    specs = [("float64", 3, True, X_FAST)]
    w = _World(cs_cases.config(6), specs, "one", lambda df, si: adj.small_values(df, 1),
               dict(FUSED, fuse_rotated=True))
    assert w.cos[0].cs_self(w.cos[0].plan(w.bis[0]))
    y = [adj.small_values(df, 2) for df in w.dfs(0)]
    x = w.values(0)
    w.forward()
    lhs = sum(float((ex * yy).sum()) for ex, yy in zip(w.state(0), y))
    w.load(lambda df, si: adj.small_values(df, 2))
    w.adjoint(True)
    assert w.forms() == [1]
    rhs = sum(float((xx * ey).sum()) for xx, ey in zip(x, w.state(0)))
    assert lhs == rhs and abs(lhs) < 2.0 ** 53
    assert any(not np.array_equal(a, b) for a, b in zip(w.state(0), y))


def test_fused_adjoint_replayed_from_a_capture():
    import torch
    w = _World(cs_cases.config(6), FLOATS, "one", _small, FUSED)
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


def test_the_keyword_needs_adjoint_rotated():
    from ghex_amd.structured import cubed_sphere as CS
    ctx = FakeContext(0, 1, [None])
    with pytest.raises(ValueError, match="needs adjoint_rotated=True"):
        CS.make_communication_object(ctx, fuse_adjoint_rotated=True)
    # without the keyword the routing is the unfused one
    w = _World(cs_cases.config(6), FLOATS, "one", _small, PLAIN)
    assert w.cos[0]._adjoint_plan(w.bis[0])._adjoint_prefix == "ghx_cs_exchange_adjoint_"
    f = _World(cs_cases.config(6), FLOATS, "one", _small, FUSED)
    assert f.cos[0]._adjoint_plan(f.bis[0])._adjoint_prefix == "ghx_cs_exchange_adjoint_self_"
