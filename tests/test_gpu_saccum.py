"""The adjoint halo exchange of structured fields on the device (ghx_saccum_create, k_accum_s,
CommunicationObject(adjoint_boxes=True).adjoint_exchange). Kernel cases through the ABI: every
field and every buffer in an arena of its own between 256-byte guard bands; after ONE execute
every byte of every arena is compared — owner cells with the NumPy definition
(tests/saccum_cases.py: adds in ascending (entry, box)), halo cells exact zero (or unchanged
without zero_halos), every other byte of the field, the buffers and the guards unchanged. Product
path: one rank, 2x2x1 domains as two emulated ranks, the transpose identity against exchange(),
adjoint twice then a forward exchange, graph replay and the refusals. Every comparison is
bit-exact.

Shapes (one periodic domain of N^3, halo H; the arrangement cuts every send box at every other
box's bounds, so sub-box rows are pieces of the 'H wide' box rows):
  N=6 H=2  sources 1 / 3 / 7, every row 16 B of f64 (one 16-B lane access)
  N=6 H=1  rows of one element beside rows of four
  N=5 H=3  f32: the 12-B box rows are cut into 8-B and 4-B sub-box rows, lists of 7 / 11 / 17 / 26;
           whole 12-B rows (three 4-B lanes) are test_rows_of_three_f32
  N=3 H=2, N=2 H=2  lists of 11 / 17 / 26: several batches of loads

Float inputs other than the order test's are drawn with magnitudes in [2^-20, 2^20] or are
integer-valued: no result is subnormal, inf or NaN (those are not part of the contract)."""
import numpy as np
import pytest

from tests import saccum_cases as SA
from tests.saccum_cases import Ent, cube
from tests.test_gpu_uput import GUARD, SENTINEL, Arena
from tests.test_saccum_host import GEOS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ghex_amd
    ghex_amd.native_library()


@pytest.fixture(autouse=True)
def _reset_knobs():
    yield
    from ghex_amd import _ghx
    _ghx.call("ghx_tune", b"reset", 0)


def _ctz(v, cap=4):
    return next(k for k in range(cap + 1) if k == cap or (v >> k) & 1)


def run_accum(contrib, zero, dtypes, fshift=0, bshift=0, zero_halos=True, seed=0, cell=None, messages=None):
    """One plan over the entries, one execute, every arena compared byte for byte. fshift / bshift:
    bytes by which field slot 0 / buffer slot 0 are moved off their 256-byte alignment (every other
    arena stays aligned). cell: the value of every field element; messages[e]: the elements of
    entry e's message (default: drawn). Returns (info, typed fields, planned and launched width
    log2 per sum sub-box)."""
    import torch
    from ghex_amd import _ghx
    rng = np.random.default_rng(7000 + seed)
    geo_of, code_of = {}, {}
    for en, c in zip(contrib, dtypes):
        geo_of[en.slot], code_of[en.slot] = en.geo, c
    for z in zero:
        geo_of.setdefault(z.slot, z.geo)
        code_of.setdefault(z.slot, SA.DT_I64 if z.geo.elem == 8 else SA.DT_I32)
    nf = 1 + max(geo_of)
    nb = 1 + max(en.bslot for en in contrib)
    fields = [None] * nf
    for k, g in geo_of.items():
        fields[k] = Arena(g.n_elems * g.elem, fshift if k == 0 else 0)
        v = SA.draw_values(rng, g.n_elems, code_of[k])
        if cell is not None:
            v[:] = cell
        raw = v.view(np.uint8)
        fields[k].host[fields[k].at:fields[k].at + raw.size] = raw
        fields[k].view.copy_(torch.from_numpy(fields[k].host))
    ends = [0] * nb
    for en in contrib:
        ends[en.bslot] = max(ends[en.bslot], en.boff + en.nbytes)
    bufs = [Arena(e, bshift if b == 0 else 0) if e else None for b, e in enumerate(ends)]
    for e, en in enumerate(contrib):
        n = en.nbytes // en.geo.elem
        m = (SA.draw_values(rng, n, dtypes[e]) if messages is None
             else np.asarray(messages[e], dtype=SA.NP[dtypes[e]]).reshape(n))
        a = bufs[en.bslot]
        a.host[a.at + en.boff:a.at + en.boff + en.nbytes] = m.view(np.uint8)
    for a in bufs:
        if a is not None:
            a.view.copy_(torch.from_numpy(a.host))
    h = SA.create(contrib, dtypes, zero)
    try:
        info = SA.info(h)
        subs, srcs = SA.boxes(h, contrib[0].geo.spatial), SA.sources(h)
        # the width each sum sub-box is launched at: the planner's, narrowed by the real pointers
        widths = []
        for s in subs:
            if not s.zero:
                w = min(s.wlog2, _ctz(fields[s.slot].ptr))
                for j in range(s.first_src, s.first_src + s.n_src):
                    w = min(w, _ctz(bufs[srcs[j][2]].ptr))
                widths.append((s.wlog2, w))
        fp = _ghx.ptr_array([a.ptr if a else 0 for a in fields])
        bp = _ghx.ptr_array([a.ptr if a else 0 for a in bufs])
        _ghx.call("ghx_saccum_execute", h, fp, nf, bp, nb, 1 if zero_halos else 0,
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        SA.destroy(h)
    typed = {k: fields[k].field()[:g.n_elems * g.elem].copy().view(SA.NP[code_of[k]]) for k, g in geo_of.items()}
    images = [a.field() if a else None for a in bufs]
    SA.definition(typed, images, contrib, dtypes, zero, zero_halos)
    for k, a in enumerate(fields):
        if a is None:
            continue
        want = a.host.copy()
        want[a.at:a.at + typed[k].nbytes] = typed[k].view(np.uint8)
        got = a.device_bytes()
        assert (got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all()
        np.testing.assert_array_equal(got, want)
        if cell is None and any(en.slot == k for en in contrib):
            assert (want != a.host).any()
    for a in bufs:
        if a is not None:
            np.testing.assert_array_equal(a.device_bytes(), a.host)   # read only, guards included
    for z in zero:                                                    # exact zeros, or untouched
        for f, l in z.boxes:
            cells = typed[z.slot][z.geo.box_index(f, l)]
            assert (cells.view(np.uint8) == 0).all() == bool(zero_halos)
    return info, typed, widths


def one_domain(N, H, code, layout=None, seed=0, geo=None, **kw):
    geo = geo or cube(N, H, SA.NP[code].itemsize, layout)
    contrib, zero = SA.one_domain_entries(geo, N, H)
    return run_accum(contrib, zero, [code], seed=seed, **kw)


# ---------------------------------------------------------------------------------------------
# kernel cases
# ---------------------------------------------------------------------------------------------
SHAPES = {(6, 2): 7, (6, 1): 7, (5, 3): 26, (3, 2): 26, (2, 2): 26}


@pytest.mark.parametrize("code", SA.DTYPES, ids=lambda c: SA.NAMES[c])
@pytest.mark.parametrize("N, H", list(SHAPES))
def test_every_shape_and_dtype(N, H, code):
    info, _, widths = one_domain(N, H, code, seed=N * 10 + H + code)
    assert info["max_sources"] == SHAPES[(N, H)] and info["n_zero_boxes"] == 26
    if (N, H) == (6, 2) and SA.NP[code].itemsize == 8:
        assert set(widths) == {(4, 4)}                   # 16-B rows, 16 B per lane
    if (N, H) == (6, 1) and SA.NP[code].itemsize == 8:
        assert (3, 3) in widths                          # one-element rows, 8 B per lane
    if (N, H) == (5, 3) and SA.NP[code].itemsize == 4:
        assert {w for _, w in widths} == {2}             # E = 11: rows 44 B apart, 4 B per lane


def test_rows_of_three_f32():
    """12-B rows (W = 4, three lanes a row) with one and with two sources, several rows a tile."""
    g = cube(6, 3, 4)
    a, b = ((0, 0, 0), (2, 5, 5)), ((3, 0, 0), (5, 5, 5))
    contrib = [Ent(g, 0, [a, b, a], 0, 0), Ent(g, 0, [b], 1, 4)]
    zero = [Ent(g, 0, [((-3, 0, 0), (-1, 5, 5)), ((6, 0, 0), (8, 5, 5))])]
    info, _, widths = run_accum(contrib, zero, [SA.DT_F32] * 2, seed=3)
    assert info["n_boxes"] == 2 and info["max_sources"] == 2 and set(widths) == {(2, 2)}


@pytest.mark.parametrize("name", list(GEOS))
def test_every_layout_component_axis_2d_and_strided_fastest_dim(name):
    geo = GEOS[name]
    N, H = geo.ext[0] - 2 * geo.offs[0], geo.offs[0]
    code = SA.DT_F64 if geo.elem == 8 else SA.DT_F32
    info, _, _ = one_domain(N, H, code, geo=geo, seed=len(name))
    assert info["n_boxes"] > 0
    one_domain(N, H, SA.DT_I64 if geo.elem == 8 else SA.DT_I32, geo=geo, seed=len(name) + 1, zero_halos=False)


@pytest.mark.parametrize("which, shift", [("field", 8), ("buffer", 8), ("field", 4), ("buffer", 4), ("field", 12)])
def test_one_misaligned_pointer_narrows_the_launch(which, shift):
    """The field pointer and one buffer pointer, each misaligned alone: the planner's width stays,
    the launch takes the narrower one the real pointers allow."""
    kw = {"fshift": shift} if which == "field" else {"bshift": shift}
    if shift == 8:
        _, _, widths = one_domain(6, 2, SA.DT_F64, seed=41, **kw)
        assert set(widths) == {(4, 3)}
    # f32, N = 8, H = 4: every sub-box has 16-B rows and seven sources
    _, _, widths = one_domain(8, 4, SA.DT_F32, seed=42, **kw)
    assert set(widths) == {(4, 3 if shift == 8 else 2)}
    _, _, widths = one_domain(8, 4, SA.DT_I32, seed=43)
    assert set(widths) == {(4, 4)}


@pytest.mark.parametrize("knobs", [{"tile_bytes": 1024}, {"grid_cap": 1}, {"grid_cap": 7},
                                   {"tile_bytes": 1024, "grid_cap": 7}],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_tile_bytes_and_grid_cap_stay_bit_exact(knobs):
    from ghex_amd import _ghx
    for k, v in knobs.items():
        _ghx.call("ghx_tune", k.encode(), v)
    # N = 19: the send boxes are cut at 0, 2, 17, 19. 1-KiB tiles hold 64 rows of 16 B or 8 rows of
    # 120 B: sub-boxes 2 wide in x have 4, 30 or 225 rows (1, 1, 4 tiles; 12 tiles each side), those
    # 15 wide 4 or 30 rows (1 or 4 tiles; 20 tiles): 44 sum tiles. The receive boxes are 2 or 19
    # wide: 4, 38 or 361 rows of 16 B (1, 1, 6 tiles; 14 each side), 4 or 38 rows of 152 B at 6 rows
    # a tile (1 or 7 tiles; 32): 60 zero tiles
    info, _, _ = one_domain(19, 2, SA.DT_F64, seed=51)
    assert info["n_tiles"] == (44 + 60 if "tile_bytes" in knobs else 52)
    # 2-D, rows of 1200 B: longer than a 1-KiB tile, cut in pieces
    g = cube(300, 2, 4, D=2)
    info, _, _ = one_domain(300, 2, SA.DT_F32, geo=g, seed=52)
    one_domain(6, 2, SA.DT_I32, seed=53, zero_halos=False)


def test_without_zero_halos_the_halo_cells_are_untouched():
    for code, (N, H) in ((SA.DT_F32, (6, 2)), (SA.DT_I64, (3, 2))):
        one_domain(N, H, code, seed=61, zero_halos=False)


def test_order_of_the_adds_is_the_lists_order():
    """f32 values of mixed magnitude over lists of up to 26: the device equals the in-order NumPy
    result bit for bit, and the reversed order gives another result in some cell — this test can
    see a wrong order."""
    for (N, H), seed in (((3, 2), 71), ((6, 2), 72)):
        geo = cube(N, H, 4)
        contrib, zero = SA.one_domain_entries(geo, N, H)
        rng = np.random.default_rng(seed)
        n = contrib[0].nbytes // 4
        msg = (np.exp2(rng.integers(-12, 25, n).astype(np.float64)) * rng.choice([-1.0, 1.0], n) *
               rng.uniform(1, 2, n)).astype(np.float32)
        _, typed, _ = run_accum(contrib, zero, [SA.DT_F32], seed=seed, cell=0.3, messages=[msg])
        buf = np.zeros(contrib[0].nbytes, dtype=np.uint8)
        buf[:] = msg.view(np.uint8)
        start = {0: np.full(geo.n_elems, 0.3, dtype=np.float32)}
        back = SA.definition({0: start[0].copy()}, [buf], contrib, [SA.DT_F32], zero, reverse=True)
        fwd = SA.definition({0: start[0].copy()}, [buf], contrib, [SA.DT_F32], zero)
        np.testing.assert_array_equal(typed[0].view(np.uint32), fwd[0].view(np.uint32))
        assert (back[0].view(np.uint32) != fwd[0].view(np.uint32)).any()


def test_integer_sums_wrap():
    g = cube(2, 2, 4)
    contrib, zero = SA.one_domain_entries(g, 2, 2)
    n = contrib[0].nbytes // 4
    _, typed, _ = run_accum(contrib, zero, [SA.DT_I32], cell=0xFFFFFFF0, messages=[np.full(n, 0x10000001, dtype=np.uint32)],
                            seed=81)
    own = typed[0][g.box_index((0, 0, 0), (1, 1, 1))]
    assert (own == (0xFFFFFFF0 + 26 * 0x10000001) % 2 ** 32).all()


def test_four_domains_with_mixed_dtypes_in_one_plan():
    """2x2x1 periodic domains of 4^3 on one rank: four field slots of four dtypes, one buffer per
    domain pair, lists of 1 / 3 / 7 across entries."""
    codes = [SA.DT_F64, SA.DT_F32, SA.DT_I32, SA.DT_I64]
    lays = [(2, 1, 0), (0, 1, 2), (1, 0, 2), (2, 0, 1)]
    geo = [cube(4, 1, SA.NP[c].itemsize, l) for c, l in zip(codes, lays)]
    contrib, zero = SA.grid_entries((2, 2, 1), 4, 1, True, lambda d: geo[d])
    info, _, _ = run_accum(contrib, zero, [codes[en.slot] for en in contrib], seed=91)
    assert info["max_sources"] == 7
    contrib, zero = SA.grid_entries((2, 2, 1), 4, 2, False, lambda d: cube(4, 2, SA.NP[codes[d]].itemsize, lays[d]))
    info, _, _ = run_accum(contrib, zero, [codes[en.slot] for en in contrib], seed=92)
    assert info["max_sources"] == 3


# ---------------------------------------------------------------------------------------------
# product path
# ---------------------------------------------------------------------------------------------
TORCH = {"f64": np.float64, "f32": np.float32, "i32": np.int32, "i64": np.int64}


def _domain(N, H, dtypes, ctx=None, **opts):
    """One periodic N^3 domain, one x-fastest field per dtype: (co, buffer infos, tensors, geo, send,
    recv boxes). Tensor k is indexed [z, y, x] over (N + 2H)^3."""
    import torch
    import ghex_amd
    from ghex_amd.structured import regular as R
    ctx = ctx or ghex_amd.make_context()
    E = N + 2 * H
    dd = R.DomainDescriptor(0, (0, 0, 0), (N - 1,) * 3)
    pc = R.make_pattern(ctx, R.HaloGenerator((0, 0, 0), (N - 1,) * 3, (H,) * 6, (True,) * 3), [dd])
    ts = [torch.zeros((E, E, E), dtype=torch.from_numpy(np.zeros(1, dtype=TORCH[d])).dtype, device="cuda")
          for d in dtypes]
    bis = [pc(R.make_field_descriptor(dd, t.permute(2, 1, 0), (H,) * 3, (E,) * 3)) for t in ts]
    co = R.make_communication_object(ctx, adjoint_boxes=True, **opts)
    send, recv = SA.periodic_cube(N, H)
    return co, bis, ts, send, recv


def _draw(rng, t, dt):
    """An integer-valued state of a tensor's shape and dtype."""
    return rng.integers(-50, 51, size=tuple(t.shape)).astype(dt)


def _adjoint_of(y, geo, send, recv, zero_halos=True):
    """E^T y of one periodic domain by the definition: box k of the send list gains box k of the
    receive list, in order; then the receive boxes are zero."""
    out = y.reshape(-1).copy()
    for (sf, sl), (rf, rl) in zip(send, recv):
        si, ri = geo.box_index(sf, sl), geo.box_index(rf, rl)
        out[si] = out[si] + y.reshape(-1)[ri]
    if zero_halos:
        for rf, rl in recv:
            out[geo.box_index(rf, rl)] = 0
    return out.reshape(y.shape)


def _load(ts, states):
    import torch
    for t, s in zip(ts, states):
        t.copy_(torch.from_numpy(s))


def _same(ts, wants):
    for t, w in zip(ts, wants):
        np.testing.assert_array_equal(t.cpu().numpy().view(np.uint8), np.ascontiguousarray(w).view(np.uint8))


@pytest.mark.parametrize("N, H", [(6, 2), (3, 2)])
def test_one_rank_five_fields_of_mixed_dtypes(N, H):
    names = ["f64", "f32", "i32", "i64", "f64"]
    co, bis, ts, send, recv = _domain(N, H, names)
    assert all(x["rank"] == co.context.rank() for x in co.plan(bis).send)
    rng = np.random.default_rng(N)
    ys = [_draw(rng, t, TORCH[n]) for t, n in zip(ts, names)]
    geos = [cube(N, H, np.dtype(TORCH[n]).itemsize) for n in names]
    _load(ts, ys)
    co.adjoint_exchange(bis).wait()
    _same(ts, [_adjoint_of(y, g, send, recv) for y, g in zip(ys, geos)])
    _load(ts, ys)
    co.adjoint_exchange(bis, zero_halos=False).wait()
    _same(ts, [_adjoint_of(y, g, send, recv, zero_halos=False) for y, g in zip(ys, geos)])
    # float values of mixed magnitude: the exchange's order is the pattern's box order
    y = (np.exp2(rng.integers(-12, 25, ts[1].shape).astype(np.float64)) * rng.choice([-1.0, 1.0], ts[1].shape)
         ).astype(np.float32)
    _load(ts, [ys[0], y] + ys[2:])
    co.adjoint_exchange(bis).wait()
    _same(ts[1:2], [_adjoint_of(y, geos[1], send, recv)])


def test_transpose_identity_against_the_forward_exchange():
    """<E x, y> = <x, E^T y> with integer-valued f64: E is exchange(), E^T adjoint_exchange()."""
    for N, H in ((6, 2), (5, 3), (2, 2)):
        co, bis, ts, send, recv = _domain(N, H, ["f64", "f64"])
        rng = np.random.default_rng(5 + N)
        for _ in range(2):
            x = [_draw(rng, t, np.float64) for t in ts]
            y = [_draw(rng, t, np.float64) for t in ts]
            out = []
            for state, op in ((x, co.exchange), (y, co.adjoint_exchange)):
                _load(ts, state)
                op(bis).wait()
                out.append([t.cpu().numpy().copy() for t in ts])
            ex, ety = out
            lhs = sum(float((a * b).sum()) for a, b in zip(ex, y))
            rhs = sum(float((a * b).sum()) for a, b in zip(x, ety))
            assert lhs == rhs and any((a != b).any() for a, b in zip(ety, y))


def test_adjoint_twice_then_a_forward_exchange_on_one_object():
    import torch
    N, H = 6, 2
    co, bis, ts, send, recv = _domain(N, H, ["f64"])
    geo = cube(N, H)
    rng = np.random.default_rng(9)
    y = _draw(rng, ts[0], np.float64)
    _load(ts, [y])
    h = co.adjoint_exchange(bis)
    with pytest.raises(RuntimeError, match="not finished"):
        co.adjoint_exchange(bis)
    h.wait()
    want = _adjoint_of(y, geo, send, recv)
    _same(ts, [want])
    co.adjoint_exchange(bis).wait()                                # the halos are zero: nothing added
    _same(ts, [want])
    co.exchange(bis).wait()                                        # halos <- their owners' sums
    fwd = want.reshape(-1).copy()
    for (sf, sl), (rf, rl) in zip(send, recv):
        fwd[geo.box_index(rf, rl)] = want.reshape(-1)[geo.box_index(sf, sl)]
    _same(ts, [fwd.reshape(want.shape)])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    _load(ts, [3 * y])
    torch.cuda.synchronize()
    h = co.schedule_adjoint_exchange(side, bis)
    h.schedule_wait(None)
    h.wait()
    _same(ts, [_adjoint_of(3 * y, geo, send, recv)])


def test_adjoint_replayed_from_a_capture():
    import torch
    N, H = 6, 2
    co, bis, ts, send, recv = _domain(N, H, ["f64", "i32"])
    geos = [cube(N, H, 8), cube(N, H, 4)]
    rng = np.random.default_rng(11)
    ys = [_draw(rng, ts[0], np.float64), _draw(rng, ts[1], np.int32)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    _load(ts, ys)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        co.adjoint_exchange(bis).wait()      # set-up and a warm run, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _same(ts, [_adjoint_of(y, g, send, recv) for y, g in zip(ys, geos)])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        co.adjoint_exchange(bis)
    for k in (3, 5):
        _load(ts, [k * y for y in ys])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _same(ts, [_adjoint_of(k * y, gg, send, recv) for y, gg in zip(ys, geos)])


def _emulated_grid(n, H, periodic, dtype):
    """2x2x1 domains of n^3 as two emulated ranks of two domains each: per rank a communication
    object and its buffer infos; per domain its tensor [z, y, x] and its (first, last)."""
    import torch
    from ghex_amd.structured import regular as R
    from tests.gpu_util import FakeContext
    E = n + 2 * H
    doms = [(r, ((r % 2) * n, (r // 2) * n, 0), ((r % 2 + 1) * n - 1, (r // 2 + 1) * n - 1, n - 1)) for r in range(4)]
    table = {rank: [(i, f, l) for i, f, l in doms[2 * rank:2 * rank + 2]] for rank in range(2)}
    cos, bis_all, ts = [], [], []
    for rank in range(2):
        ctx = FakeContext(rank, 2, table)
        dds = [R.DomainDescriptor(i, f, l) for i, f, l in doms[2 * rank:2 * rank + 2]]
        pc = R.make_pattern(ctx, R.HaloGenerator((0, 0, 0), (2 * n - 1, 2 * n - 1, n - 1), (H,) * 6,
                                                 (periodic,) * 3), dds)
        bis = []
        for dd in dds:
            t = torch.zeros((E, E, E), dtype=torch.from_numpy(np.zeros(1, dtype=dtype)).dtype, device="cuda")
            ts.append(t)
            bis.append(pc(R.make_field_descriptor(dd, t.permute(2, 1, 0), (H,) * 3, (E,) * 3)))
        cos.append(R.make_communication_object(ctx, adjoint_boxes=True))
        bis_all.append(bis)
    return cos, bis_all, ts, doms


@pytest.mark.parametrize("H, periodic, dtype", [(1, True, np.float64), (2, False, np.int32), (1, True, np.int64)])
def test_four_domains_as_two_emulated_ranks(H, periodic, dtype):
    """Every owner cell ends as its value plus the values of all its halo images, every halo cell
    that the pattern fills as zero, every other cell unchanged (integer-valued: any order)."""
    from tests.test_gpu_uaccum import emulated_adjoint
    n = 4
    cos, bis_all, ts, doms = _emulated_grid(n, H, periodic, dtype)
    rng = np.random.default_rng(H)
    ys = [_draw(rng, t, dtype) for t in ts]
    _load(ts, ys)
    moved = emulated_adjoint(cos, bis_all)
    assert moved > 0
    G = (2 * n, 2 * n, n)
    # the images of global cell g: every (domain, local halo cell) whose global position is g
    total = {}
    filled = [np.zeros(y.shape, dtype=bool) for y in ys]
    E = n + 2 * H
    for d, (_, first, _) in enumerate(doms):
        for z in range(-H, n + H):
            for yy in range(-H, n + H):
                for x in range(-H, n + H):
                    if 0 <= x < n and 0 <= yy < n and 0 <= z < n:
                        continue
                    g = (first[0] + x, first[1] + yy, first[2] + z)
                    if periodic:
                        g = tuple(c % m for c, m in zip(g, G))
                    elif not all(0 <= c < m for c, m in zip(g, G)):
                        continue
                    total[g] = total.get(g, 0) + ys[d][z + H, yy + H, x + H]
                    filled[d][z + H, yy + H, x + H] = True
    wants = []
    for d, (_, first, _) in enumerate(doms):
        w = ys[d].copy()
        for z in range(n):
            for yy in range(n):
                for x in range(n):
                    g = (first[0] + x, first[1] + yy, first[2] + z)
                    w[z + H, yy + H, x + H] += total.get(g, 0)
        w[filled[d]] = 0
        wants.append(w)
    _same(ts, wants)
    assert any((w != y).any() for w, y in zip(wants, ys))


def test_refusals_of_the_python_interface(golden_dir):
    import torch
    from ghex_amd import unstructured as U
    from ghex_amd.structured import regular as R
    from tests.test_gpu_uput import _known_answer
    N, H = 6, 1
    co, bis, ts, _, _ = _domain(N, H, ["f64"])
    ctx = co.context
    plain = R.make_communication_object(ctx)                      # without the option: as before
    with pytest.raises(ValueError, match="unstructured fields only"):
        plain.adjoint_exchange(bis)
    for kw in (dict(direct=True), dict(pipelined=True)):
        with pytest.raises(ValueError, match="plain communication object"):
            R.make_communication_object(ctx, adjoint_boxes=True, **kw).adjoint_exchange(bis)
    uctx, upc, ubis, _ = _known_answer(golden_dir, 1, True)
    with pytest.raises(ValueError, match="not both"):
        co.adjoint_exchange(bis + ubis)
    with pytest.raises(ValueError, match="not both"):
        co.adjoint_pack_only(ubis + bis)
    both = U.make_communication_object(uctx, adjoint_boxes=True)
    both.adjoint_exchange(ubis).wait()                            # all-unstructured lists: today's path
    E = N + 2 * H
    for dt in (torch.float16, torch.bfloat16, torch.uint8, torch.int16):
        t = torch.zeros((E, E, E), dtype=dt, device="cuda")
        fd = R.make_field_descriptor(bis[0].field.domain, t, (H,) * 3, (E,) * 3)
        with pytest.raises(TypeError, match="not supported"):
            co.adjoint_exchange([bis[0].pattern_container(fd)])
    import types
    from ghex_amd import _ghx
    cs = types.SimpleNamespace(field=types.SimpleNamespace(kind=0, cs_item=_ghx.CsItem(), desc=_ghx.FieldDesc(), align=8,
                                                           domain_id=lambda: 0),
                               pattern_container=object(), local_index=0)
    with pytest.raises(ValueError, match="cubed-sphere"):
        co.adjoint_pack_only([cs])
    with pytest.raises(ValueError, match="cubed-sphere"):
        co.adjoint_accumulate_only([cs] + bis)
    with pytest.raises(ValueError, match="unstructured fields only"):
        plain.adjoint_pack_only([cs])
    rng = np.random.default_rng(1)
    y = _draw(rng, ts[0], np.float64)
    _load(ts, [y])
    co.adjoint_exchange(bis).wait()          # the object is still usable
    send, recv = SA.periodic_cube(N, H)
    _same(ts, [_adjoint_of(y, cube(N, H), send, recv)])
