"""The fused self adjoint on the device (ghx_saccum_get_create, k_accum_get_s,
ghx_sexchange_adjoint_self_*, CommunicationObject(adjoint_boxes=True, fuse_adjoint=True)). Kernel
cases through the ABI: every field and every buffer in an arena of its own between 256-byte guard
bands; after ONE execute every byte of every arena is compared — owner cells with the NumPy
definition (tests/sget_cases.py: each self message gathered from the halo cells in buffer order,
adds in ascending (entry, box)), receive cells exact zero bytes (or unchanged without zero_halos),
every other byte of the fields, the buffers and the guards unchanged. Product path: the fused
object against an unfused one on equal inputs, the transpose identity against exchange(), adjoint
twice then a forward exchange, graph replay, the refusals. Every comparison is bit-exact.

Shapes as in tests/test_gpu_saccum.py (one periodic domain of N^3, halo H): sources 1 / 3 / 7 at
N=6, lists of up to 26 (several batches of four loads and a remainder) at N <= 5. Float inputs
other than the order test's are drawn with magnitudes in [2^-20, 2^20] or are integer-valued."""
import numpy as np
import pytest

from tests import saccum_cases as SA
from tests import sget_cases as SG
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


def run_get(contrib, sources, zero, dtypes, fshift=0, bshift=0, zero_halos=True, seed=0, init=None, messages=None):
    """One get plan over the entries, one execute, every arena compared byte for byte. fshift /
    bshift: bytes by which field slot 0 / the first buffer that is read are moved off their 256-byte
    alignment. init[slot]: the field's elements (default: drawn); messages[e]: the elements of a
    buffered entry's message (default: drawn). Returns (info, typed fields after, typed fields
    before, planned and launched width log2 per sum sub-box)."""
    import torch
    from ghex_amd import _ghx
    rng = np.random.default_rng(9000 + seed)
    geo_of, code_of = {}, {}
    for en, c in zip(contrib, dtypes):
        geo_of[en.slot], code_of[en.slot] = en.geo, c
    for e, s in enumerate(sources):
        if s is not None:
            geo_of.setdefault(s.slot, s.geo)
            code_of.setdefault(s.slot, dtypes[e])
    for z in zero:
        geo_of.setdefault(z.slot, z.geo)
        code_of.setdefault(z.slot, SA.DT_I64 if z.geo.elem == 8 else SA.DT_I32)
    nf = 1 + max(geo_of)
    buffered = [e for e, s in enumerate(sources) if s is None]
    nb = 1 + max([contrib[e].bslot for e in buffered], default=-1)
    fields, before = [None] * nf, {}
    for k, g in geo_of.items():
        fields[k] = Arena(g.n_elems * g.elem, fshift if k == 0 else 0)
        v = SA.draw_values(rng, g.n_elems, code_of[k])
        if init is not None and k in init:
            v[:] = init[k]
        before[k] = v.copy()
        raw = v.view(np.uint8)
        fields[k].host[fields[k].at:fields[k].at + raw.size] = raw
        fields[k].view.copy_(torch.from_numpy(fields[k].host))
    ends = [0] * nb
    for e in buffered:
        en = contrib[e]
        ends[en.bslot] = max(ends[en.bslot], en.boff + en.nbytes)
    first_buf = min((contrib[e].bslot for e in buffered), default=-1)
    bufs = [Arena(n, bshift if b == first_buf else 0) if n else None for b, n in enumerate(ends)]
    for e in buffered:
        en = contrib[e]
        n = en.nbytes // en.geo.elem
        m = (SA.draw_values(rng, n, dtypes[e]) if messages is None or messages[e] is None
             else np.asarray(messages[e], dtype=SA.NP[dtypes[e]]).reshape(n))
        a = bufs[en.bslot]
        a.host[a.at + en.boff:a.at + en.boff + en.nbytes] = m.view(np.uint8)
    for a in bufs:
        if a is not None:
            a.view.copy_(torch.from_numpy(a.host))
    h = SG.create(contrib, dtypes, sources, zero)
    try:
        info = SA.info(h)
        subs, knd = SA.boxes(h, contrib[0].geo.spatial), SG.kinds(h)
        widths = []
        for s in subs:
            if not s.zero:
                w = min(s.wlog2, _ctz(fields[s.slot].ptr))
                for j in range(s.first_src, s.first_src + s.n_src):
                    kind, slot, _ = knd[j]
                    w = min(w, _ctz((fields if kind else bufs)[slot].ptr))
                widths.append((s.wlog2, w))
        fp = _ghx.ptr_array([a.ptr if a else 0 for a in fields])
        bp = _ghx.ptr_array([a.ptr if a else 0 for a in bufs] or [0])
        _ghx.call("ghx_saccum_get_execute", h, fp, nf, bp, nb, 1 if zero_halos else 0,
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        SA.destroy(h)
    typed = {k: v.copy() for k, v in before.items()}
    images = [a.field() if a else None for a in bufs]
    SG.definition(typed, images, contrib, dtypes, sources, zero, zero_halos)
    for k, a in enumerate(fields):
        if a is None:
            continue
        want = a.host.copy()
        want[a.at:a.at + typed[k].nbytes] = typed[k].view(np.uint8)
        got = a.device_bytes()
        assert (got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all()
        np.testing.assert_array_equal(got, want)
        if init is None and any(en.slot == k for en in contrib):
            assert (want != a.host).any()
    for a in bufs:
        if a is not None:
            np.testing.assert_array_equal(a.device_bytes(), a.host)   # read only, guards included
    for z in zero:                                                    # exact zero bytes, or untouched
        for f, l in z.boxes:
            idx = z.geo.box_index(f, l)
            if zero_halos:
                assert (typed[z.slot][idx].view(np.uint8) == 0).all()
            else:
                np.testing.assert_array_equal(typed[z.slot][idx].view(np.uint8), before[z.slot][idx].view(np.uint8))
    return info, typed, before, widths


def one_domain(N, H, code, layout=None, seed=0, geo=None, **kw):
    geo = geo or cube(N, H, SA.NP[code].itemsize, layout)
    contrib, sources, zero = SG.one_domain(geo, N, H)
    return run_get(contrib, sources, zero, [code], seed=seed, **kw)


# ---------------------------------------------------------------------------------------------
# kernel cases
# ---------------------------------------------------------------------------------------------
SHAPES = {(6, 2): 7, (6, 1): 7, (5, 3): 26, (3, 2): 26, (2, 2): 26}


@pytest.mark.parametrize("zero_halos", [True, False], ids=["zero", "keep"])
@pytest.mark.parametrize("code", SA.DTYPES, ids=lambda c: SA.NAMES[c])
@pytest.mark.parametrize("N, H", list(SHAPES))
def test_every_shape_and_dtype(N, H, code, zero_halos):
    info, _, _, widths = one_domain(N, H, code, seed=N * 10 + H + code, zero_halos=zero_halos)
    assert info["max_sources"] == SHAPES[(N, H)] and info["n_zero_boxes"] == 0
    if (N, H) == (6, 2) and SA.NP[code].itemsize == 8:
        assert set(widths) == {(4, 4)}                   # 16-B rows, 16 B per lane, both sides
    if (N, H) == (6, 1) and SA.NP[code].itemsize == 8:
        assert (3, 3) in widths                          # one-element rows, 8 B per lane
    if (N, H) == (5, 3) and SA.NP[code].itemsize == 4:
        assert {w for _, w in widths} == {2}             # E = 11: rows 44 B apart, 4 B per lane


def test_rows_of_three_f32():
    """12-B rows (W = 4, three lanes a row): N = 6, H = 3, the x faces alone, one field source and a
    field source beside a buffer."""
    g = cube(6, 3, 4)
    a, b = ((0, 0, 0), (2, 5, 5)), ((3, 0, 0), (5, 5, 5))
    ha, hb = ((6, 0, 0), (8, 5, 5)), ((-3, 0, 0), (-1, 5, 5))
    contrib = [Ent(g, 0, [a, b], 0, 0), Ent(g, 0, [b], 1, 4)]
    sources = [Ent(g, 0, [ha, hb]), None]
    info, _, _, widths = run_get(contrib, sources, [Ent(g, 0, [ha, hb])], [SA.DT_F32] * 2, seed=3)
    assert info["n_boxes"] == 2 and info["max_sources"] == 2 and set(widths) == {(2, 2)}
    info, _, _, widths = one_domain(6, 3, SA.DT_F32, seed=4)
    assert {w for _, w in widths} == {2}


@pytest.mark.parametrize("name", list(GEOS))
def test_every_layout_component_axis_2d_and_strided_fastest_dim(name):
    geo = GEOS[name]
    N, H = geo.ext[0] - 2 * geo.offs[0], geo.offs[0]
    code = SA.DT_F64 if geo.elem == 8 else SA.DT_F32
    info, _, _, _ = one_domain(N, H, code, geo=geo, seed=len(name))
    assert info["n_boxes"] > 0
    one_domain(N, H, SA.DT_I64 if geo.elem == 8 else SA.DT_I32, geo=geo, seed=len(name) + 1, zero_halos=False)


def test_a_source_field_of_other_strides_and_a_strided_one():
    g = cube(6, 2)
    send = [((0, 0, 0), (1, 5, 5)), ((4, 0, 0), (5, 5, 5))]
    recv = [((6, 0, 0), (7, 5, 5)), ((-2, 0, 0), (-1, 5, 5))]
    for sg in (cube(6, 3), cube(6, 2, fast=2)):
        src = Ent(sg, 1, recv)
        run_get([Ent(g, 0, send)], [src], [src], [SA.DT_F64], seed=5)
        run_get([Ent(g, 0, send)], [src], [src], [SA.DT_I64], seed=6, zero_halos=False)


@pytest.mark.parametrize("shift", [8, 4, 12])
def test_a_misaligned_field_pointer_narrows_the_launch(shift):
    """The field holds both sides: its pointer narrows the cell vectors and the source vectors."""
    if shift == 8:
        _, _, _, widths = one_domain(6, 2, SA.DT_F64, seed=41, fshift=shift)
        assert set(widths) == {(4, 3)}
    # f32, N = 8, H = 4: every sub-box has 16-B rows and seven sources
    _, _, _, widths = one_domain(8, 4, SA.DT_F32, seed=42, fshift=shift)
    assert set(widths) == {(4, 3 if shift == 8 else 2)}
    _, _, _, widths = one_domain(8, 4, SA.DT_I32, seed=43)
    assert set(widths) == {(4, 4)}


@pytest.mark.parametrize("knobs", [{"tile_bytes": 1024}, {"grid_cap": 1}, {"grid_cap": 7},
                                   {"tile_bytes": 1024, "grid_cap": 7}],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_tile_bytes_and_grid_cap_stay_bit_exact(knobs):
    from ghex_amd import _ghx
    for k, v in knobs.items():
        _ghx.call("ghx_tune", k.encode(), v)
    # N = 19: 44 sum tiles of 1 KiB (tests/test_gpu_saccum.py), 26 of 8 KiB; no zero tiles
    info, _, _, _ = one_domain(19, 2, SA.DT_F64, seed=51)
    assert info["n_tiles"] == (44 if "tile_bytes" in knobs else 26)
    # 2-D, rows of 1200 B: longer than a 1-KiB tile, cut in pieces
    g = cube(300, 2, 4, D=2)
    one_domain(300, 2, SA.DT_F32, geo=g, seed=52)
    one_domain(6, 2, SA.DT_I32, seed=53, zero_halos=False)


def test_order_of_the_adds_is_the_lists_order():
    """f32 and f64 halo values of mixed magnitude over lists of up to 26: the device equals the
    in-order NumPy result bit for bit, and the reversed order gives another result in some cell."""
    for (N, H), code, seed in (((3, 2), SA.DT_F32, 71), ((6, 2), SA.DT_F32, 72), ((3, 2), SA.DT_F64, 73)):
        dt = SA.NP[code]
        geo = cube(N, H, dt.itemsize)
        contrib, sources, zero = SG.one_domain(geo, N, H)
        rng = np.random.default_rng(seed)
        n = geo.n_elems
        span = (-12, 25) if code == SA.DT_F32 else (-26, 53)
        F = (np.exp2(rng.integers(*span, n).astype(np.float64)) * rng.choice([-1.0, 1.0], n) *
             rng.uniform(1, 2, n)).astype(dt)
        _, typed, before, _ = run_get(contrib, sources, zero, [code], seed=seed, init={0: F})
        fwd = SG.definition({0: F.copy()}, [], contrib, [code], sources, zero)
        back = SG.definition({0: F.copy()}, [], contrib, [code], sources, zero, reverse=True)
        np.testing.assert_array_equal(typed[0].view(np.uint8), fwd[0].view(np.uint8))
        assert (back[0].view(np.uint8) != fwd[0].view(np.uint8)).any()


def test_integer_sums_wrap():
    g = cube(2, 2, 4)
    contrib, sources, zero = SG.one_domain(g, 2, 2)
    F = np.full(g.n_elems, 0x10000001, dtype=np.uint32)
    own = g.box_index((0, 0, 0), (1, 1, 1))
    F[own] = 0xFFFFFFF0
    _, typed, _, _ = run_get(contrib, sources, zero, [SA.DT_I32], init={0: F}, seed=81)
    assert (typed[0][own] == (0xFFFFFFF0 + 26 * 0x10000001) % 2 ** 32).all()


def test_four_domains_with_mixed_dtypes_in_one_plan():
    """2x2x1 domains of 4^3 on one rank: four field slots of four dtypes, every message read from
    another slot's (or the slot's own) halo cells. Not periodic: the halo cells no box holds keep
    their values (the whole-arena comparison)."""
    codes = [SA.DT_F64, SA.DT_I64, SA.DT_F64, SA.DT_I64]       # a pair shares its element
    lays = [(2, 1, 0)] * 4
    geo = [cube(4, 1, SA.NP[c].itemsize, l) for c, l in zip(codes, lays)]
    contrib, sources, zero = SG.grid((2, 2, 1), 4, 1, True, lambda d: geo[d])
    keep = [(c, s) for c, s in zip(contrib, sources) if codes[c.slot] == codes[s.slot]]
    # messages between slots of different dtypes stay buffered: a mixed plan over four fields
    sources = [s if codes[c.slot] == codes[s.slot] else None for c, s in zip(contrib, sources)]
    assert any(s is None for s in sources) and keep
    info, _, _, _ = run_get(contrib, sources, zero, [codes[en.slot] for en in contrib], seed=91)
    assert info["max_sources"] == 7
    codes = [SA.DT_F32, SA.DT_I32, SA.DT_F32, SA.DT_I32]
    lays = [(0, 1, 2)] * 4
    geo = [cube(4, 2, 4, l) for l in lays]
    contrib, sources, zero = SG.grid((2, 2, 1), 4, 2, False, lambda d: geo[d])
    sources = [s if codes[c.slot] == codes[s.slot] else None for c, s in zip(contrib, sources)]
    info, typed, before, _ = run_get(contrib, sources, zero, [codes[en.slot] for en in contrib], seed=92)
    assert info["max_sources"] == 3
    held = np.zeros(geo[0].n_elems, dtype=bool)
    for z in zero:
        if z.slot == 0:
            for f, l in z.boxes:
                held[geo[0].box_index(f, l)] = True
    held[geo[0].box_index((0, 0, 0), (3, 3, 3))] = True
    assert (~held).any()
    np.testing.assert_array_equal(typed[0][~held].view(np.uint8), before[0][~held].view(np.uint8))


def test_four_domains_all_self_periodic_and_not():
    for H, periodic, code in ((1, True, SA.DT_F64), (2, False, SA.DT_I32)):
        geo = cube(4, H, SA.NP[code].itemsize)
        contrib, sources, zero = SG.grid((2, 2, 1), 4, H, periodic, lambda d: geo)
        info, _, _, _ = run_get(contrib, sources, zero, [code] * len(contrib), seed=93 + H)
        assert info["n_zero_boxes"] == 0 and info["max_sources"] == (7 if periodic else 3)


def test_the_mixed_plan_with_drawn_peer_messages():
    """Rank 0 of (2,1,1) x 4^3, H = 2, periodic: 8 self boxes from the halos, 18 peer boxes from
    the send buffers, in one launch; zero tiles over the peer boxes."""
    from ghex_amd import _ghx
    from tests.test_sget_host import mixed_entries, two_rank_plan
    for code in (SA.DT_F64, SA.DT_I32):
        geo = cube(4, 2, SA.NP[code].itemsize)
        _, pc = two_rank_plan(_ghx, 0, [geo])
        contrib, sources, zero = mixed_entries(pc, geo, 0)
        for zh in (True, False):
            info, _, _, _ = run_get(contrib, sources, zero, [code] * len(contrib), seed=95, zero_halos=zh, bshift=8)
            assert info["n_zero_boxes"] == 18


# ---------------------------------------------------------------------------------------------
# product path
# ---------------------------------------------------------------------------------------------
TORCH = {"f64": np.float64, "f32": np.float32, "i32": np.int32, "i64": np.int64}


def _domain(N, H, dtypes, fused=True, **opts):
    """One periodic N^3 domain, one x-fastest field per dtype: (co, buffer infos, tensors, send,
    recv boxes). Tensor k is indexed [z, y, x] over (N + 2H)^3."""
    import torch
    import ghex_amd
    from ghex_amd.structured import regular as R
    ctx = ghex_amd.make_context()
    E = N + 2 * H
    dd = R.DomainDescriptor(0, (0, 0, 0), (N - 1,) * 3)
    pc = R.make_pattern(ctx, R.HaloGenerator((0, 0, 0), (N - 1,) * 3, (H,) * 6, (True,) * 3), [dd])
    ts = [torch.zeros((E, E, E), dtype=torch.from_numpy(np.zeros(1, dtype=TORCH[d])).dtype, device="cuda")
          for d in dtypes]
    bis = [pc(R.make_field_descriptor(dd, t.permute(2, 1, 0), (H,) * 3, (E,) * 3)) for t in ts]
    co = R.make_communication_object(ctx, adjoint_boxes=True, fuse_adjoint=fused, **opts)
    send, recv = SA.periodic_cube(N, H)
    return co, bis, ts, send, recv


def _draw(rng, t, dt):
    return rng.integers(-50, 51, size=tuple(t.shape)).astype(dt)


def _load(ts, states):
    import torch
    for t, s in zip(ts, states):
        t.copy_(torch.from_numpy(s))


def _same(ts, wants):
    for t, w in zip(ts, wants):
        np.testing.assert_array_equal(t.cpu().numpy().view(np.uint8), np.ascontiguousarray(w).view(np.uint8))


def _form(co, bis):
    import ctypes
    from ghex_amd import _ghx
    f = ctypes.c_int32(-1)
    _ghx.call("ghx_sexchange_adjoint_self_info", co.plan(bis).h, ctypes.byref(f), None, None, None)
    return f.value


@pytest.mark.parametrize("N, H", [(6, 2), (3, 2)])
def test_fused_object_against_an_unfused_one(N, H):
    """Equal inputs, mixed dtypes and mixed magnitudes: the fields agree bit for bit with and
    without zero_halos, and the fused form leaves the buffers of its self messages alone."""
    import torch
    names = ["f64", "f32", "i32", "i64", "f32"]
    fco, fbis, fts, _, _ = _domain(N, H, names)
    uco, ubis, uts, _, _ = _domain(N, H, names, fused=False)
    rng = np.random.default_rng(N)
    ys = [_draw(rng, t, TORCH[n]) for t, n in zip(fts, names)]
    ys[4] = (np.exp2(rng.integers(-12, 25, fts[4].shape).astype(np.float64)) * rng.choice([-1.0, 1.0], fts[4].shape)
             ).astype(np.float32)
    plan = fco.plan(fbis)
    send, recv = fco.buffers(plan, fts[0].device)
    for t in send + recv:
        t.fill_(0xA5)
    for zh in (True, False):
        _load(fts, ys)
        _load(uts, ys)
        fco.adjoint_exchange(fbis, zero_halos=zh).wait()
        uco.adjoint_exchange(ubis, zero_halos=zh).wait()
        _same(fts, [t.cpu().numpy() for t in uts])
        assert any((t.cpu().numpy() != y).any() for t, y in zip(fts, ys))
    assert _form(fco, fbis) == 1 and _form(uco, ubis) == 0
    assert plan._adjoint_prefix == "ghx_sexchange_adjoint_self_"
    assert uco.plan(ubis)._adjoint_prefix == "ghx_sexchange_adjoint_"
    torch.cuda.synchronize()
    for t in send + recv:
        assert bool((t == 0xA5).all())                    # self buffers: not touched
    # the two launches alone take the same choice
    _load(fts, ys)
    fco.adjoint_pack_only(fbis)
    fco.adjoint_accumulate_only(fbis, zero_halos=False)
    torch.cuda.synchronize()
    _same(fts, [t.cpu().numpy() for t in uts])
    for t in send + recv:
        assert bool((t == 0xA5).all())


def test_fuse_self_off_takes_the_unfused_path():
    co, bis, ts, _, _ = _domain(6, 1, ["f64"], fuse_self=False)
    rng = np.random.default_rng(2)
    y = _draw(rng, ts[0], np.float64)
    _load(ts, [y])
    co.adjoint_exchange(bis).wait()
    assert co.plan(bis)._adjoint_prefix == "ghx_sexchange_adjoint_" and _form(co, bis) == 0
    assert (ts[0].cpu().numpy() != y).any()


def test_transpose_identity_against_the_forward_exchange():
    """<E x, y> = <x, E^T y> with integer-valued f64: E is exchange(), E^T the fused adjoint."""
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
        assert _form(co, bis) == 1


def _adjoint_of(y, geo, send, recv, zero_halos=True):
    out = y.reshape(-1).copy()
    for (sf, sl), (rf, rl) in zip(send, recv):
        si, ri = geo.box_index(sf, sl), geo.box_index(rf, rl)
        out[si] = out[si] + y.reshape(-1)[ri]
    if zero_halos:
        for rf, rl in recv:
            out[geo.box_index(rf, rl)] = 0
    return out.reshape(y.shape)


def test_adjoint_twice_then_a_forward_exchange_on_one_object():
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
    for k in (3, 5, 7):
        _load(ts, [k * y for y in ys])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _same(ts, [_adjoint_of(k * y, gg, send, recv) for y, gg in zip(ys, geos)])


def test_two_emulated_ranks_fused_against_unfused():
    """(2,1,1) x 4^3, H = 2, periodic, as two emulated ranks: the mixed form (8 self boxes from the
    halos, 18 peer boxes through the buffers) against the unfused objects on equal inputs."""
    import torch
    from ghex_amd.structured import regular as R
    from tests.gpu_util import FakeContext
    from tests.test_gpu_uaccum import emulated_adjoint
    n, H = 4, 2
    E = n + 2 * H
    doms = [(r, (r * n, 0, 0), ((r + 1) * n - 1, n - 1, n - 1)) for r in range(2)]
    table = {r: [doms[r]] for r in range(2)}
    for dtype in (np.float64, np.int32):
        results = []
        rng = np.random.default_rng(4)
        ys = [_draw(rng, torch.zeros((E, E, E)), dtype) for _ in range(2)]
        for fused in (True, False):
            cos, bis_all, ts = [], [], []
            for rank in range(2):
                ctx = FakeContext(rank, 2, table)
                dd = R.DomainDescriptor(*doms[rank])
                pc = R.make_pattern(ctx, R.HaloGenerator((0, 0, 0), (2 * n - 1, n - 1, n - 1), (H,) * 6, (True,) * 3), [dd])
                t = torch.zeros((E, E, E), dtype=torch.from_numpy(np.zeros(1, dtype=dtype)).dtype, device="cuda")
                ts.append(t)
                bis_all.append([pc(R.make_field_descriptor(dd, t.permute(2, 1, 0), (H,) * 3, (E,) * 3))])
                cos.append(R.make_communication_object(ctx, adjoint_boxes=True, fuse_adjoint=fused))
            _load(ts, ys)
            assert emulated_adjoint(cos, bis_all) > 0
            torch.cuda.synchronize()
            results.append([t.cpu().numpy() for t in ts])
            assert [_form(co, b) for co, b in zip(cos, bis_all)] == ([2, 2] if fused else [0, 0])
        for a, b, y in zip(results[0], results[1], ys):
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
            assert (a != y).any()


def test_refusals_of_the_python_interface():
    import ghex_amd
    from ghex_amd.communication_object import CommunicationObject
    from ghex_amd.structured import regular as R
    ctx = ghex_amd.make_context()
    with pytest.raises(ValueError, match="adjoint_boxes"):
        CommunicationObject(ctx, fuse_adjoint=True)
    with pytest.raises(ValueError, match="adjoint_boxes"):
        R.make_communication_object(ctx, fuse_adjoint=True)
    assert CommunicationObject(ctx, adjoint_boxes=True).fuse_adjoint is False
    for kw in (dict(direct=True), dict(pipelined=True)):
        co, bis, ts, _, _ = _domain(6, 1, ["f64"], **kw)
        with pytest.raises(ValueError, match="plain communication object"):
            co.adjoint_exchange(bis)
