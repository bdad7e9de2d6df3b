"""The fused self adjoint of unstructured fields on the device (ghx_uaccum_get_create,
k_accum_get_u, CommunicationObject(fuse_adjoint_lists=True)). Kernel cases through the ABI: every
field and every buffer in an arena of its own between 256-byte guard bands; after ONE execute every
byte of every arena is compared - owner fields with the NumPy definition with field sources
(tests/uget_cases.py: adds in ascending (entry, position), a sourced entry's message read from the
halo field), halo fields hold exact zero rows where a zero entry or a source names them (or are
unchanged without zero_halos), buffers are unchanged, guards still the sentinel. Product path: the
known-answer case on one rank (form 1) and as two emulated ranks (form 2) and twenty random meshes,
a fused object against an unfused one on copies of the same fields. Every comparison is of bytes.

Float inputs other than the order pins are drawn with magnitudes in [2^-20, 2^20] or are
integer-valued: no result is subnormal, inf or NaN (those are not part of the contract)."""
import numpy as np
import pytest

from tests import uaccum_cases as UA
from tests import uget_cases as UG
from tests import uput_cases as UC
from tests import uself_cases as US
from tests.uput_cases import N_CELLS, Side, udesc

pytestmark = pytest.mark.gpu

GUARD, SENTINEL, BIAS = 256, 0xC3, 1 << 31


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


def _fill(arena, at, values):
    """Typed values into an arena's host image and device memory from field byte `at` on."""
    import torch
    raw = np.ascontiguousarray(values).reshape(-1).view(np.uint8)
    arena.host[arena.at + at:arena.at + at + raw.size] = raw
    arena.view.copy_(torch.from_numpy(arena.host))


def run_get(contrib, zero, places, sources, dtypes, oshift=0, hshift=0, bshift=0, obias=0, hbias=0,
            zero_halos=True, seed=0, values=None, messages=None, n_cells=N_CELLS):
    """contrib[e]: the owner Side of message e (dtype code dtypes[e]); sources[e]: its halo Side or
    None (then the message lies at places[e]); zero: the zero Sides. One plan, one execute, every
    arena compared byte for byte. oshift / hshift / bshift move the owner fields, the other fields
    and the buffers by that many bytes; obias / hbias add to that side's lids (an int64 table, wide
    records for hbias) and move its pointers back. values: {slot: {element index: value}} written
    over the drawn field values; messages[e]: the (n, levels) contributions of a buffered entry e
    (default: drawn). Returns (plan info, fields after, fields before) as typed arrays per slot."""
    import torch
    from ghex_amd import _ghx
    from tests.test_gpu_uput import Arena
    rng = np.random.default_rng(5000 + seed)
    halos = [s for s in sources if s is not None] + list(zero)
    nf = 1 + max(s.slot for s in list(contrib) + halos)
    code_of, desc_of, owners = {}, {}, {s.slot for s in contrib}
    for s, c in zip(contrib, dtypes):
        code_of[s.slot], desc_of[s.slot] = c, s.desc
    for e, s in enumerate(sources):
        if s is not None:
            code_of.setdefault(s.slot, dtypes[e])
            desc_of.setdefault(s.slot, s.desc)
    for z in zero:
        assert z.slot in code_of or z.desc.elem_size in (4, 8)
        code_of.setdefault(z.slot, UA.DT_I32 if z.desc.elem_size == 4 else UA.DT_I64)
        desc_of.setdefault(z.slot, z.desc)
    fields, back = [None] * nf, [0] * nf
    for k, d in desc_of.items():
        span = UC.span_bytes(d, n_cells)
        fields[k] = Arena(span, oshift if k in owners else hshift)
        v = UA.draw_values(rng, span // d.elem_size, code_of[k])
        for at, x in (values or {}).get(k, {}).items():
            v[at] = x
        _fill(fields[k], 0, v)
        back[k] = (obias if k in owners else hbias) * d.index_stride * d.elem_size
    buffered = [e for e, s in enumerate(sources) if s is None]
    nb = 1 + max([places[e][0] for e in buffered], default=-1)
    ends = [0] * nb
    for e in buffered:
        b, off = places[e]
        ends[b] = max(ends[b], off + US.message_bytes(contrib[e]))
    bufs = [Arena(e, bshift) if e else None for e in ends]
    for e in buffered:
        (b, off), d, n = places[e], contrib[e].desc, contrib[e].lids.size
        m = (UA.draw_values(rng, n * d.levels, dtypes[e]).reshape(n, d.levels) if messages is None
             else np.asarray(messages[e], dtype=UA.NP[dtypes[e]]).reshape(n, d.levels))
        _fill(bufs[b], off, m if d.levels_first else m.T)

    def biased(s):
        return None if s is None else Side(s.desc, s.slot, s.lids + (obias if s.slot in owners else hbias))
    zero_of = {id(z): biased(z) for z in zero}           # a source that is a zero entry stays the same list
    plan_s = [None if s is None else zero_of.get(id(s), biased(s)) for s in sources]
    h = UG.create([biased(s) for s in contrib], dtypes, places, plan_s, [zero_of[id(z)] for z in zero])
    try:
        fp = _ghx.ptr_array([(a.ptr - bk) if a else 0 for a, bk in zip(fields, back)])
        bp = _ghx.ptr_array([a.ptr if a else 0 for a in bufs])
        info = UA.info(h)
        _ghx.call("ghx_uaccum_get_execute", h, fp, nf, bp, nb, 1 if zero_halos else 0,
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        UA.destroy(h)
    start = {k: fields[k].field()[:UC.span_bytes(d, n_cells)].copy().view(UA.NP[code_of[k]])
             for k, d in desc_of.items()}
    typed = {k: v.copy() for k, v in start.items()}
    images = [a.field() if a else None for a in bufs]
    UG.definition(typed, images, contrib, dtypes, places, sources, zero, zero_halos)
    for k, a in enumerate(fields):
        if a is None:
            continue
        want = a.host.copy()
        want[a.at:a.at + typed[k].nbytes] = typed[k].view(np.uint8)
        got = a.device_bytes()
        assert (got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all()
        np.testing.assert_array_equal(got, want)
        changed = (want != a.host).sum()
        if k not in owners:
            assert changed > 0 if zero_halos else changed == 0
    for a in bufs:
        if a is not None:
            np.testing.assert_array_equal(a.device_bytes(), a.host)   # read only, guards included
    for z in halos:                                                   # exact zero rows
        rows = typed[z.slot][UA.element_index(z)]
        assert (rows.view(np.uint8) == 0).all() == bool(zero_halos)
    return info, typed, start


def _descs(mode, e, levels):
    """Owner and halo descriptor of a row mode (tests/test_gpu_uaccum.py's): 0 contiguous levels,
    1 levels-first messages over strided levels, 2 levels last."""
    if mode == 0:
        return udesc(e, levels), udesc(e, levels)
    if mode == 1:
        return udesc(e, levels, index_stride=1, level_stride=N_CELLS), udesc(e, levels, index_stride=1,
                                                                            level_stride=N_CELLS + 3)
    return udesc(e, levels, first=False), udesc(e, levels, first=False, level_stride=N_CELLS + 16 // e)


def three(code, mode=0, levels=3, seed=0, repeats=True, descs=None, sourced=(True, True, True), **kw):
    e = UA.NP[code].itemsize
    od, hd = descs or _descs(mode, e, levels)
    contrib, zero, places, sources = UG.three_lists(od, hd, seed=seed, repeats=repeats, sourced=sourced)
    return run_get(contrib, zero, places, sources, [code] * 3, seed=seed, **kw), (contrib, sources)


# ---------------------------------------------------------------------------------------------
# kernel cases
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_halos", [True, False], ids=["zero", "keep"])
@pytest.mark.parametrize("levels", [1, 3, 8])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("code", UA.DTYPES, ids=lambda c: UA.NAMES[c])
def test_every_dtype_row_mode_level_count_and_zero_halos(code, mode, levels, zero_halos):
    (info, _, _), _ = three(code, mode, levels, seed=code * 100 + mode * 10 + levels, zero_halos=zero_halos)
    assert info["max_per_dest"] == 287 and info["n_contrib"] == 9006 and info["bytes"] == 0
    assert info["n_zero_dest"] == 0 and info["n_tiles"] > 8        # sum tiles only, the last of a slot partial


@pytest.mark.parametrize("code", UA.DTYPES, ids=lambda c: UA.NAMES[c])
def test_a_source_field_of_other_strides_and_level_order(code):
    e = UA.NP[code].itemsize
    three(code, seed=11, descs=(udesc(e, 3, index_stride=5), udesc(e, 3, first=False, level_stride=N_CELLS + 7)))
    three(code, seed=12, descs=(udesc(e, 2, first=False, level_stride=N_CELLS + 5),
                                udesc(e, 2, index_stride=6, level_stride=3)))
    three(code, seed=13, descs=(udesc(e, 4, index_stride=1, level_stride=N_CELLS + 1), udesc(e, 4, index_stride=9)))


@pytest.mark.parametrize("code", UA.DTYPES, ids=lambda c: UA.NAMES[c])
def test_pointers_aligned_to_the_element_only(code):
    e = UA.NP[code].itemsize
    three(code, 0, 3, seed=21, oshift=e, hshift=e)
    three(code, 2, 3, seed=22, oshift=e, sourced=(True, False, True), bshift=e)
    three(code, 1, 1, seed=23, hshift=3 * e)


@pytest.mark.parametrize("obias, hbias", [(BIAS, 0), (0, BIAS), (BIAS, BIAS)])
def test_lids_of_two_to_the_31_and_more(obias, hbias):
    three(UA.DT_F64, 0, 3, seed=31, obias=obias, hbias=hbias)
    three(UA.DT_I32, 2, 2, seed=32, obias=obias, hbias=hbias, sourced=(True, False, True))
    three(UA.DT_F32, 1, 2, seed=33, obias=obias, hbias=hbias, zero_halos=False)


@pytest.mark.parametrize("code", [UA.DT_F32, UA.DT_F64], ids=lambda c: UA.NAMES[c])
def test_a_cell_with_287_halo_copies_is_the_left_to_right_sum(code):
    dt = UA.NP[code]
    (info, after, before), (contrib, sources) = three(code, 0, 1, seed=41)
    lid = int(contrib[0].lids[0])
    at = [i for i, l in enumerate(contrib[0].lids) if l == lid]
    assert len(at) == 287 and info["max_per_dest"] == 287          # many trips of four loads
    halo = before[sources[0].slot][sources[0].lids[at]]
    acc = before[0][lid]
    for v in halo:
        acc = dt.type(acc + v)
    assert after[0][lid] == acc
    by_size = dt.type(before[0][lid])
    for v in sorted(halo, key=abs):
        by_size = dt.type(by_size + v)
    pair = list(halo)
    while len(pair) > 1:
        pair = [dt.type(pair[i] + pair[i + 1]) if i + 1 < len(pair) else pair[i] for i in range(0, len(pair), 2)]
    assert acc != by_size and acc != dt.type(before[0][lid] + pair[0])   # the order is what is pinned


@pytest.mark.parametrize("code, big", [(UA.DT_F32, 2.0 ** 24), (UA.DT_F64, 2.0 ** 53)], ids=["f32", "f64"])
def test_a_sourced_entry_before_a_buffer_entry(code, big):
    """One cell fed by a sourced entry (0) and a buffer entry (1): ((cell + halo) + buffer), which
    differs in the last bit from ((cell + buffer) + halo)."""
    dt = UA.NP[code]
    d = udesc(dt.itemsize, 1, n_cells=16)
    cell, halo, buf = dt.type(big), dt.type(1.0), dt.type(-big)
    want, other = dt.type(dt.type(cell + halo) + buf), dt.type(dt.type(cell + buf) + halo)
    assert want != other and (want, other) == (0.0, 1.0)
    src = Side(d, 1, np.array([7]))
    _, after, _ = run_get([Side(d, 0, np.array([5])), Side(d, 0, np.array([5]))], [src, Side(d, 1, np.array([9]))],
                          [(0, 0), (0, 0)], [src, None], [code] * 2, values={0: {5: cell}, 1: {7: halo}},
                          messages={1: [[buf]]}, seed=51, n_cells=16)
    assert after[0][5] == want and after[1][7] == 0 and after[1][9] == 0
    # the entries swapped: the buffer entry first
    _, after, _ = run_get([Side(d, 0, np.array([5])), Side(d, 0, np.array([5]))], [src, Side(d, 1, np.array([9]))],
                          [(0, 0), (0, 0)], [None, src], [code] * 2, values={0: {5: cell}, 1: {7: halo}},
                          messages={0: [[buf]]}, seed=52, n_cells=16)
    assert after[0][5] == other


def test_integer_sums_wrap():
    d = udesc(4, 1, n_cells=16)
    src = Side(d, 1, np.array([1, 2, 3]))
    _, after, _ = run_get([Side(d, 0, np.array([5, 5, 9]))], [src], [(0, 0)], [src], [UA.DT_I32],
                          values={0: {5: 0xFFFFFFF0, 9: 0}, 1: {1: 0x20, 2: 0x7FFFFFFF, 3: 0x10}}, seed=61, n_cells=16)
    assert after[0][5] == (0xFFFFFFF0 + 0x20 + 0x7FFFFFFF) % 2 ** 32 and after[0][9] == 0x10
    d = udesc(8, 1, n_cells=16)
    src = Side(d, 1, np.array([1, 2]))
    _, after, _ = run_get([Side(d, 0, np.array([5, 5]))], [src], [(0, 0)], [src], [UA.DT_I64],
                          values={0: {5: 2 ** 63 - 1}, 1: {1: 1, 2: 2 ** 63}}, seed=62, n_cells=16)
    assert after[0][5] == 0


@pytest.mark.parametrize("knobs", [{"grid_cap": 1}, {"grid_cap": 3}, {"u_tile_rows": 1}, {"u_tile_rows": 3}],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_grid_cap_and_tile_rows_stay_bit_exact(knobs):
    from ghex_amd import _ghx
    for k, v in knobs.items():
        _ghx.call("ghx_tune", k.encode(), v)
    rows = knobs.get("u_tile_rows", 512)
    for code, mode, levels, sourced in ((UA.DT_F64, 0, 3, (True, True, True)), (UA.DT_F32, 2, 3, (True, False, True))):
        (info, _, _), _ = three(code, mode, levels, seed=70 + mode, sourced=sourced)
        n0, n1 = 3001 - 286, 6005 - 1                    # destinations of the two owner slots
        nz = 0 if all(sourced) else 3002                 # the unsourced zero entry keeps its tiles
        assert info["n_tiles"] == -(-n0 // rows) - (-n1 // rows) + -(-nz // rows)


def test_mixed_dtypes_layouts_sources_and_shared_buffers_in_one_launch():
    rng = np.random.default_rng(80)
    own, halo = UC.draw_lists(rng, (700, 800, 900, 1000)), UC.draw_lists(rng, (700, 800, 900, 1000))
    ds = [udesc(8, 3), udesc(4, 2, first=False), udesc(4, 8, index_stride=9), udesc(8, 1)]
    hs = [udesc(8, 3, first=False), udesc(4, 2, index_stride=3), udesc(4, 8, index_stride=9), udesc(8, 1, index_stride=2)]
    codes = [UA.DT_F64, UA.DT_F32, UA.DT_I32, UA.DT_I64]
    contrib = [Side(d, k, own[k]) for k, d in enumerate(ds)]
    zero = [Side(d, 4 + k, halo[k]) for k, d in enumerate(hs)]
    sources = [zero[0], None, zero[2], None]             # two from the halos, two from buffer 0
    places, at = [], 0
    for s in contrib:
        places.append((0, at))
        at += (US.message_bytes(s) + 7) // 8 * 8 + 8
    info, _, _ = run_get(contrib, zero, places, sources, codes, seed=80)
    assert info["bytes"] == US.message_bytes(contrib[1]) + US.message_bytes(contrib[3])
    assert info["n_zero_dest"] == 800 + 1000


def test_halo_cells_no_self_message_names_keep_their_values():
    """Peer messages' halos are zeroed by their zero tiles, sourced ones by the lanes, every other
    cell of a halo field keeps its bytes (the arenas are compared whole); without zero_halos every
    halo cell does."""
    for zh in (True, False):
        (info, after, before), (contrib, sources) = three(UA.DT_F64, 0, 2, seed=90, sourced=(True, False, True),
                                                          zero_halos=zh)
        named = np.zeros(before[3].size, dtype=bool)
        for s in (1, 2):
            named[UA.element_index(UG.three_lists(udesc(8, 2), udesc(8, 2), seed=90)[1][s]).reshape(-1)] = True
        np.testing.assert_array_equal(after[3][~named].view(np.uint8), before[3][~named].view(np.uint8))
        assert (~named).sum() > 0 and ((after[3][named] == 0).all() if zh else (after[3] == before[3]).all())


# ---------------------------------------------------------------------------------------------
# product path
# ---------------------------------------------------------------------------------------------
TORCH = {"f64": np.float64, "f32": np.float32, "i32": np.int32, "i64": np.int64}


def _one_rank(golden_dir, levels, first, dtype, **options):
    from ghex_amd import unstructured as U
    from tests.test_gpu_uput import _known_answer
    ctx, pc, bis, fields = _known_answer(golden_dir, levels, first, dtype=dtype)
    return U.make_communication_object(ctx, **options), bis, fields


def _two_ranks(golden_dir, levels, first, dtype, **options):
    """The known-answer case as two emulated ranks of two domains each (tests/test_gpu_uaccum.py's
    _emulated_ranks with the objects' options)."""
    from ghex_amd import unstructured as U
    from tests.gpu_util import FakeContext
    from tests.test_gpu_uaccum import _emulated_ranks
    case, _, bis_all, fields = _emulated_ranks(golden_dir, levels, first, dtype)
    table = {0: [], 1: []}
    return [U.make_communication_object(FakeContext(r, 2, table), **options) for r in range(2)], bis_all, fields


def _same_bytes(a, b):
    """Two device tensors of one shape hold the same bytes, element for element."""
    x, y = np.ascontiguousarray(a.cpu().numpy()), np.ascontiguousarray(b.cpu().numpy())
    return x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def _pattern_buffers(co, bis):
    """Every send and receive buffer of the plan filled with a byte pattern; returns the copies."""
    import torch
    plan = co.plan(bis)
    send, recv = co.buffers(plan, bis[0].field.device)
    keep = []
    for k, t in enumerate(list(send) + list(recv)):
        t.copy_(torch.arange(t.numel(), dtype=torch.int64, device=t.device).mul_(37).add_(k).to(torch.uint8))
    torch.cuda.synchronize()
    for t in list(send) + list(recv):
        keep.append(t.clone())
    return plan, send, recv, keep


@pytest.mark.parametrize("dtype", ["f64", "i32"])
@pytest.mark.parametrize("levels, first", [(1, True), (3, True), (1, False), (3, False)])
def test_fused_equals_unfused_on_one_rank(golden_dir, levels, first, dtype):
    import torch
    from tests.test_gpu_uaccum import _check, _golden, _load_adjoint_state
    case = _golden(golden_dir)
    fused, fb, ff = _one_rank(golden_dir, levels, first, TORCH[dtype], fuse_adjoint_lists=True)
    plain, pb, pf = _one_rank(golden_dir, levels, first, TORCH[dtype])
    plan, send, recv, keep = _pattern_buffers(fused, fb)
    for zh in (True, False):
        wants = _load_adjoint_state(case, ff, scale=3 if zh else 5)
        _load_adjoint_state(case, pf, scale=3 if zh else 5)
        fused.adjoint_exchange(fb, zero_halos=zh).wait()
        plain.adjoint_exchange(pb, zero_halos=zh).wait()
        assert fused.plan(fb)._adjoint_prefix == "ghx_uexchange_adjoint_self_"
        assert plain.plan(pb)._adjoint_prefix == "ghx_uexchange_adjoint_"
        for (_, a, _, _), (_, b, _, _) in zip(ff, pf):
            assert _same_bytes(a, b)
        if zh:
            _check(ff, wants)                                          # and the known answer
    assert UG.self_info(plan.h)[0] == 1
    # the buffers of self messages - here all of them - are neither written nor read
    for t, k in zip(list(send) + list(recv), keep):
        assert torch.equal(t, k)


@pytest.mark.parametrize("dtype", ["f64", "i32"])
@pytest.mark.parametrize("levels, first", [(1, True), (3, True), (1, False), (3, False)])
def test_fused_equals_unfused_as_two_emulated_ranks(golden_dir, levels, first, dtype):
    import torch
    from tests.test_gpu_uaccum import _check, _golden, _load_adjoint_state, emulated_adjoint
    case = _golden(golden_dir)
    fcos, fb, ff = _two_ranks(golden_dir, levels, first, TORCH[dtype], fuse_adjoint_lists=True)
    pcos, pb, pf = _two_ranks(golden_dir, levels, first, TORCH[dtype])
    kept = [_pattern_buffers(co, bis) for co, bis in zip(fcos, fb)]
    wants = _load_adjoint_state(case, ff)
    _load_adjoint_state(case, pf)
    assert emulated_adjoint(fcos, fb) == 8 and emulated_adjoint(pcos, pb) == 8   # four peer messages each way
    for (_, a, _, _), (_, b, _, _) in zip(ff, pf):
        assert _same_bytes(a, b)
    _check(ff, wants)
    for rank, (plan, send, recv, keep) in enumerate(kept):
        assert UG.self_info(plan.h)[0] == 2 and plan._adjoint_prefix == "ghx_uexchange_adjoint_self_"
        infos = list(plan.send) + list(plan.recv)
        n_self = 0
        for t, k, x in zip(list(send) + list(recv), keep, infos):
            if x["rank"] == rank:                                       # a self message's buffer
                assert torch.equal(t, k)
                n_self += 1
        assert n_self > 0


def test_transpose_identity_against_the_forward_exchange(golden_dir):
    """<E x, y> = <x, E^T y> with integer fields: E is exchange(), E^T the fused adjoint_exchange()."""
    import torch
    for levels, first in ((3, True), (2, False)):
        co, bis, fields = _one_rank(golden_dir, levels, first, np.int64, fuse_adjoint_lists=True)
        rng = np.random.default_rng(5)
        for _ in range(2):
            x = [rng.integers(-50, 51, size=f[2].shape).astype(np.int64) for f in fields]
            y = [rng.integers(-50, 51, size=f[2].shape).astype(np.int64) for f in fields]
            out = []
            for state, op in ((x, co.exchange), (y, co.adjoint_exchange)):
                for (r, t, _, _), v in zip(fields, state):
                    t.copy_(torch.from_numpy(v))
                op(bis).wait()
                out.append([t.cpu().numpy().copy() for _, t, _, _ in fields])
            ex, ety = out
            lhs = sum(int((a * b).sum()) for a, b in zip(ex, y))
            rhs = sum(int((a * b).sum()) for a, b in zip(x, ety))
            assert lhs == rhs and any((a != b).any() for a, b in zip(ety, y))
        assert co.plan(bis)._adjoint_prefix == "ghx_uexchange_adjoint_self_"


def test_adjoint_twice_then_forward_on_one_object(golden_dir):
    from tests.test_gpu_uaccum import _check, _golden, _load_adjoint_state
    case = _golden(golden_dir)
    co, bis, fields = _one_rank(golden_dir, 3, True, np.float64, fuse_adjoint_lists=True)
    wants = _load_adjoint_state(case, fields)
    co.adjoint_exchange(bis).wait()
    _check(fields, wants)
    co.adjoint_exchange(bis).wait()                                # the halos are zero: nothing added
    _check(fields, wants)
    co.exchange(bis).wait()                                        # halos <- their owners' sums
    for r, _, _, _ in fields:
        for src, rl in case["recv_maps"][str(r)].items():
            for lid, sl in zip(rl, case["send_maps"][src][str(r)]):
                wants[r][lid] = wants[int(src)][sl]
    _check(fields, wants)


def test_all_self_form_replayed_from_a_capture(golden_dir):
    import torch
    from tests.test_gpu_uaccum import _check, _golden, _load_adjoint_state
    case = _golden(golden_dir)
    co, bis, fields = _one_rank(golden_dir, 3, True, np.float64, fuse_adjoint_lists=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    wants = _load_adjoint_state(case, fields)
    with torch.cuda.stream(side):
        co.adjoint_exchange(bis).wait()      # set-up and a warm run, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _check(fields, wants)
    assert UG.self_info(co.plan(bis).h)[0] == 1
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        co.adjoint_exchange(bis)
    for k in (3, 5):
        wants = _load_adjoint_state(case, fields, scale=k)
        g.replay()
        torch.cuda.synchronize()
        _check(fields, wants)


# draw_mesh draws halo gids from other domains' owned cells and outer cells are never sent, so no
# drawn mesh makes a halo cell of one message an owner cell of another: the device-less planner
# accepts all twenty seeds (checked on the CPU) and every one runs fused
MESH_SEEDS = tuple(range(20))


def test_random_meshes_fused_against_unfused():
    """Twenty seeded meshes of two to four domains on one rank (tests/uget_cases.draw_mesh), four
    integer-valued fields per domain set, one per dtype, in ONE adjoint exchange: the fused object
    against the unfused one on copies of the same fields, bit for bit. All twenty run fused."""
    import torch
    import ghex_amd
    from ghex_amd import unstructured as U
    ran = 0
    ctx = ghex_amd.make_context()
    for seed in MESH_SEEDS:
        doms = UG.draw_mesh(seed)
        rng = np.random.default_rng(seed + 99)
        levels, first = 1 + seed % 4, seed % 3 != 0
        dds = [U.DomainDescriptor(i, gids, outer) for i, gids, outer in doms]
        pc = U.make_pattern(ctx, U.HaloGenerator(), dds)
        sets = []
        for _ in range(2):
            bis, views = [], []
            for name, dt in TORCH.items():
                for dd, (i, gids, outer) in zip(dds, doms):
                    n = len(gids)
                    t = (torch.zeros((n, levels + 1), dtype=torch.from_numpy(np.zeros(1, dt)).dtype, device="cuda")[:, :levels]
                         if first else torch.zeros((levels, n), dtype=torch.from_numpy(np.zeros(1, dt)).dtype, device="cuda").t())
                    bis.append(pc(U.make_field_descriptor(dd, t)))
                    views.append(t)
            sets.append((bis, views))
        for v0, v1 in zip(sets[0][1], sets[1][1]):
            a = torch.from_numpy(rng.integers(-1000, 1001, size=tuple(v0.shape))).to(v0.dtype).cuda()
            v0.copy_(a)
            v1.copy_(a)
        fused = U.make_communication_object(ctx, fuse_adjoint_lists=True)
        plain = U.make_communication_object(ctx)
        fused.adjoint_exchange(sets[0][0]).wait()
        assert fused.plan(sets[0][0])._adjoint_prefix == "ghx_uexchange_adjoint_self_"
        plain.adjoint_exchange(sets[1][0]).wait()
        changed = False
        for v0, v1, (i, gids, outer) in zip(sets[0][1], sets[1][1], doms * len(TORCH)):
            assert torch.equal(v0, v1)
            assert (v0[outer] == 0).all()
            changed = changed or bool((v0 != 0).any())
        assert changed
        ran += 1
    assert ran == len(MESH_SEEDS) >= 15
