"""The adjoint halo exchange of unstructured fields on the device (ghx_uaccum_create, k_accum_u,
CommunicationObject.adjoint_exchange). Kernel cases through the ABI: every field and every buffer
in an arena of its own between 256-byte guard bands; after ONE execute every byte of every arena
is compared — owner fields with the NumPy definition (tests/uaccum_cases.py: adds in ascending
(entry, position)), halo fields hold exact zero rows (or are unchanged without zero_halos), buffers
are unchanged, guards still the sentinel. Product path: the known-answer case on one rank and as
two emulated ranks, forty random meshes, the transpose identity against the forward exchange(),
graph replay and the refusals. Every comparison is bit-exact.

Float inputs other than the order pins are drawn with magnitudes in [2^-20, 2^20] or are
integer-valued: no result is subnormal, inf or NaN (those are not part of the contract)."""
import json
import os

import numpy as np
import pytest

from tests import uaccum_cases as UA
from tests import uput_cases as UC
from tests import uself_cases as US
from tests.uput_cases import N_CELLS, Side, udesc
from tests.test_gpu_uput import BIAS, GUARD, SENTINEL, Arena, _known_answer

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


def _fill(arena, at, values):
    """Typed values into an arena's host image and device memory from field byte `at` on."""
    import torch
    raw = np.ascontiguousarray(values).reshape(-1).view(np.uint8)
    arena.host[arena.at + at:arena.at + at + raw.size] = raw
    arena.view.copy_(torch.from_numpy(arena.host))


def run_accum(contrib, zero, places, dtypes, oshift=0, hshift=0, bshift=0, obias=0, hbias=0,
              zero_halos=True, seed=0, cell=None, messages=None):
    """contrib[e] / zero[e]: the owner and the halo Side of message e (dtype code dtypes[e], buffer
    place places[e]). One plan, one execute, every arena compared byte for byte. oshift / hshift /
    bshift move the owner fields, the halo fields and the buffers by that many bytes; obias /
    hbias add to that side's lids (an int64 table) and move its pointers back. cell: the value of
    every owner element; messages[e]: the (n, levels) contributions of entry e (default: drawn)."""
    import torch
    from ghex_amd import _ghx
    rng = np.random.default_rng(3000 + seed)
    nf = 1 + max(s.slot for s in list(contrib) + list(zero))
    nb = 1 + max(p[0] for p in places)
    code_of, desc_of, owners = {}, {}, {s.slot for s in contrib}
    for s, c in list(zip(contrib, dtypes)) + list(zip(zero, dtypes)):
        code_of[s.slot], desc_of[s.slot] = c, s.desc
    fields, back = [None] * nf, [0] * nf
    for k, d in desc_of.items():
        span = UC.span_bytes(d)
        fields[k] = Arena(span, oshift if k in owners else hshift)
        v = UA.draw_values(rng, span // d.elem_size, code_of[k])
        if cell is not None and k in owners:
            v[:] = cell
        _fill(fields[k], 0, v)
        back[k] = (obias if k in owners else hbias) * d.index_stride * d.elem_size
    ends = [0] * nb
    for s, (b, off) in zip(contrib, places):
        ends[b] = max(ends[b], off + US.message_bytes(s))
    bufs = [Arena(e, bshift) if e else None for e in ends]
    for e, (s, (b, off)) in enumerate(zip(contrib, places)):
        d, n = s.desc, s.lids.size
        m = (UA.draw_values(rng, n * d.levels, dtypes[e]).reshape(n, d.levels) if messages is None
             else np.asarray(messages[e], dtype=UA.NP[dtypes[e]]).reshape(n, d.levels))
        _fill(bufs[b], off, m if d.levels_first else m.T)
    plan_c = [Side(s.desc, s.slot, s.lids + obias) for s in contrib]
    plan_z = [Side(s.desc, s.slot, s.lids + hbias) for s in zero]
    h = UA.create(plan_c, dtypes, places, plan_z)
    try:
        fp = _ghx.ptr_array([(a.ptr - bk) if a else 0 for a, bk in zip(fields, back)])
        bp = _ghx.ptr_array([a.ptr if a else 0 for a in bufs])
        info = UA.info(h)
        _ghx.call("ghx_uaccum_execute", h, fp, nf, bp, nb, 1 if zero_halos else 0,
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        UA.destroy(h)
    # the definition on typed copies of the host images
    typed = {k: fields[k].field()[:UC.span_bytes(d)].copy().view(UA.NP[code_of[k]]) for k, d in desc_of.items()}
    images = [a.field() if a else None for a in bufs]
    UA.definition(typed, images, contrib, dtypes, places, zero, zero_halos)
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
        elif cell is None:
            assert changed > 0
    for a in bufs:
        if a is not None:
            np.testing.assert_array_equal(a.device_bytes(), a.host)   # read only, guards included
    for z in zero:                                                    # exact zero rows
        rows = typed[z.slot][UA.element_index(z)]
        assert (rows.view(np.uint8) == 0).all() == bool(zero_halos)
    return info, typed


def _descs(mode, e, levels):
    """Owner and halo descriptor of a row mode: 0 contiguous levels, 1 levels-first messages over
    strided levels, 2 levels last."""
    if mode == 0:
        return udesc(e, levels), udesc(e, levels)
    if mode == 1:
        return udesc(e, levels, index_stride=1, level_stride=N_CELLS), udesc(e, levels, index_stride=1,
                                                                            level_stride=N_CELLS + 3)
    return udesc(e, levels, first=False), udesc(e, levels, first=False, level_stride=N_CELLS + 16 // e)


def three(code, mode=0, levels=3, seed=0, repeats=True, descs=None, boff=0, **kw):
    e = UA.NP[code].itemsize
    od, hd = descs or _descs(mode, e, levels)
    contrib, zero, places = UA.three_lists_case(od, hd, seed=seed, repeats=repeats, boff=boff)
    return run_accum(contrib, zero, places, [code] * 3, seed=seed, **kw)


# ---------------------------------------------------------------------------------------------
# kernel cases
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 3, 8])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("code", UA.DTYPES, ids=lambda c: UA.NAMES[c])
def test_every_dtype_row_mode_and_level_count(code, mode, levels):
    info, _ = three(code, mode, levels, seed=code * 100 + mode * 10 + levels)
    assert info["max_per_dest"] == 287 and info["n_contrib"] == 9006
    assert info["n_tiles"] > 8                       # several tiles per slot, the last partial


@pytest.mark.parametrize("code", UA.DTYPES, ids=lambda c: UA.NAMES[c])
def test_padded_index_and_level_strides(code):
    e = UA.NP[code].itemsize
    three(code, seed=11, descs=(udesc(e, 3, index_stride=5), udesc(e, 3, index_stride=4)))
    three(code, seed=12, descs=(udesc(e, 2, index_stride=4, level_stride=2), udesc(e, 2, index_stride=6, level_stride=3)))
    three(code, seed=13, descs=(udesc(e, 3, first=False, level_stride=N_CELLS + 5),
                                udesc(e, 3, first=False, level_stride=N_CELLS + 1)))


@pytest.mark.parametrize("code", UA.DTYPES, ids=lambda c: UA.NAMES[c])
def test_pointers_and_buffer_offset_aligned_to_the_element_only(code):
    e = UA.NP[code].itemsize
    three(code, 0, 3, seed=21, oshift=e, hshift=e, bshift=e)
    three(code, 2, 3, seed=22, oshift=e, bshift=e, boff=e)
    three(code, 1, 1, seed=23, hshift=e, boff=3 * e)


@pytest.mark.parametrize("obias, hbias", [(BIAS, 0), (0, BIAS), (BIAS, BIAS)])
def test_int64_lid_tables(obias, hbias):
    three(UA.DT_F64, 0, 3, seed=31, obias=obias, hbias=hbias)
    three(UA.DT_I32, 2, 2, seed=32, obias=obias, hbias=hbias)


def test_without_zero_halos_the_halo_fields_are_untouched():
    for code, mode in ((UA.DT_F32, 0), (UA.DT_I64, 2)):
        three(code, mode, 3, seed=41, zero_halos=False)


def test_lists_without_repeats_and_a_cell_in_two_messages():
    info, _ = three(UA.DT_F64, 0, 3, seed=51, repeats=False)
    assert info["max_per_dest"] == 1
    # one owner cell in three messages of three buffers, and twice in one of them
    d = udesc(4, 2)
    rng = np.random.default_rng(52)
    a, b, c = UC.draw_lists(rng, (100, 100, 100))
    b[7] = a[3]
    c[50], c[99] = a[3], a[3]
    t = UC.draw_lists(rng, (100, 100, 100))
    info, _ = run_accum([Side(d, 0, a), Side(d, 0, b), Side(d, 0, c)], [Side(d, 1, x) for x in t],
                        [(0, 0), (1, 8), (2, 0)], [UA.DT_F32] * 3, seed=52)
    assert info["max_per_dest"] == 4


def _pin(code, big):
    """One owner cell, contributions (big, 1, -big) in that record order — once as three positions
    of one entry, once as three entries — onto 0: the result depends on the order of the adds."""
    dt = UA.NP[code]
    e = dt.itemsize
    d = udesc(e, 1, n_cells=16)
    vals = [big, 1.0, -big]
    want = dt.type(0)
    for v in vals:
        want = dt.type(want + dt.type(v))
    other = dt.type(dt.type(dt.type(0) + dt.type(big)) + dt.type(-big)) + dt.type(1.0)
    assert want != other                                      # the order matters
    lid = np.array([5, 5, 5])
    _, typed = run_accum([Side(d, 0, lid)], [Side(d, 1, np.array([1, 2, 3]))], [(0, 0)], [code], cell=0,
                         messages=[np.array(vals)[:, None]], seed=61)
    assert typed[0][5] == want
    one = [Side(d, 0, np.array([5])) for _ in range(3)]
    _, typed = run_accum(one, [Side(d, 1, np.array([k])) for k in range(3)], [(0, 0), (1, 0), (2, 0)],
                         [code] * 3, cell=0, messages=[np.array([[v]]) for v in vals], seed=62)
    assert typed[0][5] == want
    # the entry index decides, not the buffer: buffers permuted, the same result; the second and
    # third entries' values swapped, the other one
    _, typed = run_accum(one, [Side(d, 1, np.array([k])) for k in range(3)], [(2, 0), (0, 0), (1, 0)],
                         [code] * 3, cell=0, messages=[np.array([[v]]) for v in vals], seed=63)
    assert typed[0][5] == want
    _, typed = run_accum(one, [Side(d, 1, np.array([k])) for k in range(3)], [(0, 0), (1, 0), (2, 0)],
                         [code] * 3, cell=0, messages=[np.array([[v]]) for v in (big, -big, 1.0)], seed=63)
    assert typed[0][5] == other


def test_order_pin_f64():
    _pin(UA.DT_F64, 1e16)


def test_order_pin_f32():
    _pin(UA.DT_F32, 1e8)


def test_order_over_more_than_one_batch_of_loads():
    """Nine contributions whose partial sums all round differently in another order."""
    d = udesc(8, 1, n_cells=16)
    vals = np.array([1e16, 3.0, -1e16, 1.0, 2.0 ** 60, 5.0, -(2.0 ** 60), 7.0, 0.5])
    _, typed = run_accum([Side(d, 0, np.full(9, 2))], [Side(d, 1, np.arange(9))], [(0, 0)], [UA.DT_F64],
                         cell=0.25, messages=[vals[:, None]], seed=64)
    want, back = np.float64(0.25), np.float64(0.25)
    for v in vals:
        want = want + v
    for v in vals[::-1]:
        back = back + v
    assert typed[0][2] == want and want != back


def test_integer_sums_wrap():
    d = udesc(4, 1, n_cells=16)
    _, typed = run_accum([Side(d, 0, np.array([5, 5, 9]))], [Side(d, 1, np.array([1, 2, 3]))], [(0, 0)],
                         [UA.DT_I32], cell=0xFFFFFFF0, messages=[np.array([[0x20], [0x7FFFFFFF], [0x10]])], seed=65)
    assert typed[0][5] == (0xFFFFFFF0 + 0x20 + 0x7FFFFFFF) % 2 ** 32 and typed[0][9] == 0
    assert np.int32(typed[0][5:6].view(np.int32)[0]) == np.int32(0x8000000F - 2 ** 32)
    d = udesc(8, 1, n_cells=16)
    _, typed = run_accum([Side(d, 0, np.array([5, 5]))], [Side(d, 1, np.array([1, 2]))], [(0, 0)],
                         [UA.DT_I64], cell=2 ** 63 - 1, messages=[np.array([[1], [2 ** 63]], dtype=np.uint64)], seed=66)
    assert typed[0][5] == 0


@pytest.mark.parametrize("knobs", [{"grid_cap": 1}, {"grid_cap": 3}, {"u_tile_rows": 1}, {"u_tile_rows": 3},
                                   {"u_tile_rows": 5000}, {"u_tile_rows": 3, "grid_cap": 3}],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_grid_cap_and_tile_rows_stay_bit_exact(knobs):
    from ghex_amd import _ghx
    for k, v in knobs.items():
        _ghx.call("ghx_tune", k.encode(), v)
    rows = knobs.get("u_tile_rows", 512)
    for code, mode, levels in ((UA.DT_F64, 0, 3), (UA.DT_F32, 2, 3), (UA.DT_I32, 1, 8)):
        info, _ = three(code, mode, levels, seed=70 + mode)
        n0, n1 = 3001 - 286, 6005 - 1                    # destinations of the two owner slots
        assert info["n_tiles"] == -(-n0 // rows) - (-n1 // rows) + -(-3001 // rows) - (-6005 // rows)
    three(UA.DT_I64, 0, 1, seed=74, zero_halos=False)


def test_mixed_dtypes_layouts_and_shared_buffers_in_one_launch():
    rng = np.random.default_rng(80)
    own, halo = UC.draw_lists(rng, (700, 800, 900, 1000)), UC.draw_lists(rng, (700, 800, 900, 1000))
    ds = [udesc(8, 3), udesc(4, 2, first=False), udesc(4, 8, index_stride=9), udesc(8, 1)]
    codes = [UA.DT_F64, UA.DT_F32, UA.DT_I32, UA.DT_I64]
    contrib = [Side(d, k, own[k]) for k, d in enumerate(ds)]
    zero = [Side(d, 4 + k, halo[k]) for k, d in enumerate(ds)]
    places, at = [], 0
    for s in contrib:                                    # all four messages in buffer 0
        places.append((0, at))
        at += (US.message_bytes(s) + 7) // 8 * 8 + 8
    run_accum(contrib, zero, places, codes, seed=80)


# ---------------------------------------------------------------------------------------------
# product path
# ---------------------------------------------------------------------------------------------
TORCH = {"f64": np.float64, "f32": np.float32, "i32": np.int32, "i64": np.int64}


def _golden(golden_dir):
    with open(os.path.join(golden_dir, "unstructured_case.json")) as fh:
        return json.load(fh)


def _halo_value(r, lid, levels):
    return np.array([7 + r * 3 + lid * 11 + l * 101 for l in range(levels)])


def _load_adjoint_state(case, fields, scale=1):
    """Owned cells as _known_answer writes them (times scale), halo cell lid of domain r
    _halo_value(r, lid) * scale. Returns the expectation worked out from the golden tables: every
    owner cell is its value plus the values of its halo copies, halos are zero."""
    import torch
    wants = []
    for r, t, init, _ in fields:
        levels = init.shape[1]
        a = init.copy()
        for lid in case["domains"][str(r)]["halo_lids"]:
            a[lid] = _halo_value(r, lid, levels)
        a = a * scale
        t.copy_(torch.from_numpy(a).to(t.device))
        wants.append(a.copy())
    for r, _, init, _ in fields:
        levels = init.shape[1]
        for dst, sl in case["send_maps"][str(r)].items():
            for lid, hl in zip(sl, case["recv_maps"][dst][str(r)]):
                wants[r][lid] += (_halo_value(int(dst), hl, levels) * scale).astype(init.dtype)
    for r, _, init, _ in fields:
        wants[r][case["domains"][str(r)]["halo_lids"]] = 0
    return wants


def _check(fields, wants):
    for (r, t, _, _), w in zip(fields, wants):
        got = np.ascontiguousarray(t.cpu().numpy())
        np.testing.assert_array_equal(got.view(np.uint8), np.ascontiguousarray(w).view(np.uint8))


@pytest.mark.parametrize("dtype", list(TORCH))
@pytest.mark.parametrize("levels, levels_first", [(1, True), (3, True), (1, False), (3, False)])
def test_known_answer_case_on_one_rank(golden_dir, levels, levels_first, dtype):
    from ghex_amd import unstructured as U
    case = _golden(golden_dir)
    ctx, pc, bis, fields = _known_answer(golden_dir, levels, levels_first, dtype=TORCH[dtype])
    co = U.make_communication_object(ctx)
    me = ctx.rank()
    assert all(x["rank"] == me for x in co.plan(bis).send)         # every message a self message
    wants = _load_adjoint_state(case, fields)
    co.adjoint_exchange(bis).wait()
    _check(fields, wants)
    # without zero_halos the halos keep their values (assembly)
    wants = _load_adjoint_state(case, fields, scale=2)
    for r, t, init, _ in fields:
        hl = case["domains"][str(r)]["halo_lids"]
        wants[r][hl] = t.cpu().numpy()[hl]
    co.adjoint_exchange(bis, zero_halos=False).wait()
    _check(fields, wants)


def _emulated_ranks(golden_dir, levels, levels_first, dtype):
    """The known-answer case as two emulated ranks of two domains each: per rank a communication
    object, its buffer infos and its fields (as _known_answer's)."""
    import torch
    from ghex_amd import unstructured as U
    from tests.gpu_util import FakeContext, unstructured_patterns
    case = _golden(golden_dir)
    doms = [(r, case["domains"][str(r)]["gids"], case["domains"][str(r)]["halo_lids"]) for r in range(4)]
    pats = unstructured_patterns([doms[:2], doms[2:]])
    table = {0: [], 1: []}
    cos, bis_all, fields = [], [], []
    for rank in range(2):
        dds, pc = pats[rank]
        bis = []
        for dd, (r, gids, halo) in zip(dds, doms[2 * rank:2 * rank + 2]):
            n = len(gids)
            init = np.full((n, levels), -1, dtype=dtype)
            for lid, gid in enumerate(gids):
                if lid not in halo:
                    init[lid] = [r * 10000 + gid * 100 + l for l in range(levels)]
            t = torch.from_numpy(init).cuda()
            if not levels_first:
                t = torch.empty_strided((n, levels), (1, n), dtype=t.dtype, device="cuda").copy_(t)
            bis.append(pc(U.make_field_descriptor(dd, t)))
            fields.append((r, t, init, None))
        cos.append(U.make_communication_object(FakeContext(rank, 2, table)))
        bis_all.append(bis)
    return case, cos, bis_all, fields


def emulated_adjoint(cos, bis_per_rank, zero_halos=True):
    """Reverse pack on every emulated rank, route as tests/gpu_util.emulated_exchange routes with
    the roles swapped (a rank's peer receive buffer goes into the sender's send buffer of the same
    domain pair), accumulate on every rank."""
    import torch
    plans, bufs = [], []
    for co, bis in zip(cos, bis_per_rank):
        plan, send, recv = co.adjoint_pack_only(bis)
        plans.append(plan)
        bufs.append((send, recv))
    moved = 0
    for r, plan in enumerate(plans):
        for i, x in enumerate(plan.recv):
            if x["rank"] == r:
                continue  # self message: the recv buffer is the send buffer
            src = x["rank"]
            j = next(j for j, s in enumerate(plans[src].send) if s["pair"] == x["pair"] and s["rank"] == r)
            assert plans[src].send[j]["tag"] == x["tag"] and plans[src].send[j]["size"] == x["size"]
            bufs[src][0][j][:x["size"]].copy_(bufs[r][1][i][:x["size"]])
            moved += 1
    for co, bis in zip(cos, bis_per_rank):
        co.adjoint_accumulate_only(bis, zero_halos=zero_halos)
    torch.cuda.synchronize()
    return moved


@pytest.mark.parametrize("dtype", ["f64", "i32"])
@pytest.mark.parametrize("levels, levels_first", [(1, True), (3, True), (3, False)])
def test_known_answer_case_as_two_emulated_ranks(golden_dir, levels, levels_first, dtype):
    case, cos, bis_all, fields = _emulated_ranks(golden_dir, levels, levels_first, TORCH[dtype])
    wants = _load_adjoint_state(case, fields)
    assert emulated_adjoint(cos, bis_all) == 8                     # four peer messages each way
    _check(fields, wants)


def test_mesh_census():
    """What the forty meshes hold (counted on the CPU): which seeds have halo cells at all, which
    an owner cell with two or more halo copies, and the most copies of one cell."""
    from tests.test_gpu_fuzz import draw_unstructured
    from tests.test_gpu_uself import NO_HALO_SEEDS
    halo, shared, most = [], [], 0
    for seed in range(40):
        copies = {}
        for d in draw_unstructured(seed)["doms"]:
            for lid in d["outer"]:
                copies[d["gids"][lid]] = copies.get(d["gids"][lid], 0) + 1
        if copies:
            halo.append(seed)
            most = max(most, max(copies.values()))
            if max(copies.values()) >= 2:
                shared.append(seed)
    assert sorted(set(range(40)) - set(halo)) == sorted(NO_HALO_SEEDS)
    assert (len(halo), len(shared), most) == (35, 32, 4) and len(shared) >= 30


@pytest.mark.parametrize("seed", range(40))
def test_random_meshes_against_the_definition(seed):
    """Four integer-valued fields, one per dtype, in ONE adjoint exchange: every owner cell ends
    as its value plus the values of every halo cell of its gid, every halo cell as zero. Odd seeds
    hold every domain on one rank (adjoint_exchange), even seeds keep the drawn ranks (emulated)."""
    import torch
    from ghex_amd import unstructured as U
    from tests.gpu_util import FakeContext, unstructured_patterns
    from tests.test_gpu_fuzz import draw_unstructured
    from tests.test_gpu_uself import NO_HALO_SEEDS
    case = draw_unstructured(seed)
    if seed in NO_HALO_SEEDS:
        pytest.skip("the mesh draws no halo cell: nothing to exchange")
    one_rank = seed % 2 == 1
    nr = 1 if one_rank else case["nr"]
    rank_of = (lambda d: 0) if one_rank else (lambda d: d["rank"])
    f0 = case["fields"][0]
    L, first, pad = f0["levels"], f0["first"], f0["pad"]
    rng = np.random.default_rng(seed + 99)
    pats = unstructured_patterns([[(d["id"], d["gids"], d["outer"]) for d in case["doms"] if rank_of(d) == r]
                                  for r in range(nr)])
    table = {r: [] for r in range(nr)}
    cos, bis_all, recs = [], [], []
    for r in range(nr):
        dds, pc = pats[r]
        mine = [d for d in case["doms"] if rank_of(d) == r]
        bis = []
        for name, dt in TORCH.items():
            for dd, d in zip(dds, mine):
                n = len(d["gids"])
                a = rng.integers(-1000, 1001, size=(n, L)).astype(dt)
                if first:
                    t = torch.zeros((n, L + pad), dtype=torch.from_numpy(a).dtype, device="cuda")
                    view = t[:, :L]
                else:
                    t = torch.zeros((L, n), dtype=torch.from_numpy(a).dtype, device="cuda")
                    view = t.t()
                view.copy_(torch.from_numpy(a))
                bis.append(pc(U.make_field_descriptor(dd, view)))
                recs.append((name, d, view, a))
        cos.append(U.make_communication_object(FakeContext(r, nr, table)))
        bis_all.append(bis)
    if one_rank:
        cos[0].adjoint_exchange(bis_all[0]).wait()
    else:
        emulated_adjoint(cos, bis_all)
    for name in TORCH:
        mine = [(d, view, a) for n_, d, view, a in recs if n_ == name]
        total = {}
        for d, view, a in mine:
            for lid in d["outer"]:
                g = d["gids"][lid]
                total[g] = total.get(g, 0) + a[lid]
        for d, view, a in mine:
            want, outer = a.copy(), set(d["outer"])
            for lid, g in enumerate(d["gids"]):
                want[lid] = 0 if lid in outer else a[lid] + total.get(g, 0)
            np.testing.assert_array_equal(view.cpu().numpy(), want)
        assert total


def test_transpose_identity_against_the_forward_exchange(golden_dir):
    """<E x, y> = <x, E^T y> with integer-valued f64: E is exchange(), E^T adjoint_exchange()."""
    import torch
    from ghex_amd import unstructured as U
    for levels, first in ((3, True), (2, False)):
        ctx, pc, bis, fields = _known_answer(golden_dir, levels, first)
        co = U.make_communication_object(ctx)
        rng = np.random.default_rng(5)
        for _ in range(2):
            x = [rng.integers(-50, 51, size=f[2].shape).astype(np.float64) for f in fields]
            y = [rng.integers(-50, 51, size=f[2].shape).astype(np.float64) for f in fields]
            out = []
            for state, op in ((x, co.exchange), (y, co.adjoint_exchange)):
                for (r, t, _, _), v in zip(fields, state):
                    t.copy_(torch.from_numpy(v))
                op(bis).wait()
                out.append([t.cpu().numpy().copy() for _, t, _, _ in fields])
            ex, ety = out
            lhs = sum(float((a * b).sum()) for a, b in zip(ex, y))
            rhs = sum(float((a * b).sum()) for a, b in zip(x, ety))
            assert lhs == rhs and any((a != b).any() for a, b in zip(ety, y))


def test_adjoint_twice_then_forward_on_one_object(golden_dir):
    from ghex_amd import unstructured as U
    case = _golden(golden_dir)
    ctx, pc, bis, fields = _known_answer(golden_dir, 3, True)
    co = U.make_communication_object(ctx)
    wants = _load_adjoint_state(case, fields)
    h = co.adjoint_exchange(bis)
    with pytest.raises(RuntimeError, match="not finished"):
        co.adjoint_exchange(bis)                                   # _start's in-flight rule
    h.wait()
    _check(fields, wants)
    co.adjoint_exchange(bis).wait()                                # the halos are zero: nothing added
    _check(fields, wants)
    co.exchange(bis).wait()                                        # halos <- their owners' sums
    for r, _, _, _ in fields:
        for src, rl in case["recv_maps"][str(r)].items():
            for lid, sl in zip(rl, case["send_maps"][src][str(r)]):
                wants[r][lid] = wants[int(src)][sl]
    _check(fields, wants)
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    wants = _load_adjoint_state(case, fields, scale=3)
    torch.cuda.synchronize()
    h = co.schedule_adjoint_exchange(side, bis)
    h.schedule_wait(None)
    h.wait()
    _check(fields, wants)


def test_all_self_adjoint_replayed_from_a_capture(golden_dir):
    import torch
    from ghex_amd import unstructured as U
    case = _golden(golden_dir)
    ctx, pc, bis, fields = _known_answer(golden_dir, 3, True)
    co = U.make_communication_object(ctx)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    wants = _load_adjoint_state(case, fields)
    with torch.cuda.stream(side):
        co.adjoint_exchange(bis).wait()      # set-up and a warm run, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _check(fields, wants)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        co.adjoint_exchange(bis)
    for k in (3, 5):
        wants = _load_adjoint_state(case, fields, scale=k)
        g.replay()
        torch.cuda.synchronize()
        _check(fields, wants)


def test_refusals_of_the_python_interface(golden_dir):
    import torch
    import ghex_amd
    from ghex_amd import unstructured as U
    from ghex_amd.structured import regular as R
    ctx, pc, bis, fields = _known_answer(golden_dir, 1, True)
    for kw in (dict(direct=True), dict(pipelined=True)):
        co = U.make_communication_object(ctx, **kw)
        with pytest.raises(ValueError, match="plain communication object"):
            co.adjoint_exchange(bis)
        with pytest.raises(ValueError, match="plain communication object"):
            co.adjoint_pack_only(bis)
    co = U.make_communication_object(ctx)
    for dt in (torch.float16, torch.bfloat16, torch.uint8, torch.bool, torch.int16):
        dd = U.DomainDescriptor(0, _golden(golden_dir)["domains"]["0"]["gids"],
                                _golden(golden_dir)["domains"]["0"]["halo_lids"])
        t = torch.zeros(dd.size(), dtype=dt, device="cuda")
        with pytest.raises(TypeError, match="not supported"):
            co.adjoint_exchange([pc(U.make_field_descriptor(dd, t))])
    N, Hw = 6, 1
    E = N + 2 * Hw
    sdd = R.DomainDescriptor(0, (0, 0, 0), (N - 1,) * 3)
    spc = R.make_pattern(ctx, R.HaloGenerator((0, 0, 0), (N - 1,) * 3, (Hw,) * 6, (True,) * 3), [sdd])
    sf = R.make_field_descriptor(sdd, torch.zeros((E, E, E), dtype=torch.float64, device="cuda"), (Hw,) * 3,
                                 (E,) * 3)
    with pytest.raises(ValueError, match="unstructured fields only"):
        co.adjoint_exchange([spc(sf)])
    with pytest.raises(ValueError, match="unstructured fields only"):
        co.adjoint_exchange(bis + [spc(sf)])
    co.adjoint_exchange(bis).wait()          # the object is still usable
