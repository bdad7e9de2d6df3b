"""Index-list puts on the device (ghx_uput_create, k_put_u) and the bulk object over unstructured
fields. Kernel cases through the ABI: source and target fields in separate arenas with 256-byte
guard bands, every byte of both arenas compared with the NumPy form of the put's definition
(tests/uput_cases.py) after ONE execute. Product path: emulated ranks planned as the bulk object
plans them, against the halo property and the buffered exchange; the real object on one rank
(known-answer case), also next to a structured field, and replayed from a captured graph.
Every comparison is bit-exact."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import uput_cases as UC
from tests.uput_cases import N_CELLS, Side, udesc

pytestmark = pytest.mark.gpu

GUARD = 256
SENTINEL = 0xC3
BIAS = 1 << 31   # added to the lids of an int64 table; the field pointer is moved back by it


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ghex_amd
    ghex_amd.native_library()


class Arena:
    """A field in device memory between two guard bands: the allocation's base is 256-byte
    aligned, the field starts `shift` bytes after the first guard. Source arenas hold random
    bytes, target arenas the sentinel."""

    def __init__(self, span, shift, rng=None):
        import torch
        total = GUARD + shift + span + GUARD
        self.raw = torch.empty(total + 256, dtype=torch.uint8, device="cuda")
        off = (-self.raw.data_ptr()) % 256
        self.view = self.raw[off:off + total]
        assert self.view.data_ptr() % 256 == 0
        self.host = (rng.integers(0, 256, size=total, dtype=np.uint8) if rng is not None
                     else np.full(total, SENTINEL, dtype=np.uint8))
        self.view.copy_(torch.from_numpy(self.host))
        self.at = GUARD + shift
        self.ptr = self.view.data_ptr() + self.at

    def field(self):
        """The host image from the field's first byte on."""
        return self.host[self.at:]

    def device_bytes(self):
        return self.view.cpu().numpy()


def run_messages(msgs, sshift=0, dshift=0, sbias=0, dbias=0, seed=0):
    """msgs: [(source desc, target desc, source slot, target slot, source lids, target lids)].
    One plan, one execute; both arenas of every slot compared byte for byte."""
    import torch
    from ghex_amd import _ghx
    rng = np.random.default_rng(1000 + seed)
    ns = 1 + max(m[2] for m in msgs)
    nd = 1 + max(m[3] for m in msgs)
    sspan = [max(UC.span_bytes(m[0]) for m in msgs if m[2] == k) for k in range(ns)]
    dspan = [max(UC.span_bytes(m[1]) for m in msgs if m[3] == k) for k in range(nd)]
    src = [Arena(sp, sshift, rng) for sp in sspan]
    dst = [Arena(sp, dshift) for sp in dspan]
    srcs = [Side(m[0], m[2], np.asarray(m[4]) + sbias) for m in msgs]
    dsts = [Side(m[1], m[3], np.asarray(m[5]) + dbias) for m in msgs]
    h = UC.create(srcs, dsts)
    try:
        # a biased table addresses the same cells from a pointer moved back by the bias
        sback = [sbias * next(m[0] for m in msgs if m[2] == k).index_stride *
                 next(m[0] for m in msgs if m[2] == k).elem_size for k in range(ns)]
        dback = [dbias * next(m[1] for m in msgs if m[3] == k).index_stride *
                 next(m[1] for m in msgs if m[3] == k).elem_size for k in range(nd)]
        sp = _ghx.ptr_array([a.ptr - b for a, b in zip(src, sback)])
        dp = _ghx.ptr_array([a.ptr - b for a, b in zip(dst, dback)])
        segs = UC.segments(h)
        assert [(g.src_lid64, g.dst_lid64) for g in segs] == [(int(sbias > 0), int(dbias > 0))] * len(segs)
        _ghx.call("ghx_put_execute", h, sp, ns, dp, nd, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        UC.destroy(h)
    want = [a.host.copy() for a in dst]
    for m in msgs:
        UC.apply_put(src[m[2]].field(), want[m[3]][dst[m[3]].at:], Side(m[0], 0, m[4]), Side(m[1], 0, m[5]))
    for k, a in enumerate(dst):
        got = a.device_bytes()
        assert (got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all()
        np.testing.assert_array_equal(got, want[k])
        assert (want[k] != SENTINEL).sum() > 0
    for a in src:
        np.testing.assert_array_equal(a.device_bytes(), a.host)
    return segs


def three_lists(sd, dd, seed=0, repeats=False, **kw):
    """The standard case: three messages of 3001, 3002 and 3003 lids drawn without repetition
    from 10007 cells, over two source and two target fields."""
    rng = np.random.default_rng(seed)
    s, t = UC.draw_lists(rng), UC.draw_lists(rng)
    if repeats:
        s[0][1:2000:7] = s[0][0]       # one cell sent many times
        s[2][-1] = s[1][-1]            # and a cell sent in two messages
    slots = ((0, 1), (0, 0), (1, 0))
    return run_messages([(sd, dd, a, b, s[m], t[m]) for m, (a, b) in enumerate(slots)],
                        seed=seed, **kw)


# ---------------------------------------------------------------------------------------------
# general path
# ---------------------------------------------------------------------------------------------
def _mode_descs(mode, e):
    if mode == 0:   # rows of three elements: off the run path at every element size
        return udesc(e, 3), udesc(e, 3)
    if mode == 1:   # contiguous levels against strided ones
        return udesc(e, 3, index_stride=4), udesc(e, 3, index_stride=1, level_stride=N_CELLS)
    return udesc(e, 3, first=False), udesc(e, 3, first=False, level_stride=N_CELLS + 16 // e)


@pytest.mark.parametrize("e", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_every_mode_at_every_vector_width(mode, e):
    sd, dd = _mode_descs(mode, e)
    segs = three_lists(sd, dd, seed=mode * 8 + e)
    assert all(g.mode == mode and 1 << g.wlog2 == e for g in segs)
    assert all(-(-g.bytes // g.tile_bytes) > 1 for g in segs)  # several tiles, the last partial


@pytest.mark.parametrize("sshift, dshift", [(4, 0), (0, 2), (8, 1), (16, 16)])
def test_width_narrowed_by_one_pointer_alone(sshift, dshift):
    segs = three_lists(udesc(16, 2), udesc(16, 2, index_stride=3), seed=21, sshift=sshift, dshift=dshift)
    assert all(g.wlog2 == 4 and g.mode == 0 for g in segs)
    segs = three_lists(*_mode_descs(2, 16), seed=22, sshift=sshift, dshift=dshift)
    assert all(g.wlog2 == 4 and g.mode == 2 for g in segs)


@pytest.mark.parametrize("e", [3, 12])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_elements_of_3_and_12_bytes(mode, e):
    sd, dd = _mode_descs(mode, e)
    segs = three_lists(sd, dd, seed=30 + e + mode)
    assert all(1 << g.wlog2 == (1 if e == 3 else 4) for g in segs)
    one = three_lists(udesc(e), udesc(e, index_stride=2), seed=40 + e)
    assert all(g.mode == 0 and g.row_bytes == e for g in one)


@pytest.mark.parametrize("sbias, dbias", [(0, 0), (BIAS, 0), (0, BIAS), (BIAS, BIAS)])
def test_table_widths_in_all_side_combinations(sbias, dbias):
    three_lists(udesc(8, 2), udesc(8, 2, index_stride=3), seed=50, sbias=sbias, dbias=dbias)
    three_lists(*_mode_descs(1, 4), seed=51, sbias=sbias, dbias=dbias)


def test_padded_and_unpadded_strides_swapped_between_the_sides():
    padded, dense = udesc(4, 3, index_stride=5), udesc(4, 3)
    three_lists(padded, dense, seed=60)
    three_lists(dense, padded, seed=61)
    three_lists(udesc(8, 2, index_stride=4, level_stride=2), udesc(8, 2, index_stride=6, level_stride=3), seed=62)


def test_source_list_with_repeats():
    three_lists(udesc(8, 2), udesc(8, 2), seed=70, repeats=True)
    three_lists(udesc(8), udesc(8), seed=71, repeats=True)   # run path
    three_lists(*_mode_descs(2, 4), seed=72, repeats=True)


# ---------------------------------------------------------------------------------------------
# run path: 4- and 8-byte rows, mode 0
# ---------------------------------------------------------------------------------------------
def _regions(K):
    """Disjoint cell ranges for messages of n = 1, K-1, K, K+1 and 3001 lids."""
    return [(1, (0, 20)), (K - 1, (20, 40)), (K, (40, 60)), (K + 1, (60, 80)), (3001, (100, N_CELLS))]


def _full_runs(rng, n, lo, hi):
    a = int(rng.integers(lo, hi - n + 1))
    return np.arange(a, a + n, dtype=np.int64)


def _scattered(rng, n, lo, hi):
    return rng.choice(np.arange(lo, hi), size=n, replace=False).astype(np.int64)


def _mixed(rng, n, lo, hi):
    """Runs of lengths 1..7 (cycling), separated by gaps of 1-3 cells, in a shuffled order: 16-byte
    chunks straddle the run boundaries."""
    runs, at, left, k = [], lo, n, 0
    while left:
        ln = min(left, 1 + k % 7)
        runs.append(np.arange(at, at + ln, dtype=np.int64))
        at += ln + int(rng.integers(1, 4))
        left -= ln
        k += 1
    assert at <= hi + 3
    return np.concatenate([runs[i] for i in rng.permutation(len(runs))])


RUN_PATTERNS = {"runs-runs": (_full_runs, _full_runs), "scattered-runs": (_scattered, _full_runs),
                "runs-scattered": (_full_runs, _scattered), "scattered-scattered": (_scattered, _scattered),
                "mixed-mixed": (_mixed, _mixed), "mixed-runs": (_mixed, _full_runs),
                "runs-mixed": (_full_runs, _mixed)}


def _run_messages(L, pattern, seed, sd=None, dd=None, **kw):
    rng = np.random.default_rng(seed)
    sd, dd = sd or udesc(L), dd or udesc(L)
    gs, gt = RUN_PATTERNS[pattern]
    msgs = [(sd, dd, 0, 0, gs(rng, n, lo, hi), gt(rng, n, lo, hi)) for n, (lo, hi) in _regions(16 // L)]
    return run_messages(msgs, seed=seed, **kw)


@pytest.mark.parametrize("pattern", list(RUN_PATTERNS))
@pytest.mark.parametrize("L", [4, 8])
def test_run_path_patterns_and_sizes(L, pattern):
    segs = _run_messages(L, pattern, seed=100 + L)
    assert [g.n for g in segs] == [1, 16 // L - 1, 16 // L, 16 // L + 1, 3001]
    assert all(g.src_runs and g.dst_runs and g.mode == 0 for g in segs)


@pytest.mark.parametrize("L", [4, 8])
def test_run_path_with_one_sides_index_stride_not_the_row(L):
    """A side whose index stride is not the row length never forms runs (flag 0), but its offsets
    follow its own stride; the other side still does."""
    wide = udesc(L, index_stride=3)
    for pattern in ("runs-runs", "mixed-mixed"):
        segs = _run_messages(L, pattern, seed=120 + L, sd=wide)
        assert all(g.src_runs == 0 and g.dst_runs for g in segs)
        segs = _run_messages(L, pattern, seed=130 + L, dd=wide)
        assert all(g.src_runs and g.dst_runs == 0 for g in segs)


@pytest.mark.parametrize("L", [4, 8])
def test_run_path_with_pointers_aligned_to_the_row_only(L):
    for pattern in ("runs-runs", "mixed-mixed"):
        _run_messages(L, pattern, seed=140 + L, sshift=L, dshift=0)
        _run_messages(L, pattern, seed=141 + L, sshift=0, dshift=L)
        _run_messages(L, pattern, seed=142 + L, sshift=L, dshift=16 - L)
    _run_messages(L, "mixed-mixed", seed=143, sshift=1, dshift=0)  # not even that: general path


def test_run_eligible_message_next_to_one_that_is_not():
    """One launch takes one path: with a 24-byte-row message in the plan, the 8-byte-row message
    goes through the general kernel too."""
    rng = np.random.default_rng(150)
    s, t = UC.draw_lists(rng), UC.draw_lists(rng)
    segs = run_messages([(udesc(8), udesc(8), 0, 0, np.sort(s[0]), np.sort(t[0])),
                         (udesc(8, 3), udesc(8, 3), 1, 1, s[1], t[1]),
                         (udesc(4), udesc(4), 2, 2, _mixed(rng, 500, 0, 3000), t[2][:500])], seed=150)
    assert [g.row_bytes for g in segs] == [8, 24, 4]


def test_run_path_off_by_knob():
    from ghex_amd import _ghx
    try:
        _ghx.call("ghx_tune", b"urun", 0)
        segs = _run_messages(8, "mixed-mixed", seed=160)
        assert all(g.src_runs == 0 and g.dst_runs == 0 for g in segs)
        _run_messages(4, "runs-runs", seed=161)
    finally:
        _ghx.call("ghx_tune", b"reset", 0)


# ---------------------------------------------------------------------------------------------
# tiling knobs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", [{"u_tile_rows": 3, "u_tile_bytes": 1024}, {"u_run_tile_rows": 64},
                                   {"u_tile_rows": 3, "u_tile_bytes": 1024, "u_run_tile_rows": 64,
                                    "grid_cap": 5},
                                   {"small_row_bytes": 4096, "u_tile_rows": 5, "grid_cap": 1},
                                   {"tile_records": 0, "order": 0}],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_tiling_knobs_stay_bit_exact(knobs):
    """Tiny and partial tiles, tiles of 12 bytes (no whole 16-byte chunk: the run-eligible messages
    take the general kernel), fewer workgroups than tiles. The put has one table form (a record
    per tile): tile_records 0 changes nothing for it."""
    from ghex_amd import _ghx
    try:
        for k, v in knobs.items():
            _ghx.call("ghx_tune", k.encode(), v)
        for mode, e in ((0, 4), (1, 16), (2, 8), (0, 3)):
            three_lists(*_mode_descs(mode, e), seed=200 + mode)
        for L in (4, 8):
            _run_messages(L, "mixed-mixed", seed=210 + L)
            _run_messages(L, "runs-scattered", seed=220 + L)
    finally:
        _ghx.call("ghx_tune", b"reset", 0)


# ---------------------------------------------------------------------------------------------
# product path, emulated ranks: planned as the bulk object plans its puts
# ---------------------------------------------------------------------------------------------
class UPuts:
    """Every emulated rank's put plans over bis_all[r] (one process, all fields on the one GPU),
    from field_records(export=False) -> put_messages -> put_chunks -> uput_entries."""

    def __init__(self, bis_all):
        from ghex_amd import _ghx
        from ghex_amd import bulk_communication_object as B
        self.ghx = _ghx
        groups = [B.field_groups(bis) for bis in bis_all]
        allr = [{"host": "h", "fields": B.field_records(bis, g, export=False)}
                for bis, g in zip(bis_all, groups)]
        local = list(range(len(bis_all)))
        self.plans, self._keep, self.bytes = [], [], 0
        for r, bis in enumerate(bis_all):
            for chunk, srcs, dsts in B.put_chunks(B.put_messages(bis, groups[r], allr, local)):
                assert all(B.message_kind(m) == 1 for m in chunk)
                src, dst, keep = B.uput_entries(chunk, srcs, dsts, [bi.field.desc for bi in bis], allr)
                h = ctypes.c_void_p()
                _ghx.call("ghx_uput_create", src, dst, len(chunk), ctypes.byref(h))
                self._keep.append(keep)
                sp = _ghx.ptr_array([bis[k].field.data_ptr() for k in srcs])
                dp = _ghx.ptr_array([bis_all[tr][ti].field.data_ptr() for tr, ti in dsts])
                self.plans.append((h, sp, len(srcs), dp, len(dsts)))
                self.bytes += UC.put_info(h)[0]

    def execute(self, stream):
        for h, sp, ns, dp, nd in self.plans:
            self.ghx.call("ghx_put_execute", h, sp, ns, dp, nd, stream)

    def close(self):
        for h, *_ in self.plans:
            self.ghx.lib().ghx_put_destroy(h)
        self.plans = []


@pytest.mark.parametrize("seed", range(40))
def test_random_unstructured_puts_equal_the_buffered_exchange(seed):
    import torch
    from tests.gpu_util import emulated_exchange
    from tests.test_gpu_fuzz import _check_unstructured, _setup_unstructured, draw_unstructured
    case = draw_unstructured(seed)
    cos, bis_all, recs = _setup_unstructured(case)
    first = [t.clone() for (_, _, t, _) in recs]
    emulated_exchange(cos, bis_all)
    buffered = [t.clone() for (_, _, t, _) in recs]
    for (_, _, t, _), b in zip(recs, first):
        t.copy_(b)
    puts = UPuts(bis_all)
    try:
        puts.execute(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        puts.close()
    _check_unstructured(case, recs)
    for (_, _, t, _), b in zip(recs, buffered):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8))


# ---------------------------------------------------------------------------------------------
# product path, the real object: one rank holding the four domains of the known-answer case
# ---------------------------------------------------------------------------------------------
def _known_answer(golden_dir, levels, levels_first, dtype=np.float64):
    """(bulk object's buffer infos, [(domain, device tensor, expected host array, outer lids)],
    pattern): value(dom, gid, level) = dom*10000 + gid*100 + level in owned cells, -1 in halos."""
    import torch
    import ghex_amd
    from ghex_amd import unstructured as U
    with open(os.path.join(golden_dir, "unstructured_case.json")) as fh:
        case = json.load(fh)
    ctx = ghex_amd.make_context()
    doms = [case["domains"][str(r)] for r in range(4)]
    dds = [U.DomainDescriptor(r, d["gids"], d["halo_lids"]) for r, d in enumerate(doms)]
    pc = U.make_pattern(ctx, U.HaloGenerator(), dds)
    bis, fields = [], []
    for r, (d, dd) in enumerate(zip(doms, dds)):
        n = len(d["gids"])
        init = np.full((n, levels), -1, dtype=dtype)
        for lid, gid in enumerate(d["gids"]):
            if lid not in d["halo_lids"]:
                init[lid] = [r * 10000 + gid * 100 + l for l in range(levels)]
        want = init.copy()
        for rid, rr, tag, lids in pc.recv_halos(pc.local_index(r)):
            for lid in lids:
                want[lid] = [rid * 10000 + d["gids"][lid] * 100 + l for l in range(levels)]
        t = torch.from_numpy(init).cuda()
        if not levels_first:  # level-major storage, also for a single level
            last = torch.empty_strided((n, levels), (1, n), dtype=t.dtype, device="cuda")
            t = last.copy_(t)
        fd = U.make_field_descriptor(dd, t)
        assert fd.levels_first == levels_first
        bis.append(pc(fd))
        fields.append((r, t, init, want))
    return ctx, pc, bis, fields


def _rewrite(fields, scale=1):
    import torch
    for r, t, init, want in fields:
        t.copy_(torch.from_numpy(np.where(init < 0, init, init * scale)).to(t.device))


def _check_fields(fields, scale=1):
    for r, t, init, want in fields:
        np.testing.assert_array_equal(t.cpu().numpy(), np.where(want < 0, want, want * scale))


@pytest.mark.parametrize("levels, levels_first", [(1, True), (3, True), (1, False), (3, False)])
def test_bulk_object_known_answer_on_one_rank(golden_dir, levels, levels_first):
    from ghex_amd import make_bulk_communication_object
    ctx, pc, bis, fields = _known_answer(golden_dir, levels, levels_first)
    bco = make_bulk_communication_object(ctx)
    bco.add_fields(*bis)
    bco.init()
    halo = sum(len(lids) for i in range(4) for _, _, _, lids in pc.recv_halos(i))
    assert halo > 0 and bco.bytes_per_exchange() == halo * levels * 8
    for k in (1, 2):
        _rewrite(fields, k)
        bco.exchange().wait()
        _check_fields(fields, k)


def test_bulk_object_with_a_structured_and_an_unstructured_field(golden_dir):
    """One object, one exchange(): the structured field's puts (ghx_put_create) and the
    unstructured fields' (ghx_uput_create) are separate plans of the same object."""
    from oracle import oracle as orc
    from ghex_amd import make_bulk_communication_object
    from ghex_amd import bulk_communication_object as B
    from ghex_amd.structured import regular as R
    from tests import helpers as H
    from tests.gpu_util import device_field
    ctx, pc, bis, fields = _known_answer(golden_dir, 3, True, dtype=np.float32)
    N, Hw, layout = 12, 2, (2, 1, 0)
    E = N + 2 * Hw
    ranks, gf, gl = H.cube_domains(N, (1, 1, 1))
    dom = ranks[0][0]
    a, spec = H.linear_index_field(dom, N, Hw, gl, layout=layout)
    base, logical = device_field(a.copy(), layout)
    sdd = R.DomainDescriptor(0, dom.first, dom.last)
    spc = R.make_pattern(ctx, R.HaloGenerator(gf, gl, (Hw,) * 6, (True,) * 3), [sdd])
    sbi = spc(R.make_field_descriptor(sdd, logical, (Hw,) * 3, (E,) * 3))
    bco = make_bulk_communication_object(ctx)
    bco.add_fields(bis[0], bis[1], sbi, bis[2], bis[3])
    bco.init()
    assert len(bco._puts) == 3  # unstructured, structured, unstructured: a plan holds one kind
    halo = sum(len(lids) for i in range(4) for _, _, _, lids in pc.recv_halos(i))
    assert bco.bytes_per_exchange() == halo * 3 * 4 + (E ** 3 - N ** 3) * 8
    assert B.message_kind((0, [((0, 0, 0), (1, 1, 1))], (0, 0), [])) == 0
    for _ in range(2):
        bco.exchange().wait()
    _check_fields(fields)
    opat = orc.regular_make_pattern(ranks, gf, gl, (Hw,) * 6, (1, 1, 1))
    orc.regular_exchange([[(spec, 0, 0, 0)]], {0: opat}, 1)
    np.testing.assert_array_equal(base.cpu().numpy(), a)


def test_bulk_exchange_replayed_from_a_linear_capture(golden_dir):
    """One rank, no epochs: the exchange is one linear chain of put launches. Captured once,
    replayed twice from rewritten fields (new owned values, stale halos overwritten by -1)."""
    import torch
    from ghex_amd import make_bulk_communication_object
    ctx, pc, bis, fields = _known_answer(golden_dir, 3, True)
    bco = make_bulk_communication_object(ctx)
    bco.add_fields(*bis)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bco.exchange().wait()  # set-up and a warm run, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _check_fields(fields)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bco.exchange()
    for k in (3, 5):
        _rewrite(fields, k)
        g.replay()
        torch.cuda.synchronize()
        _check_fields(fields, k)
