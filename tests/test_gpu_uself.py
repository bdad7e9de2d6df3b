"""The fused index-list self exchange on the device (ghx_uself_create, k_self_u) and the
communication object's fuse_lists option. Kernel cases through the ABI: every field in an arena
of its own between 256-byte guard bands (sources hold random bytes, targets the sentinel), every
buffer in an arena of its own filled with the sentinel; after ONE execute every byte of every
arena is compared — targets with the NumPy form of the put's definition (tests/uput_cases.py),
buffers with the NumPy form of the packed message (tests/uself_cases.py; pad bytes and guards
still the sentinel), sources unchanged. Product path: the known-answer case on one rank, forty
random meshes with every domain on rank 0 against the default object, graph replay, and the
fallback with peers. Every comparison is bit-exact."""
import ctypes

import numpy as np
import pytest

from tests import uput_cases as UC
from tests import uself_cases as US
from tests.uput_cases import Side, udesc
from tests.test_gpu_uput import (BIAS, GUARD, SENTINEL, RUN_PATTERNS, Arena, _check_fields, _known_answer,
                                 _mixed, _mode_descs, _regions, _rewrite)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ghex_amd
    ghex_amd.native_library()


def _up(x, a):
    return (x + a - 1) // a * a


def run_messages(msgs, sshift=0, dshift=0, bshift=0, sbias=0, dbias=0, seed=0):
    """msgs: [(source desc, target desc, source slot, target slot, source lids, target lids,
    buffer slot, buffer offset)]; source and target slots index ONE pointer array. One plan, one
    execute; every arena compared byte for byte. sshift / dshift move the fields that are only
    sources / the fields that are targets, bshift the buffers."""
    import torch
    from ghex_amd import _ghx
    rng = np.random.default_rng(2000 + seed)
    nf = 1 + max(max(m[2], m[3]) for m in msgs)
    nb = 1 + max(m[6] for m in msgs)
    src_slots, dst_slots = {m[2] for m in msgs}, {m[3] for m in msgs}
    assert not (src_slots & dst_slots) or sbias == dbias
    fields, back = [], []
    for k in range(nf):
        descs = [m[0] for m in msgs if m[2] == k] + [m[1] for m in msgs if m[3] == k]
        if not descs:
            fields.append(None)
            back.append(0)
            continue
        span = max(UC.span_bytes(d) for d in descs)
        fields.append(Arena(span, dshift if k in dst_slots else sshift, rng if k in src_slots else None))
        # a biased table addresses the same cells from a pointer moved back by the bias
        back.append((dbias if k in dst_slots else sbias) * descs[0].index_stride * descs[0].elem_size)
    bufs = []
    for b in range(nb):
        ends = [m[7] + US.message_bytes(Side(m[0], 0, m[4])) for m in msgs if m[6] == b]
        bufs.append(Arena(max(ends), bshift) if ends else None)
    srcs = [Side(m[0], m[2], np.asarray(m[4]) + sbias) for m in msgs]
    dsts = [Side(m[1], m[3], np.asarray(m[5]) + dbias) for m in msgs]
    h = US.create(srcs, dsts, [(m[6], m[7]) for m in msgs])
    try:
        fp = _ghx.ptr_array([(a.ptr - bk) if a else 0 for a, bk in zip(fields, back)])
        bp = _ghx.ptr_array([a.ptr if a else 0 for a in bufs])
        segs = US.segments(h)
        assert [(g.src_lid64, g.dst_lid64) for g in segs] == [(int(sbias > 0), int(dbias > 0))] * len(segs)
        _ghx.call("ghx_uself_execute", h, fp, nf, bp, nb, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        US.destroy(h)
    want_f = [a.host.copy() if a else None for a in fields]
    want_b = [a.host.copy() if a else None for a in bufs]
    for m in msgs:
        s, t = Side(m[0], 0, m[4]), Side(m[1], 0, m[5])
        UC.apply_put(fields[m[2]].field(), want_f[m[3]][fields[m[3]].at:], s, t)
        US.packed(fields[m[2]].field(), s, m[7], want_b[m[6]][bufs[m[6]].at:])
    for arenas, want in ((fields, want_f), (bufs, want_b)):
        for a, w in zip(arenas, want):
            if a is None:
                continue
            got = a.device_bytes()
            if (a.host[:GUARD] == SENTINEL).all():  # not a source arena (random bytes throughout)
                assert (got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all()
            np.testing.assert_array_equal(got, w)   # guard bands included
    for k in dst_slots:
        assert (want_f[k] != fields[k].host).sum() > 0
    for w in want_b:
        assert w is None or (w != SENTINEL).sum() > 0
    return segs


def three_lists(sd, dd, seed=0, repeats=False, boff=0, align=16, **kw):
    """The standard case: three messages of 3001, 3002 and 3003 lids drawn without repetition
    from 10007 cells, from two source fields into two target fields; the first two share buffer
    0 (the second `align`ed behind the first: a pad gap unless the first ends aligned), the
    third has buffer 1."""
    rng = np.random.default_rng(seed)
    s, t = UC.draw_lists(rng), UC.draw_lists(rng)
    if repeats:
        s[0][1:2000:7] = s[0][0]       # one cell sent many times
        s[2][-1] = s[1][-1]            # and a cell sent in two messages
    nb0 = US.message_bytes(Side(sd, 0, s[0]))
    places = ((0, boff), (0, _up(boff + nb0, align)), (1, boff))
    slots = ((0, 3), (0, 2), (1, 2))
    return run_messages([(sd, dd, a, b, s[m], t[m]) + places[m] for m, (a, b) in enumerate(slots)],
                        seed=seed, **kw)


# ---------------------------------------------------------------------------------------------
# general path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_every_mode_at_every_vector_width(mode, e):
    sd, dd = _mode_descs(mode, e)
    segs = three_lists(sd, dd, seed=mode * 8 + e)
    assert all(g.mode == mode and 1 << g.wlog2 == e for g in segs)
    assert all(-(-g.bytes // g.tile_bytes) > 1 for g in segs)  # several tiles, the last partial


@pytest.mark.parametrize("e", [3, 12])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_elements_of_3_and_12_bytes(mode, e):
    sd, dd = _mode_descs(mode, e)
    segs = three_lists(sd, dd, seed=30 + e + mode, align=e)
    assert all(1 << g.wlog2 == (1 if e == 3 else 4) for g in segs)
    one = three_lists(udesc(e), udesc(e, index_stride=2), seed=40 + e, align=4)
    assert all(g.mode == 0 and g.row_bytes == e for g in one)


@pytest.mark.parametrize("which", ["source", "target", "buffer"])
def test_width_narrowed_by_one_pointer_alone(which):
    kw = {"source": dict(sshift=4), "target": dict(dshift=2), "buffer": dict(bshift=8)}[which]
    segs = three_lists(udesc(16, 2), udesc(16, 2, index_stride=3), seed=21, **kw)
    assert all(g.wlog2 == 4 and g.mode == 0 for g in segs)
    segs = three_lists(*_mode_descs(2, 16), seed=22, **kw)
    assert all(g.wlog2 == 4 and g.mode == 2 for g in segs)


@pytest.mark.parametrize("boff, w", [(4, 2), (8, 3), (2, 1), (1, 0)])
def test_width_narrowed_by_the_buffer_offset_alone(boff, w):
    """16-byte elements at a buffer offset of 4: the planner narrows every vector of the message."""
    segs = three_lists(udesc(16, 2), udesc(16, 2, index_stride=3), seed=23, boff=boff, align=1)
    assert segs[0].wlog2 == w and segs[2].wlog2 == w and segs[0].buf_off == boff
    segs = three_lists(*_mode_descs(1, 16), seed=24, boff=boff, align=1)
    assert segs[0].wlog2 == w and segs[0].mode == 1


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


def test_one_field_slot_that_is_source_and_target_on_disjoint_cells():
    rng = np.random.default_rng(80)
    a, b, c, d = UC.draw_lists(rng, (2001, 2002, 2003, 2004))
    for sd in (udesc(8, 2), udesc(8), udesc(4, 3, first=False)):
        # field 0 sends cells a to field 1 and receives cells b from it; and sends c to its own d
        run_messages([(sd, sd, 0, 1, a, a, 0, 0), (sd, sd, 1, 0, b[:2001], b[:2001], 1, 0),
                      (sd, sd, 0, 0, c, d[:2003], 2, 16)], seed=80)


def test_two_messages_in_one_buffer_with_a_pad_gap():
    rng = np.random.default_rng(90)
    s, t = UC.draw_lists(rng), UC.draw_lists(rng)
    sd, dd = udesc(4, 3), udesc(4, 3, index_stride=4)
    end0 = 3001 * 12
    segs = run_messages([(sd, dd, 0, 1, s[0], t[0], 0, 0), (sd, dd, 0, 1, s[1], t[1], 0, end0 + 52),
                         (udesc(8), udesc(8), 0, 2, s[2], t[2], 0, _up(end0 + 52 + 3002 * 12, 64) + 64)],
                        seed=90)
    assert [g.buf_off for g in segs] == [0, end0 + 52, _up(end0 + 52 + 3002 * 12, 64) + 64]


# ---------------------------------------------------------------------------------------------
# run path: 4- and 8-byte rows, mode 0
# ---------------------------------------------------------------------------------------------
def _run_messages(L, pattern, seed, sd=None, dd=None, boff=0, **kw):
    """Messages of n = 1, K-1, K, K+1 and 3001 lids from disjoint cell ranges, field 0 -> field
    1, back to back in buffer 0 at 16-byte aligned offsets from `boff`."""
    rng = np.random.default_rng(seed)
    sd, dd = sd or udesc(L), dd or udesc(L)
    gs, gt = RUN_PATTERNS[pattern]
    msgs, at = [], boff
    for n, (lo, hi) in _regions(16 // L):
        msgs.append((sd, dd, 0, 1, gs(rng, n, lo, hi), gt(rng, n, lo, hi), 0, at))
        at = _up(at + n * L, 16) + (boff % 16)
    return run_messages(msgs, seed=seed, **kw)


@pytest.mark.parametrize("pattern", list(RUN_PATTERNS))
@pytest.mark.parametrize("L", [4, 8])
def test_run_path_patterns_and_sizes(L, pattern):
    segs = _run_messages(L, pattern, seed=100 + L)
    assert [g.n for g in segs] == [1, 16 // L - 1, 16 // L, 16 // L + 1, 3001]
    assert all(g.src_runs and g.dst_runs and g.mode == 0 and g.buf_off % 16 == 0 for g in segs)


@pytest.mark.parametrize("L", [4, 8])
def test_run_path_with_one_sides_index_stride_not_the_row(L):
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
    _run_messages(L, "mixed-mixed", seed=144, bshift=L)            # buffer chunks off 16 B: general path


@pytest.mark.parametrize("L", [4, 8])
def test_buffer_offset_that_is_a_multiple_of_the_row_but_not_of_16(L):
    """The planner keeps the run flags; the launch sees a chunk of the buffer that is not 16-byte
    aligned and takes the general kernel for the whole plan."""
    for pattern in ("runs-runs", "mixed-mixed"):
        segs = _run_messages(L, pattern, seed=145 + L, boff=L)
        assert all(g.src_runs and g.dst_runs and g.buf_off % 16 == L for g in segs)
        assert all(g.wlog2 == (2 if L == 4 else 3) for g in segs)


def test_run_eligible_message_next_to_one_that_is_not():
    rng = np.random.default_rng(150)
    s, t = UC.draw_lists(rng), UC.draw_lists(rng)
    segs = run_messages([(udesc(8), udesc(8), 0, 3, np.sort(s[0]), np.sort(t[0]), 0, 0),
                         (udesc(8, 3), udesc(8, 3), 1, 4, s[1], t[1], 1, 0),
                         (udesc(4), udesc(4), 2, 5, _mixed(rng, 500, 0, 3000), t[2][:500], 2, 0)], seed=150)
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
    from ghex_amd import _ghx
    try:
        for k, v in knobs.items():
            _ghx.call("ghx_tune", k.encode(), v)
        for mode, e in ((0, 4), (1, 16), (2, 8), (0, 3)):
            three_lists(*_mode_descs(mode, e), seed=200 + mode, align=16 if e != 3 else 1)
        for L in (4, 8):
            _run_messages(L, "mixed-mixed", seed=210 + L)
            _run_messages(L, "runs-scattered", seed=220 + L)
    finally:
        _ghx.call("ghx_tune", b"reset", 0)


# ---------------------------------------------------------------------------------------------
# product path: the communication object with fuse_lists
# ---------------------------------------------------------------------------------------------
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


def _send_bytes(co, bis):
    """The message bytes of every send buffer (the buffers' pad bytes are never written)."""
    plan = co.plan(bis)
    send, _ = co.buffers(plan, bis[0].field.device)
    return [t[:x["size"]].cpu().numpy() for t, x in zip(send, plan.send)]


@pytest.mark.parametrize("levels, levels_first", [(1, True), (3, True), (1, False), (3, False)])
def test_known_answer_case_in_one_launch(golden_dir, levels, levels_first):
    from ghex_amd import unstructured as U
    ctx, pc, bis, fields = _known_answer(golden_dir, levels, levels_first)
    co = U.make_communication_object(ctx, fuse_lists=True)
    assert co.lists_self(co.plan(bis)) and not co.all_self(co.plan(bis))
    dctx, dpc, dbis, dfields = _known_answer(golden_dir, levels, levels_first)
    plain = U.make_communication_object(dctx)
    assert not plain.fuse_lists
    for k in (1, 2):
        _rewrite(fields, k)
        _rewrite(dfields, k)
        assert _launches(co, bis) == 1
        assert _launches(plain, dbis) == 2
        _check_fields(fields, k)
        _check_fields(dfields, k)
        got, exp = _send_bytes(co, bis), _send_bytes(plain, dbis)
        assert len(got) == len(exp) > 0
        # one 8-byte field per domain: every byte of a send buffer is a message byte
        for g, e in zip(got, exp):
            np.testing.assert_array_equal(g, e)


NO_HALO_SEEDS = (11, 30, 34, 35, 38)   # draw no halo cell at all: nothing to exchange


def _on_one_rank(seed):
    from tests.test_gpu_fuzz import draw_unstructured
    case = draw_unstructured(seed)
    case["nr"] = 1
    for d in case["doms"]:
        d["rank"] = 0
    return case


@pytest.mark.parametrize("seed", range(40))
def test_random_meshes_on_one_rank_equal_the_default_object(seed):
    import torch
    from ghex_amd import unstructured as U
    from tests.test_gpu_fuzz import _check_unstructured, _setup_unstructured
    results = []
    for fuse in (True, False):
        case = _on_one_rank(seed)
        cos, bis_all, recs = _setup_unstructured(case)
        bis = bis_all[0]
        co = U.make_communication_object(cos[0].context, fuse_lists=fuse)
        plan = co.plan(bis)
        if fuse:
            assert co.lists_self(plan) == (seed not in NO_HALO_SEEDS)
        # the send buffers start from the sentinel: bytes no launch writes compare equal
        send, _ = co.buffers(plan, bis[0].field.device)
        for t in send:
            t.fill_(SENTINEL)
        n = _launches(co, bis)
        if seed in NO_HALO_SEEDS:
            assert plan.send == []
        else:
            assert n == (1 if fuse else 2)
        _check_unstructured(case, recs)
        results.append(([t.clone() for (_, _, t, _) in recs],
                        [t[:x["size"]].clone() for t, x in zip(send, plan.send)]))
    (ff, fb), (pf, pb) = results
    assert len(ff) == len(pf) and len(fb) == len(pb)
    for a, b in zip(ff, pf):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for a, b in zip(fb, pb):
        assert torch.equal(a, b)


def test_fused_exchange_replayed_from_a_capture(golden_dir):
    """One rank: the exchange is one launch. Captured once, replayed twice from rewritten fields
    (new owned values, stale halos overwritten by -1)."""
    import torch
    from ghex_amd import unstructured as U
    ctx, pc, bis, fields = _known_answer(golden_dir, 3, True)
    co = U.make_communication_object(ctx, fuse_lists=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        co.exchange(bis).wait()  # set-up and a warm run, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _check_fields(fields)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        co.exchange(bis)
    for k in (3, 5):
        _rewrite(fields, k)
        g.replay()
        torch.cuda.synchronize()
        _check_fields(fields, k)


def test_with_peers_the_option_changes_nothing():
    """Two emulated ranks: the plans are not fusable and take the two-launch path."""
    import torch
    from ghex_amd import unstructured as U
    from tests.gpu_util import emulated_exchange
    from tests.test_gpu_fuzz import _check_unstructured, _setup_unstructured, draw_unstructured
    seed = next(s for s in range(40) if draw_unstructured(s)["nr"] == 2 and s not in NO_HALO_SEEDS)
    out = []
    for fuse in (True, False):
        case = draw_unstructured(seed)
        cos, bis_all, recs = _setup_unstructured(case)
        cos = [U.make_communication_object(co.context, fuse_lists=fuse) for co in cos]
        if fuse:
            assert not any(co.lists_self(co.plan(bis)) for co, bis in zip(cos, bis_all))
        emulated_exchange(cos, bis_all)
        _check_unstructured(case, recs)
        out.append([t.clone() for (_, _, t, _) in recs])
    for a, b in zip(*out):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
