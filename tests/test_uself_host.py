"""Fused index-list self exchange plans (ghx_uself_create, ghx_uexchange_self_info) without a
device: every refusal with its reason, what the planner decides per segment (ghx_uself_segment),
the NumPy form of the packed message against the oracle's unstructured pack, and which exchanges
built from patterns are planned as one launch."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import uput_cases as UC
from tests import uself_cases as US
from tests.uput_cases import Side, udesc


@pytest.fixture(scope="module")
def ghx():
    from ghex_amd import _ghx
    _ghx.lib()
    return _ghx


@pytest.fixture(autouse=True)
def _reset_knobs(ghx):
    yield
    ghx.call("ghx_tune", b"reset", 0)


def _lists(seed=0, sizes=(301, 17)):
    """Source lists and target lists, all four disjoint (one draw)."""
    rng = np.random.default_rng(seed)
    ls = UC.draw_lists(rng, tuple(sizes) * 2)
    return ls[:len(sizes)], ls[len(sizes):]


def _one(sd, dd, s=None, t=None, n=301, seed=0, off=0):
    """The single segment of a one-message plan."""
    (s0,), (t0,) = _lists(seed, (n,))
    s = s0 if s is None else s
    t = t0 if t is None else t
    h = US.create([Side(sd, 0, s)], [Side(dd, 1, t)], [(0, off)])
    segs = US.segments(h)
    US.destroy(h)
    assert len(segs) == 1
    return segs[0]


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def _refused(srcs, dsts, places, fragment, dst_places=None):
    rc, why, h = US.try_create(srcs, dsts, places, dst_places)
    assert rc == -1 and not h.value, (rc, why)
    assert fragment in why, why


def test_sides_that_differ_are_refused(ghx):
    (s0, s1), (t0, t1) = _lists()
    same = "do not describe the same message bytes"
    _refused([Side(udesc(8), 0, s0)], [Side(udesc(8), 1, t0[:-1])], [(0, 0)], same)
    _refused([Side(udesc(8), 0, s0)], [Side(udesc(4), 1, t0)], [(0, 0)], same)
    _refused([Side(udesc(4, 2), 0, s0)], [Side(udesc(4, 3), 1, t0)], [(0, 0)], same)
    _refused([Side(udesc(4, 2, first=True), 0, s0)], [Side(udesc(4, 2, first=False), 1, t0)],
             [(0, 0)], same)


def test_sides_at_different_buffer_bytes_are_refused(ghx):
    (s0, _), (t0, _) = _lists()
    why = "differ in buffer slot or buffer offset"
    _refused([Side(udesc(8), 0, s0)], [Side(udesc(8), 1, t0)], [(0, 0)], why, [(1, 0)])
    _refused([Side(udesc(8), 0, s0)], [Side(udesc(8), 1, t0)], [(0, 0)], why, [(0, 8)])


def test_messages_that_overlap_in_a_buffer_are_refused(ghx):
    (s0, s1), (t0, t1) = _lists()
    srcs = [Side(udesc(8), 0, s0), Side(udesc(8), 0, s1)]
    dsts = [Side(udesc(8), 1, t0), Side(udesc(8), 1, t1)]
    _refused(srcs, dsts, [(0, 0), (0, 301 * 8 - 8)], "two messages overlap in one buffer")
    _refused(srcs, dsts, [(2, 64), (2, 0)], "two messages overlap in one buffer")
    # back to back, with a gap, or in different buffers: fine
    for places in ([(0, 0), (0, 301 * 8)], [(0, 17 * 8 + 40), (0, 0)], [(0, 0), (1, 0)]):
        US.destroy(US.create(srcs, dsts, places))


def test_bad_lists_descriptors_slots_and_rows_are_refused(ghx):
    (s0, _), (t0, _) = _lists()
    neg = s0.copy()
    neg[100] = -1
    one = [(0, 0)]
    _refused([Side(udesc(8), 0, neg)], [Side(udesc(8), 1, t0)], one, "negative local index")
    _refused([Side(udesc(8), 0, s0)], [Side(udesc(8), 1, neg)], one, "negative local index")
    _refused([Side(udesc(0), 0, s0)], [Side(udesc(0), 1, t0)], one, "bad unstructured data descriptor")
    _refused([Side(udesc(8, 0), 0, s0)], [Side(udesc(8, 0), 1, t0)], one, "bad unstructured data descriptor")
    _refused([Side(udesc(8), -1, s0)], [Side(udesc(8), 1, t0)], one, "negative slot")
    _refused([Side(udesc(8), 0, s0)], [Side(udesc(8), -3, t0)], one, "negative slot")
    _refused([Side(udesc(8), 0, s0)], [Side(udesc(8), 1, t0)], [(-1, 0)], "negative slot")
    limit = "at most 64 field and 64 buffer slots"
    _refused([Side(udesc(8), 64, s0)], [Side(udesc(8), 1, t0)], one, limit)
    _refused([Side(udesc(8), 0, s0)], [Side(udesc(8), 64, t0)], one, limit)
    _refused([Side(udesc(8), 0, s0)], [Side(udesc(8), 1, t0)], [(64, 0)], limit)
    US.destroy(US.create([Side(udesc(8), 63, s0)], [Side(udesc(8), 62, t0)], [(63, 0)]))
    _refused([Side(udesc(1 << 20, 1025), 0, s0)], [Side(udesc(1 << 20, 1025), 1, t0)], one,
             "row of more than 1 GiB")
    L = ghx.lib()
    assert L.ghx_uself_create(None, None, 1, ctypes.byref(ctypes.c_void_p())) == -1
    assert L.ghx_uself_create(None, None, 0, None) == -1


def test_a_cell_that_is_source_and_target_is_refused(ghx):
    (s0, s1), (t0, t1) = _lists()
    both = "both a source and a target"
    hit = t0.copy()
    hit[40] = s0[200]
    # within one message, and across two messages of the same field slot
    _refused([Side(udesc(8), 0, s0)], [Side(udesc(8), 0, hit)], [(0, 0)], both)
    hit1 = t1.copy()
    hit1[3] = s0[7]
    _refused([Side(udesc(8), 2, s0), Side(udesc(8), 1, s1)],
             [Side(udesc(8), 1, t0), Side(udesc(8), 2, hit1)], [(0, 0), (1, 0)], both)
    # the same lids in different field slots are different cells
    US.destroy(US.create([Side(udesc(8), 0, s0)], [Side(udesc(8), 1, s0)], [(0, 0)]))
    # and one slot may be source and target on disjoint cells
    US.destroy(US.create([Side(udesc(8), 0, s0)], [Side(udesc(8), 0, t0)], [(0, 0)]))


def test_a_target_cell_that_appears_twice_is_refused(ghx):
    (s0, s1), (t0, t1) = _lists()
    twice = "target cell of a field slot appears twice"
    dup = t0.copy()
    dup[5] = dup[250]
    _refused([Side(udesc(8), 0, s0)], [Side(udesc(8), 1, dup)], [(0, 0)], twice)
    dup1 = t1.copy()
    dup1[0] = t0[300]
    _refused([Side(udesc(8), 0, s0), Side(udesc(8), 0, s1)],
             [Side(udesc(8), 1, t0), Side(udesc(8), 1, dup1)], [(0, 0), (1, 0)], twice)
    # in another field slot it is another cell; source lids may repeat
    US.destroy(US.create([Side(udesc(8), 0, s0), Side(udesc(8), 0, s1)],
                         [Side(udesc(8), 1, t0), Side(udesc(8), 2, dup1)], [(0, 0), (1, 0)]))
    rep = s0.copy()
    rep[1:200:7] = rep[0]
    US.destroy(US.create([Side(udesc(8), 0, rep)], [Side(udesc(8), 1, t0)], [(0, 0)]))


# ---------------------------------------------------------------------------------------------
# planner facts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sd, dd, mode, row", [
    (udesc(8, 1), udesc(8, 1), 0, 8),
    (udesc(4, 3), udesc(4, 3), 0, 12),
    (udesc(4, 3, index_stride=5), udesc(4, 3), 0, 12),
    (udesc(4, 3), udesc(4, 3, index_stride=1, level_stride=UC.N_CELLS), 1, 4),
    (udesc(4, 3, index_stride=1, level_stride=UC.N_CELLS), udesc(4, 3), 1, 4),
    (udesc(8, 3, first=False), udesc(8, 3, first=False), 2, 8),
    (udesc(2, 4, first=False), udesc(2, 4, first=False, level_stride=UC.N_CELLS + 5), 2, 2),
])
def test_mode_per_side_pairing_and_the_buffer_place(ghx, sd, dd, mode, row):
    seg = _one(sd, dd, off=4096)
    assert (seg.mode, seg.row_bytes) == (mode, row)
    assert seg.bytes == 301 * sd.levels * sd.elem_size and seg.n == 301
    assert (seg.src_slot, seg.dst_slot, seg.buf_slot, seg.buf_off) == (0, 1, 0, 4096)
    assert seg.tile_bytes % seg.row_bytes == 0          # tiles are whole rows
    # the same two sides as a put: the same decomposition
    (s0,), (t0,) = _lists(0, (301,))
    h = UC.create([Side(sd, 0, s0)], [Side(dd, 0, t0)])
    put = UC.segments(h)[0]
    UC.destroy(h)
    for f in ("mode", "row_bytes", "bytes", "tile_bytes", "wlog2", "src_index_stride_b",
              "dst_index_stride_b", "src_level_stride_b", "dst_level_stride_b"):
        assert getattr(seg, f) == getattr(put, f), f


@pytest.mark.parametrize("off, w", [(0, 4), (16, 4), (8, 3), (4, 2), (2, 1), (1, 0), (48, 4), (24, 3)])
def test_wlog2_narrowed_by_the_buffer_offset_alone(ghx, off, w):
    assert _one(udesc(16), udesc(16), off=off).wlog2 == w
    assert _one(udesc(8, 2, first=False), udesc(8, 2, first=False), off=off).wlog2 == min(w, 3)


def test_run_flags_are_per_side(ghx):
    rng = np.random.default_rng(4)
    scattered = UC.draw_lists(rng, (400,))[0]
    runs = np.arange(100, 500, dtype=np.int64)
    for elem in (4, 8):
        dense, padded = udesc(elem), udesc(elem, index_stride=2)
        seg = _one(dense, dense, runs, scattered)
        assert (seg.src_runs, seg.dst_runs) == (2, 1)
        seg = _one(dense, dense, scattered, runs)
        assert (seg.src_runs, seg.dst_runs) == (1, 2)
        seg = _one(padded, dense, runs, runs)
        assert (seg.src_runs, seg.dst_runs) == (0, 2) and seg.mode == 0
        seg = _one(dense, padded, runs, runs)
        assert (seg.src_runs, seg.dst_runs) == (2, 0)
        # a buffer offset that is not a multiple of 16 changes no flag: the launch decides
        seg = _one(dense, dense, runs, runs, off=elem)
        assert (seg.src_runs, seg.dst_runs) == (2, 2)
    ghx.call("ghx_tune", b"urun", 0)
    seg = _one(udesc(4), udesc(4), runs, runs)
    assert (seg.src_runs, seg.dst_runs) == (0, 0)


def test_tiles_are_whole_rows_and_follow_the_knobs(ghx):
    def tile(sd, s=None, t=None):
        (s0,), (t0,) = _lists(5, (3001,))
        h = US.create([Side(sd, 0, s0 if s is None else s)], [Side(sd, 1, t0 if t is None else t)],
                      [(0, 0)])
        seg = US.segments(h)[0]
        nb, ns, nt = US.info(h)
        US.destroy(h)
        assert nb == seg.bytes and ns == 1 and nt == -(-seg.bytes // seg.tile_bytes)
        assert seg.tile_bytes % seg.row_bytes == 0
        return seg.tile_bytes

    runs = np.arange(3001, dtype=np.int64)
    assert tile(udesc(8)) == 512 * 8
    assert tile(udesc(8), runs) == 2048 * 8
    assert tile(udesc(8, 8)) == 16384
    assert tile(udesc(4, 24)) == 16384 - 16384 % 96
    ghx.call("ghx_tune", b"u_tile_rows", 3)
    ghx.call("ghx_tune", b"u_tile_bytes", 1024)
    ghx.call("ghx_tune", b"u_run_tile_rows", 64)
    assert tile(udesc(8)) == 24
    assert tile(udesc(8), runs, runs + 4000) == 64 * 8
    assert tile(udesc(4, 24)) == 1024 - 1024 % 96


def test_segments_keep_slots_places_and_message_order(ghx):
    (s0, s1), (t0, t1) = _lists()
    none = np.zeros(0, dtype=np.int64)
    h = US.create([Side(udesc(8), 5, s0), Side(udesc(8), 0, none), Side(udesc(4, 2), 63, s1)],
                  [Side(udesc(8), 2, t0), Side(udesc(8), 0, none), Side(udesc(4, 2, index_stride=3), 0, t1)],
                  [(3, 0), (3, 8), (1, 24)])
    a, b = US.segments(h)
    assert (a.message, a.src_slot, a.dst_slot, a.buf_slot, a.buf_off, a.n) == (0, 5, 2, 3, 0, 301)
    assert (b.message, b.src_slot, b.dst_slot, b.buf_slot, b.buf_off, b.n) == (2, 63, 0, 1, 24, 17)
    assert US.info(h) == (301 * 8 + 17 * 8, 2, 2)
    # too few pointers are refused before anything is launched
    L = ghx.lib()
    one = ghx.ptr_array([4096])
    assert L.ghx_uself_execute(h, one, 1, one, 1, None) == -1
    assert b"do not cover" in L.ghx_last_error()
    info = ghx.USelfSegmentInfo()
    assert L.ghx_uself_segment(h, 2, ctypes.byref(info)) == -1
    assert L.ghx_uself_segment(h, -1, ctypes.byref(info)) == -1
    assert L.ghx_uself_segment(h, 0, None) == -1
    US.destroy(h)
    h = US.create([], [], [])
    assert US.segments(h) == [] and US.info(h) == (0, 0, 0)
    assert L.ghx_uself_execute(h, one, 1, one, 1, None) == 0   # nothing to do
    US.destroy(h)


@pytest.mark.parametrize("levels, first, n, pieces", [(1, True, 1 << 21, 2), (3, True, 1 << 19, 2),
                                                      (2, False, 1 << 20, 2), (2, False, 1 << 21, 4),
                                                      (1, True, 1000, 1)])
def test_long_lists_split_identically_on_both_sides_and_in_the_buffer(ghx, levels, first, n, pieces):
    s = np.arange(n, dtype=np.int64)[::-1].copy()
    t = np.arange(n, dtype=np.int64) * 2
    sd = udesc(1024, levels, first, n_cells=n)
    dd = udesc(1024, levels, first, index_stride=(levels + 1) if first else 1,
               level_stride=1 if first else 2 * n + 3, n_cells=2 * n)
    off = 4096
    h = US.create([Side(sd, 0, s)], [Side(dd, 1, t)], [(0, off)])
    segs = US.segments(h)
    assert US.info(h)[0] == n * levels * 1024
    US.destroy(h)
    hp = UC.create([Side(sd, 0, s)], [Side(dd, 0, t)])
    puts = UC.segments(hp)
    UC.destroy(hp)
    assert len(segs) == pieces == len(puts)
    covered = np.zeros(n * levels, dtype=np.int32)   # per message element of the buffer
    for g, p in zip(segs, puts):
        for f in ("first_index", "n", "bytes", "mode", "row_bytes", "src_field_off", "dst_field_off"):
            assert getattr(g, f) == getattr(p, f), f
        assert g.bytes <= 1 << 30 and g.buf_slot == 0
        if not first and pieces > 1:
            lev = g.src_field_off // g.src_level_stride_b
            assert g.dst_field_off == lev * g.dst_level_stride_b
            want = off + (lev * n + g.first_index) * 1024     # buf[i + l*n]
        else:
            want = off + g.first_index * levels * 1024        # buf[i*L + l]
        assert g.buf_off == want
        e0 = (g.buf_off - off) // 1024
        covered[e0:e0 + g.bytes // 1024] += 1
    assert (covered == 1).all()


# ---------------------------------------------------------------------------------------------
# packed(): the NumPy form of the message against the oracle's unstructured pack
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [udesc(8), udesc(4, 3), udesc(4, 3, index_stride=5),               # mode 0
                               udesc(4, 3, index_stride=1, level_stride=UC.N_CELLS),              # mode 1
                               udesc(8, 2, index_stride=4, level_stride=2),
                               udesc(8, 3, first=False), udesc(3, 2, first=False),                # mode 2
                               udesc(2, 4, first=False, level_stride=UC.N_CELLS + 5)],
                         ids=lambda d: f"e{d.elem_size}-l{d.levels}-f{d.levels_first}-{d.index_stride}-{d.level_stride}")
def test_packed_equals_the_oracles_pack(ghx, d):
    from oracle import oracle as orc
    rng = np.random.default_rng(11)
    lids = UC.draw_lists(rng, (301,))[0]
    lids[5] = lids[200]
    vals = rng.integers(0, 256, size=UC.span_bytes(d), dtype=np.uint8)
    side = Side(d, 0, lids)
    nb = US.message_bytes(side)
    off = 24
    got = US.packed(vals, side, off, np.full(off + nb + 8, 0xC3, dtype=np.uint8))
    want = np.full(off + nb + 8, 0xC3, dtype=np.uint8)
    orc.unstructured_get(vals, want, d.elem_size, lids, d.levels, bool(d.levels_first),
                         d.index_stride, d.level_stride, byte_offset=off)
    np.testing.assert_array_equal(got, want)
    assert (got[:off] == 0xC3).all() and (got[off + nb:] == 0xC3).all()
    # and the planner's row r sits at buffer_offset + r * row_bytes in that layout
    seg = _one(d, d, lids, UC.draw_lists(rng, (301,))[0] + UC.N_CELLS, off=off)
    assert (seg.buf_off, seg.bytes) == (off, nb)


# ---------------------------------------------------------------------------------------------
# exchanges built from patterns
# ---------------------------------------------------------------------------------------------
def _uitem(ghx, pc, local_index, d, align=None):
    it = ghx.ExchangeItem()
    it.pattern, it.local_index, it.kind, it.udata = pc.handle, local_index, 1, d
    it.align, it.tag_offset = align or d.elem_size, 0
    return it


def _self_info(ghx, plan):
    f, s, t = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    ghx.call("ghx_uexchange_self_info", plan.h, ctypes.byref(f), ctypes.byref(s), ctypes.byref(t))
    why = (ghx.lib().ghx_last_error() or b"").decode()
    return f.value, s.value, t.value, why


def _known_answer_domains(golden_dir):
    with open(os.path.join(golden_dir, "unstructured_case.json")) as fh:
        case = json.load(fh)
    return [(r, case["domains"][str(r)]["gids"], case["domains"][str(r)]["halo_lids"]) for r in range(4)]


def _plan(ghx, per_rank, rank, levels=3, extra=()):
    from ghex_amd.communication_object import _ExchangePlan
    from tests.gpu_util import unstructured_patterns
    dds, pc = unstructured_patterns(per_rank)[rank]
    items = [_uitem(ghx, pc, pc.local_index(dd.domain_id()), udesc(8, levels, n_cells=dd.size()))
             for dd in dds]
    plan = _ExchangePlan(items + list(extra))
    plan._keep = (dds, pc)
    return plan


def test_known_answer_case_on_one_rank_is_fusable(ghx, golden_dir):
    doms = _known_answer_domains(golden_dir)
    plan = _plan(ghx, [doms], 0)
    fus, ns, nt, _ = _self_info(ghx, plan)
    assert fus == 1 and ns > 0 and nt == ns     # tiny messages: one tile each
    assert len(plan.send) == len(plan.recv) > 0
    assert ns == sum(1 for _ in plan.send)      # one field per domain: one message per buffer
    # the other fused forms report what they reported before
    f = ctypes.c_int32(-1)
    ghx.call("ghx_exchange_self_fusable", plan.h, ctypes.byref(f))
    assert f.value == 0
    ghx.call("ghx_exchange_mixed", plan.h, ctypes.byref(f))
    assert f.value == 0
    ghx.call("ghx_cs_self_info", plan.h, ctypes.byref(f), None, None, None)
    assert f.value == 0 and b"not a cubed-sphere exchange" in ghx.lib().ghx_last_error()
    # no device needed to ask; executing without buffers is refused
    assert ghx.lib().ghx_uexchange_self(plan.h, None, 0, None, 0, None) == -1


def test_fused_launch_is_refused_on_double_buffered_send_buffers(ghx, golden_dir):
    plan = _plan(ghx, [_known_answer_domains(golden_dir)], 0)
    n = len(plan.send)
    word = ctypes.c_uint64(0)
    offsets = (ctypes.c_int64 * n)(*([256] * n))
    ghx.call("ghx_exchange_set_parity", plan.h, 0, ctypes.addressof(word), 0, offsets, n)
    ptrs = ghx.ptr_array([4096] * max(n, 4))
    L = ghx.lib()
    assert L.ghx_uexchange_self(plan.h, ptrs, 4, ptrs, n, None) == -1
    assert b"double-buffered" in L.ghx_last_error()
    assert _self_info(ghx, plan)[0] == 1          # still fusable; parity is a launch-time state
    ghx.call("ghx_exchange_set_parity", plan.h, 0, None, 0, None, 0)


def test_exchange_with_a_peer_is_not_fusable(ghx, golden_dir):
    doms = _known_answer_domains(golden_dir)
    plan = _plan(ghx, [doms[:2], doms[2:]], 0)
    fus, ns, nt, why = _self_info(ghx, plan)
    assert (fus, ns, nt) == (0, 0, 0) and "peer messages" in why
    one = ghx.ptr_array([4096])
    assert ghx.lib().ghx_uexchange_self(plan.h, one, 1, one, 1, None) == -1
    assert b"peer messages" in ghx.lib().ghx_last_error()


def test_exchange_with_no_message_is_not_fusable(ghx):
    plan = _plan(ghx, [[(0, [1, 2, 3], []), (1, [7, 8, 9], [])]], 0)
    assert plan.send == [] and plan.recv == []
    fus, _, _, why = _self_info(ghx, plan)
    assert fus == 0 and "no message" in why


def test_structured_next_to_unstructured_is_not_fusable(ghx, golden_dir):
    import ghex_amd
    from ghex_amd.structured import regular as R
    ctx = ghex_amd.make_context()
    N, Hw = 6, 1
    E = N + 2 * Hw
    sdd = R.DomainDescriptor(0, (0, 0, 0), (N - 1,) * 3)
    spc = R.make_pattern(ctx, R.HaloGenerator((0, 0, 0), (N - 1,) * 3, (Hw,) * 6, (True,) * 3), [sdd])
    fd = ghx.FieldDesc()
    fd.dim, fd.elem_size = 3, 8
    for d in range(3):
        fd.layout[d], fd.offsets[d], fd.extents[d] = 2 - d, Hw, E
    fd.byte_strides[0], fd.byte_strides[1], fd.byte_strides[2] = 8, 8 * E, 8 * E * E
    fd.num_components, fd.has_components = 1, 0
    it = ghx.ExchangeItem()
    it.pattern, it.local_index, it.kind, it.field = spc.handle, 0, 0, fd
    it.align, it.tag_offset = 8, 100
    plan = _plan(ghx, [_known_answer_domains(golden_dir)], 0, extra=[it])
    plan._keep += (spc,)
    fus, _, _, why = _self_info(ghx, plan)
    assert fus == 0 and "structured items" in why


def test_exchange_of_more_than_64_buffers_is_not_fusable(ghx):
    """Nine domains on one rank, each with a halo cell of every other: 72 domain-pair buffers."""
    def all_to_all(nd):
        doms = []
        for k in range(nd):
            inner = [100 * k + j for j in range(nd)]
            halo = [100 * o + k for o in range(nd) if o != k]
            doms.append((k, inner + halo, list(range(nd, nd + len(halo)))))
        return doms

    plan = _plan(ghx, [all_to_all(9)], 0, levels=1)
    assert len(plan.send) == 72
    fus, _, _, why = _self_info(ghx, plan)
    assert fus == 0 and "at most 64 field and 64 buffer slots" in why
    # eight domains: 56 buffers, one launch
    plan = _plan(ghx, [all_to_all(8)], 0, levels=1)
    assert len(plan.send) == 56 and _self_info(ghx, plan)[0] == 1
