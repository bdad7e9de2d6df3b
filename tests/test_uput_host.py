"""Index-list put plans (ghx_uput_create) without a device: what the planner decides per segment
(ghx_uput_segment), the proof of the pairing — the record's addressing decoded with NumPy equals
the definition's element enumeration — every refusal, the split of lists beyond 2^30 bytes, the
bulk object's chunking by field kind, and the new handle under the other put entry points."""
import ctypes

import numpy as np
import pytest

from tests import uput_cases as UC
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
    rng = np.random.default_rng(seed)
    return UC.draw_lists(rng, sizes), UC.draw_lists(rng, sizes)


def _one(sd, dd, s=None, t=None, n=301, seed=0):
    """The single segment of a one-message plan, with its two sides."""
    rng = np.random.default_rng(seed)
    s = UC.draw_lists(rng, (n,))[0] if s is None else s
    t = UC.draw_lists(rng, (n,))[0] if t is None else t
    src, dst = Side(sd, 0, s), Side(dd, 0, t)
    h = UC.create([src], [dst])
    segs = UC.segments(h)
    UC.destroy(h)
    assert len(segs) == 1
    return segs[0], src, dst


# ---------------------------------------------------------------------------------------------
# planner facts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sd, dd, mode, row", [
    # levels contiguous on both sides: one row per index
    (udesc(8, 1), udesc(8, 1), 0, 8),
    (udesc(4, 3), udesc(4, 3), 0, 12),
    (udesc(4, 3, index_stride=5), udesc(4, 3), 0, 12),          # padded against unpadded
    (udesc(4, 3), udesc(4, 3, index_stride=7), 0, 12),          # and the reverse
    # one side's levels strided: rows of one element, index-major
    (udesc(4, 3), udesc(4, 3, index_stride=1, level_stride=UC.N_CELLS), 1, 4),
    (udesc(4, 3, index_stride=1, level_stride=UC.N_CELLS), udesc(4, 3), 1, 4),
    (udesc(8, 2, index_stride=4, level_stride=2), udesc(8, 2, index_stride=6, level_stride=3), 1, 8),
    # levels last
    (udesc(8, 3, first=False), udesc(8, 3, first=False), 2, 8),
    (udesc(2, 4, first=False), udesc(2, 4, first=False, level_stride=UC.N_CELLS + 5), 2, 2),
])
def test_mode_follows_the_index_list_rule_for_both_sides_together(ghx, sd, dd, mode, row):
    seg, src, dst = _one(sd, dd)
    assert (seg.mode, seg.row_bytes) == (mode, row)
    assert seg.bytes == 301 * sd.levels * sd.elem_size and seg.n == 301
    for side, d in (("src", sd), ("dst", dd)):
        assert getattr(seg, side + "_index_stride_b") == d.index_stride * d.elem_size
        assert getattr(seg, side + "_level_stride_b") == d.level_stride * d.elem_size
        assert getattr(seg, side + "_field_off") == 0
    assert seg.tile_bytes % seg.row_bytes == 0


@pytest.mark.parametrize("sd, dd, w", [
    (udesc(16, 1), udesc(16, 1), 4),
    (udesc(8, 2), udesc(8, 2), 4),
    (udesc(8, 1), udesc(8, 1), 3),
    (udesc(4, 4, index_stride=5), udesc(4, 4), 2),      # the source's index stride (20 B) alone
    (udesc(4, 4), udesc(4, 4, index_stride=6), 3),      # the target's (24 B) alone
    (udesc(8, 2, index_stride=4, level_stride=3), udesc(8, 2, index_stride=4, level_stride=2), 3),
    (udesc(2, 8, first=False, level_stride=UC.N_CELLS), udesc(2, 8, first=False, level_stride=UC.N_CELLS + 1), 1),
    (udesc(3, 1), udesc(3, 1), 0),
    (udesc(12, 1), udesc(12, 1), 2),
])
def test_wlog2_is_the_widest_vector_both_sides_allow(ghx, sd, dd, w):
    assert _one(sd, dd)[0].wlog2 == w


def test_wlog2_ignores_the_index_strides_of_a_single_row(ghx):
    seg, _, _ = _one(udesc(4, 4, index_stride=5), udesc(4, 4, index_stride=7), n=1)
    assert seg.wlog2 == 4


def test_lid64_is_per_side(ghx):
    rng = np.random.default_rng(3)
    s, t = UC.draw_lists(rng, (50,))[0], UC.draw_lists(rng, (50,))[0]
    big = t + (1 << 31)
    for sl, tl, want in ((s, t, (0, 0)), (big, t, (1, 0)), (s, big, (0, 1)), (big, big, (1, 1))):
        seg, _, _ = _one(udesc(8), udesc(8), sl, tl)
        assert (seg.src_lid64, seg.dst_lid64) == want
    # one lid at 2^31 - 1 still fits int32
    edge = s.copy()
    edge[7] = (1 << 31) - 1
    assert _one(udesc(8), udesc(8), edge, t)[0].src_lid64 == 0


def test_run_flags_are_per_side(ghx):
    rng = np.random.default_rng(4)
    scattered = UC.draw_lists(rng, (400,))[0]
    runs = np.arange(100, 500, dtype=np.int64)
    for elem in (4, 8):
        dense, padded = udesc(elem), udesc(elem, index_stride=2)
        seg, _, _ = _one(dense, dense, runs, scattered)
        assert (seg.src_runs, seg.dst_runs) == (2, 1)    # run-heavy source, eligible target
        seg, _, _ = _one(dense, dense, scattered, runs)
        assert (seg.src_runs, seg.dst_runs) == (1, 2)
        seg, _, _ = _one(padded, dense, runs, runs)      # index stride != row: never a run
        assert (seg.src_runs, seg.dst_runs) == (0, 2) and seg.mode == 0
        seg, _, _ = _one(dense, padded, runs, runs)
        assert (seg.src_runs, seg.dst_runs) == (2, 0)
    for sd in (udesc(2), udesc(16), udesc(4, 3), udesc(4, 2, first=False)):
        seg, _, _ = _one(sd, sd, runs, runs)
        assert (seg.src_runs, seg.dst_runs) == (0, 0)
    ghx.call("ghx_tune", b"urun", 0)
    seg, _, _ = _one(udesc(4), udesc(4), runs, runs)
    assert (seg.src_runs, seg.dst_runs) == (0, 0)


def test_tile_sizes_follow_the_index_list_knobs(ghx):
    rng = np.random.default_rng(5)
    scattered = UC.draw_lists(rng, (3001,))[0]
    runs = np.arange(3001, dtype=np.int64)

    def tile(sd, s=scattered, t=scattered):
        src, dst = Side(sd, 0, s), Side(sd, 0, t)
        h = UC.create([src], [dst])
        seg = UC.segments(h)[0]
        nb, nt = UC.put_info(h)
        UC.destroy(h)
        assert nb == seg.bytes and nt == -(-seg.bytes // seg.tile_bytes)
        return seg.tile_bytes

    assert tile(udesc(8)) == 512 * 8                      # short rows: u_tile_rows
    assert tile(udesc(8), runs, scattered) == 2048 * 8    # run-heavy on either side
    assert tile(udesc(8), scattered, runs) == 2048 * 8
    assert tile(udesc(8, 8)) == 16384                     # 64-B rows: u_tile_bytes
    assert tile(udesc(4, 24)) == 16384 - 16384 % 96       # whole rows
    assert tile(udesc(4, 3, first=False)) == 512 * 4
    ghx.call("ghx_tune", b"u_tile_rows", 3)
    ghx.call("ghx_tune", b"u_tile_bytes", 1024)
    ghx.call("ghx_tune", b"u_run_tile_rows", 64)
    assert tile(udesc(8)) == 24
    assert tile(udesc(8), runs, runs) == 64 * 8
    assert tile(udesc(8, 8)) == 1024
    assert tile(udesc(4, 24)) == 1024 - 1024 % 96
    ghx.call("ghx_tune", b"small_row_bytes", 128)
    assert tile(udesc(8, 8)) == 3 * 64                    # 64-B rows are short now


def test_segments_keep_slots_and_message_order(ghx):
    (s0, s1), (t0, t1) = _lists()
    h = UC.create([Side(udesc(8), 5, s0), Side(udesc(4, 2), 63, s1)],
                  [Side(udesc(8), 2, t0), Side(udesc(4, 2, index_stride=3), 0, t1)])
    a, b = UC.segments(h)
    assert (a.message, a.src_slot, a.dst_slot, a.n, a.first_index) == (0, 5, 2, 301, 0)
    assert (b.message, b.src_slot, b.dst_slot, b.n, b.first_index) == (1, 63, 0, 17, 0)
    assert UC.put_info(h)[0] == 301 * 8 + 17 * 8
    UC.destroy(h)


def test_empty_messages_and_empty_plans(ghx):
    none = np.zeros(0, dtype=np.int64)
    (s0, _), (t0, _) = _lists()
    h = UC.create([Side(udesc(8), 0, none), Side(udesc(8), 1, s0)],
                  [Side(udesc(8), 0, none), Side(udesc(8), 1, t0)])
    segs = UC.segments(h)
    assert len(segs) == 1 and segs[0].message == 1
    UC.destroy(h)
    h = UC.create([], [])
    assert UC.segments(h) == [] and UC.put_info(h) == (0, 0)
    # nothing to do: no tables needed, with or without a device
    one = ghx.ptr_array([4096])
    assert ghx.lib().ghx_put_execute(h, one, 1, one, 1, None) == 0
    UC.destroy(h)


# ---------------------------------------------------------------------------------------------
# addressing: the host proof of the pairing
# ---------------------------------------------------------------------------------------------
PAIRINGS = [
    (udesc(8), udesc(8)),
    (udesc(4, 3), udesc(4, 3)),
    (udesc(4, 3, index_stride=5), udesc(4, 3)),
    (udesc(4, 3), udesc(4, 3, index_stride=1, level_stride=UC.N_CELLS)),
    (udesc(4, 3, index_stride=1, level_stride=UC.N_CELLS), udesc(4, 3, index_stride=4)),
    (udesc(8, 2, index_stride=4, level_stride=2), udesc(8, 2, index_stride=6, level_stride=3)),
    (udesc(8, 3, first=False), udesc(8, 3, first=False, level_stride=UC.N_CELLS + 3)),
    (udesc(3, 2, first=False), udesc(3, 2, first=False)),
    (udesc(12, 1, index_stride=2), udesc(12, 1)),
]


@pytest.mark.parametrize("k", range(len(PAIRINGS)))
def test_record_addressing_equals_the_definition(ghx, k):
    sd, dd = PAIRINGS[k]
    rng = np.random.default_rng(10 + k)
    s = UC.draw_lists(rng)
    s[1][5] = s[1][900]  # source lids may repeat
    t = UC.draw_lists(rng)
    srcs = [Side(sd, m, s[m]) for m in range(3)]
    dsts = [Side(dd, 2 - m, t[m]) for m in range(3)]
    h = UC.create(srcs, dsts)
    segs = UC.segments(h)
    UC.destroy(h)
    assert [g.message for g in segs] == [0, 1, 2]
    for g in segs:
        src, dst = srcs[g.message], dsts[g.message]
        assert (g.src_slot, g.dst_slot) == (src.slot, dst.slot)
        got = UC.segment_pairs(g, src, dst, sd.elem_size)
        want = UC.formula_pairs(src, dst)
        np.testing.assert_array_equal(UC.sorted_rows(got), UC.sorted_rows(want))
        # and at the planner's vector width every access stays inside one element row
        w = 1 << g.wlog2
        assert g.row_bytes % w == 0
        fine = UC.segment_pairs(g, src, dst, w)
        assert not (fine % w).any()


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def _refused(srcs, dsts, fragment):
    rc, why, h = UC.try_create(srcs, dsts)
    assert rc == -1 and not h.value, (rc, why)
    assert fragment in why, why


def test_sides_that_differ_are_refused(ghx):
    (s0, s1), (t0, t1) = _lists()
    same = "do not describe the same message bytes"
    _refused([Side(udesc(8), 0, s0)], [Side(udesc(8), 0, t0[:-1])], same)
    _refused([Side(udesc(8), 0, s0)], [Side(udesc(4), 0, t0)], same)
    _refused([Side(udesc(4, 2), 0, s0)], [Side(udesc(4, 3), 0, t0)], same)
    _refused([Side(udesc(4, 2, first=True), 0, s0)], [Side(udesc(4, 2, first=False), 0, t0)], same)
    # the second message is checked like the first
    _refused([Side(udesc(8), 0, s0), Side(udesc(8), 0, s1)],
             [Side(udesc(8), 0, t0), Side(udesc(2), 0, t1)], same)


def test_bad_lists_descriptors_and_slots_are_refused(ghx):
    (s0, _), (t0, _) = _lists()
    neg = s0.copy()
    neg[100] = -1
    _refused([Side(udesc(8), 0, neg)], [Side(udesc(8), 0, t0)], "negative local index")
    _refused([Side(udesc(8), 0, s0)], [Side(udesc(8), 0, neg)], "negative local index")
    _refused([Side(udesc(0), 0, s0)], [Side(udesc(0), 0, t0)], "bad unstructured data descriptor")
    _refused([Side(udesc(8, 0), 0, s0)], [Side(udesc(8, 0), 0, t0)], "bad unstructured data descriptor")
    _refused([Side(udesc(8), -1, s0)], [Side(udesc(8), 0, t0)], "negative slot")
    _refused([Side(udesc(8), 0, s0)], [Side(udesc(8), -3, t0)], "negative slot")
    _refused([Side(udesc(8), 64, s0)], [Side(udesc(8), 0, t0)], "at most 64 source and 64 target")
    _refused([Side(udesc(8), 0, s0)], [Side(udesc(8), 64, t0)], "at most 64 source and 64 target")
    _refused([Side(udesc(1 << 20, 1025), 0, s0)], [Side(udesc(1 << 20, 1025), 0, t0)],
             "row of more than 1 GiB")
    L = ghx.lib()
    assert L.ghx_uput_create(None, None, 1, ctypes.byref(ctypes.c_void_p())) == -1
    assert L.ghx_uput_create(None, None, 0, None) == -1


# ---------------------------------------------------------------------------------------------
# lists beyond 2^30 bytes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels, first, n, pieces", [(1, True, 1 << 21, 2), (3, True, 1 << 19, 2),
                                                      (2, False, 1 << 20, 2), (2, False, 1 << 21, 4),
                                                      (1, True, 1000, 1)])
def test_long_lists_split_identically_on_both_sides(ghx, levels, first, n, pieces):
    """1-KiB elements make a list of 2^20 indices one GiB (as tests/test_host.py does for
    ghx_uplan_create): index ranges in general, level by level for a levels-last list."""
    s = np.arange(n, dtype=np.int64)[::-1].copy()
    t = np.arange(n, dtype=np.int64) * 2
    sd = udesc(1024, levels, first, n_cells=n)
    dd = udesc(1024, levels, first, index_stride=(levels + 1) if first else 1,
               level_stride=1 if first else 2 * n + 3, n_cells=2 * n)
    src, dst = Side(sd, 0, s), Side(dd, 0, t)
    h = UC.create([src], [dst])
    segs = UC.segments(h)
    assert UC.put_info(h)[0] == n * levels * 1024
    UC.destroy(h)
    assert len(segs) == pieces and sum(g.bytes for g in segs) == n * levels * 1024
    assert all(g.bytes <= 1 << 30 for g in segs)
    covered = np.zeros((levels, n), dtype=np.int32)
    for g in segs:
        if not first and pieces > 1:
            # one level of the list: a mode-0 segment of element rows at that level's offset
            assert g.mode == 0 and g.row_bytes == 1024
            lev = g.src_field_off // g.src_level_stride_b
            assert g.src_field_off == lev * g.src_level_stride_b
            assert g.dst_field_off == lev * g.dst_level_stride_b
            covered[lev, g.first_index:g.first_index + g.n] += 1
        else:
            assert (g.src_field_off, g.dst_field_off) == (0, 0)
            covered[:, g.first_index:g.first_index + g.n] += 1
        # the first and last row of the piece address what the definition says
        for i in (0, g.n - 1):
            so = g.src_field_off + s[g.first_index + i] * g.src_index_stride_b
            to = g.dst_field_off + t[g.first_index + i] * g.dst_index_stride_b
            lev = 0 if first else g.src_field_off // g.src_level_stride_b
            assert so == (s[g.first_index + i] * sd.index_stride + lev * sd.level_stride) * 1024
            assert to == (t[g.first_index + i] * dd.index_stride + lev * dd.level_stride) * 1024
    assert (covered == 1).all()


# ---------------------------------------------------------------------------------------------
# the bulk object's chunking, the handle under the other entry points
# ---------------------------------------------------------------------------------------------
def test_put_chunks_cut_at_a_change_of_kind(ghx):
    from ghex_amd import bulk_communication_object as B
    box = [((0, 0, 0), (1, 1, 1))]
    lids = np.arange(4, dtype=np.int64)
    s = lambda k, t: (k, box, (0, t), box)       # noqa: E731
    u = lambda k, t: (k, lids, (0, t), lids)     # noqa: E731
    assert B.message_kind(s(0, 0)) == 0 and B.message_kind(u(0, 0)) == 1
    msgs = [s(0, 0), s(0, 1), u(1, 2), u(1, 3), u(2, 2), s(3, 4)]
    chunks = B.put_chunks(msgs)
    assert [[B.message_kind(m) for m in c] for c, _, _ in chunks] == [[0, 0], [1, 1, 1], [0]]
    assert [srcs for _, srcs, _ in chunks] == [[0], [1, 2], [3]]
    assert [dsts for _, _, dsts in chunks] == [[(0, 0), (0, 1)], [(0, 2), (0, 3)], [(0, 4)]]
    # one kind alone is cut at 64 messages, as before
    many = B.put_chunks([u(0, t) for t in range(70)])
    assert [len(c) for c, _, _ in many] == [64, 6]


def test_uput_entries_carry_descriptors_slots_and_lists(ghx):
    from ghex_amd import bulk_communication_object as B
    sd, dd = udesc(8, 2), udesc(8, 2, index_stride=3)
    allr = [{"fields": [{"desc": bytes(dd), "kind": 1}]}]
    s, t = np.array([4, 2, 9], dtype=np.int64), np.array([11, 12, 13], dtype=np.int64)
    src, dst, keep = B.uput_entries([(1, s, (0, 0), t)], [1], [(0, 0)], [None, sd], allr)
    assert (src[0].field_slot, dst[0].field_slot, src[0].n_lids, dst[0].n_lids) == (0, 0, 3, 3)
    assert list(src[0].lids[:3]) == [4, 2, 9] and list(dst[0].lids[:3]) == [11, 12, 13]
    assert (src[0].data.index_stride, dst[0].data.index_stride) == (2, 3)
    h = ctypes.c_void_p()
    ghx.call("ghx_uput_create", src, dst, 1, ctypes.byref(h))
    assert UC.put_info(h)[0] == 3 * 16
    UC.destroy(h)


def test_the_other_put_entry_points_take_the_new_handle(ghx):
    (s0, s1), (t0, t1) = _lists()
    h = UC.create([Side(udesc(8), 0, s0), Side(udesc(4, 16), 1, s1)],
                  [Side(udesc(8), 1, t0), Side(udesc(4, 16), 0, t1)])
    nb, nt = UC.put_info(h)
    assert nb == 301 * 8 + 17 * 64 and nt == 2
    p, r, x = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    ghx.call("ghx_cs_put_info", h, ctypes.byref(p), ctypes.byref(r), ctypes.byref(x))
    assert (p.value, r.value, x.value) == (nt, 0, 0)
    # too few pointers are refused before anything is launched
    L = ghx.lib()
    one = ghx.ptr_array([4096])
    assert L.ghx_put_execute(h, one, 1, one, 1, None) == -1
    assert b"do not cover" in L.ghx_last_error()
    UC.destroy(h)


def test_uput_segment_refuses_a_structured_put(ghx):
    L = ghx.lib()
    h = ctypes.c_void_p()
    ghx.call("ghx_put_create", None, 0, None, 0, ctypes.byref(h))
    info = ghx.UPutSegmentInfo()
    assert L.ghx_uput_segment(h, 0, ctypes.byref(info)) == -1
    assert b"not a put of ghx_uput_create" in L.ghx_last_error()
    assert L.ghx_put_destroy(h) == 0
    assert L.ghx_uput_segment(None, 0, ctypes.byref(info)) == -1
    (s0, _), (t0, _) = _lists()
    h = UC.create([Side(udesc(8), 0, s0)], [Side(udesc(8), 0, t0)])
    assert L.ghx_uput_segment(h, 1, ctypes.byref(info)) == -1
    assert L.ghx_uput_segment(h, -1, ctypes.byref(info)) == -1
    assert L.ghx_uput_segment(h, 0, None) == -1
    UC.destroy(h)


def test_bulk_object_takes_unstructured_fields_in_its_plain_mode_only(ghx):
    from ghex_amd import bulk_communication_object as B

    class F:
        kind = 1

    class BI:
        field = F()

    bco = B.BulkCommunicationObject(None)
    bco.add_field(BI())
    assert len(bco._bis) == 1
    with pytest.raises(ValueError, match="cubed-sphere fields only"):
        B.BulkCommunicationObject(None, cubed_sphere=True).add_field(BI())
    F.kind = 2
    with pytest.raises(TypeError):
        B.BulkCommunicationObject(None).add_field(BI())
