"""The index-list pack that also completes the self messages (ghx_umixed_create,
ghx_uexchange_mixed_info) without a device: every refusal with its reason, the counts and the
peer segments against ghx_uself_create's plan of the self part and ghx_uplan_create's pack plan of
the peer part, and which exchanges built from patterns are planned in the mixed form."""
import ctypes

import numpy as np
import pytest

from tests import umixed_cases as UM
from tests import uput_cases as UC
from tests import uself_cases as US
from tests.test_uself_host import _known_answer_domains, _plan, _self_info
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


def _lists(seed=0):
    """Self source, self target, two peer source lists: all disjoint (one draw)."""
    rng = np.random.default_rng(seed)
    return UC.draw_lists(rng, (301, 301, 257, 17))


def _refused(fragment, srcs, dsts, places, peers, peer_places, dst_places=None):
    rc, why, h = UM.try_create(srcs, dsts, places, peers, peer_places, dst_places)
    assert rc == -1 and not h.value, (rc, why)
    assert fragment in why, why


def _accepted(srcs, dsts, places, peers, peer_places):
    US.destroy(UM.create(srcs, dsts, places, peers, peer_places))


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_a_plan_without_self_or_without_peer_messages_is_refused(ghx):
    s, t, p, _ = _lists()
    d = udesc(8)
    _refused("no self message", [], [], [], [Side(d, 0, p)], [(0, 0)])
    _refused("no peer message", [Side(d, 0, s)], [Side(d, 1, t)], [(0, 0)], [], [])
    L = ghx.lib()
    assert L.ghx_umixed_create(None, None, 1, None, 1, ctypes.byref(ctypes.c_void_p())) == -1
    assert L.ghx_umixed_create(None, None, 0, None, 0, None) == -1


def test_a_slot_of_64_is_refused_on_either_part(ghx):
    s, t, p, _ = _lists()
    d = udesc(8)
    one, self_limit = [(0, 0)], "at most 64 field and 64 buffer slots"
    peer_limit = "peer message's field or buffer slot is 64 or more"
    _refused(peer_limit, [Side(d, 0, s)], [Side(d, 1, t)], one, [Side(d, 64, p)], [(1, 0)])
    _refused(peer_limit, [Side(d, 0, s)], [Side(d, 1, t)], one, [Side(d, 0, p)], [(64, 0)])
    _refused("negative slot", [Side(d, 0, s)], [Side(d, 1, t)], one, [Side(d, -1, p)], [(1, 0)])
    _refused("negative slot", [Side(d, 0, s)], [Side(d, 1, t)], one, [Side(d, 0, p)], [(-2, 0)])
    _refused(self_limit, [Side(d, 64, s)], [Side(d, 1, t)], one, [Side(d, 0, p)], [(1, 0)])
    _refused(self_limit, [Side(d, 0, s)], [Side(d, 1, t)], [(64, 0)], [Side(d, 0, p)], [(1, 0)])
    _accepted([Side(d, 63, s)], [Side(d, 62, t)], [(62, 0)], [Side(d, 63, p)], [(63, 0)])


def test_a_peer_range_that_overlaps_another_message_is_refused(ghx):
    s, t, p, q = _lists()
    d = udesc(8)
    me = ([Side(d, 0, s)], [Side(d, 1, t)], [(0, 64)])
    why = "a peer message overlaps another message in one buffer"
    # a self range: from below, from inside, its last byte
    _refused(why, *me, [Side(d, 0, p)], [(0, 0)])          # 257 * 8 > 64
    _refused(why, *me, [Side(d, 0, q)], [(0, 64 + 800)])
    _refused(why, *me, [Side(d, 0, q)], [(0, 64 + 301 * 8 - 1)])
    # another peer range
    _refused(why, *me, [Side(d, 0, p), Side(d, 0, q)], [(1, 0), (1, 257 * 8 - 8)])
    _refused(why, *me, [Side(d, 0, p), Side(d, 0, q)], [(1, 16), (1, 0)])
    # back to back, behind a pad gap, in another buffer: fine
    _accepted(*me, [Side(d, 0, q)], [(0, 64 + 301 * 8)])
    _accepted(*me, [Side(d, 0, q[:8])], [(0, 0)])           # ends where the self message begins
    _accepted(*me, [Side(d, 0, p), Side(d, 0, q)], [(1, 0), (1, 257 * 8 + 40)])


def test_a_self_target_cell_that_is_a_peer_source_is_refused(ghx):
    s, t, p, q = _lists()
    d = udesc(8)
    why = "target cell of a self message is a source cell of a peer message"
    hit = p.copy()
    hit[100] = t[7]
    _refused(why, [Side(d, 0, s)], [Side(d, 1, t)], [(0, 0)], [Side(d, 1, hit)], [(1, 0)])
    hit2 = q.copy()
    hit2[-1] = t[300]
    _refused(why, [Side(d, 0, s)], [Side(d, 1, t)], [(0, 0)], [Side(d, 0, p), Side(d, 1, hit2)],
             [(1, 0), (2, 0)])
    # the same lid on a different field slot is another cell
    _accepted([Side(d, 0, s)], [Side(d, 1, t)], [(0, 0)], [Side(d, 0, hit)], [(1, 0)])
    _accepted([Side(d, 0, s)], [Side(d, 1, t)], [(0, 0)], [Side(d, 2, t)], [(1, 0)])
    # a peer may send the cells a self message sends, and cells of the receiving field it does not write
    _accepted([Side(d, 0, s)], [Side(d, 1, t)], [(0, 0)], [Side(d, 0, s), Side(d, 1, p)], [(1, 0), (2, 0)])


def _self_refusals():
    s, t, p, q = _lists()
    d = udesc(8)
    neg = s.copy()
    neg[100] = -1
    hit = t.copy()
    hit[40] = s[200]
    dup = t.copy()
    dup[5] = dup[250]
    same = "do not describe the same message bytes"
    return [
        (same, [Side(d, 0, s)], [Side(d, 1, t[:-1])], [(0, 0)], None),
        (same, [Side(d, 0, s)], [Side(udesc(4), 1, t)], [(0, 0)], None),
        (same, [Side(udesc(4, 2), 0, s)], [Side(udesc(4, 3), 1, t)], [(0, 0)], None),
        (same, [Side(udesc(4, 2, first=True), 0, s)], [Side(udesc(4, 2, first=False), 1, t)], [(0, 0)], None),
        ("differ in buffer slot or buffer offset", [Side(d, 0, s)], [Side(d, 1, t)], [(0, 0)], [(2, 0)]),
        ("differ in buffer slot or buffer offset", [Side(d, 0, s)], [Side(d, 1, t)], [(0, 0)], [(0, 8)]),
        ("two messages overlap in one buffer", [Side(d, 0, s), Side(d, 0, q)], [Side(d, 1, t), Side(d, 2, q)],
         [(0, 0), (0, 301 * 8 - 8)], None),
        ("negative local index", [Side(d, 0, neg)], [Side(d, 1, t)], [(0, 0)], None),
        ("negative local index", [Side(d, 0, s)], [Side(d, 1, neg)], [(0, 0)], None),
        ("bad unstructured data descriptor", [Side(udesc(0), 0, s)], [Side(udesc(0), 1, t)], [(0, 0)], None),
        ("bad unstructured data descriptor", [Side(udesc(8, 0), 0, s)], [Side(udesc(8, 0), 1, t)], [(0, 0)], None),
        ("negative slot", [Side(d, -1, s)], [Side(d, 1, t)], [(0, 0)], None),
        ("negative slot", [Side(d, 0, s)], [Side(d, 1, t)], [(-1, 0)], None),
        ("at most 64 field and 64 buffer slots", [Side(d, 0, s)], [Side(d, 64, t)], [(0, 0)], None),
        ("row of more than 1 GiB", [Side(udesc(1 << 20, 1025), 0, s)], [Side(udesc(1 << 20, 1025), 1, t)],
         [(0, 0)], None),
        ("both a source and a target", [Side(d, 0, s)], [Side(d, 0, hit)], [(0, 0)], None),
        ("target cell of a field slot appears twice", [Side(d, 0, s)], [Side(d, 1, dup)], [(0, 0)], None),
    ], Side(d, 3, p)


def test_every_refusal_of_the_self_plan_is_still_raised(ghx):
    cases, peer = _self_refusals()
    for fragment, srcs, dsts, places, dst_places in cases:
        # ghx_uself_create refuses the self part alone for this reason, and so does the mixed plan
        rc, why, h = US.try_create(srcs, dsts, places, dst_places)
        assert rc == -1 and fragment in why, (fragment, why)
        _refused(fragment, srcs, dsts, places, [peer], [(5, 0)], dst_places)


def test_bad_peer_lists_and_descriptors_are_refused(ghx):
    s, t, p, _ = _lists()
    d = udesc(8)
    neg = p.copy()
    neg[3] = -1
    me = ([Side(d, 0, s)], [Side(d, 1, t)], [(0, 0)])
    _refused("negative local index", *me, [Side(d, 0, neg)], [(1, 0)])
    _refused("bad unstructured data descriptor", *me, [Side(udesc(0), 0, p)], [(1, 0)])
    _refused("row of more than 1 GiB", *me, [Side(udesc(1 << 20, 1025), 0, p)], [(1, 0)])


# ---------------------------------------------------------------------------------------------
# counts and segments: the self part is ghx_uself_create's, the peer part ghx_uplan_create's
# ---------------------------------------------------------------------------------------------
PARTS = [
    # self descriptors (source, target), peer descriptors
    ((udesc(8), udesc(8)), [udesc(8), udesc(4)]),
    ((udesc(4, 3), udesc(4, 3, index_stride=5)), [udesc(8, 3, first=False), udesc(16, 2)]),
    ((udesc(8, 3, first=False), udesc(8, 3, first=False)), [udesc(4, 3, index_stride=1, level_stride=UC.N_CELLS)]),
    ((udesc(3), udesc(3, index_stride=2)), [udesc(12, 2), udesc(1, 5, first=False)]),
]


@pytest.mark.parametrize("knobs", [{}, {"u_tile_rows": 3, "u_tile_bytes": 1024, "u_run_tile_rows": 64},
                                   {"urun": 0}, {"tile_records": 0, "order": 0}],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()) or "default")
@pytest.mark.parametrize("part", range(len(PARTS)))
def test_counts_and_segments_equal_the_two_plans_they_are_made_of(ghx, part, knobs):
    for k, v in knobs.items():
        ghx.call("ghx_tune", k.encode(), v)
    (sd, dd), pds = PARTS[part]
    rng = np.random.default_rng(part)
    s, t, s2, t2, p0, p1 = UC.draw_lists(rng, (3001, 3001, 129, 129, 1031, 257))
    srcs, dsts = [Side(sd, 0, s), Side(sd, 1, s2)], [Side(dd, 2, t), Side(dd, 3, t2)]
    places = [(0, 0), (1, 24)]
    peers = [Side(pd, j, np.sort(l) if j else l) for j, (pd, l) in enumerate(zip(pds, (p0, p1)))]
    peer_places = [(2, 16), (1, 24 + 8192)][:len(peers)]
    h = UM.create(srcs, dsts, places, peers, peer_places)
    hs = US.create(srcs, dsts, places)
    pk = UM.PackPlan(peers, peer_places)
    try:
        sb, ss, st = US.info(hs)
        pb, ps, pt = pk.info()
        assert US.info(h) == (sb + pb, ss + ps, st + pt)
        assert UM.mixed_info(h) == (st, ps, pt)
        assert UM.mixed_info(hs) == (st, 0, 0)        # a plan of ghx_uself_create: all self tiles
        assert st > 0 and pt > 0 and ps == len(peers)
        for a, b in zip(UM.self_segments(h), US.segments(hs)):
            for f, _ in ghx.USelfSegmentInfo._fields_:
                assert getattr(a, f) == getattr(b, f) or f == "n_segments", f
        got, want = UM.peer_segments(h), pk.segments()
        assert len(got) == len(want) == ps
        for a, b in zip(got, want):
            for f in UM.USEG_FIELDS:
                assert getattr(a, f) == getattr(b, f), f
        info = ghx.USegmentInfo()
        L = ghx.lib()
        assert L.ghx_umixed_peer_segment(h, ps, ctypes.byref(info)) == -1
        assert L.ghx_umixed_peer_segment(h, -1, ctypes.byref(info)) == -1
        assert L.ghx_umixed_peer_segment(h, 0, None) == -1
        assert L.ghx_umixed_peer_segment(hs, 0, ctypes.byref(info)) == -1
        assert b"no peer part" in L.ghx_last_error()
        sseg = ghx.USelfSegmentInfo()
        assert L.ghx_uself_segment(h, ss, ctypes.byref(sseg)) == -1   # the self segments only
        # too few pointers are refused before anything is launched
        one = ghx.ptr_array([4096])
        assert L.ghx_uself_execute(h, one, 1, one, 1, None) == -1
        assert b"do not cover" in L.ghx_last_error()
    finally:
        pk.destroy()
        US.destroy(hs)
        US.destroy(h)


@pytest.mark.parametrize("levels, first, n, pieces", [(1, True, 1 << 21, 2), (3, True, 1 << 19, 2),
                                                      (2, False, 1 << 20, 2), (2, False, 1 << 21, 4)])
def test_a_long_peer_list_splits_as_the_pack_plan_splits_it(ghx, levels, first, n, pieces):
    s, t, _, _ = _lists()
    d = udesc(8)
    long = np.arange(n, dtype=np.int64)[::-1].copy() + 20000
    pd = udesc(1024, levels, first, n_cells=n + 20000)
    peers, peer_places = [Side(pd, 0, long)], [(1, 4096)]
    h = UM.create([Side(d, 0, s)], [Side(d, 1, t)], [(0, 0)], peers, peer_places)
    pk = UM.PackPlan(peers, peer_places)
    try:
        got, want = UM.peer_segments(h), pk.segments()
        assert len(got) == len(want) == pieces
        assert UM.mixed_info(h)[1:] == pk.info()[1:]
        assert US.info(h)[0] == 301 * 8 + n * levels * 1024
        for a, b in zip(got, want):
            assert a.bytes <= 1 << 30
            for f in UM.USEG_FIELDS:
                assert getattr(a, f) == getattr(b, f), f
    finally:
        pk.destroy()
        US.destroy(h)


# ---------------------------------------------------------------------------------------------
# exchanges built from patterns
# ---------------------------------------------------------------------------------------------
def _mixed_info(ghx, plan):
    f, s, t = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    ghx.call("ghx_uexchange_mixed_info", plan.h, ctypes.byref(f), ctypes.byref(s), ctypes.byref(t))
    why = (ghx.lib().ghx_last_error() or b"").decode()
    return f.value, s.value, t.value, why


def test_known_answer_case_on_two_ranks_of_two_domains_is_mixed(ghx, golden_dir):
    doms = _known_answer_domains(golden_dir)
    for rank in (0, 1):
        plan = _plan(ghx, [doms[:2], doms[2:]], rank)
        # every domain receives from all three others: per rank 2 self messages, 4 peer sends, 4 peer recvs
        assert sorted(x["rank"] == rank for x in plan.send) == [False] * 4 + [True] * 2
        assert sorted(x["rank"] == rank for x in plan.recv) == [False] * 4 + [True] * 2
        mixed, n_self, n_peer, _ = _mixed_info(ghx, plan)
        assert (mixed, n_self, n_peer) == (1, 2, 4)      # tiny messages: one tile each
        # the other forms answer as before
        f = ctypes.c_int32(-1)
        ghx.call("ghx_exchange_mixed", plan.h, ctypes.byref(f))
        assert f.value == 0
        ghx.call("ghx_exchange_self_fusable", plan.h, ctypes.byref(f))
        assert f.value == 0
        fus, ns, nt, why = _self_info(ghx, plan)
        assert (fus, ns, nt) == (0, 0, 0) and "peer messages" in why
        ghx.call("ghx_cs_self_info", plan.h, ctypes.byref(f), None, None, None)
        assert f.value == 0 and b"not a cubed-sphere exchange" in ghx.lib().ghx_last_error()
        # no device needed to ask; executing without buffers is refused
        L = ghx.lib()
        assert L.ghx_uexchange_pack_self(plan.h, None, 0, None, 0, None) == -1
        assert L.ghx_uexchange_unpack_peers(plan.h, None, 0, None, 0, None) == -1


def _not_mixed(ghx, plan, fragment):
    mixed, n_self, n_peer, why = _mixed_info(ghx, plan)
    assert (mixed, n_self, n_peer) == (0, 0, 0) and fragment in why, why
    L = ghx.lib()
    ptrs = ghx.ptr_array([4096] * 16)
    for fn in (L.ghx_uexchange_pack_self, L.ghx_uexchange_unpack_peers):
        assert fn(plan.h, ptrs, 16, ptrs, 16, None) == -1
        assert fragment.encode() in L.ghx_last_error()


def test_all_domains_on_one_rank_is_not_mixed(ghx, golden_dir):
    _not_mixed(ghx, _plan(ghx, [_known_answer_domains(golden_dir)], 0), "no peer message")


def test_one_domain_per_rank_is_not_mixed(ghx, golden_dir):
    doms = _known_answer_domains(golden_dir)
    for rank in range(4):
        _not_mixed(ghx, _plan(ghx, [[d] for d in doms], rank), "no self message")


def test_structured_next_to_the_lists_is_not_mixed(ghx, golden_dir):
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
    doms = _known_answer_domains(golden_dir)
    plan = _plan(ghx, [doms[:2], doms[2:]], 0, extra=[it])
    plan._keep += (spc,)
    _not_mixed(ghx, plan, "structured items")


@pytest.mark.parametrize("direction", [0, 1])
def test_both_launches_are_refused_while_a_direction_has_parity_set(ghx, golden_dir, direction):
    doms = _known_answer_domains(golden_dir)
    plan = _plan(ghx, [doms[:2], doms[2:]], 0)
    n = len(plan.send if direction == 0 else plan.recv)
    word = ctypes.c_uint64(0)
    offsets = (ctypes.c_int64 * n)(*([256] * n))
    ghx.call("ghx_exchange_set_parity", plan.h, direction, ctypes.addressof(word), 0, offsets, n)
    ptrs = ghx.ptr_array([4096] * 8)
    L = ghx.lib()
    for fn in (L.ghx_uexchange_pack_self, L.ghx_uexchange_unpack_peers):
        assert fn(plan.h, ptrs, 2, ptrs, 6, None) == -1
        assert b"double-buffered" in L.ghx_last_error()
    assert _mixed_info(ghx, plan)[0] == 1             # still mixed; parity is a launch-time state
    ghx.call("ghx_exchange_set_parity", plan.h, direction, None, 0, None, 0)
