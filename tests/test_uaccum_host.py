"""Adjoint accumulate plans (ghx_uaccum_create, ghx_uexchange_adjoint_create) without a device:
the planner's tables read back through ghx_uaccum_dest / ghx_uaccum_contrib, every refusal with
its reason, exchanges built from the known-answer pattern, and the transpose identity
<E x, y> = <x, E^T y> on the host — E the oracle's get / set, E^T the NumPy definition driven by
the plan's own tables — exact with integer-valued f64."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import uaccum_cases as UA
from tests import uput_cases as UC
from tests import uself_cases as US
from tests.uput_cases import Side, udesc
from tests.test_uself_host import _known_answer_domains, _plan


@pytest.fixture(scope="module")
def ghx():
    from ghex_amd import _ghx
    _ghx.lib()
    return _ghx


@pytest.fixture(autouse=True)
def _reset_knobs(ghx):
    yield
    ghx.call("ghx_tune", b"reset", 0)


F64 = UA.DT_F64


# ---------------------------------------------------------------------------------------------
# planner facts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("repeats", [False, True])
def test_tables_of_the_three_list_case(ghx, repeats):
    od, hd = udesc(8, 3), udesc(8, 3, index_stride=4)
    contrib, zero, places = UA.three_lists_case(od, hd, seed=3, repeats=repeats)
    h = UA.create(contrib, [F64] * 3, places, zero)
    try:
        i, ds, recs = UA.info(h), UA.dests(h), UA.records(h)
        L = ghx.lib()   # an index past the end is refused
        assert L.ghx_uaccum_dest(h, len(ds), ctypes.byref(ghx.UAccumDestInfo())) == -1
        assert L.ghx_uaccum_contrib(h, len(recs), None, None) == -1
    finally:
        UA.destroy(h)
    cells = {}
    for e, s in enumerate(contrib):
        for pos, lid in enumerate(s.lids):
            cells.setdefault((s.slot, int(lid)), []).append((e, pos))
    sums = [d for d in ds if not d.zero]
    assert i["n_dest"] == len(sums) == len(cells) and i["n_contrib"] == len(recs) == 9006
    assert i["bytes"] == 9006 * 3 * 8
    # destinations: distinct, sorted by (slot, lid); records of each ascending by (entry, position)
    keys = [(d.field_slot, d.lid) for d in sums]
    assert keys == sorted(cells)
    at = 0
    for d in sums:
        assert d.first == at and d.count >= 1
        assert recs[d.first:d.first + d.count] == sorted(cells[(d.field_slot, d.lid)])
        at += d.count
    assert at == 9006 == sum(s.lids.size for s in contrib)
    assert i["max_per_dest"] == max(len(v) for v in cells.values()) == (287 if repeats else 1)
    if repeats:
        shared = cells[(1, int(contrib[1].lids[-1]))]
        assert [e for e, _ in shared] == [1, 2]
    # zero destinations after them, distinct and sorted, without records
    zs = [d for d in ds if d.zero]
    assert ds[:len(sums)] == sums and i["n_zero_dest"] == len(zs) == 9006
    zk = [(d.field_slot, d.lid) for d in zs]
    assert zk == sorted({(z.slot, int(l)) for z in zero for l in z.lids})
    assert all(d.first == 0 and d.count == 0 for d in zs)


def test_tiles_follow_u_tile_rows_and_field_slots(ghx):
    od = udesc(8, 3)
    contrib, zero, places = UA.three_lists_case(od, od, seed=4)

    def tiles(rows):
        ghx.call("ghx_tune", b"u_tile_rows", rows)
        h = UA.create(contrib, [F64] * 3, places, zero)
        t = UA.info(h)["n_tiles"]
        UA.destroy(h)
        return t

    def up(n, r):
        return -(-n // r)
    # owner slot 0 holds 3001 destinations, slot 1 6005; halo slots 3001 and 6005
    assert tiles(512) == 2 * (up(3001, 512) + up(6005, 512))
    assert tiles(5000) == 2 * (1 + 2)
    assert tiles(1) == 2 * 9006


def test_empty_plans_and_entries_without_lids(ghx):
    h = UA.create([], [], [], [])
    assert UA.info(h) == dict(bytes=0, n_dest=0, n_zero_dest=0, n_contrib=0, max_per_dest=0, n_tiles=0)
    assert ghx.lib().ghx_uaccum_execute(h, None, 0, None, 0, 1, None) == 0   # nothing to launch
    UA.destroy(h)
    none = np.zeros(0, dtype=np.int64)
    h = UA.create([Side(udesc(4), 0, none)], [UA.DT_I32], [(0, 0)], [Side(udesc(4), 1, none)])
    assert UA.info(h)["n_tiles"] == 0
    UA.destroy(h)


def test_plans_are_inspected_without_a_device_and_their_execute_is_refused(ghx):
    import torch
    contrib, zero, places = UA.three_lists_case(udesc(4), udesc(4), seed=5)
    h = UA.create(contrib, [UA.DT_F32] * 3, places, zero)
    L = ghx.lib()
    try:
        assert UA.info(h)["n_tiles"] > 0
        # pointer arrays that do not cover the slots are refused with or without a device
        assert L.ghx_uaccum_execute(h, None, 0, None, 0, 1, None) == -1
        assert b"do not cover" in L.ghx_last_error()
        one = ghx.ptr_array([4096] * 4)
        assert L.ghx_uaccum_execute(h, one, 4, one, 1, 1, None) == -1
        if not torch.cuda.is_available():
            assert L.ghx_uaccum_execute(h, one, 4, one, 2, 1, None) == -2
            assert b"no device tables" in L.ghx_last_error()
        else:  # with a device the launch is refused before it starts: misaligned pointers
            odd = ghx.ptr_array([4098] * 4)
            assert L.ghx_uaccum_execute(h, odd, 4, one, 2, 1, None) == -1
            assert b"not aligned" in L.ghx_last_error()
            assert L.ghx_uaccum_execute(h, one, 4, odd, 2, 1, None) == -1
            assert b"not aligned" in L.ghx_last_error()
    finally:
        UA.destroy(h)


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def _refused(contrib, dtypes, places, zero, fragment):
    rc, why, h = UA.try_create(contrib, dtypes, places, zero)
    assert rc == -1 and not h.value, (rc, why)
    assert fragment in why, why


def test_dtypes_are_checked(ghx):
    lids = np.arange(10)
    for code in (0, 5, -1, 99):
        _refused([Side(udesc(8), 0, lids)], [code], [(0, 0)], [], "unknown dtype code")
    _refused([Side(udesc(8), 0, lids)], [UA.DT_F32], [(0, 0)], [], "elem_size is 8")
    _refused([Side(udesc(4), 0, lids)], [UA.DT_I64], [(0, 0)], [], "elem_size is 4")
    _refused([Side(udesc(2), 0, lids)], [UA.DT_I32], [(0, 0)], [], "elem_size is 2")
    _refused([Side(udesc(8), 0, lids)], [F64], [(0, 0)], [Side(udesc(2), 1, lids)], "zero entry's elem_size is 2")
    # one field slot, two dtypes of one size
    _refused([Side(udesc(8), 0, lids), Side(udesc(8), 0, lids)], [F64, UA.DT_I64], [(0, 0), (1, 0)], [],
             "differ in their dtype")


def test_slots_lists_and_offsets_are_checked(ghx):
    lids = np.arange(10)
    one = "at most 64 field and 64 buffer slots"
    _refused([Side(udesc(8), 64, lids)], [F64], [(0, 0)], [], one)
    _refused([Side(udesc(8), 0, lids)], [F64], [(64, 0)], [], one)
    _refused([Side(udesc(8), 0, lids)], [F64], [(0, 0)], [Side(udesc(8), 64, lids)], one)
    _refused([Side(udesc(8), -1, lids)], [F64], [(0, 0)], [], "negative slot")
    _refused([Side(udesc(8), 0, lids)], [F64], [(-1, 0)], [], "negative slot")
    _refused([Side(udesc(8), 0, [3, -1])], [F64], [(0, 0)], [], "negative local index")
    _refused([Side(udesc(8), 0, lids)], [F64], [(0, 0)], [Side(udesc(8), 1, [3, -1])], "negative local index")
    _refused([Side(udesc(8, 0), 0, lids)], [F64], [(0, 0)], [], "levels < 1")
    _refused([Side(udesc(8), 0, lids)], [F64], [(0, 4)], [], "not a multiple of the element size")
    h = UA.create([Side(udesc(4), 0, lids)], [UA.DT_F32], [(0, 4)])  # element-aligned only: fine
    UA.destroy(h)
    # slot 63 of both kinds is the last one a launch holds
    h = UA.create([Side(udesc(8), 63, lids)], [F64], [(63, 0)], [Side(udesc(8), 62, lids)])
    UA.destroy(h)


def test_entries_of_one_field_slot_must_share_their_descriptor(ghx):
    lids, more = np.arange(10), np.arange(10, 20)
    why = "differ in their data descriptor"
    a = udesc(8, 3)
    for b in (udesc(8, 2), udesc(8, 3, index_stride=4), udesc(8, 3, first=False),
              udesc(8, 3, index_stride=1, level_stride=UC.N_CELLS)):
        _refused([Side(a, 0, lids), Side(b, 0, more)], [F64, F64], [(0, 0), (1, 0)], [], why)
        _refused([Side(a, 0, lids)], [F64], [(0, 0)], [Side(b, 0, more)], why)   # zero entry against it
        _refused([Side(a, 0, lids)], [F64], [(0, 0)], [Side(a, 1, lids), Side(b, 1, more)], why)
    h = UA.create([Side(a, 0, lids), Side(a, 0, more)], [F64, F64], [(0, 0), (1, 0)], [Side(a, 0, more + 50)])
    UA.destroy(h)


def test_a_cell_that_is_summed_and_zeroed_is_refused(ghx):
    d = udesc(4, 2)
    _refused([Side(d, 0, [5, 6, 7])], [UA.DT_I32], [(0, 0)], [Side(d, 0, [9, 7])],
             "(field slot 0, lid 7) is both a sum destination and a zero destination")
    h = UA.create([Side(d, 0, [5, 6, 7])], [UA.DT_I32], [(0, 0)], [Side(d, 1, [9, 7])])  # another slot
    UA.destroy(h)


def test_more_records_than_32_bits_index_are_refused_before_a_list_is_read(ghx):
    lids = np.arange(4, dtype=np.int64)
    L = ghx.lib()
    for split in (1, 2):
        sides = [Side(udesc(4), 0, lids)] * split
        ent = US.entries(sides, [(k, 0) for k in range(split)])
        for e in ent:
            e.n_lids = (1 << 32) // split     # the lists are never read
        h = ctypes.c_void_p()
        rc = L.ghx_uaccum_create(ent, ghx.i32_array([UA.DT_I32] * split), split, None, 0, ctypes.byref(h))
        assert rc == -1 and not h.value and b"more than 2^32 - 1 contribution records" in L.ghx_last_error()
    zent = US.entries([Side(udesc(4), 1, lids)], [(0, 0)])
    zent[0].n_lids = 1 << 32
    ent = US.entries([Side(udesc(4), 0, lids)], [(0, 0)])
    rc = L.ghx_uaccum_create(ent, ghx.i32_array([UA.DT_I32]), 1, zent, 1, ctypes.byref(h))
    assert rc == -1 and b"more than 2^32 - 1 zero cells" in L.ghx_last_error()


def test_overlapping_buffer_ranges_are_accepted(ghx):
    lids = np.arange(100)
    h = UA.create([Side(udesc(8), 0, lids), Side(udesc(8), 1, lids)], [F64, F64], [(0, 0), (0, 8)])
    assert UA.info(h)["n_contrib"] == 200
    UA.destroy(h)


def test_null_arguments_are_refused(ghx):
    L = ghx.lib()
    h = ctypes.c_void_p()
    assert L.ghx_uaccum_create(None, None, 1, None, 0, ctypes.byref(h)) == -1
    assert L.ghx_uaccum_create(None, None, 0, None, 1, ctypes.byref(h)) == -1
    assert L.ghx_uaccum_create(None, None, 0, None, 0, None) == -1
    assert L.ghx_uaccum_info(None, None, None, None, None, None, None) == -1
    assert L.ghx_uaccum_destroy(None) == 0


# ---------------------------------------------------------------------------------------------
# exchanges built from the known-answer pattern
# ---------------------------------------------------------------------------------------------
def _adjoint_info(ghx, plan):
    r, nd, nc = ctypes.c_int32(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    ghx.call("ghx_uexchange_adjoint_info", plan.h, ctypes.byref(r), ctypes.byref(nd), ctypes.byref(nc))
    return r.value, nd.value, nc.value


def _golden(golden_dir):
    with open(os.path.join(golden_dir, "unstructured_case.json")) as fh:
        return json.load(fh)


def test_adjoint_plans_of_the_known_answer_exchange(ghx, golden_dir):
    case = _golden(golden_dir)
    plan = _plan(ghx, [_known_answer_domains(golden_dir)], 0)
    L = ghx.lib()
    assert _adjoint_info(ghx, plan) == (0, 0, 0)
    four = ghx.ptr_array([4096] * 16)
    assert L.ghx_uexchange_adjoint_pack(plan.h, four, 4, four, 16, None) == -1
    assert b"ghx_uexchange_adjoint_create" in L.ghx_last_error()
    assert L.ghx_uexchange_adjoint_accumulate(plan.h, four, 4, four, 16, 1, None) == -1
    # one dtype code per item, each a known one whose size is the item's
    assert L.ghx_uexchange_adjoint_create(plan.h, ghx.i32_array([F64] * 3), 3) == -1
    assert b"one dtype code per exchange item" in L.ghx_last_error()
    assert L.ghx_uexchange_adjoint_create(plan.h, ghx.i32_array([F64, 7, F64, F64]), 4) == -1
    assert b"unknown dtype code" in L.ghx_last_error()
    assert L.ghx_uexchange_adjoint_create(plan.h, ghx.i32_array([F64, UA.DT_F32, F64, F64]), 4) == -1
    assert b"elem_size is 8" in L.ghx_last_error()
    assert _adjoint_info(ghx, plan) == (0, 0, 0)
    ghx.call("ghx_uexchange_adjoint_create", plan.h, ghx.i32_array([F64, UA.DT_I64, F64, F64]), 4)
    sent = case["send_maps"]
    n_dest = sum(len({l for lids in sent[str(r)].values() for l in lids}) for r in range(4))
    n_contrib = sum(len(lids) for r in range(4) for lids in sent[str(r)].values())
    assert _adjoint_info(ghx, plan) == (1, n_dest, n_contrib) == (1, 12, 15)
    # too few buffers are refused, with or without a device
    assert L.ghx_uexchange_adjoint_pack(plan.h, four, 4, four, len(plan.recv) - 1, None) == -1
    assert b"too few recv buffers" in L.ghx_last_error()
    assert L.ghx_uexchange_adjoint_accumulate(plan.h, four, 4, four, len(plan.send) - 1, 1, None) == -1
    assert b"too few send buffers" in L.ghx_last_error()
    # the forward forms report what they reported before
    f = ctypes.c_int32(-1)
    ghx.call("ghx_uexchange_self_info", plan.h, ctypes.byref(f), None, None)
    assert f.value == 1


def test_adjoint_of_two_domains_of_the_case_counts_this_ranks_cells(ghx, golden_dir):
    case = _golden(golden_dir)
    doms = _known_answer_domains(golden_dir)
    plan = _plan(ghx, [doms[:2], doms[2:]], 1)      # rank 1: domains 2 and 3
    ghx.call("ghx_uexchange_adjoint_create", plan.h, ghx.i32_array([F64, F64]), 2)
    sent = case["send_maps"]
    n_dest = sum(len({l for lids in sent[str(r)].values() for l in lids}) for r in (2, 3))
    n_contrib = sum(len(lids) for r in (2, 3) for lids in sent[str(r)].values())
    assert _adjoint_info(ghx, plan) == (1, n_dest, n_contrib)


def test_adjoint_is_refused_while_a_direction_has_parity(ghx, golden_dir):
    plan = _plan(ghx, [_known_answer_domains(golden_dir)], 0)
    n = len(plan.recv)
    word = ctypes.c_uint64(0)
    offsets = (ctypes.c_int64 * n)(*([256] * n))
    L = ghx.lib()
    ghx.call("ghx_exchange_set_parity", plan.h, 1, ctypes.addressof(word), 0, offsets, n)
    assert L.ghx_uexchange_adjoint_create(plan.h, ghx.i32_array([F64] * 4), 4) == -1
    assert b"double-buffered" in L.ghx_last_error()
    ghx.call("ghx_exchange_set_parity", plan.h, 1, None, 0, None, 0)
    ghx.call("ghx_uexchange_adjoint_create", plan.h, ghx.i32_array([F64] * 4), 4)
    ghx.call("ghx_exchange_set_parity", plan.h, 0, ctypes.addressof(word), 0, offsets, n)
    ptrs = ghx.ptr_array([4096] * 16)
    assert L.ghx_uexchange_adjoint_pack(plan.h, ptrs, 4, ptrs, 16, None) == -1
    assert b"double-buffered" in L.ghx_last_error()
    assert L.ghx_uexchange_adjoint_accumulate(plan.h, ptrs, 4, ptrs, 16, 1, None) == -1
    assert b"double-buffered" in L.ghx_last_error()
    ghx.call("ghx_exchange_set_parity", plan.h, 0, None, 0, None, 0)


def test_exchange_with_a_structured_item_has_no_adjoint(ghx, golden_dir):
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
    L = ghx.lib()
    assert L.ghx_uexchange_adjoint_create(plan.h, ghx.i32_array([F64] * 5), 5) == -1
    assert b"structured or cubed-sphere item" in L.ghx_last_error()
    assert _adjoint_info(ghx, plan) == (0, 0, 0)


# ---------------------------------------------------------------------------------------------
# the transpose identity on the host
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels, first", [(1, True), (3, True), (3, False)])
def test_transpose_identity_with_the_oracle_as_forward_exchange(ghx, golden_dir, levels, first):
    from oracle import oracle as orc
    case = _golden(golden_dir)
    rng = np.random.default_rng(17)
    n = {r: len(case["domains"][str(r)]["gids"]) for r in range(4)}
    desc = {r: udesc(8, levels, first=first, n_cells=n[r]) for r in range(4)}
    msgs = [(s, int(r), np.asarray(sl, dtype=np.int64), np.asarray(case["recv_maps"][r][str(s)], dtype=np.int64))
            for s in range(4) for r, sl in sorted(case["send_maps"][str(s)].items())]

    def state():
        return {r: rng.integers(-50, 51, size=n[r] * levels).astype(np.float64) for r in range(4)}

    def args(r):
        d = desc[r]
        return 8, d.levels, bool(d.levels_first), d.index_stride, d.level_stride

    def forward(x):
        """E: every message through the oracle's get (owner -> buffer) and set (buffer -> halo)."""
        out = {r: v.copy() for r, v in x.items()}
        for s, r, sl, rl in msgs:
            buf = np.zeros(sl.size * levels * 8, dtype=np.uint8)
            e, L_, f, i_s, l_s = args(s)
            orc.unstructured_get(x[s], buf, e, sl, L_, f, i_s, l_s)
            e, L_, f, i_s, l_s = args(r)
            orc.unstructured_set(out[r], buf, e, rl, L_, f, i_s, l_s)
        return out

    def adjoint(y):
        """E^T: the reverse pack (the oracle's get over the receive lists), then the plan's own
        tables: per destination its records in order, then zeros."""
        contrib = [Side(desc[s], s, sl) for s, r, sl, rl in msgs]
        zero = [Side(desc[r], r, rl) for s, r, sl, rl in msgs]
        places = [(k, 0) for k in range(len(msgs))]
        bufs = []
        for s, r, sl, rl in msgs:
            buf = np.zeros(rl.size * levels * 8, dtype=np.uint8)
            e, L_, f, i_s, l_s = args(r)
            orc.unstructured_get(y[r], buf, e, rl, L_, f, i_s, l_s)
            bufs.append(buf)
        h = UA.create(contrib, [F64] * len(msgs), places, zero)
        try:
            ds, recs = UA.dests(h), UA.records(h)
        finally:
            UA.destroy(h)
        out = {r: v.copy() for r, v in y.items()}
        UA.from_tables(out, bufs, contrib, [F64] * len(msgs), places, ds, recs)
        for d in ds:
            if d.zero:
                dd = desc[d.field_slot]
                out[d.field_slot][d.lid * dd.index_stride + np.arange(levels) * dd.level_stride] = 0
        # the definition's loop gives the same
        want = UA.definition({r: v.copy() for r, v in y.items()}, bufs, contrib, [F64] * len(msgs), places, zero)
        for r in range(4):
            np.testing.assert_array_equal(out[r], want[r])
        return out

    def dot(a, b):
        return sum(float(np.dot(a[r], b[r])) for r in range(4))

    for _ in range(3):
        x, y = state(), state()
        ex, ety = forward(x), adjoint(y)
        assert dot(ex, y) == dot(x, ety)
        assert any((ety[r] != y[r]).any() for r in range(4))
    # and twice applied to a vector of ones in the owned cells it counts the copies of each cell
    ones = {r: np.ones(n[r] * levels) for r in range(4)}
    counts = adjoint(forward(ones))
    for r in range(4):
        halo = set(case["domains"][str(r)]["halo_lids"])
        for lid in range(n[r]):
            d = desc[r]
            v = counts[r][lid * d.index_stride + np.arange(levels) * d.level_stride]
            if lid in halo:
                assert (v == 0).all()
            else:
                copies = sum(list(sl).count(lid) for s, _, sl, _ in msgs if s == r)
                assert (v == 1 + copies).all()
