"""The planner's choice of field-offset arithmetic (short_addressing in ghx_plan.cpp ->
seg_s::amode), read back through ghx_plan_segment, at every limit of the short form: rows, row
length, outer extents and strides below 2^24, strides non-negative, span below 2^32. Host only
(plans created without a device keep their host segments). A numpy model of the kernel's short
form (field_offset_f: 24-bit products, 32-bit sums) shows that every segment the planner puts
on the short form is exact there, and that the cases just beyond a limit really are inexact.
tests/test_gpu_addressing.py runs the same cases on the device."""
import ctypes

import numpy as np
import pytest

from tests import addressing_cases as A


@pytest.fixture(scope="module")
def ghx():
    from ghex_amd import _ghx
    _ghx.lib()
    return _ghx


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("name", list(A.CASES))
def test_planner_chooses_the_addressing_form(ghx, name, direction):
    case = A.CASES[name]
    with A.Plan(A.case_entry(case), direction) as p:
        segs = p.segments()
        nb = ctypes.c_uint64()
        ghx.call("ghx_plan_info", p.h, ctypes.byref(nb), None, None)
    assert nb.value == case.nbytes
    assert [A.seg_facts(s) for s in segs] == [case.expect]
    s = segs[0]
    assert s.buf_off == 0 and s.bytes == case.nbytes and s.field_slot == 0 and s.buffer_slot == 0
    assert s.field_off == (A.H_FIELD_OFF if name == "H" else 0)
    assert s.tile_bytes > 0 and s.pipe == 0
    assert list(s.ext[s.n_outer:]) == [1] * (4 - s.n_outer)


def test_fast_addr_off_plans_the_general_form_everywhere(ghx):
    L = ghx.lib()
    try:
        assert L.ghx_tune(b"fast_addr", 0) == 0
        for case in A.CASES.values():
            for direction in (0, 1):
                with A.Plan(A.case_entry(case), direction) as p:
                    segs = p.segments()
                assert [A.seg_facts(s)[:4] for s in segs] == [case.expect[:4]], case.name
                assert [s.amode for s in segs] == [0], case.name
    finally:
        assert L.ghx_tune(b"reset", 0) == 0
    with A.Plan(A.case_entry(A.CASES["A1"]), 0) as p:
        assert [s.amode for s in p.segments()] == [1]


@pytest.mark.parametrize("name", [n for n, c in A.CASES.items() if c.expect[4] != 0])
def test_short_form_is_exact_where_the_planner_uses_it(ghx, name):
    """The model of field_offset_f over every row of the segment as the planner reports it
    equals the exact int64 offsets."""
    with A.Plan(A.case_entry(A.CASES[name]), 0) as p:
        s, = p.segments()
    assert s.amode in (1, 2) and (s.amode == 2) == (s.n_outer == 3)
    exact = A.exact_row_offsets(s)
    assert exact.min() >= 0 and exact.max() + s.row_bytes <= 1 << 32
    np.testing.assert_array_equal(A.short_row_offsets(s, s.amode), exact)
    # and the segment's rows are the reference enumeration's (row starts, in buffer order)
    case = A.CASES[name]
    ref = A.case_offsets(case)[::s.row_bytes // case.elem]
    np.testing.assert_array_equal(s.field_off + exact, ref)


@pytest.mark.parametrize("name", ["A2", "B2", "C2", "D3", "F3"])
def test_beyond_a_limit_the_short_form_is_wrong(ghx, name):
    """These cases sit on the far side of a real limit, not merely a conservative one: the
    short form would compute a wrong offset for at least one row."""
    with A.Plan(A.case_entry(A.CASES[name]), 0) as p:
        s, = p.segments()
    assert s.amode == 0 and s.n_outer in (2, 3)
    assert np.any(A.short_row_offsets(s, s.n_outer - 1) != A.exact_row_offsets(s))


@pytest.mark.parametrize("name", ["D2", "F2"])
def test_conservative_limits(ghx, name):
    """The rule refuses rows == 2^24 (the largest row INDEX, 2^24 - 1, still fits a 24-bit
    operand) and a span of exactly 2^32 (the largest offset still fits): refused, though the
    short form would be exact."""
    with A.Plan(A.case_entry(A.CASES[name]), 0) as p:
        s, = p.segments()
    assert s.amode == 0
    np.testing.assert_array_equal(A.short_row_offsets(s, 1), A.exact_row_offsets(s))


def test_plan_segment_argument_checks_and_order(ghx):
    """Segments come in plan order over all launch groups with the caller's slots; an index out
    of range is GHX_ERR_INVALID."""
    L = ghx.lib()
    s = ghx.SegmentInfo()
    names = ["A1", "C1", "G", "W2"]
    ents, keep = [], []
    for k in range(70):  # 70 distinct slots: two launch groups
        e, arr = A.case_entry(A.CASES[names[k % 4]])
        e.field_slot, e.buffer_slot = k, 69 - k
        ents.append(e)
        keep.append(arr)
    arr = (ghx.PackEntry * len(ents))(*ents)
    h = ctypes.c_void_p()
    assert L.ghx_plan_create(arr, len(ents), 1, ctypes.byref(h)) == 0, L.ghx_last_error()
    try:
        n = ctypes.c_int32()
        assert L.ghx_plan_info(h, None, ctypes.byref(n), None) == 0 and n.value == 70
        for k in range(70):
            assert L.ghx_plan_segment(h, k, ctypes.byref(s)) == 0
            assert (s.field_slot, s.buffer_slot) == (k, 69 - k)
            assert A.seg_facts(s) == A.CASES[names[k % 4]].expect
        for k in (-1, 70, 1 << 30):
            assert L.ghx_plan_segment(h, k, ctypes.byref(s)) == -1
            assert b"out of range" in L.ghx_last_error()
        assert L.ghx_plan_segment(h, 0, None) == -1
        assert L.ghx_plan_segment(None, 0, ctypes.byref(s)) == -1
    finally:
        assert L.ghx_plan_destroy(h) == 0


def test_three_launch_groups_report_every_segment_in_order(ghx):
    """130 distinct field and buffer slots are three launch groups (64, 64, 2): ghx_plan_segment
    returns all 130 segments in plan order with the caller's slots, ghx_plan_info the segments
    and the tiles summed over the groups, and index 130 is refused. The unstructured plan of 130
    slots reports its bytes, segments and tiles the same way."""
    L = ghx.lib()
    nb, n, nt = ctypes.c_uint64(), ctypes.c_int32(), ctypes.c_int32()
    ents, keep = A.many_slot_entries()
    one = ctypes.c_void_p()
    assert L.ghx_plan_create(ents, 1, 0, ctypes.byref(one)) == 0, L.ghx_last_error()
    assert L.ghx_plan_info(one, None, None, ctypes.byref(nt)) == 0
    assert L.ghx_plan_destroy(one) == 0
    tiles_each = nt.value
    assert tiles_each == 1
    for direction in (0, 1):
        h = ctypes.c_void_p()
        assert L.ghx_plan_create(ents, A.N_SLOTS, direction, ctypes.byref(h)) == 0, L.ghx_last_error()
        try:
            assert L.ghx_plan_info(h, ctypes.byref(nb), ctypes.byref(n), ctypes.byref(nt)) == 0
            assert (nb.value, n.value, nt.value) == (A.N_SLOTS * A.SLOT_BOX_BYTES, A.N_SLOTS,
                                                     A.N_SLOTS * tiles_each)
            s = ghx.SegmentInfo()
            for k in range(A.N_SLOTS):
                assert L.ghx_plan_segment(h, k, ctypes.byref(s)) == 0
                assert (s.field_slot, s.buffer_slot) == (k, A.N_SLOTS - 1 - k)
                assert (s.field_off, s.buf_off, s.bytes) == (24, 0, A.SLOT_BOX_BYTES)
                assert A.seg_facts(s) == (8, 2, 4, 3, 1)
            assert L.ghx_plan_segment(h, A.N_SLOTS, ctypes.byref(s)) == -1
            assert b"out of range" in L.ghx_last_error()
        finally:
            assert L.ghx_plan_destroy(h) == 0
    lids = A.many_slot_lids()
    uents = A.many_slot_uentries(lids)
    for direction in (0, 1):
        h = ctypes.c_void_p()
        assert L.ghx_uplan_create(uents, A.N_SLOTS, direction, ctypes.byref(h)) == 0, L.ghx_last_error()
        try:
            assert L.ghx_uplan_info(h, ctypes.byref(nb), ctypes.byref(n), ctypes.byref(nt)) == 0
            assert (nb.value, n.value, nt.value) == (A.N_SLOTS * A.U_LIDS * A.U_LEVELS * 4,
                                                     A.N_SLOTS, A.N_SLOTS)
        finally:
            assert L.ghx_uplan_destroy(h) == 0
