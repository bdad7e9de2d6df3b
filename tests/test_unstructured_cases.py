"""The index-list case table (tests/unstructured_cases.py) on the host: its enumerator against
the pinned oracle, the planner's choices read back through ghx_uplan_segment (plans created
without a device keep their host segments), the coverage the table promises, asserted so that a
later edit cannot hollow it out, and the arena's closure property that keeps a wrong kernel on
the device from faulting. tests/test_gpu_uforms.py runs the same cases on the device."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as orc
from tests import unstructured_cases as U


@pytest.fixture(scope="module")
def ghx():
    from ghex_amd import _ghx
    _ghx.lib()
    return _ghx


def _host_arena(case, seed=3):
    """(arena, per-list expected message): zeros with random bytes 1..255 on the message's
    cells."""
    lay, idx = U.layout(case), U.arena_indices(case)
    rng = np.random.default_rng(seed)
    arena = np.zeros(lay.arena_bytes, dtype=np.uint8)
    every = np.unique(np.concatenate(idx))
    assert every.min() >= 0 and every.max() < lay.arena_bytes
    arena[every] = rng.integers(1, 256, size=every.size, dtype=np.uint8)
    return arena, [arena[i] for i in idx]


def _field_view(case, arena, fi):
    """The oracle's `values` array of field fi: the arena from the field pointer on. With a
    lid_bias the pointer lies before the arena: the oracle gets the unbiased lids instead and a
    pointer moved forward by the same cells (the addresses are the same)."""
    lay, f = U.layout(case), case.fields[fi]
    return arena[lay.field_ptr[fi] + case.lid_bias * f.isb:]


# ---------------------------------------------------------------------------------------------
# enumerator == oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.HOST_SIZED)
def test_enumerator_equals_the_oracle(name):
    """element_offsets gathers exactly the bytes oracle.unstructured_get gathers and scatters
    as unstructured_set does."""
    case = U.CASES[name]
    arena, want = _host_arena(case)
    idx = U.arena_indices(case)
    rng = np.random.default_rng(4)
    scattered = arena.copy()
    by_enum = arena.copy()
    for k, (l, lid) in enumerate(zip(case.lists, U.lids(case))):
        f = case.fields[l.field]
        got = np.zeros(want[k].size, dtype=np.uint8)
        orc.unstructured_get(_field_view(case, arena, l.field), got, f.elem, lid - case.lid_bias,
                             f.levels, f.levels_first, f.index_stride, f.level_stride)
        np.testing.assert_array_equal(got, want[k])
        if case.repeats:
            continue
        fresh = rng.integers(1, 256, size=want[k].size, dtype=np.uint8)
        orc.unstructured_set(_field_view(case, scattered, l.field), fresh, f.elem,
                             lid - case.lid_bias, f.levels, f.levels_first, f.index_stride,
                             f.level_stride)
        by_enum[idx[k]] = fresh
    np.testing.assert_array_equal(scattered, by_enum)


def test_unpack_lists_are_free_of_repeats():
    for case in U.CASES.values():
        idx = np.concatenate(U.arena_indices(case))
        assert case.repeats == (np.unique(idx).size < idx.size), case.name


# ---------------------------------------------------------------------------------------------
# planner facts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("name", list(U.CASES))
def test_planner_facts(ghx, name, direction):
    case = U.CASES[name]
    with U.UPlan(case, direction) as p:
        segs = p.segments()
        nb, ns = ctypes.c_uint64(), ctypes.c_int32()
        ghx.call("ghx_uplan_info", p.h, ctypes.byref(nb), ctypes.byref(ns), None)
        s = ghx.USegmentInfo()
        L = ghx.lib()
        assert L.ghx_uplan_segment(p.h, ns.value, ctypes.byref(s)) == -1
        assert L.ghx_uplan_segment(p.h, -1, ctypes.byref(s)) == -1
        assert L.ghx_uplan_segment(p.h, 0, None) == -1
        assert L.ghx_uplan_segment(None, 0, ctypes.byref(s)) == -1
    assert nb.value == case.message_bytes and ns.value == len(case.lists)
    U.assert_planned(case, segs)
    # the launch form at aligned allocation bases: mode and lid table as planned, W no wider
    for (mode, W, lid64, runs), want in zip(U.expected_form(case), U.planned(case)):
        assert (mode, lid64) == (want[0], want[2]) and W <= 1 << want[1]


def _knob_id(k):
    return "-".join(f"{a}{b}" for a, b in k.items())


KNOB_SETS = [{"u_tile_rows": 1}, {"u_tile_rows": 3}, {"u_tile_rows": 5000},
             {"u_tile_bytes": 1024, "small_row_bytes": 1},
             {"u_tile_bytes": 65536, "small_row_bytes": 1},
             {"short_pol": 3}, {"urun": 0}]


@pytest.mark.parametrize("knobs", KNOB_SETS, ids=_knob_id)
def test_planner_facts_under_the_knobs(ghx, knobs):
    """The tile and cache-policy rules of tile_bytes_rule / assert_planned under every knob the
    device tests turn, on one case per mode and the mixed plan."""
    for name in ("m0_rows24", "m1_w8_i32", "m2_e12", "m0_long80", "mixed"):
        case = U.with_knobs(U.CASES[name], **knobs)
        for direction in (0, 1):
            with U.UPlan(case, direction) as p:
                U.assert_planned(case, p.segments())
    with U.UPlan(U.CASES["m0_rows24"], 0) as p:  # the knobs were reset
        U.assert_planned(U.CASES["m0_rows24"], p.segments())


def _model_moves_the_enumerated_bytes(case):
    """The kernel's tile walk, modelled on the planner's records (kernel_model), touches every
    vector of the message, only vectors of the message (clamped positions repeat one), and
    addresses each at the enumerated field offset."""
    with U.UPlan(case, 1) as p:
        segs = p.segments()
    for s, lid, off, l, (_, W, _, _) in zip(segs, U.lids(case), U.element_offsets(case),
                                            case.lists, U.expected_form(case)):
        f = case.fields[l.field]
        want = U.byte_indices(off, f.elem)  # field byte offset of every buffer byte
        pos, fo = U.kernel_model(s, W, lid)
        assert np.array_equal(np.unique(pos), np.arange(0, s.bytes, W))
        j = np.arange(W, dtype=np.int64)[None, :]
        assert np.array_equal(want[pos[:, None] + j], fo[:, None] + j), case.name


@pytest.mark.parametrize("name", list(U.CASES))
def test_kernel_model_moves_the_enumerated_bytes(ghx, name):
    _model_moves_the_enumerated_bytes(U.CASES[name])


@pytest.mark.parametrize("knobs", KNOB_SETS, ids=_knob_id)
def test_kernel_model_under_the_knobs(ghx, knobs):
    for name in ("m0_rows24", "m1_w8_i32", "m2_e12", "m0_long80_i64", "m1_w1_i64", "mixed"):
        _model_moves_the_enumerated_bytes(U.with_knobs(U.CASES[name], **knobs))


def test_segments_of_more_slots_than_one_launch_holds(ghx):
    """ghx_uplan_segment walks the launch groups in plan order and reports the caller's slots."""
    from tests import addressing_cases as A
    lid = A.many_slot_lids()
    ents = A.many_slot_uentries(lid)
    h = ctypes.c_void_p()
    ghx.call("ghx_uplan_create", ents, A.N_SLOTS, 0, ctypes.byref(h))
    try:
        s = ghx.USegmentInfo()
        for k in range(A.N_SLOTS):
            ghx.call("ghx_uplan_segment", h, k, ctypes.byref(s))
            assert (s.field_slot, s.buffer_slot) == (k, A.N_SLOTS - 1 - k)
            assert (s.mode, s.n, s.row_bytes, s.bytes) == (0, A.U_LIDS, 8, 8 * A.U_LIDS)
        assert ghx.lib().ghx_uplan_segment(h, A.N_SLOTS, ctypes.byref(s)) == -1
    finally:
        ghx.lib().ghx_uplan_destroy(h)


# ---------------------------------------------------------------------------------------------
# coverage conditions, on the table itself
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(ghx):
    """name -> [(segment, (mode, W, lid64, runs))] of every case's pack plan."""
    out = {}
    for name, case in U.CASES.items():
        with U.UPlan(case, 0) as p:
            out[name] = list(zip(p.segments(), U.expected_form(case)))
    return out


def test_every_mode_width_and_lid_table_has_a_case(table):
    seen = {(mode, W, lid64) for rows in table.values() for _, (mode, W, lid64, runs) in rows
            if not runs}
    want = {(m, W, t) for m in (0, 1, 2) for W in (1, 2, 4, 8, 16) for t in (0, 1)}
    assert want <= seen, sorted(want - seen)


def test_no_case_takes_the_run_path(table):
    """Every launch of the table is copy_tile_u's (k_copy<*, seg_u, RUNS = false>)."""
    assert not any(runs for rows in table.values() for _, (_, _, _, runs) in rows)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_tiling_conditions_hold_for_every_mode(table, mode):
    several = clamp = False
    for rows in table.values():
        for s, (m, W, _, _) in rows:
            if m != mode:
                continue
            t = U.tiles(s, W)
            several |= len(t) >= 2 and t[-1][0] < s.tile_bytes
            clamp |= s.tile_bytes > U.KU * U.BLOCK * W and any(
                nb > U.KU * U.BLOCK * W and partial for nb, _, partial in t)
    assert several, "no segment of >= 2 tiles with a partial last tile"
    assert clamp, "no tile of more than one loop trip whose last trip is partial"


@pytest.mark.parametrize("mode", [1, 2])
def test_a_tile_straddles_a_level_or_index_boundary(table, mode):
    """Mode 2: a tile that holds the end of one level and the start of the next; mode 1: a tile
    that starts inside an index's levels. (Mode 0 tiles hold whole rows = whole indices.)"""
    found = False
    for name, rows in table.items():
        for s, (m, _, _, _) in rows:
            if m != mode:
                continue
            rows_per_tile = s.tile_bytes // s.row_bytes
            levels = s.bytes // s.row_bytes // s.n
            unit = s.n if mode == 2 else levels  # rows between two boundaries
            n_tiles = -(-s.bytes // s.tile_bytes)
            found |= any((t * rows_per_tile) % unit != 0 for t in range(1, n_tiles))
    assert found


def test_one_plan_mixes_all_modes_and_a_run_eligible_entry(table):
    rows = table["mixed"]
    assert {m for _, (m, _, _, _) in rows} == {0, 1, 2}
    eligible = [s for s, _ in rows if s.runs]
    assert len(eligible) == 1 and eligible[0].row_bytes == 4
    assert not any(runs for _, (_, _, _, runs) in rows)  # the general kernel for all four
    assert len({s.field_slot for s, _ in rows}) == 4 and max(s.buffer_slot for s, _ in rows) < 64


def test_element_sizes_and_misalignments():
    elems = {f.elem for c in U.CASES.values() for f in c.fields}
    assert {1, 2, 3, 4, 8, 12, 16} <= elems
    # W below the largest power of two dividing the element: only where a pointer or the buffer
    # offset is misaligned, by an amount from {1, 2, 4, 8, 24}
    for case in U.CASES.values():
        for l, (mode, W, _, _) in zip(case.lists, U.expected_form(case)):
            f = case.fields[l.field]
            natural = 1 << U._wlog2(f.elem)
            mis = [x for x in (f.shift, l.buffer_offset, l.buf_shift) if x % 16]
            if W < natural:
                assert mis and set(mis) <= {1, 2, 4, 8, 24}, case.name
                assert W == min(1 << U._wlog2(x) for x in mis), case.name
            else:
                assert all(x % natural == 0 for x in mis), case.name
    used = {x for c in U.CASES.values() for l in c.lists
            for x in (c.fields[l.field].shift, l.buffer_offset, l.buf_shift) if x % 16}
    assert used == {1, 2, 4, 8, 24}


def test_cases_stay_small():
    for name in U.HOST_SIZED:
        case, lay = U.CASES[name], U.layout(U.CASES[name])
        assert lay.arena_bytes <= (1 << 20) * len(case.fields), (name, lay.arena_bytes)
        assert lay.buffers_bytes < 1 << 20 and len(case.lists) in (3, 4)
        assert all(l.n in range(2990, 3011) or name == "m0_single" for l in case.lists)
        assert 8000 <= case.ncells <= 20000


# ---------------------------------------------------------------------------------------------
# the arena's closure: a wrong kernel lands in sentinel memory
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.CASES))
def test_arena_closure(name):
    """Every correct access lies inside its field's region with GUARD bytes to spare on both
    sides, and every access of the two OTHER offset forms of the same segment lies inside the
    arena. In the far cases the same holds for offsets truncated to 32 bits, and those differ
    from the exact ones."""
    case, lay = U.CASES[name], U.layout(U.CASES[name])
    right, wrong = U.element_offsets(case), U.other_form_offsets(case)
    for k, l in enumerate(case.lists):
        f, p = case.fields[l.field], lay.field_ptr[l.field]
        a, b = lay.region[l.field]
        assert 0 <= a and b <= lay.arena_bytes
        if not case.far:
            assert a + U.GUARD <= p + right[k].min() and p + right[k].max() + f.elem <= b - U.GUARD
        for o in [right[k]] + list(wrong[k].values()):
            assert 0 <= p + o.min() and p + o.max() + f.elem <= lay.arena_bytes
        m0, m1 = lay.msg[k]
        assert m1 - m0 == lay.bytes_[k] and m0 - l.buffer_offset == lay.buf_ptr[k]
        assert lay.buf_ptr[k] >= U.GUARD and m1 + U.GUARD <= lay.buffers_bytes
        if k:
            assert lay.msg[k - 1][1] + U.GUARD <= lay.buf_ptr[k]
        if case.far:
            w = U.wrapped_offsets(case)[k]
            assert 0 <= p + w.min() and p + w.max() + f.elem <= lay.arena_bytes
            assert (w != right[k]).mean() >= 0.4
    if case.far:
        assert max(int(o.max()) for o in right) >= 1 << 32


def _gather(arena, case, offsets_per_list):
    lay = U.layout(case)
    return [arena[U.byte_indices(o, case.fields[l.field].elem, lay.field_ptr[l.field])]
            for l, o in zip(case.lists, offsets_per_list)]


@pytest.mark.parametrize("name", [n for n in U.HOST_SIZED if n.startswith(("m1_", "m2_"))
                                  or n in ("m0_rows24", "m0_long80", "mixed")])
def test_a_wrong_form_fails_the_comparison_inside_the_arena(name):
    """The broken kernel, on the host: a gather that decodes each list with another mode's
    formula (for instance the mode-1 and mode-2 branches swapped) reads inside the arena — no
    fault — and returns a message that differs from the expected one; a scatter by it leaves
    cells that differ from the expected arena. Forms that coincide for a segment (mode 0 and
    mode 1 when the level stride is 1) are skipped."""
    case = U.CASES[name]
    arena, want = _host_arena(case)
    right, wrong = U.element_offsets(case), U.other_form_offsets(case)
    checked = 0
    for k in range(len(case.lists)):
        for form, off in wrong[k].items():
            if np.array_equal(off, right[k]):
                continue
            swapped = list(right)
            swapped[k] = off
            got = _gather(arena, case, swapped)
            assert not np.array_equal(got[k], want[k]), (name, k, form)
            checked += 1
    mode1or2 = [k for k, l in enumerate(case.lists) if case.fields[l.field].mode != 0]
    assert checked >= 2 * len(mode1or2) and checked >= len(case.lists)


@pytest.mark.parametrize("name", U.FAR)
def test_a_truncated_offset_fails_the_comparison_inside_the_arena(name):
    """The far cases with lid * index_stride_b / l * level_stride_b truncated to 32 bits: every
    wrapped address is inside the 4.5-GiB arena (asserted by test_arena_closure) and the wrapped
    cells are not the message's cells, so the device comparison fails without a fault. Checked
    on the cell sets (the arena itself is not built on the host)."""
    case = U.CASES[name]
    for o, w in zip(U.element_offsets(case), U.wrapped_offsets(case)):
        moved = w != o
        assert moved.any()
        # a wrapped store lands on a cell outside the list's own cells, or on another element's
        assert not np.array_equal(np.sort(w), np.sort(o))
