"""The structured case table (tests/structured_cases.py) on the host: its enumerator against the
pinned oracle, the planner's choices read back through ghx_plan_segment (plans created without a
device keep their host segments), the launch forms and tile walks the table promises, asserted so
that a later edit cannot hollow it out, and the arena's closure property that keeps a wrong
kernel on the device from faulting. tests/test_gpu_sforms.py runs the same cases on the device,
each under tile records and under the tile table."""
import ctypes

import numpy as np
import pytest

from tests import addressing_cases as A
from tests import structured_cases as S


@pytest.fixture(scope="module")
def ghx():
    from ghex_amd import _ghx
    _ghx.lib()
    return _ghx


# ---------------------------------------------------------------------------------------------
# enumerator == oracle, on every descriptor of the table
# ---------------------------------------------------------------------------------------------
def _descriptors():
    """Every field descriptor + box the tables use, once each (they differ in name or expected
    facts only where the geometry is shared)."""
    seen = {}
    every = [e.case for c in S.CASES.values() for e in c.ents]
    every += [x for p in S.PUTS.values() for x in (p.src, p.dst)]
    for c in every:
        seen.setdefault((c.elem, c.layout, c.strides, c.ext, c.offs), c)
    return list(seen.values())


@pytest.mark.parametrize("case", _descriptors(), ids=lambda c: c.name)
def test_enumerator_equals_the_oracle(case):
    A.oracle_gathers_the_enumerated_bytes(case)


def test_every_case_has_its_oracle_tie():
    keys = {(c.elem, c.layout, c.strides, c.ext, c.offs) for c in _descriptors()}
    for sc in S.CASES.values():
        for e in sc.ents:
            c = e.case
            assert (c.elem, c.layout, c.strides, c.ext, c.offs) in keys
            assert c.nbytes <= 1 << 20  # small enough for the oracle on a host array


# ---------------------------------------------------------------------------------------------
# planner facts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("name", list(S.CASES))
def test_planner_facts(ghx, name, direction):
    """Row bytes, n_outer, rows, wlog2, amode, tile_bytes and pipe of every segment equal the
    table's; the plan's tile count is the tile walk's."""
    case = S.CASES[name]
    with S.SPlan(case, direction) as p:
        segs = p.segments()
        nb, ns, nt = ctypes.c_uint64(), ctypes.c_int32(), ctypes.c_int32()
        ghx.call("ghx_plan_info", p.h, ctypes.byref(nb), ctypes.byref(ns), ctypes.byref(nt))
    S.assert_planned(case, segs, direction)
    assert nb.value == case.message_bytes and ns.value == len(S.segment_entries(case))
    assert nt.value == sum(len(S.tile_walk(s, 1)) for s in segs)
    with S.SPlan(S.CASES["long16"], 1) as p:  # the knobs were reset
        S.assert_planned(S.CASES["long16"], p.segments(), 1)


@pytest.mark.parametrize("tile_records", [1, 0])
def test_tile_records_do_not_change_the_plan(ghx, tile_records):
    for name in ("long16_u32k", "several", "short1_r64"):
        case = S.with_knobs(S.CASES[name], tile_records=tile_records)
        for direction in (0, 1):
            S.assert_planned(case, S.segments(case, direction), direction)


@pytest.mark.parametrize("name", list(S.CASES))
def test_walk_model_moves_every_vector_once(name):
    """The kernels' lane walk over the planner's tiles (walk_model) at the width and routine the
    launch takes touches every vector of the message exactly once: tiles are whole vectors."""
    case = S.CASES[name]
    for direction in (0, 1):
        for s, (routine, W, _) in zip(S.segments(case, direction),
                                      S.expected_forms(case, direction)):
            pos = S.walk_model(s, W, routine)
            assert np.array_equal(np.sort(pos), np.arange(0, s.bytes, W)), (name, direction)
            walk = S.tile_walk(s, W, routine)
            assert sum(nb for nb, _, _, _ in walk) == s.bytes


# ---------------------------------------------------------------------------------------------
# form closure: the union of the table's launch forms is exactly this set
# ---------------------------------------------------------------------------------------------
def _form_key(case, k, direction):
    """(direction, routine, W, AM, note) of segment k at aligned allocation bases. note: what the
    planner had chosen where the launch departs from it: "amode1" (short form planned, W in
    {1, 2}: general), "amode2-field" / "amode2-buffer" (two-division form planned, narrowed by
    that pointer: general), "pipe" (pipelined planned, narrowed: copy_tile), the
    unpack_tile_bytes of a pipelined launch."""
    s = S.segments(case, direction)[k]
    e, lay = case.ents[s.field_slot], S.layout(case)
    routine, W, AM = S.expected_forms(case, direction)[k]
    note = ""
    if routine == "pipelined":
        note = S.knob(case, "unpack_tile_bytes")
    elif s.pipe:
        note = "pipe"
    elif s.amode == 2 and AM == 0:
        by_field = S._wlog2(lay.fields[s.field_slot].ptr) < 4
        by_buffer = S._wlog2(lay.buf_ptr[e.buffer_slot] + s.buf_off) < 4
        assert by_field != by_buffer
        note = "amode2-field" if by_field else "amode2-buffer"
    elif s.amode == 1 and AM == 0:
        note = "amode1"
    return (direction, routine, W, AM, note)


def _required_forms():
    want = set()
    for d in (0, 1):
        want |= {(d, "tile", W, 0, "") for W in (1, 2, 4, 8, 16)}       # general
        want |= {(d, "tile", W, 1, "") for W in (4, 8, 16)}             # one division
        want.add((d, "tile", 16, 2, ""))                                # two divisions
        want |= {(d, "tile", W, 0, "amode1") for W in (1, 2)}           # amode 1 planned
        want |= {(d, "tile", 8, 0, "amode2-" + by) for by in ("field", "buffer")}
    want |= {(1, "pipelined", 16, 0, utb) for utb in (16384, 32768)}
    # pipe set, narrowed: by a buffer-pointer shift of 8 (long16_u32k_b8), by the planned width
    # (long8_u32k; the 4-B and 2-B long-row entries of several_u32k)
    want |= {(1, "tile", 8, 1, "pipe"), (1, "tile", 4, 1, "pipe"), (1, "tile", 2, 0, "pipe")}
    return want


def test_form_closure():
    """Every form of k_copy<*, seg_s> is reached by a case, pack and unpack, and no case takes a
    form outside the list: removing a case that alone reaches a form fails here."""
    seen = {}
    for name, case in S.CASES.items():
        for direction in (0, 1):
            for k in range(len(S.segments(case, direction))):
                seen.setdefault(_form_key(case, k, direction), []).append(name)
    want = _required_forms()
    assert set(seen) == want, (sorted(map(str, want - set(seen))),
                               sorted(map(str, set(seen) - want)))
    # the named cases reach the forms they were written for
    assert "long16_u32k_b8" in seen[(1, "tile", 8, 1, "pipe")]
    assert seen[(0, "tile", 8, 0, "amode2-field")] == ["outer3_f8"]
    assert seen[(0, "tile", 8, 0, "amode2-buffer")] == ["outer3_b8"]


def test_a_buffer_offset_or_pointer_narrows_the_width():
    """buffer_offset 4 lowers the planned width itself; a shifted pointer lowers the launch's
    only. Shifts of 1, 2, 4 and 8 B, on the field side and on the buffer side separately."""
    c = S.CASES["long16_off4"]
    assert S.segments(c, 0)[0].wlog2 == 2 and S.expected_forms(c, 0) == [("tile", 4, 1)]
    for shp in ("long16", "short16"):
        for sh in (1, 2, 4, 8):
            for side in "fb":
                c = S.CASES[f"{shp}_{side}{sh}"]
                assert (c.ents[0].fshift, c.bshift[0]) == ((sh, 0) if side == "f" else (0, sh))
                for d in (0, 1):
                    assert S.segments(c, d)[0].wlog2 == 4
                    assert S.expected_forms(c, d)[0][1] == sh
    rows = {S.SHAPES[n][4][0] for n in S.SHAPES if n.startswith("short")}
    assert rows == {3, 2, 4, 8, 12, 16, 24}


def test_every_width_has_a_general_twin():
    for shp in S.SHAPES:
        a, g = S.CASES[shp], S.CASES[shp + "_g"]
        for d in (0, 1):
            fa, fg = S.expected_forms(a, d)[0], S.expected_forms(g, d)[0]
            assert S.segments(g, d)[0].amode == 0 and fg == (fa[0], fa[1], 0)


# ---------------------------------------------------------------------------------------------
# tile walks
# ---------------------------------------------------------------------------------------------
def _walks(direction, routine, widths):
    """[(case name, tile_walk)] of every segment that launches as `routine` at a width in
    `widths`."""
    out = []
    for name, case in S.CASES.items():
        for s, (r, W, _) in zip(S.segments(case, direction), S.expected_forms(case, direction)):
            if r == routine and W in widths:
                out.append((name, S.tile_walk(s, W, r)))
    return out


@pytest.mark.parametrize("widths", [(1,), (2,), (4,), (8,), (16,)], ids=lambda w: f"W{w[0]}")
@pytest.mark.parametrize("direction", [0, 1])
def test_copy_tile_walks(direction, widths):
    """At every width, pack and unpack: a tile of one partial trip, a tile of several trips whose
    last is partial, a segment whose last tile is shorter than the others, a tile that starts
    inside a row; a tile of exactly one full trip (tile_bytes = 1024 * W; the default tile at
    8 B); a tile of several full trips at the narrow widths (the default tile)."""
    walks = [w for _, w in _walks(direction, "tile", widths)]
    tiles = [t for w in walks for t in w]
    assert any(trips == 1 and partial for _, trips, partial, _ in tiles)
    assert any(trips > 1 and partial for _, trips, partial, _ in tiles)
    assert any(len(w) > 1 and w[-1][0] < w[0][0] for w in walks)
    assert any(mid for _, _, _, mid in tiles)
    assert any(trips == 1 and not partial for _, trips, partial, _ in tiles)
    if widths[0] < 8:
        assert any(trips > 1 and not partial for _, trips, partial, _ in tiles)


def test_named_copy_tile_walks():
    (s,) = S.segments(S.CASES["long16_t64k"], 0)
    assert S.tile_walk(s, 16) == [(65536, 4, False, False), (18464, 2, True, True)]
    (s,) = S.segments(S.CASES["long16_u32k_b8"], 1)
    assert [t[:3] for t in S.tile_walk(s, 8)] == [(32768, 4, False), (32768, 4, False),
                                                   (18464, 3, True)]
    (s,) = S.segments(S.CASES["short1_r64"], 0)
    assert [t[:3] for t in S.tile_walk(s, 1)] == [(192, 1, True)] * 46 + [(168, 1, True)]
    for name in ("long4", "long2", "long1"):
        assert len(S.tile_walk(S.segments(S.CASES[name], 0)[0], 1)) == 3


def test_pipelined_walks():
    """32-KiB tiles: 4 steps, 4 steps, then 18,464 B = two full steps and a third in which only
    lanes 0..129 hold a vector, in slot 0 (the lanes leave the loop at different steps). 16-KiB
    tiles: exactly two full steps each, and a last tile of one partial step. A whole segment of
    exactly two full steps."""
    (s,) = S.segments(S.CASES["long16_u32k"], 1)
    assert [t[:3] for t in S.tile_walk(s, 16, "pipelined")] == [
        (32768, 4, False), (32768, 4, False), (18464, 3, True)]
    assert (18464 - 2 * S.PIPE_STEP) // 16 == 130 < S.BLOCK
    (s,) = S.segments(S.CASES["long16_u16k"], 1)
    assert [t[:3] for t in S.tile_walk(s, 16, "pipelined")] == [(16384, 2, False)] * 5 + [
        (2080, 1, True)]
    (s,) = S.segments(S.CASES["exact2_u16k"], 1)
    assert s.bytes == 16384 and S.tile_walk(s, 16, "pipelined") == [(16384, 2, False, False)]
    (s,) = S.segments(S.CASES["e16_u16k"], 1)
    assert [t[:3] for t in S.tile_walk(s, 16, "pipelined")] == [(3360, 1, True)]
    # some pipelined tile starts inside a row
    assert any(mid for _, w in _walks(1, "pipelined", (16,)) for _, _, _, mid in w)


def test_grid_cases_are_multi_tile():
    """The grid-stride cases hold more tiles than the largest cap the device test sets, so one
    workgroup walks several tiles, of several segments and widths in `several`."""
    routines = set()
    for name in S.GRID_CASES:
        case = S.CASES[name]
        for d in (0, 1):
            with S.SPlan(case, d) as p:
                assert p.n_tiles() >= 3, name
            routines |= {f[0] for f in S.expected_forms(case, d)}
    assert routines == {"tile", "pipelined"}
    c = S.CASES["several"]
    assert len({f[1] for f in S.expected_forms(c, 0)}) >= 4  # 16, 4, 2 and 1-B vectors
    slot0 = [e for e in c.ents if e.buffer_slot == 0]
    assert len(slot0) == 2 and slot0[1].buffer_offset % 16 == 4


def test_entries_of_two_boxes():
    """An entry of two boxes plans two segments, the second's buf_off advanced by the first
    box's bytes (assert_planned), over the same element offsets as the uncut box: on long rows,
    on short rows, under the pipelined unpack and beside another entry in one buffer."""
    for name, second in (("long16_2box", [48000]), ("long16_2box_u16k", [48000]),
                         ("short1_2box", [1050]), ("two_entries_2box", [24480, 85760 + 70800])):
        case = S.CASES[name]
        for d in (0, 1):
            segs = S.segments(case, d)
            assert len(segs) == 2 * len(case.ents)
            assert [s.buf_off for s in segs[1::2]] == second
        for e in case.ents:
            assert np.array_equal(A.element_offsets(e.case.layout, e.case.strides, e.case.offs,
                                                    e.boxes), S.case_offsets(e))
    assert S.expected_forms(S.CASES["long16_2box_u16k"], 1) == [("pipelined", 16, 0)] * 2


def test_tuned_blocks_nest(ghx):
    """A plan created inside a tuned block by the cached helpers (a nested block) neither
    inherits the caller's knobs nor takes them away: after it the caller's knobs are in force
    again, which a plan created then shows."""
    outer = S.with_knobs(S.CASES["long16"], unpack_tile_bytes=32768, grid_cap=3)
    fresh = S.with_knobs(S.CASES["long8"], tile_records=0, grid_cap=9)  # never planned before
    with S.SPlan(outer, 1) as p:
        assert p.knobs_in_force() and S.knobs_in_force()["grid_cap"] == 3
        (inner,) = S.segments(fresh, 1)  # opens and closes a block of its own
        assert (inner.tile_bytes, inner.pipe) == (8192, 0)  # not the caller's 32 KiB
        assert p.knobs_in_force() and S.knobs_in_force()["grid_cap"] == 3
        with S.SPlan(S.CASES["long16"], 1) as q:
            assert not p.knobs_in_force() and q.knobs_in_force()
            assert (q.segments()[0].tile_bytes, q.segments()[0].pipe) == (8192, 0)
        with A.Plan(A.case_entry(S.shape("long16")), 1) as q:  # under the caller's knobs again
            assert (q.segments()[0].tile_bytes, q.segments()[0].pipe) == (32768, 1)
    assert S.knobs_in_force() == {}
    with A.Plan(A.case_entry(S.shape("long16")), 1) as q:
        assert (q.segments()[0].tile_bytes, q.segments()[0].pipe) == (8192, 0)


# ---------------------------------------------------------------------------------------------
# the arena's closure: a wrong form lands in sentinel memory
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.CASES))
def test_arena_closure(name):
    """Every correct access lies inside its field's region with GUARD bytes to spare on both
    sides; every address of the one-division and of the two-division short form applied to the
    same segment lies inside the arena; regions and messages do not overlap; a case is a few
    hundred KiB."""
    case, lay = S.CASES[name], S.layout(S.CASES[name])
    assert lay.arena_bytes <= 1 << 20 and lay.buffers_bytes <= 1 << 20
    prev = 0
    for k, (e, reg) in enumerate(zip(case.ents, lay.fields)):
        mine = [s for s in S.segments(case, 0) if s.field_slot == k]
        assert len(mine) == len(e.boxes)
        off = S.case_offsets(e)
        a, b = reg.span
        assert a == prev and b <= lay.arena_bytes and reg.ptr % 256 == e.fshift
        prev = b
        assert a + S.GUARD <= reg.ptr + off.min()
        assert reg.ptr + off.max() + e.case.elem <= b - S.GUARD
        # the planner's rows are the enumerator's
        # the planner's rows, box after box, are the enumerator's
        exact = np.concatenate([S.exact_row_offsets(s) for s in mine])
        assert np.array_equal(exact, off.reshape(-1, mine[0].row_bytes // e.case.elem)[:, 0])
        for s in mine:
            for wrong in S.other_form_row_offsets(s).values():
                assert a <= reg.ptr + wrong.min()
                assert reg.ptr + wrong.max() + s.row_bytes <= b
    spans = sorted(lay.msg)
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 + S.PAD <= b0
    assert spans[0][0] >= S.GUARD and spans[-1][1] + S.GUARD <= lay.buffers_bytes
    for k, e in enumerate(case.ents):
        assert lay.msg[k][0] == lay.buf_ptr[e.buffer_slot] + e.buffer_offset
        assert lay.buf_ptr[e.buffer_slot] % 256 == case.bshift[e.buffer_slot]


@pytest.mark.parametrize("name,forms", [("outer3", (1,)), ("outer3_g", (1,)), ("outer4", (1, 2)),
                                        ("outer4_g", (1, 2))])
def test_a_wrong_form_fails_the_comparison_inside_the_arena(name, forms):
    """The broken kernel, on the host: a gather that addresses the rows by a short form the
    segment must not take (one division on a segment of three outer dims; either short form on
    one of four) reads inside the arena and returns another message. (Where a segment fits a
    short form, fast_addr = 0 included, that form addresses the same cells: nothing to see.)"""
    case = S.CASES[name]
    (e,), (s,), lay = case.ents, S.segments(case, 0), S.layout(case)
    idx = S.arena_indices(case)[0]
    arena = np.zeros(lay.arena_bytes, dtype=np.uint8)
    arena[idx] = np.random.default_rng(3).integers(1, 256, size=idx.size, dtype=np.uint8)
    want = arena[idx]
    exact = S.exact_row_offsets(s)
    for nd in forms:
        rows = S.other_form_row_offsets(s)[nd]
        assert not np.array_equal(rows, exact)
        got = arena[A.word_indices(rows, s.row_bytes, 1, lay.fields[0].ptr)]
        assert got.size == want.size and not np.array_equal(got, want)
    for nd in {1, 2} - set(forms):
        assert np.array_equal(S.other_form_row_offsets(s)[nd], exact)


# ---------------------------------------------------------------------------------------------
# puts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.PUTS))
def test_put_facts(ghx, name):
    """Source and target segments share rows and extents behind different strides; the form at
    aligned bases is the table's; regions are disjoint and hold both short forms' addresses; the
    put's tile count is the source plan's."""
    put = S.PUTS[name]
    s, q = S.put_segments(put)
    assert A.seg_facts(s) == put.src.expect and A.seg_facts(q) == put.dst.expect
    assert (s.row_bytes, s.bytes, tuple(s.ext)) == (q.row_bytes, q.bytes, tuple(q.ext))
    assert tuple(s.stride) != tuple(q.stride)
    size, src, dst = S.put_layout(put)
    assert size <= 1 << 20 and src.span[1] <= dst.span[0]
    assert (src.ptr % 256, dst.ptr % 256) == (put.sshift, put.dshift)
    assert put.sshift != put.dshift or put.sshift == 0  # shifted cases: the two sides differ
    assert S.put_form(s, q, src.ptr, dst.ptr) == put.form
    for reg, seg, c in ((src, s, put.src), (dst, q, put.dst)):
        off = A.case_offsets(c)
        assert reg.span[0] + S.GUARD <= reg.ptr + off.min()
        assert reg.ptr + off.max() + c.elem + S.GUARD <= reg.span[1]
        for wrong in S.other_form_row_offsets(seg).values():
            assert reg.span[0] <= reg.ptr + wrong.min()
            assert reg.ptr + wrong.max() + seg.row_bytes <= reg.span[1]
    (es, _), (ed, _) = S.put_entries(put)
    h = ctypes.c_void_p()
    with S.tuned(put.knobs):
        ghx.call("ghx_put_create", ctypes.byref(es), 1, ctypes.byref(ed), 1, ctypes.byref(h))
    try:
        nb, nt = ctypes.c_uint64(), ctypes.c_int32()
        ghx.call("ghx_put_info", h, ctypes.byref(nb), ctypes.byref(nt))
    finally:
        ghx.lib().ghx_put_destroy(h)
    walk = S.tile_walk(s, put.form[1])
    assert nb.value == put.src.nbytes and nt.value == len(walk)


def test_put_form_closure():
    """copy_direct<W> at every width, general; copy_direct<8, 1> and <16, 1>; on long rows and on
    short rows. The grid-stride cases are multi-tile with a partial last tile."""
    seen = {p.form for p in S.PUTS.values()}
    assert seen == {("direct", W, 0) for W in (1, 2, 4, 8, 16)} | {("direct", 8, 1),
                                                                     ("direct", 16, 1)}
    for rows in ("long16", "short16"):
        got = {p.form for n, p in S.PUTS.items() if n.startswith(rows)}
        assert got == seen, rows
    for name in S.PUT_GRID_CASES:
        s, _ = S.put_segments(S.PUTS[name])
        walk = S.tile_walk(s, S.PUTS[name].form[1])
        assert len(walk) == 11 and walk[-1][0] < walk[0][0]
    assert {S.PUTS[n].form for n in S.PUT_GRID_CASES} == {("direct", 16, 1), ("direct", 1, 0),
                                                          ("direct", 8, 0)}


# ---------------------------------------------------------------------------------------------
# fused self exchange: the forms of the twin plans at aligned pointers
# ---------------------------------------------------------------------------------------------
def _self_forms(c):
    from ghex_amd import make_context
    _, pc = S.self_pattern(c, make_context())
    with S.tuned(S.self_twin_knobs(c)):
        pairs = S.self_pairs(S.self_field_desc(c), pc)
    assert len(pairs) == 26
    return pairs, S.self_forms(pairs, c.shift * c.elem, 0)


def test_self_forward_widths(ghx):
    """Halo-1 domains of 1, 2, 4, 8 and 16-B elements forward at the element's width: the short
    form at 8 and 16 B, the general form below; fast_addr = 0 gives the general form there too;
    a view that starts 8 B into its storage narrows 16-B rows to 8-B vectors."""
    seen = set()
    for name in S.SELF_DTYPES:
        c = S.SELF_CASES[name]
        _, forms = _self_forms(c)
        assert set(forms) == {("forward", c.elem, int(c.elem >= 8))}, name
        seen |= set(forms)
    assert {W for _, W, _ in seen} == {1, 2, 4, 8, 16}
    for name, W in (("float64_g", 8), ("complex128_g", 16)):
        assert set(_self_forms(S.SELF_CASES[name])[1]) == {("forward", W, 0)}
    pairs, forms = _self_forms(S.SELF_CASES["float64_h2_shift1"])
    assert set(forms) == {("forward", 8, 1)} and {s.wlog2 for s, _ in pairs} == {4}


@pytest.mark.parametrize("name", ["split", "split_walk"])
def test_self_split_pairs(ghx, name):
    """float32, halo 4 in x, 6 interior cells in rows of 16: the send faces start 16 B and 24 B
    into a row, the halos 0 B and 40 B in, so 18 of the 26 pairs pack and unpack at different
    widths (16 B one side, 8 B the other) and pass the barrier; the 8 others forward."""
    c = S.SELF_CASES[name]
    pairs, forms = _self_forms(c)
    split = [f for f in forms if f[0] == "split"]
    assert len(split) == 18 and len([f for f in forms if f[0] == "forward"]) == 8
    assert {f[1] for f in split} == {(16, 8), (8, 16)}
    assert any((s.wlog2, q.wlog2) == (4, 3) for s, q in pairs)
    if name == "split_walk":
        # tiles in segment order under five workgroups: every one of them takes a split tile
        # right after a forward tile, and a forward tile right after a split tile
        walks = S.self_workgroup_walks(pairs, forms, dict(c.knobs)["grid_cap"])
        assert len(walks) == 5 and min(len(w) for w in walks) > 10
        for w in walks:
            steps = set(zip(w, w[1:]))
            assert ("forward", "split") in steps and ("split", "forward") in steps
