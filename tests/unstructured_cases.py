"""Index-list pack / unpack in every row form, vector width and tiling: the case table shared by
tests/test_unstructured_cases.py (host) and tests/test_gpu_uforms.py (device), with the element
enumerator both use as reference, the launch form a case must take and the arena its fields and
buffers live in, and a numpy model of the kernel's tile walk over the planner's records. Usable
without a GPU: plans are created and read back (ghx_uplan_segment) without a device.

The kernel under test is copy_tile_u (ghx_kernels.hip) reached through k_copy<*, seg_u, RUNS =
false>: three offset forms chosen by seg_u::mode,
    0: row r = index r, its levels contiguous (levels first, level stride 1; or one level)
    1: row r = (i, l) = (r / levels, r % levels)   (levels first, strided levels)
    2: row r = (l, i) = (r / n, r % n)             (levels last)
each element at (lid[i] * index_stride + l * level_stride) * elem from the field pointer, lids
from an int32 or int64 device table, vectors of W in {1, 2, 4, 8, 16} bytes.

A case is a plan: fields (descriptor + where the field pointer sits) and lists (which field,
how many lids, where in which buffer). Every list has its own buffer slot."""
from __future__ import annotations

import ctypes
import functools
from dataclasses import dataclass, field as dc_field
from typing import Tuple

import numpy as np

GUARD = 256                 # sentinel bytes kept around every field and every buffer
BIAS = (1 << 31) + 5        # lid_bias of the int64-table cases (as tests/test_gpu_urun.py)
FAR_ARENA_BYTES = 4831838208  # 4.5 GiB: the module-scoped arena of the two far cases
KU, BLOCK = 4, 256          # copy_tile_u: vectors in flight per lane, lanes per workgroup

# planner defaults of the knobs that shape an index-list launch (ghx_internal.hpp, tuning)
DEFAULT_KNOBS = {"u_tile_rows": 512, "u_tile_bytes": 16384, "small_row_bytes": 64,
                 "u_run_tile_rows": 2048, "urun": 1, "short_pol": 0, "tile_records": 1,
                 "grid_cap": 0}


@dataclass(frozen=True)
class Field:
    elem: int
    levels: int
    levels_first: bool
    index_stride: int     # elements
    level_stride: int     # elements
    shift: int = 0        # the field pointer's offset from a 256-B aligned address

    @property
    def isb(self):
        return self.index_stride * self.elem

    @property
    def lsb(self):
        return self.level_stride * self.elem

    @property
    def mode(self):
        """uplan::uplan: one row per index when its levels are contiguous on both sides."""
        if self.levels == 1 or (self.levels_first and self.level_stride == 1):
            return 0
        return 1 if self.levels_first else 2


@dataclass(frozen=True)
class LidList:
    field: int            # index into Case.fields (= the entry's field slot)
    n: int                # lids
    buffer_offset: int = 0
    buf_shift: int = 0    # the buffer pointer's offset from a 256-B aligned address


@dataclass(frozen=True)
class Case:
    name: str
    fields: Tuple[Field, ...]
    lists: Tuple[LidList, ...]
    ncells: int = 10007   # lids are drawn from [0, ncells)
    seed: int = 0
    lid_bias: int = 0     # added to every lid; the field pointer moves back by the same cells
    knobs: Tuple[Tuple[str, int], ...] = ()
    repeats: bool = False  # lids drawn with repetition: pack only (the gather is defined)
    far: bool = False      # lives in the 4.5-GiB arena (device tests only)
    lid_ranges: Tuple[Tuple[int, int], ...] = ()  # far mode 1: lids drawn from these ranges

    @property
    def message_bytes(self):
        return sum(l.n * self.fields[l.field].levels * self.fields[l.field].elem
                   for l in self.lists)


def uniform(name, elem, levels, levels_first, index_stride, level_stride, *, shift=0,
            buffer_offset=0, buf_shift=0, n=3001, lists=3, **kw):
    """`lists` lists (n, n + 1, ... lids) of one field, every buffer placed alike."""
    f = Field(elem, levels, levels_first, index_stride, level_stride, shift)
    return Case(name, (f,), tuple(LidList(0, n + k, buffer_offset, buf_shift)
                                  for k in range(lists)), **kw)


# ---------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------
NCELLS = 10007


def _mode_field(mode, elem, shift=0, variant=0):
    """A field of 3 levels (variant 1: 5) that plans as `mode`, at most ~0.8 MB with 16-B elements.
    mode 0: levels contiguous, index stride levels + 1 (rows of levels * elem bytes, never 4 or
    8 B wide with the index stride equal to the row: off the run path);
    mode 1: levels first with level stride 2 inside an index stride of 2 * levels - 1, or
    (variant 1) level-major memory walked index-major: index stride 1, level stride ncells + 3;
    mode 2: levels last, level stride ncells + 3 (a padded level), index stride 1."""
    L = 5 if variant else 3
    if mode == 0:
        return Field(elem, L, True, L + 1, 1, shift)
    if mode == 1:
        if variant:
            return Field(elem, L, True, 1, NCELLS + 3, shift)
        return Field(elem, L, True, 2 * L - 1, 2, shift)
    return Field(elem, L, False, 1, NCELLS + 3, shift)


def _grid_cases():
    """{mode 0 off the run path, 1, 2} x W in {1, 2, 4, 8, 16} x {int32, int64} lid table.
    int32 column: the element size gives W (1, 2, 4, 8, 16 B elements, aligned pointers).
    int64 column: a wider element narrowed to W by misalignment alone: field shifts and buffer
    offsets / shifts from {1, 2, 4, 8, 24}; W = 16 has nothing wider and keeps 16-B elements."""
    out = []
    narrowed = {1: (4, dict(shift=1)), 2: (8, dict(buffer_offset=2)),
                4: (16, dict(buf_shift=4)), 8: (16, dict(shift=24)),
                16: (16, dict(buffer_offset=16))}
    for mode in (0, 1, 2):
        for W in (1, 2, 4, 8, 16):
            f = _mode_field(mode, W)
            out.append(Case(f"m{mode}_w{W}_i32", (f,),
                            tuple(LidList(0, 3001 + k) for k in range(3)),
                            seed=100 * mode + W))
            elem, mis = narrowed[W]
            f = _mode_field(mode, elem, mis.get("shift", 0), variant=1 if mode == 1 else 0)
            out.append(Case(f"m{mode}_w{W}_i64", (f,),
                            tuple(LidList(0, 3001 + k, mis.get("buffer_offset", 0),
                                          mis.get("buf_shift", 0)) for k in range(3)),
                            seed=100 * mode + W + 50, lid_bias=BIAS))
    return out


def _extra_cases():
    out = []
    # non-power-of-two elements: 3 B (W = 1) and 12 B (W = 4) in every mode. 12-B rows in 512-row
    # tiles are 1.5 loop trips of 4 * 256 * 4 B: the clamp of a partial second trip
    for mode in (0, 1, 2):
        for elem in (3, 12):
            f = _mode_field(mode, elem) if mode else Field(elem, 1, True, 2, 1)
            out.append(Case(f"m{mode}_e{elem}", (f,),
                            tuple(LidList(0, 3001 + k) for k in range(3)),
                            seed=300 + 10 * mode + elem))
    # mode 0, 24-B rows of fp64 at W = 8: 512-row tiles of 1.5 loop trips
    out.append(uniform("m0_rows24", 8, 3, True, 3, 1, seed=340))
    # mode 0, long rows (>= small_row_bytes: u_tile_bytes tiles): 5 levels of 16 B, padded
    out.append(uniform("m0_long80", 16, 5, True, 6, 1, seed=341))
    # the same with an int64 table: the lid64 branch on long rows
    out.append(uniform("m0_long80_i64", 16, 5, True, 6, 1, seed=342, lid_bias=BIAS))
    # mode 0 rows of 8 B that stay off the run path only through the buffer offset (8) and
    # through the field pointer (4-B shift): one-row-per-lane general path at W = 8 and W = 4
    out.append(uniform("m0_fp64_bufoff8", 8, 1, True, 1, 1, buffer_offset=8, seed=343))
    out.append(uniform("m0_fp64_shift4", 8, 1, True, 1, 1, shift=4, seed=344))
    # mode 2 with an index stride of 2 and an even level padding: W = 16 from 8-B elements
    out.append(Case("m2_istride2", (Field(8, 4, False, 2, 2 * NCELLS + 6),),
                    tuple(LidList(0, 3001 + k) for k in range(3)), seed=345))
    # single-lid lists: the index stride (20 B) does not bound W when n == 1 (planner rule), so
    # the 16-B rows of the two one-lid lists move as 16-B vectors from 4-B aligned addresses
    out.append(Case("m0_single", (Field(4, 4, True, 5, 1),),
                    (LidList(0, 1), LidList(0, 3001), LidList(0, 1)), seed=346))
    # pack only: lids repeat (the gather is defined for repeats, the scatter is not)
    for mode in (0, 1, 2):
        out.append(Case(f"m{mode}_repeats", (_mode_field(mode, 8),),
                        tuple(LidList(0, 3001 + k) for k in range(3)), seed=350 + mode,
                        repeats=True))
    # one launch of all three modes plus a run-eligible 4-B-row entry: `runs` must hold for
    # every segment, so the launch drops to the general kernel for all four
    out.append(Case("mixed", (_mode_field(0, 8), _mode_field(1, 4), _mode_field(2, 16),
                              Field(4, 1, True, 1, 1)),
                    (LidList(0, 3001), LidList(1, 3002, 8), LidList(2, 3003, 0, 8),
                     LidList(3, 3004, 16)), seed=360))
    return out


def _far_cases():
    """Offsets past 2^32 in the 4.5-GiB arena, the field pointer at the arena's base so that an
    offset wrapped to 32 bits falls inside the arena too.
    far_m2: fp64, 2 levels, level stride 2^29 + 3 elements: level_stride_b = 2^32 + 24;
    far_m1: fp64, 3 levels with level stride 2 in an index stride of 5 (40 B): lids from two
    bands either side of 2^32 / 40, so lid * index_stride_b passes 2^32 for half of them."""
    edge = (1 << 32) // 40
    return [
        Case("far_m2", (Field(8, 2, False, 1, (1 << 29) + 3),),
             tuple(LidList(0, 3001 + k) for k in range(3)), seed=400, far=True),
        Case("far_m1", (Field(8, 3, True, 5, 2),),
             tuple(LidList(0, 3001 + k) for k in range(3)), seed=401, far=True,
             lid_ranges=((edge - 6000, edge - 1000), (edge + 1000, edge + 6000))),
    ]


CASES = {c.name: c for c in _grid_cases() + _extra_cases() + _far_cases()}
HOST_SIZED = tuple(n for n, c in CASES.items() if not c.far)
FAR = tuple(n for n, c in CASES.items() if c.far)


def with_knobs(case: Case, **knobs) -> Case:
    import dataclasses
    merged = dict(case.knobs)
    merged.update(knobs)
    return dataclasses.replace(case, knobs=tuple(sorted(merged.items())))


def knob(case: Case, name):
    return dict(case.knobs).get(name, DEFAULT_KNOBS[name])


# ---------------------------------------------------------------------------------------------
# lids and the reference enumeration
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lids_cached(case: Case):
    rng = np.random.default_rng(1000 + case.seed)
    out = [None] * len(case.lists)
    for fi in range(len(case.fields)):
        mine = [k for k, l in enumerate(case.lists) if l.field == fi]
        total = sum(case.lists[k].n for k in mine)
        if case.lid_ranges:
            pool = np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in case.lid_ranges])
        else:
            pool = np.arange(case.ncells, dtype=np.int64)
        if case.repeats:
            drawn = rng.choice(pool[:total // 2], size=total, replace=True)
        else:
            assert total <= pool.size
            drawn = rng.permutation(pool)[:total]
        a = 0
        for k in mine:
            out[k] = np.ascontiguousarray(drawn[a:a + case.lists[k].n] + case.lid_bias)
            out[k].setflags(write=False)
            a += case.lists[k].n
    return tuple(out)


def lids(case: Case):
    """The case's lid lists as the plan gets them (int64, lid_bias included). Within a field the
    lists are disjoint and free of repeats (an unpack plan's scatter is order-independent),
    except in the pack-only `repeats` cases."""
    return _lids_cached(case)


def _form_offsets(f: Field, lid, form):
    """Field byte offset of every element of one list in buffer order, by offset form `form`
    (the list's own when form == f.mode)."""
    n, L = lid.size, f.levels
    base = lid * np.int64(f.isb)
    lev = np.arange(L, dtype=np.int64)
    if form == 0:      # i-major, the levels of an index contiguous
        return (base[:, None] + (lev * np.int64(f.elem))[None, :]).reshape(-1)
    if form == 1:      # i-major, levels level_stride apart
        return (base[:, None] + (lev * np.int64(f.lsb))[None, :]).reshape(-1)
    return ((lev * np.int64(f.lsb))[:, None] + base[None, :]).reshape(-1)  # l-major


def element_offsets(case: Case):
    """Per list: the field byte offset (from the field pointer the plan is executed with) of
    every message element in buffer order, int64: (lid * index_stride + l * level_stride) *
    elem, i-major when levels_first, l-major otherwise."""
    out = []
    for l, lid in zip(case.lists, lids(case)):
        f = case.fields[l.field]
        out.append(_form_offsets(f, lid, 1 if f.levels_first else 2))
    return out


def other_form_offsets(case: Case):
    """Per list: {form: offsets} of the two offset forms the list's segment must NOT take, for
    the same segment (same lids, levels and strides): what a kernel that decodes the rows with
    another mode's formula would address, its table index still inside the list. (A kernel that
    runs another mode's BRANCH on this segment's record divides by the wrong quantity and may
    index the lid table past the list: the table is the plan's own allocation, which no arena
    of the test's can contain.)"""
    out = []
    for l, lid in zip(case.lists, lids(case)):
        f = case.fields[l.field]
        out.append({m: _form_offsets(f, lid, m) for m in (0, 1, 2) if m != f.mode})
    return out


def wrapped_offsets(case: Case):
    """Per list: the element offsets with lid * index_stride_b and l * level_stride_b each
    truncated to 32 bits (unsigned), as a short-form addressing that overflows would give."""
    M = np.int64(0xFFFFFFFF)
    out = []
    for l, lid in zip(case.lists, lids(case)):
        f = case.fields[l.field]
        base = (lid * np.int64(f.isb)) & M
        lev = (np.arange(f.levels, dtype=np.int64) * np.int64(f.lsb)) & M
        if f.levels_first:
            out.append((base[:, None] + lev[None, :]).reshape(-1))
        else:
            out.append((lev[:, None] + base[None, :]).reshape(-1))
    return out


def byte_indices(off, elem, base=0):
    """Byte positions [o + base, o + base + elem) of every element offset o, in order."""
    return (off[:, None] + np.int64(base) + np.arange(elem, dtype=np.int64)[None, :]).reshape(-1)


# ---------------------------------------------------------------------------------------------
# the arena: where fields and buffers sit
# ---------------------------------------------------------------------------------------------
@dataclass
class Layout:
    arena_bytes: int
    field_ptr: list        # per field: the field pointer's byte offset from the arena's base
    #                        (negative with lid_bias: the pointer lies before the arena)
    region: list           # per field: (first, last + 1) arena byte of its region, guards included
    buffers_bytes: int
    buf_ptr: list          # per list: the buffer pointer's offset in the buffer allocation
    msg: list              # per list: (first, last + 1) byte of its message in that allocation
    bytes_: list = dc_field(default_factory=list)  # per list: message bytes


def _round_up(x, a):
    return (int(x) + a - 1) // a * a


@functools.lru_cache(maxsize=None)
def layout(case: Case) -> Layout:
    """Fields back to back in one zero-filled allocation (its base at least 256-B aligned), each
    between guard bands: GUARD bytes below the lowest and above the highest byte that the right
    OR either wrong offset form addresses, so a wrong-form access stays inside the arena and a
    stray store next to the field is seen. Buffers likewise in a second allocation: GUARD bytes,
    the buffer pointer (+ buf_shift), buffer_offset bytes the plan must not touch, the message,
    GUARD bytes. A far case's single field starts at the base of the 4.5-GiB arena."""
    right, wrong = element_offsets(case), other_form_offsets(case)
    fptr, region, pos = [], [], 0
    for fi, f in enumerate(case.fields):
        lo = hi = None
        for k, l in enumerate(case.lists):
            if l.field != fi:
                continue
            for o in [right[k]] + list(wrong[k].values()):
                lo = int(o.min()) if lo is None else min(lo, int(o.min()))
                hi = int(o.max()) + f.elem if hi is None else max(hi, int(o.max()) + f.elem)
        if case.far:
            assert len(case.fields) == 1 and lo >= 0
            fptr.append(f.shift)
            region.append((0, FAR_ARENA_BYTES))
            pos = FAR_ARENA_BYTES
            continue
        # the pointer is congruent to f.shift mod 256 (lid_bias moves it by whole cells)
        start = pos + GUARD
        p = start - lo
        p += (f.shift - p) % 256
        fptr.append(p)
        end = _round_up(p + hi + GUARD, 256)
        region.append((pos, end))
        pos = end
    bptr, msg, nbytes, bpos = [], [], [], 0
    for l in case.lists:
        f = case.fields[l.field]
        nb = l.n * f.levels * f.elem
        p = bpos + GUARD + l.buf_shift
        bptr.append(p)
        msg.append((p + l.buffer_offset, p + l.buffer_offset + nb))
        nbytes.append(nb)
        bpos = _round_up(p + l.buffer_offset + nb + GUARD, 256)
    return Layout(pos, fptr, region, bpos, bptr, msg, nbytes)


def arena_indices(case: Case):
    """Per list: the arena byte index of every message byte in buffer order (int64)."""
    lay = layout(case)
    return [byte_indices(o, case.fields[l.field].elem, lay.field_ptr[l.field])
            for l, o in zip(case.lists, element_offsets(case))]


# ---------------------------------------------------------------------------------------------
# the form a launch must take (restated from uplan::uplan, uplan::execute and k_copy)
# ---------------------------------------------------------------------------------------------
def _wlog2(x):
    """log2 of the largest power of two <= 16 that divides x (16 for 0)."""
    x = abs(int(x))
    w = 0
    while w < 4 and x % (2 << w) == 0:
        w += 1
    return w


def planned(case: Case):
    """Per list what the planner must report: (mode, wlog2, lid64, runs > 0, row_bytes, bytes).
    wlog2 is the largest power of two <= 16 dividing the row length, buffer_offset and the byte
    strides (the index stride only when n > 1, the level stride only when mode != 0)."""
    out = []
    for l, lid in zip(case.lists, lids(case)):
        f = case.fields[l.field]
        mode = f.mode
        row = f.levels * f.elem if mode == 0 else f.elem
        w = min(_wlog2(row), _wlog2(l.buffer_offset))
        if l.n > 1:
            w = min(w, _wlog2(f.isb))
        if mode != 0:
            w = min(w, _wlog2(f.lsb))
        lid64 = int(bool((lid >= (1 << 31)).any()))
        runs = bool(knob(case, "urun") and mode == 0 and row in (4, 8) and f.isb == row
                    and l.buffer_offset % 16 == 0)
        out.append((mode, w, lid64, runs, row, l.n * f.levels * f.elem))
    return out


def expected_form(case: Case, field_base=0, buffer_base=0):
    """Per list the (mode, W, lid64, runs) its launch must take, the allocations' base addresses
    given (any multiple of 16 gives the same answer). W: the planned width narrowed by the actual
    field pointer and the actual buffer pointer + offset. runs: the launch takes the run-path
    kernel, which needs every segment flagged by the planner, tiles of whole 16-B chunks, 16-B
    aligned buffer ranges and a field pointer aligned to the row; otherwise all segments take
    copy_tile_u."""
    assert field_base % 16 == 0 and buffer_base % 16 == 0
    lay, plan = layout(case), planned(case)
    tb = tile_bytes_rule(case)
    runs = all(p[3] and t % 16 == 0 and (buffer_base + lay.msg[k][0]) % 16 == 0
               and (field_base + lay.field_ptr[l.field]) % p[4] == 0
               for k, (l, p, t) in enumerate(zip(case.lists, plan, tb)))
    out = []
    for k, (l, p) in enumerate(zip(case.lists, plan)):
        w = min(p[1], _wlog2(field_base + lay.field_ptr[l.field]),
                _wlog2(buffer_base + lay.msg[k][0]))
        out.append((p[0], 1 << w, p[2], runs))
    return out


def tile_bytes_rule(case: Case):
    """Per list the planner's tile (build_tiles): u_tile_rows rows of rows shorter than
    small_row_bytes (at most 1 MiB), else u_tile_bytes; whole rows, at least one. (Run-heavy
    lists, runs == 2, take u_run_tile_rows; the table has none: its lids are random.)"""
    out = []
    for p in planned(case):
        row = p[4]
        if row < knob(case, "small_row_bytes"):
            tb = max(row, min(knob(case, "u_tile_rows") * row, 1 << 20))
        else:
            tb = max(knob(case, "u_tile_bytes"), row)
        out.append(tb - tb % row)
    return out


# ---------------------------------------------------------------------------------------------
# plans through the C ABI
# ---------------------------------------------------------------------------------------------
def entries(case: Case):
    """The case's ghx_upack_entry array: list k on field slot = its field, buffer slot k.
    Returns (array, keep-alive)."""
    from ghex_amd import _ghx
    ents, keep = [], lids(case)
    for k, (l, lid) in enumerate(zip(case.lists, keep)):
        f = case.fields[l.field]
        e = _ghx.UPackEntry()
        e.data.elem_size, e.data.levels = f.elem, f.levels
        e.data.levels_first = 1 if f.levels_first else 0
        e.data.index_stride, e.data.level_stride = f.index_stride, f.level_stride
        e.field_slot, e.buffer_slot, e.buffer_offset = l.field, k, l.buffer_offset
        e.lids, e.n_lids = _ghx.i64_ptr(lid), lid.size
        ents.append(e)
    return (_ghx.UPackEntry * len(ents))(*ents), keep


class UPlan:
    """A ghx_uplan of a case (pack 0 / unpack 1) created under the case's knobs, which stay set
    while the plan lives (grid_cap is read at launch); destroyed, and the knobs reset, on exit."""

    def __init__(self, case: Case, direction):
        from ghex_amd import _ghx
        self._ents, self._keep = entries(case)
        self.h = ctypes.c_void_p()
        try:
            for k, v in case.knobs:
                _ghx.call("ghx_tune", k.encode(), int(v))
            _ghx.call("ghx_uplan_create", self._ents, len(case.lists), direction,
                      ctypes.byref(self.h))
        except Exception:
            _ghx.call("ghx_tune", b"reset", 0)
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        from ghex_amd import _ghx
        _ghx.lib().ghx_uplan_destroy(self.h)
        self.h = None
        _ghx.call("ghx_tune", b"reset", 0)

    def segments(self):
        from ghex_amd import _ghx
        n = ctypes.c_int32()
        _ghx.call("ghx_uplan_info", self.h, None, ctypes.byref(n), None)
        out = []
        for k in range(n.value):
            s = _ghx.USegmentInfo()
            _ghx.call("ghx_uplan_segment", self.h, k, ctypes.byref(s))
            out.append(s)
        return out


def planner_facts(s):
    """A segment as planned() states it."""
    return (s.mode, s.wlog2, s.lid64, s.runs > 0, s.row_bytes, s.bytes)


def assert_planned(case: Case, segs):
    """One segment per list in plan order, each as planned() says, its tile a whole number of
    rows and as tile_bytes_rule() says, its slots and strides the entry's."""
    assert len(segs) == len(case.lists)
    for k, (s, l, want, tb) in enumerate(zip(segs, case.lists, planned(case),
                                             tile_bytes_rule(case))):
        f = case.fields[l.field]
        assert planner_facts(s) == want, (case.name, k, planner_facts(s), want)
        assert s.tile_bytes > 0 and s.tile_bytes % s.row_bytes == 0
        assert s.tile_bytes == tb, (case.name, k, s.tile_bytes, tb)
        assert (s.field_slot, s.buffer_slot, s.buf_off, s.n) == (l.field, k, l.buffer_offset, l.n)
        assert (s.index_stride_b, s.level_stride_b, s.field_off) == (f.isb, f.lsb, 0)
        small = s.row_bytes < knob(case, "small_row_bytes")
        assert s.fpol == (knob(case, "short_pol") if small else 0)


def tiles(s, W):
    """[(bytes of the tile, loop trips, the last trip is partial)] of a segment at vector width
    W: copy_tile_u moves KU * BLOCK * W bytes per trip."""
    trip = KU * BLOCK * W
    out = []
    for a in range(0, s.bytes, s.tile_bytes):
        nb = min(s.tile_bytes, s.bytes - a)
        out.append((nb, -(-nb // trip), nb % trip != 0))
    return out


def launch_form(segs, field_ptrs, buffer_ptrs):
    """Per segment the (mode, W, lid64, runs) its launch takes, from the planner's records and
    the pointers of the execute call (indexed by slot), as uplan::execute and k_copy decide."""
    runs = all(s.runs and s.tile_bytes % 16 == 0
               and (buffer_ptrs[s.buffer_slot] + s.buf_off) % 16 == 0
               and field_ptrs[s.field_slot] % s.row_bytes == 0 for s in segs)
    return [(s.mode, 1 << min(s.wlog2, _wlog2(field_ptrs[s.field_slot]),
                              _wlog2(buffer_ptrs[s.buffer_slot] + s.buf_off)), s.lid64, runs)
            for s in segs]


def kernel_model(s, W, lid):
    """copy_tile_u's walk over a segment as the planner reports it (numpy, exact integers): for
    every tile [start, end) the lanes whose first position lies inside it take KU positions per
    loop trip, each clamped to the tile's last vector, and decode them by the segment's mode.
    Returns (buffer positions, field byte offsets) of every vector the kernel moves, duplicates
    from the clamp included, and asserts that tiles are whole vectors."""
    levels = s.bytes // s.row_bytes // s.n
    pos = []
    lane = np.arange(BLOCK, dtype=np.int64) * W
    trip = KU * BLOCK * W
    for start in range(0, s.bytes, s.tile_bytes):
        end = min(start + s.tile_bytes, s.bytes)
        assert start % W == 0 and (end - start) % W == 0 and end - start >= W
        base = (start + lane)[None, :] + (np.arange(-(-(end - start) // trip), dtype=np.int64)
                                          * trip)[:, None]
        base = base[base < end]
        p = base[:, None] + (np.arange(KU, dtype=np.int64) * BLOCK * W)[None, :]
        pos.append(np.minimum(p, end - W).reshape(-1))
    p = np.concatenate(pos)
    row = p // s.row_bytes
    rem = p - row * s.row_bytes
    if s.mode == 0:
        idx, extra = row, rem
    elif s.mode == 1:
        idx = row // levels
        extra = (row - idx * levels) * np.int64(s.level_stride_b) + rem
    else:
        lev = row // s.n
        idx = row - lev * s.n
        extra = lev * np.int64(s.level_stride_b) + rem
    assert idx.min() >= 0 and idx.max() < lid.size  # the lid table is read inside the list
    return p, np.int64(s.field_off) + lid[idx] * np.int64(s.index_stride_b) + extra
