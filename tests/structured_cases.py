"""The structured copy kernels in every vector width, offset form and tile walk: the case table
shared by tests/test_structured_cases.py (host) and tests/test_gpu_sforms.py (device), with the
launch form a case must take, a model of the kernels' tile walk and the arena its fields and
buffers live in. Usable without a GPU: plans are created and read back (ghx_plan_segment)
without a device.

The kernels under test (ghx_kernels.hip): k_copy<*, seg_s> with copy_any's choice between
unpack_tile_pipelined<16> and copy_tile<W, AM>; self_pair_tile (k_self) with self_forward<W, AM>,
the pack / barrier / unpack path and the pack-only peer tile; put_pair_tile (k_put) with
copy_direct<W, AM>.

Reference: addressing_cases.element_offsets, the int64 byte offset of every message element in
buffer order. Case descriptors, entries, plans and the oracle tie are addressing_cases' own; a
case here is one or more of its `Case`s (one box each, one field slot each) placed in buffers,
with pointer shifts and the knobs the plan is created and launched under."""
from __future__ import annotations

import ctypes
import dataclasses
import functools
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from tests import addressing_cases as A

GUARD = 256            # sentinel bytes kept around every field region and every buffer
PAD = 64               # of them, the bytes next to a message the device test names explicitly
KU, BLOCK = 4, 256     # copy_tile: vectors in flight per lane, lanes per workgroup
PIPE_STEP = 2 * BLOCK * 16  # unpack_tile_pipelined<16>: kP = 2 vectors of 16 B per lane per step
L3, L4 = (2, 1, 0), (3, 2, 1, 0)

# planner defaults of the knobs that shape a structured launch (ghx_internal.hpp, tuning)
DEFAULT_KNOBS = {"tile_bytes": 8192, "unpack_tile_bytes": 0, "self_tile_bytes": 8192,
                 "small_tile_rows": 0, "small_row_bytes": 64, "tile_records": 1, "grid_cap": 0,
                 "fast_addr": 1}


@dataclass(frozen=True)
class Ent:
    """One entry of a plan: the box of `case` on its own field slot (its index in SCase.ents)."""
    case: A.Case
    buffer_slot: int = 0
    buffer_offset: int = 0
    fshift: int = 0        # the field pointer's offset from a 256-B aligned address
    cut: int = 0           # > 0: two boxes in this one entry, the case's box cut at this index of
    #                        its slowest dim; the message and its element offsets stay the same

    @property
    def slowest(self):
        return self.case.layout.index(0)

    @property
    def boxes(self):
        c, d = self.case, self.slowest
        last = tuple(x - 1 for x in c.ext)
        if not self.cut:
            return [((0,) * c.dim, last)]
        assert 0 < self.cut < c.ext[d]
        lo = tuple(self.cut - 1 if k == d else x for k, x in enumerate(last))
        hi = tuple(self.cut if k == d else 0 for k in range(c.dim))
        return [((0,) * c.dim, lo), (hi, last)]

    @property
    def parts(self):
        """The share of the slowest extent each box holds."""
        n = self.case.ext[self.slowest]
        return [n] if not self.cut else [self.cut, n - self.cut]


@dataclass(frozen=True)
class SCase:
    name: str
    ents: Tuple[Ent, ...]
    bshift: Tuple[int, ...] = (0,)  # per buffer slot: the pointer's offset from 256-B alignment
    knobs: Tuple[Tuple[str, int], ...] = ()

    @property
    def message_bytes(self):
        return sum(e.case.nbytes for e in self.ents)


def with_knobs(case: SCase, **knobs) -> SCase:
    merged = dict(case.knobs)
    merged.update(knobs)
    return dataclasses.replace(case, knobs=tuple(sorted(merged.items())))


def knob(case: SCase, name):
    return dict(case.knobs).get(name, DEFAULT_KNOBS[name])


# ---------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------
# name: (elem, layout, strides, box extents, (row bytes, n_outer, rows, wlog2, amode))
SHAPES = {
    # long rows (>= small_row_bytes): tiles of tile_bytes, which start in the middle of a row
    "long16": (8, L3, (8, 416, 12480), (50, 30, 7), (400, 2, 210, 4, 1)),    # 84,000 B
    "long8": (8, L3, (8, 424, 12720), (51, 30, 7), (408, 2, 210, 3, 1)),     # 85,680 B
    "long4": (4, L3, (4, 80, 3200), (17, 40, 9), (68, 2, 360, 2, 1)),        # 24,480 B, 3 tiles
    "long2": (2, L3, (2, 70, 2800), (33, 40, 9), (66, 2, 360, 1, 1)),        # 23,760 B, 3 tiles
    "long1": (1, L3, (1, 71, 2840), (67, 40, 9), (67, 2, 360, 0, 1)),        # 24,120 B, 3 tiles
    "exact2": (8, L3, (8, 528, 16896), (64, 32, 1), (512, 2, 32, 4, 1)),     # 16,384 B
    "e16": (16, L3, (16, 144, 1296), (5, 7, 6), (80, 2, 42, 4, 1)),          # 16-B elements
    # short rows: tiles of whole rows (512 of them by default)
    "short1": (1, L3, (1, 16, 800), (3, 50, 60), (3, 2, 3000, 0, 1)),
    "short2": (2, L3, (2, 16, 800), (1, 50, 60), (2, 2, 3000, 1, 1)),
    "short4": (4, L3, (4, 16, 800), (1, 50, 60), (4, 2, 3000, 2, 1)),
    "short8": (8, L3, (8, 16, 800), (1, 50, 60), (8, 2, 3000, 3, 1)),
    "short12": (4, L3, (4, 16, 800), (3, 50, 60), (12, 2, 3000, 2, 1)),
    "short16": (8, L3, (8, 32, 1600), (2, 50, 60), (16, 2, 3000, 4, 1)),
    "short24": (8, L3, (8, 32, 1600), (3, 50, 60), (24, 2, 3000, 3, 1)),
    # three outer dims: the two-division short form
    "outer3": (8, L4, (8, 96, 1152, 13824), (2, 10, 10, 3), (16, 3, 300, 4, 2)),  # 4,800 B
    # a strided fastest dim: element rows under four outer dims, general whatever the knobs; both
    # short forms address other cells than the exact offsets do
    "outer4": (16, L4, (32, 192, 2304, 27648), (3, 5, 5, 3), (16, 4, 225, 4, 0)),  # 3,600 B
}


def shape(name, wlog2=None, amode=None, tag=""):
    elem, layout, strides, ext, expect = SHAPES[name]
    expect = expect[:3] + (expect[3] if wlog2 is None else wlog2,
                           expect[4] if amode is None else amode)
    return A.Case(name + tag, elem, layout, strides, ext, expect)


def _one(name, shp, *, fshift=0, bshift=0, buffer_offset=0, wlog2=None, **knobs):
    amode = 0 if knobs.get("fast_addr", 1) == 0 else None
    c = shape(shp, wlog2, amode)
    return SCase(name, (Ent(c, 0, buffer_offset, fshift),), (bshift,), tuple(sorted(knobs.items())))


def _table():
    out = []
    # every shape as planned, and its general (amode 0) twin
    for shp in SHAPES:
        out.append(_one(shp, shp))
        out.append(_one(shp + "_g", shp, fast_addr=0))
    # short rows of 1 B in 64-row tiles: 47 tiles of 192 B, every one a partial trip
    out.append(_one("short1_r64", "short1", small_tile_rows=64))
    # pointer shifts of 1, 2, 4 and 8 B on each side separately: 16-B rows narrowed to the shift
    # (amode 1 planned; W in {1, 2} falls to the general form), on long and on short rows
    for shp in ("long16", "short16"):
        for sh in (1, 2, 4, 8):
            out.append(_one(f"{shp}_f{sh}", shp, fshift=sh))
            out.append(_one(f"{shp}_b{sh}", shp, bshift=sh))
    # amode 2 planned, W = 8 at launch: the general form; by the field pointer, by the buffer's
    out.append(_one("outer3_f8", "outer3", fshift=8))
    out.append(_one("outer3_b8", "outer3", bshift=8))
    # buffer_offset 4: the planner's own wlog2 falls to 2
    out.append(_one("long16_off4", "long16", buffer_offset=4, wlog2=2))
    # pack tiles of 16 KiB (one full trip at W = 16) and 64 KiB (4 full trips, then 2 with a
    # partial last)
    out.append(_one("long16_t16k", "long16", tile_bytes=16384))
    out.append(_one("long16_t64k", "long16", tile_bytes=65536))
    # tiles of exactly one full trip at 4, 2 and 1-B vectors (1 KiB is the knob's minimum)
    out.append(_one("long4_t4k", "long4", tile_bytes=4096))
    out.append(_one("long2_t2k", "long2", tile_bytes=2048))
    out.append(_one("long1_t1k", "long1", tile_bytes=1024))
    # two boxes in ONE entry (the box cut along its slowest dim): two segments, the second's
    # buf_off advanced by the first box's bytes inside the entry. long16: 4 + 3 planes, the second
    # segment at 48,000 B; short1: 7 + 53 planes, the second at 1,050 B (2-B aligned only, which
    # 1-B vectors do not mind); with the pipelined unpack; and beside a one-box entry
    c = _one("long16_2box", "long16")
    out.append(dataclasses.replace(c, ents=(dataclasses.replace(c.ents[0], cut=4),)))
    out.append(with_knobs(dataclasses.replace(out[-1], name="long16_2box_u16k"),
                          unpack_tile_bytes=16384))
    c = _one("short1_2box", "short1")
    out.append(dataclasses.replace(c, ents=(dataclasses.replace(c.ents[0], cut=7),)))
    out.append(SCase("two_entries_2box", (
        Ent(shape("long8"), 0, 0, cut=2),
        Ent(shape("short24"), 0, 85680 + 80, fshift=8, cut=59),
    ), (0,)))
    # the pipelined unpack: tiles of 4 steps and a last of 3 with lanes of slot 0 only in the
    # third (32 KiB); tiles of two full steps and a last of one partial step (16 KiB); a whole
    # segment of exactly two full steps; the general twin; 16-B elements
    out.append(_one("long16_u32k", "long16", unpack_tile_bytes=32768))
    out.append(_one("long16_u16k", "long16", unpack_tile_bytes=16384))
    out.append(_one("long16_u32k_g", "long16", unpack_tile_bytes=32768, fast_addr=0))
    out.append(_one("exact2_u16k", "exact2", unpack_tile_bytes=16384))
    out.append(_one("e16_u16k", "e16", unpack_tile_bytes=16384))
    # pipe set, but 8-B vectors by the buffer pointer: copy_tile<8, 1>, four trips per 32-KiB tile
    out.append(_one("long16_u32k_b8", "long16", unpack_tile_bytes=32768, bshift=8))
    out.append(_one("long8_u32k", "long8", unpack_tile_bytes=32768))
    # one plan of entries of different widths: the width is uniform within a workgroup, not across
    # the launch. Entries 0 and 1 share buffer slot 0, the second at an offset that is not
    # 16-aligned (its planned width falls to 4 B); slot 1's pointer is 2-B aligned
    out.append(SCase("several", (
        Ent(shape("long16"), 0, 0),
        Ent(shape("long8", wlog2=2, tag="@84068"), 0, 84068),
        Ent(shape("short1"), 1, 0, fshift=3),
        Ent(shape("outer3"), 2, 0),
        Ent(shape("short24"), 1, 9072, fshift=8),
        Ent(shape("long2"), 2, 4864),
    ), (0, 2, 0)))
    out.append(with_knobs(dataclasses.replace(out[-1], name="several_u32k"),
                          unpack_tile_bytes=32768))
    return out


CASES = {c.name: c for c in _table()}

# multi-tile cases of each routine (copy_tile, pipelined unpack) for the grid-stride walk
GRID_CASES = ("long16", "long1", "short1_r64", "long16_u32k", "long16_u16k", "long16_u32k_b8",
              "long16_2box_u16k", "several", "several_u32k")


# ---------------------------------------------------------------------------------------------
# what the planner must report
# ---------------------------------------------------------------------------------------------
def _wlog2(x):
    """log2 of the largest power of two <= 16 that divides x (16 for 0)."""
    x = abs(int(x))
    w = 0
    while w < 4 and x % (2 << w) == 0:
        w += 1
    return w


def tile_rule(case: SCase, direction):
    """Per entry (tile_bytes, pipe) as build_tiles decides: long rows take tile_bytes (unpack:
    unpack_tile_bytes when set) and are pipelined when that is above 8 KiB; short rows take whole
    rows, small_tile_rows of them or, by default, 512 doubled while the field's short rows make
    more than 256 tiles (128 for 16-B rows, 1024 for pack rows of several vectors), at most
    4096."""
    out = []
    utb = knob(case, "unpack_tile_bytes")
    for e in case.ents:
        row, _, rows = e.case.expect[:3]
        if row >= knob(case, "small_row_bytes"):
            out.append((utb if direction == 1 and utb else knob(case, "tile_bytes"),
                        int(direction == 1 and utb > 8192)))
            continue
        r = knob(case, "small_tile_rows")
        if not r:
            multi = row > 16 or row & (row - 1)
            want = rows // (1024 if direction == 0 and multi else 128 if row == 16 else 256)
            r = 512
            while r < 4096 and 2 * r <= want:
                r *= 2
        tb = max(row, min(r * row, 1 << 20))
        out.append((tb - tb % row, 0))
    return out


def planner_facts(s):
    """A segment as the table states it: addressing_cases.seg_facts + (tile_bytes, pipe)."""
    return A.seg_facts(s) + (s.tile_bytes, s.pipe)


def expected_facts(case: SCase, direction):
    """Per segment in plan order (an entry's boxes in order): the table's facts, the rows shared
    out over the entry's boxes."""
    out = []
    for e, t in zip(case.ents, tile_rule(case, direction)):
        row, n_outer, rows, wlog2, amode = e.case.expect
        total = sum(e.parts)
        for part in e.parts:
            out.append((row, n_outer, rows * part // total, wlog2, amode) + t)
    return out


def segment_entries(case: SCase):
    """Per segment in plan order: (index of its entry, byte offset of its box in the entry's
    message)."""
    out = []
    for k, e in enumerate(case.ents):
        total, done = sum(e.parts), 0
        for part in e.parts:
            out.append((k, e.case.nbytes * done // total))
            done += part
    return out


# ---------------------------------------------------------------------------------------------
# plans through the C ABI
# ---------------------------------------------------------------------------------------------
def entries(case: SCase):
    """The case's ghx_pack_entry array, entry k on field slot k; returns (array, keep-alive)."""
    from ghex_amd import _ghx
    ents, keep = [], []
    for k, e in enumerate(case.ents):
        pe, arr = A.entry(A.field_desc(e.case), e.boxes, k, e.buffer_slot, e.buffer_offset)
        ents.append(pe)
        keep.append(arr)
    return (_ghx.PackEntry * len(ents))(*ents), keep


_TUNED = []  # the knob sets of the open `tuned` blocks, innermost last


def _apply(knobs):
    from ghex_amd import _ghx
    _ghx.call("ghx_tune", b"reset", 0)
    for k, v in knobs.items():
        _ghx.call("ghx_tune", k.encode(), int(v))


def knobs_in_force():
    """The knob set last sent to ghx_tune through `tuned` ({}: the defaults)."""
    return dict(_TUNED[-1]) if _TUNED else {}


class tuned:
    """Exactly the given knobs (every other at its default) for the duration of a with block.
    Blocks nest: an inner block replaces the outer one's knobs, and leaving it puts the outer
    block's back, so a plan created as a side effect inside a block (the cached segments() and
    layout()) neither inherits nor loses the caller's knobs."""

    def __init__(self, knobs):
        self.knobs = dict(knobs)

    def __enter__(self):
        _TUNED.append(self.knobs)
        try:
            _apply(self.knobs)
        except Exception:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        assert _TUNED and _TUNED[-1] is self.knobs, "tuned blocks closed out of order"
        _TUNED.pop()
        _apply(knobs_in_force())

    def in_force(self):
        return bool(_TUNED) and _TUNED[-1] is self.knobs


class SPlan:
    """A ghx_plan of a case (pack 0 / unpack 1) created under the case's knobs, which stay set
    while the plan lives (grid_cap is read at launch); destroyed, and the knobs reset, on exit."""

    def __init__(self, case: SCase, direction):
        from ghex_amd import _ghx
        self._ents, self._keep = entries(case)
        self._tuned = tuned(case.knobs)
        self.h = ctypes.c_void_p()
        self._tuned.__enter__()
        try:
            _ghx.call("ghx_plan_create", self._ents, len(case.ents), direction,
                      ctypes.byref(self.h))
        except Exception:
            self._tuned.__exit__()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        from ghex_amd import _ghx
        _ghx.lib().ghx_plan_destroy(self.h)
        self.h = None
        self._tuned.__exit__()

    segments = A.Plan.segments

    def knobs_in_force(self):
        """The case's knobs are the ones set right now (asked right before a launch: grid_cap is
        read there)."""
        return self._tuned.in_force()

    def n_tiles(self):
        from ghex_amd import _ghx
        n = ctypes.c_int32()
        _ghx.call("ghx_plan_info", self.h, None, None, ctypes.byref(n))
        return n.value


@functools.lru_cache(maxsize=None)
def segments(case: SCase, direction):
    """The planner's records of a case (cached; read-only use)."""
    with SPlan(case, direction) as p:
        return tuple(p.segments())


def assert_planned(case: SCase, segs, direction):
    """One segment per box in plan order, each as the table and tile_rule say, on its entry's
    slots, its buf_off advanced by the boxes before it in the entry."""
    where = segment_entries(case)
    assert len(segs) == len(where)
    for i, (s, (k, done), want) in enumerate(zip(segs, where, expected_facts(case, direction))):
        e = case.ents[k]
        assert planner_facts(s) == want, (case.name, i, planner_facts(s), want)
        assert (s.field_slot, s.buffer_slot) == (k, e.buffer_slot)
        assert s.buf_off == e.buffer_offset + done
    for k, e in enumerate(case.ents):
        assert sum(s.bytes for s in segs if s.field_slot == k) == e.case.nbytes


# ---------------------------------------------------------------------------------------------
# the form a launch takes (restated from k_copy, copy_any, self_pair_tile and put_pair_tile)
# ---------------------------------------------------------------------------------------------
def launch_form(seg, field_ptr, buf_ptr, direction):
    """(routine, W, AM) of a k_copy tile of `seg`: the planned width narrowed by the field
    pointer and by the buffer pointer + buf_off; the pipelined unpack (general offsets) when the
    segment is flagged and the width stayed 16 B; the one-division short form at 4, 8 and 16 B,
    the two-division one at 16 B only; the general int64 form otherwise."""
    w = min(seg.wlog2, _wlog2(field_ptr), _wlog2(buf_ptr + seg.buf_off))
    if direction == 1 and seg.pipe and w == 4:
        return ("pipelined", 16, 0)
    if seg.amode == 1 and w >= 2:
        return ("tile", 1 << w, 1)
    if seg.amode == 2 and w == 4:
        return ("tile", 16, 2)
    return ("tile", 1 << w, 0)


def self_form(s, q, field_p, field_u, buf_ptr):
    """self_pair_tile on pack segment s and unpack segment q: ("pack_only", W, AM) for a peer
    message (q.bytes == 0), ("forward", W, AM) when both halves take the same width (AM 1 only at
    8 and 16 B with both segments on the one-division form), else ("split", (Wp, Wu), (pack
    form, unpack form)) through the workgroup barrier."""
    wp = min(s.wlog2, _wlog2(field_p), _wlog2(buf_ptr + s.buf_off))
    wu = min(q.wlog2, _wlog2(field_u), _wlog2(buf_ptr + s.buf_off))
    if q.bytes == 0:
        return ("pack_only",) + launch_form(s, field_p, buf_ptr, 0)[1:]
    if wp == wu:
        return ("forward", 1 << wp, int(s.amode == 1 and q.amode == 1 and wp >= 3))
    return ("split", (1 << wp, 1 << wu),
            (launch_form(s, field_p, buf_ptr, 0), launch_form(q, field_u, buf_ptr + s.buf_off
                                                              - q.buf_off, 1)))


def put_form(s, q, src_ptr, dst_ptr):
    """put_pair_tile: ("direct", W, AM), the width both segments and both pointers allow, the
    short form at 8 and 16 B when both segments plan the one-division form."""
    w = min(s.wlog2, q.wlog2, _wlog2(src_ptr), _wlog2(dst_ptr))
    return ("direct", 1 << w, int(s.amode == 1 and q.amode == 1 and w >= 3))


def tile_walk(seg, W, routine="tile"):
    """[(bytes, trips, the last trip is partial, the tile starts inside a row)] per tile of a
    segment: copy_tile / self_forward / copy_direct move KU * BLOCK * W bytes per loop trip, the
    pipelined unpack PIPE_STEP bytes per step."""
    per = PIPE_STEP if routine == "pipelined" else KU * BLOCK * W
    out = []
    for a in range(0, seg.bytes, seg.tile_bytes):
        nb = min(seg.tile_bytes, seg.bytes - a)
        out.append((nb, -(-nb // per), nb % per != 0, a % seg.row_bytes != 0))
    return out


def walk_model(seg, W, routine="tile"):
    """The buffer positions of every vector the routine moves over the segment's tiles (numpy):
    lane t of a tile [start, end) takes start + t * W + u * BLOCK * W + trip * per for u < KU (2
    when pipelined) while below end. Asserts that tiles are whole vectors."""
    nu = 2 if routine == "pipelined" else KU
    per = nu * BLOCK * W
    lane = np.arange(BLOCK * nu, dtype=np.int64) * W
    pos = []
    for start in range(0, seg.bytes, seg.tile_bytes):
        end = min(start + seg.tile_bytes, seg.bytes)
        assert start % W == 0 and (end - start) % W == 0
        p = (start + lane)[None, :] + (np.arange(-(-(end - start) // per), dtype=np.int64)
                                       * per)[:, None]
        pos.append(p[p < end])
    return np.concatenate(pos)


# ---------------------------------------------------------------------------------------------
# reference offsets, and those of the forms a segment must NOT take
# ---------------------------------------------------------------------------------------------
def other_form_row_offsets(seg):
    """{form: byte offset (from the field pointer) of every row} by the short forms with one and
    with two divisions, applied to this segment whatever it planned: what copy_tile<W, 1> and
    copy_tile<W, 2> would address. (Equal to the exact offsets where the segment fits the form.)"""
    return {nd: np.int64(seg.field_off) + A.short_row_offsets(seg, nd) for nd in (1, 2)}


def exact_row_offsets(seg):
    return np.int64(seg.field_off) + A.exact_row_offsets(seg)


@dataclass
class Region:
    ptr: int               # the field pointer's byte offset in the arena
    span: Tuple[int, int]  # (first, last + 1) arena byte of the region, guards included


def place_field(pos, offsets, row_offsets, row_bytes, shift):
    """A field region from arena byte `pos`: GUARD bytes, then the lowest byte that the element
    offsets or any of the row offset sets reach, ..., the highest, GUARD bytes; the pointer
    congruent to `shift` mod 256. Returns (Region, next pos)."""
    lo = min([int(offsets.min())] + [int(r.min()) for r in row_offsets])
    hi = max([int(offsets.max()) + row_bytes] + [int(r.max()) + row_bytes for r in row_offsets])
    p = pos + GUARD - lo
    p += (shift - p) % 256
    end = (p + hi + GUARD + 255) // 256 * 256
    return Region(p, (pos, end)), end


@dataclass
class Layout:
    arena_bytes: int
    fields: list           # per entry: Region
    buffers_bytes: int
    buf_ptr: list          # per buffer slot: the buffer pointer's offset in the buffer allocation
    msg: list              # per entry: (first, last + 1) byte of its message in that allocation


def case_offsets(e: Ent):
    return A.case_offsets(e.case)


@functools.lru_cache(maxsize=None)
def layout(case: SCase) -> Layout:
    """Fields back to back in one zero-filled allocation (its base 256-B aligned), each between
    guard bands that also hold the addresses of both short forms applied to its segment. Buffers
    likewise in a second allocation, slot by slot: GUARD bytes, the pointer (+ bshift), the
    entries' messages at their buffer offsets with at least PAD bytes between them, GUARD bytes."""
    segs = segments(case, 0)
    fields, pos = [], 0
    for k, e in enumerate(case.ents):
        mine = [s for s in segs if s.field_slot == k]
        wrong = [r for s in mine for r in other_form_row_offsets(s).values()]
        reg, pos = place_field(pos, case_offsets(e), wrong, mine[0].row_bytes, e.fshift)
        fields.append(reg)
    nslots = max(e.buffer_slot for e in case.ents) + 1
    assert len(case.bshift) == nslots
    bptr, msg, bpos = [], [None] * len(case.ents), 0
    for b in range(nslots):
        p = bpos + GUARD + case.bshift[b]
        bptr.append(p)
        end = p
        for k, e in enumerate(case.ents):
            if e.buffer_slot == b:
                msg[k] = (p + e.buffer_offset, p + e.buffer_offset + e.case.nbytes)
                end = max(end, msg[k][1])
        bpos = (end + GUARD + 255) // 256 * 256
    return Layout(pos, fields, bpos, bptr, msg)


def arena_indices(case: SCase):
    """Per entry: the arena byte index of every message byte in buffer order (int64)."""
    lay = layout(case)
    return [A.word_indices(case_offsets(e), e.case.elem, 1, reg.ptr)
            for e, reg in zip(case.ents, lay.fields)]


def expected_forms(case: SCase, direction, field_base=0, buffer_base=0):
    """Per segment the (routine, W, AM) its k_copy launch must take, the allocations' base
    addresses given (any multiple of 256 gives the same answer)."""
    lay = layout(case)
    return [launch_form(s, field_base + lay.fields[s.field_slot].ptr,
                        buffer_base + lay.buf_ptr[s.buffer_slot], direction)
            for s in segments(case, direction)]


# ---------------------------------------------------------------------------------------------
# puts: a source and a target case of the same rows behind different strides and shifts
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Put:
    name: str
    src: A.Case
    dst: A.Case
    sshift: int
    dshift: int
    form: Tuple            # ("direct", W, AM)
    knobs: Tuple[Tuple[str, int], ...] = ()


def _retarget(shp, strides, amode=None):
    elem, layout_, _, ext, expect = SHAPES[shp]
    return A.Case(shp + "'", elem, layout_, strides, ext,
                  expect[:4] + (expect[4] if amode is None else amode,))


def _puts():
    g = (("fast_addr", 0),)
    t16 = _retarget("long16", (8, 432, 13824))
    t16g = _retarget("long16", (8, 432, 13824), 0)
    ts = _retarget("short16", (8, 48, 2400))
    tsg = _retarget("short16", (8, 48, 2400), 0)
    t4 = _retarget("long4", (4, 96, 3840))
    s16, s16g = shape("long16"), shape("long16", amode=0)
    ss, ssg = shape("short16"), shape("short16", amode=0)
    return [
        # 84,000 B of 400-B rows: 11 tiles, the last one partial
        Put("long16", s16, t16, 0, 0, ("direct", 16, 1)),
        Put("long16_d8", s16, t16, 16, 8, ("direct", 8, 1)),
        Put("long16_s8", s16, t16, 8, 32, ("direct", 8, 1)),
        Put("long16_d4", s16, t16, 0, 4, ("direct", 4, 0)),
        Put("long16_s2", s16, t16, 2, 8, ("direct", 2, 0)),
        Put("long16_s1", s16, t16, 1, 2, ("direct", 1, 0)),
        Put("long16_g", s16g, t16g, 0, 0, ("direct", 16, 0), g),
        Put("long16_g_d8", s16g, t16g, 0, 8, ("direct", 8, 0), g),
        # 3000 rows of 16 B: tiles of whole rows
        Put("short16", ss, ts, 0, 0, ("direct", 16, 1)),
        Put("short16_s8", ss, ts, 8, 0, ("direct", 8, 1)),
        Put("short16_d4", ss, ts, 16, 4, ("direct", 4, 0)),
        Put("short16_d2", ss, ts, 0, 2, ("direct", 2, 0)),
        Put("short16_d1", ss, ts, 4, 1, ("direct", 1, 0)),
        Put("short16_g", ssg, tsg, 0, 0, ("direct", 16, 0), g),
        Put("short16_g_s8", ssg, tsg, 8, 0, ("direct", 8, 0), g),
        # 4-B elements: the planned width is 4
        Put("long4", shape("long4"), t4, 0, 8, ("direct", 4, 0)),
    ]


PUTS = {p.name: p for p in _puts()}
PUT_GRID_CASES = ("long16", "long16_s1", "long16_g_d8")


def _single(c: A.Case, knobs):
    return SCase(c.name, (Ent(c),), (0,), tuple(knobs))


@functools.lru_cache(maxsize=None)
def put_segments(put: Put):
    """(source pack segment, target unpack segment) as the put's two plans hold them."""
    (s,) = segments(_single(put.src, put.knobs), 0)
    (q,) = segments(_single(put.dst, put.knobs), 1)
    return s, q


@functools.lru_cache(maxsize=None)
def put_layout(put: Put):
    """Source and target regions, disjoint, in one arena: (arena bytes, source Region, target
    Region), each holding the addresses of both short forms on its segment as well."""
    s, q = put_segments(put)
    src, pos = place_field(0, A.case_offsets(put.src), list(other_form_row_offsets(s).values()),
                           s.row_bytes, put.sshift)
    dst, pos = place_field(pos, A.case_offsets(put.dst), list(other_form_row_offsets(q).values()),
                           q.row_bytes, put.dshift)
    return pos, src, dst


def put_entries(put: Put):
    """((source entry, keep), (target entry, keep)) of ghx_put_create."""
    return A.case_entry(put.src), A.case_entry(put.dst)


# ---------------------------------------------------------------------------------------------
# fused self exchange: one periodic domain behind the strides of a padded view
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class SelfCase:
    name: str
    dtype: str             # torch / numpy dtype name
    N: Tuple[int, int, int]       # interior cells
    halo: Tuple[int, int, int]    # halo width per dim (both sides)
    ext: Tuple[int, int, int]     # allocated cells per dim (>= N + 2 * halo: padded rows)
    shift: int = 0         # storage offset of the view, in elements
    knobs: Tuple[Tuple[str, int], ...] = ()

    @property
    def elem(self):
        return np.dtype(self.dtype).itemsize

    @property
    def shape(self):
        return tuple(n + 2 * h for n, h in zip(self.N, self.halo))

    @property
    def strides(self):
        """Element strides of the (x, y, z) view."""
        return (1, self.ext[0], self.ext[0] * self.ext[1])

    @property
    def halos6(self):
        return tuple(h for h in self.halo for _ in range(2))


SELF_CASES = {c.name: c for c in [
    # halo 1 everywhere, rows padded to 16 cells: x faces of one element per row, y and z faces of
    # rows of 6 elements; every pair forwards at the width of the element
    SelfCase("uint8", "uint8", (6, 5, 4), (1, 1, 1), (16, 8, 6)),
    SelfCase("int16", "int16", (6, 5, 4), (1, 1, 1), (16, 8, 6)),
    SelfCase("float32", "float32", (6, 5, 4), (1, 1, 1), (16, 8, 6)),
    SelfCase("float64", "float64", (6, 5, 4), (1, 1, 1), (16, 8, 6)),
    SelfCase("complex128", "complex128", (6, 5, 4), (1, 1, 1), (16, 8, 6)),
    # the view starts one element into the storage: fp64 rows of 16 B narrowed to 8-B vectors
    SelfCase("float64_h2_shift1", "float64", (6, 5, 4), (2, 1, 1), (16, 8, 6), shift=1),
    # float32, halo 4 in x, 6 interior cells in rows of 16: the left send face starts 16 B into a
    # row (16-B vectors), the right halo 40 B in (8-B vectors): pack, barrier, unpack
    SelfCase("split", "float32", (6, 40, 30), (4, 1, 1), (16, 42, 32)),
    # the same in small tiles under five workgroups: a workgroup takes split tiles after forward
    # tiles (the barrier pair inside a grid-stride loop). Every row here is short, so the tiles
    # are cut by small_tile_rows; self_tile_bytes makes the exchange build its own self plans;
    # order 0 dispatches the tiles in segment order, so self_workgroup_walks can tell who takes what
    SelfCase("split_walk", "float32", (6, 40, 30), (4, 1, 1), (16, 42, 32),
             knobs=(("grid_cap", 5), ("order", 0), ("self_tile_bytes", 1024),
                    ("small_tile_rows", 64))),
    # the general self_forward at 8 and 16 B
    SelfCase("float64_g", "float64", (6, 5, 4), (1, 1, 1), (16, 8, 6), knobs=(("fast_addr", 0),)),
    SelfCase("complex128_g", "complex128", (6, 5, 4), (1, 1, 1), (16, 8, 6),
             knobs=(("fast_addr", 0),)),
]}
SELF_DTYPES = ("uint8", "int16", "float32", "float64", "complex128")


def self_field_desc(c: SelfCase):
    """The field descriptor make_field_descriptor derives from the case's view (3-D, x fastest,
    offsets = the halo)."""
    e = c.elem
    return A.field_desc(A.Case(c.name, e, L3, tuple(s * e for s in c.strides), c.shape, None,
                               offsets=c.halo))


def self_pairs(desc, pattern):
    """[(pack segment, unpack segment)] of a single-domain self exchange of one field: twin
    plans over the pattern's send and receive boxes, which share ONE buffer in key order, as the
    exchange lays them out. Created under the knobs in force, with tile_bytes = self_tile_bytes
    where the caller set both alike."""
    out = []
    for direction, halos in ((0, pattern.send_halos(0)), (1, pattern.recv_halos(0))):
        assert len(halos) == 1  # one key: every message goes to this domain itself
        boxes = [(sp[0], sp[1]) for _, _, _, spaces in halos for sp in spaces]
        with A.Plan(A.entry(desc, boxes), direction) as p:
            segs = p.segments()
        assert len(segs) == len(boxes)
        out.append(segs)
    for s, q in zip(*out):
        assert (s.buf_off, s.bytes, s.row_bytes) == (q.buf_off, q.bytes, q.row_bytes)
    return list(zip(*out))


def self_forms(pairs, field_ptr, buf_ptr):
    return [self_form(s, q, field_ptr, field_ptr, buf_ptr) for s, q in pairs]


def self_pattern(c: SelfCase, ctx):
    """(domain descriptor, pattern container) of the case's one periodic domain."""
    from ghex_amd.structured import regular as R
    gf, gl = (0, 0, 0), tuple(n - 1 for n in c.N)
    dd = R.DomainDescriptor(0, gf, gl)
    return dd, R.make_pattern(ctx, R.HaloGenerator(gf, gl, c.halos6, (True,) * 3), [dd])


def self_twin_knobs(c: SelfCase):
    """The knobs the twin plans of self_pairs are created under: the case's, with the fused
    exchange's tile (self_tile_bytes) as the plans' tile_bytes."""
    kn = {k: v for k, v in c.knobs if k != "grid_cap"}
    if "self_tile_bytes" in kn:
        kn["tile_bytes"] = kn["self_tile_bytes"]
    return kn


def self_workgroup_walks(pairs, forms, grid):
    """Per workgroup of a k_self launch of `grid` groups the kinds ("forward" / "split") of the
    tiles it takes, in order, when tiles are dispatched in segment order (knob order = 0):
    workgroup b takes tiles b, b + grid, ..."""
    kinds = [f[0] for (s, _), f in zip(pairs, forms) for _ in tile_walk(s, 1)]
    return [kinds[b::grid] for b in range(min(grid, len(kinds)))]
