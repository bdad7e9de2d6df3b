"""Field descriptors at the limits of the short-form field addressing (seg_s::amode, planner
short_addressing, kernel field_offset_f), shared by tests/test_plan_addressing.py (host) and
tests/test_gpu_addressing.py (device): the case table, plan / segment access through the C ABI,
a numpy model of the short form and the element enumerator the device tests use as reference.

A field descriptor carries arbitrary byte strides, so a box of a few rows with a 16-MiB stride
reaches every limit with a message of a few hundred bytes in a sparse allocation."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Tuple

import numpy as np

K = 1 << 24


@dataclass(frozen=True)
class Case:
    name: str
    elem: int
    layout: Tuple[int, ...]        # layout map: the dim with value dim-1 is the fastest
    strides: Tuple[int, ...]       # byte strides per dim
    ext: Tuple[int, ...]           # box extents per dim (the box's first is all zero)
    expect: Tuple[int, int, int, int, int]  # row bytes, n_outer, rows, wlog2, amode
    offsets: Tuple[int, ...] = None  # field offsets (default: 0)

    @property
    def dim(self):
        return len(self.layout)

    @property
    def offs(self):
        return self.offsets if self.offsets is not None else (0,) * self.dim

    @property
    def nbytes(self):
        return int(np.prod(self.ext, dtype=np.int64)) * self.elem

    @property
    def unit_stride(self):
        """The fastest dim is contiguous (else every element is its own row)."""
        return self.strides[self.layout.index(self.dim - 1)] == self.elem


L3 = (2, 1, 0)
CASES = {c.name: c for c in [
    # stride of the middle / the slowest outer dim just below and at 2^24
    Case("A1", 8, L3, (8, K - 16, 64), (4, 3, 2), (32, 2, 6, 4, 1)),
    Case("A2", 8, L3, (8, K, 64), (4, 3, 2), (32, 2, 6, 4, 0)),
    Case("B1", 8, L3, (8, 64, K - 16), (4, 2, 3), (32, 2, 6, 4, 1)),
    Case("B2", 8, L3, (8, 64, K), (4, 2, 3), (32, 2, 6, 4, 0)),
    # three outer dims (strided fastest dim: element rows), each stride in turn at the limit
    Case("C1", 16, L3, (32, 4096, K - 16), (4, 3, 3), (16, 3, 36, 4, 2)),
    Case("C2", 16, L3, (32, 4096, K), (4, 3, 3), (16, 3, 36, 4, 0)),
    Case("C3", 16, L3, (32, K - 16, 4096), (4, 3, 3), (16, 3, 36, 4, 2)),
    Case("C4", 16, L3, (K - 16, 4096, 256), (3, 3, 3), (16, 3, 27, 4, 2)),
    # rows: 2^24 - 1 and 2^24
    Case("D1", 8, (1, 0), (16, 65536), (4095, 4097), (8, 2, K - 1, 3, 1)),
    Case("D2", 8, (1, 0), (16, 65536), (4096, 4096), (8, 2, K, 3, 0)),
    # D2's largest row index still fits 24 bits (the rule is conservative by one row); D3's not
    Case("D3", 8, (1, 0), (16, 65536), (4096, 4097), (8, 2, K + 4096, 3, 0)),
    # row length (E2 cannot separate it from the stride limit; with row length 2^24 and stride
    # 2^24 + 8 the two truncations happen to cancel, so only E2's amode is asserted)
    Case("E1", 8, (1, 0), (8, K - 8), ((1 << 21) - 2, 3), (K - 16, 1, 3, 3, 1)),
    Case("E2", 8, (1, 0), (8, K + 8), (1 << 21, 3), (K, 1, 3, 3, 0)),
    # span: 2^32 - 16, exactly 2^32 (conservative: its largest offset still fits), beyond
    Case("F1", 8, L3, (8, 3824, 16711920), (2, 2, 258), (16, 2, 516, 4, 1)),
    Case("F2", 8, L3, (8, 3840, 16711920), (2, 2, 258), (16, 2, 516, 4, 0)),
    Case("F3", 8, L3, (8, 3840, 16711920), (2, 2, 270), (16, 2, 540, 4, 0)),
    # a negative stride
    Case("G", 8, L3, (8, -256, 8192), (4, 3, 3), (32, 2, 9, 4, 0)),
    # a short-form segment whose field_off is beyond 2^32 (the form is relative to it)
    Case("H", 8, L3, (8, 3824, 16711920), (2, 2, 3), (16, 2, 6, 4, 1), offsets=(0, 2, 257)),
    # 4-byte elements, 12-B rows
    Case("W2", 4, L3, (4, K - 16, 64), (3, 3, 2), (12, 2, 6, 2, 1)),
]}
H_FIELD_OFF = 4294971088

# cases whose whole field fits a host array of 512 MiB (the oracle runs on them)
HOST_SIZED = ("A1", "A2", "B1", "B2", "C1", "C2", "C3", "C4", "D1", "D2", "D3", "E1", "E2", "G", "W2")


def field_desc(case: Case, offsets=None):
    from ghex_amd import _ghx
    d = _ghx.FieldDesc()
    d.dim, d.elem_size = case.dim, case.elem
    offs = case.offs if offsets is None else offsets
    for k in range(case.dim):
        d.layout[k] = case.layout[k]
        d.byte_strides[k] = case.strides[k]
        d.offsets[k] = offs[k]
        d.extents[k] = 0  # unchecked
    d.num_components, d.has_components = 1, 0
    return d


def entry(desc, boxes, field_slot=0, buffer_slot=0, buffer_offset=0):
    """A ghx_pack_entry over `boxes` = [(first, last)]; returns (entry, keep-alive)."""
    from ghex_amd import _ghx
    arr = (_ghx.Box * max(1, len(boxes)))()
    for i, (first, last) in enumerate(boxes):
        for k in range(len(first)):
            arr[i].first[k], arr[i].last[k] = first[k], last[k]
    e = _ghx.PackEntry()
    e.field, e.field_slot, e.buffer_slot, e.buffer_offset = desc, field_slot, buffer_slot, \
        buffer_offset
    e.boxes, e.n_boxes = ctypes.cast(arr, ctypes.POINTER(_ghx.Box)), len(boxes)
    return e, arr


def case_entry(case: Case, offsets=None):
    box = ((0,) * case.dim, tuple(x - 1 for x in case.ext))
    return entry(field_desc(case, offsets), [box])


# More slots than two launches carry (64 each): 130 distinct field and buffer slots are three
# launch groups of 64, 64 and 2, shared by tests/test_plan_addressing.py (host) and
# tests/test_gpu_fuzz.py (device). Entry k: field slot k, buffer slot N_SLOTS - 1 - k.
N_SLOTS = 130
SLOT_BOX = ((2, 1, 0), (3, 2, 1))  # x, y, z: a[0:2, 1:3, 2:4] of a (z, y, x) array
SLOT_BOX_BYTES = 32
U_CELLS, U_LEVELS, U_LIDS = 10, 2, 4


def many_slot_entries():
    """N_SLOTS structured entries, each the 2x2x2 box SLOT_BOX of its own unit-stride 4x4x4 fp32
    field; returns (ghx_pack_entry array, keep-alive)."""
    from ghex_amd import _ghx
    case = Case("S", 4, L3, (4, 16, 64), (4, 4, 4), (8, 2, 4, 3, 1))
    desc = field_desc(case)
    for k in range(3):
        desc.extents[k] = 4
    ents, keep = [], []
    for k in range(N_SLOTS):
        e, arr = entry(desc, [SLOT_BOX], k, N_SLOTS - 1 - k)
        ents.append(e)
        keep.append(arr)
    return (_ghx.PackEntry * N_SLOTS)(*ents), keep


def many_slot_lids():
    """Entry k's U_LIDS distinct cells of U_CELLS, in a seeded random order: (N_SLOTS, U_LIDS)."""
    rng = np.random.default_rng(130)
    return np.stack([rng.permutation(U_CELLS)[:U_LIDS] for _ in range(N_SLOTS)]).astype(np.int64)


def many_slot_uentries(lids):
    """N_SLOTS unstructured entries over many_slot_lids(): fp32 values of U_LEVELS levels,
    levels first (one 8-B row per cell); returns the ghx_upack_entry array (lids kept by caller)."""
    from ghex_amd import _ghx
    ents = []
    for k in range(N_SLOTS):
        e = _ghx.UPackEntry()
        e.data.elem_size, e.data.levels, e.data.levels_first = 4, U_LEVELS, 1
        e.data.index_stride, e.data.level_stride = U_LEVELS, 1
        e.field_slot, e.buffer_slot, e.buffer_offset = k, N_SLOTS - 1 - k, 0
        e.lids, e.n_lids = _ghx.i64_ptr(lids[k]), U_LIDS
        ents.append(e)
    return (_ghx.UPackEntry * N_SLOTS)(*ents)


class Plan:
    """A ghx_plan handle (pack 0 / unpack 1) destroyed on exit."""

    def __init__(self, e, direction):
        from ghex_amd import _ghx
        self._e = e
        self.h = ctypes.c_void_p()
        _ghx.call("ghx_plan_create", ctypes.byref(e[0]), 1, direction, ctypes.byref(self.h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        from ghex_amd import _ghx
        _ghx.lib().ghx_plan_destroy(self.h)
        self.h = None

    def segments(self):
        from ghex_amd import _ghx
        n = ctypes.c_int32()
        _ghx.call("ghx_plan_info", self.h, None, ctypes.byref(n), None)
        out = []
        for k in range(n.value):
            s = _ghx.SegmentInfo()
            _ghx.call("ghx_plan_segment", self.h, k, ctypes.byref(s))
            out.append(s)
        return out


def seg_facts(s):
    return (s.row_bytes, s.n_outer, s.bytes // s.row_bytes, s.wlog2, s.amode)


def amodes(e, direction):
    with Plan(e, direction) as p:
        return [s.amode for s in p.segments()]


# ---------------------------------------------------------------------------------------------
# the two offset arithmetics of a segment, over all of its rows
# ---------------------------------------------------------------------------------------------
def _row_coords(s):
    rows = s.bytes // s.row_bytes
    r = np.arange(rows, dtype=np.int64)
    c = []
    for k in range(3):
        c.append(r % s.ext[k])
        r = r // s.ext[k]
    c.append(r)
    return c


def exact_row_offsets(s):
    """Row offsets relative to field_off, exact (int64): sum_k c_k * stride_k."""
    c = _row_coords(s)
    return sum(c[k] * np.int64(s.stride[k]) for k in range(4))


def umul24(a, b):
    """v_mul_u32_u24: the low 32 bits of the product of the operands' low 24 bits."""
    a = np.asarray(a, dtype=np.uint64) & np.uint64(0xFFFFFF)
    b = np.asarray(b, dtype=np.uint64) & np.uint64(0xFFFFFF)
    return (a * b) & np.uint64(0xFFFFFFFF)


def short_row_offsets(s, ndiv):
    """field_offset_f<ndiv> at the first byte of every row (p = row * row_bytes, 32-bit):
    32-bit sums of 24-bit products, one or two divisions."""
    M = np.uint64(0xFFFFFFFF)
    rows = s.bytes // s.row_bytes
    row = np.arange(rows, dtype=np.uint64)
    p = (row * np.uint64(s.row_bytes)) & M
    st = [np.uint64(s.stride[k] & 0xFFFFFFFF) for k in range(3)]
    off = (p - umul24(row, s.row_bytes)) & M
    q0 = row // np.uint64(s.ext[0])
    off = (off + umul24((row - umul24(q0, s.ext[0])) & M, st[0])) & M
    if ndiv == 1:
        off = (off + umul24(q0, st[1])) & M
    else:
        q1 = q0 // np.uint64(s.ext[1])
        off = (off + umul24((q0 - umul24(q1, s.ext[1])) & M, st[1])) & M
        off = (off + umul24(q1, st[2])) & M
    return off.astype(np.int64)


# ---------------------------------------------------------------------------------------------
# reference: the field byte offset of every message element, in buffer order
# ---------------------------------------------------------------------------------------------
def element_offsets(layout, strides, offsets, boxes):
    """Boxes in order; within a box the dims from slowest to fastest by layout value; the offset
    of cell i is sum_d (first_d + offset_d + i_d) * byte_stride_d. int64."""
    D = len(layout)
    order = sorted(range(D), key=lambda d: layout[d])  # slowest ... fastest
    out = []
    for first, last in boxes:
        off = np.zeros(1, dtype=np.int64)
        for d in order:
            i = np.arange(first[d], last[d] + 1, dtype=np.int64) + np.int64(offsets[d])
            off = (off[:, None] + (i * np.int64(strides[d]))[None, :]).reshape(-1)
        out.append(off)
    return np.concatenate(out)


def case_offsets(case: Case, offsets=None):
    box = ((0,) * case.dim, tuple(x - 1 for x in case.ext))
    return element_offsets(case.layout, case.strides, case.offs if offsets is None else offsets,
                           [box])


def word_indices(off, elem, g, shift=0):
    """Indices into a view of g-byte words of the bytes [o + shift, o + shift + elem) of every
    element offset o (all multiples of g)."""
    assert elem % g == 0 and shift % g == 0 and not np.any(off % g)
    idx = (off + shift) // g
    if elem == g:
        return idx
    return (idx[:, None] + np.arange(elem // g, dtype=np.int64)[None, :]).reshape(-1)


def oracle_gathers_the_enumerated_bytes(case: Case):
    """The project's pinned reference (oracle.structured_pack) on a host array of the case's
    strides packs exactly the bytes the enumerator gathers."""
    from oracle import oracle as orc
    off = case_offsets(case)
    shift = 1024 if off.min() < 0 else 0  # negative strides: the field starts inside the array
    size = int(off.max()) + shift + case.elem
    assert off.min() + shift >= 0 and size <= 512 << 20
    g = min(case.elem, 8)
    host = np.zeros((size + 7) // 8 * 8, dtype=np.uint8)
    rng = np.random.default_rng(11)
    data = rng.integers(1, 256, size=case.nbytes, dtype=np.uint8)
    idx = word_indices(off, case.elem, g, shift)
    host.view(f"u{g}")[idx] = data.view(f"u{g}")
    spec = orc.FieldSpec(host[shift:], case.elem, case.layout, case.offs, (0,) * case.dim,
                         byte_strides=case.strides)
    box = orc.ISPair((0,) * case.dim, tuple(x - 1 for x in case.ext), None, None)
    got = np.zeros(case.nbytes, dtype=np.uint8)
    n = orc.structured_pack(spec, got, [box], elementwise=not case.unit_stride)
    assert n == case.nbytes
    np.testing.assert_array_equal(got, data)
    np.testing.assert_array_equal(host.view(f"u{g}")[idx].view(np.uint8), data)
