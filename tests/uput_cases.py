"""Shared set-up of the index-list put tests (ghx_uput_create, k_put_u): entry arrays from plain
descriptions, the planner's segments read back through ghx_uput_segment, and the NumPy form of
the put's definition — for every i < n_lids and l < levels

    dst.values[(t[i]*dst.index_stride + l*dst.level_stride)*elem] <-
    src.values[(s[i]*src.index_stride + l*src.level_stride)*elem]

Works without a device (the plans can be described, not executed)."""
from __future__ import annotations

import ctypes

import numpy as np

N_CELLS = 10007                 # tests/unstructured_cases.py's sizes: several 512-row tiles,
LIST_SIZES = (3001, 3002, 3003)  # the last one partial


def udesc(elem, levels=1, first=True, index_stride=None, level_stride=None, n_cells=N_CELLS):
    """A ghx_udata_desc; the strides default to the dense ones of data_descriptor's constructor
    (levels first: index stride = levels, level stride 1; levels last: 1 and the cell count)."""
    from ghex_amd import _ghx
    d = _ghx.UDataDesc()
    d.elem_size, d.levels, d.levels_first = elem, levels, 1 if first else 0
    d.index_stride = index_stride if index_stride is not None else (levels if first else 1)
    d.level_stride = level_stride if level_stride is not None else (1 if first else n_cells)
    return d


def span_bytes(d, n_cells=N_CELLS):
    """Bytes from a field's first byte to the end of its last addressable element."""
    return ((n_cells - 1) * abs(d.index_stride) + (d.levels - 1) * abs(d.level_stride) + 1) * d.elem_size


class Side:
    """One end of a message: descriptor, field slot, index list (kept alive as int64)."""

    def __init__(self, desc, slot, lids):
        self.desc, self.slot = desc, slot
        self.lids = np.ascontiguousarray(lids, dtype=np.int64)


def entries(sides):
    from ghex_amd import _ghx
    arr = (_ghx.UPutEntry * max(1, len(sides)))()
    for e, s in zip(arr, sides):
        e.data, e.field_slot = s.desc, s.slot
        e.lids, e.n_lids = _ghx.i64_ptr(s.lids), s.lids.size
    return arr


def try_create(srcs, dsts):
    """(return code, last error, handle) of ghx_uput_create over two lists of Side."""
    from ghex_amd import _ghx
    L = _ghx.lib()
    h = ctypes.c_void_p()
    rc = L.ghx_uput_create(entries(srcs), entries(dsts), len(srcs), ctypes.byref(h))
    return rc, (L.ghx_last_error() or b"").decode(), h


def create(srcs, dsts):
    rc, why, h = try_create(srcs, dsts)
    assert rc == 0, why
    return h


def destroy(h):
    from ghex_amd import _ghx
    assert _ghx.lib().ghx_put_destroy(h) == 0


def segments(h):
    from ghex_amd import _ghx
    L = _ghx.lib()
    first = _ghx.UPutSegmentInfo()
    if L.ghx_uput_segment(h, 0, ctypes.byref(first)) != 0:
        return []  # an empty plan: index 0 is out of range
    out = [first]
    for k in range(1, first.n_segments):
        s = _ghx.UPutSegmentInfo()
        _ghx.call("ghx_uput_segment", h, k, ctypes.byref(s))
        out.append(s)
    return out


def put_info(h):
    from ghex_amd import _ghx
    b, t = ctypes.c_uint64(), ctypes.c_int32()
    _ghx.call("ghx_put_info", h, ctypes.byref(b), ctypes.byref(t))
    return b.value, t.value


def formula_pairs(src, dst):
    """The definition's element enumeration of one message: (source, target) byte offsets of
    every (i, l), as an (n*levels, 2) int64 array."""
    sd, dd = src.desc, dst.desc
    lv = np.arange(sd.levels, dtype=np.int64)[None, :]
    so = (src.lids[:, None] * sd.index_stride + lv * sd.level_stride) * sd.elem_size
    to = (dst.lids[:, None] * dd.index_stride + lv * dd.level_stride) * dd.elem_size
    return np.stack([so.reshape(-1), to.reshape(-1)], axis=1)


def segment_pairs(seg, src, dst, step):
    """The record's addressing decoded over the segment's message positions 0, step, 2*step, ...
    (step divides the row): (source, target) byte offsets, as the kernel computes them."""
    p = np.arange(0, seg.bytes, step, dtype=np.int64)
    row, rem = p // seg.row_bytes, p % seg.row_bytes
    if seg.mode == 0:
        i, lev = row, np.zeros_like(row)
    elif seg.mode == 1:
        levels = seg.bytes // seg.row_bytes // seg.n
        i, lev = row // levels, row % levels
    else:
        lev, i = row // seg.n, row % seg.n
    assert i.size == 0 or (i.max() < seg.n and i.min() >= 0)  # no table read at or beyond n
    sl = src.lids[seg.first_index:seg.first_index + seg.n][i]
    tl = dst.lids[seg.first_index:seg.first_index + seg.n][i]
    so = seg.src_field_off + sl * seg.src_index_stride_b + lev * seg.src_level_stride_b + rem
    to = seg.dst_field_off + tl * seg.dst_index_stride_b + lev * seg.dst_level_stride_b + rem
    return np.stack([so, to], axis=1)


def sorted_rows(a):
    return a[np.lexsort((a[:, 1], a[:, 0]))]


def apply_put(src_bytes, dst_bytes, src, dst):
    """The definition on host byte arrays (each starting at its field's first byte): dst_bytes
    is changed in place."""
    pairs = formula_pairs(src, dst)
    for b in range(src.desc.elem_size):
        dst_bytes[pairs[:, 1] + b] = src_bytes[pairs[:, 0] + b]


def draw_lists(rng, sizes=LIST_SIZES, n_cells=N_CELLS):
    """Index lists drawn without repetition, disjoint from one another (target lists of one field
    are distinct)."""
    perm = rng.permutation(n_cells)
    out, at = [], 0
    for n in sizes:
        out.append(perm[at:at + n].astype(np.int64))
        at += n
    return out
