"""Shared set-up of the fused index-list self exchange tests (ghx_uself_create, k_self_u): pack /
unpack entry arrays from the put tests' plain descriptions (tests/uput_cases.py) plus each
message's place in a buffer, the planner's segments read back through ghx_uself_segment, and the
NumPy form of the packed message — message element (i, l) of a list of n indices and L levels
sits at buffer_offset + (i*L + l)*elem for levels first and buffer_offset + (i + l*n)*elem for
levels last, the layout of the reference's unstructured pack.

Works without a device (the plans can be described, not executed)."""
from __future__ import annotations

import ctypes

import numpy as np


def entries(sides, places):
    """ghx_upack_entry array of one direction: sides[k] with its (buffer slot, buffer offset)."""
    from ghex_amd import _ghx
    arr = (_ghx.UPackEntry * max(1, len(sides)))()
    for e, s, (slot, off) in zip(arr, sides, places):
        e.data, e.field_slot = s.desc, s.slot
        e.buffer_slot, e.buffer_offset = slot, off
        e.lids, e.n_lids = _ghx.i64_ptr(s.lids), s.lids.size
    return arr


def try_create(srcs, dsts, places, dst_places=None):
    """(return code, last error, handle) of ghx_uself_create over two lists of Side and the
    messages' places (dst_places: the unpack entries' own, default the same)."""
    from ghex_amd import _ghx
    L = _ghx.lib()
    h = ctypes.c_void_p()
    rc = L.ghx_uself_create(entries(srcs, places), entries(dsts, dst_places or places), len(srcs),
                            ctypes.byref(h))
    return rc, (L.ghx_last_error() or b"").decode(), h


def create(srcs, dsts, places):
    rc, why, h = try_create(srcs, dsts, places)
    assert rc == 0, why
    return h


def destroy(h):
    from ghex_amd import _ghx
    assert _ghx.lib().ghx_uself_destroy(h) == 0


def info(h):
    """(message bytes, segments, tiles)"""
    from ghex_amd import _ghx
    b, s, t = ctypes.c_uint64(), ctypes.c_int32(), ctypes.c_int32()
    _ghx.call("ghx_uself_info", h, ctypes.byref(b), ctypes.byref(s), ctypes.byref(t))
    return b.value, s.value, t.value


def segments(h):
    from ghex_amd import _ghx
    out = []
    for k in range(info(h)[1]):
        s = _ghx.USelfSegmentInfo()
        _ghx.call("ghx_uself_segment", h, k, ctypes.byref(s))
        out.append(s)
    return out


def message_bytes(side):
    return side.lids.size * side.desc.levels * side.desc.elem_size


def packed(src_bytes, side, buffer_offset, out):
    """The packed message of `side` (a source Side; src_bytes starts at its field's first byte)
    written into the host buffer image `out` at buffer_offset: buf[i*L + l] for levels first,
    buf[i + l*n] for levels last."""
    d, n = side.desc, side.lids.size
    lv = np.arange(d.levels, dtype=np.int64)[None, :]
    so = (side.lids[:, None] * d.index_stride + lv * d.level_stride) * d.elem_size   # (n, L)
    i = np.arange(n, dtype=np.int64)[:, None]
    pos = (i * d.levels + lv) if d.levels_first else (i + lv * n)
    bo = buffer_offset + pos * d.elem_size
    for b in range(d.elem_size):
        out[bo.reshape(-1) + b] = src_bytes[so.reshape(-1) + b]
    return out
