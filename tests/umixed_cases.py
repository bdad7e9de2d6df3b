"""Shared set-up of the index-list mixed pack tests (ghx_umixed_create, k_pack_self_u): a plan
from plain descriptions (tests/uput_cases.py's Side, tests/uself_cases.py's entry arrays) of the
self messages and of the peer messages, its counts, and its two kinds of segments read back —
the self segments through ghx_uself_segment, the peer segments through ghx_umixed_peer_segment —
next to the pack plan a ghx_uplan makes of the same peer entries.

Works without a device (the plans can be described, not executed)."""
from __future__ import annotations

import ctypes

from tests import uself_cases as US

USEG_FIELDS = ("field_off", "buf_off", "index_stride_b", "level_stride_b", "bytes", "row_bytes",
               "tile_bytes", "n", "field_slot", "buffer_slot", "mode", "wlog2", "lid64", "runs", "fpol")


def try_create(srcs, dsts, places, peers, peer_places, dst_places=None):
    """(return code, last error, handle) of ghx_umixed_create: self messages srcs[k] -> dsts[k] at
    places[k] = (buffer slot, buffer offset), peer messages peers[j] at peer_places[j]."""
    from ghex_amd import _ghx
    L = _ghx.lib()
    h = ctypes.c_void_p()
    rc = L.ghx_umixed_create(US.entries(srcs, places), US.entries(dsts, dst_places or places), len(srcs),
                             US.entries(peers, peer_places), len(peers), ctypes.byref(h))
    return rc, (L.ghx_last_error() or b"").decode(), h


def create(srcs, dsts, places, peers, peer_places):
    rc, why, h = try_create(srcs, dsts, places, peers, peer_places)
    assert rc == 0, why
    return h


def mixed_info(h):
    """(self tiles, peer segments, peer tiles)"""
    from ghex_amd import _ghx
    a, b, c = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    _ghx.call("ghx_umixed_info", h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return a.value, b.value, c.value


def self_segments(h):
    from ghex_amd import _ghx
    out = []
    for k in range(US.info(h)[1] - mixed_info(h)[1]):
        s = _ghx.USelfSegmentInfo()
        _ghx.call("ghx_uself_segment", h, k, ctypes.byref(s))
        out.append(s)
    return out


def peer_segments(h):
    from ghex_amd import _ghx
    out = []
    for k in range(mixed_info(h)[1]):
        s = _ghx.USegmentInfo()
        _ghx.call("ghx_umixed_peer_segment", h, k, ctypes.byref(s))
        out.append(s)
    return out


class PackPlan:
    """A ghx_uplan over entries (sides with their places), direction 0 (pack) or 1 (unpack)."""

    def __init__(self, sides, places, direction=0):
        from ghex_amd import _ghx
        self._keep = US.entries(sides, places)
        self.h = ctypes.c_void_p()
        _ghx.call("ghx_uplan_create", self._keep, len(sides), direction, ctypes.byref(self.h))

    def info(self):
        from ghex_amd import _ghx
        b, s, t = ctypes.c_uint64(), ctypes.c_int32(), ctypes.c_int32()
        _ghx.call("ghx_uplan_info", self.h, ctypes.byref(b), ctypes.byref(s), ctypes.byref(t))
        return b.value, s.value, t.value

    def segments(self):
        from ghex_amd import _ghx
        out = []
        for k in range(self.info()[1]):
            s = _ghx.USegmentInfo()
            _ghx.call("ghx_uplan_segment", self.h, k, ctypes.byref(s))
            out.append(s)
        return out

    def execute(self, fp, nf, bp, nb, stream):
        from ghex_amd import _ghx
        _ghx.call("ghx_uplan_execute", self.h, fp, nf, bp, nb, stream)

    def destroy(self):
        from ghex_amd import _ghx
        assert _ghx.lib().ghx_uplan_destroy(self.h) == 0
