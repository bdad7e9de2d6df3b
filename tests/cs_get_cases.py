"""Helpers of the fused cubed-sphere adjoint tests (ghx_cs_exchange_adjoint_self_*, k_accum_get_x):
an exchange of any emulated rank under any placement that keeps its items, the plan's counters, and
the expansion of every source record of the get plan into the halo cells it reads, checked against
the recorded fixture (tests/cs_cases.py, tests/cs_adjoint_cases.py; no transform table lives here)."""
from __future__ import annotations

import ctypes

import numpy as np

from tests.cs_adjoint_cases import image
from tests.test_cs_self_host import _item
from tests.test_cubed_sphere_host import PLACEMENTS, _patterns

X_FAST, Y_FAST, Z_FAST, K_FAST = (3, 2, 1, 0), (2, 3, 1, 0), (1, 2, 3, 0), (0, 1, 2, 3)
F32, F64, I32, I64 = 1, 2, 3, 4
# an fp64 scalar and an f32 3-vector per domain, x stride-1
TWO = [(X_FAST, 8, 1, 0, 1), (X_FAST, 4, 3, 1, 1)]
PLACES = dict(PLACEMENTS, two_ranks=lambda i, dom: dom["tile"] // 3)


class Exchange:
    """One exchange of `specs` = [(layout, elem, nc, vector, kind)] fields per domain of `rank`'s
    pattern, spec-major; self.items / self.domains: per item its ExchangeItem and fixture domain."""

    def __init__(self, ghx, cfg, specs, placement="one_rank", rank=0):
        self.ghx, self.cfg = ghx, cfg
        place = PLACES[placement]
        self.pats, _, order = _patterns(ghx, cfg, place)
        mine = [i for i in order if place(i, cfg["domains"][i]) == rank]
        self.items, cs_items, self.domains, self.specs = [], [], [], []
        for spec in specs:
            layout, elem, nc, vector, kind = spec
            for li, i in enumerate(mine):
                it, cs = _item(ghx, cfg, self.pats[rank], li, cfg["domains"][i], layout, elem, nc, vector, kind)
                self.items.append(it)
                cs_items.append(cs)
                self.domains.append(i)
                self.specs.append(spec)
        self.h = ctypes.c_void_p()
        ghx.call("ghx_cs_exchange_create", (ghx.ExchangeItem * len(self.items))(*self.items),
                 (ghx.CsItem * len(self.items))(*cs_items), len(self.items), ctypes.byref(self.h))
        self.n_items = len(self.items)

    def codes(self):
        return [{(4, 1): F32, (8, 1): F64, (4, 2): I32, (8, 2): I64}[(s[1], s[4] if s[3] else 1)]
                for s in self.specs]

    def error(self):
        return self.ghx.lib().ghx_last_error().decode()

    def create(self, codes=None):
        codes = self.codes() if codes is None else codes
        return self.ghx.lib().ghx_cs_exchange_adjoint_self_create(self.h, self.ghx.i32_array(codes), len(codes))

    def create_unfused(self, codes=None):
        codes = self.codes() if codes is None else codes
        return self.ghx.lib().ghx_cs_exchange_adjoint_create(self.h, self.ghx.i32_array(codes), len(codes))

    def info(self):
        f = ctypes.c_int32(-1)
        v = [ctypes.c_int64(-1) for _ in range(4)]
        self.ghx.call("ghx_cs_exchange_adjoint_self_info", self.h, ctypes.byref(f), *[ctypes.byref(x) for x in v])
        return dict(form=f.value, boxes=v[0].value, sources=v[1].value, field_sources=v[2].value,
                    rotated_sources=v[3].value)

    def unfused_info(self):
        r, xr, xt = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
        b, s = ctypes.c_int64(-1), ctypes.c_int64(-1)
        self.ghx.call("ghx_cs_exchange_adjoint_info", self.h, ctypes.byref(r), ctypes.byref(b), ctypes.byref(s),
                      ctypes.byref(xr), ctypes.byref(xt))
        return dict(ready=r.value, boxes=b.value, sources=s.value, x_records=xr.value, x_tiles=xt.value)

    def segments(self):
        """(ordinary segments, k_pack_x records) of the fused form's reverse pack, then the unfused one's."""
        p, x, up, uu = (ctypes.c_int32(-1) for _ in range(4))
        self.ghx.call("ghx_cs_exchange_adjoint_self_segments", self.h, ctypes.byref(p), ctypes.byref(x))
        self.ghx.call("ghx_cs_exchange_adjoint_segments", self.h, ctypes.byref(up), ctypes.byref(uu))
        return (p.value, x.value), (up.value, self.unfused_info()["x_records"])

    def plan(self):
        acc = ctypes.c_void_p()
        self.ghx.call("ghx_cs_exchange_adjoint_self_plan", self.h, ctypes.byref(acc))
        return acc

    def buffers(self, direction):
        """[(first_id, second_id, rank, size)] of the send (0) or receive (1) buffers."""
        n = ctypes.c_int32()
        self.ghx.call("ghx_exchange_num_buffers", self.h, direction, ctypes.byref(n))
        return n.value

    def close(self):
        self.ghx.lib().ghx_exchange_destroy(self.h)
        for p in self.pats:
            self.ghx.lib().ghx_pattern_destroy(p)


def sum_boxes(ghx, acc):
    """The sum sub-boxes of a plan: [(SAccumBoxInfo, [source index])]."""
    nb = ctypes.c_int64()
    ghx.call("ghx_saccum_info", acc, None, ctypes.byref(nb), None, None, None, None)
    out = []
    for k in range(nb.value):
        bx = ghx.SAccumBoxInfo()
        ghx.call("ghx_saccum_box", acc, k, ctypes.byref(bx))
        out.append((bx, list(range(bx.first_src, bx.first_src + bx.n_src))))
    return out


def source(ghx, acc, j):
    """Source record j: kind (1: field), slot, byte offset of the sub-box's origin, signed byte
    stride per dimension of the contribution's field, negate mask, component dimension, (entry, box)."""
    kind, slot, neg, comp, e, b = (ctypes.c_int32(-9) for _ in range(6))
    off = ctypes.c_uint64()
    strides = (ctypes.c_int64 * 4)()
    ghx.call("ghx_saccum_source_kind", acc, j, ctypes.byref(kind), ctypes.byref(slot), ctypes.byref(off))
    ghx.call("ghx_saccum_source_map", acc, j, strides, ctypes.byref(neg), ctypes.byref(comp))
    ghx.call("ghx_saccum_source", acc, j, ctypes.byref(e), ctypes.byref(b), None, None)
    origin = off.value - (1 << 64) if off.value >= (1 << 63) else off.value
    return dict(kind=kind.value, slot=slot.value, origin=origin, strides=list(strides), neg=neg.value,
                comp=comp.value, entry=e.value, box=b.value)


def receive_box(dom, x, y):
    """The generated box of fixture domain `dom` that holds local cell (x, y), or None."""
    for b in dom["boxes"]:
        if b["l"][0] <= x <= b["l"][3] and b["l"][1] <= y <= b["l"][4]:
            return b
    return None


def check_sources(ex):
    """Expand every field source record of ex's get plan over every cell of its sub-box and compare
    with the fixture: the byte offset is that of the halo cell whose image is the owner cell, the
    sign is the box's recorded sign. Returns per receiving item the read count of every cell of its
    local array (x, y, z, k)."""
    ghx, cfg = ex.ghx, ex.cfg
    acc = ex.plan()
    levels = cfg["levels"]
    reads = {}
    for bx, srcs in sum_boxes(ghx, acc):
        owner = cfg["domains"][ex.domains[bx.field_slot]]
        nc = ex.specs[bx.field_slot][2]
        x, y, z, k = np.meshgrid(np.arange(bx.first[0], bx.last[0] + 1), np.arange(bx.first[1], bx.last[1] + 1),
                                 np.arange(bx.first[2], bx.last[2] + 1), np.arange(nc), indexing="ij")
        for j in srcs:
            s = source(ghx, acc, j)
            if s["kind"] != 1:
                continue
            assert s["comp"] == 3
            fd = ex.items[s["slot"]].field
            rdom = cfg["domains"][ex.domains[s["slot"]]]
            st = s["strides"]
            off = (s["origin"] + (x - bx.first[0]) * st[0] + (y - bx.first[1]) * st[1] + (z - bx.first[2]) * st[2]
                   + k * st[3])
            # the receiving field is dense: the offset names one cell
            rem = off.copy()
            coord = [None] * 4
            for d in sorted(range(4), key=lambda d: -fd.byte_strides[d]):
                coord[d] = rem // fd.byte_strides[d]
                rem = rem - coord[d] * fd.byte_strides[d]
            assert (rem == 0).all()
            for d in range(4):
                assert (coord[d] >= 0).all() and (coord[d] < fd.extents[d]).all()
            hx, hy = coord[0] - fd.offsets[0], coord[1] - fd.offsets[1]
            assert np.array_equal(coord[2], z) and np.array_equal(coord[3], k)
            # one recorded box holds all these halo cells (a sub-box lies in one send box)
            b = receive_box(rdom, int(hx.flat[0]), int(hy.flat[0]))
            assert b is not None and b["t"] == owner["tile"]
            assert (hx >= b["l"][0]).all() and (hx <= b["l"][3]).all()
            assert (hy >= b["l"][1]).all() and (hy <= b["l"][4]).all()
            xn, yn = image(b, hx, hy)
            assert np.array_equal(xn, x + owner["x"][0]) and np.array_equal(yn, y + owner["y"][0])
            vector = ex.specs[s["slot"]][3]
            want = sum(1 << c for c in (0, 1) if vector and c < nc and b["sign"][c] < 0)
            assert s["neg"] == want, (s, b["sign"])
            r = reads.setdefault(s["slot"], np.zeros([fd.extents[d] for d in range(4)], dtype=np.int32))
            np.add.at(r, (coord[0], coord[1], coord[2], coord[3]), 1)
    assert levels > 0
    return reads
