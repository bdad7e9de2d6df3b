"""The cubed-sphere fixture (tests/golden/cubed_sphere_case.json, recorded from the reference by
tests/golden/make_cubed_sphere_case.py) and the expectations the tests expand from it.

Per configuration {edge_size, levels, halos (-x, +x, -y, +y), domains}; per domain {tile, x, y,
boxes}; per generated box: l / g = local / global (x, y, z) first then last, t = the tile of the
global box, img = the neighbour-tile (x, y) of the local cells first, first + (1, 0) and
first + (0, 1) — the map is affine, so these three give every cell —, sign = the factors of
vector components 0 and 1, x = the non-empty seven-argument intersections
[domain index, local first, local last, global first, global last].

No transform table lives here: every per-cell expectation comes from the recorded images."""
from __future__ import annotations

import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL_BYTE = 0xC3


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(HERE, "golden", "cubed_sphere_case.json")) as fh:
        return json.load(fh)


def config(edge_size):
    return next(c for c in fixture() if c["edge_size"] == edge_size)


def domain_id(c, dom):
    return (dom["tile"] * c + dom["y"][0]) * c + dom["x"][0]


def uint_of(dtype):
    return {4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]


def cell_bits(dtype, tile, x, y, z, k, c, levels, nc):
    """The bit pattern of global cell (tile, x, y, z, k): distinct per cell, exactly
    representable in every tested type; float fields carry -0.0, inf and a NaN at some cells."""
    n = ((((tile * c + x) * c + y) * levels + z) * nc + k) + 1
    dt = np.dtype(dtype)
    v = np.asarray(n).astype(dt)
    u = uint_of(dt)
    bits = v.view(u).copy()
    if dt.kind == "f":
        special = {5: -0.0, 11: np.inf}
        for r, val in special.items():
            bits[n % 97 == r] = np.asarray(val, dt).view(u)
        nan = u(0x7FC01234) if dt.itemsize == 4 else u(0x7FF8000000001234)
        bits[n % 97 == 17] = nan
    return bits


def negate_bits(bits, dtype):
    """Negation as the unpack performs it: sign-bit flip (floats), two's complement (ints)."""
    dt = np.dtype(dtype)
    u = uint_of(dt)
    if dt.kind == "f":
        return bits ^ u(1 << (8 * dt.itemsize - 1))
    return (~bits + u(1)).astype(u)


def layout_order(layout):
    """Memory axis order (slowest first) of a layout map (layout[d] = 0 for the slowest dim)."""
    return sorted(range(len(layout)), key=lambda d: layout[d])


class DomainField:
    """One domain's field as bit patterns: logical (x, y, z, k) numpy array with `pad` untouched
    cells beyond the widest halo on every x / y side, and what an exchange must leave in it."""

    def __init__(self, cfg, di, dtype, nc, vector, pad=1):
        self.cfg, self.di, self.dom = cfg, di, cfg["domains"][di]
        self.dtype, self.nc, self.vector = np.dtype(dtype), nc, vector
        self.c, self.levels = cfg["edge_size"], cfg["levels"]
        self.h = max(cfg["halos"]) + pad
        self.nx = self.dom["x"][1] - self.dom["x"][0] + 1
        self.ny = self.dom["y"][1] - self.dom["y"][0] + 1
        self.shape = (self.nx + 2 * self.h, self.ny + 2 * self.h, self.levels, nc)
        self.offsets = (self.h, self.h, 0)
        self.extents = self.shape[:3]
        u = uint_of(dtype)
        self.sentinel = u(int.from_bytes(bytes([SENTINEL_BYTE]) * self.dtype.itemsize, "little"))

    def _grid(self, xs, ys):
        return np.meshgrid(xs, ys, np.arange(self.levels), np.arange(self.nc), indexing="ij")

    def initial(self):
        """Interior = the cell values, everything else the sentinel."""
        a = np.full(self.shape, self.sentinel, dtype=uint_of(self.dtype))
        x, y, z, k = self._grid(np.arange(self.nx), np.arange(self.ny))
        a[self.h:self.h + self.nx, self.h:self.h + self.ny] = cell_bits(
            self.dtype, self.dom["tile"], x + self.dom["x"][0], y + self.dom["y"][0], z, k,
            self.c, self.levels, self.nc)
        return a

    def box_values(self, b):
        """(local x, local y index arrays, expected bits over (x, y, z, k)) of generated box b."""
        lf, ll = b["l"][:3], b["l"][3:]
        xs, ys = np.arange(lf[0], ll[0] + 1), np.arange(lf[1], ll[1] + 1)
        x, y, z, k = self._grid(xs, ys)
        i0, i1, i2 = b["img"][0:2], b["img"][2:4], b["img"][4:6]
        xn = i0[0] + (x - lf[0]) * (i1[0] - i0[0]) + (y - lf[1]) * (i2[0] - i0[0])
        yn = i0[1] + (x - lf[0]) * (i1[1] - i0[1]) + (y - lf[1]) * (i2[1] - i0[1])
        bits = cell_bits(self.dtype, b["t"], xn, yn, z, k, self.c, self.levels, self.nc)
        if self.vector:
            for comp in (0, 1):
                if comp < self.nc and b["sign"][comp] < 0:
                    bits[..., comp] = negate_bits(bits[..., comp], self.dtype)
        return xs, ys, bits

    def expected(self, boxes=None):
        """The field after the exchange (or after unpacking `boxes` only)."""
        a = self.initial()
        for b in (self.dom["boxes"] if boxes is None else boxes):
            xs, ys, bits = self.box_values(b)
            a[xs[0] + self.h:xs[-1] + self.h + 1, ys[0] + self.h:ys[-1] + self.h + 1] = bits
        return a

    def buffer(self, boxes, layout):
        """What the senders pack for `boxes`, back to back: per box the dense global box in the
        neighbour's coordinates, row-major in the field's layout order."""
        order = layout_order(layout)
        out = []
        for b in boxes:
            gf, gl = b["g"][:3], b["g"][3:]
            x, y, z, k = np.meshgrid(np.arange(gf[0], gl[0] + 1), np.arange(gf[1], gl[1] + 1),
                                     np.arange(gf[2], gl[2] + 1), np.arange(self.nc),
                                     indexing="ij")
            bits = cell_bits(self.dtype, b["t"], x, y, z, k, self.c, self.levels, self.nc)
            out.append(np.ascontiguousarray(bits.transpose(order)).ravel())
        return np.concatenate(out)

    def spaces(self, boxes):
        return [(tuple(b["l"][:3]), tuple(b["l"][3:]), tuple(b["g"][:3]), tuple(b["g"][3:]),
                 b["t"]) for b in boxes]


def to_device(bits, layout, dtype):
    """(base, logical): the logical (x, y, z, k) bit array on the device in the memory layout of
    `layout`, viewed as `dtype`; logical is the permuted view indexed (x, y, z, k)."""
    import torch
    order = layout_order(layout)
    mem = np.ascontiguousarray(bits.transpose(order))
    base = torch.from_numpy(mem.view(np.dtype(dtype))).cuda()
    return base, base.permute(*[order.index(d) for d in range(len(layout))])


def from_device(base, layout, dtype):
    """The logical bit array of a device field made by to_device."""
    order = layout_order(layout)
    mem = base.cpu().numpy().view(uint_of(dtype))
    return mem.transpose([order.index(d) for d in range(len(layout))])
