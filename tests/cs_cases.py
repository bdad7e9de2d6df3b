"""The cubed-sphere fixture (tests/golden/cubed_sphere_case.json, recorded from the reference by
tests/golden/make_cubed_sphere_case.py) and the expectations the tests expand from it.

Per configuration {edge_size, levels, halos (-x, +x, -y, +y), domains}; per domain {tile, x, y,
boxes}; per generated box: l / g = local / global (x, y, z) first then last, t = the tile of the
global box, img = the neighbour-tile (x, y) of the local cells first, first + (1, 0) and
first + (0, 1) — the map is affine, so these three give every cell —, sign = the factors of
vector components 0 and 1, x = the non-empty seven-argument intersections
[domain index, local first, local last, global first, global last].

No transform table lives here: every per-cell expectation comes from the recorded images.

Element types are named: a numpy dtype name, "bfloat16", or "rawN" (N opaque bytes). Bit patterns
are unsigned integers of the element's size (1, 2, 4, 8 bytes) or, for every other size, uint8
with one trailing axis of N bytes."""
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


_NO_NUMPY = {"bfloat16": 2}  # element types numpy has no dtype for: their size


def elem_size(dtype):
    name = dtype if isinstance(dtype, str) else np.dtype(dtype).name
    if name in _NO_NUMPY:
        return _NO_NUMPY[name]
    if name.startswith("raw"):
        return int(name[3:])
    return np.dtype(name).itemsize


def elem_kind(dtype):
    """'f' (negated by its sign bit), 'i' (two's complement) or anything else (opaque bits)."""
    name = dtype if isinstance(dtype, str) else np.dtype(dtype).name
    return "V" if name in _NO_NUMPY or name.startswith("raw") else np.dtype(name).kind


def uint_of(dtype):
    """The unsigned type of an element's bits; uint8 (with a trailing byte axis, see tail_of) for
    sizes that have none."""
    return {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}.get(elem_size(dtype), np.uint8)


def tail_of(dtype):
    """() for elements held as one unsigned integer, (N,) for those held as N bytes."""
    n = elem_size(dtype)
    return () if n in (1, 2, 4, 8) else (n,)


def mix64(n):
    """splitmix64's output function of the uint64 array n."""
    with np.errstate(over="ignore"):
        z = np.asarray(n).astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


# n % 97 of the cells that hold a special integer (integer fields made with special=True): where
# a negation done in halves, or without its carry, goes wrong
INT_SPECIAL = {3: "zero", 7: "min", 13: "minus_one", 19: "low_word_zero", 23: "low_word_ones"}


def cell_bits(dtype, tile, x, y, z, k, c, levels, nc, special=False):
    """The bit pattern of global cell (tile, x, y, z, k). 4- and 8-byte numpy types: the cell
    number n as a value of the type, distinct per cell, exactly representable in every tested
    type; float fields carry -0.0, inf and a NaN at some cells, and integer fields made with
    special=True carry 0, the minimum, -1 and (int64) k << 32 and (k << 32) | 0xFFFFFFFF at the
    cells of INT_SPECIAL. Every other size: bits of splitmix64 of n (the low bits for 1 and 2
    bytes, the first N bytes of two mixed words up to 16)."""
    n = ((((tile * c + x) * c + y) * levels + z) * nc + k) + 1
    size = elem_size(dtype)
    if size not in (4, 8) or elem_kind(dtype) == "V":
        if size <= 8:
            return mix64(n).astype(uint_of(dtype))
        if size > 16:
            raise ValueError("elements of at most 16 bytes")
        two = np.stack([mix64(2 * np.asarray(n)), mix64(2 * np.asarray(n) + 1)], axis=-1)
        return np.ascontiguousarray(two.astype("<u8")).view(np.uint8)[..., :size].copy()
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
    elif dt.kind == "i" and special:
        w = 8 * dt.itemsize
        for r, what in INT_SPECIAL.items():
            at = n % 97 == r
            if what == "zero":
                bits[at] = u(0)
            elif what == "min":
                bits[at] = u(1 << (w - 1))
            elif what == "minus_one":
                bits[at] = u((1 << w) - 1)
            elif w == 64:
                low = u(0) if what == "low_word_zero" else u(0xFFFFFFFF)
                bits[at] = (np.asarray(n).astype(u)[at] << u(32)) | low
    return bits


def as_bytes(bits, dtype):
    """Bit patterns as uint8 with a trailing axis of the element's bytes (little endian)."""
    size = elem_size(dtype)
    if tail_of(dtype):
        return np.ascontiguousarray(bits)
    b = np.ascontiguousarray(bits).astype(np.dtype(uint_of(dtype)).newbyteorder("<"))
    return b.view(np.uint8).reshape(bits.shape + (size,))


def negate_bits(bits, dtype):
    """Negation as the unpack performs it: sign-bit flip (floats), two's complement (ints)."""
    dt = np.dtype(dtype)
    u = uint_of(dt)
    if dt.kind == "f":
        return bits ^ u(1 << (8 * dt.itemsize - 1))
    return (~bits + u(1)).astype(u)


def _axes(perm, a):
    """The axis permutation `perm` of an array's leading axes, any trailing byte axis kept last."""
    return list(perm) + list(range(len(perm), a.ndim))


def layout_order(layout):
    """Memory axis order (slowest first) of a layout map (layout[d] = 0 for the slowest dim)."""
    return sorted(range(len(layout)), key=lambda d: layout[d])


class DomainField:
    """One domain's field as bit patterns: logical (x, y, z, k) numpy array with `pad` untouched
    cells beyond the widest halo on every x / y side, and what an exchange must leave in it."""

    def __init__(self, cfg, di, dtype, nc, vector, pad=1, special=False):
        self.cfg, self.di, self.dom = cfg, di, cfg["domains"][di]
        self.dtype = np.dtype(dtype) if elem_kind(dtype) != "V" else dtype
        self.nc, self.vector, self.special = nc, vector, special
        self.tail = tail_of(dtype)
        self.c, self.levels = cfg["edge_size"], cfg["levels"]
        self.h = max(cfg["halos"]) + pad
        self.nx = self.dom["x"][1] - self.dom["x"][0] + 1
        self.ny = self.dom["y"][1] - self.dom["y"][0] + 1
        self.shape = (self.nx + 2 * self.h, self.ny + 2 * self.h, self.levels, nc)
        self.offsets = (self.h, self.h, 0)
        self.extents = self.shape[:3]
        u = uint_of(dtype)
        self.sentinel = u(int.from_bytes(bytes([SENTINEL_BYTE]) * np.dtype(u).itemsize, "little"))

    def _grid(self, xs, ys):
        return np.meshgrid(xs, ys, np.arange(self.levels), np.arange(self.nc), indexing="ij")

    def initial(self):
        """Interior = the cell values, everything else the sentinel."""
        a = np.full(self.shape + self.tail, self.sentinel, dtype=uint_of(self.dtype))
        x, y, z, k = self._grid(np.arange(self.nx), np.arange(self.ny))
        a[self.h:self.h + self.nx, self.h:self.h + self.ny] = self._bits(
            self.dom["tile"], x + self.dom["x"][0], y + self.dom["y"][0], z, k)
        return a

    def _bits(self, tile, x, y, z, k):
        return cell_bits(self.dtype, tile, x, y, z, k, self.c, self.levels, self.nc,
                         **({"special": True} if self.special else {}))

    def box_values(self, b):
        """(local x, local y index arrays, expected bits over (x, y, z, k)) of generated box b."""
        lf, ll = b["l"][:3], b["l"][3:]
        xs, ys = np.arange(lf[0], ll[0] + 1), np.arange(lf[1], ll[1] + 1)
        x, y, z, k = self._grid(xs, ys)
        i0, i1, i2 = b["img"][0:2], b["img"][2:4], b["img"][4:6]
        xn = i0[0] + (x - lf[0]) * (i1[0] - i0[0]) + (y - lf[1]) * (i2[0] - i0[0])
        yn = i0[1] + (x - lf[0]) * (i1[1] - i0[1]) + (y - lf[1]) * (i2[1] - i0[1])
        bits = self._bits(b["t"], xn, yn, z, k)
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
            bits = self._bits(b["t"], x, y, z, k)
            out.append(np.ascontiguousarray(bits.transpose(_axes(order, bits))).ravel())
        return np.concatenate(out)

    def spaces(self, boxes):
        return [(tuple(b["l"][:3]), tuple(b["l"][3:]), tuple(b["g"][:3]), tuple(b["g"][3:]),
                 b["t"]) for b in boxes]


def _torch_dtype(dtype):
    import torch
    return getattr(torch, dtype if isinstance(dtype, str) else np.dtype(dtype).name)


def to_device(bits, layout, dtype):
    """(base, logical): the logical (x, y, z, k) bit array on the device in the memory layout of
    `layout`, viewed as `dtype`; logical is the permuted view indexed (x, y, z, k)."""
    import torch
    order = layout_order(layout)
    mem = np.ascontiguousarray(bits.transpose(_axes(order, bits)))
    if elem_kind(dtype) != "V" and not tail_of(dtype):
        base = torch.from_numpy(mem.view(np.dtype(dtype))).cuda()
    else:
        # no numpy view of the type (bfloat16) or no integer of its size (complex128): the bytes
        # go up as they are and torch views them
        size = elem_size(dtype)
        raw = torch.from_numpy(as_bytes(mem, dtype).reshape(mem.shape[:len(layout) - 1] + (-1,)))
        base = raw.cuda().view(_torch_dtype(dtype))
        assert tuple(base.shape) == mem.shape[:len(layout)] and base.element_size() == size
    return base, base.permute(*[order.index(d) for d in range(len(layout))])


def from_device(base, layout, dtype):
    """The logical bit array of a device field made by to_device."""
    import torch
    order = layout_order(layout)
    raw = base.cpu().contiguous().view(torch.uint8).numpy()
    mem = raw.reshape(tuple(base.shape) + (elem_size(dtype),))
    mem = mem if tail_of(dtype) else mem.view(uint_of(dtype)).reshape(tuple(base.shape))
    return mem.transpose(_axes([order.index(d) for d in range(len(layout))], mem))


def buffer_to_device(bits, dtype):
    """A packed buffer (DomainField.buffer) on the device, as bytes."""
    import torch
    return torch.from_numpy(as_bytes(bits, dtype).ravel().copy()).cuda()


# ---------------------------------------------------------------------------------------------
# byte-addressed fields
# ---------------------------------------------------------------------------------------------
def dense_strides(shape, layout, elem, pad=None):
    """Byte strides of a (x, y, z, k) field of `shape` in the memory order of `layout`; pad =
    {dim: bytes} adds pitch padding to a dim's stride (the slower dims grow with it)."""
    strides, s = [0] * len(shape), elem
    for d in reversed(layout_order(layout)):
        s += (pad or {}).get(d, 0)
        strides[d] = s
        s *= shape[d]
    return tuple(strides)


class ArenaField:
    """A DomainField in a uint8 arena filled with the sentinel: element (x, y, z, k) lies at
    base + sum(coordinate * byte stride) for any positive byte strides, with GUARD bytes before
    the first and after the last element; base = GUARD + shift. arena(bits) is the whole arena
    holding the logical bit array, so comparing two arenas also compares guards and padding."""

    GUARD = 256

    def __init__(self, df, byte_strides, shift=0):
        self.df, self.elem = df, elem_size(df.dtype)
        self.strides = tuple(int(s) for s in byte_strides)
        self.base = self.GUARD + shift
        grid = np.meshgrid(*[np.arange(n, dtype=np.int64) for n in df.shape], indexing="ij")
        first = self.base + sum(g * s for g, s in zip(grid, self.strides))
        self.index = first[..., None] + np.arange(self.elem)
        self.size = int(self.index.max()) + 1 + self.GUARD
        assert np.unique(self.index).size == self.index.size  # no two elements overlap

    def arena(self, bits):
        a = np.full(self.size, SENTINEL_BYTE, dtype=np.uint8)
        a[self.index] = as_bytes(bits, self.df.dtype)
        return a

    def layout(self):
        """layout[d] = 0 for the dim of the largest stride."""
        order = sorted(range(4), key=lambda d: -self.strides[d])
        return tuple(order.index(d) for d in range(4))
