"""Expectations of the cubed-sphere adjoint exchange, expanded from the recorded fixture through
tests/cs_cases.py (images and signs of every generated box; no transform table lives here):

* the rotated buffer of a box from the LOCAL field's bits: what the reverse pack must write, the
  dense global box in the neighbour's coordinates, row-major in the field's layout order, with
  vector components negated where the box's sign says so;
* the NumPy adjoint of a whole configuration on values: every halo cell of every receive box is
  added (negated likewise) to its owner cell, found among the configuration's domains by
  (t, xn, yn), and then, with zero_halos, set to zero.

The adjoint is computed on values for which the sum is exact in any order: small integers stored in
the element type (floats and integers), or integers that wrap."""
from __future__ import annotations

import numpy as np

from tests import cs_cases
from tests.cs_cases import _axes, layout_order, negate_bits


def image(b, x, y):
    """The neighbour-tile (xn, yn) of local cells (x, y) of generated box b (the map is affine)."""
    lf = b["l"][:3]
    i0, i1, i2 = b["img"][0:2], b["img"][2:4], b["img"][4:6]
    xn = i0[0] + (x - lf[0]) * (i1[0] - i0[0]) + (y - lf[1]) * (i2[0] - i0[0])
    yn = i0[1] + (x - lf[0]) * (i1[1] - i0[1]) + (y - lf[1]) * (i2[1] - i0[1])
    return xn, yn


def full_bits(df):
    """Bit patterns for EVERY cell of df's local array (halos and padding included), distinct per
    cell, with the special patterns of cs_cases.cell_bits."""
    big = max(df.shape[0], df.shape[1])
    x, y, z, k = df._grid(np.arange(df.shape[0]), np.arange(df.shape[1]))
    return cs_cases.cell_bits(df.dtype, df.dom["tile"], x, y, z, k, big, df.levels, df.nc,
                              special=df.special)


def _local_slice(df, b):
    lf, ll = b["l"][:3], b["l"][3:]
    return (slice(lf[0] + df.h, ll[0] + df.h + 1), slice(lf[1] + df.h, ll[1] + df.h + 1))


def rotated_buffer(df, bits, boxes, layout):
    """What the reverse pack writes for `boxes` of the local bit array `bits`, back to back."""
    order = layout_order(layout)
    out = []
    for b in boxes:
        lf, ll, gf, gl = b["l"][:3], b["l"][3:], b["g"][:3], b["g"][3:]
        x, y, z, k = df._grid(np.arange(lf[0], ll[0] + 1), np.arange(lf[1], ll[1] + 1))
        xn, yn = image(b, x, y)
        v = bits[_local_slice(df, b)].copy()
        if df.vector:
            for comp in (0, 1):
                if comp < df.nc and b["sign"][comp] < 0:
                    v[:, :, :, comp] = negate_bits(v[:, :, :, comp], df.dtype)
        g = np.zeros((gl[0] - gf[0] + 1, gl[1] - gf[1] + 1, df.levels, df.nc) + df.tail, v.dtype)
        hit = np.zeros(g.shape[:4], dtype=np.int32)
        g[xn - gf[0], yn - gf[1], z, k] = v
        np.add.at(hit, (xn - gf[0], yn - gf[1], z, k), 1)
        assert (hit == 1).all()  # the image of the local box is the whole global box, once
        out.append(np.ascontiguousarray(g.transpose(_axes(order, g))).ravel())
    return np.concatenate(out)


def small_values(df, salt=0):
    """The whole local array as integers 1..200 stored in df's type: sums of a few are exact."""
    x, y, z, k = df._grid(np.arange(df.shape[0]), np.arange(df.shape[1]))
    n = (((df.di * 131 + x) * 127 + y) * 31 + z) * 7 + k + salt
    return ((n * 37) % 200 + 1).astype(df.dtype)


def _mixed(df, salt):
    x, y, z, k = df._grid(np.arange(df.shape[0]), np.arange(df.shape[1]))
    n = ((((df.di * 131 + x) * 127 + y) * 31 + z) * 7 + k + salt).astype(np.uint64)
    return cs_cases.mix64(n)


def wrapping_values(df, salt=0):
    """The whole local array as integers over the type's full range: sums wrap."""
    return _mixed(df, salt).astype(cs_cases.uint_of(df.dtype)).view(df.dtype)


def order_sensitive_values(df, salt=0):
    """float32 values of mixed sign, full mantissas and exponents 2^-27 .. 2^22: a sum of three
    or more depends on the order of the additions."""
    bits = _mixed(df, salt).astype(np.uint32)
    expo = np.uint32(100) + (bits >> np.uint32(9)) % np.uint32(50)
    return ((bits & np.uint32(0x807FFFFF)) | (expo << np.uint32(23))).view(np.float32)


def owner_of(cfg, t, xn, yn):
    """Index of the configuration's domain that owns cell (xn, yn) of tile t."""
    for i, d in enumerate(cfg["domains"]):
        if d["tile"] == t and d["x"][0] <= xn <= d["x"][1] and d["y"][0] <= yn <= d["y"][1]:
            return i
    raise AssertionError(("no owner", t, xn, yn))


def numpy_adjoint(cfg, dfs, values, zero_halos):
    """The adjoint of the exchange of one field per domain: dfs[i] / values[i] are domain i's
    DomainField and whole local value array. Returns the new arrays. Every halo value is read
    before anything is added (the contributions land on owned cells only)."""
    out = [v.copy() for v in values]
    with np.errstate(over="ignore"):
        for i, (df, val) in enumerate(zip(dfs, values)):
            for b in df.dom["boxes"]:
                lf, ll = b["l"][:3], b["l"][3:]
                x, y, z, k = df._grid(np.arange(lf[0], ll[0] + 1), np.arange(lf[1], ll[1] + 1))
                xn, yn = image(b, x, y)
                v = val[_local_slice(df, b)].copy()
                if df.vector:
                    for comp in (0, 1):
                        if comp < df.nc and b["sign"][comp] < 0:
                            v[:, :, :, comp] = -v[:, :, :, comp]
                # the box's image lies in one or more domains of tile b["t"]
                own = np.vectorize(lambda a, c: owner_of(cfg, b["t"], a, c))(xn[:, :, 0, 0], yn[:, :, 0, 0])
                for o in np.unique(own):
                    m = np.broadcast_to((own == o)[:, :, None, None], v.shape)
                    od = dfs[o]
                    np.add.at(out[o], (xn[m] - od.dom["x"][0] + od.h, yn[m] - od.dom["y"][0] + od.h,
                                       z[m], k[m]), v[m])
        if zero_halos:
            for i, df in enumerate(dfs):
                for b in df.dom["boxes"]:
                    out[i][_local_slice(df, b)] = 0
    return out


def bits_of(values):
    return values.view(cs_cases.uint_of(values.dtype))
