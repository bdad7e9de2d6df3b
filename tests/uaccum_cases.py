"""Shared set-up of the adjoint accumulate tests (ghx_uaccum_create, k_accum_u): the NumPy form
of the operation's definition, ctypes helpers around the plan and its introspection calls, and
the element types.

The definition. Contribution entry e places a message of n lids and L levels in a buffer: element
(i, l) at buffer_offset + (i*L + l)*elem for levels first, buffer_offset + (i + l*n)*elem for
levels last. The accumulate does, for e ascending, i ascending and every level l,

    owner.values[lid_e[i]*index_stride + l*level_stride] += message_e[i, l]

in the element type (integers as unsigned: they wrap), so a cell starts from its own value and
adds its contributions in ascending (entry, position) — and then, with zero_halos, sets every
cell of the zero entries to zero bytes.

Works without a device (the plans can be described, not executed)."""
from __future__ import annotations

import ctypes

import numpy as np

from tests import uself_cases as US

DT_F32, DT_F64, DT_I32, DT_I64 = 1, 2, 3, 4
DTYPES = (DT_F32, DT_F64, DT_I32, DT_I64)
# the arithmetic type per code: integers are added as unsigned
NP = {DT_F32: np.dtype(np.float32), DT_F64: np.dtype(np.float64),
      DT_I32: np.dtype(np.uint32), DT_I64: np.dtype(np.uint64)}
NAMES = {DT_F32: "f32", DT_F64: "f64", DT_I32: "i32", DT_I64: "i64"}


def element_index(side):
    """(n, levels) element indices of the side's cells in its field."""
    d = side.desc
    lv = np.arange(d.levels, dtype=np.int64)[None, :]
    return side.lids[:, None] * d.index_stride + lv * d.level_stride


def message(buf_bytes, side, offset, dt):
    """Message of `side` read from the buffer image (uint8, from the buffer's first byte) as an
    (n, levels) array of dt."""
    d, n = side.desc, side.lids.size
    raw = np.frombuffer(buf_bytes[offset:offset + n * d.levels * dt.itemsize].tobytes(), dtype=dt)
    return raw.reshape(n, d.levels) if d.levels_first else raw.reshape(d.levels, n).T


def definition(fields, bufs, contrib, dtypes, places, zero, zero_halos=True):
    """The definition on host arrays, in place. fields[slot]: 1-D array of the slot's arithmetic
    type from the field's first element; bufs[slot]: uint8 image from the buffer's first byte;
    contrib / zero: lists of Side; places[e] = (buffer slot, buffer offset). An explicit loop in
    (entry, position) order; an entry whose lids are all distinct adds to each cell once, so its
    positions are taken in one vector operation."""
    for e, (s, (bslot, off)) in enumerate(zip(contrib, places)):
        dt = NP[dtypes[e]]
        F = fields[s.slot]
        assert F.dtype == dt
        c, idx = message(bufs[bslot], s, off, dt), element_index(s)
        if np.unique(s.lids).size == s.lids.size:
            F[idx] = F[idx] + c
        else:
            for i in range(s.lids.size):
                F[idx[i]] = F[idx[i]] + c[i]
    if zero_halos:
        for z in zero:
            fields[z.slot][element_index(z)] = 0
    return fields


def from_tables(fields, bufs, contrib, dtypes, places, dests, recs):
    """The sums again, driven by a plan's own tables (dests / recs as read back below): per sum
    destination its records in table order."""
    for d in dests:
        if d.zero:
            continue
        for j in range(d.first, d.first + d.count):
            e, pos = recs[j]
            s, (bslot, off) = contrib[e], places[e]
            dt = NP[dtypes[e]]
            c = message(bufs[bslot], s, off, dt)[pos]
            dd = s.desc
            idx = d.lid * dd.index_stride + np.arange(dd.levels) * dd.level_stride
            fields[d.field_slot][idx] = fields[d.field_slot][idx] + c
    return fields


# ---------------------------------------------------------------------------------------------
# ctypes
# ---------------------------------------------------------------------------------------------
def try_create(contrib, dtypes, places, zero=()):
    """(return code, last error, handle) of ghx_uaccum_create over lists of Side."""
    from ghex_amd import _ghx
    L = _ghx.lib()
    h = ctypes.c_void_p()
    rc = L.ghx_uaccum_create(US.entries(contrib, places), _ghx.i32_array(list(dtypes)), len(contrib),
                             US.entries(zero, [(0, 0)] * len(zero)), len(zero), ctypes.byref(h))
    return rc, (L.ghx_last_error() or b"").decode(), h


def create(contrib, dtypes, places, zero=()):
    rc, why, h = try_create(contrib, dtypes, places, zero)
    assert rc == 0, why
    return h


def destroy(h):
    from ghex_amd import _ghx
    assert _ghx.lib().ghx_uaccum_destroy(h) == 0


def info(h):
    """dict(bytes, n_dest, n_zero_dest, n_contrib, max_per_dest, n_tiles)"""
    from ghex_amd import _ghx
    b, t = ctypes.c_uint64(), ctypes.c_int32()
    v = [ctypes.c_int64() for _ in range(4)]
    _ghx.call("ghx_uaccum_info", h, ctypes.byref(b), *[ctypes.byref(x) for x in v], ctypes.byref(t))
    return dict(bytes=b.value, n_dest=v[0].value, n_zero_dest=v[1].value, n_contrib=v[2].value,
                max_per_dest=v[3].value, n_tiles=t.value)


def dests(h):
    from ghex_amd import _ghx
    i, out = info(h), []
    for k in range(i["n_dest"] + i["n_zero_dest"]):
        d = _ghx.UAccumDestInfo()
        _ghx.call("ghx_uaccum_dest", h, k, ctypes.byref(d))
        out.append(d)
    return out


def records(h):
    """[(entry, position)] of every contribution record."""
    from ghex_amd import _ghx
    e, p, out = ctypes.c_int32(), ctypes.c_int64(), []
    for j in range(info(h)["n_contrib"]):
        _ghx.call("ghx_uaccum_contrib", h, j, ctypes.byref(e), ctypes.byref(p))
        out.append((e.value, p.value))
    return out


def draw_values(rng, n, code):
    """n elements of the code's arithmetic type: floats with magnitudes in [2^-20, 2^20] and
    either sign (no sum of a few hundred of them is subnormal, inf or NaN), integers over the
    whole range (sums wrap)."""
    dt = NP[code]
    if dt.kind == "f":
        return (np.exp2(rng.uniform(-20, 20, n)) * rng.choice([-1.0, 1.0], n)).astype(dt)
    return rng.integers(0, np.iinfo(dt).max, size=n, dtype=dt, endpoint=True)


def three_lists_case(od, hd, seed=0, repeats=False, boff=0):
    """The standard case (tests/test_gpu_uself.py's lists): three messages of 3001, 3002 and 3003
    lids drawn without repetition from 10007 cells. Owner fields are slots 0 (message 0) and 1
    (messages 1 and 2), halo fields slots 2 and 3; messages 0 and 1 share buffer 0 (the second
    16-byte aligned behind the first), message 2 has buffer 1. repeats: one owner cell 286 more
    times in message 0, and one cell of message 1 also in message 2. Returns (contrib sides, zero
    sides, places)."""
    from tests import uput_cases as UC
    from tests.uput_cases import Side
    rng = np.random.default_rng(seed)
    s, t = UC.draw_lists(rng), UC.draw_lists(rng)
    if repeats:
        s[0][1:2000:7] = s[0][0]
        s[2][-1] = s[1][-1]
    contrib = [Side(od, 0, s[0]), Side(od, 1, s[1]), Side(od, 1, s[2])]
    zero = [Side(hd, 2, t[0]), Side(hd, 3, t[1]), Side(hd, 3, t[2])]
    nb0 = US.message_bytes(contrib[0])
    places = [(0, boff), (0, (boff + nb0 + 15) // 16 * 16), (1, boff)]
    return contrib, zero, places
