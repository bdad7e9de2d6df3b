"""Shared set-up of the structured adjoint accumulate tests (ghx_saccum_create, k_accum_s): field
geometries, the case table, the NumPy form of the operation's definition, ctypes helpers around
the plan and its introspection calls.

The definition. Contribution entry e places its boxes one after the other from buffer_offset on,
each dense in the field's layout order with the component axis (the position ghx_plan_create
gives a box cell). The accumulate does, for e ascending, box b ascending and every cell of the box,

    field[cell] += message_e_b[cell]

in the element type (integers as unsigned: they wrap) — a box holds a cell at most once, so a cell
starts from its own value and adds its contributions in ascending (entry, box) — and then, with
zero_halos, sets every cell of the zero entries' boxes to zero bytes.

Works without a device (the plans can be described, not executed)."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from tests.uaccum_cases import DT_F32, DT_F64, DT_I32, DT_I64, DTYPES, NAMES, NP, draw_values  # noqa: F401

LAYOUTS_3D = ((2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 0, 2), (0, 2, 1), (0, 1, 2))


@dataclass(frozen=True)
class Geo:
    """A field: spatial extents (halos included) and offsets, element size, layout map over all
    dims (the component axis, when ncomp > 0, is the last dim), element stride of the fastest dim."""
    ext: Tuple[int, ...]
    offs: Tuple[int, ...]
    elem: int
    layout: Tuple[int, ...]
    ncomp: int = 0
    fast: int = 1

    @property
    def dims(self):
        return self.ext + ((self.ncomp,) if self.ncomp else ())

    @property
    def spatial(self):
        return len(self.ext)

    @property
    def by_speed(self):
        """dims, fastest first"""
        D = len(self.layout)
        return [self.layout.index(D - 1 - k) for k in range(D)]

    @property
    def strides(self):
        """element stride per dim"""
        st, s = [0] * len(self.layout), self.fast
        for d in self.by_speed:
            st[d] = s
            s *= self.dims[d]
        return tuple(st)

    @property
    def n_elems(self):
        d = self.by_speed[-1]
        return self.strides[d] * self.dims[d]

    def desc(self):
        from ghex_amd import _ghx
        fd = _ghx.FieldDesc()
        fd.dim, fd.elem_size = len(self.layout), self.elem
        for d in range(len(self.layout)):
            fd.layout[d] = self.layout[d]
            fd.byte_strides[d] = self.strides[d] * self.elem
            fd.offsets[d] = self.offs[d] if d < self.spatial else 0
            fd.extents[d] = self.dims[d]
        fd.num_components = max(1, self.ncomp)
        fd.has_components = 1 if self.ncomp else 0
        return fd

    def spec(self, data):
        """The oracle's description of the field over `data` (its raw storage)."""
        from oracle import oracle as orc
        offs = self.offs + ((0,) if self.ncomp else ())
        return orc.FieldSpec(data, self.elem, self.layout, offs, self.dims,
                             tuple(s * self.elem for s in self.strides), max(1, self.ncomp), bool(self.ncomp))

    def lattice(self, first, last, stride_of, origin=None):
        """sum over the dims of (coordinate - origin) * stride_of[dim] for every cell of the box
        [first, last] (spatial; every component), in the box's buffer order: slowest layout dim
        outermost. origin None: the coordinate itself plus the field's offset (a field index)."""
        out = np.zeros(1, dtype=np.int64)
        for d in reversed(self.by_speed):
            if d < self.spatial:
                c = np.arange(first[d], last[d] + 1, dtype=np.int64)
                c = c + self.offs[d] if origin is None else c - origin[d]
            else:
                c = np.arange(self.ncomp, dtype=np.int64)
            out = np.add.outer(out, c * stride_of[d]).reshape(-1)
        return out

    def box_index(self, first, last):
        """element indices in the field of the box's cells, in buffer order"""
        return self.lattice(first, last, self.strides)

    def box_strides(self, first, last):
        """byte stride per dim of the box's dense buffer box"""
        st, s = [0] * len(self.layout), self.elem
        for d in self.by_speed:
            st[d] = s
            s *= (last[d] - first[d] + 1) if d < self.spatial else self.ncomp
        return st

    def box_bytes(self, first, last):
        n = max(1, self.ncomp) * self.elem
        for f, l in zip(first, last):
            n *= l - f + 1
        return n


def cube(N, H, elem=8, layout=None, D=3, ncomp=0, fast=1):
    """A field over one N^D domain with halo H (layout None: the first dim fastest)."""
    layout = tuple(range(D - 1, -1, -1)) if layout is None else tuple(layout)
    return Geo((N + 2 * H,) * D, (H,) * D, elem, layout, ncomp, fast)


@dataclass
class Ent:
    """One entry: a field slot's boxes [(first, last)] placed in a buffer."""
    geo: Geo
    slot: int
    boxes: list
    bslot: int = 0
    boff: int = 0

    @property
    def nbytes(self):
        return sum(self.geo.box_bytes(f, l) for f, l in self.boxes)


def c_entries(ents):
    """ctypes array of ghx_pack_entry over a list of Ent (the array keeps its boxes alive)."""
    from ghex_amd import _ghx
    arr = (_ghx.PackEntry * max(1, len(ents)))()
    keep = []
    for k, e in enumerate(ents):
        bx = (_ghx.Box * max(1, len(e.boxes)))()
        for i, (f, l) in enumerate(e.boxes):
            for d in range(len(f)):
                bx[i].first[d], bx[i].last[d] = f[d], l[d]
        keep.append(bx)
        arr[k].field = e.geo.desc()
        arr[k].field_slot, arr[k].buffer_slot, arr[k].buffer_offset = e.slot, e.bslot, e.boff
        arr[k].boxes, arr[k].n_boxes = bx, len(e.boxes)
    arr._keep = keep
    return arr


def try_create(contrib, dtypes, zero=()):
    """(return code, last error, handle) of ghx_saccum_create over lists of Ent."""
    from ghex_amd import _ghx
    L = _ghx.lib()
    h = ctypes.c_void_p()
    c, z = c_entries(list(contrib)), c_entries(list(zero))
    rc = L.ghx_saccum_create(c, _ghx.i32_array(list(dtypes)), len(contrib), z, len(zero), ctypes.byref(h))
    return rc, (L.ghx_last_error() or b"").decode(), h


def create(contrib, dtypes, zero=()):
    rc, why, h = try_create(contrib, dtypes, zero)
    assert rc == 0, why
    return h


def destroy(h):
    from ghex_amd import _ghx
    assert _ghx.lib().ghx_saccum_destroy(h) == 0


def info(h):
    """dict(bytes, n_boxes, n_zero_boxes, n_sources, max_sources, n_tiles)"""
    from ghex_amd import _ghx
    b, t = ctypes.c_uint64(), ctypes.c_int32()
    v = [ctypes.c_int64() for _ in range(4)]
    _ghx.call("ghx_saccum_info", h, ctypes.byref(b), *[ctypes.byref(x) for x in v], ctypes.byref(t))
    return dict(bytes=b.value, n_boxes=v[0].value, n_zero_boxes=v[1].value, n_sources=v[2].value,
                max_sources=v[3].value, n_tiles=t.value)


@dataclass
class SubBox:
    slot: int
    zero: bool
    first: tuple
    last: tuple
    row_elems: int
    wlog2: int
    first_src: int
    n_src: int


def boxes(h, spatial=3):
    from ghex_amd import _ghx
    i, out = info(h), []
    for k in range(i["n_boxes"] + i["n_zero_boxes"]):
        b = _ghx.SAccumBoxInfo()
        _ghx.call("ghx_saccum_box", h, k, ctypes.byref(b))
        out.append(SubBox(b.field_slot, bool(b.zero), tuple(b.first[:spatial]), tuple(b.last[:spatial]),
                          b.row_elems, b.wlog2, b.first_src, b.n_src))
    return out


def sources(h):
    """[(entry, box, buffer slot, buffer offset of the sub-box's origin)] of every source record."""
    from ghex_amd import _ghx
    e, b, s, o, out = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64(), []
    for j in range(info(h)["n_sources"]):
        _ghx.call("ghx_saccum_source", h, j, ctypes.byref(e), ctypes.byref(b), ctypes.byref(s), ctypes.byref(o))
        out.append((e.value, b.value, s.value, o.value))
    return out


def tables(contrib, dtypes, zero=()):
    """(info, sub-boxes, sources) of the plan of the entries."""
    h = create(contrib, dtypes, zero)
    try:
        sp = contrib[0].geo.spatial if contrib else (zero[0].geo.spatial if zero else 3)
        return info(h), boxes(h, sp), sources(h)
    finally:
        destroy(h)


# ---------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------
def definition(fields, bufs, contrib, dtypes, zero, zero_halos=True, reverse=False):
    """The definition on host arrays, in place. fields[slot]: 1-D array of the slot's arithmetic
    type from the field's first element; bufs[slot]: uint8 image from the buffer's first byte.
    An explicit loop over (entry, box) in order (reverse: in the opposite order, for the order
    tests); a box holds a cell once, so its cells are taken in one vector operation."""
    todo = []
    for e, en in enumerate(contrib):
        at = en.boff
        for f, l in en.boxes:
            todo.append((e, en, f, l, at))
            at += en.geo.box_bytes(f, l)
    for e, en, f, l, at in (todo[::-1] if reverse else todo):
        dt = NP[dtypes[e]]
        F = fields[en.slot]
        assert F.dtype == dt
        idx = en.geo.box_index(f, l)
        msg = np.frombuffer(bufs[en.bslot][at:at + idx.size * dt.itemsize].tobytes(), dtype=dt)
        F[idx] = F[idx] + msg
    if zero_halos:
        for z in zero:
            for f, l in z.boxes:
                fields[z.slot][z.geo.box_index(f, l)] = 0
    return fields


def source_bytes(geo, sub, ent, box, origin_off):
    """Byte offsets in the source's buffer of every cell of sub-box `sub` (in the sub-box's own
    buffer order, the order of geo.box_index(sub.first, sub.last)), from the record's offset of
    the origin and the strides of box `box` of `ent`'s dense buffer box."""
    f, l = ent.boxes[box]
    return origin_off + geo.lattice(sub.first, sub.last, geo.box_strides(f, l), origin=sub.first)


def from_tables(fields, bufs, contrib, dtypes, subs, srcs, zero_halos=True):
    """The operation again, driven by a plan's own tables: per sum sub-box its sources in list
    order, then the zero sub-boxes."""
    geo_of = {en.slot: en.geo for en in contrib}
    for sb in subs:
        if sb.zero:
            continue
        geo = geo_of[sb.slot]
        idx = geo.box_index(sb.first, sb.last)
        for j in range(sb.first_src, sb.first_src + sb.n_src):
            e, b, bslot, off = srcs[j]
            dt = NP[dtypes[e]]
            at = source_bytes(geo, sb, contrib[e], b, off)
            assert (at % dt.itemsize == 0).all() and bslot == contrib[e].bslot
            msg = bufs[bslot][:bufs[bslot].size // dt.itemsize * dt.itemsize].view(dt)[at // dt.itemsize]
            fields[sb.slot][idx] = fields[sb.slot][idx] + msg
    return fields


# ---------------------------------------------------------------------------------------------
# geometries from the product's patterns
# ---------------------------------------------------------------------------------------------
def pattern_boxes(domains, gfirst, glast, H, periodic):
    """The product's make_pattern over `domains` [(id, first, last)] held by one rank: per domain
    (send, recv), each a list of (remote id, [(local first, local last)]) in pattern order."""
    import ghex_amd
    from ghex_amd.structured import regular as R
    D = len(gfirst)
    dds = [R.DomainDescriptor(i, tuple(f), tuple(l)) for i, f, l in domains]
    pc = R.make_pattern(ghex_amd.make_context(), R.HaloGenerator(tuple(gfirst), tuple(glast), (H,) * (2 * D),
                                                                 (bool(periodic),) * D), dds)
    out = []
    for k in range(len(dds)):
        side = []
        for halos in (pc.send_halos(k), pc.recv_halos(k)):
            side.append([(rid, [(tuple(sp[0]), tuple(sp[1])) for sp in spaces]) for rid, _, _, spaces in halos])
        out.append(tuple(side))
    return out


def periodic_cube(N, H, D=3):
    """One periodic domain of N^D with halo H: (send boxes, recv boxes)."""
    (send, recv), = pattern_boxes([(0, (0,) * D, (N - 1,) * D)], (0,) * D, (N - 1,) * D, H, True)
    return [b for _, bx in send for b in bx], [b for _, bx in recv for b in bx]


def one_domain_entries(geo, N, H, code=None, bshift=0):
    """Contribution and zero entry of one periodic N^D domain over `geo`: every send box in one
    entry (one self message), at buffer offset bshift."""
    send, recv = periodic_cube(N, H, geo.spatial)
    return [Ent(geo, 0, send, 0, bshift)], [Ent(geo, 0, recv)]


def grid_entries(parts, n, H, periodic, geo_of):
    """Domains of n^3 on a parts grid, all on one rank: field slot = domain, one buffer per
    (sender, receiver) pair, entries in (domain, remote id) order. geo_of(domain) -> Geo."""
    px, py, pz = parts
    doms = []
    for r in range(px * py * pz):
        c = (r % px, (r // px) % py, r // (px * py))
        doms.append((r, tuple(c[d] * n for d in range(3)), tuple((c[d] + 1) * n - 1 for d in range(3))))
    glast = (px * n - 1, py * n - 1, pz * n - 1)
    contrib, zero, pair = [], [], {}
    for d, (send, recv) in enumerate(pattern_boxes(doms, (0, 0, 0), glast, H, periodic)):
        for rid, bx in send:
            contrib.append(Ent(geo_of(d), d, bx, pair.setdefault((d, rid), len(pair)), 0))
        for rid, bx in recv:
            zero.append(Ent(geo_of(d), d, bx))
    return contrib, zero


def census(ents, slot):
    """{number of boxes holding a cell: cells} over the spatial cells of a slot's entries."""
    count = {}
    for en in ents:
        if en.slot != slot:
            continue
        g = Geo(en.geo.ext, en.geo.offs, 1, tuple(range(en.geo.spatial)))
        for f, l in en.boxes:
            for i in g.box_index(f, l):
                count[int(i)] = count.get(int(i), 0) + 1
    out = {}
    for v in count.values():
        out[v] = out.get(v, 0) + 1
    return out
