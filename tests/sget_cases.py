"""Shared set-up of the get-accumulate tests (ghx_saccum_get_create, k_accum_get_s,
ghx_sexchange_adjoint_self_*), on tests/saccum_cases.py.

The definition with field sources. Contribution entry e with a source reads, in place of its
buffer, box k of the source entry where it would read box k of its message: the message is the
source box's cells of the source field AS THEY WERE BEFORE THE LAUNCH, in buffer order (dense in
the layout order both sides share, component axis included). With the messages gathered so, the
operation is saccum_cases.definition: adds in ascending (entry, box), then, with zero_halos, zero
bytes over every cell of the zero entries' boxes (a source entry is one of them).

Works without a device (the plans can be described, not executed)."""
from __future__ import annotations

import ctypes

import numpy as np

from tests import saccum_cases as SA
from tests.saccum_cases import Ent, cube  # noqa: F401


def c_sources(sources):
    """(pointer array, kept entries) over a list of Ent or None, one per contribution entry."""
    from ghex_amd import _ghx
    real = [s for s in sources if s is not None]
    arr = SA.c_entries(real)
    ptrs = (ctypes.POINTER(_ghx.PackEntry) * max(1, len(sources)))()
    k = 0
    for i, s in enumerate(sources):
        if s is not None:
            ptrs[i] = ctypes.pointer(arr[k])
            k += 1
    return ptrs, arr


def try_create(contrib, dtypes, sources, zero=()):
    """(return code, last error, handle) of ghx_saccum_get_create over lists of Ent."""
    from ghex_amd import _ghx
    L = _ghx.lib()
    h = ctypes.c_void_p()
    c, z = SA.c_entries(list(contrib)), SA.c_entries(list(zero))
    ptrs, keep = c_sources(list(sources))
    rc = L.ghx_saccum_get_create(c, _ghx.i32_array(list(dtypes)), ptrs, len(contrib), z, len(zero), ctypes.byref(h))
    del keep
    return rc, (L.ghx_last_error() or b"").decode(), h


def create(contrib, dtypes, sources, zero=()):
    rc, why, h = try_create(contrib, dtypes, sources, zero)
    assert rc == 0, why
    return h


def kinds(h):
    """[(kind, slot, offset of the sub-box's origin)] of every source record: kind 0 a buffer,
    1 a field source; slot the buffer slot or the source field's slot."""
    from ghex_amd import _ghx
    k, s, o, out = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64(), []
    for j in range(SA.info(h)["n_sources"]):
        _ghx.call("ghx_saccum_source_kind", h, j, ctypes.byref(k), ctypes.byref(s), ctypes.byref(o))
        out.append((k.value, s.value, o.value))
    return out


def tables(contrib, dtypes, sources, zero=()):
    """(info, sub-boxes, sources, kinds) of the get plan of the entries."""
    h = create(contrib, dtypes, sources, zero)
    try:
        return SA.info(h), SA.boxes(h, contrib[0].geo.spatial), SA.sources(h), kinds(h)
    finally:
        SA.destroy(h)


def gather(fields, bufs, contrib, dtypes, sources):
    """The entries and buffer images saccum_cases.definition takes: every sourced entry gets a
    buffer of its own (appended slots) that holds its message, gathered from the source fields'
    current state in buffer order."""
    images = list(bufs)
    entries = []
    for e, (en, src) in enumerate(zip(contrib, sources)):
        if src is None:
            entries.append(en)
            continue
        assert len(src.boxes) == len(en.boxes)
        msg = [fields[src.slot][src.geo.box_index(f, l)] for f, l in src.boxes]
        msg = np.concatenate(msg) if msg else np.zeros(0, dtype=SA.NP[dtypes[e]])
        assert msg.dtype == SA.NP[dtypes[e]]
        images.append(msg.view(np.uint8).copy())
        entries.append(Ent(en.geo, en.slot, en.boxes, len(images) - 1, 0))
    return entries, images


def definition(fields, bufs, contrib, dtypes, sources, zero, zero_halos=True, reverse=False):
    """The definition on host arrays, in place (fields[slot]: 1-D typed array; bufs[slot]: uint8
    image or None)."""
    entries, images = gather(fields, bufs, contrib, dtypes, sources)
    return SA.definition(fields, images, entries, dtypes, zero, zero_halos, reverse)


def from_tables(fields, bufs, contrib, dtypes, sources, subs, srcs, knd, zero_halos=True):
    """The operation again, driven by a get plan's own tables: per sum sub-box its sources in list
    order — a buffer source through the dense box's strides, a field source through the source
    field's descriptor from the record's offset — every field source cell read once and, with
    zero_halos, zeroed; then the zero sub-boxes."""
    start = {k: v.copy() for k, v in fields.items()}
    read = {k: np.zeros(v.size, dtype=np.int32) for k, v in fields.items()}
    geo_of = {en.slot: en.geo for en in contrib}
    for sb in subs:
        if sb.zero:
            continue
        geo = geo_of[sb.slot]
        idx = geo.box_index(sb.first, sb.last)
        for j in range(sb.first_src, sb.first_src + sb.n_src):
            e, b, _, off = srcs[j]
            kind, slot, off2 = knd[j]
            dt = SA.NP[dtypes[e]]
            assert off == off2
            if kind == 0:
                assert sources[e] is None and slot == contrib[e].bslot
                at = SA.source_bytes(geo, sb, contrib[e], b, off)
                msg = bufs[slot][:bufs[slot].size // dt.itemsize * dt.itemsize].view(dt)[at // dt.itemsize]
            else:
                src = sources[e]
                assert src is not None and slot == src.slot
                sg = src.geo
                at = off + geo.lattice(sb.first, sb.last, [s * sg.elem for s in sg.strides], origin=sb.first)
                assert (at % dt.itemsize == 0).all()
                at = at // dt.itemsize
                read[slot][at] += 1
                msg = start[slot][at]
            fields[sb.slot][idx] = fields[sb.slot][idx] + msg
    for slot, n in read.items():
        assert n.max(initial=0) <= 1                      # every halo cell is read at most once
        if zero_halos:
            fields[slot][n == 1] = 0
    if zero_halos:
        for sb in subs:
            if sb.zero:
                g = geo_of.get(sb.slot) or next(s.geo for s in sources if s is not None and s.slot == sb.slot)
                fields[sb.slot][g.box_index(sb.first, sb.last)] = 0
    return fields, read


def one_domain(geo, N, H):
    """One periodic N^D domain over `geo`, every message a self message: (contrib, sources, zero).
    The send entry is sourced by the receive entry, which is also the zero entry."""
    contrib, zero = SA.one_domain_entries(geo, N, H)
    return contrib, [zero[0]], zero


def grid(parts, n, H, periodic, geo_of):
    """saccum_cases.grid_entries with every message a self message: per (sender, receiver) pair the
    send entry is sourced by the receiver's entry of the boxes it receives from that sender.
    Returns (contrib, sources, zero)."""
    px, py, pz = parts
    doms = []
    for r in range(px * py * pz):
        c = (r % px, (r // px) % py, r // (px * py))
        doms.append((r, tuple(c[d] * n for d in range(3)), tuple((c[d] + 1) * n - 1 for d in range(3))))
    glast = (px * n - 1, py * n - 1, pz * n - 1)
    pats = SA.pattern_boxes(doms, (0, 0, 0), glast, H, periodic)
    contrib, sources, zero, pair = [], [], [], {}
    recv_of = {}                                       # (receiver, sender) -> [entries in pattern order]
    for d, (send, recv) in enumerate(pats):
        for rid, bx in recv:
            z = Ent(geo_of(d), d, bx)
            zero.append(z)
            recv_of.setdefault((d, rid), []).append(z)
    taken = {}
    for d, (send, recv) in enumerate(pats):
        for rid, bx in send:
            k = taken.get((rid, d), 0)
            taken[(rid, d)] = k + 1
            contrib.append(Ent(geo_of(d), d, bx, pair.setdefault((d, rid), len(pair)), 0))
            sources.append(recv_of[(rid, d)][k])
    return contrib, sources, zero
