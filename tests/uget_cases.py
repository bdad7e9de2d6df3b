"""Shared set-up of the index-list get-accumulate tests (ghx_uaccum_get_create, k_accum_get_u,
ghx_uexchange_adjoint_self_*), on tests/uaccum_cases.py.

The definition with field sources. Contribution entry e with a source reads, in place of its
buffer, position i of the source entry's list where it would read position i of its message: the
message is the source list's cells of the source field AS THEY WERE BEFORE THE LAUNCH, element
(i, l) at source.lids[i]*index_stride + l*level_stride of the source's own descriptor. With the
messages gathered so, the operation is uaccum_cases.definition: adds in ascending (entry,
position) and then, with zero_halos, zero bytes over every cell of the zero entries (a source
entry is one of them; without zero_halos a source keeps its values like every other halo cell).

Works without a device (the plans can be described, not executed)."""
from __future__ import annotations

import ctypes

import numpy as np

from tests import uaccum_cases as UA
from tests import uself_cases as US
from tests.uput_cases import Side


def c_sources(sources):
    """(pointer array, kept entries) over a list of Side or None, one per contribution entry."""
    from ghex_amd import _ghx
    real = [s for s in sources if s is not None]
    arr = US.entries(real, [(0, 0)] * len(real))
    ptrs = (ctypes.POINTER(_ghx.UPackEntry) * max(1, len(sources)))()
    k = 0
    for i, s in enumerate(sources):
        if s is not None:
            ptrs[i] = ctypes.pointer(arr[k])
            k += 1
    return ptrs, arr


def try_create(contrib, dtypes, places, sources, zero=()):
    """(return code, last error, handle) of ghx_uaccum_get_create over lists of Side; places[e]
    is the (buffer slot, offset) of entry e, looked at only where sources[e] is None."""
    from ghex_amd import _ghx
    L = _ghx.lib()
    h = ctypes.c_void_p()
    ptrs, keep = c_sources(list(sources))
    rc = L.ghx_uaccum_get_create(US.entries(contrib, places), _ghx.i32_array(list(dtypes)), ptrs, len(contrib),
                                 US.entries(zero, [(0, 0)] * len(zero)), len(zero), ctypes.byref(h))
    del keep
    return rc, (L.ghx_last_error() or b"").decode(), h


def create(contrib, dtypes, places, sources, zero=()):
    rc, why, h = try_create(contrib, dtypes, places, sources, zero)
    assert rc == 0, why
    return h


def kinds(h):
    """[(kind, slot, source lid)] of every contribution record: kind 0 a buffer (lid -1), 1 a
    field source; slot the buffer slot or the source field's slot."""
    from ghex_amd import _ghx
    k, s, l, out = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64(), []
    for j in range(UA.info(h)["n_contrib"]):
        _ghx.call("ghx_uaccum_contrib_kind", h, j, ctypes.byref(k), ctypes.byref(s), ctypes.byref(l))
        out.append((k.value, s.value, l.value))
    return out


def tables(contrib, dtypes, places, sources, zero=()):
    """(info, destinations, records, kinds) of the get plan of the entries."""
    h = create(contrib, dtypes, places, sources, zero)
    try:
        return UA.info(h), UA.dests(h), UA.records(h), kinds(h)
    finally:
        UA.destroy(h)


def gather(fields, bufs, contrib, dtypes, places, sources):
    """The places and buffer images uaccum_cases.definition takes: every sourced entry gets a
    buffer of its own (appended slots) that holds its message in the entry's buffer layout,
    gathered from the source fields' current state."""
    images, out = list(bufs), []
    for e, (en, src) in enumerate(zip(contrib, sources)):
        if src is None:
            out.append(places[e])
            continue
        assert src.lids.size == en.lids.size and src.desc.levels == en.desc.levels
        msg = fields[src.slot][UA.element_index(src)]                 # (n, levels)
        assert msg.dtype == UA.NP[dtypes[e]]
        msg = msg if en.desc.levels_first else msg.T
        images.append(np.ascontiguousarray(msg).reshape(-1).view(np.uint8).copy())
        out.append((len(images) - 1, 0))
    return out, images


def definition(fields, bufs, contrib, dtypes, places, sources, zero, zero_halos=True):
    """The definition on host arrays, in place (fields[slot]: 1-D typed array; bufs[slot]: uint8
    image or None)."""
    where, images = gather(fields, bufs, contrib, dtypes, places, sources)
    return UA.definition(fields, images, contrib, dtypes, where, zero, zero_halos)


def from_tables(fields, bufs, contrib, dtypes, places, sources, dests, recs, knd, zero_halos=True):
    """The operation again, driven by a get plan's own tables: per sum destination its records in
    table order - a buffer record through the message layout, a field-source record through the
    source field's descriptor from the record's lid - every source cell read once and, with
    zero_halos, zeroed; then the zero destinations. Returns (fields, reads per source slot)."""
    start = {k: v.copy() for k, v in fields.items()}
    read = {k: np.zeros(v.size, dtype=np.int32) for k, v in fields.items()}
    desc_of = {s.slot: s.desc for s in list(contrib) + [x for x in sources if x is not None]}
    for d in dests:
        if d.zero:
            continue
        dd = desc_of[d.field_slot]
        idx = d.lid * dd.index_stride + np.arange(dd.levels) * dd.level_stride
        for j in range(d.first, d.first + d.count):
            e, pos = recs[j]
            kind, slot, lid = knd[j]
            dt = UA.NP[dtypes[e]]
            if kind == 0:
                assert sources[e] is None and slot == places[e][0] and lid == -1
                c = UA.message(bufs[slot], contrib[e], places[e][1], dt)[pos]
            else:
                src = sources[e]
                assert src is not None and slot == src.slot and lid == src.lids[pos]
                at = lid * src.desc.index_stride + np.arange(src.desc.levels) * src.desc.level_stride
                read[slot][at] += 1
                c = start[slot][at]
            fields[d.field_slot][idx] = fields[d.field_slot][idx] + c
    for slot, n in read.items():
        assert n.max(initial=0) <= 1                      # every halo cell is read at most once
        if zero_halos:
            fields[slot][n == 1] = 0
    if zero_halos:
        for d in dests:
            if d.zero:
                dd = desc_of[d.field_slot]
                fields[d.field_slot][d.lid * dd.index_stride + np.arange(dd.levels) * dd.level_stride] = 0
    return fields, read


def three_lists(od, hd, seed=0, repeats=False, boff=0, sourced=(True, True, True)):
    """uaccum_cases.three_lists_case with entry e sourced by its halo side where sourced[e]:
    (contrib, zero, places, sources)."""
    contrib, zero, places = UA.three_lists_case(od, hd, seed=seed, repeats=repeats, boff=boff)
    return contrib, zero, places, [z if s else None for z, s in zip(zero, sourced)]


def self_info(plan_h):
    """(form, sum destinations, records, entries with a field source) of an exchange's fused set."""
    from ghex_amd import _ghx
    f = ctypes.c_int32(-1)
    v = [ctypes.c_int64(-1) for _ in range(3)]
    _ghx.call("ghx_uexchange_adjoint_self_info", plan_h, ctypes.byref(f), *[ctypes.byref(x) for x in v])
    return (f.value,) + tuple(x.value for x in v)


def draw_mesh(seed):
    """A small random mesh on ONE rank: two to four domains, each owning 5-90 cells with globally
    unique gids and holding a halo of 1-30 gids owned by the others (one time in three with a gid
    twice: two outer cells of one gid), in a random storage order. Returns [(id, gids, outer lids)]."""
    rng = np.random.default_rng(1000 + seed)
    doms, next_gid = [], 1000
    for i in range(int(rng.integers(2, 5))):
        n = int(rng.integers(5, 91))
        doms.append(list(range(next_gid, next_gid + n)))
        next_gid += n + int(rng.integers(0, 50))
    out = []
    for k, inner in enumerate(doms):
        others = [g for kk, d in enumerate(doms) if kk != k for g in d]
        nh = int(rng.integers(1, min(len(others), 30) + 1))
        halo = [int(g) for g in rng.choice(others, size=nh, replace=False)]
        if rng.random() < 0.3:
            halo.append(halo[0])                      # a repeated halo gid: two outer cells of one gid
        gids = inner + halo
        perm = rng.permutation(len(gids))
        gids = [gids[p] for p in perm]
        outer = sorted(int(np.where(perm == len(inner) + h)[0][0]) for h in range(len(halo)))
        out.append((k, gids, outer))
    return out
