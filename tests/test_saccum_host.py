"""Structured adjoint accumulate plans (ghx_saccum_create, ghx_sexchange_adjoint_create) without a
device: the arrangement of overlapping send boxes into sub-boxes read back through ghx_saccum_box /
ghx_saccum_source and checked against a brute-force census of the same boxes, the known answers of
one periodic domain, the buffer position of every (sub-box cell, source) against the oracle's pack,
a host replay of the tables against the NumPy definition, the transpose identity
<E x, y> = <x, E^T y> with the oracle as E, every refusal with its reason, and the exchange-level
calls."""
import ctypes

import numpy as np
import pytest

from tests import saccum_cases as SA
from tests.saccum_cases import Ent, Geo, cube

F64 = SA.DT_F64


@pytest.fixture(scope="module")
def ghx():
    from ghex_amd import _ghx
    _ghx.lib()
    return _ghx


@pytest.fixture(autouse=True)
def _reset_knobs(ghx):
    yield
    ghx.call("ghx_tune", b"reset", 0)


# ---------------------------------------------------------------------------------------------
# the arrangement
# ---------------------------------------------------------------------------------------------
def _cell_geo(geo):
    """spatial cells of a field as indices: one per cell, whatever the field's layout"""
    return Geo(geo.ext, geo.offs, 1, tuple(range(geo.spatial)))


def assert_arrangement(contrib, subs, srcs):
    """Properties (a)-(e) of the issue and the census, by brute force over cells."""
    total = 0
    for slot in sorted({en.slot for en in contrib}):
        geo = next(en.geo for en in contrib if en.slot == slot)
        cg = _cell_geo(geo)
        holders = {}                                 # cell -> [(entry, box)] ascending
        for e, en in enumerate(contrib):
            if en.slot == slot:
                for b, (f, l) in enumerate(en.boxes):
                    for c in cg.box_index(f, l):
                        holders.setdefault(int(c), []).append((e, b))
        mine = [s for s in subs if s.slot == slot and not s.zero]
        seen = set()
        by_count = {}
        for s in mine:
            lst = [srcs[j][:2] for j in range(s.first_src, s.first_src + s.n_src)]
            assert lst == sorted(lst) and len(set(lst)) == len(lst) and s.n_src >= 1      # (d)
            cells = [int(c) for c in cg.box_index(s.first, s.last)]
            assert not seen.intersection(cells)                                            # (a)
            seen.update(cells)
            for c in cells:                      # (c): inside every box of its list, outside the others
                assert holders[c] == lst, (s, c)
            by_count[s.n_src] = by_count.get(s.n_src, 0) + len(cells)
            for j in range(s.first_src, s.first_src + s.n_src):   # the origin's place in each source
                e, b, bslot, off = srcs[j]
                f, l = contrib[e].boxes[b]
                at = contrib[e].boff + sum(geo.box_bytes(*bx) for bx in contrib[e].boxes[:b])
                st = geo.box_strides(f, l)
                assert bslot == contrib[e].bslot
                assert off == at + sum((s.first[d] - f[d]) * st[d] for d in range(geo.spatial))
        assert seen == set(holders)                                                        # (b)
        assert by_count == SA.census(contrib, slot)
        fast = max(range(geo.spatial), key=lambda d: geo.layout[d])
        for a in mine:                                                                     # (e)
            for b in mine:
                if a is b or a.first[fast] != b.last[fast] + 1:
                    continue
                same = all(a.first[d] == b.first[d] and a.last[d] == b.last[d]
                           for d in range(geo.spatial) if d != fast)
                la = [srcs[j][:2] for j in range(a.first_src, a.first_src + a.n_src)]
                lb = [srcs[j][:2] for j in range(b.first_src, b.first_src + b.n_src)]
                assert not (same and la == lb), (a, b)
        total += len(mine)
    assert total == sum(1 for s in subs if not s.zero)
    first = 0
    for s in subs:                                   # the lists lie one after the other
        if not s.zero:
            assert s.first_src == first
            first += s.n_src
    assert first == len(srcs)


KNOWN = {(6, 2): (26, {1: 6, 3: 12, 7: 8}), (4, 2): (8, {7: 8}), (3, 2): (27, {26: 1, 17: 6, 11: 12, 7: 8}),
         (2, 2): (1, {26: 1})}


@pytest.mark.parametrize("N, H", list(KNOWN))
def test_known_answers_of_one_periodic_domain(ghx, N, H):
    contrib, zero = SA.one_domain_entries(cube(N, H), N, H)
    assert len(contrib[0].boxes) == 26
    i, subs, srcs = SA.tables(contrib, [F64], zero)
    n, by = KNOWN[(N, H)]
    sums = [s for s in subs if not s.zero]
    assert i["n_boxes"] == len(sums) == n and i["n_zero_boxes"] == 26 and i["max_sources"] == max(by)
    got = {}
    for s in sums:
        got[s.n_src] = got.get(s.n_src, 0) + 1
    assert got == by
    if (N, H) == (3, 2):
        assert all(s.first == s.last for s in sums)           # one cell each
    assert i["n_sources"] == sum(k * v for k, v in by.items()) == len(srcs)
    assert_arrangement(contrib, subs, srcs)
    # the census of the issue, from the pattern itself
    want = {(6, 2): {1: 48, 3: 96, 7: 64}, (4, 2): {7: 64}, (3, 2): {7: 8, 11: 12, 17: 6, 26: 1}, (2, 2): {26: 8}}
    assert SA.census(contrib, 0) == want[(N, H)]
    assert i["bytes"] == 8 * sum(k * v for k, v in want[(N, H)].items())


@pytest.mark.parametrize("N, H, want", [(6, 1, {1: 96, 3: 48, 7: 8}), (5, 3, {7: 64, 11: 48, 17: 12, 26: 1})])
def test_arrangement_of_the_other_census_rows(ghx, N, H, want):
    contrib, zero = SA.one_domain_entries(cube(N, H, 4), N, H)
    assert SA.census(contrib, 0) == want
    i, subs, srcs = SA.tables(contrib, [SA.DT_F32], zero)
    assert_arrangement(contrib, subs, srcs)


def test_arrangement_of_four_domains_periodic_and_not(ghx):
    geo = cube(4, 1)
    contrib, zero = SA.grid_entries((2, 2, 1), 4, 1, True, lambda d: geo)
    assert all(SA.census(contrib, d) == {1: 24, 3: 24, 7: 8} for d in range(4))
    i, subs, srcs = SA.tables(contrib, [F64] * len(contrib), zero)
    assert_arrangement(contrib, subs, srcs)
    assert i["max_sources"] == 7 and {s.slot for s in subs} == {0, 1, 2, 3}
    geo = cube(4, 2)
    contrib, zero = SA.grid_entries((2, 2, 1), 4, 2, False, lambda d: geo)
    assert all(len([e for e in contrib if e.slot == d]) == 3 for d in range(4))      # 3 keys each
    assert all(SA.census(contrib, d) == {1: 32, 3: 16} for d in range(4))
    i, subs, srcs = SA.tables(contrib, [F64] * len(contrib), zero)
    assert_arrangement(contrib, subs, srcs)
    assert i["max_sources"] == 3


GEOS = {**{"layout%d%d%d" % lay: cube(5, 2, 8, lay) for lay in SA.LAYOUTS_3D},
        "comp_fastest": cube(5, 2, 4, (2, 1, 0, 3), ncomp=3),
        "comp_slowest": cube(5, 2, 4, (3, 2, 1, 0), ncomp=2),
        "comp_middle": cube(4, 1, 8, (3, 1, 0, 2), ncomp=2),
        "two_d": cube(6, 2, 8, (1, 0), D=2),
        "two_d_y_fastest": cube(5, 2, 4, (0, 1), D=2),
        "strided_fastest": cube(5, 2, 8, (2, 1, 0), fast=2),
        "strided_fastest_f32": cube(4, 2, 4, (0, 1, 2), fast=3)}


def _case(name):
    geo = GEOS[name]
    N = geo.ext[0] - 2 * geo.offs[0]
    contrib, zero = SA.one_domain_entries(geo, N, geo.offs[0], bshift=geo.elem * 3)
    return geo, contrib, zero, [F64 if geo.elem == 8 else SA.DT_F32]


@pytest.mark.parametrize("name", list(GEOS))
def test_arrangement_in_every_layout(ghx, name):
    geo, contrib, zero, dt = _case(name)
    i, subs, srcs = SA.tables(contrib, dt, zero)
    assert_arrangement(contrib, subs, srcs)
    fast = geo.by_speed[0]
    for s in subs:
        assert 1 << s.wlog2 >= geo.elem
        if geo.fast != 1:
            assert s.row_elems == 1                               # a strided fastest dim: one element
        elif fast < geo.spatial:
            assert s.row_elems == s.last[fast] - s.first[fast] + 1
        else:  # components fastest: the runs along the next dim are contiguous in field and buffers
            nxt = geo.by_speed[1]
            assert s.row_elems == geo.ncomp * (s.last[nxt] - s.first[nxt] + 1)


@pytest.mark.parametrize("name", list(GEOS))
def test_every_source_address_holds_its_cell_in_the_oracles_buffer(ghx, name):
    """A field of cell ids packed by the oracle: the address the records give for (sub-box cell,
    source) holds that cell's id."""
    from oracle import oracle as orc
    geo, contrib, zero, dt = _case(name)
    it = np.dtype(np.uint64 if geo.elem == 8 else np.uint32)
    ids = np.arange(geo.n_elems, dtype=it) + 1000
    en = contrib[0]
    buf = np.zeros(en.boff + en.nbytes + 64, dtype=np.uint8)
    pairs = [orc.ISPair(f, l, None, None) for f, l in en.boxes]
    orc.structured_pack(geo.spec(ids), buf, pairs, en.boff, elementwise=geo.fast != 1)
    i, subs, srcs = SA.tables(contrib, dt, zero)
    words = buf[:buf.size // geo.elem * geo.elem].view(it)
    checked = 0
    for s in subs:
        if s.zero:
            continue
        idx = geo.box_index(s.first, s.last)
        for j in range(s.first_src, s.first_src + s.n_src):
            e, b, bslot, off = srcs[j]
            at = SA.source_bytes(geo, s, contrib[e], b, off)
            assert (at % geo.elem == 0).all() and at.max() + geo.elem <= en.boff + en.nbytes
            np.testing.assert_array_equal(words[at // geo.elem], ids[idx])
            checked += idx.size
    assert checked * geo.elem == en.nbytes == i["bytes"]


def _state(rng, geo, code):
    return rng.integers(-50, 51, size=geo.n_elems).astype(SA.NP[code])


@pytest.mark.parametrize("name", ["layout210", "layout012", "comp_fastest", "two_d", "strided_fastest"])
def test_host_replay_of_the_tables_equals_the_definition(ghx, name):
    geo, contrib, zero, dt = _case(name)
    rng = np.random.default_rng(5)
    en = contrib[0]
    F = SA.draw_values(rng, geo.n_elems, dt[0])
    buf = np.zeros(en.boff + en.nbytes, dtype=np.uint8)
    buf[en.boff:] = SA.draw_values(rng, en.nbytes // geo.elem, dt[0]).view(np.uint8)
    i, subs, srcs = SA.tables(contrib, dt, zero)
    got = SA.from_tables({0: F.copy()}, [buf], contrib, dt, subs, srcs)
    for s in subs:
        if s.zero:
            got[0][geo.box_index(s.first, s.last)] = 0
    want = SA.definition({0: F.copy()}, [buf], contrib, dt, zero)
    np.testing.assert_array_equal(got[0].view(np.uint8), want[0].view(np.uint8))
    assert (want[0] != F).any()
    back = SA.definition({0: F.copy()}, [buf], contrib, dt, zero, reverse=True)
    assert (back[0].view(np.uint8) != want[0].view(np.uint8)).any()         # the order is visible


@pytest.mark.parametrize("name", ["layout210", "layout102", "comp_slowest", "two_d_y_fastest"])
def test_transpose_identity_with_the_oracle_as_forward_exchange(ghx, name):
    from oracle import oracle as orc
    geo, contrib, zero, _ = _case(name)
    dt = [F64 if geo.elem == 8 else SA.DT_F32]
    en, ze = contrib[0], zero[0]
    send = [orc.ISPair(f, l, None, None) for f, l in en.boxes]
    recv = [orc.ISPair(f, l, None, None) for f, l in ze.boxes]
    i, subs, srcs = SA.tables(contrib, dt, zero)
    rng = np.random.default_rng(17)

    def forward(x):
        out, buf = x.copy(), np.zeros(en.boff + en.nbytes, dtype=np.uint8)
        orc.structured_pack(geo.spec(x), buf, send, en.boff)
        orc.structured_unpack(geo.spec(out), buf, recv, en.boff)
        return out

    def adjoint(y):
        buf = np.zeros(en.boff + en.nbytes, dtype=np.uint8)
        orc.structured_pack(geo.spec(y), buf, recv, en.boff)      # the reverse pack
        out = SA.from_tables({0: y.copy()}, [buf], contrib, dt, subs, srcs)[0]
        for s in subs:
            if s.zero:
                out[geo.box_index(s.first, s.last)] = 0
        return out

    for _ in range(3):
        x, y = _state(rng, geo, dt[0]), _state(rng, geo, dt[0])
        ex, ety = forward(x), adjoint(y)
        assert float(np.dot(ex.astype(np.float64), y)) == float(np.dot(x.astype(np.float64), ety))
        assert (ety != y).any() and (ex != x).any()


def test_tiles_follow_tile_bytes_in_field_bytes(ghx):
    contrib, zero = SA.one_domain_entries(cube(19, 2), 19, 2)

    def tiles(tb):
        ghx.call("ghx_tune", b"tile_bytes", tb)
        i, subs, _ = SA.tables(contrib, [F64], zero)
        return i["n_tiles"], subs

    n, subs = tiles(8192)
    assert n == len(subs) == 26 + 26                           # every sub-box fits one tile
    # 1-KiB tiles (the knob's smallest): an x face holds 225 rows of 16 B = 3.5 tiles, a z face
    # 30 rows of 120 B: 8 rows a tile, the last tile partial
    n, subs = tiles(1024)
    want = 0
    for s in subs:
        cells = int(np.prod([l - f + 1 for f, l in zip(s.first, s.last)]))
        rows = cells // s.row_elems
        want += -(-rows // max(1, 1024 // (8 * s.row_elems)))
    assert n == want > 52
    x_face = next(s for s in subs if not s.zero and s.n_src == 1 and s.row_elems == 2)
    assert (x_face.last[1] - x_face.first[1] + 1) * (x_face.last[2] - x_face.first[2] + 1) == 225
    # a row longer than a tile is cut in pieces of the tile size
    wide = [Ent(cube(300, 2, D=2), 0, [((0, 0), (299, 1))])]
    ghx.call("ghx_tune", b"tile_bytes", 1024)
    i, subs, _ = SA.tables(wide, [F64])
    assert subs[0].row_elems == 300 and i["n_tiles"] == 2 * 3     # 2400-B rows: 1024 + 1024 + 352


def test_wlog2_is_the_widest_vector_of_rows_offsets_and_strides(ghx):
    g = cube(6, 2)                                                 # E = 10: rows 80 B apart
    one = lambda box, boff=0, geo=g: SA.tables([Ent(geo, 0, [box], 0, boff)], [F64])[1][0].wlog2
    assert one(((0, 0, 0), (1, 3, 3))) == 4                        # 16-B rows at x = 2: offset 16 mod 80
    assert one(((1, 0, 0), (2, 3, 3))) == 3                        # the field offset is 8 mod 16
    assert one(((0, 0, 0), (2, 3, 3))) == 3                        # 24-B rows
    assert one(((0, 0, 0), (1, 3, 3)), boff=8) == 3                # the buffer offset
    assert one(((0, 0, 0), (3, 3, 3)), geo=cube(5, 2)) == 3        # E = 9: 72-B strides
    f32 = cube(6, 2, 4)
    t = lambda box, boff=0: SA.tables([Ent(f32, 0, [box], 0, boff)], [SA.DT_F32])[1][0].wlog2
    assert t(((2, 0, 0), (5, 3, 3))) == 3 and t(((0, 0, 0), (2, 3, 3))) == 2 and t(((2, 0, 0), (5, 3, 3)), 4) == 2
    # a source's buffer strides narrow too: an 8-B wide box beside a 16-B wide one over the same cells
    two = [Ent(g, 0, [((0, 0, 0), (1, 3, 3)), ((0, 0, 0), (2, 3, 3))])]
    subs = SA.tables(two, [F64])[1]
    assert [(s.last[0], s.n_src, s.wlog2) for s in subs] == [(1, 2, 3), (2, 1, 3)]


def test_empty_plans(ghx):
    h = SA.create([], [], [])
    assert SA.info(h) == dict(bytes=0, n_boxes=0, n_zero_boxes=0, n_sources=0, max_sources=0, n_tiles=0)
    assert ghx.lib().ghx_saccum_execute(h, None, 0, None, 0, 1, None) == 0   # nothing to launch
    SA.destroy(h)
    h = SA.create([Ent(cube(4, 1), 0, [])], [F64], [Ent(cube(4, 1), 0, [])])
    assert SA.info(h)["n_tiles"] == 0
    SA.destroy(h)


def test_plans_are_inspected_without_a_device_and_their_execute_checks_its_pointers(ghx):
    import torch
    contrib, zero = SA.one_domain_entries(cube(4, 1), 4, 1)
    h = SA.create(contrib, [F64], zero)
    L = ghx.lib()
    try:
        i = SA.info(h)
        assert i["n_tiles"] > 0
        assert L.ghx_saccum_execute(h, None, 0, None, 0, 1, None) == -1
        assert b"do not cover" in L.ghx_last_error()
        one, odd = ghx.ptr_array([4096]), ghx.ptr_array([4100])
        assert L.ghx_saccum_execute(h, one, 0, one, 1, 1, None) == -1
        assert L.ghx_saccum_execute(h, one, 1, one, 0, 1, None) == -1
        assert L.ghx_saccum_execute(h, odd, 1, one, 1, 1, None) == -1
        assert b"field pointer is not aligned" in L.ghx_last_error()
        assert L.ghx_saccum_execute(h, one, 1, odd, 1, 1, None) == -1
        assert b"buffer pointer is not aligned" in L.ghx_last_error()
        assert L.ghx_saccum_execute(h, ghx.ptr_array([0]), 1, one, 1, 1, None) == -1
        assert b"null field pointer" in L.ghx_last_error()
        if not torch.cuda.is_available():
            assert L.ghx_saccum_execute(h, one, 1, one, 1, 1, None) == -2
            assert b"no device tables" in L.ghx_last_error()
        # indices out of range and null arguments
        assert L.ghx_saccum_box(h, i["n_boxes"] + i["n_zero_boxes"], ctypes.byref(ghx.SAccumBoxInfo())) == -1
        assert L.ghx_saccum_box(h, -1, ctypes.byref(ghx.SAccumBoxInfo())) == -1
        assert L.ghx_saccum_box(h, 0, None) == -1
        assert L.ghx_saccum_source(h, i["n_sources"], None, None, None, None) == -1
        assert L.ghx_saccum_source(h, -1, None, None, None, None) == -1
        assert L.ghx_saccum_source(h, 0, None, None, None, None) == 0
    finally:
        SA.destroy(h)
    hh = ctypes.c_void_p()
    assert L.ghx_saccum_create(None, None, 1, None, 0, ctypes.byref(hh)) == -1
    assert L.ghx_saccum_create(None, None, 0, None, 1, ctypes.byref(hh)) == -1
    assert L.ghx_saccum_create(None, None, 0, None, 0, None) == -1
    assert L.ghx_saccum_info(None, None, None, None, None, None, None) == -1
    assert L.ghx_saccum_execute(None, None, 0, None, 0, 1, None) == -1
    assert L.ghx_saccum_destroy(None) == 0


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def _refused(contrib, dtypes, zero, fragment):
    rc, why, h = SA.try_create(contrib, dtypes, zero)
    assert rc == -1 and not h.value, (rc, why)
    assert fragment in why, why


def test_every_refusal_with_its_reason(ghx):
    g, g4 = cube(4, 1), cube(4, 1, 4)
    box = ((0, 0, 0), (0, 3, 3))
    halo = ((-1, 0, 0), (-1, 3, 3))
    for code in (0, 5, -1, 99):
        _refused([Ent(g, 0, [box])], [code], [], "unknown dtype code")
    _refused([Ent(g, 0, [box])], [SA.DT_F32], [], "elem_size is 8")
    _refused([Ent(g4, 0, [box])], [SA.DT_I64], [], "elem_size is 4")
    _refused([Ent(cube(4, 1, 2), 0, [box])], [SA.DT_I32], [], "elem_size is 2")
    _refused([Ent(g, 0, [box])], [F64], [Ent(cube(4, 1, 2), 1, [halo])], "zero entry's elem_size is 2")
    one = "at most 64 field and 64 buffer slots"
    _refused([Ent(g, 64, [box])], [F64], [], one)
    _refused([Ent(g, 0, [box], 64)], [F64], [], one)
    _refused([Ent(g, 0, [box])], [F64], [Ent(g, 64, [halo])], one)
    _refused([Ent(g, -1, [box])], [F64], [], "negative slot")
    _refused([Ent(g, 0, [box], -1)], [F64], [], "negative slot")
    h = SA.create([Ent(g, 63, [box], 63)], [F64], [Ent(g, 62, [halo], -7)])    # the last slots; zero: buffer ignored
    SA.destroy(h)
    why = "differ in their field descriptor"
    for other in (cube(4, 2), cube(4, 1, 8, (0, 1, 2)), Geo((6, 6, 6), (1, 1, 2), 8, (2, 1, 0)),
                  cube(4, 1, 8, (2, 1, 0), fast=2)):
        _refused([Ent(g, 0, [box]), Ent(other, 0, [box], 1)], [F64, F64], [], why)
        _refused([Ent(g, 0, [box])], [F64], [Ent(other, 0, [halo])], why)
    _refused([Ent(g, 0, [box]), Ent(g, 0, [box], 1)], [F64, SA.DT_I64], [], "differ in their dtype")
    _refused([Ent(g, 0, [box], 0, 4)], [F64], [], "not a multiple of the element size")
    h = SA.create([Ent(g4, 0, [box], 0, 4)], [SA.DT_F32])                       # element-aligned only: fine
    SA.destroy(h)
    _refused([Ent(g, 0, [box])], [F64], [Ent(g, 0, [((0, 3, 3), (1, 4, 4))])],
             "a cell of field slot 0 is both summed and zeroed")
    h = SA.create([Ent(g, 0, [box])], [F64], [Ent(g, 1, [box])])                # another slot
    SA.destroy(h)
    for bad in (((-2, 0, 0), (0, 3, 3)), ((0, 0, 0), (5, 3, 3)), ((0, 0, -2), (0, 3, 3))):
        _refused([Ent(g, 0, [bad])], [F64], [], "outside the field extents")
        _refused([Ent(g, 0, [box])], [F64], [Ent(g, 1, [bad])], "outside the field extents")
    _refused([Ent(g, 0, [((2, 0, 0), (1, 3, 3))])], [F64], [], "first must be <= last")
    # a byte stride that is no multiple of the element
    from ghex_amd import _ghx
    ent = SA.c_entries([Ent(g, 0, [box])])
    ent[0].field.byte_strides[1] += 4
    hh = ctypes.c_void_p()
    L = _ghx.lib()
    assert L.ghx_saccum_create(ent, _ghx.i32_array([F64]), 1, None, 0, ctypes.byref(hh)) == -1
    assert b"byte stride of the field is not a multiple" in L.ghx_last_error()
    ent = SA.c_entries([Ent(g, 0, [box])])
    ent[0].field.layout[0] = 1
    assert L.ghx_saccum_create(ent, _ghx.i32_array([F64]), 1, None, 0, ctypes.byref(hh)) == -1
    assert b"permutation" in L.ghx_last_error()
    ent[0].field.layout[0] = 2
    ent[0].boxes = None
    assert L.ghx_saccum_create(ent, _ghx.i32_array([F64]), 1, None, 0, ctypes.byref(hh)) == -1
    assert b"bad boxes" in L.ghx_last_error()


def test_overlapping_buffer_ranges_are_accepted(ghx):
    g = cube(4, 1)
    box = ((0, 0, 0), (0, 3, 3))
    i, subs, srcs = SA.tables([Ent(g, 0, [box], 0, 0), Ent(g, 1, [box], 0, 8)], [F64, F64])
    assert i["n_sources"] == 2 and [s[3] for s in srcs] == [0, 8]


# ---------------------------------------------------------------------------------------------
# exchanges
# ---------------------------------------------------------------------------------------------
_KEEP = []   # the patterns behind hand-made exchange items


def _exchange_items(ghx, geos, N, H, tag_offset=0):
    """One exchange item per field geometry over one periodic N^3 domain."""
    import ghex_amd
    from ghex_amd.structured import regular as R
    dd = R.DomainDescriptor(0, (0, 0, 0), (N - 1,) * 3)
    pc = R.make_pattern(ghex_amd.make_context(), R.HaloGenerator((0, 0, 0), (N - 1,) * 3, (H,) * 6,
                                                                 (True,) * 3), [dd])
    _KEEP.append(pc)
    items = []
    for g in geos:
        it = ghx.ExchangeItem()
        it.pattern, it.local_index, it.kind, it.field = pc.handle, 0, 0, g.desc()
        it.align, it.tag_offset = g.elem, tag_offset
        items.append(it)
    return items


def _exchange(ghx, geos, N, H):
    from ghex_amd.communication_object import _ExchangePlan
    return _ExchangePlan(_exchange_items(ghx, geos, N, H))


def _adjoint_info(ghx, plan, which="s"):
    r, nb, ns = ctypes.c_int32(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    ghx.call("ghx_%sexchange_adjoint_info" % which, plan.h, ctypes.byref(r), ctypes.byref(nb), ctypes.byref(ns))
    return r.value, nb.value, ns.value


def test_adjoint_plans_of_an_exchange(ghx):
    plan = _exchange(ghx, [cube(6, 2), cube(6, 2, 4)], 6, 2)
    L = ghx.lib()
    assert _adjoint_info(ghx, plan) == (0, 0, 0)
    ptrs = ghx.ptr_array([4096] * 4)
    assert L.ghx_sexchange_adjoint_pack(plan.h, ptrs, 2, ptrs, 1, None) == -1
    assert b"ghx_sexchange_adjoint_create" in L.ghx_last_error()
    assert L.ghx_sexchange_adjoint_accumulate(plan.h, ptrs, 2, ptrs, 1, 1, None) == -1
    assert L.ghx_sexchange_adjoint_create(plan.h, ghx.i32_array([F64]), 1) == -1
    assert b"one dtype code per exchange item" in L.ghx_last_error()
    assert L.ghx_sexchange_adjoint_create(plan.h, None, 2) == -1
    assert L.ghx_sexchange_adjoint_create(plan.h, ghx.i32_array([F64, 7]), 2) == -1
    assert b"unknown dtype code" in L.ghx_last_error()
    assert L.ghx_sexchange_adjoint_create(plan.h, ghx.i32_array([F64, SA.DT_I64]), 2) == -1
    assert b"elem_size is 4" in L.ghx_last_error()
    assert _adjoint_info(ghx, plan) == (0, 0, 0)
    ghx.call("ghx_sexchange_adjoint_create", plan.h, ghx.i32_array([F64, SA.DT_I32]), 2)
    assert _adjoint_info(ghx, plan) == (1, 2 * 26, 2 * (6 + 12 * 3 + 8 * 7))
    assert L.ghx_sexchange_adjoint_pack(plan.h, ptrs, 2, ptrs, len(plan.recv) - 1, None) == -1
    assert b"too few recv buffers" in L.ghx_last_error()
    assert L.ghx_sexchange_adjoint_accumulate(plan.h, ptrs, 2, ptrs, len(plan.send) - 1, 1, None) == -1
    assert b"too few send buffers" in L.ghx_last_error()
    assert L.ghx_sexchange_adjoint_info(None, None, None, None) == -1
    # the unstructured call still refuses a structured exchange, word for word
    assert L.ghx_uexchange_adjoint_create(plan.h, ghx.i32_array([F64, SA.DT_I32]), 2) == -1
    assert (b"adjoint exchange: the exchange holds a structured or cubed-sphere item (their send boxes overlap; "
            b"only index-list items have an adjoint)") == L.ghx_last_error()
    assert _adjoint_info(ghx, plan, "u") == (0, 0, 0)
    # the forward forms report what they reported before
    f = ctypes.c_int32(-1)
    ghx.call("ghx_exchange_self_fusable", plan.h, ctypes.byref(f))
    assert f.value == 1


def test_adjoint_is_refused_while_a_direction_has_parity(ghx):
    plan = _exchange(ghx, [cube(6, 1)], 6, 1)
    n = len(plan.recv)
    word = ctypes.c_uint64(0)
    offsets = (ctypes.c_int64 * n)(*([1 << 20] * n))
    L = ghx.lib()
    ghx.call("ghx_exchange_set_parity", plan.h, 1, ctypes.addressof(word), 0, offsets, n)
    assert L.ghx_sexchange_adjoint_create(plan.h, ghx.i32_array([F64]), 1) == -1
    assert b"double-buffered" in L.ghx_last_error()
    ghx.call("ghx_exchange_set_parity", plan.h, 1, None, 0, None, 0)
    ghx.call("ghx_sexchange_adjoint_create", plan.h, ghx.i32_array([F64]), 1)
    ghx.call("ghx_exchange_set_parity", plan.h, 0, ctypes.addressof(word), 0, offsets, n)
    ptrs = ghx.ptr_array([4096] * 4)
    assert L.ghx_sexchange_adjoint_pack(plan.h, ptrs, 1, ptrs, n, None) == -1
    assert b"double-buffered" in L.ghx_last_error()
    assert L.ghx_sexchange_adjoint_accumulate(plan.h, ptrs, 1, ptrs, n, 1, None) == -1
    assert b"double-buffered" in L.ghx_last_error()
    ghx.call("ghx_exchange_set_parity", plan.h, 0, None, 0, None, 0)


def test_exchanges_with_other_items_have_no_structured_adjoint(ghx, golden_dir):
    from tests.test_uself_host import _known_answer_domains, _plan
    L = ghx.lib()
    plan = _plan(ghx, [_known_answer_domains(golden_dir)], 0)          # index lists only
    assert L.ghx_sexchange_adjoint_create(plan.h, ghx.i32_array([F64] * 4), 4) == -1
    assert b"holds an unstructured item" in L.ghx_last_error()
    assert _adjoint_info(ghx, plan) == (0, 0, 0)
    # a cubed-sphere exchange
    from tests import cs_cases
    from tests.test_cs_self_host import X_FAST, _Exchange
    ex = _Exchange(ghx, cs_cases.config(6), [(X_FAST, 8, 1, 0, 1)])
    try:
        assert L.ghx_sexchange_adjoint_create(ex.h, ghx.i32_array([F64] * ex.n_items), ex.n_items) == -1
        assert b"holds a cubed-sphere item" in L.ghx_last_error()
        assert L.ghx_uexchange_adjoint_create(ex.h, ghx.i32_array([F64] * ex.n_items), ex.n_items) == -1
        assert b"structured or cubed-sphere item" in L.ghx_last_error()
    finally:
        ex.close()
    # structured and unstructured items in one exchange
    plan = _plan(ghx, [_known_answer_domains(golden_dir)], 0, extra=_exchange_items(ghx, [cube(6, 1)], 6, 1, tag_offset=100))
    assert L.ghx_sexchange_adjoint_create(plan.h, ghx.i32_array([F64] * 5), 5) == -1
    assert b"holds an unstructured item" in L.ghx_last_error()


def test_python_option_is_opt_in_and_forwarded(ghx):
    from ghex_amd.communication_object import CommunicationObject
    from ghex_amd.structured import regular as R
    from tests.gpu_util import FakeContext
    ctx = FakeContext(0, 1, [None])
    assert CommunicationObject(ctx).adjoint_boxes is False
    assert R.make_communication_object(ctx, adjoint_boxes=True).adjoint_boxes is True
    for opts in (dict(direct=True), dict(pipelined=True)):
        with pytest.raises(ValueError, match="plain communication object"):
            CommunicationObject(ctx, adjoint_boxes=True, **opts)._adjoint_plan([])
