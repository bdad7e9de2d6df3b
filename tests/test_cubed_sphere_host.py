"""CPU tests of the cubed-sphere grid (no GPU): the halo generator, make_pattern with the
transforming intersect, domain ids, the device-less planning of rotated receive spaces and the
refusals, all against tests/golden/cubed_sphere_case.json (recorded from the reference's
cubed_sphere/halo_generator.hpp and transform.hpp by tests/golden/make_cubed_sphere_case.py)."""
import ctypes
import types

import pytest

from tests import cs_cases
from tests.gpu_util import FakeContext

EDGES = (10, 6, 70, 8)


@pytest.fixture(scope="module")
def ghx():
    from ghex_amd import _ghx
    _ghx.lib()
    return _ghx


def _cs_domain(ghx, dom, rank=0):
    d = ghx.CsDomain()
    d.rank, d.tile = rank, dom["tile"]
    d.x_first, d.x_last = dom["x"]
    d.y_first, d.y_last = dom["y"]
    return d


def _box6(b):
    return tuple(b.first[:3]) + tuple(b.last[:3])


@pytest.mark.parametrize("edge", EDGES)
def test_halo_boxes_equal_the_reference(ghx, edge):
    cfg = cs_cases.config(edge)
    halos = ghx.i32_array(cfg["halos"])
    for dom in cfg["domains"]:
        d = _cs_domain(ghx, dom)
        n = ctypes.c_int32()
        ghx.call("ghx_cs_halo_boxes", edge, cfg["levels"], ctypes.byref(d), halos, None, None,
                 None, 0, ctypes.byref(n))
        assert n.value == len(dom["boxes"])
        loc, glo = (ghx.Box * n.value)(), (ghx.Box * n.value)()
        til = (ctypes.c_int32 * n.value)()
        ghx.call("ghx_cs_halo_boxes", edge, cfg["levels"], ctypes.byref(d), halos, loc, glo, til,
                 n.value, ctypes.byref(n))
        got = [(_box6(loc[i]), _box6(glo[i]), til[i]) for i in range(n.value)]
        assert got == [(tuple(b["l"]), tuple(b["g"]), b["t"]) for b in dom["boxes"]]


def test_halo_width_order_is_the_codes(ghx):
    """(1, 2, 0, 3) = -x, +x, -y, +y as halo_generator.hpp:111-146 applies them: tile 0 of the
    c = 6 case gets 1 column from -x, 2 from +x, nothing from -y and 3 rows from +y."""
    dom = cs_cases.config(6)["domains"][0]
    width = {}
    for b in dom["boxes"]:
        l = b["l"]
        if l[3] < 0:
            width["-x"] = l[3] - l[0] + 1
        elif l[0] > 5:
            width["+x"] = l[3] - l[0] + 1
        elif l[4] < 0:
            width["-y"] = l[4] - l[1] + 1
        elif l[1] > 5:
            width["+y"] = max(width.get("+y", 0), l[4] - l[1] + 1)
    assert width == {"-x": 1, "+x": 2, "+y": 3}


PLACEMENTS = {"one_rank": lambda i, dom: 0, "six_ranks": lambda i, dom: dom["tile"],
              "three_ranks": lambda i, dom: dom["tile"] // 2}


def _patterns(ghx, cfg, place):
    """Every rank's pattern handle and the rank of every domain."""
    ranks = [place(i, d) for i, d in enumerate(cfg["domains"])]
    # domains ordered by rank, each rank's in fixture order
    order = sorted(range(len(ranks)), key=lambda i: (ranks[i], i))
    arr = (ghx.CsDomain * len(order))(*[_cs_domain(ghx, cfg["domains"][i], ranks[i])
                                        for i in order])
    pats = []
    for r in range(max(ranks) + 1):
        h = ctypes.c_void_p()
        ghx.call("ghx_cs_pattern_create", cfg["edge_size"], cfg["levels"], arr, len(order),
                 ghx.i32_array(cfg["halos"]), r, ctypes.byref(h))
        pats.append(h)
    return pats, ranks, order


def _keys(ghx, h, li, direction):
    n = ctypes.c_int32()
    ghx.call("ghx_pattern_num_keys", h, li, direction, ctypes.byref(n))
    out = []
    for k in range(n.value):
        rid, rr, tag, ns = (ctypes.c_int32() for _ in range(4))
        ne = ctypes.c_int64()
        ghx.call("ghx_pattern_key", h, li, direction, k, ctypes.byref(rid), ctypes.byref(rr),
                 ctypes.byref(tag), ctypes.byref(ns), ctypes.byref(ne))
        loc, glo = (ghx.Box * ns.value)(), (ghx.Box * ns.value)()
        til = (ctypes.c_int32 * ns.value)()
        ghx.call("ghx_pattern_key_boxes", h, li, direction, k, loc, glo, ns.value)
        ghx.call("ghx_pattern_key_tiles", h, li, direction, k, til, ns.value)
        out.append(dict(id=rid.value, rank=rr.value, tag=tag.value, n=ne.value,
                        boxes=[(_box6(loc[i]), _box6(glo[i]), til[i]) for i in range(ns.value)]))
    return out


@pytest.mark.parametrize("placement", sorted(PLACEMENTS))
@pytest.mark.parametrize("edge", EDGES)
def test_patterns_equal_the_reference(ghx, edge, placement):
    cfg = cs_cases.config(edge)
    c, doms = edge, cfg["domains"]
    ids = [cs_cases.domain_id(c, d) for d in doms]
    pats, ranks, order = _patterns(ghx, cfg, PLACEMENTS[placement])
    try:
        recv_tag = {}   # (receiver index, sender index) -> (tag, elements)
        send_seen = {}  # (sender index, receiver index) -> (tag, elements)
        for r, h in enumerate(pats):
            mine = [i for i in order if ranks[i] == r]
            n = ctypes.c_int32()
            ghx.call("ghx_pattern_num_domains", h, ctypes.byref(n))
            assert n.value == len(mine)
            for li, a in enumerate(mine):
                did = ctypes.c_int32()
                ghx.call("ghx_pattern_domain_id", h, li, ctypes.byref(did))
                assert did.value == ids[a]  # the formula, in the rank's domain order
                # receive keys: the fixture's intersections grouped by source domain, in box
                # order, keys in id order
                want = {}
                for b in doms[a]["boxes"]:
                    for x in b["x"]:
                        want.setdefault(x[0], []).append((tuple(x[1:7]), tuple(x[7:13]), b["t"]))
                keys = _keys(ghx, h, li, 1)
                assert [k["id"] for k in keys] == sorted(ids[j] for j in want)
                for k in keys:
                    j = ids.index(k["id"])
                    assert k["rank"] == ranks[j]
                    assert k["boxes"] == want[j]
                    recv_tag[(a, j)] = (k["tag"], k["n"])
                for k in _keys(ghx, h, li, 0):
                    j = ids.index(k["id"])
                    assert k["rank"] == ranks[j]
                    # send boxes: the receiver's intersections with this domain, their global
                    # boxes (this domain's tile coordinates) and the same in local coordinates
                    theirs = [(tuple(x[7:13]), b["t"]) for b in doms[j]["boxes"] for x in b["x"]
                              if x[0] == a]
                    f = (doms[a]["x"][0], doms[a]["y"][0], 0)
                    assert [(g, t) for _, g, t in k["boxes"]] == theirs
                    for l, g, t in k["boxes"]:
                        assert t == doms[a]["tile"]
                        assert l == tuple(g[q] - f[q % 3] for q in range(6))
                    send_seen[(a, j)] = (k["tag"], k["n"])
        # every receive has its send with the same tag and size, and the other way round
        assert {(j, a): v for (a, j), v in recv_tag.items()} == send_seen
        mt = ctypes.c_int32()
        ghx.call("ghx_pattern_max_tag", pats[0], ctypes.byref(mt))
        assert mt.value == max(t for t, _ in recv_tag.values())
    finally:
        for h in pats:
            ghx.lib().ghx_pattern_destroy(h)


# ---------------------------------------------------------------------------------------------
# planning without a device
# ---------------------------------------------------------------------------------------------
C, LEVELS = 8, 4


def _field_desc(ghx, layout, elem=8, nc=1, halo=2):
    """A (x, y, z, k) field of one c = 8 tile with `halo` cells around, memory by `layout`."""
    shape = (C + 2 * halo, C + 2 * halo, LEVELS, nc)
    fd = ghx.FieldDesc()
    fd.dim, fd.elem_size = 4, elem
    stride = elem
    for d in sorted(range(4), key=lambda d: -layout[d]):
        fd.byte_strides[d] = stride
        stride *= shape[d]
    for d in range(4):
        fd.layout[d] = layout[d]
        fd.offsets[d] = halo if d < 2 else 0
        fd.extents[d] = shape[d]
    fd.num_components, fd.has_components = nc, 1
    return fd


class _Exchange:
    """Tile 0's exchange of one field on a cube of one domain per tile, one rank per tile."""

    def __init__(self, ghx, halos, layout, elem=8, nc=1, vector=0, kind=1):
        self.ghx = ghx
        doms = [dict(tile=t, x=(0, C - 1), y=(0, C - 1)) for t in range(6)]
        arr = (ghx.CsDomain * 6)(*[_cs_domain(ghx, d, d["tile"]) for d in doms])
        self.pat = ctypes.c_void_p()
        ghx.call("ghx_cs_pattern_create", C, LEVELS, arr, 6, ghx.i32_array(halos), 0,
                 ctypes.byref(self.pat))
        it = ghx.ExchangeItem()
        it.pattern, it.local_index, it.kind = self.pat, 0, 0
        it.field = _field_desc(ghx, layout, elem, nc, max(max(halos), 1))
        it.align, it.tag_offset = elem, 0
        cs = ghx.CsItem()
        cs.tile, cs.first_x, cs.first_y, cs.edge_size = 0, 0, 0, C
        cs.is_vector, cs.value_kind = vector, kind
        self.item, self.cs = it, cs
        self.h = ctypes.c_void_p()
        self.rc = ghx.lib().ghx_cs_exchange_create(ctypes.byref(it), ctypes.byref(cs), 1,
                                                   ctypes.byref(self.h))
        self.error = ghx.lib().ghx_last_error().decode()

    def info(self):
        n, t, r = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        b = ctypes.c_uint64()
        self.ghx.call("ghx_cs_plan_info", self.h, ctypes.byref(n), ctypes.byref(b),
                      ctypes.byref(t), ctypes.byref(r))
        return dict(records=n.value, bytes=b.value, tiles=t.value, rotated=r.value)

    def close(self):
        if self.h:
            self.ghx.lib().ghx_exchange_destroy(self.h)
        self.ghx.lib().ghx_pattern_destroy(self.pat)


X_FAST, Z_FAST, K_FAST = (3, 2, 1, 0), (1, 2, 3, 0), (0, 1, 2, 3)
# tile 0 (cubed_sphere/transform.hpp:83-87): -x and +y are rotated neighbours, +x and -y
# translation-only ones
ROTATED, TRANSLATED = (2, 0, 0, 2), (0, 2, 2, 0)


def test_translation_only_spaces_are_ordinary(ghx):
    ex = _Exchange(ghx, TRANSLATED, X_FAST)
    try:
        assert ex.rc == 0, ex.error
        assert ex.info() == dict(records=0, bytes=0, tiles=0, rotated=0)
        ghx.call("ghx_exchange_split", ex.h)  # nothing rotates: the per-buffer plans exist
    finally:
        ex.close()


@pytest.mark.parametrize("layout", [Z_FAST, K_FAST])
def test_rotated_scalar_spaces_that_keep_rows_are_ordinary(ghx, layout):
    ex = _Exchange(ghx, ROTATED, layout, nc=1 if layout == Z_FAST else 3)
    try:
        assert ex.rc == 0, ex.error
        assert ex.info() == dict(records=0, bytes=0, tiles=0, rotated=2)
    finally:
        ex.close()


def test_rotated_x_fast_spaces_are_transformed(ghx):
    ex = _Exchange(ghx, ROTATED, X_FAST)
    try:
        assert ex.rc == 0, ex.error
        i = ex.info()
        nbytes = 2 * (C * 2 * LEVELS * 8)
        assert i["records"] == 2 and i["rotated"] == 2 and i["bytes"] == nbytes
        assert i["tiles"] >= 2
        # the ordinary part no longer holds them: the plan's recv buffers still do
        n = ctypes.c_int32()
        ghx.call("ghx_exchange_num_buffers", ex.h, 1, ctypes.byref(n))
        assert n.value == 2
        fus, mix = ctypes.c_int32(1), ctypes.c_int32(1)
        ghx.call("ghx_exchange_self_fusable", ex.h, ctypes.byref(fus))
        ghx.call("ghx_exchange_mixed", ex.h, ctypes.byref(mix))
        assert (fus.value, mix.value) == (0, 0)
    finally:
        ex.close()


def test_vector_field_negation_needs_the_transformed_launch(ghx):
    """z stride-1 keeps rows, but tile 0's -x neighbour negates component 1 and its +y
    neighbour component 0 (transform.hpp:84, 87; field_descriptor.hpp:98-104)."""
    ex = _Exchange(ghx, ROTATED, Z_FAST, elem=4, nc=3, vector=1, kind=1)
    try:
        assert ex.rc == 0, ex.error
        assert ex.info()["records"] == 2
    finally:
        ex.close()
    ex = _Exchange(ghx, TRANSLATED, Z_FAST, elem=4, nc=3, vector=1, kind=1)
    try:
        assert ex.rc == 0, ex.error
        assert ex.info()["records"] == 0
    finally:
        ex.close()


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem,kind", [(1, 1), (2, 2), (8, 0), (16, 1)])
def test_vector_field_of_another_value_type_is_refused(ghx, elem, kind):
    ex = _Exchange(ghx, ROTATED, X_FAST, elem=elem, nc=2, vector=1, kind=kind)
    try:
        assert ex.rc == -1 and "vector field" in ex.error
        assert not ex.h
    finally:
        ex.close()


def test_paths_that_cannot_rotate_refuse(ghx):
    ex = _Exchange(ghx, ROTATED, X_FAST)
    try:
        assert ex.rc == 0, ex.error
        L = ghx.lib()
        assert L.ghx_exchange_split(ex.h) == -1
        assert "rotated" in L.ghx_last_error().decode()
        word = ctypes.c_uint64(0)
        offs = (ctypes.c_int64 * 2)(256 * 4, 256 * 4)
        rc = L.ghx_exchange_set_parity(ex.h, 1, ctypes.addressof(word), 0, offs, 2)
        assert rc == -1 and "rotated" in L.ghx_last_error().decode()
        # the send side has no rotation: its buffers may be double-buffered
        n = ctypes.c_int32()
        ghx.call("ghx_exchange_num_buffers", ex.h, 0, ctypes.byref(n))
        soffs = (ctypes.c_int64 * n.value)(*([1024] * n.value))
        assert L.ghx_exchange_set_parity(ex.h, 0, ctypes.addressof(word), 0, soffs, n.value) == 0
        pl = ctypes.c_void_p()
        rc = L.ghx_pipeline_create(ex.h, 0, 0, ghx.i32_array([]), ghx.ptr_array([]),
                                   ghx.i32_array([]), 4, ctypes.byref(pl))
        assert rc == -1 and not pl
    finally:
        ex.close()


def test_put_of_a_rotated_space_is_refused(ghx):
    """ghx_put_create sees fields and boxes only: the sender's box of a rotated space (tile 4
    sends its +y rows to tile 0's -x columns) and the receiver's differ in shape, which it
    refuses as two sides that do not describe the same bytes."""
    fd = _field_desc(ghx, X_FAST)
    src, dst = ghx.PackEntry(), ghx.PackEntry()
    sb, db = ghx.Box(), ghx.Box()
    sb.first[:3], sb.last[:3] = (0, C - 2, 0), (C - 1, C - 1, LEVELS - 1)   # tile 4's last rows
    db.first[:3], db.last[:3] = (-2, 0, 0), (-1, C - 1, LEVELS - 1)         # tile 0's -x halo
    for e, b in ((src, sb), (dst, db)):
        e.field, e.field_slot, e.buffer_slot, e.buffer_offset = fd, 0, 0, 0
        e.boxes, e.n_boxes = ctypes.pointer(b), 1
    h = ctypes.c_void_p()
    rc = ghx.lib().ghx_put_create(ctypes.byref(src), 1, ctypes.byref(dst), 1, ctypes.byref(h))
    assert rc == -1 and "same" in ghx.lib().ghx_last_error().decode() and not h


def _fake_buffer_info(ghx):
    cs = ghx.CsItem()
    field = types.SimpleNamespace(kind=0, cs_item=cs, desc=ghx.FieldDesc(), align=8,
                                  domain_id=lambda: 0)
    return types.SimpleNamespace(field=field, pattern_container=object(), local_index=0)


def test_python_bulk_direct_and_pipelined_refuse(ghx):
    from ghex_amd.bulk_communication_object import make_bulk_communication_object
    from ghex_amd.communication_object import CommunicationObject
    ctx = FakeContext(0, 1, [None])
    bi = _fake_buffer_info(ghx)
    with pytest.raises(ValueError, match="cubed-sphere"):
        make_bulk_communication_object(ctx).add_field(bi)
    for opts in (dict(direct=True), dict(pipelined=True)):
        with pytest.raises(ValueError, match="cubed-sphere"):
            CommunicationObject(ctx, **opts).plan([bi])
    plain = types.SimpleNamespace(field=types.SimpleNamespace(kind=0, desc=ghx.FieldDesc(),
                                                              align=8),
                                  pattern_container=bi.pattern_container, local_index=0)
    with pytest.raises(ValueError, match="not both"):
        CommunicationObject(ctx).plan([bi, plain])


def test_python_module_mirrors_the_generator(ghx):
    from ghex_amd.structured import cubed_sphere as CS
    cfg = cs_cases.config(6)
    cube = CS.Cube(cfg["edge_size"], cfg["levels"])
    table = [[(cube.edge_size, cube.levels, d["tile"], *d["x"], *d["y"])] for d in cfg["domains"]]
    for r, dom in enumerate(cfg["domains"]):
        dd = CS.DomainDescriptor(cube, dom["tile"], *dom["x"], *dom["y"])
        assert dd.domain_id() == cs_cases.domain_id(6, dom)
        gen = CS.HaloGenerator(cfg["halos"])
        assert gen(dd) == [(tuple(b["l"][:3]), tuple(b["l"][3:]), tuple(b["g"][:3]),
                            tuple(b["g"][3:]), b["t"]) for b in dom["boxes"]]
        pc = CS.make_pattern(FakeContext(r, 6, table), gen, [dd])
        want = {}
        for b in dom["boxes"]:
            for x in b["x"]:
                want.setdefault(cs_cases.domain_id(6, cfg["domains"][x[0]]), []).append(b["t"])
        got = {rid: tiles for (rid, _, _, _), tiles in zip(pc.recv_halos(0), pc.halo_tiles(0, 1))}
        assert got == want


# ---------------------------------------------------------------------------------------------
# tile sizes of the transformed unpack
# ---------------------------------------------------------------------------------------------
def _fixture_exchange(ghx, cfg, layout, elem, nc, vector, kind):
    """(pattern, exchange) of one field per domain of a fixture configuration, all on one rank."""
    pats, _, order = _patterns(ghx, cfg, PLACEMENTS["one_rank"])
    h = max(cfg["halos"]) + 1
    items, cs_items = [], []
    for li, i in enumerate(order):
        dom = cfg["domains"][i]
        shape = (dom["x"][1] - dom["x"][0] + 1 + 2 * h, dom["y"][1] - dom["y"][0] + 1 + 2 * h,
                 cfg["levels"], nc)
        it = ghx.ExchangeItem()
        it.pattern, it.local_index, it.kind, it.align, it.tag_offset = pats[0], li, 0, elem, 0
        fd = it.field
        fd.dim, fd.elem_size, fd.num_components, fd.has_components = 4, elem, nc, 1
        stride = elem
        for d in sorted(range(4), key=lambda d: -layout[d]):
            fd.byte_strides[d] = stride
            stride *= shape[d]
        for d in range(4):
            fd.layout[d], fd.offsets[d], fd.extents[d] = layout[d], (h if d < 2 else 0), shape[d]
        cs = ghx.CsItem()
        cs.tile, cs.first_x, cs.first_y = dom["tile"], dom["x"][0], dom["y"][0]
        cs.edge_size, cs.is_vector, cs.value_kind = cfg["edge_size"], vector, kind
        items.append(it)
        cs_items.append(cs)
    ex = ctypes.c_void_p()
    ghx.call("ghx_cs_exchange_create", (ghx.ExchangeItem * len(items))(*items),
             (ghx.CsItem * len(items))(*cs_items), len(items), ctypes.byref(ex))
    return pats[0], ex


def _rotated_elements(cfg, nc):
    """Elements of every rotated receive space: the recorded intersections of the boxes whose
    image turns a step in x into a step in y'."""
    out = []
    for dom in cfg["domains"]:
        for b in dom["boxes"]:
            if b["t"] != dom["tile"] and b["img"][2] == b["img"][0]:
                for x in b["x"]:
                    out.append((x[4] - x[1] + 1) * (x[5] - x[2] + 1) * (x[6] - x[3] + 1) * nc)
    return out


@pytest.mark.parametrize("edge,elem,nc,vector", [(70, 8, 1, 0), (10, 4, 3, 1)])
def test_x_tile_elems_cuts_the_transformed_records_into_more_or_fewer_tiles(ghx, edge, elem, nc,
                                                                            vector):
    """x_tile_elems 32, 48, 256 (the default) and 4096 on the c = 70 scalar f64 field (1,050
    elements per edge box) and the c = 10 3-vector f32 field (no box above 256 elements): records
    and bytes do not depend on the knob, the tiles cover every record, and their number falls as
    the tile grows. The knob is read when the exchange is created."""
    cfg = cs_cases.config(edge)
    elements = _rotated_elements(cfg, nc)
    seen = {}
    try:
        for T in (256, 32, 48, 4096):
            if T != 256:
                ghx.call("ghx_tune", b"x_tile_elems", T)
            pat, ex = _fixture_exchange(ghx, cfg, X_FAST, elem, nc, vector, 1)
            try:
                n, t, r, b = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64()
                ghx.call("ghx_cs_plan_info", ex, ctypes.byref(n), ctypes.byref(b), ctypes.byref(t),
                         ctypes.byref(r))
            finally:
                ghx.lib().ghx_exchange_destroy(ex)
                ghx.lib().ghx_pattern_destroy(pat)
            seen[T] = t.value
            assert n.value == r.value == len(elements)
            assert b.value == sum(elements) * elem
            assert t.value >= sum(-(-e // T) for e in elements), T
    finally:
        ghx.call("ghx_tune", b"reset", 0)
    assert seen[32] > seen[48] > seen[256] >= seen[4096] == len(elements)
    if edge == 70:
        assert max(elements) == 1050 and seen[256] > seen[4096]
    else:  # one tile per record from 256 elements on
        assert max(elements) <= 256 and seen[256] == seen[4096]
    for bad in (31, 4097, 0):
        assert ghx.lib().ghx_tune(b"x_tile_elems", bad) == -1
