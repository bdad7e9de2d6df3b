"""Get-accumulate plans (ghx_saccum_get_create, ghx_sexchange_adjoint_self_create) without a device:
the tables beside those of the buffer plan, source offsets and strides against the field
descriptor, the width, the mixed tables of a rank with self and peer messages, every refusal, and
the plans of ghx_saccum_create record by record as they were."""
import ctypes

import numpy as np
import pytest

from tests import saccum_cases as SA
from tests import sget_cases as SG
from tests.saccum_cases import Ent, cube
from tests.test_saccum_host import GEOS

F64 = SA.DT_F64
SHAPES = {(6, 2): 7, (6, 1): 7, (5, 3): 26, (3, 2): 26, (2, 2): 26}


@pytest.fixture(scope="module")
def ghx():
    from ghex_amd import _ghx
    _ghx.lib()
    return _ghx


@pytest.fixture(autouse=True)
def _reset_knobs(ghx):
    yield
    ghx.call("ghx_tune", b"reset", 0)


def _field_offset(geo, cell):
    return sum((cell[d] + geo.offs[d]) * geo.strides[d] for d in range(geo.spatial)) * geo.elem


@pytest.mark.parametrize("N, H", list(SHAPES))
@pytest.mark.parametrize("elem", [8, 4])
def test_tables_of_one_periodic_domain_beside_the_buffer_plan(ghx, N, H, elem):
    geo = cube(N, H, elem)
    code = F64 if elem == 8 else SA.DT_F32
    contrib, sources, zero = SG.one_domain(geo, N, H)
    bi, bsubs, bsrcs = SA.tables(contrib, [code], zero)
    gi, gsubs, gsrcs, knd = SG.tables(contrib, [code], sources, zero)
    # the same sub-boxes with the same lists; no zero tiles: every zero box is a source
    sums = [s for s in bsubs if not s.zero]
    assert gi["n_zero_boxes"] == 0 and bi["n_zero_boxes"] == 26
    assert [(s.first, s.last, s.first_src, s.n_src) for s in gsubs] == [(s.first, s.last, s.first_src, s.n_src)
                                                                        for s in sums]
    assert [s[:2] for s in gsrcs] == [s[:2] for s in bsrcs]
    assert gi["max_sources"] == bi["max_sources"] == SHAPES[(N, H)]
    assert gi["n_boxes"] == bi["n_boxes"] and gi["n_sources"] == bi["n_sources"] and gi["bytes"] == bi["bytes"]
    # every source is a field source of slot 0 at table index 0; its offset is the field offset of
    # the halo cell that pairs with the sub-box's origin
    assert all(k == (1, 0, s[3]) for k, s in zip(knd, gsrcs)) and all(s[2] == 0 for s in gsrcs)
    send, recv = contrib[0].boxes, zero[0].boxes
    for sb in gsubs:
        w = min(_ctz(sb.row_elems * elem), _ctz(_field_offset(geo, sb.first)))
        for j in range(sb.first_src, sb.first_src + sb.n_src):
            e, b, _, off = gsrcs[j]
            cell = tuple(recv[b][0][d] + sb.first[d] - send[b][0][d] for d in range(3))
            assert off == _field_offset(geo, cell)
            w = min(w, _ctz(off))
        # rows stay one box row or less: the y and z strides of both sides are the field's
        rows = int(np.prod([l - f + 1 for f, l in zip(sb.first, sb.last)])) // sb.row_elems
        if rows > 1:
            w = min(w, _ctz(geo.strides[1] * elem))
        assert sb.wlog2 == w, (sb, w)


def _ctz(v, cap=4):
    return next(k for k in range(cap + 1) if k == cap or (v >> k) & 1)


def test_wlog2_is_narrowed_by_the_halo_sides_offsets(ghx):
    g = cube(6, 2)                                                 # E = 10: rows 80 B apart
    box = ((0, 0, 0), (1, 3, 3))                                   # 16-B rows at field offset 16 mod 80

    def one(halo, geo=g):
        return SG.tables([Ent(g, 0, [box])], [F64], [Ent(geo, 1, [halo])])[1][0].wlog2

    assert SA.tables([Ent(g, 0, [box])], [F64])[1][0].wlog2 == 4
    assert one(((6, 0, 0), (7, 3, 3))) == 4                        # x = 8: offset 64
    assert one(((-1, 0, 0), (0, 3, 3))) == 3                       # x = 1: offset 8
    assert one(((4, 0, 0), (5, 3, 3)), cube(5, 2)) == 3            # the source field's 72-B strides
    g4 = cube(6, 1, 4)                                             # E = 8: rows 32 B apart
    t = lambda halo: SG.tables([Ent(g4, 0, [((3, 0, 0), (6, 3, 3))])], [SA.DT_F32], [Ent(g4, 1, [halo])])[1][0].wlog2
    assert t(((-1, 0, 0), (2, 3, 3))) == 4 and t(((1, 0, 0), (4, 3, 3))) == 3 and t(((0, 0, 0), (3, 3, 3))) == 2


def _state(rng, geo, code):
    return rng.integers(-50, 51, size=geo.n_elems).astype(SA.NP[code])


@pytest.mark.parametrize("name", list(GEOS))
def test_host_replay_of_the_tables_equals_the_definition(ghx, name):
    """Offsets AND strides of the field sources: the replay addresses every source cell through the
    source field's descriptor from the record's offset. Every halo cell of a receive box is read
    exactly once, nothing else is."""
    geo = GEOS[name]
    N, H = geo.ext[0] - 2 * geo.offs[0], geo.offs[0]
    code = F64 if geo.elem == 8 else SA.DT_F32
    contrib, sources, zero = SG.one_domain(geo, N, H)
    rng = np.random.default_rng(len(name))
    F = SA.draw_values(rng, geo.n_elems, code)
    i, subs, srcs, knd = SG.tables(contrib, [code], sources, zero)
    for zh in (True, False):
        got, read = SG.from_tables({0: F.copy()}, [], contrib, [code], sources, subs, srcs, knd, zh)
        want = SG.definition({0: F.copy()}, [], contrib, [code], sources, zero, zh)
        np.testing.assert_array_equal(got[0].view(np.uint8), want[0].view(np.uint8))
        halo = np.zeros(geo.n_elems, dtype=np.int32)
        for f, l in zero[0].boxes:
            halo[geo.box_index(f, l)] += 1
        np.testing.assert_array_equal(read[0], halo)
    assert (want[0] != F).any()


def test_a_source_field_of_other_strides_and_a_strided_one(ghx):
    """The pair shares the layout order, not the strides: a source field with another halo width,
    and one whose fastest dimension is strided (rows become single elements)."""
    g = cube(6, 2)
    send = [((0, 0, 0), (1, 5, 5)), ((4, 0, 0), (5, 5, 5))]
    for sg, rows in ((cube(6, 3), 2), (cube(6, 2, fast=2), 1)):
        recv = [((6, 0, 0), (7, 5, 5)), ((-2, 0, 0), (-1, 5, 5))]
        contrib, sources = [Ent(g, 0, send)], [Ent(sg, 1, recv)]
        i, subs, srcs, knd = SG.tables(contrib, [F64], sources, sources)
        assert {s.row_elems for s in subs} == {rows} and i["n_zero_boxes"] == 0
        rng = np.random.default_rng(3)
        F = {0: _state(rng, g, F64), 1: _state(rng, sg, F64)}
        got, _ = SG.from_tables({k: v.copy() for k, v in F.items()}, [], contrib, [F64], sources, subs, srcs, knd)
        want = SG.definition({k: v.copy() for k, v in F.items()}, [], contrib, [F64], sources, sources)
        for k in F:
            np.testing.assert_array_equal(got[k], want[k])
        assert (want[0] != F[0]).any() and (want[1] != F[1]).any()


def test_transpose_identity_with_the_oracle_as_forward_exchange(ghx):
    """Box k of the send list and box k of the receive list are one message: <E x, y> = <x, E^T y>
    with the oracle's pack and unpack as E and the get tables as E^T."""
    from oracle import oracle as orc
    for N, H in ((6, 2), (5, 3), (2, 2)):
        geo = cube(N, H)
        contrib, sources, zero = SG.one_domain(geo, N, H)
        en, ze = contrib[0], zero[0]
        send = [orc.ISPair(f, l, None, None) for f, l in en.boxes]
        recv = [orc.ISPair(f, l, None, None) for f, l in ze.boxes]
        i, subs, srcs, knd = SG.tables(contrib, [F64], sources, zero)
        rng = np.random.default_rng(17 + N)
        for _ in range(2):
            x, y = _state(rng, geo, F64), _state(rng, geo, F64)
            ex, buf = x.copy(), np.zeros(en.nbytes, dtype=np.uint8)
            orc.structured_pack(geo.spec(x), buf, send, 0)
            orc.structured_unpack(geo.spec(ex), buf, recv, 0)
            ety = SG.from_tables({0: y.copy()}, [], contrib, [F64], sources, subs, srcs, knd)[0][0]
            assert float(np.dot(ex, y)) == float(np.dot(x, ety))
            assert (ety != y).any() and (ex != x).any()


# ---------------------------------------------------------------------------------------------
# the mixed tables: (2,1,1) x 4^3, H = 2, periodic, two ranks
# ---------------------------------------------------------------------------------------------
_KEEP = []


def two_rank_plan(ghx, rank, geos, n=4, H=2):
    """The exchange plan of emulated rank `rank` of two, one domain of n^3 each side by side in x,
    one item per field geometry; and the pattern's (send, recv) halos of the domain."""
    from ghex_amd.communication_object import _ExchangePlan
    from ghex_amd.structured import regular as R
    from tests.gpu_util import FakeContext
    doms = [(r, (r * n, 0, 0), ((r + 1) * n - 1, n - 1, n - 1)) for r in range(2)]
    table = {r: [doms[r]] for r in range(2)}
    ctx = FakeContext(rank, 2, table)
    dd = R.DomainDescriptor(*doms[rank])
    pc = R.make_pattern(ctx, R.HaloGenerator((0, 0, 0), (2 * n - 1, n - 1, n - 1), (H,) * 6, (True,) * 3), [dd])
    _KEEP.append(pc)
    items = []
    for g in geos:
        it = ghx.ExchangeItem()
        it.pattern, it.local_index, it.kind, it.field = pc.handle, 0, 0, g.desc()
        it.align, it.tag_offset = g.elem, 0
        items.append(it)
    return _ExchangePlan(items), pc


def _self_info(ghx, plan):
    f = ctypes.c_int32(-1)
    v = [ctypes.c_int64(-1) for _ in range(3)]
    ghx.call("ghx_sexchange_adjoint_self_info", plan.h, ctypes.byref(f), *[ctypes.byref(x) for x in v])
    return (f.value,) + tuple(x.value for x in v)


def mixed_entries(pc, geo, rank):
    """(contrib, sources, zero) of one rank of the two-rank case by hand: the self halos pair, the
    peer halos read a buffer each."""
    contrib, sources, zero = [], [], []
    recv = [(rid, [(tuple(sp[0]), tuple(sp[1])) for sp in spaces]) for rid, _, _, spaces in pc.recv_halos(0)]
    send = [(rid, [(tuple(sp[0]), tuple(sp[1])) for sp in spaces]) for rid, _, _, spaces in pc.send_halos(0)]
    zs = {}
    for rid, bx in recv:
        z = Ent(geo, 0, bx)
        zero.append(z)
        zs.setdefault(rid, []).append(z)
    nb, taken = 0, {}
    for rid, bx in send:
        k = taken.get(rid, 0)
        taken[rid] = k + 1
        contrib.append(Ent(geo, 0, bx, nb, 0))
        sources.append(zs[rid][k] if rid == rank else None)
        nb += 1
    return contrib, sources, zero


def test_mixed_tables_of_two_ranks(ghx):
    geo = cube(4, 2)
    plan, pc = two_rank_plan(ghx, 0, [geo])
    contrib, sources, zero = mixed_entries(pc, geo, 0)
    assert sum(len(e.boxes) for e in contrib) == 26
    assert sum(len(e.boxes) for e, s in zip(contrib, sources) if s is not None) == 8
    i, subs, srcs, knd = SG.tables(contrib, [F64] * len(contrib), sources, zero)
    bi, bsubs, bsrcs = SA.tables(contrib, [F64] * len(contrib), zero)
    # the arrangement is the buffer plan's; the lists ascend across both kinds
    assert [s[:2] for s in srcs] == [s[:2] for s in bsrcs] and i["n_boxes"] == bi["n_boxes"]
    for sb in subs:
        if not sb.zero:
            lst = [srcs[j][:2] for j in range(sb.first_src, sb.first_src + sb.n_src)]
            assert lst == sorted(lst)
    assert {k[0] for k in knd} == {0, 1}
    assert any(len({knd[j][0] for j in range(sb.first_src, sb.first_src + sb.n_src)}) == 2 for sb in subs if not sb.zero)
    for (e, b, tab, off), (kind, slot, _) in zip(srcs, knd):
        assert kind == (1 if sources[e] is not None else 0)
        assert slot == (0 if kind else contrib[e].bslot)
    # the buffers that are read come first in the pointer table, then the source field
    n_bufs = sum(1 for s in sources if s is None)
    assert {s[2] for s, k in zip(srcs, knd) if k[0] == 1} == {n_bufs}
    assert {s[2] for s, k in zip(srcs, knd) if k[0] == 0} == set(range(n_bufs))
    # zero tiles cover exactly the 18 peer boxes
    peer = sorted(bx for z in zero if not any(z is s for s in sources) for bx in z.boxes)
    assert len(peer) == 18 and sorted((s.first, s.last) for s in subs if s.zero) == peer
    # the replay equals the definition with drawn peer messages
    rng = np.random.default_rng(2)
    F = _state(rng, geo, F64)
    bufs = [SA.draw_values(rng, e.nbytes // 8, F64).view(np.uint8) if s is None else None
            for e, s in zip(contrib, sources)]
    got, _ = SG.from_tables({0: F.copy()}, bufs, contrib, [F64] * len(contrib), sources, subs, srcs, knd)
    want = SG.definition({0: F.copy()}, bufs, contrib, [F64] * len(contrib), sources, zero)
    np.testing.assert_array_equal(got[0], want[0])


def test_self_plans_of_an_exchange(ghx):
    L = ghx.lib()
    ptrs = ghx.ptr_array([4096] * 8)
    # mixed: rank 0 of two
    plan, pc = two_rank_plan(ghx, 0, [cube(4, 2), cube(4, 2, 4)])
    assert _self_info(ghx, plan) == (0, 0, 0, 0)
    assert L.ghx_sexchange_adjoint_self_pack(plan.h, ptrs, 2, ptrs, len(plan.recv), None) == -1
    assert b"ghx_sexchange_adjoint_self_create" in L.ghx_last_error()
    assert L.ghx_sexchange_adjoint_self_accumulate(plan.h, ptrs, 2, ptrs, len(plan.send), 1, None) == -1
    assert L.ghx_sexchange_adjoint_self_create(plan.h, ghx.i32_array([F64]), 1) == -1
    assert b"one dtype code per exchange item" in L.ghx_last_error()
    assert L.ghx_sexchange_adjoint_self_create(plan.h, ghx.i32_array([F64, 7]), 2) == -1
    assert b"unknown dtype code" in L.ghx_last_error()
    assert L.ghx_sexchange_adjoint_self_create(plan.h, ghx.i32_array([F64, SA.DT_I64]), 2) == -1
    assert b"elem_size is 4" in L.ghx_last_error()
    ghx.call("ghx_sexchange_adjoint_self_create", plan.h, ghx.i32_array([F64, SA.DT_F32]), 2)
    form, nb, ns, nf = _self_info(ghx, plan)
    contrib, sources, zero = mixed_entries(pc, cube(4, 2), 0)
    i = SA.tables(contrib, [F64] * len(contrib), zero)[0]
    assert (form, nb, ns) == (2, 2 * i["n_boxes"], 2 * i["n_sources"])
    assert nf == 2 * sum(1 for s in sources if s is not None) > 0
    assert L.ghx_sexchange_adjoint_self_pack(plan.h, ptrs, 2, ptrs, len(plan.recv) - 1, None) == -1
    assert b"too few recv buffers" in L.ghx_last_error()
    assert L.ghx_sexchange_adjoint_self_accumulate(plan.h, ptrs, 2, ptrs, len(plan.send) - 1, 1, None) == -1
    assert b"too few send buffers" in L.ghx_last_error()
    # the unfused plans are another pair: untouched by _self_create
    r = ctypes.c_int32(-1)
    ghx.call("ghx_sexchange_adjoint_info", plan.h, ctypes.byref(r), None, None)
    assert r.value == 0
    # all self: one periodic domain
    from tests.test_saccum_host import _exchange
    plan = _exchange(ghx, [cube(6, 2)], 6, 2)
    ghx.call("ghx_sexchange_adjoint_self_create", plan.h, ghx.i32_array([F64]), 1)
    assert _self_info(ghx, plan) == (1, 26, 6 + 12 * 3 + 8 * 7, 1)
    # the pack of an all-self plan launches nothing: OK without a device, whatever the pointers
    ghx.call("ghx_sexchange_adjoint_self_pack", plan.h, ptrs, 1, ptrs, len(plan.recv), None)
    # while a direction has parity set
    n = len(plan.recv)
    word = ctypes.c_uint64(0)
    offsets = (ctypes.c_int64 * n)(*([1 << 20] * n))
    ghx.call("ghx_exchange_set_parity", plan.h, 0, ctypes.addressof(word), 0, offsets, n)
    assert L.ghx_sexchange_adjoint_self_accumulate(plan.h, ptrs, 1, ptrs, n, 1, None) == -1
    assert b"double-buffered" in L.ghx_last_error()
    assert L.ghx_sexchange_adjoint_self_create(plan.h, ghx.i32_array([F64]), 1) == -1
    assert b"double-buffered" in L.ghx_last_error()
    ghx.call("ghx_exchange_set_parity", plan.h, 0, None, 0, None, 0)


def _plain_info(ghx, plan):
    r, nb, ns = ctypes.c_int32(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    ghx.call("ghx_sexchange_adjoint_info", plan.h, ctypes.byref(r), ctypes.byref(nb), ctypes.byref(ns))
    return r.value, nb.value, ns.value


def test_a_refused_create_leaves_the_plans_it_would_have_replaced(ghx):
    """One periodic domain, N = 6, H = 2: the plain adjoint survives two refused creates as it was,
    the fused form is created beside it, and a refused create of that one leaves both."""
    from tests.test_saccum_host import _exchange
    L = ghx.lib()
    plan = _exchange(ghx, [cube(6, 2)], 6, 2)
    ghx.call("ghx_sexchange_adjoint_create", plan.h, ghx.i32_array([F64]), 1)
    plain = _plain_info(ghx, plan)
    assert plain == (1, 26, 6 + 12 * 3 + 8 * 7)
    assert L.ghx_sexchange_adjoint_create(plan.h, ghx.i32_array([7]), 1) == -1
    assert b"unknown dtype code 7" in L.ghx_last_error()
    assert L.ghx_sexchange_adjoint_create(plan.h, ghx.i32_array([F64, F64]), 2) == -1
    assert b"one dtype code per exchange item" in L.ghx_last_error()
    assert _plain_info(ghx, plan) == plain
    assert _self_info(ghx, plan) == (0, 0, 0, 0)
    ghx.call("ghx_sexchange_adjoint_self_create", plan.h, ghx.i32_array([F64]), 1)
    fused = _self_info(ghx, plan)
    assert fused == (1, 26, 6 + 12 * 3 + 8 * 7, 1)
    assert _plain_info(ghx, plan) == plain
    assert L.ghx_sexchange_adjoint_self_create(plan.h, ghx.i32_array([7]), 1) == -1
    assert L.ghx_sexchange_adjoint_self_create(plan.h, ghx.i32_array([F64, F64]), 2) == -1
    assert (_plain_info(ghx, plan), _self_info(ghx, plan)) == (plain, fused)


def test_a_refused_create_leaves_the_cubed_sphere_plans(ghx):
    """The same on the c = 6 cube on one rank, with ghx_cs_exchange_adjoint_create and _self_create."""
    from tests import cs_cases
    from tests import cs_get_cases as G
    ex = G.Exchange(ghx, cs_cases.config(6), G.TWO)
    good = ex.codes()
    try:
        assert ex.create_unfused() == 0, ex.error()
        plain = ex.unfused_info()
        assert plain["ready"] == 1 and plain["boxes"] > 0 and plain["sources"] > 0 and plain["x_records"] > 0
        assert ex.create_unfused([7] + good[1:]) == -1 and "unknown dtype code 7" in ex.error()
        assert ex.create_unfused(good[:-1]) == -1 and "one dtype code per exchange item" in ex.error()
        assert ex.unfused_info() == plain
        assert ex.info()["form"] == 0
        assert ex.create() == 0, ex.error()
        fused = ex.info()
        assert fused["form"] == 1 and (fused["boxes"], fused["sources"]) == (plain["boxes"], plain["sources"])
        assert fused["field_sources"] > 0
        assert ex.unfused_info() == plain
        assert ex.create([7] + good[1:]) == -1 and ex.create(good[:-1]) == -1
        assert (ex.unfused_info(), ex.info()) == (plain, fused)
    finally:
        ex.close()


def test_an_exchange_without_a_self_message_is_refused(ghx):
    """(2,1,1) not periodic: every message of a rank goes to its peer."""
    from ghex_amd.communication_object import _ExchangePlan
    from ghex_amd.structured import regular as R
    from tests.gpu_util import FakeContext
    n, H, geo = 4, 1, cube(4, 1)
    doms = [(r, (r * n, 0, 0), ((r + 1) * n - 1, n - 1, n - 1)) for r in range(2)]
    ctx = FakeContext(0, 2, {r: [doms[r]] for r in range(2)})
    pc = R.make_pattern(ctx, R.HaloGenerator((0, 0, 0), (2 * n - 1, n - 1, n - 1), (H,) * 6, (False,) * 3),
                        [R.DomainDescriptor(*doms[0])])
    _KEEP.append(pc)
    it = ghx.ExchangeItem()
    it.pattern, it.local_index, it.kind, it.field = pc.handle, 0, 0, geo.desc()
    it.align, it.tag_offset = 8, 0
    plan = _ExchangePlan([it])
    L = ghx.lib()
    assert L.ghx_sexchange_adjoint_self_create(plan.h, ghx.i32_array([F64]), 1) == -1
    assert b"no self message" in L.ghx_last_error()
    assert _self_info(ghx, plan) == (0, 0, 0, 0)
    ghx.call("ghx_sexchange_adjoint_create", plan.h, ghx.i32_array([F64]), 1)      # the plain adjoint takes it


def test_exchanges_with_other_items_have_no_fused_adjoint(ghx, golden_dir):
    from tests.test_uself_host import _known_answer_domains, _plan
    L = ghx.lib()
    plan = _plan(ghx, [_known_answer_domains(golden_dir)], 0)
    assert L.ghx_sexchange_adjoint_self_create(plan.h, ghx.i32_array([F64] * 4), 4) == -1
    assert b"holds an unstructured item" in L.ghx_last_error()
    from tests import cs_cases
    from tests.test_cs_self_host import X_FAST, _Exchange
    ex = _Exchange(ghx, cs_cases.config(6), [(X_FAST, 8, 1, 0, 1)])
    try:
        assert L.ghx_sexchange_adjoint_self_create(ex.h, ghx.i32_array([F64] * ex.n_items), ex.n_items) == -1
        assert b"holds a cubed-sphere item" in L.ghx_last_error()
    finally:
        ex.close()


# ---------------------------------------------------------------------------------------------
# refusals of the planner
# ---------------------------------------------------------------------------------------------
def _refused(contrib, dtypes, sources, zero, fragment):
    rc, why, h = SG.try_create(contrib, dtypes, sources, zero)
    assert rc == -1 and not h.value, (rc, why)
    assert fragment in why, why


def test_every_refusal_with_its_reason(ghx):
    g, g4 = cube(4, 1), cube(4, 1, 4)
    box, box2 = ((0, 0, 0), (0, 3, 3)), ((3, 0, 0), (3, 3, 3))
    halo, halo2 = ((4, 0, 0), (4, 3, 3)), ((-1, 0, 0), (-1, 3, 3))
    ok = SG.create([Ent(g, 0, [box, box2])], [F64], [Ent(g, 0, [halo, halo2])], [Ent(g, 0, [halo, halo2])])
    SA.destroy(ok)
    # a pair that differs
    _refused([Ent(g, 0, [box, box2])], [F64], [Ent(g, 0, [halo])], [], "differ in their number of boxes")
    _refused([Ent(g, 0, [box])], [F64], [Ent(g, 0, [((4, 0, 0), (4, 3, 2))])], [], "differ in the extents of box 0")
    _refused([Ent(g, 0, [box])], [F64], [Ent(g, 0, [((5, 0, 0), (5, 3, 3))])], [], "iteration space outside")
    _refused([Ent(g, 0, [box])], [F64], [Ent(cube(4, 2), 1, [((4, 0, 0), (5, 3, 3))])], [], "differ in the extents")
    _refused([Ent(g, 0, [box])], [F64], [Ent(g4, 1, [halo])], [], "differ in elem_size")
    _refused([Ent(g, 0, [box])], [F64], [Ent(cube(4, 1, 8, (2, 1, 0, 3), ncomp=2), 1, [halo])], [],
             "differ in their dimensions or components")
    gc2, gc3 = cube(4, 1, 8, (2, 1, 0, 3), ncomp=2), cube(4, 1, 8, (2, 1, 0, 3), ncomp=3)
    _refused([Ent(gc2, 0, [box])], [F64], [Ent(gc3, 1, [halo])], [], "differ in their dimensions or components")
    _refused([Ent(g, 0, [box])], [F64], [Ent(cube(4, 1, 8, (0, 1, 2)), 1, [halo])], [], "differ in layout order")
    # a source of the slot's own field must have the slot's descriptor
    _refused([Ent(g, 0, [box])], [F64], [Ent(cube(4, 2), 0, [halo])], [], "differ in their field descriptor")
    # source boxes that meet
    _refused([Ent(g, 0, [box, box2])], [F64], [Ent(g, 0, [halo, halo])], [], "two source boxes of field slot 0 meet")
    _refused([Ent(g, 0, [box]), Ent(g, 1, [box], 1)], [F64, F64], [Ent(g, 2, [halo]), Ent(g, 2, [halo])], [],
             "two source boxes of field slot 2 meet")
    # a source box that meets a contribution box or a zero box of the same slot
    _refused([Ent(g, 0, [box])], [F64], [Ent(g, 0, [box])], [], "meets a contribution box")
    _refused([Ent(g, 0, [box, box2])], [F64], [Ent(g, 0, [halo, ((3, 1, 1), (3, 4, 4))])], [],
             "meets a contribution box")
    _refused([Ent(g, 0, [box])], [F64], [Ent(g, 0, [halo])], [Ent(g, 0, [((4, 3, 3), (4, 4, 4))])],
             "meets a zero box")
    _refused([Ent(g, 0, [box])], [F64], [Ent(g, 0, [halo])], [Ent(g, 0, [halo, halo2])], "meets a zero box")
    # more than 64 source slots: 33 buffers and 32 source fields
    g8 = cube(8, 1)
    contrib = [Ent(g8, 0, [((0, k % 8, k // 8), (0, k % 8, k // 8))], k, 0) for k in range(33)]
    contrib += [Ent(g8, 0, [((1, k % 8, k // 8), (1, k % 8, k // 8))], 0, 0) for k in range(32)]
    sources = [None] * 33 + [Ent(g8, 1 + k, [((8, 0, 0), (8, 0, 0))]) for k in range(32)]
    _refused(contrib, [F64] * 65, sources, [], "at most 64 source slots")
    h = SG.create(contrib[1:], [F64] * 64, sources[1:])                        # 32 + 32: the last slot
    assert SA.info(h)["n_sources"] == 64
    SA.destroy(h)
    # every refusal of ghx_saccum_create
    _refused([Ent(g, 0, [box])], [7], [None], [], "unknown dtype code")
    _refused([Ent(g, 0, [box])], [SA.DT_F32], [Ent(g, 0, [halo])], [], "elem_size is 8")
    _refused([Ent(g, 64, [box])], [F64], [Ent(g, 0, [halo])], [], "at most 64 field and 64 buffer slots")
    _refused([Ent(g, 0, [box])], [F64], [Ent(g, 64, [halo])], [], "at most 64 field and 64 buffer slots")
    _refused([Ent(g, 0, [box], 64)], [F64], [None], [], "at most 64 field and 64 buffer slots")
    _refused([Ent(g, 0, [box], -1)], [F64], [None], [], "negative slot")
    _refused([Ent(g, 0, [box])], [F64], [Ent(g, -1, [halo])], [], "negative slot")
    _refused([Ent(g, 0, [box], 0, 4)], [F64], [None], [], "not a multiple of the element size")
    _refused([Ent(g, 0, [box])], [F64], [None], [Ent(g, 0, [((0, 3, 3), (1, 4, 4))])], "both summed and zeroed")
    _refused([Ent(g, 0, [((0, 0, 0), (5, 3, 3))])], [F64], [None], [], "outside the field extents")
    h = SG.create([Ent(g, 0, [box], -5, 4)], [F64], [Ent(g, 0, [halo])])      # a sourced entry: buffer members ignored
    SA.destroy(h)
    L = ghx.lib()
    hh = ctypes.c_void_p()
    ent = SA.c_entries([Ent(g, 0, [box])])
    assert L.ghx_saccum_get_create(ent, ghx.i32_array([F64]), None, 1, None, 0, ctypes.byref(hh)) == -1
    assert b"source" in L.ghx_last_error()


def test_execute_checks_its_plan_and_pointers(ghx):
    L = ghx.lib()
    g = cube(4, 1)
    box, halo = ((0, 0, 0), (0, 3, 3)), ((4, 0, 0), (4, 3, 3))
    get = SG.create([Ent(g, 0, [box])], [F64], [Ent(g, 1, [halo])], [Ent(g, 1, [halo])])
    plain = SA.create([Ent(g, 0, [box])], [F64], [Ent(g, 1, [halo])])
    ptrs = ghx.ptr_array([4096, 8192])
    assert L.ghx_saccum_execute(get, ptrs, 2, ptrs, 1, 1, None) == -1
    assert b"ghx_saccum_get_execute" in L.ghx_last_error()
    assert L.ghx_saccum_get_execute(plain, ptrs, 2, ptrs, 1, 1, None) == -1
    assert b"not a get plan" in L.ghx_last_error()
    assert L.ghx_saccum_get_execute(get, ptrs, 1, None, 0, 1, None) == -1
    assert b"do not cover" in L.ghx_last_error()
    assert L.ghx_saccum_get_execute(get, ghx.ptr_array([4096, 0]), 2, None, 0, 1, None) == -1
    assert b"null field pointer" in L.ghx_last_error()
    assert L.ghx_saccum_get_execute(get, ghx.ptr_array([4096, 8196]), 2, None, 0, 1, None) == -1
    assert b"not aligned" in L.ghx_last_error()
    assert L.ghx_saccum_source_kind(get, 5, None, None, None) == -1
    assert b"out of range" in L.ghx_last_error()
    assert SG.kinds(plain) == [(0, 0, 0)]
    SA.destroy(get)
    SA.destroy(plain)


# ---------------------------------------------------------------------------------------------
# plans of ghx_saccum_create are what they were
# ---------------------------------------------------------------------------------------------
def test_plans_of_saccum_create_keep_their_records(ghx, golden_dir):
    """Every sub-box and source record of ghx_saccum_create's plans against the records the parent
    commit made (tests/golden/saccum_tables.json, written from ghx_saccum_box / _source)."""
    import json
    import os
    with open(os.path.join(golden_dir, "saccum_tables.json")) as fh:
        golden = json.load(fh)
    cases = {}
    for (N, H) in SHAPES:
        for elem, code in ((8, F64), (4, SA.DT_F32)):
            contrib, zero = SA.one_domain_entries(cube(N, H, elem), N, H, bshift=elem * 3)
            cases["cube_%d_%d_%d" % (N, H, elem)] = (contrib, [code], zero)
    for name, geo in GEOS.items():
        N = geo.ext[0] - 2 * geo.offs[0]
        contrib, zero = SA.one_domain_entries(geo, N, geo.offs[0])
        cases["geo_" + name] = (contrib, [F64 if geo.elem == 8 else SA.DT_F32], zero)
    contrib, zero = SA.grid_entries((2, 2, 1), 4, 2, False, lambda d: cube(4, 2))
    cases["grid_221"] = (contrib, [F64] * len(contrib), zero)
    assert set(cases) == set(golden)
    for name, (contrib, dt, zero) in cases.items():
        i, subs, srcs = SA.tables(contrib, dt, zero)
        got = dict(info=i, boxes=[[s.slot, int(s.zero), list(s.first), list(s.last), s.row_elems, s.wlog2,
                                   s.first_src, s.n_src] for s in subs], sources=[list(s) for s in srcs])
        assert got == golden[name], name
