"""Index-list get-accumulate plans (ghx_uaccum_get_create, ghx_uexchange_adjoint_self_create)
without a device: the planner's tables beside those of ghx_uaccum_create on the same entries,
record kinds and source lids, a host replay of the tables against the definition with field
sources (tests/uget_cases.py), every refusal with its reason, the forms of exchanges built from
the known-answer pattern, and which prefix the Python object takes."""
import ctypes

import numpy as np
import pytest

from tests import uaccum_cases as UA
from tests import uget_cases as UG
from tests import uput_cases as UC
from tests import uself_cases as US
from tests.uput_cases import Side, udesc
from tests.test_uself_host import _known_answer_domains, _plan

F64 = UA.DT_F64
BIG = 1 << 33


@pytest.fixture(scope="module")
def ghx():
    from ghex_amd import _ghx
    _ghx.lib()
    return _ghx


@pytest.fixture(autouse=True)
def _reset_knobs(ghx):
    yield
    ghx.call("ghx_tune", b"reset", 0)


def _plain_tables(contrib, dtypes, places, zero):
    h = UA.create(contrib, dtypes, places, zero)
    try:
        return UA.info(h), UA.dests(h), UA.records(h)
    finally:
        UA.destroy(h)


def _state(rng, sides, code, n_cells=UC.N_CELLS):
    """Typed 1-D fields per slot over the sides' descriptors."""
    return {s.slot: UA.draw_values(rng, UC.span_bytes(s.desc, n_cells) // s.desc.elem_size, code) for s in sides}


def _key(d):
    return (d.field_slot, d.zero, d.lid, d.first, d.count)


# ---------------------------------------------------------------------------------------------
# planner facts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("repeats", [False, True])
@pytest.mark.parametrize("sourced", [(True, True, True), (True, False, True)], ids=["all", "entry1-buffered"])
def test_tables_of_the_three_list_case_beside_the_buffer_plan(ghx, sourced, repeats):
    od, hd = udesc(8, 3), udesc(8, 3, first=False, index_stride=1, level_stride=UC.N_CELLS + 2)
    contrib, zero, places, sources = UG.three_lists(od, hd, seed=3, repeats=repeats, sourced=sourced)
    codes = [F64] * 3
    info, ds, recs, knd = UG.tables(contrib, codes, places, sources, zero)
    pinfo, pds, precs = _plain_tables(contrib, codes, places, zero)
    # the sum destinations, their ranges and the (entry, position) records are the buffer plan's
    sums, psums = [d for d in ds if not d.zero], [d for d in pds if not d.zero]
    assert [_key(d) for d in sums] == [_key(d) for d in psums]
    assert recs == precs and info["n_contrib"] == pinfo["n_contrib"] == 9006
    assert info["max_per_dest"] == pinfo["max_per_dest"] == (287 if repeats else 1)
    if repeats:                          # one cell in two messages: entry 1, then entry 2
        cell = next(d for d in sums if (d.field_slot, d.lid) == (1, int(contrib[1].lids[-1])))
        assert [recs[j][0] for j in range(cell.first, cell.first + cell.count)] == [1, 2]
        assert [knd[j][0] for j in range(cell.first, cell.first + cell.count)] == [1 if sourced[1] else 0, 1]
    # record kinds: a sourced entry's records carry the source slot and the lid at the same position
    for (e, pos), (kind, slot, lid) in zip(recs, knd):
        if sources[e] is None:
            assert (kind, slot, lid) == (0, places[e][0], -1)
        else:
            assert (kind, slot, lid) == (1, sources[e].slot, int(sources[e].lids[pos]))
    # buffer bytes read: the unsourced entries' messages alone
    assert info["bytes"] == sum(US.message_bytes(c) for c, s in zip(contrib, sources) if s is None)
    # sourced zero entries have no zero tiles; the unsourced one keeps its own
    zs = [d for d in ds if d.zero]
    keep = sorted((z.slot, int(l)) for z, s in zip(zero, sources) if s is None for l in z.lids)
    assert [(d.field_slot, d.lid) for d in zs] == keep and info["n_zero_dest"] == len(keep)
    ghx.call("ghx_tune", b"u_tile_rows", 512)
    n_sum = {}
    for d in sums:
        n_sum[d.field_slot] = n_sum.get(d.field_slot, 0) + 1
    want_tiles = sum(-(-n // 512) for n in n_sum.values()) + (-(-len(keep) // 512) if keep else 0)
    assert info["n_tiles"] == want_tiles
    # a host replay of the tables equals the definition, with and without zero_halos
    rng = np.random.default_rng(7)
    for zh in (True, False):
        fields = _state(rng, contrib + zero, F64)
        bufs = [rng.integers(0, 256, size=2 * 9006 * 3 * 8, dtype=np.uint8) for _ in range(2)]
        for b in bufs:       # finite doubles everywhere in the buffers
            b[:] = UA.draw_values(rng, b.size // 8, F64).view(np.uint8)
        want = UG.definition({k: v.copy() for k, v in fields.items()}, bufs, contrib, codes, places, sources, zero, zh)
        got, read = UG.from_tables({k: v.copy() for k, v in fields.items()}, bufs, contrib, codes, places, sources,
                                   ds, recs, knd, zh)
        for k in fields:
            np.testing.assert_array_equal(got[k].view(np.uint8), want[k].view(np.uint8))
        assert sum(int(r.sum()) for r in read.values()) == 3 * sum(c.lids.size for c, s in zip(contrib, sources) if s)


def test_contrib_kind_on_a_plan_of_uaccum_create(ghx):
    contrib, zero, places = UA.three_lists_case(udesc(4), udesc(4), seed=5)
    h = UA.create(contrib, [UA.DT_F32] * 3, places, zero)
    try:
        knd = UG.kinds(h)
        assert knd == [(0, places[e][0], -1) for e, _ in UA.records(h)]
        assert ghx.lib().ghx_uaccum_contrib_kind(h, len(knd), None, None, None) == -1
    finally:
        UA.destroy(h)


@pytest.mark.parametrize("obias, hbias", [(0, BIG), (BIG, 0), (BIG, BIG)])
def test_lids_of_two_to_the_31_and_more_on_either_side(ghx, obias, hbias):
    od, hd = udesc(8, 2), udesc(8, 2, index_stride=3)
    contrib, zero, places, sources = UG.three_lists(od, hd, seed=9, repeats=True)
    big_c = [Side(s.desc, s.slot, s.lids + obias) for s in contrib]
    big_z = [Side(s.desc, s.slot, s.lids + hbias) for s in zero]
    info, ds, recs, knd = UG.tables(big_c, [F64] * 3, places, big_z, big_z)
    _, ds0, recs0, knd0 = UG.tables(contrib, [F64] * 3, places, sources, zero)
    assert recs == recs0 and info["n_zero_dest"] == 0
    assert [(d.field_slot, d.lid - obias, d.first, d.count) for d in ds] == \
           [(d.field_slot, d.lid, d.first, d.count) for d in ds0]
    assert [(k, s, l - hbias) for k, s, l in knd] == knd0
    assert min(l for _, _, l in knd) >= hbias and min(d.lid for d in ds) >= obias


# ---------------------------------------------------------------------------------------------
# refusals of the planner
# ---------------------------------------------------------------------------------------------
def _refused(contrib, dtypes, places, sources, zero, fragment):
    rc, why, h = UG.try_create(contrib, dtypes, places, sources, zero)
    assert rc == -1 and not h.value, (rc, why)
    assert fragment in why, why


def test_every_refusal_of_uaccum_create_holds(ghx):
    lids, hl = np.arange(10), np.arange(20, 30)
    d = udesc(8)
    src = Side(d, 1, hl)
    for code in (0, 5, -1):
        _refused([Side(d, 0, lids)], [code], [(0, 0)], [src], [src], "unknown dtype code")
    _refused([Side(d, 0, lids)], [UA.DT_F32], [(0, 0)], [src], [src], "elem_size is 8")
    _refused([Side(d, 0, lids)], [F64], [(0, 0)], [src], [Side(udesc(2), 2, lids)], "zero entry's elem_size is 2")
    _refused([Side(d, 0, lids), Side(d, 0, lids + 10)], [F64, UA.DT_I64], [(0, 0), (1, 0)], [None, None], [],
             "differ in their dtype")
    _refused([Side(d, -1, lids)], [F64], [(0, 0)], [src], [], "negative slot")
    _refused([Side(d, 0, lids)], [F64], [(-1, 0)], [None], [], "negative slot")
    _refused([Side(d, 0, [3, -1])], [F64], [(0, 0)], [Side(d, 1, [4, 5])], [], "negative local index")
    _refused([Side(d, 0, [3, 4])], [F64], [(0, 0)], [Side(d, 1, [4, -5])], [], "negative local index")
    _refused([Side(udesc(8, 0), 0, lids)], [F64], [(0, 0)], [None], [], "levels < 1")
    _refused([Side(d, 0, lids)], [F64], [(0, 4)], [None], [], "not a multiple of the element size")
    _refused([Side(d, 0, lids)], [F64], [(0, 0)], [None], [Side(d, 0, [12, 9])], "both a sum destination and a zero")
    why = "differ in their data descriptor"
    _refused([Side(udesc(8, 3), 0, lids), Side(udesc(8, 2), 0, lids + 10)], [F64, F64], [(0, 0), (1, 0)],
             [None, None], [], why)
    # a source against another entry of its field slot, of either kind
    _refused([Side(udesc(8, 3), 0, lids), Side(udesc(8, 3), 1, lids)], [F64, F64], [(0, 0), (1, 0)],
             [Side(udesc(8, 3, index_stride=4), 1, hl), None], [], why)
    # the sourced entry's buffer members are not looked at: any slot, any offset
    h = UG.create([Side(d, 0, lids)], [F64], [(-7, 3)], [src], [src])
    assert UA.info(h)["bytes"] == 0
    UA.destroy(h)
    # more records than 32 bits index, before a list is read
    ent = US.entries([Side(udesc(4), 0, lids)], [(0, 0)])
    ent[0].n_lids = 1 << 32
    ptrs, keep = UG.c_sources([None])
    hh = ctypes.c_void_p()
    L = ghx.lib()
    assert L.ghx_uaccum_get_create(ent, ghx.i32_array([UA.DT_I32]), ptrs, 1, None, 0, ctypes.byref(hh)) == -1
    assert b"more than 2^32 - 1 contribution records" in L.ghx_last_error()
    assert L.ghx_uaccum_get_create(ent, ghx.i32_array([UA.DT_I32]), None, 1, None, 0, ctypes.byref(hh)) == -1
    assert L.ghx_uaccum_get_create(None, None, ptrs, 1, None, 0, ctypes.byref(hh)) == -1


def test_an_entry_and_its_source_must_agree(ghx):
    lids, hl = np.arange(10), np.arange(20, 30)
    why = "differ in n_lids, levels or elem_size"
    _refused([Side(udesc(8, 3), 0, lids)], [F64], [(0, 0)], [Side(udesc(8, 3), 1, hl[:9])], [], why)
    _refused([Side(udesc(8, 3), 0, lids)], [F64], [(0, 0)], [Side(udesc(8, 2), 1, hl)], [], why)
    _refused([Side(udesc(8, 3), 0, lids)], [F64], [(0, 0)], [Side(udesc(4, 3), 1, hl)], [], why)
    # strides and the level order may differ
    for hd in (udesc(8, 3, index_stride=7), udesc(8, 3, first=False), udesc(8, 3, index_stride=1, level_stride=99)):
        h = UG.create([Side(udesc(8, 3), 0, lids)], [F64], [(0, 0)], [Side(hd, 1, hl)], [Side(hd, 1, hl)])
        assert UA.info(h)["n_zero_dest"] == 0
        UA.destroy(h)


def test_a_source_cell_has_one_reader_and_nothing_else_touches_it(ghx):
    d = udesc(4, 2)
    own, own2 = np.arange(5), np.arange(5, 10)
    codes = [UA.DT_I32]
    # a lid repeated within a receive list
    _refused([Side(d, 0, own)], codes, [(0, 0)], [Side(d, 1, [20, 21, 22, 21, 23])], [],
             "source cell (field slot 1, lid 21) is read by more than one record")
    # two receive lists of one field slot naming the same cell
    _refused([Side(d, 0, own), Side(d, 0, own2)], codes * 2, [(0, 0), (1, 0)],
             [Side(d, 1, np.arange(20, 25)), Side(d, 1, np.arange(24, 29))], [],
             "source cell (field slot 1, lid 24) is read by more than one record")
    # ... in two slots it is two cells
    h = UG.create([Side(d, 0, own), Side(d, 0, own2)], codes * 2, [(0, 0), (1, 0)],
                  [Side(d, 1, np.arange(20, 25)), Side(d, 2, np.arange(24, 29))], [])
    UA.destroy(h)
    # a source cell that is also a sum destination (one field holds owner and halo cells)
    _refused([Side(d, 0, own)], codes, [(0, 0)], [Side(d, 0, [20, 21, 3, 22, 23])], [],
             "source cell (field slot 0, lid 3) is also a sum destination")
    h = UG.create([Side(d, 0, own)], codes, [(0, 0)], [Side(d, 0, np.arange(20, 25))], [])
    UA.destroy(h)
    # a source cell in a zero entry that is no source
    src = Side(d, 1, np.arange(20, 25))
    _refused([Side(d, 0, own)], codes, [(0, 0)], [src], [src, Side(d, 1, [40, 22])],
             "source cell (field slot 1, lid 22) lies in a zero entry that is no source")
    # the same list in another order is another list: no source, and it holds source cells
    _refused([Side(d, 0, own)], codes, [(0, 0)], [src], [Side(d, 1, np.arange(24, 19, -1))], "is no source")
    # field slots past 64, of the entry and of the source
    one = "at most 64 field and 64 buffer slots"
    _refused([Side(d, 64, own)], codes, [(0, 0)], [src], [], one)
    _refused([Side(d, 0, own)], codes, [(0, 0)], [Side(d, 64, np.arange(20, 25))], [], one)
    _refused([Side(d, 0, own)], codes, [(64, 0)], [None], [], one)
    h = UG.create([Side(d, 63, own)], codes, [(64, 0)], [Side(d, 62, np.arange(20, 25))], [])   # sourced: no buffer
    UA.destroy(h)


def test_execute_checks_its_plan_and_pointers(ghx):
    import torch
    L = ghx.lib()
    contrib, zero, places, sources = UG.three_lists(udesc(4), udesc(4), seed=5, sourced=(True, False, True))
    g = UG.create(contrib, [UA.DT_F32] * 3, places, sources, zero)
    p = UA.create(contrib, [UA.DT_F32] * 3, places, zero)
    four = ghx.ptr_array([4096] * 4)
    try:
        # each execute refuses the other kind of plan, before any device use
        assert L.ghx_uaccum_execute(g, four, 4, four, 2, 1, None) == -1
        assert b"ghx_uaccum_get_execute" in L.ghx_last_error()
        assert L.ghx_uaccum_get_execute(p, four, 4, four, 2, 1, None) == -1
        assert b"ghx_uaccum_execute" in L.ghx_last_error()
        assert L.ghx_uaccum_get_execute(None, four, 4, four, 2, 1, None) == -1
        # the fields of both sides and the buffer of the unsourced entry (slot 0) are needed
        assert L.ghx_uaccum_get_execute(g, four, 3, four, 1, 1, None) == -1
        assert b"do not cover" in L.ghx_last_error()
        assert L.ghx_uaccum_get_execute(g, four, 4, None, 0, 1, None) == -1
        assert b"do not cover" in L.ghx_last_error()
        if not torch.cuda.is_available():
            assert L.ghx_uaccum_get_execute(g, four, 4, four, 1, 1, None) == -2
            assert b"no device tables" in L.ghx_last_error()
        else:
            odd = ghx.ptr_array([4098] * 4)
            assert L.ghx_uaccum_get_execute(g, odd, 4, four, 1, 1, None) == -1
            assert b"not aligned" in L.ghx_last_error()
    finally:
        UA.destroy(g)
        UA.destroy(p)
    # an empty get plan launches nothing
    ptrs, keep = UG.c_sources([])
    h = UG.create([], [], [], [], [])
    assert L.ghx_uaccum_get_execute(h, None, 0, None, 0, 1, None) == 0
    UA.destroy(h)


# ---------------------------------------------------------------------------------------------
# exchanges built from the known-answer pattern
# ---------------------------------------------------------------------------------------------
def _plain_info(ghx, plan):
    r, nd, nc = ctypes.c_int32(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    ghx.call("ghx_uexchange_adjoint_info", plan.h, ctypes.byref(r), ctypes.byref(nd), ctypes.byref(nc))
    return r.value, nd.value, nc.value


def test_forms_of_the_known_answer_exchange(ghx, golden_dir):
    L = ghx.lib()
    doms = _known_answer_domains(golden_dir)
    plan = _plan(ghx, [doms], 0)                                   # four domains on one rank
    assert UG.self_info(plan.h) == (0, 0, 0, 0)
    four = ghx.ptr_array([4096] * 16)
    assert L.ghx_uexchange_adjoint_self_pack(plan.h, four, 4, four, 16, None) == -1
    assert b"ghx_uexchange_adjoint_self_create" in L.ghx_last_error()
    assert L.ghx_uexchange_adjoint_self_accumulate(plan.h, four, 4, four, 16, 1, None) == -1
    ghx.call("ghx_uexchange_adjoint_self_create", plan.h, ghx.i32_array([F64] * 4), 4)
    assert UG.self_info(plan.h) == (1, 12, 15, len(plan.send))    # every message from the halos
    assert _plain_info(ghx, plan) == (0, 0, 0)                    # the plain set is another one
    # form 1: the reverse pack launches nothing, with or without a device
    assert L.ghx_uexchange_adjoint_self_pack(plan.h, four, 4, four, 16, None) == 0
    assert L.ghx_uexchange_adjoint_self_pack(plan.h, four, 4, four, len(plan.recv) - 1, None) == -1
    assert b"too few recv buffers" in L.ghx_last_error()
    assert L.ghx_uexchange_adjoint_self_accumulate(plan.h, four, 4, four, len(plan.send) - 1, 1, None) == -1
    assert b"too few send buffers" in L.ghx_last_error()
    # two emulated ranks: the messages between a rank's two domains are self messages
    for rank in range(2):
        plan = _plan(ghx, [doms[:2], doms[2:]], rank)
        ghx.call("ghx_uexchange_adjoint_create", plan.h, ghx.i32_array([F64] * 2), 2)
        ghx.call("ghx_uexchange_adjoint_self_create", plan.h, ghx.i32_array([F64] * 2), 2)
        form, nd, nc, nfs = UG.self_info(plan.h)
        n_self = sum(1 for x in plan.send if x["rank"] == rank)
        assert form == 2 and 0 < nfs == n_self < len(plan.send)
        assert (1, nd, nc) == _plain_info(ghx, plan)              # the destinations and records of the plain plan


def test_a_refused_create_leaves_the_plain_and_the_fused_set(ghx, golden_dir):
    L = ghx.lib()
    plan = _plan(ghx, [_known_answer_domains(golden_dir)], 0)
    ghx.call("ghx_uexchange_adjoint_create", plan.h, ghx.i32_array([F64] * 4), 4)
    plain = _plain_info(ghx, plan)
    assert plain == (1, 12, 15)
    assert L.ghx_uexchange_adjoint_self_create(plan.h, ghx.i32_array([F64, 7, F64, F64]), 4) == -1
    assert b"unknown dtype code 7" in L.ghx_last_error()
    assert (UG.self_info(plan.h), _plain_info(ghx, plan)) == ((0, 0, 0, 0), plain)
    ghx.call("ghx_uexchange_adjoint_self_create", plan.h, ghx.i32_array([F64] * 4), 4)
    fused = UG.self_info(plan.h)
    assert fused[0] == 1 and fused[1:3] == plain[1:]
    assert L.ghx_uexchange_adjoint_self_create(plan.h, ghx.i32_array([F64] * 3), 3) == -1
    assert b"one dtype code per exchange item" in L.ghx_last_error()
    assert L.ghx_uexchange_adjoint_self_create(plan.h, ghx.i32_array([F64, UA.DT_F32, F64, F64]), 4) == -1
    assert b"elem_size is 8" in L.ghx_last_error()
    assert L.ghx_uexchange_adjoint_create(plan.h, ghx.i32_array([7] * 4), 4) == -1
    assert (UG.self_info(plan.h), _plain_info(ghx, plan)) == (fused, plain)
    four = ghx.ptr_array([4096] * 16)
    assert L.ghx_uexchange_adjoint_self_pack(plan.h, four, 4, four, 16, None) == 0   # still usable


def test_refusals_of_the_exchange_create(ghx, golden_dir):
    L = ghx.lib()
    doms = _known_answer_domains(golden_dir)
    # one domain per rank: no self message
    plan = _plan(ghx, [[d] for d in doms], 1)
    assert L.ghx_uexchange_adjoint_self_create(plan.h, ghx.i32_array([F64]), 1) == -1
    why = L.ghx_last_error()
    assert b"no self message" in why and b"ghx_uexchange_adjoint_create" in why
    assert UG.self_info(plan.h) == (0, 0, 0, 0)
    ghx.call("ghx_uexchange_adjoint_create", plan.h, ghx.i32_array([F64]), 1)        # the plain adjoint takes it
    # double-buffered buffers
    plan = _plan(ghx, [doms], 0)
    n = len(plan.recv)
    word = ctypes.c_uint64(0)
    offsets = (ctypes.c_int64 * n)(*([256] * n))
    ghx.call("ghx_exchange_set_parity", plan.h, 1, ctypes.addressof(word), 0, offsets, n)
    assert L.ghx_uexchange_adjoint_self_create(plan.h, ghx.i32_array([F64] * 4), 4) == -1
    assert b"double-buffered" in L.ghx_last_error()
    ghx.call("ghx_exchange_set_parity", plan.h, 1, None, 0, None, 0)
    ghx.call("ghx_uexchange_adjoint_self_create", plan.h, ghx.i32_array([F64] * 4), 4)
    ghx.call("ghx_exchange_set_parity", plan.h, 0, ctypes.addressof(word), 0, offsets, n)
    ptrs = ghx.ptr_array([4096] * 16)
    assert L.ghx_uexchange_adjoint_self_accumulate(plan.h, ptrs, 4, ptrs, 16, 1, None) == -1
    assert b"double-buffered" in L.ghx_last_error()
    ghx.call("ghx_exchange_set_parity", plan.h, 0, None, 0, None, 0)
    # self messages whose sides do not pair: two items per domain with their level counts swapped
    # between neighbours. The buffers of a domain pair have equal sizes, so they pair as a self
    # message, but the second entry of the two sides lies at different message bytes
    from ghex_amd.communication_object import _ExchangePlan
    from tests.gpu_util import unstructured_patterns
    from tests.test_uself_host import _uitem
    dds, pc = unstructured_patterns([doms])[0]
    items = [_uitem(ghx, pc, pc.local_index(dd.domain_id()), udesc(8, l, n_cells=dd.size()))
             for dd in dds for l in ((3, 1) if dd.domain_id() % 2 == 0 else (1, 3))]
    odd = _ExchangePlan(items)
    odd._keep = (dds, pc)
    assert L.ghx_uexchange_adjoint_self_create(odd.h, ghx.i32_array([F64] * 8), 8) == -1
    assert b"same message bytes" in L.ghx_last_error()
    assert UG.self_info(odd.h) == (0, 0, 0, 0)
    # a structured exchange
    from tests.saccum_cases import cube
    from tests.test_saccum_host import _exchange
    splan = _exchange(ghx, [cube(6, 2)], 6, 2)
    assert L.ghx_uexchange_adjoint_self_create(splan.h, ghx.i32_array([F64]), 1) == -1
    assert b"structured or cubed-sphere item" in L.ghx_last_error()
    # the planner's reasons come through: 65 domains in a ring are 65 field slots
    ring = [(k, [10 * k, 10 * k + 1, 10 * ((k + 1) % 65)], [2]) for k in range(65)]
    plan = _plan(ghx, [ring], 0, levels=1)
    assert L.ghx_uexchange_adjoint_self_create(plan.h, ghx.i32_array([F64] * 65), 65) == -1
    assert b"at most 64 field and 64 buffer slots" in L.ghx_last_error()
    assert UG.self_info(plan.h) == (0, 0, 0, 0)
    # nine domains that all exchange with each other have 72 buffers: the plain adjoint has too many
    # buffer slots, the fused one reads no buffer
    nd = 9
    a2a = [(k, [100 * k + j for j in range(nd)] + [100 * o + k for o in range(nd) if o != k],
            list(range(nd, 2 * nd - 1))) for k in range(nd)]
    plan = _plan(ghx, [a2a], 0, levels=1)
    assert len(plan.send) == 72
    assert L.ghx_uexchange_adjoint_create(plan.h, ghx.i32_array([F64] * nd), nd) == -1
    assert b"at most 64 field and 64 buffer slots" in L.ghx_last_error()
    ghx.call("ghx_uexchange_adjoint_self_create", plan.h, ghx.i32_array([F64] * nd), nd)
    assert UG.self_info(plan.h) == (1, 72, 72, 72)


def test_python_object_takes_the_fused_prefix_only_with_a_self_message_and_fuse_self(golden_dir):
    from ghex_amd.communication_object import CommunicationObject

    class Field:
        kind = 1

    class Info:
        field = Field()

    class Plan:
        def __init__(self, ranks):
            self.recv = [{"rank": r} for r in ranks]

    def prefix(ranks, **kw):
        class Ctx:
            def rank(self):
                return 0
        co = CommunicationObject(Ctx(), **kw)
        co.plan = lambda bis: Plan(ranks)
        co._with_adjoint = lambda bis, prefix: prefix
        return co._adjoint_plan([Info()])

    assert prefix([0, 0], fuse_adjoint_lists=True) == "ghx_uexchange_adjoint_self_"
    assert prefix([1, 0], fuse_adjoint_lists=True) == "ghx_uexchange_adjoint_self_"
    assert prefix([1, 2], fuse_adjoint_lists=True) == "ghx_uexchange_adjoint_"            # no self message
    assert prefix([0, 0], fuse_adjoint_lists=True, fuse_self=False) == "ghx_uexchange_adjoint_"
    assert prefix([0, 0]) == "ghx_uexchange_adjoint_"                                     # opt-in
