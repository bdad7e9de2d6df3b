"""The fused cubed-sphere adjoint as planned without a device (ghx_cs_exchange_adjoint_self_create,
_info, _plan, _segments, ghx_saccum_source_map): what the get plan counts, where every source record
reads (against the recorded fixture, cell by cell), which rows survive a transform, the 24-domain
cube, form 2's reverse pack, and every refusal with its words."""
import ctypes

import numpy as np
import pytest

from tests import cs_cases
from tests import cs_get_cases as G
from tests.cs_get_cases import F32, F64, I32, I64, K_FAST, TWO, X_FAST, Y_FAST, Z_FAST

# y-, z- and k-fastest fields in one exchange, among them an f64 x 2 vector k-fastest
LAYOUTS = [(Y_FAST, 8, 2, 1, 1), (Z_FAST, 4, 3, 1, 1), (K_FAST, 8, 2, 1, 1), (K_FAST, 4, 2, 1, 2)]


@pytest.fixture(scope="module")
def ghx():
    import ghex_amd
    ghex_amd.native_library()
    from ghex_amd import _ghx
    return _ghx


def test_abi_symbols_resolve(ghx):
    for name in ("create", "info", "plan", "segments", "pack", "accumulate"):
        assert getattr(ghx.lib(), "ghx_cs_exchange_adjoint_self_" + name)
    assert ghx.lib().ghx_saccum_source_map


@pytest.mark.parametrize("edge", [6, 8, 10])
def test_plan_shape_of_a_cube_on_one_rank(ghx, edge):
    """One field per domain: every message is a self message, every send entry has a field source,
    and the arrangement — sub-boxes and source lists — is the unfused plan's."""
    ex = G.Exchange(ghx, cs_cases.config(edge), [(X_FAST, 4, 3, 1, 1)])
    try:
        assert ex.info() == dict(form=0, boxes=0, sources=0, field_sources=0, rotated_sources=0)
        assert ex.create() == 0, ex.error()
        info = ex.info()
        assert info["form"] == 1
        # one field per domain: one send entry per send buffer
        assert info["field_sources"] == ex.buffers(0)
        assert info["rotated_sources"] > 0
        assert ex.segments()[0] == (0, 0)  # form 1 packs nothing
        if edge == 6:
            assert ex.unfused_info()["ready"] == 0  # the unfused plans are left alone
            assert ex.create_unfused() == 0, ex.error()
            un = ex.unfused_info()
            assert (info["boxes"], info["sources"]) == (un["boxes"], un["sources"])
            fused, plain = G.sum_boxes(ghx, ex.plan()), None
            acc = ctypes.c_void_p()
            ghx.call("ghx_cs_exchange_adjoint_plan", ex.h, ctypes.byref(acc))
            plain = G.sum_boxes(ghx, acc)
            assert len(fused) == len(plain)
            for (a, sa), (b, sb) in zip(fused, plain):
                assert (a.field_slot, list(a.first), list(a.last), a.n_src) == (b.field_slot, list(b.first), list(b.last), b.n_src)
                for ja, jb in zip(sa, sb):
                    ea, eb = G.source(ghx, ex.plan(), ja), G.source(ghx, acc, jb)
                    assert (ea["entry"], ea["box"]) == (eb["entry"], eb["box"])
                    assert (ea["kind"], eb["kind"]) == (1, 0)
    finally:
        ex.close()


def _receive_cells(ex, slot):
    """1 on every cell of every receive box of item `slot`, on its whole local array."""
    dom, fd = ex.cfg["domains"][ex.domains[slot]], ex.items[slot].field
    want = np.zeros([fd.extents[d] for d in range(4)], dtype=np.int32)
    for b in dom["boxes"]:
        want[b["l"][0] + fd.offsets[0]:b["l"][3] + fd.offsets[0] + 1,
             b["l"][1] + fd.offsets[1]:b["l"][4] + fd.offsets[1] + 1] += 1
    return want


@pytest.mark.parametrize("edge,specs", [(6, TWO), (6, LAYOUTS), (8, TWO), (8, LAYOUTS), (10, TWO), (10, LAYOUTS[1:3])])
def test_source_records_against_the_fixture(ghx, edge, specs):
    """Every cell of every source record's sub-box reads the halo cell whose recorded image is the
    owner cell, with the recorded sign; over the plan every cell of every receive box is read
    exactly once and no other cell."""
    ex = G.Exchange(ghx, cs_cases.config(edge), specs)
    try:
        assert ex.create() == 0, ex.error()
        reads = G.check_sources(ex)
        assert sorted(reads) == list(range(ex.n_items))  # every domain receives
        for slot, r in reads.items():
            assert np.array_equal(r, _receive_cells(ex, slot)), slot
    finally:
        ex.close()


def test_rows_survive_only_an_untransformed_source(ghx):
    cfg = cs_cases.config(8)
    ex = G.Exchange(ghx, cfg, [(X_FAST, 4, 3, 1, 1), (K_FAST, 8, 2, 1, 1)])
    try:
        assert ex.create() == 0, ex.error()
        acc = ex.plan()
        kept = cut = mixed_sign = 0
        for bx, srcs in G.sum_boxes(ghx, acc):
            recs = [G.source(ghx, acc, j) for j in srcs]
            k_fast = ex.specs[bx.field_slot][0] == K_FAST
            moved = False
            for s in recs:
                own = list(ex.items[s["slot"]].field.byte_strides)[:4]
                moved = moved or s["strides"] != own
            signs = {s["neg"] for s in recs}
            width = bx.last[0] - bx.first[0] + 1
            if not k_fast:
                if moved:  # a transposed or reversed source: every element a row
                    assert bx.row_elems == 1 and bx.wlog2 == 2
                    cut += 1
                else:      # own tile or a translation: whole rows of the x-fastest field, 3 per cell column
                    assert signs == {0} and bx.row_elems >= width
                    kept += bx.row_elems > 1
            elif signs & {1, 2}:
                # the row is the two components and they differ in sign: one f64 per lane
                assert bx.row_elems == 2 and bx.wlog2 == 3
                mixed_sign += 1
            elif not moved:
                assert bx.row_elems >= 2 and bx.wlog2 == 4  # both components in one 16-byte vector
        assert kept > 0 and cut > 0 and mixed_sign > 0
    finally:
        ex.close()


def test_the_24_domain_cube_on_one_rank_has_a_fused_adjoint(ghx):
    two = G.Exchange(ghx, cs_cases.config(10), TWO)
    try:
        assert two.n_items == 48 and two.buffers(0) == 168 > ghx.MAX_SLOTS
        assert two.create_unfused() == -1
        assert "at most 64 field and 64 buffer slots" in two.error()
        assert two.create() == 0, two.error()
        info = two.info()
        assert info["form"] == 1 and info["field_sources"] == 2 * 168
    finally:
        two.close()
    three = G.Exchange(ghx, cs_cases.config(10), TWO + [(X_FAST, 4, 1, 0, 1)])
    try:
        assert three.n_items == 72
        assert three.create() == -1
        assert "at most 64 field and 64 buffer slots" in three.error()
        assert three.info()["form"] == 0
    finally:
        three.close()


def _peer_spaces(ex, placement, rank):
    """(unrotated, rotated) receive spaces of `rank`'s domains whose sender lies on another rank,
    from the recorded intersections; a space is rotated when a step in local x moves the image in y."""
    place, cfg = G.PLACES[placement], ex.cfg
    plain = rotated = 0
    for i, dom in enumerate(cfg["domains"]):
        if place(i, dom) != rank:
            continue
        for b in dom["boxes"]:
            turn = b["t"] != dom["tile"] and b["img"][2] == b["img"][0]
            for x in b["x"]:
                if place(x[0], cfg["domains"][x[0]]) != rank:
                    plain, rotated = plain + (not turn), rotated + turn
    return plain, rotated


@pytest.mark.parametrize("placement,rank", [("six_ranks", 0), ("six_ranks", 3), ("two_ranks", 0), ("two_ranks", 1)])
def test_form_2_packs_the_peer_spaces_alone(ghx, placement, rank):
    """c = 8, two domains per tile: in-tile self messages, cross-tile peers (six ranks), and
    rotated self messages beside rotated peers (two ranks). x-fastest fields: every rotated space is
    a k_pack_x record, every other space one ordinary segment."""
    ex = G.Exchange(ghx, cs_cases.config(8), TWO, placement=placement, rank=rank)
    try:
        assert ex.create() == 0, ex.error()
        assert ex.create_unfused() == 0, ex.error()
        info = ex.info()
        assert info["form"] == 2 and 0 < info["field_sources"] < ex.buffers(0) * len(TWO)
        (seg, xrec), (useg, uxrec) = ex.segments()
        plain, rotated = _peer_spaces(ex, placement, rank)
        assert (seg, xrec) == (plain * len(TWO), rotated * len(TWO))
        assert seg < useg and xrec <= uxrec and seg + xrec < useg + uxrec
        if placement == "two_ranks":
            assert info["rotated_sources"] > 0 and 0 < xrec < uxrec
        reads = G.check_sources(ex)
        assert reads  # the self messages' halos, once each (peer boxes are not read)
        for r in reads.values():
            assert r.max() == 1
    finally:
        ex.close()


def test_refusals(ghx):
    L = ghx.lib()
    ex = G.Exchange(ghx, cs_cases.config(6), TWO)
    good = ex.codes()
    try:
        # before create: both launches are refused without touching their pointer arguments
        for fn in ("pack", "accumulate"):
            args = (ex.h, None, 0, None, 0) + ((1,) if fn == "accumulate" else ()) + (None,)
            assert getattr(L, "ghx_cs_exchange_adjoint_self_" + fn)(*args) == -1
            assert "no plans (ghx_cs_exchange_adjoint_self_create)" in ex.error()
        out = ctypes.c_void_p()
        assert L.ghx_cs_exchange_adjoint_self_plan(ex.h, ctypes.byref(out)) == -1
        for codes, word in [
                (good[:-1], "one dtype code per exchange item"),
                ([0] + good[1:], "unknown dtype code 0"),
                ([5] + good[1:], "unknown dtype code 5"),
                ([F32] + good[1:], "elem_size 8"),
                (good[:6] + [I32] + good[7:], "value_kind 1 but dtype code 3")]:
            assert ex.create(codes) == -1
            assert word in ex.error(), ex.error()
            assert ex.info()["form"] == 0
        assert L.ghx_cs_exchange_adjoint_self_create(ex.h, None, ex.n_items) == -1
        # parity: create and both launches are refused while a direction has it
        n = ex.buffers(0)
        word = ctypes.c_uint64(0)
        offs = (ctypes.c_int64 * n)(*([1 << 20] * n))
        ghx.call("ghx_exchange_set_parity", ex.h, 0, ctypes.addressof(word), 0, offs, n)
        assert ex.create() == -1 and "double-buffered" in ex.error()
        ghx.call("ghx_exchange_set_parity", ex.h, 0, None, 0, offs, n)
        assert ex.create() == 0, ex.error()
        ghx.call("ghx_exchange_set_parity", ex.h, 0, ctypes.addressof(word), 0, offs, n)
        ptrs = ghx.ptr_array([256] * max(n, ex.n_items))
        assert L.ghx_cs_exchange_adjoint_self_pack(ex.h, ptrs, ex.n_items, ptrs, n, None) == -1
        assert "double-buffered" in ex.error()
        assert L.ghx_cs_exchange_adjoint_self_accumulate(ex.h, ptrs, ex.n_items, ptrs, n, 1, None) == -1
        assert "double-buffered" in ex.error()
        ghx.call("ghx_exchange_set_parity", ex.h, 0, None, 0, offs, n)
        # too few buffers
        assert L.ghx_cs_exchange_adjoint_self_pack(ex.h, ptrs, ex.n_items, ptrs, n - 1, None) == -1
        assert "too few recv buffers" in ex.error()
        assert L.ghx_cs_exchange_adjoint_self_accumulate(ex.h, ptrs, ex.n_items, ptrs, n - 1, 1, None) == -1
        assert "too few send buffers" in ex.error()
        # form 1: the pack launches nothing, with or without a device
        assert L.ghx_cs_exchange_adjoint_self_pack(ex.h, ptrs, ex.n_items, ptrs, n, None) == 0
    finally:
        ex.close()


def test_integer_vectors_need_integer_codes(ghx):
    ex = G.Exchange(ghx, cs_cases.config(6), [(X_FAST, 8, 2, 1, 2)])
    try:
        assert ex.create([F64] * ex.n_items) == -1
        assert "value_kind 2 but dtype code 2" in ex.error()
        assert ex.create([I64] * ex.n_items) == 0, ex.error()
    finally:
        ex.close()


def test_an_exchange_without_a_self_message_is_refused(ghx):
    """c = 6 over six ranks, one tile each: every message leaves the rank."""
    ex = G.Exchange(ghx, cs_cases.config(6), TWO, placement="six_ranks")
    try:
        assert ex.create() == -1
        assert "no self message (ghx_cs_exchange_adjoint_create)" in ex.error()
        assert ex.info()["form"] == 0
        assert ex.create_unfused() == 0, ex.error()
    finally:
        ex.close()


def test_other_exchanges_are_refused(ghx, golden_dir):
    from tests.test_saccum_host import _exchange, cube
    from tests.test_uself_host import _known_answer_domains, _plan
    plan = _exchange(ghx, [cube(6, 2)], 6, 2)
    assert ghx.lib().ghx_cs_exchange_adjoint_self_create(plan.h, ghx.i32_array([F64]), 1) == -1
    assert "not a cubed-sphere exchange" in ghx.lib().ghx_last_error().decode()
    f = ctypes.c_int32(-1)
    ghx.call("ghx_cs_exchange_adjoint_self_info", plan.h, ctypes.byref(f), None, None, None, None)
    assert f.value == 0
    lists = _plan(ghx, [_known_answer_domains(golden_dir)], 0)
    assert ghx.lib().ghx_cs_exchange_adjoint_self_create(lists.h, ghx.i32_array([F64] * 4), 4) == -1
    assert "not a cubed-sphere exchange" in ghx.lib().ghx_last_error().decode()


def test_source_map_of_a_buffer_source_and_its_bounds(ghx):
    """ghx_saccum_source_map answers for any plan: a buffer source has its dense box's strides and
    no sign."""
    ex = G.Exchange(ghx, cs_cases.config(6), [(X_FAST, 8, 1, 0, 1)])
    try:
        assert ex.create_unfused() == 0, ex.error()
        acc = ctypes.c_void_p()
        ghx.call("ghx_cs_exchange_adjoint_plan", ex.h, ctypes.byref(acc))
        s = G.source(ghx, acc, 0)
        assert s["kind"] == 0 and s["neg"] == 0 and s["comp"] == 3 and s["strides"][0] == 8
        assert ghx.lib().ghx_saccum_source_map(acc, -1, None, None, None) == -1
        assert ghx.lib().ghx_saccum_source_map(acc, 1 << 40, None, None, None) == -1
    finally:
        ex.close()


def test_python_keyword_needs_adjoint_rotated(ghx):
    from ghex_amd.communication_object import CommunicationObject
    from ghex_amd.structured import cubed_sphere as CS
    from tests.gpu_util import FakeContext
    ctx = FakeContext(0, 1, [None])
    assert CommunicationObject(ctx).fuse_adjoint_rotated is False
    assert CS.make_communication_object(ctx, adjoint_rotated=True).fuse_adjoint_rotated is False
    co = CS.make_communication_object(ctx, adjoint_rotated=True, fuse_adjoint_rotated=True)
    assert co.fuse_adjoint_rotated is True and co.fuse_adjoint is False
    with pytest.raises(ValueError, match="needs adjoint_rotated=True"):
        CommunicationObject(ctx, fuse_adjoint_rotated=True)
    with pytest.raises(ValueError, match="needs adjoint_rotated=True"):
        CS.make_communication_object(ctx, fuse_adjoint_rotated=True)
    with pytest.raises(ValueError, match="needs adjoint_boxes=True"):
        CommunicationObject(ctx, adjoint_rotated=True, fuse_adjoint=True)
