"""The cubed-sphere adjoint exchange as planned without a device (ghx_cs_exchange_adjoint_create,
_info, _plan, _segments): what its plans count, how the accumulate arranges the overlapping send
boxes, and every refusal with its words."""
import ctypes

import numpy as np
import pytest

from tests import cs_cases
from tests.test_cs_self_host import _Exchange

X_FAST, Z_FAST = (3, 2, 1, 0), (1, 2, 3, 0)
F32, F64, I32, I64 = 1, 2, 3, 4
# an fp64 scalar and an f32 3-vector per domain, x stride-1
TWO = [(X_FAST, 8, 1, 0, 1), (X_FAST, 4, 3, 1, 1)]


@pytest.fixture(scope="module")
def ghx():
    import ghex_amd
    ghex_amd.native_library()
    from ghex_amd import _ghx
    return _ghx


def _create(ghx, ex, codes):
    return ghx.lib().ghx_cs_exchange_adjoint_create(ex.h, ghx.i32_array(codes), len(codes))


def _error(ghx):
    return ghx.lib().ghx_last_error().decode()


def _info(ghx, ex):
    r, xr, xt = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    b, s = ctypes.c_int64(-1), ctypes.c_int64(-1)
    ghx.call("ghx_cs_exchange_adjoint_info", ex.h, ctypes.byref(r), ctypes.byref(b), ctypes.byref(s),
             ctypes.byref(xr), ctypes.byref(xt))
    return dict(ready=r.value, boxes=b.value, sources=s.value, x_records=xr.value, x_tiles=xt.value)


def _segments(ghx, ex):
    p, u = ctypes.c_int32(-1), ctypes.c_int32(-1)
    ghx.call("ghx_cs_exchange_adjoint_segments", ex.h, ctypes.byref(p), ctypes.byref(u))
    return p.value, u.value


def _codes(ex, specs, per_spec):
    n = ex.n_items // len(specs)
    return [c for c in per_spec for _ in range(n)]


def test_info_before_create_and_on_another_exchange(ghx):
    ex = _Exchange(ghx, cs_cases.config(6), TWO)
    try:
        assert _info(ghx, ex) == dict(ready=0, boxes=0, sources=0, x_records=0, x_tiles=0)
        assert _segments(ghx, ex)[0] == 0
        out = ctypes.c_void_p()
        assert ghx.lib().ghx_cs_exchange_adjoint_plan(ex.h, ctypes.byref(out)) == -1
        assert "ghx_cs_exchange_adjoint_create" in _error(ghx)
        # both launches are refused before create, without touching their pointer arguments
        for fn in ("ghx_cs_exchange_adjoint_pack", "ghx_cs_exchange_adjoint_accumulate"):
            args = (ex.h, None, 0, None, 0) + ((1,) if fn.endswith("accumulate") else ()) + (None,)
            assert getattr(ghx.lib(), fn)(*args) == -1
            assert "no adjoint plans" in _error(ghx)
    finally:
        ex.close()


def _send_cells(cfg, oi):
    """How many send boxes hold each cell of domain oi's local (x, y) extent, from the recorded
    intersections: a box received by any domain from oi is sent by oi in its own coordinates."""
    od = cfg["domains"][oi]
    nx, ny = od["x"][1] - od["x"][0] + 1, od["y"][1] - od["y"][0] + 1
    n = np.zeros((nx, ny), dtype=np.int32)
    for dom in cfg["domains"]:
        for b in dom["boxes"]:
            for x in b["x"]:
                if x[0] == oi:
                    gf, gl = x[7:10], x[10:13]
                    n[gf[0] - od["x"][0]:gl[0] - od["x"][0] + 1,
                      gf[1] - od["y"][0]:gl[1] - od["y"][0] + 1] += 1
    return n


@pytest.mark.parametrize("edge", [6, 70])
def test_plans_of_a_cube_on_one_rank(ghx, edge):
    """Six whole-tile domains, up to 24 buffers: k_pack_x runs the transformed unpack's own records and
    tiles; the accumulate's sum sub-boxes are pairwise disjoint, cover exactly the send boxes, list
    their sources in ascending (entry, box), and some (the tile corners) have several."""
    cfg = cs_cases.config(edge)
    ex = _Exchange(ghx, cfg, TWO)
    try:
        # one buffer per tile edge with a halo: 24, or 18 under c = 6's halos (1, 2, 0, 3)
        assert ex.num_buffers() == sum(len(d["boxes"]) for d in cfg["domains"]) == (24 if edge == 70 else 18)
        assert _create(ghx, ex, _codes(ex, TWO, [F64, F32])) == 0, _error(ghx)
        info, plan = _info(ghx, ex), ex.plan_info()
        assert info["ready"] == 1 and plan["records"] > 0
        assert (info["x_records"], info["x_tiles"]) == (plan["records"], plan["tiles"])
        pk, un = _segments(ghx, ex)
        assert pk == un > 0
        acc = ctypes.c_void_p()
        ghx.call("ghx_cs_exchange_adjoint_plan", ex.h, ctypes.byref(acc))
        nb, nz, ns = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        ghx.call("ghx_saccum_info", acc, None, ctypes.byref(nb), ctypes.byref(nz), ctypes.byref(ns),
                 None, None)
        assert (nb.value, ns.value) == (info["boxes"], info["sources"]) and nz.value > 0
        n_dom = len(cfg["domains"])
        cover = {}  # field slot -> how many sum sub-boxes hold each local (x, y) cell
        several = 0
        for k in range(nb.value):
            bx = ghx.SAccumBoxInfo()
            ghx.call("ghx_saccum_box", acc, k, ctypes.byref(bx))
            assert bx.zero == 0 and bx.n_src >= 1
            several += bx.n_src > 1
            assert (bx.first[2], bx.last[2]) == (0, cfg["levels"] - 1)
            dom = cfg["domains"][bx.field_slot % n_dom]
            c = cover.setdefault(bx.field_slot, np.zeros(
                (dom["x"][1] - dom["x"][0] + 1, dom["y"][1] - dom["y"][0] + 1), dtype=np.int32))
            c[bx.first[0]:bx.last[0] + 1, bx.first[1]:bx.last[1] + 1] += 1
            prev = (-1, -1)
            for j in range(bx.first_src, bx.first_src + bx.n_src):
                e, b = ctypes.c_int32(), ctypes.c_int32()
                ghx.call("ghx_saccum_source", acc, j, ctypes.byref(e), ctypes.byref(b), None, None)
                assert (e.value, b.value) > prev
                prev = (e.value, b.value)
            # as many sources as send boxes hold the sub-box's cells
            held = _send_cells(cfg, bx.field_slot % n_dom)
            assert (held[bx.first[0]:bx.last[0] + 1, bx.first[1]:bx.last[1] + 1] == bx.n_src).all()
        assert several > 0
        assert sorted(cover) == list(range(ex.n_items))
        for slot, c in cover.items():
            assert c.max() == 1  # pairwise disjoint
            assert np.array_equal(c > 0, _send_cells(cfg, slot % n_dom) > 0)  # the union
    finally:
        ex.close()


def test_z_fast_scalars_have_no_transformed_records(ghx):
    """c = 8 over six emulated ranks, z stride-1 scalars: every rotated space keeps its rows, so the
    reverse pack is one ordinary launch with as many segments as the unpack has."""
    ex = _Exchange(ghx, cs_cases.config(8), [(Z_FAST, 8, 1, 0, 0)], placement="six_ranks")
    try:
        assert _create(ghx, ex, [F64] * ex.n_items) == 0, _error(ghx)
        info = _info(ghx, ex)
        assert info["ready"] == 1 and (info["x_records"], info["x_tiles"]) == (0, 0)
        assert ex.plan_info()["rotated"] > 0
        pk, un = _segments(ghx, ex)
        assert pk == un > 0
    finally:
        ex.close()


def test_refusals_of_create(ghx):
    ex = _Exchange(ghx, cs_cases.config(6), TWO)
    good = _codes(ex, TWO, [F64, F32])
    try:
        for codes, word in [
                (good[:-1], "one dtype code per exchange item"),
                ([0] + good[1:], "unknown dtype code 0"),
                ([5] + good[1:], "unknown dtype code 5"),
                ([F32] + good[1:], "elem_size 8"),
                (good[:6] + [I32] + good[7:], "value_kind 1 but dtype code 3")]:
            assert _create(ghx, ex, codes) == -1
            assert word in _error(ghx), _error(ghx)
            assert _info(ghx, ex)["ready"] == 0
        assert ghx.lib().ghx_cs_exchange_adjoint_create(ex.h, None, ex.n_items) == -1
        # a scalar's value kind is free: its cells are summed as the code says
        assert _create(ghx, ex, [I64] * 6 + good[6:]) == 0, _error(ghx)
        # parity: create and both launches are refused while a direction has it
        n = ex.num_buffers()
        word = ctypes.c_uint64(0)
        offs = (ctypes.c_int64 * n)(*([1 << 20] * n))
        ghx.call("ghx_exchange_set_parity", ex.h, 0, ctypes.addressof(word), 0, offs, n)
        assert _create(ghx, ex, good) == -1 and "double-buffered" in _error(ghx)
        ptrs = ghx.ptr_array([256] * max(n, ex.n_items))
        L = ghx.lib()
        assert L.ghx_cs_exchange_adjoint_pack(ex.h, ptrs, ex.n_items, ptrs, n, None) == -1
        assert "double-buffered" in _error(ghx)
        assert L.ghx_cs_exchange_adjoint_accumulate(ex.h, ptrs, ex.n_items, ptrs, n, 1, None) == -1
        assert "double-buffered" in _error(ghx)
        ghx.call("ghx_exchange_set_parity", ex.h, 0, None, 0, offs, n)
        assert _create(ghx, ex, good) == 0, _error(ghx)
    finally:
        ex.close()


def test_integer_vectors_need_integer_codes(ghx):
    ex = _Exchange(ghx, cs_cases.config(6), [(X_FAST, 8, 2, 1, 2)])
    try:
        assert _create(ghx, ex, [F64] * ex.n_items) == -1
        assert "value_kind 2 but dtype code 2" in _error(ghx)
        assert _create(ghx, ex, [I64] * ex.n_items) == 0, _error(ghx)
    finally:
        ex.close()


def test_a_whole_24_domain_cube_on_one_rank_is_refused_for_its_slots(ghx):
    ex = _Exchange(ghx, cs_cases.config(10), [(X_FAST, 8, 1, 0, 1)])
    try:
        assert ex.num_buffers() == 168 > ghx.MAX_SLOTS
        assert _create(ghx, ex, [F64] * ex.n_items) == -1
        assert "at most 64 field and 64 buffer slots" in _error(ghx)
        assert _info(ghx, ex)["ready"] == 0
    finally:
        ex.close()


def test_the_same_cube_over_six_ranks_is_planned(ghx):
    ex = _Exchange(ghx, cs_cases.config(10), TWO, placement="six_ranks")
    try:
        assert _create(ghx, ex, _codes(ex, TWO, [F64, F32])) == 0, _error(ghx)
        info, plan = _info(ghx, ex), ex.plan_info()
        assert (info["x_records"], info["x_tiles"]) == (plan["records"], plan["tiles"])
        assert plan["records"] > 0
    finally:
        ex.close()


def test_not_a_cubed_sphere_exchange(ghx):
    """A regular structured exchange is refused; the other two adjoints answer a cubed-sphere
    exchange as before."""
    from tests.test_saccum_host import _exchange, cube
    plan = _exchange(ghx, [cube(6, 2)], 6, 2)
    assert ghx.lib().ghx_cs_exchange_adjoint_create(plan.h, ghx.i32_array([F64]), 1) == -1
    assert "not a cubed-sphere exchange" in _error(ghx)
    r = ctypes.c_int32(-1)
    ghx.call("ghx_cs_exchange_adjoint_info", plan.h, ctypes.byref(r), None, None, None, None)
    assert r.value == 0
    ex = _Exchange(ghx, cs_cases.config(6), [(X_FAST, 8, 1, 0, 1)])
    try:
        codes = ghx.i32_array([F64] * ex.n_items)
        assert ghx.lib().ghx_sexchange_adjoint_create(ex.h, codes, ex.n_items) == -1
        assert "would rotate and flip signs" in _error(ghx)
        assert ghx.lib().ghx_uexchange_adjoint_create(ex.h, codes, ex.n_items) == -1
        assert "structured or cubed-sphere item" in _error(ghx)
    finally:
        ex.close()


def test_python_option_is_opt_in_and_keeps_the_refusals(ghx):
    from ghex_amd.communication_object import CommunicationObject
    from ghex_amd.structured import cubed_sphere as CS
    from tests.gpu_util import FakeContext
    from tests.test_cubed_sphere_host import _fake_buffer_info
    import types
    ctx = FakeContext(0, 1, [None])
    assert CommunicationObject(ctx).adjoint_rotated is False
    assert CS.make_communication_object(ctx).adjoint_rotated is False
    assert CS.make_communication_object(ctx, adjoint_rotated=True).adjoint_rotated is True
    bi = _fake_buffer_info(ghx)
    # without the option: today's refusals, with or without adjoint_boxes
    with pytest.raises(ValueError, match="unstructured fields only"):
        CommunicationObject(ctx)._adjoint_plan([bi])
    with pytest.raises(ValueError, match="cubed-sphere"):
        CommunicationObject(ctx, adjoint_boxes=True)._adjoint_plan([bi])
    # with it: no direct, no pipelined, no mixing with other fields
    for opts in (dict(direct=True), dict(pipelined=True)):
        with pytest.raises(ValueError, match="plain communication object"):
            CommunicationObject(ctx, adjoint_rotated=True, **opts)._adjoint_plan([bi])
    other = types.SimpleNamespace(field=types.SimpleNamespace(kind=0, desc=ghx.FieldDesc(), align=8),
                                  pattern_container=object(), local_index=0)
    with pytest.raises(ValueError, match="cubed-sphere fields or other fields, not both"):
        CommunicationObject(ctx, adjoint_rotated=True)._adjoint_plan([bi, other])
    # a list without cubed-sphere fields takes the path it took
    with pytest.raises(ValueError, match="unstructured fields only"):
        CommunicationObject(ctx, adjoint_rotated=True)._adjoint_plan([other])
