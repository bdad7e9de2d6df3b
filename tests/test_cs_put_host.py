"""Cubed-sphere puts as planned without a device (ghx_cs_put_create, ghx_cs_put_info): what the
plans count, what they refuse and why, and the Python factory's local checks."""
import ctypes
import types

import pytest

from tests import cs_cases
from tests.cs_put_cases import X_FAST, Z_FAST, Puts, descriptor_fields
from tests.test_cs_self_host import _Exchange, _unpaired_rotated

ONE_RANK = lambda i, dom: 0  # noqa: E731
SIX_RANKS = lambda i, dom: dom["tile"]  # noqa: E731


@pytest.fixture(scope="module")
def ghx():
    import ghex_amd
    ghex_amd.native_library()
    from ghex_amd import _ghx
    return _ghx


def _send_bytes(ghx, ex):
    n, tot = ex.num_buffers(), 0
    for i in range(n):
        size = ctypes.c_uint64()
        ghx.call("ghx_exchange_buffer", ex.h, 0, i, None, None, None, None, ctypes.byref(size))
        tot += size.value
    return tot


@pytest.mark.parametrize("place", [ONE_RANK, SIX_RANKS], ids=["one_rank", "six_ranks"])
def test_six_domains_of_x_fast_f64_make_pair_tiles_and_put_tile_records(ghx, place):
    """One domain per tile, x stride-1 f64 scalar: transformed spaces become put tile records,
    the others pairs, and the plans move exactly the bytes the buffered exchange's send buffers
    hold (one field per buffer: no alignment pads to subtract). The same whether the six
    domains sit on one rank or on six."""
    cfg = cs_cases.config(6)
    spec = (X_FAST, 8, 1, 0, 0)
    puts = Puts(descriptor_fields(cfg, place, [spec]))
    ex = _Exchange(ghx, cfg, [spec])  # the whole cube on one rank: every message once
    try:
        info = puts.info()
        assert info["records"] > 0 and info["pair_tiles"] > 0 and info["x_tiles"] >= info["records"]
        assert info["records"] == ex.plan_info()["records"]  # the transformed unpack's spaces
        assert info["bytes"] == _send_bytes(ghx, ex) > 0
    finally:
        puts.close()
        ex.close()


@pytest.mark.parametrize("edge", [6, 10])
def test_z_fast_scalars_make_records_only_of_the_spaces_whose_pairing_fails(ghx, edge):
    """z stride-1: cs_plan_space transforms nothing; the rotated spaces whose rows the sender's
    rows match stay pairs, and only the others (the sender merges its z rows with y) become put
    tile records — the count the fused self exchange arrives at."""
    cfg = cs_cases.config(edge)
    spec = (Z_FAST, 8, 1, 0, 0)
    puts = Puts(descriptor_fields(cfg, ONE_RANK, [spec]))
    ex = _Exchange(ghx, cfg, [spec])
    try:
        info, p = puts.info(), ex.plan_info()
        assert p["records"] == 0 and p["rotated"] > 0
        assert info["records"] == _unpaired_rotated(cfg)
        assert info["pair_tiles"] > 0
        if edge == 6:  # halos (1, 2, 0, 3): some rotated boxes are one cell wide and pair
            assert 0 < info["records"] < p["rotated"]
        assert info["bytes"] == _send_bytes(ghx, ex)
    finally:
        puts.close()
        ex.close()


def _refused(ghx, word, specs, mutate=None, place=SIX_RANKS):
    """GHX_ERR_INVALID (-1) with `word` in the reason: GhxError's text is "<call> failed (<rc>):
    <ghx_last_error()>", read right after the failed call."""
    with pytest.raises(ghx.GhxError, match=rf"ghx_cs_put_create failed \(-1\): .*{word}"):
        Puts(descriptor_fields(cs_cases.config(6), place, specs), mutate).close()


def test_fields_of_different_layout_order_are_refused(ghx):
    _refused(ghx, "layout order", [(lambda i: X_FAST if i % 2 else Z_FAST, 8, 1, 0, 0)])


def test_fields_of_different_element_size_are_refused(ghx):
    def widen(src, dst):
        src[0].field.elem_size = 4
    _refused(ghx, "element size", [(X_FAST, 8, 1, 0, 0)], widen)


def test_an_unpaired_space_of_12_byte_elements_is_refused(ghx):
    _refused(ghx, "1, 2, 4, 8 or 16", [(X_FAST, 12, 1, 0, 0)])


def test_a_source_box_of_another_shape_is_refused(ghx):
    def shrink(src, dst):
        src[0].boxes[0].last[2] -= 1
    _refused(ghx, "differ in shape", [(X_FAST, 8, 1, 0, 0)], shrink)


def test_a_vector_field_of_opaque_values_is_refused(ghx):
    _refused(ghx, "vector field must hold", [(X_FAST, 4, 3, 1, 0)])
    _refused(ghx, "vector field must hold", [(X_FAST, 2, 3, 1, 1)])


def test_a_source_box_that_starts_in_the_senders_halo_is_refused(ghx):
    for axis in range(3):
        def lower(src, dst, axis=axis):
            src[0].boxes[0].first[axis] = -1
        _refused(ghx, "halo", [(X_FAST, 8, 1, 0, 0)], lower)


def test_a_plain_put_reports_no_transformed_records(ghx):
    fd = ghx.FieldDesc()
    fd.dim, fd.elem_size, fd.num_components, fd.has_components = 3, 8, 1, 0
    for d, (lay, stride) in enumerate(((2, 8), (1, 80), (0, 800))):
        fd.layout[d], fd.byte_strides[d], fd.offsets[d], fd.extents[d] = lay, stride, 1, 10
    src, dst = ghx.PackEntry(), ghx.PackEntry()
    sb, db = ghx.Box(), ghx.Box()
    sb.first[:3], sb.last[:3] = (0, 0, 0), (7, 7, 0)
    db.first[:3], db.last[:3] = (0, 0, 8), (7, 7, 8)
    for e, b in ((src, sb), (dst, db)):
        e.field, e.field_slot, e.buffer_slot, e.buffer_offset = fd, 0, 0, 0
        e.boxes, e.n_boxes = ctypes.pointer(b), 1
    h = ctypes.c_void_p()
    ghx.call("ghx_put_create", ctypes.byref(src), 1, ctypes.byref(dst), 1, ctypes.byref(h))
    try:
        t, p, r, x = (ctypes.c_int32(-1) for _ in range(4))
        ghx.call("ghx_put_info", h, None, ctypes.byref(t))
        ghx.call("ghx_cs_put_info", h, ctypes.byref(p), ctypes.byref(r), ctypes.byref(x))
        assert (p.value, r.value, x.value) == (t.value, 0, 0) and t.value > 0
    finally:
        ghx.lib().ghx_put_destroy(h)


def _fake_buffer_info(ghx, elem):
    """tests/test_cubed_sphere_host.py's fake cubed-sphere buffer info, with an element size."""
    desc = ghx.FieldDesc()
    desc.elem_size = elem
    field = types.SimpleNamespace(kind=0, cs_item=ghx.CsItem(), desc=desc, align=8,
                                  domain_id=lambda: 0)
    return types.SimpleNamespace(field=field, pattern_container=object(), local_index=0)


def test_the_factory_takes_what_the_plain_object_refuses(ghx):
    from ghex_amd.bulk_communication_object import (BulkCommunicationObject,
                                                    make_bulk_communication_object)
    from ghex_amd.structured import cubed_sphere as CS
    from tests.gpu_util import FakeContext
    ctx = FakeContext(0, 1, [None])
    bi = _fake_buffer_info(ghx, 8)
    for plain in (make_bulk_communication_object(ctx), BulkCommunicationObject(ctx)):
        with pytest.raises(ValueError, match="cubed-sphere"):
            plain.add_field(bi)
    bco = CS.make_bulk_communication_object(ctx)
    bco.add_field(bi)
    assert bco.cubed_sphere and not bco.initialized() and len(bco._bis) == 1
    not_cs = types.SimpleNamespace(field=types.SimpleNamespace(kind=0, desc=ghx.FieldDesc()),
                                   pattern_container=object(), local_index=0)
    with pytest.raises(ValueError, match="cubed-sphere fields only"):
        bco.add_field(not_cs)


@pytest.mark.parametrize("elem", [12, 3, 32])
def test_the_factory_refuses_element_sizes_a_rotating_put_cannot_move(ghx, elem):
    """Refused in add_field: locally, before any collective step."""
    from ghex_amd.structured import cubed_sphere as CS
    from tests.gpu_util import FakeContext
    bco = CS.make_bulk_communication_object(FakeContext(0, 1, [None]))
    with pytest.raises(ValueError, match="1, 2, 4, 8 or 16"):
        bco.add_field(_fake_buffer_info(ghx, elem))
    assert not bco._bis
