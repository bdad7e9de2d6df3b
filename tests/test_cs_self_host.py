"""The fused cubed-sphere self exchange as planned without a device (ghx_cs_self_info,
ghx_cs_exchange_self): when it is built, what its records count, and why it is refused."""
import ctypes

import pytest

from tests import cs_cases
from tests.test_cubed_sphere_host import PLACEMENTS, _patterns

EDGES = (10, 6, 70, 8)
X_FAST, Z_FAST = (3, 2, 1, 0), (1, 2, 3, 0)


@pytest.fixture(scope="module")
def ghx():
    import ghex_amd
    ghex_amd.native_library()
    from ghex_amd import _ghx
    return _ghx


def _item(ghx, cfg, pat, li, dom, layout, elem, nc, vector, kind):
    h = max(cfg["halos"]) + 1
    shape = (dom["x"][1] - dom["x"][0] + 1 + 2 * h, dom["y"][1] - dom["y"][0] + 1 + 2 * h,
             cfg["levels"], nc)
    it = ghx.ExchangeItem()
    it.pattern, it.local_index, it.kind, it.align, it.tag_offset = pat, li, 0, elem, 0
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
    return it, cs


class _Exchange:
    """One exchange of `specs` = [(layout or per-domain layout function, elem, nc, vector, kind)]
    fields per domain of rank 0's pattern, spec-major."""

    def __init__(self, ghx, cfg, specs, placement="one_rank"):
        self.ghx = ghx
        self.pats, _, order = _patterns(ghx, cfg, PLACEMENTS[placement])
        mine = [i for i in order if PLACEMENTS[placement](i, cfg["domains"][i]) == 0]
        items, cs_items = [], []
        for layout, elem, nc, vector, kind in specs:
            for li, i in enumerate(mine):
                lay = layout(li) if callable(layout) else layout
                it, cs = _item(ghx, cfg, self.pats[0], li, cfg["domains"][i], lay, elem, nc,
                               vector, kind)
                items.append(it)
                cs_items.append(cs)
        self.h = ctypes.c_void_p()
        ghx.call("ghx_cs_exchange_create", (ghx.ExchangeItem * len(items))(*items),
                 (ghx.CsItem * len(items))(*cs_items), len(items), ctypes.byref(self.h))
        self.n_items = len(items)

    def self_info(self):
        f, p, r, t = (ctypes.c_int32(-1) for _ in range(4))
        self.ghx.call("ghx_cs_self_info", self.h, ctypes.byref(f), ctypes.byref(p),
                      ctypes.byref(r), ctypes.byref(t))
        return dict(fusable=f.value, pair_tiles=p.value, records=r.value, tiles=t.value,
                    reason=self.ghx.lib().ghx_last_error().decode())

    def plan_info(self):
        n, t, r = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self.ghx.call("ghx_cs_plan_info", self.h, ctypes.byref(n), None, ctypes.byref(t),
                      ctypes.byref(r))
        return dict(records=n.value, tiles=t.value, rotated=r.value)

    def num_buffers(self):
        n = ctypes.c_int32()
        self.ghx.call("ghx_exchange_num_buffers", self.h, 0, ctypes.byref(n))
        return n.value

    def close(self):
        self.ghx.lib().ghx_exchange_destroy(self.h)
        for p in self.pats:
            self.ghx.lib().ghx_pattern_destroy(p)


@pytest.mark.parametrize("edge", EDGES)
def test_a_whole_cube_of_x_fast_fields_on_one_rank_is_fusable(ghx, edge):
    """An fp64 scalar and an f32 3-vector per domain, x stride-1: the self tile records are
    exactly the transformed unpack's records, cut into the same tiles; every other space is a
    pair. The plain fused self exchange stays refused."""
    ex = _Exchange(ghx, cs_cases.config(edge), [(X_FAST, 8, 1, 0, 1), (X_FAST, 4, 3, 1, 1)])
    try:
        s, p = ex.self_info(), ex.plan_info()
        assert s["fusable"] == 1 and s["reason"] == "", s
        assert p["records"] > 0
        assert s["records"] == p["records"] and s["tiles"] == p["tiles"]
        assert s["pair_tiles"] > 0
        fus = ctypes.c_int32(1)
        ghx.call("ghx_exchange_self_fusable", ex.h, ctypes.byref(fus))
        assert fus.value == 0
    finally:
        ex.close()


def _unpaired_rotated(cfg):
    """Rotated receive spaces of a z-stride-1 scalar field whose pack and unpack segments differ.
    The levels are dense, so the packing side merges a box's z rows with its next-fastest axis y
    (rows of levels * y-extent elements); the receiving side of a rotated space walks the buffer's
    y' axis along the field's x and keeps rows of `levels` elements. The rows agree, and the space
    is a pair, only when the box is one cell wide in y'."""
    n = 0
    for dom in cfg["domains"]:
        for b in dom["boxes"]:
            if b["t"] == dom["tile"] or b["img"][2] != b["img"][0]:
                continue  # own tile, or a translation
            # x = [domain, local first, local last, global first, global last]: y' extent
            n += sum(1 for x in b["x"] if x[11] - x[8] + 1 > 1)
    return n


@pytest.mark.parametrize("edge", EDGES)
def test_z_fast_scalars_make_records_only_of_the_spaces_whose_pairing_fails(ghx, edge):
    cfg = cs_cases.config(edge)
    ex = _Exchange(ghx, cfg, [(Z_FAST, 8, 1, 0, 0)])
    try:
        s, p = ex.self_info(), ex.plan_info()
        assert s["fusable"] == 1, s
        assert p["records"] == 0 and p["rotated"] > 0  # nothing is transformed on the plain path
        assert s["records"] == _unpaired_rotated(cfg)
        assert 0 < s["records"] <= p["rotated"] and s["tiles"] >= s["records"]
        if edge == 6:  # halos (1, 2, 0, 3): some rotated boxes are one cell wide and pair
            assert s["records"] < p["rotated"]
    finally:
        ex.close()


def _refused(ghx, ex, word):
    s = ex.self_info()
    assert s["fusable"] == 0 and (s["pair_tiles"], s["records"], s["tiles"]) == (0, 0, 0), s
    assert word in s["reason"], s["reason"]
    # the launch is refused without touching its pointer arguments
    rc = ghx.lib().ghx_cs_exchange_self(ex.h, None, 0, None, 0, None)
    assert rc == -1 and word in ghx.lib().ghx_last_error().decode()


def test_peer_messages_are_not_fusable(ghx):
    ex = _Exchange(ghx, cs_cases.config(6), [(X_FAST, 8, 1, 0, 1)], placement="six_ranks")
    try:
        _refused(ghx, ex, "peer messages")
    finally:
        ex.close()


def test_more_slots_than_one_launch_holds_are_not_fusable(ghx):
    """A plan in several launch groups. The fused launch carries its own pointer table (448
    field and buffer pointers together; the 24-domain geometry alone has 168 buffers, so
    GHX_MAX_SLOTS of each would not do): 80 fields per domain of the six-domain cube are 480
    field slots, far beyond the 64 of one ordinary launch group, and do not fit."""
    ex = _Exchange(ghx, cs_cases.config(6), [(X_FAST, 4, 1, 0, 0)] * 80)
    try:
        assert ex.n_items == 480 > ghx.MAX_SLOTS
        _refused(ghx, ex, "launch group")
    finally:
        ex.close()
    # within the table: more than 64 buffers (c = 8: 66; c = 10: 168) is still one launch
    for edge in (8, 10):
        ex = _Exchange(ghx, cs_cases.config(edge), [(X_FAST, 8, 1, 0, 1)])
        try:
            assert ex.num_buffers() > ghx.MAX_SLOTS and ex.self_info()["fusable"] == 1
        finally:
            ex.close()


def test_paired_fields_of_different_layout_order_are_not_fusable(ghx):
    """Every other domain z stride-1: a message's dense box has one axis order seen from the
    sender and another seen from the receiver."""
    ex = _Exchange(ghx, cs_cases.config(6), [(lambda li: X_FAST if li % 2 else Z_FAST, 8, 1, 0, 1)])
    try:
        _refused(ghx, ex, "layout order")
    finally:
        ex.close()


def test_send_side_parity_refuses_the_fused_launch(ghx):
    ex = _Exchange(ghx, cs_cases.config(6), [(X_FAST, 8, 1, 0, 1)])
    try:
        assert ex.self_info()["fusable"] == 1
        n = ex.num_buffers()
        word = ctypes.c_uint64(0)
        offs = (ctypes.c_int64 * n)(*([1 << 20] * n))
        ghx.call("ghx_exchange_set_parity", ex.h, 0, ctypes.addressof(word), 0, offs, n)
        ptrs = ghx.ptr_array([256] * max(n, ex.n_items))
        rc = ghx.lib().ghx_cs_exchange_self(ex.h, ptrs, ex.n_items, ptrs, n, None)
        assert rc == -1 and "double-buffered" in ghx.lib().ghx_last_error().decode()
    finally:
        ex.close()


def test_python_option_is_opt_in_and_keeps_the_refusals(ghx):
    from ghex_amd.communication_object import CommunicationObject
    from ghex_amd.structured import cubed_sphere as CS
    from tests.gpu_util import FakeContext
    from tests.test_cubed_sphere_host import _fake_buffer_info
    ctx = FakeContext(0, 1, [None])
    assert CommunicationObject(ctx).fuse_rotated is False
    assert CS.make_communication_object(ctx, fuse_rotated=True).fuse_rotated is True
    bi = _fake_buffer_info(ghx)
    for opts in (dict(direct=True), dict(pipelined=True)):
        with pytest.raises(ValueError, match="cubed-sphere"):
            CommunicationObject(ctx, fuse_rotated=True, **opts).plan([bi])
