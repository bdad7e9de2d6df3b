"""GPU tests of the cubed-sphere halo exchange: the rotating unpack (k_unpack_x after the
ordinary unpack launch) against expectations expanded cell by cell from the reference's recorded
halo boxes and tile-coordinate images (tests/golden/cubed_sphere_case.json, tests/cs_cases.py).
Fields are compared as bit patterns: every expected halo cell bit-equal (floats carry -0.0, inf
and a NaN), every other byte — interior, cube-corner cells, padding — unchanged. The tests run
in-process like the suite's other kernel tests (a few milliseconds of device work each; the
suite's time limits bound child processes, of which there are none here)."""
import numpy as np
import pytest

from tests import cs_cases
from tests.cs_cases import DomainField, from_device, to_device
from tests.gpu_util import FakeContext, emulated_exchange

pytestmark = pytest.mark.gpu

X_FAST, Z_FAST, K_FAST = (3, 2, 1, 0), (1, 2, 3, 0), (0, 1, 2, 3)
Y_FAST = (2, 3, 1, 0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ghex_amd
    ghex_amd.native_library()


def _descriptor(CS, cube, df, logical):
    dom = df.dom
    dd = CS.DomainDescriptor(cube, dom["tile"], *dom["x"], *dom["y"])
    return dd, CS.FieldDescriptor(dd, logical, df.offsets, df.extents, df.nc, df.vector)


# every distinct transform: the four neighbour directions of an even and an odd tile (domain 0
# of tile 0 sees -x and -y, domain 3 sees +x and +y; likewise tile 1's domains 4 and 7)
@pytest.mark.parametrize("layout", [X_FAST, Z_FAST, K_FAST, Y_FAST], ids="xzky")
@pytest.mark.parametrize("dtype,nc,vector", [("float64", 1, False), ("float32", 3, True),
                                             ("int32", 3, True), ("float64", 3, True),
                                             ("int32", 1, False)])
def test_cs_unpack_of_one_field(layout, dtype, nc, vector):
    import torch
    from ghex_amd.structured import cubed_sphere as CS
    cfg = cs_cases.config(10)
    cube = CS.Cube(cfg["edge_size"], cfg["levels"])
    for di in (0, 3, 4, 7):
        df = DomainField(cfg, di, dtype, nc, vector)
        boxes = df.dom["boxes"]
        base, logical = to_device(df.initial(), layout, dtype)
        _, fd = _descriptor(CS, cube, df, logical)
        buf = torch.from_numpy(df.buffer(boxes, layout).view(np.dtype(dtype))).cuda()
        fd.unpack(buf, df.spaces(boxes))
        torch.cuda.synchronize()
        got, exp = from_device(base, layout, dtype), df.expected(boxes)
        assert np.array_equal(got, exp), (di, np.argwhere(got != exp)[:5])


def test_cs_unpack_of_a_three_dimensional_tensor():
    """A scalar field without a component axis (x stride-1)."""
    import torch
    from ghex_amd.structured import cubed_sphere as CS
    cfg = cs_cases.config(6)
    cube = CS.Cube(cfg["edge_size"], cfg["levels"])
    for di in (0, 1):
        df = DomainField(cfg, di, "float32", 1, False)
        base, logical = to_device(df.initial(), X_FAST, "float32")
        dom = df.dom
        dd = CS.DomainDescriptor(cube, dom["tile"], *dom["x"], *dom["y"])
        fd = CS.make_field_descriptor(dd, logical[..., 0], df.offsets, df.extents)
        buf = torch.from_numpy(df.buffer(dom["boxes"], X_FAST).view(np.float32)).cuda()
        fd.unpack(buf, df.spaces(dom["boxes"]))
        torch.cuda.synchronize()
        assert np.array_equal(from_device(base, X_FAST, "float32"), df.expected())


def _one_rank(cfg, specs, **co_options):
    """All domains of `cfg` on one rank with one field per spec (dtype, nc, vector, layout):
    (communication object, buffer infos, [(DomainField, base, layout, dtype)])."""
    import ghex_amd
    from ghex_amd.structured import cubed_sphere as CS
    cube = CS.Cube(cfg["edge_size"], cfg["levels"])
    ctx = ghex_amd.make_context()
    dds = [CS.DomainDescriptor(cube, d["tile"], *d["x"], *d["y"]) for d in cfg["domains"]]
    pc = CS.make_pattern(ctx, CS.HaloGenerator(cfg["halos"]), dds)
    bis, fields = [], []
    for dtype, nc, vector, layout in specs:
        for di, dd in enumerate(dds):
            df = DomainField(cfg, di, dtype, nc, vector)
            base, logical = to_device(df.initial(), layout, dtype)
            bis.append(pc(CS.FieldDescriptor(dd, logical, df.offsets, df.extents, nc, vector)))
            fields.append((df, base, layout, dtype))
    return CS.make_communication_object(ctx, **co_options), bis, fields


def _check(fields):
    for df, base, layout, dtype in fields:
        got, exp = from_device(base, layout, dtype), df.expected()
        assert np.array_equal(got, exp), (df.di, dtype, np.argwhere(got != exp)[:5])


REFERENCE_FIELDS = [("float64", 1, False, X_FAST), ("float32", 3, True, X_FAST)]


@pytest.mark.parametrize("fuse_self", [False, True])
def test_exchange_of_the_reference_geometry_on_one_rank(fuse_self):
    """24 domains (c = 10, four 5 x 5 per tile, halo 2, test_cubed_sphere_exchange.cpp:945-955),
    a scalar f64 and a 3-component vector f32 field in one exchange. The default (fuse_self)
    object must take the two-launch path: an exchange with a rotated space is not fusable."""
    import ctypes
    from ghex_amd import _ghx
    co, bis, fields = _one_rank(cs_cases.config(10), REFERENCE_FIELDS, fuse_self=fuse_self)
    plan = co.plan(bis)
    assert not co.all_self(plan) and not co.mixed(plan)
    n, r = ctypes.c_int32(), ctypes.c_int32()
    _ghx.call("ghx_cs_plan_info", plan.h, ctypes.byref(n), None, None, ctypes.byref(r))
    assert n.value > 0 and n.value == r.value  # x stride-1: every rotated space is transformed
    co.exchange(bis).wait()
    _check(fields)


def test_exchange_with_rows_kept_rides_the_ordinary_launch():
    """z stride-1 scalar fields: the rotated spaces are ordinary segments with signed strides."""
    import ctypes
    from ghex_amd import _ghx
    co, bis, fields = _one_rank(cs_cases.config(8), [("float64", 1, False, Z_FAST),
                                                      ("int32", 2, False, K_FAST)])
    plan = co.plan(bis)
    n, r = ctypes.c_int32(), ctypes.c_int32()
    _ghx.call("ghx_cs_plan_info", plan.h, ctypes.byref(n), None, None, ctypes.byref(r))
    assert n.value == 0 and r.value > 0
    co.exchange(bis).wait()
    _check(fields)


def test_six_emulated_ranks_with_asymmetric_halos():
    """One tile per rank, c = 6, halos (1, 2, 0, 3)."""
    from ghex_amd.structured import cubed_sphere as CS
    cfg = cs_cases.config(6)
    cube = CS.Cube(cfg["edge_size"], cfg["levels"])
    table = [[(cube.edge_size, cube.levels, d["tile"], *d["x"], *d["y"])] for d in cfg["domains"]]
    cos, bis_all, fields = [], [], []
    for r, dom in enumerate(cfg["domains"]):
        ctx = FakeContext(r, 6, table)
        dd = CS.DomainDescriptor(cube, dom["tile"], *dom["x"], *dom["y"])
        pc = CS.make_pattern(ctx, CS.HaloGenerator(cfg["halos"]), [dd])
        bis = []
        for dtype, nc, vector, layout in (("float32", 2, True, X_FAST), ("float64", 1, False, Y_FAST)):
            df = DomainField(cfg, r, dtype, nc, vector)
            base, logical = to_device(df.initial(), layout, dtype)
            bis.append(pc(CS.FieldDescriptor(dd, logical, df.offsets, df.extents, nc, vector)))
            fields.append((df, base, layout, dtype))
        cos.append(CS.make_communication_object(ctx))
        bis_all.append(bis)
    emulated_exchange(cos, bis_all)
    _check(fields)


def test_edge_boxes_longer_than_a_wave_and_a_tile():
    """c = 70, 5 levels, halo 3, f64, one domain per tile: each edge box is 8,400 B (just over
    8 KiB) in several workgroup tiles, its rows are longer than a wave, and the reversed axes
    cross wave and tile boundaries."""
    co, bis, fields = _one_rank(cs_cases.config(70), [("float64", 1, False, X_FAST)])
    co.exchange(bis).wait()
    _check(fields)


def test_pack_and_unpack_replayed_from_a_linear_capture():
    """Pack and unpack (ordinary launch, then the transformed one) of the 24-domain exchange
    captured on one stream without branches; two replays with changed interiors."""
    import torch
    from ghex_amd import _ghx
    co, bis, fields = _one_rank(cs_cases.config(10), REFERENCE_FIELDS, fuse_self=False)
    plan = co.plan(bis)
    send, recv = co.buffers(plan, fields[0][1].device)
    L = _ghx.lib()
    fp = _ghx.ptr_array([bi.field.data_ptr() for bi in bis])
    sp = _ghx.ptr_array([t.data_ptr() for t in send])
    rp = _ghx.ptr_array([t.data_ptr() for t in recv])

    def step(s):
        _ghx.check(L.ghx_exchange_pack(plan.h, fp, len(bis), sp, len(send), s), "pack")
        _ghx.check(L.ghx_exchange_unpack(plan.h, fp, len(bis), rp, len(recv), s), "unpack")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(side.cuda_stream)  # warm, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(torch.cuda.current_stream().cuda_stream)
    for flip in (0x1, 0x2):
        # new interiors (low mantissa / value bits flipped), stale halos from the run before
        for df, base, layout, dtype in fields:
            a = from_device(base, layout, dtype).copy()
            first = df.initial()
            own = first != df.sentinel
            a[own] = first[own] ^ cs_cases.uint_of(dtype)(flip)
            order = cs_cases.layout_order(layout)
            base.copy_(torch.from_numpy(np.ascontiguousarray(a.transpose(order))
                                        .view(np.dtype(dtype))))
        g.replay()
        torch.cuda.synchronize()
        for df, base, layout, dtype in fields:
            exp = _expected_with_interior_flip(df, flip)
            got = from_device(base, layout, dtype)
            assert np.array_equal(got, exp), (df.di, dtype, flip)


def _expected_with_interior_flip(df, flip):
    """df.expected() when every interior cell of every domain has `flip` XORed into its bits
    (applied before a vector component's negation, as the exchange sees it)."""
    u = cs_cases.uint_of(df.dtype)
    a = df.initial()
    own = a != df.sentinel
    a[own] ^= u(flip)
    for b in df.dom["boxes"]:
        xs, ys, _ = df.box_values(b)
        saved, df.vector = df.vector, False
        _, _, plain = df.box_values(b)
        df.vector = saved
        bits = plain ^ u(flip)
        if df.vector:
            for comp in (0, 1):
                if comp < df.nc and b["sign"][comp] < 0:
                    bits[..., comp] = cs_cases.negate_bits(bits[..., comp], df.dtype)
        a[xs[0] + df.h:xs[-1] + df.h + 1, ys[0] + df.h:ys[-1] + df.h + 1] = bits
    return a
