"""Times the transformed unpack launch (k_unpack_x) of a cubed-sphere halo against the same
spaces expressed as element-row segments of the ordinary unpack kernel.

The rank is FV3-like: one tile of c = 96, 80 levels, halo 3, f64, x stride-1, scalar. For each of
the four rotated edge orientations (an even tile's -x and +y neighbours, an odd tile's +x and
-y) the one edge box is unpacked
  new:      ghx_cs_unpack -> one k_unpack_x launch (sub-box tiles walked in field order);
  baseline: a ghx_plan_create unpack plan over a view of the field whose dims are the buffer's
            (x', y', z) with the rotated, signed byte strides: element-sized rows on the general
            addressing path (fast_addr off), i.e. what the library could do before this kernel.
Both are checked bit for bit against the NumPy expectation first. Timing: a captured graph of
LAUNCHES back-to-back launches, replayed REPLAYS times between two events, new and baseline
alternating for ROUNDS rounds; the median per-launch time of each is reported with the ratio,
the algorithmic bytes (box read + box written) and their fraction of the HBM peak.

The tile transforms are not restated here: rotation, translation and offset of each orientation
are solved from the recorded images of tests/golden/cubed_sphere_case.json (c = 70 and c = 8).

    python tools/cs_unpack_bench.py [--out profiles/cs_unpack_bench.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, LEVELS, HALO, ELEM = 96, 80, 3, 8
LAUNCHES, REPLAYS, ROUNDS = 20, 25, 7
HBM_PEAK = 8.0e12  # B/s (MI355X, 8 stacks of HBM3E)
ORIENTATIONS = [("even -x", 0, 4), ("even +y", 0, 2), ("odd +x", 1, 3), ("odd -y", 1, 5)]


def solve_transform(tile, nbr):
    """(R, t, o) with T(p, c) = R p + t c + o, from the fixture's images at two edge sizes."""
    with open(os.path.join(ROOT, "tests", "golden", "cubed_sphere_case.json")) as fh:
        cases = {cfg["edge_size"]: cfg for cfg in json.load(fh)}
    found = {}
    for c in (70, 8):
        for dom in cases[c]["domains"]:
            if dom["tile"] != tile:
                continue
            for b in dom["boxes"]:
                if b["t"] == nbr and c not in found:
                    i0, i1, i2 = (np.array(b["img"][k:k + 2]) for k in (0, 2, 4))
                    R = np.stack([i1 - i0, i2 - i0], axis=1)
                    p0 = np.array([b["l"][0] + dom["x"][0], b["l"][1] + dom["y"][0]])
                    found[c] = (R, i0 - R @ p0)
    (R, b70), (R8, b8) = found[70], found[8]
    assert (R == R8).all()
    t = (b70 - b8) // 62
    assert ((b70 - b8) == 62 * t).all()
    return R, t, b8 - 8 * t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cs_unpack_bench.json"))
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE",
                    help="ghx_tune knob set before the plans are made (development A/Bs)")
    a = ap.parse_args()
    import torch
    import ghex_amd
    from ghex_amd import _ghx
    ghex_amd.native_library()
    assert torch.cuda.is_available(), "cs_unpack_bench needs a GPU"
    L = _ghx.lib()
    for kv in a.tune:
        key, value = kv.split("=")
        _ghx.call("ghx_tune", key.encode(), int(value))
    E = C + 2 * HALO
    sx, sy, sz = ELEM, ELEM * E, ELEM * E * E
    rng = np.random.default_rng(7)
    results = []
    for name, tile, nbr in ORIENTATIONS:
        R, t, o = solve_transform(tile, nbr)
        shift = t * C + o
        dom = _ghx.CsDomain()
        dom.rank, dom.tile, dom.x_first, dom.x_last, dom.y_first, dom.y_last = 0, tile, 0, C - 1, 0, C - 1
        n = ctypes.c_int32()
        halos = _ghx.i32_array([HALO] * 4)
        _ghx.call("ghx_cs_halo_boxes", C, LEVELS, ctypes.byref(dom), halos, None, None, None, 0,
                  ctypes.byref(n))
        loc, glo = (_ghx.Box * n.value)(), (_ghx.Box * n.value)()
        til = (ctypes.c_int32 * n.value)()
        _ghx.call("ghx_cs_halo_boxes", C, LEVELS, ctypes.byref(dom), halos, loc, glo, til, n.value,
                  ctypes.byref(n))
        (k,) = [i for i in range(n.value) if til[i] == nbr]
        lf, ll = np.array(loc[k].first[:3]), np.array(loc[k].last[:3])
        gf, gl = np.array(glo[k].first[:3]), np.array(glo[k].last[:3])
        bext = gl - gf + 1  # (x', y', z)
        nbytes = int(bext.prod()) * ELEM
        # buffer: the dense box, x' fastest; expectation: field cell <- buffer cell (T(x, y) - gf, z)
        buf_h = rng.integers(1, 1 << 62, size=(bext[2], bext[1], bext[0]), dtype=np.int64)
        field_h = rng.integers(1, 1 << 62, size=(LEVELS, E, E), dtype=np.int64)  # [z][y][x]
        exp = field_h.copy()
        xs, ys = np.meshgrid(np.arange(lf[0], ll[0] + 1), np.arange(lf[1], ll[1] + 1), indexing="ij")
        img = np.einsum("ij,jxy->ixy", R, np.stack([xs, ys])) + shift[:, None, None]
        for z in range(bext[2]):
            exp[lf[2] + z, ys + HALO, xs + HALO] = buf_h[z, img[1] - gf[1], img[0] - gf[0]]
        buf = torch.from_numpy(buf_h).cuda()
        field = torch.from_numpy(field_h).cuda()
        # new: the library's cubed-sphere unpack of the (x, y, z) view
        fd = _ghx.FieldDesc()
        fd.dim, fd.elem_size, fd.num_components, fd.has_components = 3, ELEM, 1, 0
        for d, (s, ext) in enumerate(((sx, E), (sy, E), (sz, LEVELS))):
            fd.layout[d], fd.byte_strides[d] = 2 - d, s
            fd.offsets[d], fd.extents[d] = (HALO if d < 2 else 0), ext
        cs = _ghx.CsItem()
        cs.tile, cs.first_x, cs.first_y, cs.edge_size, cs.is_vector, cs.value_kind = tile, 0, 0, C, 0, 1
        one = ctypes.c_int32(nbr)

        def run_new(s):
            _ghx.check(L.ghx_cs_unpack(ctypes.byref(fd), ctypes.byref(cs), field.data_ptr(),
                                       buf.data_ptr(), ctypes.byref(loc[k]), ctypes.byref(glo[k]),
                                       ctypes.byref(one), 1, s), "ghx_cs_unpack")
        # baseline: dims (x', y', z) with the rotated strides, element rows, general addressing
        inv = R.T  # the rotation is orthogonal
        org = inv @ (gf[:2] - shift)  # own-tile cell of buffer cell (0, 0)
        vd = _ghx.FieldDesc()
        vd.dim, vd.elem_size, vd.num_components, vd.has_components = 3, ELEM, 1, 0
        vstr = (int(R[0, 0] * sx + R[0, 1] * sy), int(R[1, 0] * sx + R[1, 1] * sy), sz)
        for d in range(3):
            vd.layout[d], vd.byte_strides[d] = 2 - d, vstr[d]
        e = _ghx.PackEntry()
        e.field, e.field_slot, e.buffer_slot, e.buffer_offset = vd, 0, 0, 0
        vb = _ghx.Box()
        for d in range(3):
            vb.first[d], vb.last[d] = 0, int(bext[d]) - 1
        e.boxes, e.n_boxes = ctypes.pointer(vb), 1
        plan = ctypes.c_void_p()
        _ghx.call("ghx_tune", b"fast_addr", 0)
        try:
            _ghx.call("ghx_plan_create", ctypes.byref(e), 1, 1, ctypes.byref(plan))
        finally:
            _ghx.call("ghx_tune", b"fast_addr", 1)
        seg = _ghx.SegmentInfo()
        _ghx.call("ghx_plan_segment", plan, 0, ctypes.byref(seg))
        assert seg.row_bytes == ELEM and seg.amode == 0, (seg.row_bytes, seg.amode)
        vptr = field.data_ptr() + int((org[0] + HALO) * sx + (org[1] + HALO) * sy + lf[2] * sz)
        fp, bp = _ghx.ptr_array([vptr]), _ghx.ptr_array([buf.data_ptr()])

        def run_base(s):
            _ghx.check(L.ghx_plan_execute(plan, fp, 1, bp, 1, s), "ghx_plan_execute")
        # both verified before any timing
        for what, fn in (("new", run_new), ("baseline", run_base)):
            field.copy_(torch.from_numpy(field_h))
            fn(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert np.array_equal(field.cpu().numpy(), exp), f"{name}: {what} differs from NumPy"
        graphs = {}
        for what, fn in (("new", run_new), ("baseline", run_base)):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(LAUNCHES):
                    fn(torch.cuda.current_stream().cuda_stream)
            g.replay()
            graphs[what] = g
        torch.cuda.synchronize()
        times = {"new": [], "baseline": []}
        for _ in range(ROUNDS):
            for what in ("new", "baseline"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(REPLAYS):
                    graphs[what].replay()
                e1.record()
                e1.synchronize()
                times[what].append(e0.elapsed_time(e1) * 1e3 / (LAUNCHES * REPLAYS))
        L.ghx_plan_destroy(plan)
        new, base = statistics.median(times["new"]), statistics.median(times["baseline"])
        alg = 2 * nbytes
        results.append(dict(orientation=name, tile=tile, neighbour=nbr, box_bytes=nbytes,
                            algorithmic_bytes=alg, new_us=round(new, 3), baseline_us=round(base, 3),
                            new_over_baseline=round(new / base, 3),
                            new_us_all=[round(x, 3) for x in times["new"]],
                            baseline_us_all=[round(x, 3) for x in times["baseline"]],
                            new_fraction_of_hbm_peak=round(alg / (new * 1e-6) / HBM_PEAK, 4),
                            baseline_fraction_of_hbm_peak=round(alg / (base * 1e-6) / HBM_PEAK, 4)))
        print(json.dumps(results[-1]))
    out = dict(what="transformed unpack (k_unpack_x) vs element-row seg_s unpack, per launch, "
                    "graph-replayed back-to-back launches (L2-warm)",
               edge_size=C, levels=LEVELS, halo=HALO, elem_size=ELEM, launches_per_graph=LAUNCHES,
               replays=REPLAYS, rounds=ROUNDS, tune=a.tune, hbm_peak_Bps=HBM_PEAK, device=torch.cuda.get_device_name(0),
               results=results)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
