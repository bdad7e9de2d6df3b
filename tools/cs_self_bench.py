"""Times the fused cubed-sphere self exchange (ghx_cs_exchange_self, one k_self_cs launch) against
the three launches it replaces (ghx_exchange_pack + ghx_exchange_unpack: pack, ordinary unpack,
k_unpack_x).

The rank is FV3-like and holds the whole cube: six tiles of c = 96, 80 levels, halo 3, and per
tile an fp64 scalar and an f32 3-component vector field, x stride-1, all twelve in one exchange.
Both forms are first run once from identical fields and checked bit for bit: every field against
a NumPy expectation (each halo cell's neighbour-tile image, solved from the recorded images of
tests/golden/cubed_sphere_case.json, and the recorded component signs), every send buffer of the
fused form against the baseline's. Timing: each form is captured in a graph of EXCHANGES
back-to-back exchanges, replayed REPLAYS times between two events, the forms alternating for
ROUNDS rounds; the median time per exchange of each is reported with the ratio.

    python tools/cs_self_bench.py [--out profiles/cs_self_bench.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, LEVELS, HALO = 96, 80, 3
FIELDS = [("float64", 1, False), ("float32", 3, True)]
EXCHANGES, REPLAYS, ROUNDS = 10, 20, 7


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "cubed_sphere_case.json")) as fh:
        return {cfg["edge_size"]: cfg for cfg in json.load(fh)}


def solve_transform(cases, tile, nbr):
    """(R, t, o, sign) with T(p, c) = R p + t c + o, from the fixture's images at two edge sizes
    (one domain per tile at c = 70, a row of two at c = 8), and the recorded component signs."""
    found, sign = {}, None
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
                    sign = b["sign"] if sign is None else sign
                    assert sign == b["sign"]
    (R, b70), (R8, b8) = found[70], found[8]
    assert (R == R8).all()
    t = (b70 - b8) // 62
    assert ((b70 - b8) == 62 * t).all()
    return R, t, b8 - 8 * t, sign


def cell_values(dtype, nc, tile, x, y, z, k):
    """The value of global cell (tile, x, y, z, k): its number, exact in f32 (< 2^24)."""
    n = ((((tile * C + x) * C + y) * LEVELS + z) * nc + k) + 1
    assert 6 * C * C * LEVELS * nc < (1 << 24)
    return n.astype(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cs_self_bench.json"))
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE",
                    help="ghx_tune knob set before the plans are made (development A/Bs)")
    a = ap.parse_args()
    import torch
    import ghex_amd
    from ghex_amd import _ghx
    from ghex_amd.structured import cubed_sphere as CS
    ghex_amd.native_library()
    assert torch.cuda.is_available(), "cs_self_bench needs a GPU"
    L = _ghx.lib()
    for kv in a.tune:
        key, value = kv.split("=")
        _ghx.call("ghx_tune", key.encode(), int(value))
    cases = fixture()
    cube = CS.Cube(C, LEVELS)
    ctx = ghex_amd.make_context()
    dds = [CS.DomainDescriptor(cube, t, 0, C - 1, 0, C - 1) for t in range(6)]
    gen = CS.HaloGenerator(HALO)
    pc = CS.make_pattern(ctx, gen, dds)
    E = C + 2 * HALO
    idx = np.arange(C)

    def initial(dtype, nc, tile):
        """Memory order (k, z, y, x): x stride-1. Halos hold -1."""
        a_ = np.full((nc, LEVELS, E, E), -1, dtype=dtype)
        k, z, y, x = np.meshgrid(np.arange(nc), np.arange(LEVELS), idx, idx, indexing="ij")
        a_[:, :, HALO:HALO + C, HALO:HALO + C] = cell_values(dtype, nc, tile, x, y, z, k)
        return a_

    def expected(dtype, nc, vector, tile):
        e = initial(dtype, nc, tile)
        for lf, ll, _, _, t in gen(dds[tile]):
            assert t != tile
            R, tr, o, sign = solve_transform(cases, tile, t)
            k, z, y, x = np.meshgrid(np.arange(nc), np.arange(lf[2], ll[2] + 1),
                                     np.arange(lf[1], ll[1] + 1), np.arange(lf[0], ll[0] + 1),
                                     indexing="ij")
            xn = R[0, 0] * x + R[0, 1] * y + tr[0] * C + o[0]
            yn = R[1, 0] * x + R[1, 1] * y + tr[1] * C + o[1]
            assert xn.min() >= 0 and xn.max() < C and yn.min() >= 0 and yn.max() < C
            v = cell_values(dtype, nc, t, xn, yn, z, k)
            if vector:
                for comp in (0, 1):
                    if sign[comp] < 0:
                        v[comp] = -v[comp]
            e[:, lf[2]:ll[2] + 1, lf[1] + HALO:ll[1] + HALO + 1, lf[0] + HALO:ll[0] + HALO + 1] = v
        return e

    def make(**options):
        co = CS.make_communication_object(ctx, **options)
        bis, bases, init = [], [], []
        for dtype, nc, vector in FIELDS:
            for t in range(6):
                h = initial(dtype, nc, t)
                base = torch.from_numpy(h).cuda()
                logical = base.permute(3, 2, 1, 0)  # (x, y, z, k)
                bis.append(pc(CS.FieldDescriptor(dds[t], logical, (HALO, HALO, 0), (E, E, LEVELS),
                                                 nc, vector)))
                bases.append(base)
                init.append(h)
        plan = co.plan(bis)
        send, recv = co.buffers(plan, bases[0].device)
        fp = _ghx.ptr_array([bi.field.data_ptr() for bi in bis])
        sp = _ghx.ptr_array([t.data_ptr() for t in send])
        rp = _ghx.ptr_array([t.data_ptr() for t in recv])
        return dict(co=co, bis=bis, bases=bases, init=init, plan=plan, send=send, recv=recv, fp=fp,
                    sp=sp, rp=rp)

    new, base = make(fuse_rotated=True), make(fuse_self=False)
    assert new["co"].cs_self(new["plan"]), _ghx.lib().ghx_last_error()
    info = [ctypes.c_int32() for _ in range(4)]
    _ghx.call("ghx_cs_self_info", new["plan"].h, *[ctypes.byref(i) for i in info])

    def run_new(s):
        m = new
        _ghx.check(L.ghx_cs_exchange_self(m["plan"].h, m["fp"], len(m["bis"]), m["sp"],
                                          len(m["send"]), s), "ghx_cs_exchange_self")

    def run_base(s):
        m = base
        _ghx.check(L.ghx_exchange_pack(m["plan"].h, m["fp"], len(m["bis"]), m["sp"],
                                       len(m["send"]), s), "ghx_exchange_pack")
        _ghx.check(L.ghx_exchange_unpack(m["plan"].h, m["fp"], len(m["bis"]), m["rp"],
                                         len(m["recv"]), s), "ghx_exchange_unpack")
    forms = {"new": (new, run_new), "baseline": (base, run_base)}
    # both verified before any timing; the baseline's launches counted
    launches = {}
    ms, n = (ctypes.c_float * 16)(), ctypes.c_int32()
    for what, (m, fn) in forms.items():
        _ghx.call("ghx_launch_timing", 1)
        try:
            fn(torch.cuda.current_stream().cuda_stream)
            _ghx.call("ghx_launch_timing_read", ms, 16, ctypes.byref(n))
        finally:
            _ghx.call("ghx_launch_timing", 0)
        launches[what] = n.value
        torch.cuda.synchronize()
        i = 0
        for dtype, nc, vector in FIELDS:
            for t in range(6):
                got = m["bases"][i].cpu().numpy()
                exp = expected(dtype, nc, vector, t)
                u = np.uint64 if dtype == "float64" else np.uint32
                assert np.array_equal(got.view(u), exp.view(u)), f"{what}: {dtype} tile {t} differs"
                i += 1
    for i, (x, y) in enumerate(zip(new["send"], base["send"])):
        assert torch.equal(x, y), f"send buffer {i} differs between the forms"
    halo_bytes = sum(x["size"] for x in new["plan"].send)
    graphs = {}
    for what, (m, fn) in forms.items():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(EXCHANGES):
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
            times[what].append(e0.elapsed_time(e1) * 1e3 / (EXCHANGES * REPLAYS))
    tn, tb = statistics.median(times["new"]), statistics.median(times["baseline"])
    out = dict(what="fused cubed-sphere self exchange (ghx_cs_exchange_self, one launch) vs "
                    "ghx_exchange_pack + ghx_exchange_unpack (three launches), per exchange, "
                    "graph-replayed back-to-back exchanges (L2-warm)",
               edge_size=C, levels=LEVELS, halo=HALO, tiles=6,
               fields=[dict(dtype=d, components=nc, vector=v) for d, nc, v in FIELDS],
               message_bytes=halo_bytes, launches=launches,
               self_plan=dict(fusable=info[0].value, pair_tiles=info[1].value,
                              self_records=info[2].value, self_tiles=info[3].value),
               verified=dict(new=True, baseline=True, buffers_equal=True),
               exchanges_per_graph=EXCHANGES, replays=REPLAYS, rounds=ROUNDS, tune=a.tune,
               device=torch.cuda.get_device_name(0),
               new_us=round(tn, 3), baseline_us=round(tb, 3), new_over_baseline=round(tn / tb, 3),
               new_us_all=[round(x, 3) for x in times["new"]],
               baseline_us_all=[round(x, 3) for x in times["baseline"]])
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
