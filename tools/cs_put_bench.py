"""Times the cubed-sphere put exchange (structured.cubed_sphere.make_bulk_communication_object:
ghx_cs_put_create plans, one k_put_cs launch each, no buffers) against the two buffered forms of
the same exchange on the same box in the same run: the three launches of ghx_exchange_pack +
ghx_exchange_unpack (pack, ordinary unpack, k_unpack_x) and the one launch of
ghx_cs_exchange_self (k_self_cs).

Geometry and method are tools/cs_self_bench.py's: one rank holding the whole cube, six tiles of
c = 96, 80 levels, halo 3, per tile an fp64 scalar and an f32 3-component vector field, x
stride-1, all twelve in one exchange. Every form is first run once from identical fields and
checked bit for bit against the NumPy expectation. Timing: each form is captured in a graph of
EXCHANGES back-to-back exchanges, replayed REPLAYS times between two events, the forms
alternating for ROUNDS rounds; the median time per exchange of each is reported. Per message
byte the put moves 2 bytes (field -> field), k_self_cs 3 (field -> buffer and -> field), the
three launches 4 (field -> buffer, buffer -> field).

    python tools/cs_put_bench.py [--out profiles/cs_put_bench.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.cs_self_bench import (C, EXCHANGES, FIELDS, HALO, LEVELS, REPLAYS, ROUNDS,  # noqa: E402
                                 cell_values, fixture, solve_transform)

FORMS = ("put", "self", "baseline")
BYTES_PER_MESSAGE_BYTE = {"put": 2, "self": 3, "baseline": 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cs_put_bench.json"))
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE",
                    help="ghx_tune knob set before the plans are made (development A/Bs)")
    a = ap.parse_args()
    import torch
    import ghex_amd
    from ghex_amd import _ghx
    from ghex_amd.structured import cubed_sphere as CS
    ghex_amd.native_library()
    assert torch.cuda.is_available(), "cs_put_bench needs a GPU"
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

    def fields():
        bis, bases = [], []
        for dtype, nc, vector in FIELDS:
            for t in range(6):
                base = torch.from_numpy(initial(dtype, nc, t)).cuda()
                logical = base.permute(3, 2, 1, 0)  # (x, y, z, k)
                bis.append(pc(CS.FieldDescriptor(dds[t], logical, (HALO, HALO, 0), (E, E, LEVELS),
                                                 nc, vector)))
                bases.append(base)
        return bis, bases

    def make_buffered(**options):
        co = CS.make_communication_object(ctx, **options)
        bis, bases = fields()
        plan = co.plan(bis)
        send, recv = co.buffers(plan, bases[0].device)
        fp = _ghx.ptr_array([bi.field.data_ptr() for bi in bis])
        sp = _ghx.ptr_array([t.data_ptr() for t in send])
        rp = _ghx.ptr_array([t.data_ptr() for t in recv])
        return dict(co=co, bis=bis, bases=bases, plan=plan, send=send, recv=recv, fp=fp, sp=sp, rp=rp)

    def make_put():
        bco = CS.make_bulk_communication_object(ctx)
        bis, bases = fields()
        bco.add_fields(*bis)
        bco.init()
        assert bco._ep is None and bco._co is None  # one rank: the put launches and nothing else
        return dict(bco=bco, bis=bis, bases=bases)

    put, fused, base = make_put(), make_buffered(fuse_rotated=True), make_buffered(fuse_self=False)
    assert fused["co"].cs_self(fused["plan"]), L.ghx_last_error()

    def run_put(s):
        for h, sp, ns, dp, nd in put["bco"]._puts:
            _ghx.check(L.ghx_put_execute(h, sp, ns, dp, nd, s), "ghx_put_execute")

    def run_self(s):
        m = fused
        _ghx.check(L.ghx_cs_exchange_self(m["plan"].h, m["fp"], len(m["bis"]), m["sp"],
                                          len(m["send"]), s), "ghx_cs_exchange_self")

    def run_base(s):
        m = base
        _ghx.check(L.ghx_exchange_pack(m["plan"].h, m["fp"], len(m["bis"]), m["sp"],
                                       len(m["send"]), s), "ghx_exchange_pack")
        _ghx.check(L.ghx_exchange_unpack(m["plan"].h, m["fp"], len(m["bis"]), m["rp"],
                                         len(m["recv"]), s), "ghx_exchange_unpack")
    forms = {"put": (put, run_put), "self": (fused, run_self), "baseline": (base, run_base)}
    # every form verified before any timing, its launches counted
    launches = {}
    ms, n = (ctypes.c_float * 64)(), ctypes.c_int32()
    for what, (m, fn) in forms.items():
        _ghx.call("ghx_launch_timing", 1)
        try:
            fn(torch.cuda.current_stream().cuda_stream)
            _ghx.call("ghx_launch_timing_read", ms, 64, ctypes.byref(n))
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
    message_bytes = sum(x["size"] for x in fused["plan"].send)
    assert put["bco"].bytes_per_exchange() == message_bytes
    plans = []
    for h, *_ in put["bco"]._puts:
        p, r, x = (ctypes.c_int32() for _ in range(3))
        _ghx.call("ghx_cs_put_info", h, ctypes.byref(p), ctypes.byref(r), ctypes.byref(x))
        plans.append(dict(pair_tiles=p.value, put_records=r.value, put_tiles=x.value))
    graphs = {}
    for what, (m, fn) in forms.items():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(EXCHANGES):
                fn(torch.cuda.current_stream().cuda_stream)
        g.replay()
        graphs[what] = g
    torch.cuda.synchronize()
    times = {what: [] for what in FORMS}
    for _ in range(ROUNDS):
        for what in FORMS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPLAYS):
                graphs[what].replay()
            e1.record()
            e1.synchronize()
            times[what].append(e0.elapsed_time(e1) * 1e3 / (EXCHANGES * REPLAYS))
    med = {what: statistics.median(times[what]) for what in FORMS}
    out = dict(what="cubed-sphere put exchange (one k_put_cs launch per put plan, no buffers) vs "
                    "ghx_cs_exchange_self (one launch) and ghx_exchange_pack + ghx_exchange_unpack "
                    "(three launches), per exchange, graph-replayed back-to-back exchanges (L2-warm), "
                    "all measured in this run",
               edge_size=C, levels=LEVELS, halo=HALO, tiles=6,
               fields=[dict(dtype=d, components=nc, vector=v) for d, nc, v in FIELDS],
               message_bytes=message_bytes, launches=launches,
               bytes_moved={what: BYTES_PER_MESSAGE_BYTE[what] * message_bytes for what in FORMS},
               put_plans=plans,
               verified={what: True for what in FORMS},
               exchanges_per_graph=EXCHANGES, replays=REPLAYS, rounds=ROUNDS, tune=a.tune,
               device=torch.cuda.get_device_name(0),
               us={what: round(med[what], 3) for what in FORMS},
               put_over_self=round(med["put"] / med["self"], 3),
               put_over_baseline=round(med["put"] / med["baseline"], 3),
               us_all={what: [round(x, 3) for x in times[what]] for what in FORMS})
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
