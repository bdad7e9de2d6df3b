"""Times the fused adjoint of a cubed-sphere exchange whose every message is a self message
(ghx_cs_exchange_adjoint_self_accumulate: ONE k_accum_get_x launch with zero_halos; its pack launches
nothing) against the unfused adjoint of the same exchange (ghx_cs_exchange_adjoint_pack: the ordinary
reverse pack and k_pack_x, then ghx_cs_exchange_adjoint_accumulate: k_accum_s) and against the
forward launches (ghx_exchange_pack + ghx_exchange_unpack).

The geometry and the method are tools/cs_adjoint_bench.py's: one rank holds the whole cube, six tiles
of c = 96, 80 levels, halo 3, and per tile an fp64 scalar and an f32 3-component vector field, x
stride-1, all twelve in one exchange. Every form is first run once from identical integer-valued
fields and checked on every cell: the forward form against the NumPy expectation, both adjoints
against the NumPy adjoint built from the solved transforms. Timing: each form is captured in a graph
of EXCHANGES back-to-back runs, replayed REPLAYS times between two events, the forms alternating for
ROUNDS rounds; medians, every round's figure, the range of the fused / unfused and fused / forward
ratios over the rounds and the bytes each form must move are reported.

    python tools/cs_adjoint_self_bench.py [--out profiles/cs_adjoint_self_bench.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cs_adjoint_bench import values  # noqa: E402
from cs_self_bench import C, FIELDS, HALO, LEVELS, fixture, solve_transform  # noqa: E402

EXCHANGES, REPLAYS, ROUNDS = 10, 20, 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cs_adjoint_self_bench.json"))
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE",
                    help="ghx_tune knob set before the plans are made (development A/Bs)")
    a = ap.parse_args()
    import torch
    import ghex_amd
    from ghex_amd import _ghx
    from ghex_amd.structured import cubed_sphere as CS
    ghex_amd.native_library()
    assert torch.cuda.is_available(), "cs_adjoint_self_bench needs a GPU"
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
    boxes = {t: gen(dds[t]) for t in range(6)}
    xf = {(t, b[4]): solve_transform(cases, t, b[4]) for t in range(6) for b in boxes[t]}

    def box_cells(nc, tile, b):
        """Index arrays (memory order k, z, y, x) of box b's halo cells in tile's field, of their
        owner cells in tile b[4]'s field, and the component signs."""
        lf, ll, _, _, t = b
        R, tr, o, sign = xf[(tile, t)]
        k, z, y, x = np.meshgrid(np.arange(nc), np.arange(lf[2], ll[2] + 1), np.arange(lf[1], ll[1] + 1),
                                 np.arange(lf[0], ll[0] + 1), indexing="ij")
        xn = R[0, 0] * x + R[0, 1] * y + tr[0] * C + o[0]
        yn = R[1, 0] * x + R[1, 1] * y + tr[1] * C + o[1]
        assert xn.min() >= 0 and xn.max() < C and yn.min() >= 0 and yn.max() < C
        return (k, z, y + HALO, x + HALO), (k, z, yn + HALO, xn + HALO), sign

    def forward_of(state, nc, vector):
        out = [s.copy() for s in state]
        for tile in range(6):
            for b in boxes[tile]:
                halo, own, sign = box_cells(nc, tile, b)
                v = state[b[4]][own]
                if vector:
                    for comp in (0, 1):
                        if sign[comp] < 0:
                            v[comp] = -v[comp]
                out[tile][halo] = v
        return out

    def adjoint_of(state, nc, vector):
        out = [s.copy() for s in state]
        for tile in range(6):
            for b in boxes[tile]:
                halo, own, sign = box_cells(nc, tile, b)
                v = state[tile][halo]
                if vector:
                    for comp in (0, 1):
                        if sign[comp] < 0:
                            v[comp] = -v[comp]
                np.add.at(out[b[4]], own, v)
        for tile in range(6):
            for b in boxes[tile]:
                out[tile][box_cells(nc, tile, b)[0]] = 0
        return out

    co = CS.make_communication_object(ctx, fuse_self=False, adjoint_rotated=True)
    bis, bases, init = [], [], []
    for dtype, nc, vector in FIELDS:
        for t in range(6):
            h = values(dtype, nc, t, (nc, LEVELS, E, E), 0)
            base = torch.from_numpy(h).cuda()
            fd = CS.FieldDescriptor(dds[t], base.permute(3, 2, 1, 0), (HALO, HALO, 0), (E, E, LEVELS), nc, vector)
            bis.append(pc(fd))
            bases.append(base)
            init.append(h)
    plan = co._adjoint_plan(bis)  # the unfused plans; the fused ones beside them on the same exchange
    codes = [bi.field.dtype_code() for bi in bis]
    _ghx.call("ghx_cs_exchange_adjoint_self_create", plan.h, _ghx.i32_array(codes), len(codes))
    send, recv = co.buffers(plan, bases[0].device)
    fp = _ghx.ptr_array([bi.field.data_ptr() for bi in bis])
    sp = _ghx.ptr_array([t.data_ptr() for t in send])
    rp = _ghx.ptr_array([t.data_ptr() for t in recv])
    assert len(bis) == 12 and len(send) == 24 and len(recv) == 24

    def run_forward(s):
        _ghx.check(L.ghx_exchange_pack(plan.h, fp, len(bis), sp, len(send), s), "ghx_exchange_pack")
        _ghx.check(L.ghx_exchange_unpack(plan.h, fp, len(bis), rp, len(recv), s), "ghx_exchange_unpack")

    def run_unfused(s):
        _ghx.check(L.ghx_cs_exchange_adjoint_pack(plan.h, fp, len(bis), rp, len(recv), s),
                   "ghx_cs_exchange_adjoint_pack")
        _ghx.check(L.ghx_cs_exchange_adjoint_accumulate(plan.h, fp, len(bis), sp, len(send), 1, s),
                   "ghx_cs_exchange_adjoint_accumulate")

    def run_fused(s):
        _ghx.check(L.ghx_cs_exchange_adjoint_self_pack(plan.h, fp, len(bis), rp, len(recv), s),
                   "ghx_cs_exchange_adjoint_self_pack")
        _ghx.check(L.ghx_cs_exchange_adjoint_self_accumulate(plan.h, fp, len(bis), sp, len(send), 1, s),
                   "ghx_cs_exchange_adjoint_self_accumulate")

    def reload():
        for base, h in zip(bases, init):
            base.copy_(torch.from_numpy(h))
        torch.cuda.synchronize()

    def launches_of(fn):
        ms, n = (ctypes.c_float * 64)(), ctypes.c_int32()
        _ghx.call("ghx_launch_timing", 1)
        try:
            fn(torch.cuda.current_stream().cuda_stream)
            _ghx.call("ghx_launch_timing_read", ms, 64, ctypes.byref(n))
        finally:
            _ghx.call("ghx_launch_timing", 0)
        torch.cuda.synchronize()
        return n.value

    def check(want_of, what):
        i = 0
        for dtype, nc, vector in FIELDS:
            want = want_of(init[i:i + 6], nc, vector)
            for t in range(6):
                got = bases[i].cpu().numpy()
                u = np.uint64 if dtype == "float64" else np.uint32
                assert np.array_equal(got.view(u), want[t].view(u)), f"{what}: {dtype} tile {t} differs"
                i += 1

    # every form verified on every cell before any timing; its launches counted
    forms = {"fused": run_fused, "unfused": run_unfused, "forward": run_forward}
    launches = {}
    for what, fn in forms.items():
        reload()
        launches[what] = launches_of(fn)
        check(forward_of if what == "forward" else adjoint_of, what)
    assert launches["fused"] == 1, launches

    # bytes each form must move, from the shapes
    M = sum(x["size"] for x in plan.send)
    acc = ctypes.c_void_p()
    _ghx.call("ghx_cs_exchange_adjoint_self_plan", plan.h, ctypes.byref(acc))
    nb = ctypes.c_int64()
    _ghx.call("ghx_saccum_info", acc, None, ctypes.byref(nb), None, None, None, None)
    U = 0
    for k in range(nb.value):
        bx = _ghx.SAccumBoxInfo()
        _ghx.call("ghx_saccum_box", acc, k, ctypes.byref(bx))
        dtype, nc, _ = FIELDS[bx.field_slot // 6]
        U += int(np.prod([bx.last[d] - bx.first[d] + 1 for d in range(3)])) * nc * np.dtype(dtype).itemsize
    form = ctypes.c_int32()
    info = [ctypes.c_int64() for _ in range(4)]
    _ghx.call("ghx_cs_exchange_adjoint_self_info", plan.h, ctypes.byref(form), *[ctypes.byref(i) for i in info])
    assert form.value == 1

    graphs = {}
    for what, fn in forms.items():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(EXCHANGES):
                fn(torch.cuda.current_stream().cuda_stream)
        g.replay()
        graphs[what] = g
    torch.cuda.synchronize()
    times = {what: [] for what in forms}
    for _ in range(ROUNDS):
        for what in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPLAYS):
                graphs[what].replay()
            e1.record()
            e1.synchronize()
            times[what].append(e0.elapsed_time(e1) * 1e3 / (EXCHANGES * REPLAYS))
    med = {what: statistics.median(v) for what, v in times.items()}
    over_unfused = [round(x / y, 3) for x, y in zip(times["fused"], times["unfused"])]
    over_forward = [round(x / y, 3) for x, y in zip(times["fused"], times["forward"])]
    out = dict(what="fused adjoint of a cubed-sphere exchange (one k_accum_get_x launch with zero_halos) vs the "
                    "unfused adjoint (reverse pack + k_pack_x + k_accum_s) vs the forward launches of the same "
                    "exchange (ghx_exchange_pack + ghx_exchange_unpack), per run, graph-replayed back-to-back "
                    "runs (L2-warm); one rank, self messages only: nothing between GPUs is measured",
               edge_size=C, levels=LEVELS, halo=HALO, tiles=6,
               fields=[dict(dtype=d, components=nc, vector=v) for d, nc, v in FIELDS],
               field_slots=len(bis), buffers=len(send), launches=launches,
               fused_plan=dict(form=form.value, sum_boxes=info[0].value, sources=info[1].value,
                               field_sources=info[2].value, rotated_sources=info[3].value),
               bytes=dict(message=M, summed_cells=U, forward_must_move=4 * M, unfused_must_move=4 * M + 2 * U,
                          fused_must_move=2 * M + 2 * U,
                          note="forward: pack reads M and writes M, unpack reads M and writes M. unfused: reverse "
                               "pack reads M and writes M, accumulate reads M from the buffers, reads and writes "
                               "the U bytes of the cells it sums into, and writes M zero bytes. fused: reads M "
                               "from the halos, reads and writes U, writes M zero bytes"),
               verified=dict(forward=True, unfused=True, fused=True),
               exchanges_per_graph=EXCHANGES, replays=REPLAYS, rounds=ROUNDS, tune=a.tune,
               device=torch.cuda.get_device_name(0),
               median_us={k: round(v, 3) for k, v in med.items()},
               fused_over_unfused=round(med["fused"] / med["unfused"], 3),
               fused_over_unfused_range=[min(over_unfused), max(over_unfused)],
               fused_over_forward=round(med["fused"] / med["forward"], 3),
               fused_over_forward_range=[min(over_forward), max(over_forward)],
               ratios_per_round=dict(fused_over_unfused=over_unfused, fused_over_forward=over_forward),
               us_all={k: [round(x, 3) for x in v] for k, v in times.items()})
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
