"""Times the adjoint halo exchange of index lists — the reverse pack (a ghx_uplan of direction 0
over the RECEIVE lists) and the accumulate (ghx_uaccum_create, one k_accum_u launch) — against the
forward exchange's pack and unpack launches over the same lists, on the same box in the same run.

Geometry: BASELINE config 5's generator (tools/config5_gen.cpp: 10M owned cells per rank, 5 %
halo cells drawn from the other ranks, permuted storage) for TWO ranks, both ranks' fields on
the one GPU; the lists are those of the product's make_pattern<unstructured> (bench.py's
config5_patterns). fp64, levels first, at levels 1 (8-byte rows) and levels 8 (64-byte rows). An
exchange moves both ranks' halos:
  forward   one pack launch per rank into its send buffers, then one unpack launch per rank
            straight from the peer's send buffers
  adjoint   one reverse-pack launch per rank (halo cells -> its receive buffers), then one
            accumulate launch per rank that reads its contributions straight from the peer's
            receive buffers, adds them to the owner cells and zeroes its halo cells
(no transport step between the launches of either form: on one GPU there is none to time).
Both forms are first run once and checked bit for bit: the forward exchange against the owners'
values, the adjoint (from fields whose halos hold their owners' values) against value * (1 +
number of halo copies of the cell) in the owner cells and zero in the halos. Timing: each form is
captured in a graph of EXCHANGES back-to-back exchanges, replayed REPLAYS times between two
events, the forms alternating for ROUNDS rounds; the median time per exchange of each and the
ratio are reported. The kernel's register count comes from the compiler's resource-usage remarks
(--resource-usage FILE: the saved output of hipcc -Rpass-analysis=kernel-resource-usage on
ghx_accum.hip; without it the tool compiles the file's device code itself). One GPU only: the
adjoint has not run between GPUs.

    python tools/uaccum_bench.py [--out profiles/uaccum_bench.json]"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXCHANGES, REPLAYS, ROUNDS = 10, 20, 9
FORMS = ("adjoint", "forward")


def resource_usage(path=None):
    """VGPRs, scratch bytes per lane and occupancy of k_accum_u from the compiler's remarks."""
    if path:
        with open(path) as fh:
            text = fh.read()
    else:
        src = os.path.join(ROOT, "ghex_amd", "csrc", "ghx_accum.hip")
        with tempfile.TemporaryDirectory() as tmp:
            text = subprocess.run(
                [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O3", "-I" + os.path.join(ROOT, "include"),
                 "--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                 "-o", os.path.join(tmp, "accum.o")], check=True, capture_output=True, text=True).stderr
    at = text.index("k_accum_u")
    def num(key):
        return int(re.search(key + r"[^:]*: (\d+)", text[at:]).group(1))
    return dict(vgprs=num("VGPRs"), scratch_bytes_per_lane=num("ScratchSize"), waves_per_simd=num("Occupancy"))


def measure(torch, _ghx, pats, levels, cells):
    L = _ghx.lib()
    dev = torch.device("cuda", 0)
    world = len(pats)
    copies = {}
    for gids, outer, _, _ in pats:
        g, c = np.unique(gids[outer], return_counts=True)
        for a, b in zip(g, c):
            copies[int(a)] = copies.get(int(a), 0) + int(b)
    want, init, awant = [], [], []
    for gids, outer, _, _ in pats:
        host = gids.astype(np.float64)[:, None] * 100.0 + np.arange(levels, dtype=np.float64)[None, :]
        w = torch.from_numpy(host).to(dev)
        i = w.clone()
        i[torch.from_numpy(outer).to(dev)] = -1.0
        want.append(w)
        init.append(i)
        mult = np.array([1 + copies.get(int(g), 0) for g in gids], dtype=np.float64)[:, None]
        a = host * mult
        a[outer] = 0.0
        awant.append(torch.from_numpy(a).to(dev))
    # the adjoint starts from exchanged fields: every halo cell holds its owner's value
    fields = {"forward": [t.clone() for t in init], "adjoint": [t.clone() for t in want]}

    def desc():
        d = _ghx.UDataDesc()
        d.elem_size, d.levels, d.levels_first, d.index_stride, d.level_stride = 8, levels, 1, levels, 1
        return d

    keep = []

    def entries(lists):
        ents = (_ghx.UPackEntry * len(lists))()
        for k, (_, _, _, l) in enumerate(lists):
            arr = np.ascontiguousarray(l, dtype=np.int64)
            keep.append(arr)
            e = ents[k]
            e.data, e.field_slot, e.buffer_slot, e.buffer_offset = desc(), 0, k, 0
            e.lids, e.n_lids = _ghx.i64_ptr(arr), arr.size
        return ents

    def uplan(lists, direction):
        h = ctypes.c_void_p()
        _ghx.call("ghx_uplan_create", entries(lists), len(lists), direction, ctypes.byref(h))
        return h

    def nbytes(l):
        return len(l) * levels * 8

    sbufs = [[torch.empty(nbytes(l), dtype=torch.uint8, device=dev) for *_, l in sends] for _, _, sends, _ in pats]
    rbufs = [[torch.empty(nbytes(l), dtype=torch.uint8, device=dev) for *_, l in recvs] for _, _, _, recvs in pats]
    packs, unpacks, rpacks, accums, infos = [], [], [], [], []
    message_bytes = 0
    for r, (_, _, sends, recvs) in enumerate(pats):
        ff = _ghx.ptr_array([fields["forward"][r].data_ptr()])
        fa = _ghx.ptr_array([fields["adjoint"][r].data_ptr()])
        packs.append((uplan(sends, 0), ff, _ghx.ptr_array([b.data_ptr() for b in sbufs[r]]), len(sends)))
        from_peers = []
        for rid, rr, tag, lids in recvs:
            j = next(j for j, (i, q, tg, l) in enumerate(pats[rr][2]) if q == r and tg == tag)
            from_peers.append(sbufs[rr][j].data_ptr())
        unpacks.append((uplan(recvs, 1), ff, _ghx.ptr_array(from_peers), len(recvs)))
        # adjoint: the halo cells into this rank's receive buffers ...
        rpacks.append((uplan(recvs, 0), fa, _ghx.ptr_array([b.data_ptr() for b in rbufs[r]]), len(recvs)))
        # ... and the contributions to this rank's owner cells from the peers' receive buffers
        back = []
        for rid, rr, tag, lids in sends:
            j = next(j for j, (i, q, tg, l) in enumerate(pats[rr][3]) if q == r and tg == tag)
            assert len(pats[rr][3][j][3]) == len(lids)
            back.append(rbufs[rr][j].data_ptr())
            message_bytes += nbytes(lids)
        h = ctypes.c_void_p()
        _ghx.call("ghx_uaccum_create", entries(sends), _ghx.i32_array([_ghx.DT_F64] * len(sends)), len(sends),
                  entries(recvs), len(recvs), ctypes.byref(h))
        accums.append((h, fa, _ghx.ptr_array(back), len(sends)))
        b, t = ctypes.c_uint64(), ctypes.c_int32()
        v = [ctypes.c_int64() for _ in range(4)]
        _ghx.call("ghx_uaccum_info", h, ctypes.byref(b), *[ctypes.byref(x) for x in v], ctypes.byref(t))
        infos.append(dict(bytes=b.value, n_dest=v[0].value, n_zero_dest=v[1].value, n_contrib=v[2].value,
                          max_per_dest=v[3].value, n_tiles=t.value))

    def run_forward(s):
        for h, fp, bp, nb in packs:
            _ghx.check(L.ghx_uplan_execute(h, fp, 1, bp, nb, s), "uplan pack")
        for h, fp, bp, nb in unpacks:
            _ghx.check(L.ghx_uplan_execute(h, fp, 1, bp, nb, s), "uplan unpack")

    def run_adjoint(s):
        for h, fp, bp, nb in rpacks:
            _ghx.check(L.ghx_uplan_execute(h, fp, 1, bp, nb, s), "reverse pack")
        for h, fp, bp, nb in accums:
            _ghx.check(L.ghx_uaccum_execute(h, fp, 1, bp, nb, 1, s), "ghx_uaccum_execute")
    run = {"forward": run_forward, "adjoint": run_adjoint}
    expect = {"forward": want, "adjoint": awant}
    for what in FORMS:  # every form verified before any timing
        run[what](torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for r in range(world):
            assert torch.equal(fields[what][r].view(torch.int64), expect[what][r].view(torch.int64)), (what, r)
    graphs = {}
    for what in FORMS:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(EXCHANGES):
                run[what](torch.cuda.current_stream().cuda_stream)
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
    del graphs
    for h, *_ in packs + unpacks + rpacks:
        L.ghx_uplan_destroy(h)
    for h, *_ in accums:
        L.ghx_uaccum_destroy(h)
    med = {what: statistics.median(times[what]) for what in FORMS}
    return dict(levels=levels, row_bytes=levels * 8, cells_per_rank=cells, ranks=world,
                message_bytes=message_bytes, launches={what: 2 * world for what in FORMS},
                n_dest=sum(i["n_dest"] for i in infos), n_zero_dest=sum(i["n_zero_dest"] for i in infos),
                n_contrib=sum(i["n_contrib"] for i in infos), max_per_dest=max(i["max_per_dest"] for i in infos),
                accumulate_tiles=[i["n_tiles"] for i in infos], verified={what: True for what in FORMS},
                us={what: round(med[what], 3) for what in FORMS},
                adjoint_over_forward=round(med["adjoint"] / med["forward"], 3),
                us_all={what: [round(x, 3) for x in times[what]] for what in FORMS})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uaccum_bench.json"))
    ap.add_argument("--cells", type=int, default=None, help="owned cells per rank (default: config 5's 10M)")
    ap.add_argument("--resource-usage", default=None, metavar="FILE",
                    help="saved kernel-resource-usage remarks of ghx_accum.hip (default: compile it now)")
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE",
                    help="ghx_tune knob set before the plans are made (development A/Bs)")
    a = ap.parse_args()
    import torch
    import ghex_amd
    from ghex_amd import _ghx
    import bench
    from tools import config5 as C5
    ghex_amd.native_library()
    assert torch.cuda.is_available(), "uaccum_bench needs a GPU"
    usage = resource_usage(a.resource_usage)
    cells = C5.CELLS if a.cells is None else a.cells
    pats, _, _ = bench.config5_patterns(world=2, cells=cells)
    results = []
    for levels in (1, 8):
        try:
            for kv in a.tune:
                key, value = kv.split("=")
                _ghx.call("ghx_tune", key.encode(), int(value))
            results.append(measure(torch, _ghx, pats, levels, cells))
        finally:
            _ghx.call("ghx_tune", b"reset", 0)
    out = dict(what="adjoint index-list exchange (reverse pack + k_accum_u accumulate, the accumulate reading the "
                    "peer's receive buffers) vs the forward exchange's fused pack + unpack launches of the same "
                    "lists (unpacking straight from the peer's send buffers), two config-5 ranks' fields on one "
                    "GPU, per exchange of both ranks' halos, graph-replayed back-to-back exchanges (L2-warm), "
                    "all measured in this run",
               between_gpus="not measured: the adjoint has not run between GPUs",
               k_accum_u=usage, exchanges_per_graph=EXCHANGES, replays=REPLAYS, rounds=ROUNDS, tune=a.tune,
               device=torch.cuda.get_device_name(0), results=results)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
