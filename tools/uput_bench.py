"""Times the index-list put (ghx_uput_create, one k_put_u launch per rank, no buffers) against
the buffered form of the same exchange — the fused ghx_uplan pack and unpack launches over the
same lists — on the same box in the same run.

Geometry: BASELINE config 5's generator (tools/config5_gen.cpp: 10M owned cells per rank, 5 %
halo cells drawn from the other ranks, permuted storage) for TWO ranks, both ranks' fields on
the one GPU; the lists are those of the product's make_pattern<unstructured> (bench.py's
config5_patterns). fp64, levels first, at levels 1 (8-byte rows: request-bound, the run path) and
levels 8 (64-byte rows). An exchange moves both ranks' halos:
  put       one launch per rank: send list on the sender's field -> receive list on the
            receiver's field
  buffered  one pack launch per rank into its send buffer, then one unpack launch per rank
            straight from the peer's send buffer (no transport step between them: on one GPU
            there is none to time, which favours this form)
Both forms are first run once from identical fields and checked bit for bit: against the owners'
values and against each other. Timing: each form is captured in a graph of EXCHANGES back-to-back
exchanges, replayed REPLAYS times between two events, the forms alternating for ROUNDS rounds;
the median time per exchange of each and the ratio are reported, at levels 1 also with the run
path off (knob urun = 0, plans of both forms rebuilt). One GPU only: the put has not run between
GPUs, where it also removes the transport step.

    python tools/uput_bench.py [--out profiles/uput_bench.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXCHANGES, REPLAYS, ROUNDS = 10, 20, 9
FORMS = ("put", "buffered")


def measure(torch, _ghx, pats, levels, cells):
    """One configuration under the knobs as they are set now: plans of both forms, the bit-exact
    check, the alternating timing."""
    L = _ghx.lib()
    dev = torch.device("cuda", 0)
    world = len(pats)
    want, init = [], []
    for gids, outer, _, _ in pats:
        host = gids.astype(np.float64)[:, None] * 100.0 + np.arange(levels, dtype=np.float64)[None, :]
        w = torch.from_numpy(host).to(dev)
        i = w.clone()
        i[torch.from_numpy(outer).to(dev)] = -1.0
        want.append(w)
        init.append(i)
    fields = {what: [t.clone() for t in init] for what in FORMS}

    def desc():
        d = _ghx.UDataDesc()
        d.elem_size, d.levels, d.levels_first, d.index_stride, d.level_stride = 8, levels, 1, levels, 1
        return d

    keep = []
    # put: per rank its send lists paired with the receivers' receive lists of the same tag
    puts, message_bytes = [], 0
    for r, (_, _, sends, _) in enumerate(pats):
        n = len(sends)
        src, dst = (_ghx.UPutEntry * n)(), (_ghx.UPutEntry * n)()
        targets = []
        for k, (rid, rr, tag, lids) in enumerate(sends):
            tl = next(l for (i, q, tg, l) in pats[rr][3] if q == r and tg == tag)
            assert len(tl) == len(lids)
            if rr not in targets:
                targets.append(rr)
            for e, slot, arr in ((src[k], 0, lids), (dst[k], targets.index(rr), tl)):
                arr = np.ascontiguousarray(arr, dtype=np.int64)
                keep.append(arr)
                e.data, e.field_slot, e.lids, e.n_lids = desc(), slot, _ghx.i64_ptr(arr), arr.size
            message_bytes += len(lids) * levels * 8
        h = ctypes.c_void_p()
        _ghx.call("ghx_uput_create", src, dst, n, ctypes.byref(h))
        puts.append((h, _ghx.ptr_array([fields["put"][r].data_ptr()]), 1,
                     _ghx.ptr_array([fields["put"][q].data_ptr() for q in targets]), len(targets)))

    # buffered: the fused pack and unpack plans of every rank, unpacking from the peers' send buffers
    def uplan(lists, direction):
        ents = (_ghx.UPackEntry * len(lists))()
        for k, (_, _, _, l) in enumerate(lists):
            arr = np.ascontiguousarray(l, dtype=np.int64)
            keep.append(arr)
            e = ents[k]
            e.data, e.field_slot, e.buffer_slot, e.buffer_offset = desc(), 0, k, 0
            e.lids, e.n_lids = _ghx.i64_ptr(arr), arr.size
        h = ctypes.c_void_p()
        _ghx.call("ghx_uplan_create", ents, len(lists), direction, ctypes.byref(h))
        return h

    packs, unpacks, sbufs = [], [], []
    for r, (_, _, sends, _) in enumerate(pats):
        sbufs.append([torch.empty(len(l) * levels * 8, dtype=torch.uint8, device=dev) for *_, l in sends])
    for r, (_, _, sends, recvs) in enumerate(pats):
        fp = _ghx.ptr_array([fields["buffered"][r].data_ptr()])
        packs.append((uplan(sends, 0), fp, _ghx.ptr_array([b.data_ptr() for b in sbufs[r]]), len(sends)))
        from_peers = []
        for rid, rr, tag, lids in recvs:
            j = next(j for j, (i, q, tg, l) in enumerate(pats[rr][2]) if q == r and tg == tag)
            from_peers.append(sbufs[rr][j].data_ptr())
        unpacks.append((uplan(recvs, 1), fp, _ghx.ptr_array(from_peers), len(recvs)))

    def run_put(s):
        for h, sp, ns, dp, nd in puts:
            _ghx.check(L.ghx_put_execute(h, sp, ns, dp, nd, s), "ghx_put_execute")

    def run_buffered(s):
        for h, fp, bp, nb in packs:
            _ghx.check(L.ghx_uplan_execute(h, fp, 1, bp, nb, s), "uplan pack")
        for h, fp, bp, nb in unpacks:
            _ghx.check(L.ghx_uplan_execute(h, fp, 1, bp, nb, s), "uplan unpack")
    run = {"put": run_put, "buffered": run_buffered}
    for what in FORMS:  # every form verified before any timing
        run[what](torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for r in range(world):
            assert torch.equal(fields[what][r].view(torch.int64), want[r].view(torch.int64)), (what, r)
    for r in range(world):
        assert torch.equal(fields["put"][r].view(torch.int64), fields["buffered"][r].view(torch.int64))
    tiles = []
    for h, *_ in puts:
        b, t = ctypes.c_uint64(), ctypes.c_int32()
        _ghx.call("ghx_put_info", h, ctypes.byref(b), ctypes.byref(t))
        tiles.append(t.value)
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
    for h, *_ in puts:
        L.ghx_put_destroy(h)
    for h, *_ in packs + unpacks:
        L.ghx_uplan_destroy(h)
    med = {what: statistics.median(times[what]) for what in FORMS}
    return dict(levels=levels, row_bytes=levels * 8, cells_per_rank=cells, ranks=world,
                message_bytes=message_bytes, lids_per_exchange=message_bytes // (levels * 8),
                launches={"put": len(puts), "buffered": len(packs) + len(unpacks)},
                put_tiles=tiles, verified={what: True for what in FORMS},
                us={what: round(med[what], 3) for what in FORMS},
                put_over_buffered=round(med["put"] / med["buffered"], 3),
                us_all={what: [round(x, 3) for x in times[what]] for what in FORMS})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uput_bench.json"))
    ap.add_argument("--cells", type=int, default=None, help="owned cells per rank (default: config 5's 10M)")
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE",
                    help="ghx_tune knob set before the plans are made (development A/Bs)")
    a = ap.parse_args()
    import torch
    import ghex_amd
    from ghex_amd import _ghx
    import bench
    from tools import config5 as C5
    ghex_amd.native_library()
    assert torch.cuda.is_available(), "uput_bench needs a GPU"
    cells = C5.CELLS if a.cells is None else a.cells
    pats, _, _ = bench.config5_patterns(world=2, cells=cells)
    results = []
    for levels, urun in ((1, 1), (1, 0), (8, 1)):
        try:
            for kv in a.tune:
                key, value = kv.split("=")
                _ghx.call("ghx_tune", key.encode(), int(value))
            if not urun:
                _ghx.call("ghx_tune", b"urun", 0)
            res = measure(torch, _ghx, pats, levels, cells)
        finally:
            _ghx.call("ghx_tune", b"reset", 0)
        res["urun"] = urun
        results.append(res)
    out = dict(what="index-list put (one k_put_u launch per rank, no buffers) vs the fused ghx_uplan "
                    "pack + unpack launches of the same lists (unpacking straight from the peer's send "
                    "buffer, no transport step), two config-5 ranks' fields on one GPU, per exchange of "
                    "both ranks' halos, graph-replayed back-to-back exchanges (L2-warm), all measured "
                    "in this run; urun 0: both forms' plans rebuilt with the run path off",
               between_gpus="not measured: the put has not run between GPUs",
               exchanges_per_graph=EXCHANGES, replays=REPLAYS, rounds=ROUNDS, tune=a.tune,
               device=torch.cuda.get_device_name(0), results=results)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
