"""Times the fused index-list self exchange (ghx_uexchange_self: ONE k_self_u launch) against the
buffered form of the same exchange — ghx_exchange_pack followed by ghx_exchange_unpack, one fused
launch each — on the same box in the same run.

Geometry: BASELINE config 5's generator (tools/config5_gen.cpp: 10M owned cells per domain, 5 %
halo cells drawn from the other domain, permuted storage) for TWO domains, both held by ONE rank,
so every message is a self message and the recv buffers are the send buffers; the exchange is the
product's (make_pattern<unstructured>, ghx_exchange_create, the communication object's buffers).
fp64, levels first, at levels 1 (8-byte rows: request-bound, the run path) and levels 8 (64-byte
rows). An exchange moves both domains' halos and leaves the packed messages in the send buffers:
  fused     one launch: send lists on the sending fields -> send buffers and -> receive lists on
            the receiving fields; no buffer byte is read
  buffered  one pack launch into the send buffers, then one unpack launch that reads them back
Both forms are first run once from identical fields and sentinel-filled buffers and checked bit
for bit: the fields against the owners' values, and fields and buffers against each other.
Timing: each form is captured in a graph of EXCHANGES back-to-back exchanges, replayed REPLAYS
times between two events, the forms alternating for ROUNDS rounds; the median time per exchange
of each, the ratio of the medians and the spread of the per-round ratio are reported, at levels 1
also with the run path off (knob urun = 0, the exchange rebuilt). One GPU.

    python tools/uself_bench.py [--out profiles/uself_bench.json]"""
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
FORMS = ("fused", "buffered")
SENTINEL = 0xC3


def measure(torch, ghex_amd, _ghx, domains, levels, cells):
    """One configuration under the knobs as they are set now: the exchange (one per form, over
    that form's own fields and buffers), the bit-exact check, the alternating timing."""
    from ghex_amd import unstructured as U
    L = _ghx.lib()
    dev = torch.device("cuda", 0)
    ctx = ghex_amd.make_context()
    dds = [U.DomainDescriptor(k, gids, outer) for k, (gids, outer) in enumerate(domains)]
    pc = U.make_pattern(ctx, U.HaloGenerator(), dds)
    want = []
    for gids, outer in domains:
        host = gids.astype(np.float64)[:, None] * 100.0 + np.arange(levels, dtype=np.float64)[None, :]
        want.append(torch.from_numpy(host).to(dev))
    state = {}
    for what in FORMS:
        fields = []
        for w, (gids, outer) in zip(want, domains):
            t = w.clone()
            t[torch.from_numpy(np.asarray(outer)).to(dev)] = -1.0
            fields.append(t)
        bis = [pc(U.make_field_descriptor(dd, t)) for dd, t in zip(dds, fields)]
        co = U.make_communication_object(ctx, fuse_lists=(what == "fused"))
        plan = co.plan(bis)
        send, recv = co.buffers(plan, dev)
        assert all(r.data_ptr() == s.data_ptr() for r, s in zip(recv, send)), "recv buffers alias send"
        for t in send:
            t.fill_(SENTINEL)
        state[what] = dict(fields=fields, bis=bis, co=co, plan=plan, send=send,
                           fp=_ghx.ptr_array([t.data_ptr() for t in fields]),
                           sp=_ghx.ptr_array([t.data_ptr() for t in send]))
    fus, nseg, ntiles = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _ghx.call("ghx_uexchange_self_info", state["fused"]["plan"].h, ctypes.byref(fus), ctypes.byref(nseg),
              ctypes.byref(ntiles))
    assert fus.value == 1, L.ghx_last_error()
    nf = len(domains)

    def run_fused(s):
        st = state["fused"]
        _ghx.check(L.ghx_uexchange_self(st["plan"].h, st["fp"], nf, st["sp"], len(st["send"]), s),
                   "ghx_uexchange_self")

    def run_buffered(s):
        st = state["buffered"]
        _ghx.check(L.ghx_exchange_pack(st["plan"].h, st["fp"], nf, st["sp"], len(st["send"]), s),
                   "ghx_exchange_pack")
        _ghx.check(L.ghx_exchange_unpack(st["plan"].h, st["fp"], nf, st["sp"], len(st["send"]), s),
                   "ghx_exchange_unpack")
    run = {"fused": run_fused, "buffered": run_buffered}
    for what in FORMS:  # every form verified before any timing
        run[what](torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for k in range(nf):
            assert torch.equal(state[what]["fields"][k].view(torch.int64), want[k].view(torch.int64)), (what, k)
    for a, b in zip(state["fused"]["fields"], state["buffered"]["fields"]):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    message_bytes = 0
    for a, b, x in zip(state["fused"]["send"], state["buffered"]["send"], state["fused"]["plan"].send):
        assert torch.equal(a, b), "send buffers differ between the forms"
        assert bool((a[:x["size"]] != SENTINEL).any())
        message_bytes += x["size"]
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
    med = {what: statistics.median(times[what]) for what in FORMS}
    ratios = [f / b for f, b in zip(times["fused"], times["buffered"])]
    spread = {what: (max(times[what]) - min(times[what])) for what in FORMS}
    return dict(levels=levels, row_bytes=levels * 8, cells_per_domain=cells, domains=nf,
                message_bytes=message_bytes, lids_per_exchange=message_bytes // (levels * 8),
                launches={"fused": 1, "buffered": 2}, fused_segments=nseg.value, fused_tiles=ntiles.value,
                verified={what: True for what in FORMS}, buffers_equal=True,
                us={what: round(med[what], 3) for what in FORMS},
                fused_over_buffered=round(med["fused"] / med["buffered"], 3),
                ratio_per_round=dict(min=round(min(ratios), 3), median=round(statistics.median(ratios), 3),
                                     max=round(max(ratios), 3)),
                us_spread={what: round(spread[what], 3) for what in FORMS},
                fused_faster_beyond_spread=bool(med["buffered"] - med["fused"] > max(spread.values())),
                us_all={what: [round(x, 3) for x in times[what]] for what in FORMS})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uself_bench.json"))
    ap.add_argument("--cells", type=int, default=None, help="owned cells per domain (default: config 5's 10M)")
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE",
                    help="ghx_tune knob set before the plans are made (development A/Bs)")
    a = ap.parse_args()
    import torch
    import ghex_amd
    from ghex_amd import _ghx
    from tools import config5 as C5
    ghex_amd.native_library()
    assert torch.cuda.is_available(), "uself_bench needs a GPU"
    cells = C5.CELLS if a.cells is None else a.cells
    domains = [C5.generate(r, 2, cells) for r in range(2)]
    results = []
    for levels, urun in ((1, 1), (1, 0), (8, 1)):
        try:
            for kv in a.tune:
                key, value = kv.split("=")
                _ghx.call("ghx_tune", key.encode(), int(value))
            if not urun:
                _ghx.call("ghx_tune", b"urun", 0)
            res = measure(torch, ghex_amd, _ghx, domains, levels, cells)
        finally:
            _ghx.call("ghx_tune", b"reset", 0)
        res["urun"] = urun
        results.append(res)
    out = dict(what="fused index-list self exchange (ghx_uexchange_self, one k_self_u launch) vs the "
                    "ghx_exchange_pack + ghx_exchange_unpack launches of the same exchange (the unpack "
                    "reads the send buffers back), two config-5 domains held by one rank on one GPU, per "
                    "exchange of both domains' halos, graph-replayed back-to-back exchanges (L2-warm), "
                    "all measured in this run; urun 0: the exchange rebuilt with the run path off",
               exchanges_per_graph=EXCHANGES, replays=REPLAYS, rounds=ROUNDS, tune=a.tune,
               device=torch.cuda.get_device_name(0), results=results)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
