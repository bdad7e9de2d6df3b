"""Times the mixed form of an index-list exchange with self AND peer messages
(ghx_uexchange_pack_self: ONE k_pack_self_u launch that packs every send buffer and writes the
self messages' halos, then ghx_uexchange_unpack_peers over the peer recv buffers only) against the
two-launch form of the same plan (ghx_exchange_pack, then ghx_exchange_unpack over every recv
buffer, the self messages read back from their send buffers) on the same box in the same run.

Geometry: BASELINE config 5's generator (tools/config5_gen.cpp: 10M owned cells per domain, 5 %
halo cells drawn from the other domains, permuted storage) for FOUR domains over TWO emulated
ranks of two domains each; the plan timed is rank 0's (make_pattern<unstructured> on both ranks,
ghx_exchange_create, the communication object's buffers). Rank 1 packs once; its send buffers are
copied into rank 0's peer recv buffers and stay there, so rank 0's unpack finds real messages.
fp64, levels first, at levels 1 (8-byte rows: request-bound, the run path) and levels 8 (64-byte
rows). Both forms are first run once from identical fields and sentinel-filled buffers and checked
bit for bit: rank 0's fields against the owners' values, and fields and send buffers against each
other. Timing: each form is captured in a graph of EXCHANGES back-to-back exchanges, replayed
REPLAYS times between two events, the forms alternating for ROUNDS rounds; the median time per
exchange of each, the ratio of the medians and the spread of the per-round ratio are reported,
with the self messages' share of the message bytes. One GPU.

    python tools/umixed_bench.py [--out profiles/umixed_bench.json]"""
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
FORMS = ("mixed", "two_launch")
SENTINEL = 0xC3


def patterns(domains):
    """Both emulated ranks' (context, domain ids, domain descriptors, pattern): rank r holds
    domains 2r and 2r + 1; the ranks run as threads of this process (LoopbackWorld)."""
    from ghex_amd import unstructured as U
    from ghex_amd.context import LoopbackWorld

    def rank_fn(ctx):
        ids = (2 * ctx.rank(), 2 * ctx.rank() + 1)
        dds = [U.DomainDescriptor(k, domains[k][0], domains[k][1]) for k in ids]
        return ctx, ids, dds, U.make_pattern(ctx, U.HaloGenerator(), dds)

    return LoopbackWorld(2).run(rank_fn)


def measure(torch, _ghx, domains, ranks, levels, cells):
    """One configuration under the knobs as they are set now: rank 0's exchange (one per form,
    over that form's own fields and buffers), the bit-exact check, the alternating timing."""
    from ghex_amd import unstructured as U
    L = _ghx.lib()
    dev = torch.device("cuda", 0)

    def owned(k):
        gids = domains[k][0]
        return torch.from_numpy(gids.astype(np.float64)[:, None] * 100.0 +
                                np.arange(levels, dtype=np.float64)[None, :]).to(dev)

    def make(rank, halos_unset, **options):
        ctx, ids, dds, pc = ranks[rank]
        fields = []
        for k in ids:
            t = owned(k)
            if halos_unset:
                t[torch.from_numpy(np.asarray(domains[k][1])).to(dev)] = -1.0
            fields.append(t)
        bis = [pc(U.make_field_descriptor(dd, t)) for dd, t in zip(dds, fields)]
        co = U.make_communication_object(ctx, **options)
        plan = co.plan(bis)
        send, recv = co.buffers(plan, dev)
        for t in send + recv:
            t.fill_(SENTINEL)
        return dict(fields=fields, bis=bis, co=co, plan=plan, send=send, recv=recv,
                    fp=_ghx.ptr_array([t.data_ptr() for t in fields]),
                    sp=_ghx.ptr_array([t.data_ptr() for t in send]),
                    rp=_ghx.ptr_array([t.data_ptr() for t in recv]))

    want = [owned(k) for k in ranks[0][1]]
    # rank 1 packs once (its owners' values); its messages to rank 0 stay in rank 0's recv buffers
    peer = make(1, False)
    peer["co"].pack_only(peer["bis"])
    state = {what: make(0, True, fuse_lists_mixed=(what == "mixed")) for what in FORMS}
    for st in state.values():
        for i, x in enumerate(st["plan"].recv):
            if x["rank"] == 0:
                continue
            j = next(j for j, s in enumerate(peer["plan"].send) if s["pair"] == x["pair"] and s["rank"] == 0)
            assert peer["plan"].send[j]["size"] == x["size"]
            st["recv"][i][:x["size"]].copy_(peer["send"][j][:x["size"]])
    torch.cuda.synchronize()
    del peer
    mixed, nst, npt = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _ghx.call("ghx_uexchange_mixed_info", state["mixed"]["plan"].h, ctypes.byref(mixed), ctypes.byref(nst),
              ctypes.byref(npt))
    assert mixed.value == 1 and state["mixed"]["co"].lists_mixed(state["mixed"]["plan"]), L.ghx_last_error()
    nf = 2

    def run_form(what, pack, unpack):
        st = state[what]

        def run(s):
            _ghx.check(pack(st["plan"].h, st["fp"], nf, st["sp"], len(st["send"]), s), "pack")
            _ghx.check(unpack(st["plan"].h, st["fp"], nf, st["rp"], len(st["recv"]), s), "unpack")
        return run
    run = {"mixed": run_form("mixed", L.ghx_uexchange_pack_self, L.ghx_uexchange_unpack_peers),
           "two_launch": run_form("two_launch", L.ghx_exchange_pack, L.ghx_exchange_unpack)}
    for what in FORMS:  # every form verified before any timing
        run[what](torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for k in range(nf):
            assert torch.equal(state[what]["fields"][k].view(torch.int64), want[k].view(torch.int64)), (what, k)
    for a, b in zip(state["mixed"]["fields"], state["two_launch"]["fields"]):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    plan = state["mixed"]["plan"]
    self_bytes = peer_send_bytes = 0
    for a, b, x in zip(state["mixed"]["send"], state["two_launch"]["send"], plan.send):
        assert torch.equal(a, b), "send buffers differ between the forms"
        assert bool((a[:x["size"]] != SENTINEL).any())
        if x["rank"] == 0:
            self_bytes += x["size"]
        else:
            peer_send_bytes += x["size"]
    peer_recv_bytes = sum(x["size"] for x in plan.recv if x["rank"] != 0)
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
    ratios = [m / t for m, t in zip(times["mixed"], times["two_launch"])]
    spread = {what: (max(times[what]) - min(times[what])) for what in FORMS}
    return dict(levels=levels, row_bytes=levels * 8, cells_per_domain=cells, domains=4, ranks=2,
                self_message_bytes=self_bytes, peer_send_bytes=peer_send_bytes,
                peer_recv_bytes=peer_recv_bytes,
                self_share_of_packed_bytes=round(self_bytes / (self_bytes + peer_send_bytes), 3),
                launches={"mixed": 2, "two_launch": 2}, self_tiles=nst.value, peer_tiles=npt.value,
                verified={what: True for what in FORMS}, buffers_equal=True,
                us={what: round(med[what], 3) for what in FORMS},
                mixed_over_two_launch=round(med["mixed"] / med["two_launch"], 3),
                ratio_per_round=dict(min=round(min(ratios), 3), median=round(statistics.median(ratios), 3),
                                     max=round(max(ratios), 3)),
                us_spread={what: round(spread[what], 3) for what in FORMS},
                mixed_faster_beyond_spread=bool(med["two_launch"] - med["mixed"] > max(spread.values())),
                us_all={what: [round(x, 3) for x in times[what]] for what in FORMS})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "umixed_bench.json"))
    ap.add_argument("--cells", type=int, default=None, help="owned cells per domain (default: config 5's 10M)")
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE",
                    help="ghx_tune knob set before the plans are made (development A/Bs)")
    a = ap.parse_args()
    import torch
    import ghex_amd
    from ghex_amd import _ghx
    from tools import config5 as C5
    ghex_amd.native_library()
    assert torch.cuda.is_available(), "umixed_bench needs a GPU"
    cells = C5.CELLS if a.cells is None else a.cells
    domains = [C5.generate(r, 4, cells) for r in range(4)]
    ranks = patterns(domains)
    results = []
    for levels in (1, 8):
        try:
            for kv in a.tune:
                key, value = kv.split("=")
                _ghx.call("ghx_tune", key.encode(), int(value))
            results.append(measure(torch, _ghx, domains, ranks, levels, cells))
        finally:
            _ghx.call("ghx_tune", b"reset", 0)
    out = dict(what="index-list exchange with self and peer messages: ghx_uexchange_pack_self (one "
                    "k_pack_self_u launch) + ghx_uexchange_unpack_peers vs ghx_exchange_pack + "
                    "ghx_exchange_unpack of the same plan (the unpack reads the self messages back from "
                    "their send buffers), rank 0 of two emulated ranks holding two config-5 domains each "
                    "on one GPU, per exchange, graph-replayed back-to-back exchanges (L2-warm), all "
                    "measured in this run",
               exchanges_per_graph=EXCHANGES, replays=REPLAYS, rounds=ROUNDS, tune=a.tune,
               device=torch.cuda.get_device_name(0), results=results)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
