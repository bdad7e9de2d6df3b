"""Times the adjoint halo exchange of index lists whose every message is a self message in its two
forms — unfused (reverse pack into the receive buffers, then k_accum_u from the send buffers: two
launches) and fused (ghx_uexchange_adjoint_self_accumulate: one k_accum_get_u launch that reads the
halo cells where they lie and zeroes them) — against the forward exchange's pack and unpack launches
of the same exchange, on the same box in the same run.

Geometry: that of profiles/uself_bench.json — BASELINE config 5's generator (tools/config5_gen.cpp:
10M owned cells per domain, 5 % halo cells drawn from the other domain, permuted storage) for TWO
domains, both held by ONE rank, so every message is a self message and the recv buffers are the send
buffers; the exchange is the product's (make_pattern<unstructured>, ghx_exchange_create, the
communication object's buffers). fp64, levels first, at levels 1 (8-byte rows) and levels 8 (64-byte
rows). No form has a transport step. All three forms are first run once and checked bit for bit:
the forward exchange against the owners' values, each adjoint (from fields whose halos hold their
owners' values) against value * (1 + number of halo copies of the cell) in the owner cells and zero
in the halos, and the two adjoints against each other. Timing: each form is captured in a graph of
EXCHANGES back-to-back exchanges, replayed REPLAYS times between two events, the forms alternating
for ROUNDS rounds; the median time per exchange of each and the spread over the rounds are reported,
the ratios fused / unfused and fused / forward per round (median, min, max), and the payload bytes
each form must move (tables not counted): forward 4 x message bytes (field -> buffer -> field);
unfused 2 x message bytes for the reverse pack, then per sum destination a cell load and store and
one buffer load per record, then a zero store per halo cell; fused the cell load and store, one halo
load per record and one zero store per record. One GPU only.

    python tools/uadjoint_self_bench.py [--out profiles/uadjoint_self_bench.json]"""
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
FORMS = ("forward", "unfused", "fused")


def measure(torch, ghex_amd, _ghx, domains, levels, cells):
    from ghex_amd import unstructured as U
    L = _ghx.lib()
    dev = torch.device("cuda", 0)
    ctx = ghex_amd.make_context()
    dds = [U.DomainDescriptor(k, gids, outer) for k, (gids, outer) in enumerate(domains)]
    pc = U.make_pattern(ctx, U.HaloGenerator(), dds)
    copies = {}
    for gids, outer in domains:
        g, c = np.unique(np.asarray(gids)[np.asarray(outer)], return_counts=True)
        for a, b in zip(g, c):
            copies[int(a)] = copies.get(int(a), 0) + int(b)
    want, adjoint = [], []
    for gids, outer in domains:
        host = gids.astype(np.float64)[:, None] * 100.0 + np.arange(levels, dtype=np.float64)[None, :]
        want.append(torch.from_numpy(host).to(dev))
        a = host * np.array([1 + copies.get(int(g), 0) for g in gids], dtype=np.float64)[:, None]
        a[np.asarray(outer)] = 0.0
        adjoint.append(torch.from_numpy(a).to(dev))
    expect = {"forward": want, "unfused": adjoint, "fused": adjoint}
    nf = len(domains)
    co = U.make_communication_object(ctx)
    state = {}
    for what in FORMS:
        fields = [w.clone() for w in want]
        if what == "forward":
            for t, (gids, outer) in zip(fields, domains):
                t[torch.from_numpy(np.asarray(outer)).to(dev)] = -1.0
        state[what] = dict(fields=fields, bis=[pc(U.make_field_descriptor(dd, t)) for dd, t in zip(dds, fields)],
                           fp=_ghx.ptr_array([t.data_ptr() for t in fields]))
    plan = co.plan(state["forward"]["bis"])
    assert co.plan(state["unfused"]["bis"]) is plan and co.plan(state["fused"]["bis"]) is plan
    send, recv = co.buffers(plan, dev)
    assert all(r.data_ptr() == s.data_ptr() for r, s in zip(recv, send)), "recv buffers alias send"
    sp = _ghx.ptr_array([t.data_ptr() for t in send])
    codes = _ghx.i32_array([_ghx.DT_F64] * nf)
    _ghx.call("ghx_uexchange_adjoint_create", plan.h, codes, nf)
    _ghx.call("ghx_uexchange_adjoint_self_create", plan.h, codes, nf)
    form, nd, nc, nfs = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    _ghx.call("ghx_uexchange_adjoint_self_info", plan.h, ctypes.byref(form), ctypes.byref(nd), ctypes.byref(nc),
              ctypes.byref(nfs))
    assert form.value == 1, L.ghx_last_error()
    message_bytes = sum(x["size"] for x in plan.send)
    n_halo = sum(len(outer) for _, outer in domains)

    def run_forward(s):
        fp = state["forward"]["fp"]
        _ghx.check(L.ghx_exchange_pack(plan.h, fp, nf, sp, len(send), s), "pack")
        _ghx.check(L.ghx_exchange_unpack(plan.h, fp, nf, sp, len(send), s), "unpack")

    def run_unfused(s):
        fp = state["unfused"]["fp"]
        _ghx.check(L.ghx_uexchange_adjoint_pack(plan.h, fp, nf, sp, len(send), s), "reverse pack")
        _ghx.check(L.ghx_uexchange_adjoint_accumulate(plan.h, fp, nf, sp, len(send), 1, s), "accumulate")

    def run_fused(s):
        fp = state["fused"]["fp"]
        _ghx.check(L.ghx_uexchange_adjoint_self_pack(plan.h, fp, nf, sp, len(send), s), "reverse pack")
        _ghx.check(L.ghx_uexchange_adjoint_self_accumulate(plan.h, fp, nf, sp, len(send), 1, s), "get-accumulate")
    run = {"forward": run_forward, "unfused": run_unfused, "fused": run_fused}
    for what in FORMS:  # every form verified on every cell before any timing
        run[what](torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for k in range(nf):
            assert torch.equal(state[what]["fields"][k].view(torch.int64), expect[what][k].view(torch.int64)), (what, k)
    for a, b in zip(state["fused"]["fields"], state["unfused"]["fields"]):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
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
    row = levels * 8
    cell_bytes = 2 * nd.value * row                      # every sum destination loaded and stored once
    moved = {"forward": 4 * message_bytes,
             "unfused": 2 * message_bytes + cell_bytes + nc.value * row + n_halo * row,
             "fused": cell_bytes + 2 * nc.value * row}
    med = {what: statistics.median(times[what]) for what in FORMS}

    def ratio(a, b):
        r = [x / y for x, y in zip(times[a], times[b])]
        return dict(median=round(statistics.median(r), 3), min=round(min(r), 3), max=round(max(r), 3))
    return dict(levels=levels, row_bytes=row, cells_per_domain=cells, domains=nf, message_bytes=message_bytes,
                n_dest=nd.value, n_contrib=nc.value, n_field_sources=nfs.value, halo_cells=n_halo,
                launches={"forward": 2, "unfused": 2, "fused": 1}, bytes_moved=moved,
                bytes_fused_over_unfused=round(moved["fused"] / moved["unfused"], 3),
                bytes_fused_over_forward=round(moved["fused"] / moved["forward"], 3),
                verified={what: True for what in FORMS}, us={what: round(med[what], 3) for what in FORMS},
                us_min={what: round(min(times[what]), 3) for what in FORMS},
                us_max={what: round(max(times[what]), 3) for what in FORMS},
                fused_over_unfused=ratio("fused", "unfused"), fused_over_forward=ratio("fused", "forward"),
                unfused_over_forward=ratio("unfused", "forward"),
                us_all={what: [round(x, 3) for x in times[what]] for what in FORMS})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uadjoint_self_bench.json"))
    ap.add_argument("--cells", type=int, default=None, help="owned cells per domain (default: config 5's 10M)")
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE",
                    help="ghx_tune knob set before the plans are made (development A/Bs)")
    a = ap.parse_args()
    import torch
    import ghex_amd
    from ghex_amd import _ghx
    from tools import config5 as C5
    ghex_amd.native_library()
    assert torch.cuda.is_available(), "uadjoint_self_bench needs a GPU"
    cells = C5.CELLS if a.cells is None else a.cells
    domains = [C5.generate(r, 2, cells) for r in range(2)]
    results = []
    for levels in (1, 8):
        try:
            for kv in a.tune:
                key, value = kv.split("=")
                _ghx.call("ghx_tune", key.encode(), int(value))
            results.append(measure(torch, ghex_amd, _ghx, domains, levels, cells))
        finally:
            _ghx.call("ghx_tune", b"reset", 0)
        torch.cuda.empty_cache()
    out = dict(what="adjoint index-list exchange of two config-5 domains held by one rank on one GPU (every message a "
                    "self message, no transport step), fp64, zero_halos: unfused (reverse pack + k_accum_u, two "
                    "launches) and fused (one k_accum_get_u launch reading the halo cells in place) vs the forward "
                    "exchange's pack + unpack launches of the same exchange, per exchange of both domains' halos, "
                    "graph-replayed back-to-back exchanges (L2-warm), all measured alternately in this run",
               not_measured="form 2 (self and peer messages), other geometries, anything between GPUs",
               exchanges_per_graph=EXCHANGES, replays=REPLAYS, rounds=ROUNDS, tune=a.tune,
               device=torch.cuda.get_device_name(0), results=results)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
