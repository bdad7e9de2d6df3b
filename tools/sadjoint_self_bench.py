"""Times the adjoint halo exchange of a structured field whose every message is a self message in
its two forms — unfused (reverse pack into the receive buffers, then k_accum_s from the send
buffers: two launches) and fused (ghx_sexchange_adjoint_self_accumulate: one k_accum_get_s launch
that reads the halo cells where they lie and zeroes them) — against the forward exchange's pack and
unpack launches of the same exchange, on the same box in the same run.

Geometry: BASELINE config 2, one periodic 512^3 fp64 domain with halo 2 (x fastest), then the same
domain with halo 1 and halo 3. No form has a transport step. All three forms are first run once
and checked on every cell: the forward exchange against the periodic image of the owned cells, each
adjoint (from a field whose halos hold their owners' values) against value * (1 + number of halo
images of the cell) in the owned cells and zero in the halos. Timing: each form is captured in a
graph of EXCHANGES back-to-back exchanges, replayed REPLAYS times between two events, the forms
alternating for ROUNDS rounds; the median time per exchange of each and the spread over the rounds
are reported, the ratios fused / unfused and fused / forward per round (median, min, max), and the
bytes each form must move: forward 4 x message bytes; unfused 2 x message bytes for the reverse
pack plus, per sum sub-box, (2 + sources) x its bytes plus the zero stores; fused, per sum sub-box,
(2 + sources) x its bytes plus one zero store per halo byte. One GPU only.

    python tools/sadjoint_self_bench.py [--out profiles/sadjoint_self_bench.json] [--n 512]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

EXCHANGES, REPLAYS, ROUNDS = 10, 20, 9
FORMS = ("forward", "unfused", "fused")


def measure(torch, _ghx, N, H):
    import ghex_amd
    from ghex_amd.structured import regular as R
    from saccum_bench import accumulate_bytes
    L = _ghx.lib()
    dev = torch.device("cuda", 0)
    E = N + 2 * H
    ctx = ghex_amd.make_context()
    dd = R.DomainDescriptor(0, (0, 0, 0), (N - 1,) * 3)
    pc = R.make_pattern(ctx, R.HaloGenerator((0, 0, 0), (N - 1,) * 3, (H,) * 6, (True,) * 3), [dd])
    # every cell's periodic owner value and its number of halo images, on the device
    ax = (torch.arange(E, device=dev) - H) % N
    lin = (ax[:, None, None] * N + ax[None, :, None]) * N + ax[None, None, :]          # [z, y, x]
    inner = torch.zeros(E, dtype=torch.bool, device=dev)
    inner[H:H + N] = True
    owned = inner[:, None, None] & inner[None, :, None] & inner[None, None, :]
    per = 1 + (torch.arange(N, device=dev) < H).long() + (torch.arange(N, device=dev) >= N - H).long()
    images = torch.ones(E, dtype=torch.long, device=dev)
    images[H:H + N] = per
    mult = images[:, None, None] * images[None, :, None] * images[None, None, :]
    want = lin.double()
    adjoint = torch.where(owned, want * mult.double(), torch.zeros_like(want))
    fields = {"forward": torch.where(owned, want, torch.full_like(want, -1.0)), "unfused": want.clone(),
              "fused": want.clone()}
    expect = {"forward": want, "unfused": adjoint, "fused": adjoint}
    del lin, mult
    co = R.make_communication_object(ctx, adjoint_boxes=True)
    bis = {k: [pc(R.make_field_descriptor(dd, t.permute(2, 1, 0), (H,) * 3, (E,) * 3))] for k, t in fields.items()}
    plan = co.plan(bis["forward"])
    assert co.plan(bis["unfused"]) is plan and co.plan(bis["fused"]) is plan
    send, recv = co.buffers(plan, dev)
    sptrs = _ghx.ptr_array([t.data_ptr() for t in send])
    rptrs = _ghx.ptr_array([t.data_ptr() for t in recv])
    fptr = {k: _ghx.ptr_array([t.data_ptr()]) for k, t in fields.items()}
    _ghx.call("ghx_sexchange_adjoint_create", plan.h, _ghx.i32_array([_ghx.DT_F64]), 1)
    _ghx.call("ghx_sexchange_adjoint_self_create", plan.h, _ghx.i32_array([_ghx.DT_F64]), 1)
    form = ctypes.c_int32()
    _ghx.call("ghx_sexchange_adjoint_self_info", plan.h, ctypes.byref(form), None, None, None)
    assert form.value == 1
    message_bytes = sum(x["size"] for x in plan.send)

    def run_forward(s):
        _ghx.check(L.ghx_exchange_pack(plan.h, fptr["forward"], 1, sptrs, len(send), s), "pack")
        _ghx.check(L.ghx_exchange_unpack(plan.h, fptr["forward"], 1, rptrs, len(recv), s), "unpack")

    def run_unfused(s):
        _ghx.check(L.ghx_sexchange_adjoint_pack(plan.h, fptr["unfused"], 1, rptrs, len(recv), s), "reverse pack")
        _ghx.check(L.ghx_sexchange_adjoint_accumulate(plan.h, fptr["unfused"], 1, sptrs, len(send), 1, s), "accumulate")

    def run_fused(s):
        _ghx.check(L.ghx_sexchange_adjoint_self_pack(plan.h, fptr["fused"], 1, rptrs, len(recv), s), "reverse pack")
        _ghx.check(L.ghx_sexchange_adjoint_self_accumulate(plan.h, fptr["fused"], 1, sptrs, len(send), 1, s),
                   "get-accumulate")
    run = {"forward": run_forward, "unfused": run_unfused, "fused": run_fused}
    for what in FORMS:  # every form verified on every cell before any timing
        run[what](torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(fields[what].view(torch.int64), expect[what].view(torch.int64)), what
    del expect, adjoint
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
    spaces = [[(sp[0], sp[1]) for _, _, _, sps in halos for sp in sps] for halos in (pc.send_halos(0), pc.recv_halos(0))]
    acc = accumulate_bytes(_ghx, bis["unfused"][0].field.desc, spaces[0], spaces[1])
    med = {what: statistics.median(times[what]) for what in FORMS}
    moved = {"forward": 4 * message_bytes, "unfused": 2 * message_bytes + acc["sum_bytes"] + acc["zero_bytes"],
             "fused": acc["sum_bytes"] + message_bytes}

    def ratio(a, b):
        r = [x / y for x, y in zip(times[a], times[b])]
        return dict(median=round(statistics.median(r), 3), min=round(min(r), 3), max=round(max(r), 3))
    return dict(N=N, halo=H, message_bytes=message_bytes, launches={"forward": 2, "unfused": 2, "fused": 1},
                accumulate=acc, bytes_moved=moved,
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sadjoint_self_bench.json"))
    ap.add_argument("--n", type=int, default=512, help="cells per dimension of the domain (default: config 2's 512)")
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE",
                    help="ghx_tune knob set before the plans are made (development A/Bs)")
    a = ap.parse_args()
    import torch
    import ghex_amd
    from ghex_amd import _ghx
    ghex_amd.native_library()
    assert torch.cuda.is_available(), "sadjoint_self_bench needs a GPU"
    results = []
    for halo in (2, 1, 3):
        try:
            for kv in a.tune:
                key, value = kv.split("=")
                _ghx.call("ghx_tune", key.encode(), int(value))
            results.append(measure(torch, _ghx, a.n, halo))
        finally:
            _ghx.call("ghx_tune", b"reset", 0)
        torch.cuda.empty_cache()
    out = dict(what="adjoint structured exchange of one periodic fp64 domain (every message a self message, no "
                    "transport step), zero_halos: unfused (reverse pack + k_accum_s, two launches) and fused (one "
                    "k_accum_get_s launch reading the halo cells in place) vs the forward exchange's pack + unpack "
                    "launches of the same exchange, per exchange, graph-replayed back-to-back exchanges (L2-warm), all "
                    "measured alternately in this run",
               exchanges_per_graph=EXCHANGES, replays=REPLAYS, rounds=ROUNDS, tune=a.tune,
               device=torch.cuda.get_device_name(0), results=results)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
