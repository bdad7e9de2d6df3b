"""Times the adjoint halo exchange of a structured field — the reverse pack (a structured pack plan
over the RECEIVE entries) and the accumulate (ghx_sexchange_adjoint_accumulate, one k_accum_s
launch) — against the forward exchange's pack and unpack launches of the same exchange, on the
same box in the same run.

Geometry: BASELINE config 2, one periodic 512^3 fp64 domain with halo 2 (x fastest), then the same
domain with halo 1 and halo 3. Every message is a self message, so neither form has a transport
step: the forward form is ghx_exchange_pack + ghx_exchange_unpack (the two-launch path, not the
fused self launch), the adjoint ghx_sexchange_adjoint_pack + ghx_sexchange_adjoint_accumulate with
zero_halos. Both forms are first run once and checked on every cell: the forward exchange against
the periodic image of the owned cells, the adjoint (from a field whose halos hold their owners'
values) against value * (1 + number of halo images of the cell) in the owned cells and zero in the
halos. Timing: each form is captured in a graph of EXCHANGES back-to-back exchanges, replayed
REPLAYS times between two events, the forms alternating for ROUNDS rounds; the median time per
exchange of each, the spread over the rounds and the ratio are reported, with the bytes each form
must move: forward 4 x message bytes (pack and unpack each read and write them), adjoint 2 x
message bytes for the reverse pack plus, per sum sub-box, (2 + sources) x its bytes (the cell read
and written, one read per source) plus the zero stores. The kernel's register count comes from
the compiler's resource-usage remarks (--resource-usage FILE: the saved output of
hipcc -Rpass-analysis=kernel-resource-usage on ghx_accum.hip; without it the tool compiles the
file's device code itself). One GPU only.

    python tools/saccum_bench.py [--out profiles/saccum_bench.json] [--n 512]"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXCHANGES, REPLAYS, ROUNDS = 10, 20, 9
FORMS = ("adjoint", "forward")


def resource_usage(path=None):
    """SGPRs, VGPRs, scratch bytes per lane and occupancy of k_accum_s from the compiler's remarks."""
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
    at = text.index("k_accum_s")

    def num(key):
        return int(re.search(key + r"[^:]*: (\d+)", text[at:]).group(1))
    return dict(sgprs=num("SGPRs"), vgprs=num("VGPRs"), scratch_bytes_per_lane=num("ScratchSize"),
                waves_per_simd=num("Occupancy"))


def accumulate_bytes(_ghx, desc, send, recv):
    """What the accumulate must move, from a plan of the same entries: per sum sub-box (2 + sources)
    x its bytes, plus the zero stores; with the sub-boxes by source count."""
    def entry(spaces):
        bx = (_ghx.Box * len(spaces))()
        for i, sp in enumerate(spaces):
            for d in range(3):
                bx[i].first[d], bx[i].last[d] = sp[0][d], sp[1][d]
        e = _ghx.PackEntry()
        e.field, e.field_slot, e.buffer_slot, e.buffer_offset, e.boxes, e.n_boxes = desc, 0, 0, 0, bx, len(spaces)
        return e, bx
    (c, keep_c), (z, keep_z) = entry(send), entry(recv)
    h = ctypes.c_void_p()
    _ghx.call("ghx_saccum_create", ctypes.byref(c), _ghx.i32_array([_ghx.DT_F64]), 1, ctypes.byref(z), 1, ctypes.byref(h))
    nb, nz, nt = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
    _ghx.call("ghx_saccum_info", h, None, ctypes.byref(nb), ctypes.byref(nz), None, None, ctypes.byref(nt))
    moved, zeroed, by_sources = 0, 0, {}
    for k in range(nb.value + nz.value):
        b = _ghx.SAccumBoxInfo()
        _ghx.call("ghx_saccum_box", h, k, ctypes.byref(b))
        nbytes = 8
        for d in range(3):
            nbytes *= b.last[d] - b.first[d] + 1
        if b.zero:
            zeroed += nbytes
        else:
            moved += (2 + b.n_src) * nbytes
            by_sources[int(b.n_src)] = by_sources.get(int(b.n_src), 0) + 1
    _ghx.lib().ghx_saccum_destroy(h)
    return dict(sub_boxes=nb.value, zero_boxes=nz.value, tiles=nt.value, sub_boxes_by_sources=by_sources,
                sum_bytes=moved, zero_bytes=zeroed)


def measure(torch, _ghx, N, H):
    import ghex_amd
    from ghex_amd.structured import regular as R
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
    fields = {"forward": torch.where(owned, want, torch.full_like(want, -1.0)), "adjoint": want.clone()}
    expect = {"forward": want, "adjoint": torch.where(owned, want * mult.double(), torch.zeros_like(want))}
    del lin, mult
    co = R.make_communication_object(ctx, adjoint_boxes=True)
    bis = {k: [pc(R.make_field_descriptor(dd, t.permute(2, 1, 0), (H,) * 3, (E,) * 3))] for k, t in fields.items()}
    plan = co.plan(bis["forward"])
    assert co.plan(bis["adjoint"]) is plan
    send, recv = co.buffers(plan, dev)
    sptrs = _ghx.ptr_array([t.data_ptr() for t in send])
    rptrs = _ghx.ptr_array([t.data_ptr() for t in recv])
    fptr = {k: _ghx.ptr_array([t.data_ptr()]) for k, t in fields.items()}
    _ghx.call("ghx_sexchange_adjoint_create", plan.h, _ghx.i32_array([_ghx.DT_F64]), 1)
    message_bytes = sum(x["size"] for x in plan.send)

    def run_forward(s):
        _ghx.check(L.ghx_exchange_pack(plan.h, fptr["forward"], 1, sptrs, len(send), s), "pack")
        _ghx.check(L.ghx_exchange_unpack(plan.h, fptr["forward"], 1, rptrs, len(recv), s), "unpack")

    def run_adjoint(s):
        _ghx.check(L.ghx_sexchange_adjoint_pack(plan.h, fptr["adjoint"], 1, rptrs, len(recv), s), "reverse pack")
        _ghx.check(L.ghx_sexchange_adjoint_accumulate(plan.h, fptr["adjoint"], 1, sptrs, len(send), 1, s), "accumulate")
    run = {"forward": run_forward, "adjoint": run_adjoint}
    for what in FORMS:  # every form verified on every cell before any timing
        run[what](torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(fields[what].view(torch.int64), expect[what].view(torch.int64)), what
    del expect
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
    acc = accumulate_bytes(_ghx, bis["adjoint"][0].field.desc, spaces[0], spaces[1])
    med = {what: statistics.median(times[what]) for what in FORMS}
    moved = {"forward": 4 * message_bytes, "adjoint": 2 * message_bytes + acc["sum_bytes"] + acc["zero_bytes"]}
    return dict(N=N, halo=H, message_bytes=message_bytes, launches={what: 2 for what in FORMS}, accumulate=acc,
                bytes_moved=moved, bytes_adjoint_over_forward=round(moved["adjoint"] / moved["forward"], 3),
                verified={what: True for what in FORMS}, us={what: round(med[what], 3) for what in FORMS},
                us_min={what: round(min(times[what]), 3) for what in FORMS},
                us_max={what: round(max(times[what]), 3) for what in FORMS},
                adjoint_over_forward=round(med["adjoint"] / med["forward"], 3),
                us_all={what: [round(x, 3) for x in times[what]] for what in FORMS})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "saccum_bench.json"))
    ap.add_argument("--n", type=int, default=512, help="cells per dimension of the domain (default: config 2's 512)")
    ap.add_argument("--resource-usage", default=None, metavar="FILE",
                    help="saved kernel-resource-usage remarks of ghx_accum.hip (default: compile it now)")
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE",
                    help="ghx_tune knob set before the plans are made (development A/Bs)")
    a = ap.parse_args()
    import torch
    import ghex_amd
    from ghex_amd import _ghx
    ghex_amd.native_library()
    assert torch.cuda.is_available(), "saccum_bench needs a GPU"
    usage = resource_usage(a.resource_usage)
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
    out = dict(what="adjoint structured exchange (reverse pack + k_accum_s accumulate with zero_halos) vs the forward "
                    "exchange's pack + unpack launches of the same exchange, one periodic fp64 domain (every message a "
                    "self message: no transport step in either form), per exchange, graph-replayed back-to-back "
                    "exchanges (L2-warm), all measured in this run",
               between_gpus="not measured: the adjoint has not run between GPUs",
               k_accum_s=usage, exchanges_per_graph=EXCHANGES, replays=REPLAYS, rounds=ROUNDS, tune=a.tune,
               device=torch.cuda.get_device_name(0), results=results)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
