"""Worker for tests/test_gpu_uget_multiproc.py: one rank of a real two-process adjoint exchange of
the unstructured known-answer case (tests/golden/unstructured_case.json), both ranks on cuda:0,
once with a fused object (fuse_adjoint_lists=True) and once with an unfused one on copies of the
same fields. Launched with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment. Rank r
holds domains 2r and 2r + 1, so its exchange has two self messages next to four peer sends and
four peer receives: the fused adjoint is the mixed form (form 2) - the reverse pack gathers the
peer messages' halos alone, gloo carries them back (staging="host"), and the one accumulate launch
reads the self messages from the halo cells and the peer messages from the send buffers. In
exchange k an owned cell holds (domain*10000 + gid*100 + level) * (k + 1) and halo cell lid of
domain d holds (7 + 3*d + 11*lid + 101*level) * (k + 1). After each exchange the fused fields must
equal the unfused ones byte for byte, and both the answer worked out from the golden maps.

usage: python tests/mp_uget_worker.py <levels> <n_exchanges>"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    levels, reps = (int(v) for v in sys.argv[1:3])
    import numpy as np
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    torch.cuda.set_device(0)
    import ghex_amd
    from ghex_amd import _ghx
    from ghex_amd import unstructured as U
    ghex_amd.native_library()
    with open(os.path.join(ROOT, "tests", "golden", "unstructured_case.json")) as fh:
        case = json.load(fh)
    doms = {r: case["domains"][str(r)] for r in range(4)}
    mine = (2 * rank, 2 * rank + 1)
    ctx = ghex_amd.make_context()
    dds = [U.DomainDescriptor(r, doms[r]["gids"], doms[r]["halo_lids"]) for r in mine]
    pc = U.make_pattern(ctx, U.HaloGenerator(), dds)
    lv = np.arange(levels, dtype=np.float64)[None, :]

    def halo_value(d, lid):
        return 7.0 + 3 * d + 11 * lid + 101 * lv[0]

    wants, inits = [], []
    for r in mine:
        gids = np.asarray(doms[r]["gids"], dtype=np.float64)[:, None]
        init = r * 10000 + gids * 100 + lv
        for lid in doms[r]["halo_lids"]:
            init[lid] = halo_value(r, lid)
        want = init.copy()
        for dst, sl in case["send_maps"][str(r)].items():
            for lid, hl in zip(sl, case["recv_maps"][dst][str(r)]):
                want[lid] += halo_value(int(dst), hl)
        want[doms[r]["halo_lids"]] = 0.0
        wants.append(want)
        inits.append(init)
    sides = []
    for options in (dict(fuse_adjoint_lists=True), dict()):
        fields = [torch.empty((len(doms[r]["gids"]), levels), dtype=torch.float64, device="cuda") for r in mine]
        bis = [pc(U.make_field_descriptor(dd, t)) for dd, t in zip(dds, fields)]
        sides.append((U.make_communication_object(ctx, staging="host", **options), fields, bis))
    bad = 0
    for k in range(reps):
        for co, fields, bis in sides:
            dist.barrier()
            for t, init in zip(fields, inits):
                t.copy_(torch.from_numpy(init * (k + 1)))
            torch.cuda.synchronize()
            dist.barrier()
            co.adjoint_exchange(bis).wait()
        for a, b, want in zip(sides[0][1], sides[1][1], wants):
            bad += 0 if torch.equal(a.view(torch.uint8), b.view(torch.uint8)) else 1
            bad += int(np.count_nonzero(a.cpu().numpy() != want * (k + 1)))
    fused, unfused = sides[0][0].plan(sides[0][2]), sides[1][0].plan(sides[1][2])
    form = ctypes.c_int32(-1)
    _ghx.call("ghx_uexchange_adjoint_self_info", fused.h, ctypes.byref(form), None, None, None)
    ok = (form.value == 2 and fused._adjoint_prefix == "ghx_uexchange_adjoint_self_"
          and unfused._adjoint_prefix == "ghx_uexchange_adjoint_")
    t = torch.tensor([bad + (0 if ok else 1000)])
    dist.all_reduce(t)
    if rank == 0:
        print(f"uget world {world} levels {levels}: bad cells {int(t.item())}")
    dist.barrier()
    del sides
    dist.destroy_process_group()
    return 0 if int(t.item()) == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
