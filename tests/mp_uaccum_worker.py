"""Worker for tests/test_gpu_uaccum_multiproc.py: one rank of a real two-process adjoint exchange
of the unstructured known-answer case (tests/golden/unstructured_case.json), both ranks on cuda:0.
Launched with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment. Rank r holds
domains 2r and 2r + 1, so its exchange has two self messages next to four peer sends and four
peer receives; the communication object is made with staging="host", so adjoint_exchange() packs
the halo cells into the receive buffers, gloo carries the peer receive buffers back into the
peers' send buffers, and the accumulate reads the send buffers. In exchange k an owned cell holds
(domain*10000 + gid*100 + level) * (k + 1) and halo cell lid of domain d holds
(7 + 3*d + 11*lid + 101*level) * (k + 1): the fields are rewritten before every exchange. Every
cell of both fields is checked after each one: owner = its value + the values of its halo copies
(worked out from the golden send / receive maps), halos zero.

usage: python tests/mp_uaccum_worker.py <levels> <n_exchanges>"""
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

    fields, wants, inits, bis = [], [], [], []
    for r, dd in zip(mine, dds):
        gids = np.asarray(doms[r]["gids"], dtype=np.float64)[:, None]
        init = r * 10000 + gids * 100 + lv
        for lid in doms[r]["halo_lids"]:
            init[lid] = halo_value(r, lid)
        want = init.copy()
        for dst, sl in case["send_maps"][str(r)].items():
            for lid, hl in zip(sl, case["recv_maps"][dst][str(r)]):
                want[lid] += halo_value(int(dst), hl)
        want[doms[r]["halo_lids"]] = 0.0
        t = torch.empty((len(doms[r]["gids"]), levels), dtype=torch.float64, device="cuda")
        fields.append(t)
        wants.append(want)
        inits.append(init)
        bis.append(pc(U.make_field_descriptor(dd, t)))
    co = U.make_communication_object(ctx, staging="host")
    plan = co.plan(bis)
    assert sorted(x["rank"] == rank for x in plan.send) == [False] * 4 + [True] * 2
    bad = 0
    for k in range(reps):
        dist.barrier()
        for t, init in zip(fields, inits):
            t.copy_(torch.from_numpy(init * (k + 1)))
        torch.cuda.synchronize()
        dist.barrier()
        co.adjoint_exchange(bis).wait()
        for t, want in zip(fields, wants):
            bad += int(np.count_nonzero(t.cpu().numpy() != want * (k + 1)))
    # the forward exchange of the same object still takes its own host buffers
    co.exchange(bis).wait()
    for r, t, want in zip(mine, fields, wants):
        got = t.cpu().numpy()
        own = [lid for lid in range(len(doms[r]["gids"])) if lid not in doms[r]["halo_lids"]]
        bad += int(np.count_nonzero(got[own] != want[own] * reps))
        bad += int(np.count_nonzero(got[doms[r]["halo_lids"]] == 0.0))
    t = torch.tensor([bad])
    dist.all_reduce(t)
    if rank == 0:
        print(f"uaccum world {world} levels {levels}: bad cells {int(t.item())}")
    dist.barrier()
    del co
    dist.destroy_process_group()
    return 0 if int(t.item()) == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
