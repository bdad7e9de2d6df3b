"""Worker for tests/test_gpu_umixed_multiproc.py: one rank of a real two-process exchange of the
unstructured known-answer case (tests/golden/unstructured_case.json), both ranks on cuda:0.
Launched with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment. Rank r holds
domains 2r and 2r + 1, so its exchange has two self messages next to four peer sends and four
peer receives; the communication object is made with fuse_lists_mixed=True and staging="host"
(gloo carries the peer buffers), so exchange() packs with ghx_uexchange_pack_self and unpacks
with ghx_uexchange_unpack_peers. value(domain, gid, level) = (domain*10000 + gid*100 + level) *
(k + 1) in exchange k: the fields are rewritten before every exchange (halos to -1), so a halo
left over from another exchange is seen. Every cell of both fields is checked after each one.

usage: python tests/mp_umixed_worker.py <levels> <n_exchanges>"""
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
    owner = {g: r for r, d in doms.items() for lid, g in enumerate(d["gids"]) if lid not in d["halo_lids"]}
    mine = (2 * rank, 2 * rank + 1)
    ctx = ghex_amd.make_context()
    dds = [U.DomainDescriptor(r, doms[r]["gids"], doms[r]["halo_lids"]) for r in mine]
    pc = U.make_pattern(ctx, U.HaloGenerator(), dds)
    lv = np.arange(levels, dtype=np.float64)[None, :]
    fields, wants, inits, bis = [], [], [], []
    for r, dd in zip(mine, dds):
        gids = np.asarray(doms[r]["gids"], dtype=np.float64)[:, None]
        own = np.asarray([owner[g] for g in doms[r]["gids"]], dtype=np.float64)[:, None]
        want = own * 10000 + gids * 100 + lv
        init = want.copy()
        init[doms[r]["halo_lids"]] = -1.0
        t = torch.empty((len(doms[r]["gids"]), levels), dtype=torch.float64, device="cuda")
        fields.append(t)
        wants.append(want)
        inits.append(init)
        bis.append(pc(U.make_field_descriptor(dd, t)))
    co = U.make_communication_object(ctx, fuse_lists_mixed=True, staging="host")
    plan = co.plan(bis)
    assert co.lists_mixed(plan) and not co.mixed(plan) and not co.lists_self(plan)
    assert sorted(x["rank"] == rank for x in plan.send) == [False] * 4 + [True] * 2
    bad = 0
    for k in range(reps):
        dist.barrier()
        for t, init in zip(fields, inits):
            t.copy_(torch.from_numpy(np.where(init < 0, init, init * (k + 1))))
        torch.cuda.synchronize()
        dist.barrier()
        co.exchange(bis).wait()
        for t, want in zip(fields, wants):
            bad += int(np.count_nonzero(t.cpu().numpy() != want * (k + 1)))
    t = torch.tensor([bad])
    dist.all_reduce(t)
    if rank == 0:
        print(f"umixed world {world} levels {levels}: bad cells {int(t.item())}")
    dist.barrier()
    del co
    dist.destroy_process_group()
    return 0 if int(t.item()) == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
