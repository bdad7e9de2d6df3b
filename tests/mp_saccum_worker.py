"""Worker for tests/test_gpu_saccum_multiproc.py: one rank of a real two-process adjoint exchange
of structured fields, both ranks on cuda:0. Launched with RANK / WORLD_SIZE / MASTER_ADDR /
MASTER_PORT in the environment. The global grid is 2x2x1 periodic domains of 4^3 with halo H; rank
r holds domains 2r and 2r + 1, so its exchange has self messages next to peer sends and peer
receives. The communication object is made with adjoint_boxes=True and staging="host", so
adjoint_exchange() packs the halo cells into the receive buffers, gloo carries the peer receive
buffers back into the peers' send buffers, and the accumulate (k_accum_s) reads the send buffers.
In exchange k every cell (owned or halo) of domain d at local (x, y, z) holds
((d + 1) * 1000 + x + E*(y + E*z)) * (k + 1), E = 4 + 2H, counted from the halo's corner: the
fields are rewritten before every exchange. Every cell of both fields is checked after each one:
an owned cell = its value + the values of all its halo images in the four domains, halo cells
zero.

usage: python tests/mp_saccum_worker.py <H> <n_exchanges>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    H, reps = (int(v) for v in sys.argv[1:3])
    import numpy as np
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    torch.cuda.set_device(0)
    import ghex_amd
    from ghex_amd.structured import regular as R
    ghex_amd.native_library()
    n = 4
    E = n + 2 * H
    G = (2 * n, 2 * n, n)
    first = {d: ((d % 2) * n, (d // 2) * n, 0) for d in range(4)}
    init = {d: ((d + 1) * 1000 + np.arange(E ** 3, dtype=np.float64)).reshape(E, E, E) for d in range(4)}  # [z, y, x]
    total = {}
    halo = np.ones((E, E, E), dtype=bool)
    halo[H:H + n, H:H + n, H:H + n] = False
    for d in range(4):
        for z, y, x in zip(*np.nonzero(halo)):
            g = tuple((f + c - H) % m for f, c, m in zip(first[d], (x, y, z), G))
            total[g] = total.get(g, 0.0) + init[d][z, y, x]
    mine = (2 * rank, 2 * rank + 1)
    wants = []
    for d in mine:
        w = init[d].copy()
        for z in range(n):
            for y in range(n):
                for x in range(n):
                    w[z + H, y + H, x + H] += total.get((first[d][0] + x, first[d][1] + y, first[d][2] + z), 0.0)
        w[halo] = 0.0
        wants.append(w)
    ctx = ghex_amd.make_context()
    dds = [R.DomainDescriptor(d, first[d], tuple(f + n - 1 for f in first[d])) for d in mine]
    pc = R.make_pattern(ctx, R.HaloGenerator((0, 0, 0), tuple(m - 1 for m in G), (H,) * 6, (True,) * 3), dds)
    fields = [torch.empty((E, E, E), dtype=torch.float64, device="cuda") for _ in mine]
    bis = [pc(R.make_field_descriptor(dd, t.permute(2, 1, 0), (H,) * 3, (E,) * 3)) for dd, t in zip(dds, fields)]
    co = R.make_communication_object(ctx, staging="host", adjoint_boxes=True)
    plan = co.plan(bis)
    assert any(x["rank"] == rank for x in plan.send) and any(x["rank"] != rank for x in plan.send)
    bad = 0
    for k in range(reps):
        dist.barrier()
        for t, d in zip(fields, mine):
            t.copy_(torch.from_numpy(init[d] * (k + 1)))
        torch.cuda.synchronize()
        dist.barrier()
        co.adjoint_exchange(bis).wait()
        for t, want in zip(fields, wants):
            bad += int(np.count_nonzero(t.cpu().numpy() != want * (k + 1)))
    # the forward exchange of the same object still takes its own host buffers: every halo cell
    # becomes its owner's sum
    co.exchange(bis).wait()
    for t, want in zip(fields, wants):
        got = t.cpu().numpy()
        bad += int(np.count_nonzero(got[~halo] != want[~halo] * reps))
        bad += int(np.count_nonzero(got[halo] == 0.0))
    t = torch.tensor([bad])
    dist.all_reduce(t)
    if rank == 0:
        print(f"saccum world {world} H {H}: bad cells {int(t.item())}")
    dist.barrier()
    del co
    dist.destroy_process_group()
    return 0 if int(t.item()) == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
