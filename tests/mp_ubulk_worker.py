"""Worker for tests/test_gpu_ubulk_multiproc.py: one rank of a real multi-process bulk exchange
of an unstructured field, every rank on cuda:0. Launched with RANK / WORLD_SIZE / MASTER_ADDR /
MASTER_PORT in the environment. Every rank owns `cells` cells (gids rank*10^6 + i) and holds
cells/4 halo cells drawn from every other rank, all in a random storage order, `levels` levels
(levels first) — the geometry of tests/mp_exchange_worker.py's udirect mode. value(gid, level) =
(gid*100 + level) * (k + 1) in exchange k: the field is rewritten before every exchange (halos
to -1), so a halo left over from another exchange is seen. The puts (ghx_uput_create, k_put_u)
go through IPC mappings into the peers' fields, ordered by the device epochs.

Mode "mixed": two emulated hosts (even / odd ranks, GHX_HOSTNAME): puts inside a host, the
host-staged buffered exchange of the pattern's remote part between the hosts.

usage: python tests/mp_ubulk_worker.py <cells> <levels> <n_exchanges> <bulk|mixed>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    cells, levels, reps = (int(v) for v in sys.argv[1:4])
    mode = sys.argv[4]
    import numpy as np
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    import ghex_amd
    from ghex_amd import unstructured as U
    ghex_amd.native_library()
    rng = np.random.default_rng(977 + rank)
    nh = cells // 4
    others = np.array([r for r in range(world) if r != rank])
    owner = others[rng.integers(0, len(others), size=4 * nh)]
    halo = np.unique(owner.astype(np.int64) * 1_000_000 + rng.integers(0, cells, size=4 * nh))
    halo = rng.permutation(halo)[:nh]
    gids = np.concatenate([rank * 1_000_000 + np.arange(cells, dtype=np.int64), halo])
    perm = rng.permutation(len(gids))
    gids = gids[perm]
    outer = np.nonzero(perm >= cells)[0]
    ctx = ghex_amd.make_context()
    dd = U.DomainDescriptor(rank, gids, outer)
    pc = U.make_pattern(ctx, U.HaloGenerator(), [dd])
    base = gids.astype(np.float64)[:, None] * 100.0 + np.arange(levels)[None, :]
    field = torch.empty((len(gids), levels), dtype=torch.float64, device="cuda")
    fd = U.make_field_descriptor(dd, field)
    if mode == "mixed":
        os.environ["GHX_HOSTNAME"] = f"emulated-host-{rank % 2}"
        bco = ghex_amd.make_bulk_communication_object(ctx, timeout=60,
                                                      remote_options={"staging": "host"})
    else:
        bco = ghex_amd.make_bulk_communication_object(ctx, timeout=60)
    bco.add_field(pc(fd))
    bco.init()
    assert (bco._co is not None) == (mode == "mixed")
    assert len(bco._puts) >= 1
    want_bytes = sum(len(lids) for rid, rr, tag, lids in pc.send_halos(0)
                     if bco._co is None or rr % 2 == rank % 2) * levels * 8
    assert bco.bytes_per_exchange() == want_bytes, (bco.bytes_per_exchange(), want_bytes)
    bad = 0
    for k in range(reps):
        want = base * (k + 1)
        init = want.copy()
        init[outer] = -1.0
        # nobody's field is rewritten while a peer of the previous exchange may still read or
        # write it: the epochs order puts against the TARGET's earlier kernels on its stream,
        # and the host copy below is ordered by the wait() of the previous exchange on every rank
        dist.barrier()
        field.copy_(torch.from_numpy(init))
        torch.cuda.synchronize()
        dist.barrier()
        bco.exchange().wait()
        bad += int(np.count_nonzero(field.cpu().numpy() != want))
    t = torch.tensor([bad])
    dist.all_reduce(t)
    if rank == 0:
        print(f"ubulk {mode} world {world} cells {cells} levels {levels}: bad cells {int(t.item())}")
    dist.barrier()
    del bco
    dist.destroy_process_group()
    return 0 if int(t.item()) == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
