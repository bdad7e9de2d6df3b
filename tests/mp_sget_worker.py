"""Worker for tests/test_gpu_sget_multiproc.py: one rank of a real two-process adjoint exchange with
the self messages fused, both ranks on cuda:0. Launched with RANK / WORLD_SIZE / MASTER_ADDR /
MASTER_PORT in the environment. The global grid is (2,1,1) periodic domains of 4^3 with halo 2;
rank r holds domain r, so 8 of its 26 messages wrap onto itself in y and z and 18 go to the peer.
Two communication objects with staging="host" run on equal inputs, one with fuse_adjoint=True (the
reverse pack gathers the peer messages only, gloo carries them, k_accum_get_s reads the self
messages from the halo cells) and one without: their fields must agree bit for bit, with and
without zero_halos, for an f64 and an i32 field in one exchange.

usage: python tests/mp_sget_worker.py <n_exchanges>"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    reps = int(sys.argv[1])
    import numpy as np
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    torch.cuda.set_device(0)
    import ghex_amd
    from ghex_amd import _ghx
    from ghex_amd.structured import regular as R
    ghex_amd.native_library()
    n, H = 4, 2
    E = n + 2 * H
    ctx = ghex_amd.make_context()
    dd = R.DomainDescriptor(rank, (rank * n, 0, 0), ((rank + 1) * n - 1, n - 1, n - 1))
    pc = R.make_pattern(ctx, R.HaloGenerator((0, 0, 0), (2 * n - 1, n - 1, n - 1), (H,) * 6, (True,) * 3), [dd])
    sides = []
    for fused in (True, False):
        ts = [torch.empty((E, E, E), dtype=dt, device="cuda") for dt in (torch.float64, torch.int32)]
        bis = [pc(R.make_field_descriptor(dd, t.permute(2, 1, 0), (H,) * 3, (E,) * 3)) for t in ts]
        co = R.make_communication_object(ctx, staging="host", adjoint_boxes=True, fuse_adjoint=fused)
        sides.append((co, bis, ts))
    rng = np.random.default_rng(100 + rank)
    bad = 0
    for k in range(reps):
        ys = [rng.integers(-50, 51, size=(E, E, E)).astype(np.float64) * 2.0 ** int(rng.integers(-8, 9)),
              rng.integers(-2 ** 31, 2 ** 31, size=(E, E, E)).astype(np.int32)]
        got = []
        for co, bis, ts in sides:
            dist.barrier()
            for t, y in zip(ts, ys):
                t.copy_(torch.from_numpy(y))
            torch.cuda.synchronize()
            dist.barrier()
            co.adjoint_exchange(bis, zero_halos=(k % 2 == 0)).wait()
            got.append([t.cpu().numpy() for t in ts])
        for a, b, y in zip(got[0], got[1], ys):
            bad += int(np.count_nonzero(a.view(np.uint8) != b.view(np.uint8)))
            bad += 0 if (a != y).any() else 1
    forms = []
    for co, bis, _ in sides:
        f = ctypes.c_int32(-1)
        _ghx.call("ghx_sexchange_adjoint_self_info", co.plan(bis).h, ctypes.byref(f), None, None, None)
        forms.append(f.value)
    bad += 0 if forms == [2, 0] else 1
    t = torch.tensor([bad])
    dist.all_reduce(t)
    if rank == 0:
        print(f"sget world {world}: forms {forms} bad cells {int(t.item())}")
    dist.barrier()
    del sides
    dist.destroy_process_group()
    return 0 if int(t.item()) == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
