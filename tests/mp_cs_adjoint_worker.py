"""Worker for tests/test_gpu_cs_adjoint_multiproc.py: one rank of a real two-process adjoint
exchange of cubed-sphere fields, both ranks on cuda:0. Launched with RANK / WORLD_SIZE /
MASTER_ADDR / MASTER_PORT in the environment. The geometry is the fixture's c = 6 configuration
(six whole-tile domains, halos 1, 2, 0, 3); rank r holds tiles 3r .. 3r + 2, so its exchange has
self messages next to peer sends and peer receives. The communication object is made with
adjoint_rotated=True and staging="host": adjoint_exchange() packs the halo cells, rotated and
negated, into the receive buffers (k_pack_x and the ordinary reverse pack), gloo carries the peer
receive buffers back into the peers' send buffers, and the accumulate (k_accum_s) reads the send
buffers. An fp64 scalar and an f32 3-vector per domain hold small integers, rewritten before every
exchange; every cell of every field is compared bit for bit with the NumPy adjoint of the whole
configuration (tests/cs_adjoint_cases.py), then the forward exchange of the same object is checked
against the recorded images.

usage: python tests/mp_cs_adjoint_worker.py <n_exchanges> <zero_halos 0|1>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    reps, zero = int(sys.argv[1]), bool(int(sys.argv[2]))
    import numpy as np
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    torch.cuda.set_device(0)
    import ghex_amd
    from ghex_amd.structured import cubed_sphere as CS
    from tests import cs_adjoint_cases as adj
    from tests import cs_cases
    from tests.cs_cases import DomainField, from_device, to_device
    ghex_amd.native_library()
    cfg = cs_cases.config(6)
    specs = [("float64", 1, False, (3, 2, 1, 0)), ("float32", 3, True, (3, 2, 1, 0))]
    cube = CS.Cube(cfg["edge_size"], cfg["levels"])
    mine = [i for i, d in enumerate(cfg["domains"]) if d["tile"] // 3 == rank]
    ctx = ghex_amd.make_context()
    dds = {i: CS.DomainDescriptor(cube, cfg["domains"][i]["tile"], *cfg["domains"][i]["x"],
                                  *cfg["domains"][i]["y"]) for i in mine}
    pc = CS.make_pattern(ctx, CS.HaloGenerator(cfg["halos"]), [dds[i] for i in mine])
    n_dom = len(cfg["domains"])
    dfs = [[DomainField(cfg, i, dt, nc, vec) for i in range(n_dom)] for dt, nc, vec, _ in specs]
    bis, dev = [], {}
    for si, (dt, nc, vec, layout) in enumerate(specs):
        for i in mine:
            df = dfs[si][i]
            base, logical = to_device(adj.bits_of(adj.small_values(df, si)), layout, dt)
            bis.append(pc(CS.FieldDescriptor(dds[i], logical, df.offsets, df.extents, nc, vec)))
            dev[(si, i)] = base
    co = CS.make_communication_object(ctx, staging="host", adjoint_rotated=True)
    plan = co.plan(bis)
    assert any(x["rank"] == rank for x in plan.send) and any(x["rank"] != rank for x in plan.send)
    bad = 0
    for k in range(reps):
        vals = [[adj.small_values(df, si + 7 * k) for df in dfs[si]] for si in range(len(specs))]
        dist.barrier()
        for si, (dt, nc, vec, layout) in enumerate(specs):
            order = cs_cases.layout_order(layout)
            for i in mine:
                dev[(si, i)].copy_(torch.from_numpy(np.ascontiguousarray(vals[si][i].transpose(order))))
        torch.cuda.synchronize()
        dist.barrier()
        co.adjoint_exchange(bis, zero_halos=zero).wait()
        for si, (dt, nc, vec, layout) in enumerate(specs):
            want = adj.numpy_adjoint(cfg, dfs[si], vals[si], zero)
            for i in mine:
                got = from_device(dev[(si, i)], layout, dt)
                bad += int(np.count_nonzero(got != adj.bits_of(want[i])))
    # the forward exchange of the same object still takes its own host buffers
    for si, (dt, nc, vec, layout) in enumerate(specs):
        order = cs_cases.layout_order(layout)
        for i in mine:
            first = dfs[si][i].initial()
            dev[(si, i)].copy_(torch.from_numpy(np.ascontiguousarray(first.transpose(order)).view(np.dtype(dt))))
    torch.cuda.synchronize()
    dist.barrier()
    co.exchange(bis).wait()
    for si, (dt, nc, vec, layout) in enumerate(specs):
        for i in mine:
            bad += int(np.count_nonzero(from_device(dev[(si, i)], layout, dt) != dfs[si][i].expected()))
    t = torch.tensor([bad])
    dist.all_reduce(t)
    if rank == 0:
        print(f"cs adjoint world {world} zero_halos {int(zero)}: bad cells {int(t.item())}")
    dist.barrier()
    del co
    dist.destroy_process_group()
    return 0 if int(t.item()) == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
