"""Worker for tests/test_gpu_cs_get_multiproc.py: one rank of a real two-process adjoint exchange of
cubed-sphere fields with the self messages fused, both ranks on cuda:0. Launched with RANK /
WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment. The geometry is the fixture's c = 6
configuration (six whole-tile domains, halos 1, 2, 0, 3); rank r holds tiles 3r .. 3r + 2, so its
exchange has rotated self messages next to peer sends and peer receives. Two communication objects
with staging="host" run on equal inputs, one with fuse_adjoint_rotated=True (the reverse pack
gathers the peer spaces only, gloo carries them, k_accum_get_x reads the self messages from the halo
cells) and one without: their fields must agree bit for bit, with and without zero_halos, for an
fp64 scalar and an f32 3-vector per domain whose sums depend on their order.

usage: python tests/mp_cs_get_worker.py <n_exchanges>"""
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
    dfs = {(si, i): DomainField(cfg, i, dt, nc, vec) for si, (dt, nc, vec, _) in enumerate(specs) for i in mine}

    def values(si, i, salt):
        df = dfs[(si, i)]
        if specs[si][0] == "float32":
            return adj.order_sensitive_values(df, salt)
        return adj.small_values(df, salt).astype(np.float64) * 2.0 ** (salt % 5 - 2)

    sides = []
    for fused in (True, False):
        bis, dev = [], {}
        for si, (dt, nc, vec, layout) in enumerate(specs):
            for i in mine:
                df = dfs[(si, i)]
                base, logical = to_device(adj.bits_of(values(si, i, 0)), layout, dt)
                bis.append(pc(CS.FieldDescriptor(dds[i], logical, df.offsets, df.extents, nc, vec)))
                dev[(si, i)] = base
        co = CS.make_communication_object(ctx, staging="host", adjoint_rotated=True, fuse_adjoint_rotated=fused)
        sides.append((co, bis, dev))
    bad = 0
    for k in range(reps):
        vals = {key: values(key[0], key[1], 1 + 7 * k) for key in dfs}
        got = []
        for co, bis, dev in sides:
            dist.barrier()
            for (si, i), v in vals.items():
                order = cs_cases.layout_order(specs[si][3])
                dev[(si, i)].copy_(torch.from_numpy(np.ascontiguousarray(v.transpose(order))))
            torch.cuda.synchronize()
            dist.barrier()
            co.adjoint_exchange(bis, zero_halos=(k % 2 == 0)).wait()
            got.append({key: from_device(dev[key], specs[key[0]][3], specs[key[0]][0]) for key in dfs})
        changed = False
        for key in dfs:
            bad += int(np.count_nonzero(got[0][key] != got[1][key]))
            changed = changed or bool((got[0][key] != adj.bits_of(vals[key])).any())
        bad += 0 if changed else 1
    forms = []
    for co, bis, _ in sides:
        f = ctypes.c_int32(-1)
        _ghx.call("ghx_cs_exchange_adjoint_self_info", co.plan(bis).h, ctypes.byref(f), None, None, None, None)
        forms.append(f.value)
    bad += 0 if forms == [2, 0] else 1
    t = torch.tensor([bad])
    dist.all_reduce(t)
    if rank == 0:
        print(f"cs get world {world}: forms {forms} bad cells {int(t.item())}")
    dist.barrier()
    del sides
    dist.destroy_process_group()
    return 0 if int(t.item()) == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
