"""Worker for tests/test_gpu_cs_put_multiproc.py: one rank of six, one cube tile each, every rank
on cuda:0 (the peers' fields are mapped through IPC; on a multi-GPU node they would be peer GPUs
over xGMI). The c = 6 fixture geometry, halos (1, 2, 0, 3), two fields per rank: an f32 2-vector
x stride-1 and an f64 scalar y stride-1. One cubed-sphere bulk object per process, epochs="device";
before each exchange the interiors are rewritten (a bit pattern XORed into every owned cell) and
the halos filled with the sentinel, after it every cell is compared with the expectation for
that pattern. Launched with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment;
rank 0 prints the world's count of bad cells.

usage: python tests/mp_cs_put_worker.py [n_exchanges]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

X_FAST, Y_FAST = (3, 2, 1, 0), (2, 3, 1, 0)
FIELDS = (("float32", 2, True, X_FAST), ("float64", 1, False, Y_FAST))


def expected_with_interior_flip(df, flip):
    """df.expected() when every interior cell of every domain has `flip` XORed into its bits
    (applied before a vector component's negation, as the exchange sees it)."""
    from tests import cs_cases
    u = cs_cases.uint_of(df.dtype)
    a = df.initial()
    own = a != df.sentinel
    a[own] ^= u(flip)
    for b in df.dom["boxes"]:
        xs, ys, _ = df.box_values(b)
        saved, df.vector = df.vector, False
        _, _, plain = df.box_values(b)
        df.vector = saved
        bits = plain ^ u(flip)
        if df.vector:
            for comp in (0, 1):
                if comp < df.nc and b["sign"][comp] < 0:
                    bits[..., comp] = cs_cases.negate_bits(bits[..., comp], df.dtype)
        a[xs[0] + df.h:xs[-1] + df.h + 1, ys[0] + df.h:ys[-1] + df.h + 1] = bits
    return a


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    import numpy as np
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 6
    torch.cuda.set_device(0)
    import ghex_amd
    from ghex_amd.structured import cubed_sphere as CS
    from tests import cs_cases
    from tests.cs_cases import DomainField, from_device, to_device
    ghex_amd.native_library()
    cfg = cs_cases.config(6)
    dom = cfg["domains"][rank]
    cube = CS.Cube(cfg["edge_size"], cfg["levels"])
    ctx = ghex_amd.make_context()
    dd = CS.DomainDescriptor(cube, dom["tile"], *dom["x"], *dom["y"])
    pc = CS.make_pattern(ctx, CS.HaloGenerator(cfg["halos"]), [dd])
    bco = CS.make_bulk_communication_object(ctx, epochs="device", timeout=60)
    fields = []
    for dtype, nc, vector, layout in FIELDS:
        df = DomainField(cfg, rank, dtype, nc, vector)
        base, logical = to_device(df.initial(), layout, dtype)
        bco.add_field(pc(CS.FieldDescriptor(dd, logical, df.offsets, df.extents, nc, vector)))
        fields.append((df, base, layout))
    bad = 0
    for k in range(reps):
        flip = k  # low mantissa bits: no cell turns into the sentinel; 0 = the fixture's values
        for df, base, layout in fields:
            a = df.initial()
            own = a != df.sentinel
            a[own] ^= cs_cases.uint_of(df.dtype)(flip)
            order = cs_cases.layout_order(layout)
            base.copy_(torch.from_numpy(np.ascontiguousarray(a.transpose(order))
                                        .view(np.dtype(df.dtype))))
        bco.exchange().wait()
        for df, base, layout in fields:
            got = from_device(base, layout, df.dtype)
            bad += int(np.count_nonzero(got != expected_with_interior_flip(df, flip)))
    assert bco._ep is not None and bco._co is None  # device epochs, node-local puts only
    t = torch.tensor([bad])
    dist.all_reduce(t)
    if rank == 0:
        print(f"cs put world {world} c {cfg['edge_size']} x{reps}: bad cells {int(t.item())}")
    dist.barrier()
    del bco
    dist.destroy_process_group()
    sys.exit(0 if int(t.item()) == 0 else 1)


if __name__ == "__main__":
    main()
