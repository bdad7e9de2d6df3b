"""Device parity of the structured copy kernels in every vector width, offset form and tile walk:
the cases of tests/structured_cases.py packed and unpacked through ghx_plan_create /
ghx_plan_execute (k_copy<*, seg_s>: copy_tile<W, AM> and unpack_tile_pipelined<16>), put through
ghx_put_create / ghx_put_execute (k_put: copy_direct<W, AM>) and exchanged through the fused self
exchange of the Python API (k_self: self_forward<W, AM>, the pack / barrier / unpack path, the
pack-only peer tile), each asserting from the planner's records and the real pointers which form
the launch takes before it runs.

Reference: the numpy int64 enumeration of the field byte offset of every message element
(addressing_cases.element_offsets), which tests/test_structured_cases.py ties to the pinned
oracle; for the exchanges, the oracle's exchange on a compact twin. Everything is bit-exact.
Every field lives in a zero-filled (sentinel) device arena with message bytes in 1..255 and guard
bands sized on the host so that the addresses of the short forms a segment must NOT take stay
inside the arena as well (test_arena_closure): a kernel that decodes with the wrong form lands in
sentinel memory and fails the comparison instead of faulting."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import addressing_cases as A
from tests import helpers as H
from tests import structured_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ghex_amd
    ghex_amd.native_library()


def _random_bytes(n, seed):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(1, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)


def _nonzero(t):
    import torch
    return int(torch.count_nonzero(t))


@functools.lru_cache(maxsize=4)
def _device_indices(case):
    """(per-entry arena byte indices, their sorted union) on the device, bounds checked on the
    host; computed once per case and left unchanged."""
    import torch
    lay, idx = S.layout(case), S.arena_indices(case)
    for i in idx:
        assert i.min() >= 0 and i.max() < lay.arena_bytes
    dev = [torch.from_numpy(i).cuda() for i in idx]
    cells = torch.unique(torch.cat(dev))
    assert cells.numel() == case.message_bytes  # no cell twice: the scatter is defined
    return dev, cells


def _execute(h, fptrs, bptrs):
    import torch
    from ghex_amd import _ghx
    _ghx.call("ghx_plan_execute", h, _ghx.ptr_array(fptrs), len(fptrs), _ghx.ptr_array(bptrs),
              len(bptrs), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


class _Arena:
    """A case's field arena and buffer allocation on the device, with the pointers its plans are
    executed with. The knob-free part of the case names the geometry: `base` (the table's case)
    gives the layout, `case` (base + launch knobs) the plans."""

    def __init__(self, case, base=None):
        import torch
        base = case if base is None else base
        self.case, self.lay = case, S.layout(base)
        lay = self.lay
        self.arena = torch.zeros(lay.arena_bytes, dtype=torch.uint8, device="cuda")
        self.bufs = torch.zeros(lay.buffers_bytes, dtype=torch.uint8, device="cuda")
        assert self.arena.data_ptr() % 256 == 0 and self.bufs.data_ptr() % 256 == 0
        self.idx, self.cells = _device_indices(base)
        assert all(S.GUARD <= a and b + S.GUARD <= lay.buffers_bytes for a, b in lay.msg)
        self.fptrs = [self.arena.data_ptr() + r.ptr for r in lay.fields]
        self.bptrs = [self.bufs.data_ptr() + p for p in lay.buf_ptr]
        # worked out before any plan under test is open: these create plans of their own
        self.forms = [S.expected_forms(case, d) for d in (0, 1)]

    def check_plan(self, plan, direction):
        """The planner's records say what the table says, and with these pointers every segment
        takes the form the host test lists for it."""
        segs = plan.segments()
        S.assert_planned(self.case, segs, direction)
        got = [S.launch_form(s, self.fptrs[s.field_slot], self.bptrs[s.buffer_slot], direction)
               for s in segs]
        assert got == self.forms[direction]
        # the case's knobs are the ones in force at the launch (grid_cap is read there)
        assert plan.knobs_in_force()
        assert S.knobs_in_force() == dict(self.case.knobs)
        return got

    def pads_are_clean(self):
        for a, b in self.lay.msg:
            assert not bool(self.bufs[a - S.PAD:a].any()) and not bool(self.bufs[b:b + S.PAD].any())

    def pack(self):
        import torch
        case, lay = self.case, self.lay
        self.arena.zero_()
        self.bufs.zero_()
        self.arena[self.cells] = _random_bytes(self.cells.numel(), 5)
        want = [self.arena[i] for i in self.idx]
        with S.SPlan(case, 0) as p:
            self.check_plan(p, 0)
            _execute(p.h, self.fptrs, self.bptrs)
        for (a, b), w in zip(lay.msg, want):
            assert torch.equal(self.bufs[a:b], w)
        self.pads_are_clean()
        # nothing before buffer_offset, in the guards or between the messages was written
        assert _nonzero(self.bufs) == case.message_bytes
        # the pack wrote nothing into the arena
        assert _nonzero(self.arena) == case.message_bytes
        for i, w in zip(self.idx, want):
            assert torch.equal(self.arena[i], w)

    def unpack(self):
        import torch
        case, lay = self.case, self.lay
        self.arena.zero_()
        self.bufs.zero_()
        for k, (a, b) in enumerate(lay.msg):
            self.bufs[a:b] = _random_bytes(b - a, 6 + k)
        sent = self.bufs.clone()
        with S.SPlan(case, 1) as p:
            self.check_plan(p, 1)
            _execute(p.h, self.fptrs, self.bptrs)
        for (a, b), i in zip(lay.msg, self.idx):
            assert torch.equal(self.arena[i], sent[a:b])
        # the message's cells and nothing else
        assert _nonzero(self.arena) == case.message_bytes
        assert torch.equal(self.bufs, sent)
        self.pads_are_clean()


def _pack_and_unpack(name, **knobs):
    base = S.CASES[name]
    a = _Arena(S.with_knobs(base, **knobs), base)
    a.pack()
    a.unpack()


# ---------------------------------------------------------------------------------------------
# k_copy: the whole table, by tile records and by the tile table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile_records", [1, 0])
@pytest.mark.parametrize("name", list(S.CASES))
def test_pack_unpack_every_form(name, tile_records):
    _pack_and_unpack(name, tile_records=tile_records)


def _grid_params():
    """grid_cap 1 (one workgroup walks every tile) and 2 on every multi-tile case (each has at
    least 3 tiles in both directions), 7 on those of dozens of tiles (a stride that does not
    divide the tile count)."""
    out = []
    for name in S.GRID_CASES:
        for cap in (1, 2) + ((7,) if name in ("short1_r64", "several", "several_u32k") else ()):
            out.append((name, cap))
    return out


@pytest.mark.parametrize("tile_records", [1, 0])
@pytest.mark.parametrize("name,cap", _grid_params())
def test_grid_cap(name, cap, tile_records):
    """k_copy's grid-stride do ... while over copy_tile and over the pipelined unpack; in
    `several` one workgroup walks tiles of different segments and widths."""
    _pack_and_unpack(name, grid_cap=cap, tile_records=tile_records)


# ---------------------------------------------------------------------------------------------
# k_put
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _put_indices(put):
    import torch
    size, src, dst = S.put_layout(put)
    si = A.word_indices(A.case_offsets(put.src), put.src.elem, 1, src.ptr)
    ti = A.word_indices(A.case_offsets(put.dst), put.dst.elem, 1, dst.ptr)
    assert src.span[0] <= si.min() and si.max() < src.span[1] <= dst.span[0]  # disjoint regions
    assert dst.span[0] <= ti.min() and ti.max() < dst.span[1] <= size
    assert np.unique(ti).size == ti.size == si.size == put.src.nbytes
    return torch.from_numpy(si).cuda(), torch.from_numpy(ti).cuda()


def _put(put, **knobs):
    import torch
    from ghex_amd import _ghx
    size, src, dst = S.put_layout(put)
    si, ti = _put_indices(put)
    n = put.src.nbytes
    arena = torch.zeros(size, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 256 == 0
    data = _random_bytes(n, 7)
    arena[si] = data
    sp, dp = arena.data_ptr() + src.ptr, arena.data_ptr() + dst.ptr
    s, q = S.put_segments(put)
    assert S.put_form(s, q, sp, dp) == put.form
    (es, _), (ed, _) = S.put_entries(put)
    h = ctypes.c_void_p()
    with S.tuned(dict(put.knobs, **knobs)) as t:
        _ghx.call("ghx_put_create", ctypes.byref(es), 1, ctypes.byref(ed), 1, ctypes.byref(h))
        try:
            nt = ctypes.c_int32()
            _ghx.call("ghx_put_info", h, None, ctypes.byref(nt))
            assert nt.value == len(S.tile_walk(s, put.form[1]))
            assert t.in_force() and S.knobs_in_force().get("grid_cap", 0) == knobs.get("grid_cap", 0)
            _ghx.call("ghx_put_execute", h, _ghx.ptr_array([sp]), 1, _ghx.ptr_array([dp]), 1,
                      torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        finally:
            _ghx.lib().ghx_put_destroy(h)
    assert torch.equal(arena[ti], data)
    assert torch.equal(arena[si], data)
    assert _nonzero(arena) == 2 * n  # the source, the target's cells, nothing else


@pytest.mark.parametrize("tile_records", [1, 0])
@pytest.mark.parametrize("name", list(S.PUTS))
def test_put_every_width(name, tile_records):
    """copy_direct<1 .. 16> general and copy_direct<8, 1> / <16, 1>, on long rows (11 tiles, the
    last one partial) and on short rows, source and target behind different strides and
    shifts."""
    _put(S.PUTS[name], tile_records=tile_records)


@pytest.mark.parametrize("tile_records", [1, 0])
@pytest.mark.parametrize("cap", [1, 5])
@pytest.mark.parametrize("name", S.PUT_GRID_CASES)
def test_put_grid_cap(name, cap, tile_records):
    _put(S.PUTS[name], grid_cap=cap, tile_records=tile_records)


# ---------------------------------------------------------------------------------------------
# k_self through the Python API
# ---------------------------------------------------------------------------------------------
def _twin(c, rng):
    """The compact host twin of a self case, exchanged by the oracle: (logical start, logical
    expected), indexed (x, y, z). Interior values are non-zero in every byte's worth of the
    element; the halo starts as zeros and is filled completely."""
    dt = np.dtype(c.dtype)
    shape = c.shape
    a_mem = np.zeros(shape[::-1], dtype=dt)
    logical = a_mem.transpose(2, 1, 0)
    inner = tuple(slice(h, h + n) for h, n in zip(c.halo, c.N))
    hi = 256 if dt.itemsize == 1 else 30000
    vals = rng.integers(1, hi, size=c.N)
    logical[inner] = (vals + 1j * rng.integers(1, hi, size=c.N)) if dt.kind == "c" else vals
    start = logical.copy()
    dom = orc.RegularDomain(0, (0, 0, 0), tuple(n - 1 for n in c.N))
    spec = orc.FieldSpec(a_mem, dt.itemsize, (2, 1, 0), c.halo, shape)
    opat = orc.regular_make_pattern([[dom]], dom.first, dom.last, c.halos6, (1, 1, 1))
    orc.regular_exchange([[(spec, 0, 0, 0)]], {0: opat}, 1)
    assert not np.any(logical == 0)  # the whole halo is filled
    return start, logical


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("name", list(S.SELF_CASES))
def test_self_exchange_forms(name, fuse):
    """One periodic domain whose field is a padded, possibly shifted view of a sentinel arena.
    Before the exchange: the form of every pair from twin plans and the real pointers equals the
    host test's. After: the view equals the oracle's exchange on a compact twin, fused and
    unfused, and no byte outside the view's cells was written."""
    import torch
    from ghex_amd import make_context
    from ghex_amd.structured import regular as R
    c = S.SELF_CASES[name]
    start, want = _twin(c, np.random.default_rng(17))
    e = c.elem
    cells = c.shift + c.ext[0] * c.ext[1] * c.ext[2]
    span = c.shift + sum((n - 1) * s for n, s in zip(c.shape, c.strides)) + 1
    assert span <= cells and all(x >= n for x, n in zip(c.ext, c.shape))
    arena = torch.zeros(2 * S.GUARD + cells * e, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 256 == 0
    base = arena[S.GUARD:S.GUARD + cells * e].view(getattr(torch, c.dtype))
    view = torch.as_strided(base, c.shape, c.strides, base.storage_offset() + c.shift)
    assert view.data_ptr() == arena.data_ptr() + S.GUARD + c.shift * e
    view.copy_(torch.from_numpy(start))
    ctx = make_context()
    dd, pc = S.self_pattern(c, ctx)
    fd = R.make_field_descriptor(dd, view, c.halo, c.shape)
    ref = S.self_field_desc(c)
    assert fd.layout == (2, 1, 0) and fd.desc.elem_size == e
    assert list(fd.desc.byte_strides[:3]) == list(ref.byte_strides[:3])
    assert list(fd.desc.offsets[:3]) == list(ref.offsets[:3])
    with S.tuned(S.self_twin_knobs(c)):
        pairs = S.self_pairs(fd.desc, pc)
    with S.tuned(c.knobs) as t:
        co = R.make_communication_object(ctx, fuse_self=fuse)
        plan = co.plan([pc(fd)])
        assert co.all_self(plan)
        send, _ = co.buffers(plan, view.device)
        # the twin plans lay the one buffer out as the exchange does: same bytes, no gaps
        total = sum(s.bytes for s, _ in pairs)
        assert pairs[-1][0].buf_off + pairs[-1][0].bytes == total
        assert len(plan.send) == 1 and plan.send[0]["size"] == total
        assert len(send) == 1 and send[0].numel() == total
        forms = S.self_forms(pairs, view.data_ptr(), send[0].data_ptr())
        assert forms == S.self_forms(pairs, c.shift * e, 0)
        if name.startswith("split"):
            assert sum(f[0] == "split" for f in forms) == 18
            if name == "split_walk":  # each of the five workgroups: a split tile after a forward
                for w in S.self_workgroup_walks(pairs, forms, 5):
                    assert ("forward", "split") in set(zip(w, w[1:]))
        else:
            assert {f[0] for f in forms} == {"forward"}
        assert t.in_force() and S.knobs_in_force() == dict(c.knobs)
        co.exchange([pc(fd)]).wait()
        torch.cuda.synchronize()
    np.testing.assert_array_equal(view.cpu().numpy(), want)
    view.zero_()
    assert _nonzero(arena) == 0  # nothing outside the view's cells was written


@pytest.mark.parametrize("dtype", ["uint8", "int16", "float32"])
def test_mixed_pack_only_peer_tiles_below_16_bytes(dtype):
    """Two emulated ranks side by side in x, halo 1, mixed plans forced: the peer messages (x
    faces, edges and corners: rows of one element) are the pack-only tiles of k_self, at 1, 2
    and 4-B vectors; the y and z wrap stays on the rank and is forwarded. Every cell equals the
    oracle's exchange."""
    from ghex_amd import _ghx
    from ghex_amd.structured import regular as R
    from tests.gpu_util import FakeContext, device_field, emulated_exchange
    N, Hw, parts = 6, 1, (2, 1, 1)
    ranks, gf, gl = H.cube_domains(N, parts)
    table = {r: [(d.id, d.first, d.last) for d in ranks[r]] for r in range(2)}
    opat = orc.regular_make_pattern(ranks, gf, gl, (Hw,) * 6, (1, 1, 1))
    elem = np.dtype(dtype).itemsize
    cos, bis, bases, arrs, rf = [], [], [], [], []
    for r in range(2):
        ctx = FakeContext(r, 2, table)
        dd = R.DomainDescriptor(ranks[r][0].id, ranks[r][0].first, ranks[r][0].last)
        pc = R.make_pattern(ctx, R.HaloGenerator(gf, gl, (Hw,) * 6, (1, 1, 1)), [dd])
        a, spec = H.linear_index_field(ranks[r][0], N, Hw, gl, dtype=np.dtype(dtype))
        base, logical = device_field(a.copy(), (2, 1, 0))
        fd = R.make_field_descriptor(dd, logical, (Hw,) * 3, (N + 2 * Hw,) * 3)
        assert base.data_ptr() % 16 == 0
        peer = 0
        for _, rank, _, spaces in pc.send_halos(0):
            if rank == r:
                continue
            with A.Plan(A.entry(fd.desc, [(sp[0], sp[1]) for sp in spaces]), 0) as p:
                for s in p.segments():  # each key packs into a buffer of its own, from offset 0
                    assert S.launch_form(s, 0, 0, 0) == ("tile", elem, int(elem == 4))
                    peer += 1
        assert peer == 18  # both x faces with their edges and corners
        cos.append(R.make_communication_object(ctx))
        bis.append([pc(fd)])
        bases.append(base)
        arrs.append(a)
        rf.append([(spec, ranks[r][0].id, 0, 0)])
    orc.regular_exchange(rf, {0: opat}, 2)
    _ghx.call("ghx_tune", b"mixed_always", 1)
    try:
        plans, bufs = emulated_exchange(cos, bis, mixed=True)
    finally:
        _ghx.call("ghx_tune", b"reset", 0)
    assert emulated_exchange.mixed_ranks == 2
    for send, _ in bufs:
        assert all(t.data_ptr() % 16 == 0 for t in send)
    for b, a, doms in zip(bases, arrs, ranks):
        np.testing.assert_array_equal(b.cpu().numpy(), a)
        np.testing.assert_array_equal(a, H.expected_linear_halo(a, doms[0], N, Hw, gl))
