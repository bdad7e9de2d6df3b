"""The index-list pack that also completes the self messages, on the device (ghx_umixed_create,
k_pack_self_u), and the communication object's fuse_lists_mixed option.

Kernel cases through the ABI: every field and every buffer in an arena of its own between
256-byte guard bands (source fields hold random bytes, fields that are only written and all
buffers the sentinel), built twice from the same seed. One set gets ONE ghx_uself_execute of the
mixed plan; the other the two-launch form it must equal: a ghx_uplan pack of every entry, then a
ghx_uplan unpack of the self messages' entries from the same buffers. Every byte of every arena
is compared between the sets, the message bytes also with the NumPy form of the definition
(tests/uput_cases.py, tests/uself_cases.py), and every buffer byte outside a message must still
be the sentinel.

Product path: the known-answer case as two emulated ranks of two domains, forty random meshes
with the mixed ranks worked out from the geometry alone, and graph replay. Every comparison is
bit-exact."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import umixed_cases as UM
from tests import uput_cases as UC
from tests import uself_cases as US
from tests.uput_cases import N_CELLS, Side, udesc
from tests.test_gpu_uput import BIAS, SENTINEL, RUN_PATTERNS, Arena, _mode_descs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ghex_amd
    ghex_amd.native_library()


@pytest.fixture(autouse=True)
def _reset_knobs():
    from ghex_amd import _ghx
    yield
    _ghx.call("ghx_tune", b"reset", 0)


def _up(x, a):
    return (x + a - 1) // a * a


# ---------------------------------------------------------------------------------------------
# kernel cases
# ---------------------------------------------------------------------------------------------
def run_mixed(selfs, peers, fshift=None, bshift=None, bias=(), seed=0):
    """selfs: [(source desc, target desc, source slot, target slot, source lids, target lids,
    buffer slot, buffer offset)], peers: [(desc, field slot, lids, buffer slot, buffer offset)];
    all field slots index ONE pointer array. fshift / bshift: {slot: bytes the field / buffer is
    moved off its 256-byte alignment}; bias: field slots whose tables are int64 (their lids carry
    BIAS, their pointer is moved back by it). Returns (self segments, peer segments)."""
    import torch
    from ghex_amd import _ghx
    fshift, bshift = fshift or {}, bshift or {}
    nf = 1 + max([max(m[2], m[3]) for m in selfs] + [p[1] for p in peers])
    nb = 1 + max([m[6] for m in selfs] + [p[3] for p in peers])
    readers = {k: [m[0] for m in selfs if m[2] == k] + [p[0] for p in peers if p[1] == k] for k in range(nf)}
    writers = {k: [m[1] for m in selfs if m[3] == k] for k in range(nf)}

    def arenas():
        rng = np.random.default_rng(3000 + seed)
        fields, bufs = [], []
        for k in range(nf):
            descs = readers[k] + writers[k]
            span = max(UC.span_bytes(d) for d in descs)
            fields.append(Arena(span, fshift.get(k, 0), rng if readers[k] else None))
        for b in range(nb):
            ends = [m[7] + US.message_bytes(Side(m[0], 0, m[4])) for m in selfs if m[6] == b]
            ends += [p[4] + US.message_bytes(Side(p[0], 0, p[2])) for p in peers if p[3] == b]
            bufs.append(Arena(max(ends) + 40, bshift.get(b, 0)))
        return fields, bufs

    def lids(slot, l):
        return np.asarray(l) + (BIAS if slot in bias else 0)

    back = []
    for k in range(nf):
        steps = {d.index_stride * d.elem_size for d in readers[k] + writers[k]}
        assert k not in bias or len(steps) == 1   # one pointer serves every biased table of the slot
        back.append(BIAS * steps.pop() if k in bias else 0)
    srcs = [Side(m[0], m[2], lids(m[2], m[4])) for m in selfs]
    dsts = [Side(m[1], m[3], lids(m[3], m[5])) for m in selfs]
    places = [(m[6], m[7]) for m in selfs]
    psides = [Side(p[0], p[1], lids(p[1], p[2])) for p in peers]
    pplaces = [(p[3], p[4]) for p in peers]
    stream = torch.cuda.current_stream().cuda_stream

    def pointers(fields, bufs):
        return (_ghx.ptr_array([a.ptr - bk for a, bk in zip(fields, back)]),
                _ghx.ptr_array([a.ptr for a in bufs]))

    # ONE launch
    fields, bufs = arenas()
    h = UM.create(srcs, dsts, places, psides, pplaces)
    try:
        ssegs, psegs = UM.self_segments(h), UM.peer_segments(h)
        fp, bp = pointers(fields, bufs)
        _ghx.call("ghx_uself_execute", h, fp, nf, bp, nb, stream)
        torch.cuda.synchronize()
    finally:
        US.destroy(h)
    # the two launches it must equal: pack of every entry, unpack of the self messages
    rfields, rbufs = arenas()
    pack = UM.PackPlan(srcs + psides, places + pplaces, 0)
    unpack = UM.PackPlan(dsts, places, 1)
    try:
        fp, bp = pointers(rfields, rbufs)
        pack.execute(fp, nf, bp, nb, stream)
        unpack.execute(fp, nf, bp, nb, stream)
        torch.cuda.synchronize()
    finally:
        pack.destroy()
        unpack.destroy()
    # and the definition
    want_f = [a.host.copy() for a in fields]
    want_b = [a.host.copy() for a in bufs]
    written = [np.zeros(a.host.size, dtype=bool) for a in bufs]
    for m in selfs:
        s, t = Side(m[0], 0, m[4]), Side(m[1], 0, m[5])
        UC.apply_put(fields[m[2]].field(), want_f[m[3]][fields[m[3]].at:], s, t)
        US.packed(fields[m[2]].field(), s, m[7], want_b[m[6]][bufs[m[6]].at:])
        written[m[6]][bufs[m[6]].at + m[7]:bufs[m[6]].at + m[7] + US.message_bytes(s)] = True
    for p in peers:
        s = Side(p[0], 0, p[2])
        US.packed(fields[p[1]].field(), s, p[4], want_b[p[3]][bufs[p[3]].at:])
        written[p[3]][bufs[p[3]].at + p[4]:bufs[p[3]].at + p[4] + US.message_bytes(s)] = True
    for got_set, ref_set, want in ((fields, rfields, want_f), (bufs, rbufs, want_b)):
        for a, r, w in zip(got_set, ref_set, want):
            got = a.device_bytes()
            np.testing.assert_array_equal(got, r.device_bytes())   # guard bands included
            np.testing.assert_array_equal(got, w)
    for a, wr in zip(bufs, written):
        got = a.device_bytes()
        assert wr.any() and (got[~wr] == SENTINEL).all()           # pad bytes and guards untouched
        assert (got[wr] != SENTINEL).any()
    for k in range(nf):
        if writers[k]:
            assert (want_f[k] != fields[k].host).sum() > 0
    return ssegs, psegs


def standard(sd, dd, pds, seed=0, repeats=False, boff=0, pboff=0, align=16, **kw):
    """Fields 0 and 1 send, 2 and 3 receive. Self messages of 1031, 257 and 5 lids: the first two
    share buffer 0 (the second `align`ed behind the first), the third opens buffer 1. Peer
    messages: 1031 lids of field 0 and 3 lids of field 1 in buffer 2 with a pad gap between them,
    1 lid of field 2 (a receiving field: a cell no self message writes, in that field's own
    layout dd) alone in buffer 3, and 257 lids of field 0 behind the self message in buffer 1.
    pds: the descriptors of the peers on the sending fields, cycled."""
    rng = np.random.default_rng(seed)
    s0, s1, s2, p0, p1, p3 = UC.draw_lists(rng, (1031, 257, 5, 1031, 3, 257))
    t0, t1, t2, p2 = UC.draw_lists(rng, (1031, 257, 5, 1))
    if repeats:
        s0[1:800:7] = s0[0]        # one cell sent many times
        s2[-1] = s1[-1]            # a cell sent in two self messages
        p0[5:900:3] = p0[2]        # and by the peers: many times, and a cell a self message sends too
        p3[0] = s0[3]
    nb0 = US.message_bytes(Side(sd, 0, s0))
    selfs = [(sd, dd, 0, 2, s0, t0, 0, boff), (sd, dd, 1, 3, s1, t1, 0, _up(boff + nb0, align)),
             (sd, dd, 0, 3, s2, t2, 1, boff)]
    pd = [pds[j % len(pds)] for j in range(4)]
    pd[2] = dd   # cells are (field slot, lid): every entry of a written field describes its one layout
    end1 = _up(boff + US.message_bytes(Side(sd, 0, s2)), 16)
    end2 = pboff + US.message_bytes(Side(pd[0], 0, p0))
    peers = [(pd[0], 0, p0, 2, pboff), (pd[1], 1, p1, 2, _up(end2, 16) + 48 + pboff % 16),
             (pd[2], 2, p2, 3, pboff), (pd[3], 0, p3, 1, end1 + 32 + pboff % 16)]
    return run_mixed(selfs, peers, seed=seed, **kw)


def _peer_desc(mode, e):
    """One side's descriptor that a pack plan decomposes in `mode` (strided levels for mode 1)."""
    return _mode_descs(mode, e)[1 if mode == 1 else 0]


@pytest.mark.parametrize("e", [1, 2, 4, 8, 16, 3, 12])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_every_mode_and_width_with_the_other_modes_as_peers(mode, e):
    """Self messages in `mode`, peer messages in the two other modes, in one launch."""
    sd, dd = _mode_descs(mode, e)
    pds = [_peer_desc((mode + 1) % 3, e), _peer_desc((mode + 2) % 3, e)]
    ssegs, psegs = standard(sd, dd, pds, seed=mode * 16 + e, align=16 if e not in (3, 12) else e)
    w = {3: 1, 12: 4}.get(e, e)
    assert all(g.mode == mode and 1 << g.wlog2 == w for g in ssegs)
    assert sorted({g.mode for g in psegs[:2] + psegs[3:]}) == sorted({(mode + 1) % 3, (mode + 2) % 3})
    assert psegs[2].mode == mode
    assert all(1 << g.wlog2 == w for g in psegs)
    assert -(-ssegs[0].bytes // ssegs[0].tile_bytes) > 1 and -(-psegs[0].bytes // psegs[0].tile_bytes) > 1


RUN_SIZES = [(1, (0, 20)), (3, (20, 40)), (5, (40, 60)), (257, (100, 1500)), (1031, (2000, N_CELLS))]


def _run_case(L, pattern, seed, sd=None, dd=None, pd=None, peer_pattern=None, pboff=0, **kw):
    """Self messages of 1, 3, 5, 257 and 1031 lids from field 0 into field 1 back to back in
    buffer 0 at 16-byte aligned offsets, and peer messages of the same sizes from field 0 (1031,
    5, 1) and field 2 (257, 3) in buffers 1 and 2: chunks of 16/L rows see tails of every length."""
    rng = np.random.default_rng(seed)
    sd, dd, pd = sd or udesc(L), dd or udesc(L), pd or udesc(L)
    gs, gt = RUN_PATTERNS[pattern]
    gp = RUN_PATTERNS[peer_pattern or pattern][0]
    selfs, peers, at = [], [], 0
    pat = {1: pboff, 2: pboff}
    for k, (n, (lo, hi)) in enumerate(RUN_SIZES):
        selfs.append((sd, dd, 0, 1, gs(rng, n, lo, hi), gt(rng, n, lo, hi), 0, at))
        at = _up(at + n * sd.elem_size * sd.levels, 16)
        slot, b = (0, 1) if k % 2 == 0 else (2, 2)
        peers.append((pd, slot, gp(rng, n, lo, hi), b, pat[b]))
        pat[b] = _up(pat[b] + n * pd.elem_size * pd.levels, 16) + pboff % 16
    return run_mixed(selfs, peers, seed=seed, **kw)


@pytest.mark.parametrize("pattern", ["runs-runs", "mixed-mixed", "scattered-runs", "runs-scattered"])
@pytest.mark.parametrize("L", [4, 8])
def test_run_path_on_both_parts(L, pattern):
    ssegs, psegs = _run_case(L, pattern, seed=100 + L)
    assert [g.n for g in ssegs] == [1, 3, 5, 257, 1031] == sorted(g.n for g in psegs)
    assert all(g.src_runs and g.dst_runs and g.mode == 0 for g in ssegs)
    assert all(g.runs and g.mode == 0 for g in psegs)


def test_run_eligible_self_messages_beside_peers_that_are_not_and_the_reverse():
    ssegs, psegs = _run_case(8, "mixed-mixed", seed=110, pd=udesc(8, 3))
    assert all(g.src_runs and g.dst_runs for g in ssegs) and not any(g.runs for g in psegs)
    ssegs, psegs = _run_case(8, "mixed-mixed", seed=111, sd=udesc(8, 3), dd=udesc(8, 3), pd=udesc(8))
    assert not any(g.src_runs or g.dst_runs for g in ssegs) and all(g.runs for g in psegs)
    # a peer whose buffer offset is a multiple of the row only: the planner clears its flag
    ssegs, psegs = _run_case(4, "runs-runs", seed=112, pboff=4)
    assert all(g.src_runs for g in ssegs) and not any(g.runs for g in psegs)
    # and pointers that decide at the launch: a peer-only field, a peer-only buffer, a self field
    for kw in (dict(fshift={2: 4}), dict(bshift={2: 8}), dict(fshift={1: 8}), dict(bshift={0: 4}),
               dict(fshift={2: 1})):
        ssegs, psegs = _run_case(8, "mixed-mixed", seed=113, **kw)
        assert all(g.src_runs and g.dst_runs for g in ssegs) and all(g.runs for g in psegs)


def test_run_path_off_by_knob():
    from ghex_amd import _ghx
    _ghx.call("ghx_tune", b"urun", 0)
    ssegs, psegs = _run_case(8, "mixed-mixed", seed=120)
    assert not any(g.src_runs or g.dst_runs for g in ssegs) and not any(g.runs for g in psegs)
    _run_case(4, "runs-runs", seed=121)


@pytest.mark.parametrize("bias", [(0,), (2,), (3,), (1,), (0, 1, 2, 3)], ids=str)
def test_int64_tables_on_either_part(bias):
    """Field 0: read by self and peer messages; 1: by both; 2: written, and read by a peer; 3:
    written only."""
    sd = udesc(8, 2)
    ssegs, psegs = standard(sd, sd, [sd], seed=130, bias=bias)
    assert [g.src_lid64 for g in ssegs] == [int(0 in bias), int(1 in bias), int(0 in bias)]
    assert [g.dst_lid64 for g in ssegs] == [int(2 in bias), int(3 in bias), int(3 in bias)]
    assert [g.lid64 for g in psegs] == [int(0 in bias), int(1 in bias), int(2 in bias), int(0 in bias)]
    sd, dd = _mode_descs(1, 4)
    standard(sd, sd, [sd], seed=131, bias=bias)
    ssegs, psegs = _run_case(8, "mixed-mixed", seed=132, bias=bias[:1])
    assert all(g.runs for g in psegs)


@pytest.mark.parametrize("kw", [dict(fshift={1: 4}), dict(fshift={3: 2}), dict(bshift={3: 8}), dict(bshift={2: 1}),
                                dict(bshift={0: 4}), dict(boff=8), dict(pboff=4), dict(pboff=2, boff=16)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_width_narrowed_on_one_part_only(kw):
    """Field 1 is read by self message 1 and peer 1, field 3 written by self messages only; buffer
    3 holds a peer message alone, buffer 2 two peer messages, buffer 0 two self messages. A
    pointer narrows at the launch, a buffer offset in the plan."""
    sd, dd = udesc(16, 2), udesc(16, 2, index_stride=3)
    ssegs, psegs = standard(sd, dd, [udesc(16, 3, first=False), sd], seed=140, align=1 if "boff" in kw else 16, **kw)
    want_s = {8: 3}.get(kw.get("boff", 0), 4)
    want_p = {4: 2, 2: 1}.get(kw.get("pboff", 0), 4)
    assert ssegs[0].wlog2 == want_s and psegs[0].wlog2 == want_p and psegs[2].wlog2 == want_p


@pytest.mark.parametrize("knobs", [{"u_tile_rows": 3, "u_tile_bytes": 1024}, {"u_run_tile_rows": 64},
                                   {"u_tile_rows": 3, "u_tile_bytes": 1024, "u_run_tile_rows": 64, "grid_cap": 5},
                                   {"small_row_bytes": 4096, "u_tile_rows": 5},
                                   {"tile_records": 0, "order": 0}],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_tiling_knobs_stay_bit_exact(knobs):
    from ghex_amd import _ghx
    for k, v in knobs.items():
        _ghx.call("ghx_tune", k.encode(), v)
    for mode, e in ((0, 4), (1, 16), (2, 8), (0, 3)):
        sd, dd = _mode_descs(mode, e)
        standard(sd, dd, [_peer_desc((mode + 1) % 3, e), sd], seed=200 + mode, align=16 if e != 3 else 1)
    for L in (4, 8):
        _run_case(L, "mixed-mixed", seed=210 + L)
        _run_case(L, "runs-scattered", seed=220 + L, peer_pattern="scattered-runs")


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_one_workgroup_crosses_from_self_tiles_into_peer_tiles(cap):
    """grid_cap workgroups walk every tile grid-stride: each runs tiles of both kinds."""
    from ghex_amd import _ghx
    _ghx.call("ghx_tune", b"grid_cap", cap)
    _ghx.call("ghx_tune", b"u_tile_rows", 100)
    sd, dd = _mode_descs(1, 8)
    ssegs, psegs = standard(sd, dd, [udesc(8, 3), _peer_desc(2, 4)], seed=300 + cap)
    n_self = sum(-(-g.bytes // g.tile_bytes) for g in ssegs)
    n_peer = sum(-(-g.bytes // g.tile_bytes) for g in psegs)
    assert n_self > 2 * cap and n_peer > 2 * cap
    _run_case(8, "mixed-mixed", seed=310 + cap)
    _run_case(4, "runs-runs", seed=320 + cap, pd=udesc(4, 3))


def test_repeated_source_lids():
    standard(udesc(8, 2), udesc(8, 2), [udesc(8, 2), udesc(4, 3, first=False)], seed=400, repeats=True)
    sd, dd = _mode_descs(2, 4)
    standard(sd, dd, [udesc(4)], seed=401, repeats=True)
    rng = np.random.default_rng(402)
    rep = np.repeat(rng.integers(0, 50, size=300), 4)[:1031].astype(np.int64)   # runs of equal lids
    t = UC.draw_lists(rng, (1031,))[0]
    run_mixed([(udesc(8), udesc(8), 0, 1, rep, t, 0, 0)], [(udesc(8), 0, rep[::-1].copy(), 1, 0)], seed=402)


# ---------------------------------------------------------------------------------------------
# product path: two emulated ranks in one process
# ---------------------------------------------------------------------------------------------
def _count(fn):
    """fn's kernel launches (ghx_launch_timing counts them on this thread)."""
    from ghex_amd import _ghx
    ms, n = (ctypes.c_float * 64)(), ctypes.c_int32()
    _ghx.call("ghx_launch_timing", 1)
    try:
        fn()
        _ghx.call("ghx_launch_timing_read", ms, 64, ctypes.byref(n))
    finally:
        _ghx.call("ghx_launch_timing", 0)
    return n.value


def emulated_mixed_exchange(cos, bis_per_rank, counts=None):
    """tests.gpu_util.emulated_exchange with the index-list mixed launches on every rank whose
    plan has them (lists_mixed) and the plain ones elsewhere: pack on every rank, peer send
    buffers copied to the matching recv buffers by (rank, tag, pair), unpack on every rank.
    counts, if given, gains per mixed rank (pack launches, unpack launches, whether the rank
    receives from a peer: 1 or 0, the unpack launches it must then have)."""
    import torch
    plans, bufs, used = [], [], []
    for co, bis in zip(cos, bis_per_rank):
        m = co.lists_mixed(co.plan(bis))
        out = []
        n = _count(lambda: out.append(co.pack_lists_self_only(bis) if m else co.pack_only(bis)))
        plan, send, recv = out[0]
        plans.append(plan)
        bufs.append((send, recv))
        used.append((m, n))
    for r, plan in enumerate(plans):
        for i, x in enumerate(plan.recv):
            if x["rank"] == r:
                continue  # self message: recv buffer aliases the send buffer
            src = x["rank"]
            j = next(j for j, s in enumerate(plans[src].send) if s["pair"] == x["pair"] and s["rank"] == r)
            assert plans[src].send[j]["tag"] == x["tag"] and plans[src].send[j]["size"] == x["size"]
            bufs[r][1][i][:x["size"]].copy_(bufs[src][0][j][:x["size"]])
    for co, bis, (m, n) in zip(cos, bis_per_rank, used):
        k = _count(lambda: co.unpack_list_peers_only(bis) if m else co.unpack_only(bis))
        if m and counts is not None:
            counts.append((n, k, int(any(x["rank"] != co.context.rank() for x in co.plan(bis).recv))))
    torch.cuda.synchronize()
    return plans, bufs, [m for m, _ in used]


def _two_ranks(golden_dir, levels, levels_first, **options):
    """The known-answer case as two emulated ranks of two domains: (communication objects, buffer
    infos per rank, [(domain, device tensor, initial host array, expected host array)]);
    value(dom, gid, level) = dom*10000 + gid*100 + level in owned cells, -1 in halos."""
    import torch
    from ghex_amd import unstructured as U
    from tests.gpu_util import FakeContext, unstructured_patterns
    with open(os.path.join(golden_dir, "unstructured_case.json")) as fh:
        case = json.load(fh)
    doms = [case["domains"][str(r)] for r in range(4)]
    pats = unstructured_patterns([[(r, doms[r]["gids"], doms[r]["halo_lids"]) for r in rs] for rs in ((0, 1), (2, 3))])
    table = {0: [], 1: []}
    cos, bis_all, fields = [], [], []
    for rank, rs in enumerate(((0, 1), (2, 3))):
        dds, pc = pats[rank]
        bis = []
        for r, dd in zip(rs, dds):
            d = doms[r]
            n = len(d["gids"])
            init = np.full((n, levels), -1, dtype=np.float64)
            for lid, gid in enumerate(d["gids"]):
                if lid not in d["halo_lids"]:
                    init[lid] = [r * 10000 + gid * 100 + l for l in range(levels)]
            want = init.copy()
            for rid, rr, tag, lids in pc.recv_halos(pc.local_index(r)):
                for lid in lids:
                    want[lid] = [rid * 10000 + d["gids"][lid] * 100 + l for l in range(levels)]
            assert (want >= 0).all()
            t = torch.from_numpy(init).cuda()
            if not levels_first:
                t = torch.empty_strided((n, levels), (1, n), dtype=t.dtype, device="cuda").copy_(t)
            fd = U.make_field_descriptor(dd, t)
            assert fd.levels_first == levels_first
            bis.append(pc(fd))
            fields.append((r, t, init, want))
        cos.append(U.make_communication_object(FakeContext(rank, 2, table), **options))
        bis_all.append(bis)
    return cos, bis_all, fields


def _rewrite(fields, scale=1):
    import torch
    for r, t, init, want in fields:
        t.copy_(torch.from_numpy(np.where(init < 0, init, init * scale)).to(t.device))


def _check_fields(fields, scale=1):
    for r, t, init, want in fields:
        np.testing.assert_array_equal(t.cpu().numpy(), want * scale)


def _message_bytes(plans, bufs):
    return [t[:x["size"]].cpu().numpy() for plan, (send, _) in zip(plans, bufs) for t, x in zip(send, plan.send)]


@pytest.mark.parametrize("levels, levels_first", [(1, True), (3, True), (1, False), (3, False)])
def test_known_answer_case_on_two_ranks_of_two_domains(golden_dir, levels, levels_first):
    from tests.gpu_util import emulated_exchange
    cos, bis_all, fields = _two_ranks(golden_dir, levels, levels_first, fuse_lists_mixed=True)
    dcos, dbis_all, dfields = _two_ranks(golden_dir, levels, levels_first)
    assert not any(co.fuse_lists_mixed for co in dcos)
    for co, bis in zip(cos, bis_all):
        plan = co.plan(bis)
        assert co.lists_mixed(plan) and not co.mixed(plan) and not co.lists_self(plan)
    for k in (1, 2):
        _rewrite(fields, k)
        _rewrite(dfields, k)
        counts = []
        plans, bufs, used = emulated_mixed_exchange(cos, bis_all, counts)
        assert used == [True, True] and counts == [(1, 1, 1), (1, 1, 1)]
        dplans, dbufs = emulated_exchange(dcos, dbis_all)
        _check_fields(fields, k)
        _check_fields(dfields, k)
        for (_, a, _, _), (_, b, _, _) in zip(fields, dfields):
            np.testing.assert_array_equal(np.ascontiguousarray(a.cpu().numpy()).view(np.uint8),
                                          np.ascontiguousarray(b.cpu().numpy()).view(np.uint8))
        got, exp = _message_bytes(plans, bufs), _message_bytes(dplans, dbufs)
        assert len(got) == len(exp) == 12
        for g, e in zip(got, exp):
            np.testing.assert_array_equal(g, e)


def _ranks_with_self_and_peer_messages(case):
    """From the mesh alone: the ranks that hold a halo cell owned by another of their own domains
    (a self message) and exchange a halo cell with another rank, in either direction."""
    owner = {}
    for d in case["doms"]:
        outer = set(d["outer"])
        owner.update({g: d["rank"] for lid, g in enumerate(d["gids"]) if lid not in outer})
    out = set()
    for r in range(case["nr"]):
        pairs = [(d["rank"], owner[d["gids"][lid]]) for d in case["doms"] for lid in d["outer"]]
        if (r, r) in pairs and any((a == r) != (b == r) for a, b in pairs):
            out.add(r)
    return out


def test_the_random_meshes_hold_mixed_ranks_in_at_least_20_seeds():
    from tests.test_gpu_fuzz import draw_unstructured
    ranks = [_ranks_with_self_and_peer_messages(draw_unstructured(seed)) for seed in range(40)]
    assert sum(1 for r in ranks if r) >= 20
    assert (sum(len(r) for r in ranks), sum(1 for r in ranks if r)) == (49, 25)


@pytest.mark.parametrize("seed", range(40))
def test_random_meshes_equal_the_default_path(seed):
    import torch
    from ghex_amd import unstructured as U
    from tests.gpu_util import emulated_exchange
    from tests.test_gpu_fuzz import _check_unstructured, _setup_unstructured, draw_unstructured
    expect = _ranks_with_self_and_peer_messages(draw_unstructured(seed))
    results = []
    for fuse in (True, False):
        case = draw_unstructured(seed)
        cos, bis_all, recs = _setup_unstructured(case)
        cos = [U.make_communication_object(co.context, fuse_lists_mixed=fuse) for co in cos]
        sends = []
        for co, bis in zip(cos, bis_all):
            if not bis:
                continue
            # the send buffers start from the sentinel: bytes no launch writes compare equal
            send, _ = co.buffers(co.plan(bis), bis[0].field.device)
            for t in send:
                t.fill_(SENTINEL)
            sends += [t[:x["size"]] for t, x in zip(send, co.plan(bis).send)]
        if fuse:
            assert {r for r, (co, bis) in enumerate(zip(cos, bis_all)) if co.lists_mixed(co.plan(bis))} == expect
            counts = []
            _, _, used = emulated_mixed_exchange(cos, bis_all, counts)
            assert {r for r, m in enumerate(used) if m} == expect
            assert len(counts) == len(expect) and all(n == 1 and k == peer for n, k, peer in counts)
        else:
            emulated_exchange(cos, bis_all)
        _check_unstructured(case, recs)
        results.append(([t.clone() for (_, _, t, _) in recs], [t.clone() for t in sends]))
    (ff, fb), (pf, pb) = results
    assert len(ff) == len(pf) and len(fb) == len(pb)
    for a, b in zip(ff, pf):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for a, b in zip(fb, pb):
        assert torch.equal(a, b)


def test_mixed_launches_replayed_from_a_capture(golden_dir):
    """Rank 0's two launches captured once, replayed twice from rewritten fields (new owned values,
    stale halos overwritten by -1) after rank 1's send buffers were copied into its recv buffers."""
    import torch
    cos, bis_all, fields = _two_ranks(golden_dir, 3, True, fuse_lists_mixed=True)
    plans, bufs, _ = emulated_mixed_exchange(cos, bis_all)   # set-up and a warm run, outside the capture
    _check_fields(fields)
    co, bis = cos[0], bis_all[0]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        co.pack_lists_self_only(bis)
        co.unpack_list_peers_only(bis)
    for k in (3, 5):
        _rewrite(fields, k)
        cos[1].pack_only(bis_all[1])
        for i, x in enumerate(plans[0].recv):
            if x["rank"] == 1:
                j = next(j for j, s in enumerate(plans[1].send) if s["pair"] == x["pair"] and s["rank"] == 0)
                bufs[0][1][i][:x["size"]].copy_(bufs[1][0][j][:x["size"]])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _check_fields(fields[:2], k)
