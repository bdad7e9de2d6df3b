"""Device parity of the index-list general path (copy_tile_u through k_copy<*, seg_u, RUNS =
false>) in every row form, vector width, lid-table width and tiling: the cases of
tests/unstructured_cases.py packed and unpacked through ghx_uplan_create / ghx_uplan_execute,
each asserting through ghx_uplan_segment which form the launch takes before it runs.

Reference: the numpy int64 enumeration of the field byte offset of every message element
(unstructured_cases.element_offsets), which tests/test_unstructured_cases.py ties to the pinned
oracle. Everything is bit-exact. Every field lives in a zero-filled (sentinel) device arena with
message bytes in 1..255 and guard bands sized on the host so that the accesses of the two offset
forms a segment must NOT take stay inside the arena as well (test_arena_closure): a kernel that
decodes with the wrong form lands in sentinel memory and fails the comparison instead of
faulting. The two far cases put offsets past 2^32 into one 4.5-GiB arena whose base is the field
pointer, so an offset truncated to 32 bits stays inside it too."""
import ctypes
import functools

import numpy as np
import pytest

from tests import unstructured_cases as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ghex_amd
    ghex_amd.native_library()


@pytest.fixture(scope="module")
def far_arena():
    import torch
    t = torch.zeros(U.FAR_ARENA_BYTES, dtype=torch.uint8, device="cuda")
    yield t
    del t
    torch.cuda.empty_cache()


def _nonzero_bytes(t):
    """Non-sentinel bytes of a buffer, counted in chunks (no second full-size tensor)."""
    import torch
    total = torch.zeros((), dtype=torch.int64, device=t.device)
    step = 256 << 20
    for a in range(0, t.numel(), step):
        total += torch.count_nonzero(t[a:a + step])
    return int(total)


def _random_bytes(n, seed):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(1, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)


@functools.lru_cache(maxsize=4)
def _device_indices(case):
    """(per-list arena byte indices, their sorted union) on the device; computed once per case
    and left unchanged."""
    import torch
    idx = [torch.from_numpy(i).cuda() for i in U.arena_indices(case)]
    return idx, torch.unique(torch.cat(idx))


def _execute(h, fptrs, bptrs):
    import torch
    from ghex_amd import _ghx
    _ghx.call("ghx_uplan_execute", h, _ghx.ptr_array(fptrs), len(fptrs), _ghx.ptr_array(bptrs),
              len(bptrs), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


class _Arena:
    """A case's field arena and buffer allocation on the device, with the pointers its plans
    are executed with. Bounds are checked on the host before anything runs."""

    def __init__(self, case, arena=None):
        import torch
        self.case, self.lay = case, U.layout(case)
        lay = self.lay
        self.arena = torch.zeros(lay.arena_bytes, dtype=torch.uint8, device="cuda") \
            if arena is None else arena
        assert self.arena.numel() == lay.arena_bytes
        self.bufs = torch.zeros(lay.buffers_bytes, dtype=torch.uint8, device="cuda")
        assert self.arena.data_ptr() % 256 == 0 and self.bufs.data_ptr() % 256 == 0
        self.idx, self.cells = _device_indices(case)
        assert int(self.cells[0]) >= 0 and int(self.cells[-1]) < lay.arena_bytes
        assert all(0 <= a and b <= lay.buffers_bytes for a, b in lay.msg)
        self.fptrs = [self.arena.data_ptr() + p for p in lay.field_ptr]
        self.bptrs = [self.bufs.data_ptr() + p for p in lay.buf_ptr]
        self.form = U.expected_form(case, self.arena.data_ptr(), self.bufs.data_ptr())
        assert not any(runs for _, _, _, runs in self.form)  # copy_tile_u for every segment

    def check_plan(self, plan):
        """The planner's records say what the table says, and with these pointers the launch
        takes the expected form."""
        segs = plan.segments()
        U.assert_planned(self.case, segs)
        assert U.launch_form(segs, self.fptrs, self.bptrs) == self.form

    def pack(self):
        import torch
        case, lay = self.case, self.lay
        self.arena.zero_()
        self.bufs.zero_()
        self.arena[self.cells] = _random_bytes(self.cells.numel(), 5)
        want = [self.arena[i] for i in self.idx]
        with U.UPlan(case, 0) as p:
            self.check_plan(p)
            _execute(p.h, self.fptrs, self.bptrs)
        for (a, b), w in zip(lay.msg, want):
            assert torch.equal(self.bufs[a:b], w)
        # nothing before buffer_offset, in the guards or between the buffers was written
        assert _nonzero_bytes(self.bufs) == case.message_bytes
        # the pack wrote nothing into the arena
        assert _nonzero_bytes(self.arena) == self.cells.numel()
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
        with U.UPlan(case, 1) as p:
            self.check_plan(p)
            _execute(p.h, self.fptrs, self.bptrs)
        for (a, b), i in zip(lay.msg, self.idx):
            assert torch.equal(self.arena[i], sent[a:b])
        # the message's cells and nothing else (a duplicate clamped store is byte-identical)
        assert _nonzero_bytes(self.arena) == case.message_bytes
        assert torch.equal(self.bufs, sent)


def _pack_and_unpack(case, arena=None):
    a = _Arena(case, arena)
    a.pack()
    if not case.repeats:
        a.unpack()


# ---------------------------------------------------------------------------------------------
# the whole table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile_records", [1, 0])
@pytest.mark.parametrize("name", U.HOST_SIZED)
def test_pack_unpack_every_form(name, tile_records):
    _pack_and_unpack(U.with_knobs(U.CASES[name], tile_records=tile_records))


@pytest.mark.parametrize("tile_records", [1, 0])
@pytest.mark.parametrize("name", U.FAR)
def test_pack_unpack_past_4gib(far_arena, name, tile_records):
    """far_m2: level_stride_b = 2^32 + 24; far_m1: lid * index_stride_b passes 2^32. A product
    or stride truncated to 32 bits addresses sentinel cells of the same arena."""
    _pack_and_unpack(U.with_knobs(U.CASES[name], tile_records=tile_records), far_arena)


# ---------------------------------------------------------------------------------------------
# tiling and launch knobs, one case per mode
# ---------------------------------------------------------------------------------------------
PER_MODE = ("m0_rows24", "m1_w8_i32", "m2_e12")
INT64_GENERAL = ("m0_long80_i64", "m1_w16_i64", "m2_w16_i64")


@pytest.mark.parametrize("rows", [1, 3, 5000])
@pytest.mark.parametrize("name", PER_MODE)
def test_u_tile_rows(name, rows):
    """One row per tile (every position but the first few clamped), three rows (tiles that start
    anywhere in a level / an index), 5000 rows (tiles of several loop trips)."""
    _pack_and_unpack(U.with_knobs(U.CASES[name], u_tile_rows=rows))


@pytest.mark.parametrize("tile_bytes", [1024, 65536])
@pytest.mark.parametrize("name", PER_MODE)
def test_u_tile_bytes_with_element_rows_counted_long(name, tile_bytes):
    _pack_and_unpack(U.with_knobs(U.CASES[name], u_tile_bytes=tile_bytes, small_row_bytes=1))


@pytest.mark.parametrize("tile_records", [1, 0])
@pytest.mark.parametrize("cap", [1, 7])
@pytest.mark.parametrize("name", PER_MODE + ("mixed",))
def test_grid_cap(name, cap, tile_records):
    """k_copy's grid-stride do ... while: one workgroup walks every tile, seven walk them with a
    stride that does not divide the tile count."""
    _pack_and_unpack(U.with_knobs(U.CASES[name], grid_cap=cap, tile_records=tile_records))


@pytest.mark.parametrize("pol", [1, 2, 3])
@pytest.mark.parametrize("W", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_short_pol(mode, W, pol):
    """seg_u::fpol on short rows: non-temporal loads (bit 0) and sc1 stores (bit 1) at 4, 8 and
    16 B; the 1- and 2-byte stores fall through to plain stores."""
    case = U.with_knobs(U.CASES[f"m{mode}_w{W}_i32"], short_pol=pol)
    assert all(p[4] < 64 for p in U.planned(case))  # short rows: the policy applies
    _pack_and_unpack(case)


@pytest.mark.parametrize("knobs", [{"u_tile_rows": 3}, {"grid_cap": 7, "tile_records": 0},
                                   {"short_pol": 3}, {"u_tile_bytes": 1024, "small_row_bytes": 1}],
                         ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
@pytest.mark.parametrize("name", INT64_GENERAL)
def test_int64_lid_tables_under_the_knobs(name, knobs):
    """The lid64 branch of copy_tile_u (lids >= 2^31: every lid biased by 2^31 + 5, the field
    pointer by the opposite amount) for mode 0 with long rows, mode 1 and mode 2."""
    case = U.with_knobs(U.CASES[name], **knobs)
    assert all(p[2] == 1 for p in U.planned(case))
    _pack_and_unpack(case)


# ---------------------------------------------------------------------------------------------
# the one-shot entry points
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lid_bytes", [("m1_w8_i32", 4), ("m1_w8_i32", 8), ("m2_w4_i32", 4),
                                            ("m2_w4_i32", 8), ("m1_w16_i64", 8),
                                            ("m2_w16_i64", 8)])
def test_one_shot_pack_unpack(name, lid_bytes):
    """ghx_unstructured_pack / ghx_unstructured_unpack, one list per call, from int32 and int64
    host lists."""
    import torch
    from ghex_amd import _ghx
    case = U.CASES[name]
    a = _Arena(case)
    lay = a.lay
    s = torch.cuda.current_stream().cuda_stream
    lists = [np.ascontiguousarray(l, dtype=np.int32 if lid_bytes == 4 else np.int64)
             for l in U.lids(case)]
    assert all(np.array_equal(x, y) for x, y in zip(lists, U.lids(case)))

    def descs():
        for l, lid, (m0, m1) in zip(case.lists, lists, lay.msg):
            f = case.fields[l.field]
            d = _ghx.UDataDesc()
            d.elem_size, d.levels, d.levels_first = f.elem, f.levels, 1 if f.levels_first else 0
            d.index_stride, d.level_stride = f.index_stride, f.level_stride
            yield d, a.fptrs[l.field], a.bufs.data_ptr() + m0, lid

    a.arena[a.cells] = _random_bytes(a.cells.numel(), 5)
    want = [a.arena[i] for i in a.idx]
    for d, fp, bp, lid in descs():
        _ghx.call("ghx_unstructured_pack", ctypes.byref(d), fp, bp, lid.ctypes.data, lid_bytes,
                  lid.size, s)
    torch.cuda.synchronize()
    for (m0, m1), w in zip(lay.msg, want):
        assert torch.equal(a.bufs[m0:m1], w)
    assert _nonzero_bytes(a.bufs) == case.message_bytes
    assert _nonzero_bytes(a.arena) == a.cells.numel()
    a.arena.zero_()
    for k, (m0, m1) in enumerate(lay.msg):
        a.bufs[m0:m1] = _random_bytes(m1 - m0, 6 + k)
    sent = a.bufs.clone()
    for d, fp, bp, lid in descs():
        _ghx.call("ghx_unstructured_unpack", ctypes.byref(d), fp, bp, lid.ctypes.data, lid_bytes,
                  lid.size, s)
    torch.cuda.synchronize()
    for (m0, m1), i in zip(lay.msg, a.idx):
        assert torch.equal(a.arena[i], sent[m0:m1])
    assert _nonzero_bytes(a.arena) == case.message_bytes
    assert torch.equal(a.bufs, sent)


# ---------------------------------------------------------------------------------------------
# through the Python API: levels-last fields with a padded level stride, every dtype
# ---------------------------------------------------------------------------------------------
# every dtype a DataDescriptor accepts (any torch dtype: it reads the element size only), by
# the integer or complex type of the same size that numpy can hold its bytes in
API_DTYPES = {"uint8": "uint8", "int8": "uint8", "bool": "uint8", "int16": "int16",
              "float16": "int16", "bfloat16": "int16", "int32": "int32", "float32": "int32",
              "int64": "int64", "float64": "int64", "complex64": "int64",
              "complex128": "complex128"}
API_CELLS, API_HALO, API_LEVELS, API_PAD = 3001, 1501, 3, 3


def _api_case():
    """Two ranks, one domain each: 3001 owned cells and a halo of 1501 cells the other owns, in
    a random storage order."""
    rng = np.random.default_rng(77)
    inner = [list(range(1000, 1000 + API_CELLS)), list(range(9000, 9000 + API_CELLS))]
    doms = []
    for r in range(2):
        halo = [int(g) for g in rng.choice(inner[1 - r], size=API_HALO, replace=False)]
        gids = inner[r] + halo
        perm = rng.permutation(len(gids))
        gids = [gids[p] for p in perm]
        outer = sorted(int(x) for x in np.nonzero(perm >= API_CELLS)[0])
        doms.append({"rank": r, "id": r, "gids": gids, "outer": outer})
    return doms


@functools.lru_cache(maxsize=1)
def _api_patterns():
    from tests.gpu_util import unstructured_patterns
    doms = _api_case()
    return doms, unstructured_patterns([[(d["id"], d["gids"], d["outer"])] for d in doms])


def _api_setup(dtype):
    """(case, cos, bis_all, recs) as tests/test_gpu_fuzz.py's _check_unstructured takes them: per
    rank an (L, n + pad) tensor of random bytes viewed as [:, :n].t(): levels last, the level
    stride padded."""
    import torch
    from ghex_amd import unstructured as UN
    from tests.gpu_util import FakeContext
    doms, pats = _api_patterns()
    f = {"dtype": np.dtype(API_DTYPES[dtype]), "levels": API_LEVELS, "first": False}
    case = {"nr": 2, "doms": doms, "fields": [f], "seed": 77}
    rng = np.random.default_rng(78)
    cos, bis_all, recs = [], [], []
    for r, d in enumerate(doms):
        dds, pc = pats[r]
        n = len(d["gids"])
        raw = rng.integers(0, 256, size=API_LEVELS * (n + API_PAD) * f["dtype"].itemsize,
                           dtype=np.uint8)
        a = raw.view(f["dtype"]).reshape(API_LEVELS, n + API_PAD).copy()
        t = torch.from_numpy(a).cuda()
        view = t.view(getattr(torch, dtype))[:, :n].t()
        fd = UN.make_field_descriptor(dds[0], view)
        assert (fd.levels_first, fd.index_stride, fd.level_stride) == (False, 1, n + API_PAD)
        assert fd.desc.elem_size == f["dtype"].itemsize
        bis_all.append([pc(fd)])
        recs.append((f, d, t, a))
        cos.append(UN.make_communication_object(FakeContext(r, 2, {0: [], 1: []})))
    return case, cos, bis_all, recs


@pytest.mark.parametrize("dtype", list(API_DTYPES))
def test_padded_levels_last_exchange(dtype):
    from tests.gpu_util import emulated_exchange
    from tests.test_gpu_fuzz import _check_unstructured
    case, cos, bis_all, recs = _api_setup(dtype)
    emulated_exchange(cos, bis_all)
    _check_unstructured(case, recs)


@pytest.mark.parametrize("dtype", list(API_DTYPES))
def test_padded_levels_last_direct_double_buffered_exchange(dtype):
    """The same through the direct exchange's double-buffered launches (k_copy<..., DBL>):
    exchanges 1 and 2, each from the pre-exchange fields; exchange 1 leaves copy 0 untouched."""
    from tests.gpu_util import EmulatedDirect
    from tests.test_gpu_fuzz import _check_unstructured
    case, cos, bis_all, recs = _api_setup(dtype)
    before = [t.clone() for (_, _, t, _) in recs]
    dx = EmulatedDirect(cos, bis_all)
    msgs = dx.peer_messages()
    assert len(msgs) == 2
    for e in (1, 2):
        for (_, _, t, _), b0 in zip(recs, before):
            t.copy_(b0)
        dx.exchange(e)
        _check_unstructured(case, recs)
        if e == 1:
            for r, i, q, x, d in msgs:
                assert x["size"] >= API_HALO * API_LEVELS * case["fields"][0]["dtype"].itemsize
                assert bool((dx.recv[r][i][:x["size"]] == 0xA5).all())
