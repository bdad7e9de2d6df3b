"""Device parity at the limits of the short-form field addressing (seg_s::amode): the cases of
tests/addressing_cases.py packed and unpacked through ghx_plan_*, the fused self exchange
(k_self) and the zero-copy put (k_put), each asserting through ghx_plan_segment which arithmetic
the launch takes before it runs.

Reference: a numpy int64 enumeration of the field byte offset of every message element
(addressing_cases.element_offsets), tied to the project's pinned oracle wherever the field fits
a host array. Every field lives in ONE 4.5-GiB device buffer filled with sentinel 0 (message
bytes are 1..255): all correct accesses fit in it, and so does any 32-bit-wrapped offset from a
case whose field_off is 0, so a wrong short-form address lands in sentinel memory and fails the
comparison instead of faulting."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import addressing_cases as A

pytestmark = pytest.mark.gpu

ARENA_BYTES = 4831838208  # 4.5 GiB
K = A.K


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ghex_amd
    ghex_amd.native_library()


@pytest.fixture(scope="module")
def arena():
    import torch
    t = torch.zeros(ARENA_BYTES, dtype=torch.uint8, device="cuda")
    yield t
    del t
    _reference.cache_clear()
    torch.cuda.empty_cache()


def _nonzero_bytes(arena):
    """Non-sentinel bytes of the whole buffer, counted in chunks (no second full-size tensor)."""
    import torch
    total = torch.zeros((), dtype=torch.int64, device=arena.device)
    step = 256 << 20
    for a in range(0, arena.numel(), step):
        total += torch.count_nonzero(arena[a:a + step])
    return int(total)


def _random_bytes(n, seed):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(1, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)


@functools.lru_cache(maxsize=1)
def _reference(name, shift):
    """(device word indices, word bytes, field pointer offset in the arena) of a case whose field
    pointer is the arena's base + shift (+ 1024 where strides are negative): the words of the
    arena that hold the message's elements, in buffer order."""
    import torch
    case = A.CASES[name]
    off = A.case_offsets(case)
    base = shift + (1024 if off.min() < 0 else 0)
    # bounds, before anything runs: every element inside the arena
    assert off.min() + base >= 0 and off.max() + base + case.elem <= ARENA_BYTES
    g = min(case.elem, 8, shift or 8)  # gather through a view no wider than the shift
    idx = torch.from_numpy(A.word_indices(off, case.elem, g, base)).cuda()
    return idx, g, base


def _words(arena, g):
    import torch
    return arena.view({4: torch.int32, 8: torch.int64}[g])


def _execute(h, fptr, bptr):
    import torch
    from ghex_amd import _ghx
    _ghx.call("ghx_plan_execute", h, _ghx.ptr_array([fptr]), 1, _ghx.ptr_array([bptr]), 1,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _pack_and_unpack(arena, name, shift, expect=None):
    """Pack then unpack case `name` with the field at arena + shift. expect: the segment facts
    asserted before each launch (default: the table's)."""
    import torch
    case = A.CASES[name]
    expect = case.expect if expect is None else expect
    idx, g, base = _reference(name, shift)
    words = _words(arena, g)
    n = case.nbytes
    fptr = arena.data_ptr() + base
    pad = 64
    # pack: the data scattered to the reference offsets must arrive in buffer order
    arena.zero_()
    data = _random_bytes(n, 5)
    words[idx] = data.view(words.dtype)
    msg = torch.zeros(n + 2 * pad, dtype=torch.uint8, device="cuda")
    with A.Plan(A.case_entry(case), 0) as p:
        assert [A.seg_facts(s) for s in p.segments()] == [expect]
        _execute(p.h, fptr, msg.data_ptr() + pad)
    assert torch.equal(msg[pad:pad + n], data)
    assert not bool(msg[:pad].any()) and not bool(msg[pad + n:].any())
    assert _nonzero_bytes(arena) == n  # the pack wrote nothing into the field
    # unpack: a fresh message into the sentinel field; nothing else is written
    arena.zero_()
    msg[pad:pad + n] = _random_bytes(n, 6)
    with A.Plan(A.case_entry(case), 1) as p:
        assert [A.seg_facts(s) for s in p.segments()] == [expect]
        _execute(p.h, fptr, msg.data_ptr() + pad)
    assert torch.equal(words[idx].view(torch.uint8), msg[pad:pad + n])
    assert _nonzero_bytes(arena) == n


@pytest.mark.parametrize("name", A.HOST_SIZED)
def test_enumerator_equals_the_oracle(name):
    A.oracle_gathers_the_enumerated_bytes(A.CASES[name])


@pytest.mark.parametrize("tile_records", [1, 0])
@pytest.mark.parametrize("name", list(A.CASES))
def test_pack_unpack_at_the_limits(arena, name, tile_records):
    from ghex_amd import _ghx
    try:
        _ghx.call("ghx_tune", b"tile_records", tile_records)
        _pack_and_unpack(arena, name, 0)
    finally:
        _ghx.call("ghx_tune", b"reset", 0)


@pytest.mark.parametrize("tile_records", [1, 0])
@pytest.mark.parametrize("name,shift", [("A1", 8), ("C1", 8), ("W2", 4)])
def test_pack_unpack_with_a_shifted_field_pointer(arena, name, shift, tile_records):
    """The field pointer's alignment narrows the launch's vectors to the shift: A1 runs the short
    form at 8 B instead of the planned 16, C1 (amode 2, planned 16 B) must fall to the general
    form at 8 B, W2 runs copy_tile<4, amode 1> from a pointer that is only 4-B aligned."""
    from ghex_amd import _ghx
    case = A.CASES[name]
    assert (1 << case.expect[3]) >= shift
    try:
        _ghx.call("ghx_tune", b"tile_records", tile_records)
        _pack_and_unpack(arena, name, shift)
    finally:
        _ghx.call("ghx_tune", b"reset", 0)


# ---------------------------------------------------------------------------------------------
# fused self exchange (k_self) and its two-launch twin through the Python API
# ---------------------------------------------------------------------------------------------
SELF_CASES = {
    # name: (N, halo, element strides of the view incl. the component axis, components, amode)
    "S1": ((4, 3, 3), 1, (1, 8, (K - 16) // 8), 0, 1),
    "S2": ((4, 3, 3), 1, (1, 8, K // 8), 0, 0),
    "S3": ((4, 3, 3), 2, (1, 8, 4096, (K - 16) // 8), 3, 2),
}


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("name", list(SELF_CASES))
def test_self_exchange_at_the_limits(arena, name, fuse):
    """One periodic fp64 domain whose field is a strided view of the shared buffer. S1: every
    segment on the short form (self_forward<W, 1> when fused); S2: the z stride at 2^24, every
    segment general; S3: three outer dims, amode 2 (copy_tile<16, 2> unfused; fused it must take
    the general self_forward, not the one-division form). Expected: the oracle's exchange on a
    compact twin of the same logical contents."""
    import torch
    from ghex_amd import make_context
    from ghex_amd.structured import regular as R
    N, Hw, estr, nc, amode = SELF_CASES[name]
    ext = tuple(n + 2 * Hw for n in N)
    shape = ext + ((nc,) if nc else ())
    dom = orc.RegularDomain(0, (0, 0, 0), tuple(n - 1 for n in N))
    gf, gl = dom.first, dom.last
    # compact twin in memory order (slowest dim first): [c,] z, y, x
    rng = np.random.default_rng(17)
    a_mem = np.full(shape[::-1], -1.0)
    inner = tuple(slice(Hw, Hw + n) for n in N)
    perm = tuple(range(len(shape)))[::-1]
    logical = a_mem.transpose(perm)  # indexed (x, y, z[, c]), a view of a_mem
    logical[inner] = rng.integers(1, 1 << 40, size=N + ((nc,) if nc else ())).astype(np.float64)
    layout = tuple(len(shape) - 1 - d for d in range(len(shape)))
    spec = orc.FieldSpec(a_mem, 8, layout, (Hw,) * 3 + ((0,) if nc else ()), shape,
                         num_components=max(nc, 1), has_components=bool(nc))
    start = logical.copy()
    opat = orc.regular_make_pattern([[dom]], gf, gl, (Hw,) * 6, (1, 1, 1))
    orc.regular_exchange([[(spec, 0, 0, 0)]], {0: opat}, 1)
    assert not np.any(logical == -1.0)  # the whole halo is filled
    # the device field: the same logical contents behind the case's strides
    span = sum((s - 1) * e for s, e in zip(shape, estr)) + 1
    assert span * 8 <= ARENA_BYTES
    arena.zero_()
    view = torch.as_strided(arena.view(torch.float64), shape, estr)
    view.copy_(torch.from_numpy(start))
    ctx = make_context()
    dd = R.DomainDescriptor(0, gf, gl)
    pc = R.make_pattern(ctx, R.HaloGenerator(gf, gl, (Hw,) * 6, (True,) * 3), [dd])
    fd = R.make_field_descriptor(dd, view, (Hw,) * 3, ext)
    assert fd.layout == layout and fd.num_components == max(nc, 1)
    # which arithmetic both directions take: twin plans over the pattern's boxes
    for direction, halos in ((0, pc.send_halos(0)), (1, pc.recv_halos(0))):
        boxes = [(sp[0], sp[1]) for _, _, _, spaces in halos for sp in spaces]
        assert len(boxes) == 26
        with A.Plan(A.entry(fd.desc, boxes), direction) as p:
            segs = p.segments()
        assert len(segs) == 26 and {s.amode for s in segs} == {amode}
        assert {s.n_outer for s in segs} == {3 if nc else 2}
        # H = 1: the interior starts 8 B into a row, 8-B vectors; H = 2: 16-B rows and vectors
        assert {s.wlog2 for s in segs} == {4 if Hw == 2 else 3}
    co = R.make_communication_object(ctx, fuse_self=fuse)
    assert co.all_self(co.plan([pc(fd)]))
    co.exchange([pc(fd)]).wait()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(view.cpu().numpy(), logical)
    view.zero_()
    assert _nonzero_bytes(arena) == 0  # nothing outside the view's cells was written


# ---------------------------------------------------------------------------------------------
# zero-copy put (k_put)
# ---------------------------------------------------------------------------------------------
PUTS = {
    # name: (source case, target case, target field offsets, (source amode, target amode))
    "A1-A1": ("A1", "A1", (2, 1, 1), (1, 1)),  # copy_direct<16, 1>
    "A1-A2": ("A1", "A2", None, (1, 0)),       # mixed: the general form on both sides
    "A2-A1": ("A2", "A1", None, (0, 1)),
    "C1-C1": ("C1", "C1", None, (2, 2)),       # amode 2 never takes the one-division form
    "W2-W2": ("W2", "W2", None, (1, 1)),       # 4-B vectors: below the short form's widths
}
PUT_TARGET = 256 << 20  # the target field's base in the arena; base + 2^32 is still inside


@pytest.mark.parametrize("tile_records", [1, 0])
@pytest.mark.parametrize("name", list(PUTS))
def test_put_at_the_limits(arena, name, tile_records):
    import torch
    from ghex_amd import _ghx
    sn, tn, toffs, want = PUTS[name]
    src, dst = A.CASES[sn], A.CASES[tn]
    n = src.nbytes
    assert dst.nbytes == n and src.elem == dst.elem
    g = min(src.elem, 8)
    so = A.case_offsets(src)
    to = A.case_offsets(dst, toffs) + PUT_TARGET
    assert so.min() >= 0 and so.max() + src.elem <= PUT_TARGET  # disjoint regions
    assert to.min() >= PUT_TARGET and to.max() + dst.elem <= ARENA_BYTES
    si = torch.from_numpy(A.word_indices(so, src.elem, g)).cuda()
    ti = torch.from_numpy(A.word_indices(to, dst.elem, g)).cuda()
    words = _words(arena, g)
    arena.zero_()
    data = _random_bytes(n, 7)
    words[si] = data.view(words.dtype)
    L = _ghx.lib()
    try:
        _ghx.call("ghx_tune", b"tile_records", tile_records)
        es, ed = A.case_entry(src), A.case_entry(dst, toffs)
        assert (A.amodes(es, 0), A.amodes(ed, 1)) == ([want[0]], [want[1]])
        h = ctypes.c_void_p()
        _ghx.call("ghx_put_create", ctypes.byref(es[0]), 1, ctypes.byref(ed[0]), 1,
                  ctypes.byref(h))
    finally:
        _ghx.call("ghx_tune", b"reset", 0)
    try:
        _ghx.call("ghx_put_execute", h, _ghx.ptr_array([arena.data_ptr()]), 1,
                  _ghx.ptr_array([arena.data_ptr() + PUT_TARGET]), 1,
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        L.ghx_put_destroy(h)
    assert torch.equal(words[ti].view(torch.uint8), data)
    assert torch.equal(words[si].view(torch.uint8), data)
    assert _nonzero_bytes(arena) == 2 * n  # the source, the target's cells, nothing else
