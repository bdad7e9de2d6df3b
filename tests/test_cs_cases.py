"""CPU tests of the cubed-sphere test helpers themselves (tests/cs_cases.py): the inputs the GPU
tests rely on must be able to show the faults they look for."""
import numpy as np
import pytest

from tests import cs_cases
from tests.cs_cases import ArenaField, DomainField, dense_strides

X_FAST, Y_FAST = (3, 2, 1, 0), (2, 3, 1, 0)

# (edge, domains, element types) as the GPU tests of the transformed unpack use them
USED = [(10, (0, 3, 4, 7), [("uint8", 1), ("uint8", 3), ("int16", 1), ("float16", 1),
                            ("bfloat16", 1), ("complex64", 1), ("complex128", 1), ("raw12", 1),
                            ("int64", 3), ("int64", 1), ("float32", 3)]),
        (10, range(24), [("uint8", 3), ("int16", 1), ("complex128", 1)]),
        (6, (0, 1), [("int16", 1), ("float32", 1), ("float64", 1), ("complex128", 1)])]


def test_four_and_eight_byte_cells_are_the_cell_number():
    """The values the first cubed-sphere tests were written against: n as a value of the type,
    -0.0 / inf / a NaN at n % 97 == 5 / 11 / 17."""
    x, y, z, k = np.meshgrid(np.arange(10), np.arange(10), np.arange(3), np.arange(3), indexing="ij")
    n = (((2 * 10 + x) * 10 + y) * 3 + z) * 3 + k + 1
    for dtype, u, nan in (("float32", np.uint32, 0x7FC01234), ("float64", np.uint64, 0x7FF8000000001234),
                          ("int32", np.uint32, None), ("int64", np.uint64, None)):
        want = n.astype(dtype)
        if nan is not None:
            want[n % 97 == 5] = -0.0
            want[n % 97 == 11] = np.inf
        want = want.view(u).copy()
        if nan is not None:
            want[n % 97 == 17] = nan
        got = cs_cases.cell_bits(dtype, 2, x, y, z, k, 10, 3, 3)
        assert got.dtype == u and np.array_equal(got, want)


def test_integer_special_cells():
    n = np.arange(1, 400)
    z = np.zeros_like(n)
    # one tile row: tile 0, x = 0, y = 0, z = 0, k = n - 1 of nc = 400 gives the cell number n
    b64 = cs_cases.cell_bits("int64", z, z, z, z, n - 1, 10, 1, 400, special=True)
    b32 = cs_cases.cell_bits("int32", z, z, z, z, n - 1, 10, 1, 400, special=True)
    for r, what in cs_cases.INT_SPECIAL.items():
        at = n % 97 == r
        assert at.sum() >= 3
        if what == "zero":
            assert not b64[at].any() and not b32[at].any()
        elif what == "min":
            assert (b64[at] == 1 << 63).all() and (b32[at] == 1 << 31).all()
        elif what == "minus_one":
            assert (b64[at] == 2 ** 64 - 1).all() and (b32[at] == 2 ** 32 - 1).all()
        elif what == "low_word_zero":
            assert (b64[at] & np.uint64(0xFFFFFFFF) == 0).all() and (b64[at] >> np.uint64(32) == n[at]).all()
        else:
            assert (b64[at] & np.uint64(0xFFFFFFFF) == 0xFFFFFFFF).all()
    # negation: the model is the two's complement of the whole word
    neg = cs_cases.negate_bits(b64, "int64")
    assert np.array_equal(neg.view(np.int64), (-b64.view(np.int64)))
    lo = np.uint64(0xFFFFFFFF)
    halves = ((-(b64 >> np.uint64(32)).astype(np.int64)).astype(np.uint64) & lo) << np.uint64(32) | \
             ((-(b64 & lo).astype(np.int64)).astype(np.uint64) & lo)
    assert (halves != neg).sum() > n.size // 2  # a negation by halves is wrong nearly everywhere


def test_mixed_cells_by_size():
    n = np.arange(1, 5000)
    z = np.zeros_like(n)
    for dtype, size in (("uint8", 1), ("int16", 2), ("bfloat16", 2), ("raw12", 12), ("complex128", 16)):
        b = cs_cases.as_bytes(cs_cases.cell_bits(dtype, z, z, z, z, n - 1, 10, 1, 5000), dtype)
        assert b.shape == (n.size, size) and b.dtype == np.uint8
        if size >= 12:
            assert np.unique(b, axis=0).shape[0] == n.size  # distinct per cell
        assert all(np.unique(b[:, j]).size > 200 for j in range(size))  # every byte lane varies


@pytest.mark.parametrize("edge,domains,types", USED, ids=["c10", "c10_all", "c6"])
def test_every_box_shows_a_reversal_and_a_transposition(edge, domains, types):
    """One- and two-byte values repeat, so distinct cells do not follow from the generator: for
    every box used, the expected content differs from itself reversed along x, y, z (and the
    component axis) and, where the box is square, transposed in (x, y)."""
    cfg = cs_cases.config(edge)
    for dtype, nc in types:
        for di in domains:
            df = DomainField(cfg, di, dtype, nc, False)
            for b in df.dom["boxes"]:
                _, _, bits = df.box_values(b)
                for ax in range(4):
                    if bits.shape[ax] > 1:
                        assert not np.array_equal(bits, np.flip(bits, ax)), (dtype, di, b["l"], ax)
                if bits.shape[0] == bits.shape[1] and bits.shape[0] > 1:
                    assert not np.array_equal(bits, np.swapaxes(bits, 0, 1)), (dtype, di, b["l"])


def test_arena_places_every_element_and_nothing_else():
    cfg = cs_cases.config(6)
    df = DomainField(cfg, 0, "float32", 1, False)
    bits = df.initial()
    for layout, pad, shift in ((X_FAST, None, 0), (X_FAST, {1: 2}, 0), (Y_FAST, {0: 2}, 1), (X_FAST, None, 3)):
        strides = dense_strides(df.shape, layout, 4, pad)
        af = ArenaField(df, strides, shift)
        assert af.layout() == layout
        a = af.arena(bits)
        assert a.size == af.size and (a[:af.base] == cs_cases.SENTINEL_BYTE).all()
        assert (a[-ArenaField.GUARD:] == cs_cases.SENTINEL_BYTE).all()
        for cell in ((0, 0, 0, 0), (3, 4, 1, 0), tuple(n - 1 for n in df.shape)):
            at = af.base + sum(c * s for c, s in zip(cell, strides))
            assert a[at:at + 4].tobytes() == bits[cell].astype("<u4").tobytes()
        touched = np.zeros(a.size, bool)
        touched[af.index] = True
        assert touched.sum() == bits.size * 4
        assert (a[~touched] == cs_cases.SENTINEL_BYTE).all()
        if pad:  # pitch padding lies between the elements
            assert af.size > ArenaField(df, dense_strides(df.shape, layout, 4), shift).size
