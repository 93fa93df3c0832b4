"""The status word of the radix passes (csrc/radix.h k_rx_pass): 32 bits - two flag bits and 30 of count - where a chain's total is below
2^30, 64 bits elsewhere and with CDM_RX_STATUS=u64.  Both give the same arrays, bit for bit, and both equal the plain reference (numpy's
stable argsort; primkit.ref_slot_tuples), at the sizes where the chained scan changes shape: one tile, three tiles and a key, a segment
of exactly a tile and of a tile and a tuple, one long chain in one head segment."""
import numpy as np
import pytest

import primkit
from primkit import EMPTY, RX_TILE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prims():
    from carpedeam_amd import capi
    primkit.build()
    return primkit.Prims(capi.Ctx(0))


def same(got, exp, what):
    assert got.shape == exp.shape, "%s: %s items, expected %s" % (what, got.shape, exp.shape)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, "%s: %d of %d differ, first at %d" % (what, bad.size, got.size, bad[0])


def both_words(monkeypatch, fn):
    """fn() with the word the sizes allow (32 bits in every case of this file) and with the 64-bit word forced"""
    monkeypatch.delenv("CDM_RX_STATUS", raising=False)
    a = fn()
    monkeypatch.setenv("CDM_RX_STATUS", "u64")
    b = fn()
    monkeypatch.delenv("CDM_RX_STATUS")
    return a, b


@pytest.mark.parametrize("bits", (9, 5))
@pytest.mark.parametrize("n", (RX_TILE, 3 * RX_TILE + 1, 1))
@pytest.mark.parametrize("kt,vt", (("u64", "u32"), ("u64", None), ("u32", "u64")))
def test_one_pass_u32_equals_u64_and_the_reference(prims, monkeypatch, bits, n, kt, vt):
    rng = np.random.default_rng(bits * 1000003 + n)
    k = rng.integers(0, 1 << (32 if kt == "u32" else 64), n, dtype=np.uint64).astype(primkit.DTYPES[kt])
    if n > 64:
        k[: n // 2] &= k.dtype.type(((1 << (32 if kt == "u32" else 64)) - 1) ^ 0xFFF)     # half the keys in one digit: its chain carries most of the array
    v = None if vt is None else np.arange(n, dtype=primkit.DTYPES[vt])
    b = 3
    (ka, va, fa), (kb, vb, fb) = both_words(monkeypatch, lambda: prims.sort_pairs(kt, vt, k, v, b, b + bits))
    assert fa == fb
    same(ka, kb, "keys, u32 against u64")
    order = np.argsort((k.astype(np.uint64) >> np.uint64(b)) & np.uint64((1 << bits) - 1), kind="stable")
    same(ka, k[order], "keys")
    if vt is not None:
        same(va, vb, "values, u32 against u64")
        same(va, v[order], "values")


def slot_keys(rng, counts, top_bit):
    """counts[d] real keys with head digit d (random bits below it, random strand), shuffled among 5 % empty slots"""
    shift = top_bit - 9
    parts = [(np.uint64(d) << np.uint64(shift)) | rng.integers(0, 1 << shift, c, dtype=np.uint64) | (rng.integers(0, 2, c, dtype=np.uint64) << np.uint64(63)) for d, c in counts.items()]
    keys = np.concatenate(parts + [np.full(sum(counts.values()) // 20 + 1, EMPTY, np.uint64)])
    return keys[rng.permutation(keys.size)]


SLOT_CASES = {
    "segment_of_a_tile": {7: RX_TILE, 8: 3, 300: 100},
    "segment_of_a_tile_and_one": {7: RX_TILE + 1, 8: 3, 511: 100},
    "two_full_segments_side_by_side": {0: RX_TILE, 1: RX_TILE + 1, 2: RX_TILE - 1},
    "one_digit_holds_nearly_everything": {200: 40 * RX_TILE + 17, 3: 5, 201: 1, 511: 9},
}


@pytest.mark.parametrize("name", list(SLOT_CASES))
@pytest.mark.parametrize("tb,lb", ((40, 13), (40, 14), (28, 1)))
def test_slot_sort_u32_equals_u64_and_the_reference(prims, monkeypatch, name, tb, lb):
    rng = np.random.default_rng(len(name) * 7919 + tb + lb)
    keys = slot_keys(rng, SLOT_CASES[name], tb)
    (la, sa, ta), (lb_, sb, tb_) = both_words(monkeypatch, lambda: prims.sort_slot_keys(keys, tb, lb, None))
    assert la == lb_
    same(sa, sb, "seg, u32 against u64")
    same(ta, tb_, "slot tuples, u32 against u64")
    elive, eseg, etup = primkit.ref_slot_tuples(keys, tb, lb)
    assert la == elive
    same(sa, eseg, "seg")
    same(ta, etup, "slot tuples")


def test_slot_sort_with_a_callers_histogram_and_a_range_of_digits(prims, monkeypatch):
    """the largest segment the host reads back is the largest KEPT one (a rank's range of head digits)"""
    rng = np.random.default_rng(99)
    keys = slot_keys(rng, {5: 2 * RX_TILE + 3, 6: RX_TILE, 400: 77}, 40)
    for keep in ((0, 512), (6, 401), (0, 6)):
        (la, sa, ta), (lb_, sb, tb_) = both_words(monkeypatch, lambda: prims.sort_slot_keys(keys, 40, 13, primkit.head_hist(keys, 40), keep))
        elive, eseg, etup = primkit.ref_slot_tuples(keys, 40, 13, keep)
        assert la == lb_ == elive
        same(sa, eseg, "seg"); same(sb, eseg, "seg (u64)")
        same(ta, etup, "slot tuples"); same(tb_, etup, "slot tuples (u64)")


def test_the_switch_takes_u64_only(prims, monkeypatch):
    """any other value leaves the default choice (the library's switches are read, not validated, on this path)"""
    rng = np.random.default_rng(5)
    k = rng.integers(0, 1 << 64, 2 * RX_TILE + 5, dtype=np.uint64)
    monkeypatch.setenv("CDM_RX_STATUS", "u32")
    ka, _, _ = prims.sort_pairs("u64", None, k, None, 0, 9)
    monkeypatch.delenv("CDM_RX_STATUS")
    same(ka, k[np.argsort(k & np.uint64(0x1FF), kind="stable")], "keys")
