"""The device primitives everything else rests on - the onesweep radix sort, compaction and slot-key sort of csrc/radix.h, the scans
of csrc/scan.h, the bucket finish of csrc/bucket.h, the software x87 and the small block / wave helpers of csrc/devutil.h - each
against a plain exact reference (numpy's stable argsort, cumsum, maximum.accumulate, np.longdouble), bit for bit: there is no
tolerance anywhere in this file.  The primitives are reached through the test-only harness tests/csrc/primitives.hip (primkit.py).
All inputs come from np.random.default_rng with a fixed seed; a case's id names its shape."""
import zlib

import numpy as np
import pytest

import primkit
from primkit import CP_TILE, EMPTY, RX_TILE, SC_TILE

pytestmark = pytest.mark.gpu

U64MAX = 0xFFFFFFFFFFFFFFFF


def rng_for(*parts):
    return np.random.default_rng(zlib.crc32(repr(parts).encode()))


def rand_u64(rng, n):
    return rng.integers(0, 1 << 64, n, dtype=np.uint64)


@pytest.fixture(scope="module")
def prims():
    from carpedeam_amd import capi
    primkit.build()
    return primkit.Prims(capi.Ctx(0))


def same(got, exp, what):
    """exact equality of two arrays, with the first difference in the message"""
    assert got.shape == exp.shape, "%s: %s items, expected %s" % (what, got.shape, exp.shape)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %r, expected %r" % (what, bad.size, got.size, bad[0], got[bad[0]], exp[bad[0]])


# ====================================================================================================== radix sort
KEY_BITS = {"u64": 64, "u32": 32}
SORT_TYPES = [("u64", "u64"), ("u64", "u32"), ("u32", "u32"), ("u32", "u64"), ("u64", None)]       # every (K, V) the product instantiates; None = sortKeys
SORT_N = [0, 1, 63, 64, 65, RX_TILE - 1, RX_TILE, RX_TILE + 1, 2 * RX_TILE, 65 * RX_TILE + 1, (1 << 20) + 3]
BITS64 = [(0, 1), (0, 9), (0, 10), (1, 42), (13, 64), (0, 63), (0, 64)]
BITS32 = [(0, 5), (0, 32), (0, 1), (0, 9), (0, 10)]
DISTS = ["uniform", "allequal", "twodigits", "sorted", "reversed", "onedigit", "zerobits"]


def set_field(full, vals, b, e):
    """full with its bits [b, e) replaced by vals"""
    w = e - b
    fm = np.uint64((((1 << w) - 1) << b) & U64MAX)
    return (full & ~fm) | ((np.asarray(vals, np.uint64) << np.uint64(b)) & fm)


def make_keys(rng, dist, n, kt, b, e):
    bits = KEY_BITS[kt]
    full = rand_u64(rng, n) >> np.uint64(64 - bits)
    w = e - b
    field = rng.integers(0, 1 << w, n, dtype=np.uint64) if w < 64 else rand_u64(rng, n)
    if dist == "uniform":
        k = full
    elif dist == "allequal":
        k = set_field(full, np.full(n, int(field[0]) if n else 0, np.uint64), b, e)
    elif dist == "twodigits":
        two = np.array([int(field[0]) if n else 0, int(field[-1]) if n else 0], np.uint64)
        k = set_field(full, two[rng.integers(0, 2, n)], b, e)
    elif dist == "sorted":
        k = set_field(full, np.sort(field), b, e)
    elif dist == "reversed":
        k = set_field(full, np.sort(field)[::-1], b, e)
    elif dist == "onedigit":        # one digit holds all but 64 items: runs of whole tiles of one digit in the LDS exchange
        f = np.full(n, int(field[0]) if n else 0, np.uint64)
        if n:
            at = rng.choice(n, min(64, n), replace=False)
            f[at] = field[at]
        k = set_field(full, f, b, e)
    elif dist == "zerobits":        # the sorted bits are zero, the others random
        k = set_field(full, np.zeros(n, np.uint64), b, e)
    else:
        raise ValueError(dist)
    return k.astype(primkit.DTYPES[kt])


def make_values(rng, vt, n, random_values):
    if vt is None:
        return None
    if not random_values:
        return np.arange(n, dtype=primkit.DTYPES[vt])
    return (rand_u64(rng, n) >> np.uint64(64 - KEY_BITS[vt])).astype(primkit.DTYPES[vt])


def sort_cases():
    cases = []
    for kt, vt in SORT_TYPES:
        top = KEY_BITS[kt]
        for n in SORT_N:                                            # every size, all key bits (u64: 8 passes = MAXPASS)
            cases.append((kt, vt, n, (0, top), "uniform"))
        for be in (BITS64 if kt == "u64" else BITS32):            # every bit range at a tile edge, and over more than one look-back round
            cases.append((kt, vt, RX_TILE + 1, be, "uniform"))
            cases.append((kt, vt, 65 * RX_TILE + 1, be, "uniform"))
        for dist in DISTS[1:]:
            for be in ((13, 64), (0, 10)) if kt == "u64" else ((0, 32), (0, 5)):
                cases.append((kt, vt, RX_TILE + 1, be, dist))
                cases.append((kt, vt, 65 * RX_TILE + 1, be, dist))
    for be in BITS64:                                               # (u64, u64): every bit range with every distribution
        for dist in DISTS[1:]:
            cases.append(("u64", "u64", 3 * RX_TILE + 17, be, dist))
    for dist in DISTS:
        cases.append(("u64", "u32", (1 << 20) + 3, (13, 64), dist))  # as kmermatch.hip sorts its staged runs
    cases.append(("u64", "u32", 1 << 25, (0, 64), "uniform"))
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def sort_id(c):
    kt, vt, n, (b, e), dist = c
    return "%s-%s-n%d-bits%d:%d-%s" % (kt, vt or "keys", n, b, e, dist)


@pytest.mark.parametrize("case", sort_cases(), ids=sort_id)
def test_sortPairs(prims, case):
    """rx::sortPairs / rx::sortKeys = numpy's stable argsort on the key bits [b, e): whole keys (the bits outside the range arrive
    untouched) and values in that order, read from the buffer inFirst names.  Values = input index (stability is visible), then random
    (values travel with their keys)."""
    kt, vt, n, (b, e), dist = case
    rng = rng_for("sort", case)
    k = make_keys(rng, dist, n, kt, b, e)
    order = np.argsort(primkit.masked(k, b, e), kind="stable")
    passes = (e - b + primkit.RX_BITS - 1) // primkit.RX_BITS
    for random_values in ((False, True) if vt else (False,)):
        v = make_values(rng, vt, n, random_values)
        ko, vo, in_first = prims.sort_pairs(kt, vt, k, v, b, e)
        assert in_first == (n == 0 or passes % 2 == 0), "inFirst after %d passes" % passes
        same(ko, k[order], "keys")
        if vt:
            same(vo, v[order], "values (%s)" % ("random" if random_values else "input index"))


@pytest.mark.parametrize("kt,vt", SORT_TYPES, ids=lambda t: str(t or "keys"))
@pytest.mark.parametrize("be", [(5, 5), (9, 3), (64, 64)], ids=lambda be: "bits%d:%d" % be)
def test_sortPairs_empty_bit_range(prims, kt, vt, be):
    """endBit <= beginBit: the input comes back untouched, inFirst true"""
    if be[0] > KEY_BITS[kt]:
        be = (KEY_BITS[kt], KEY_BITS[kt])
    rng = rng_for("sort-empty", kt, vt, be)
    k = make_keys(rng, "uniform", 10000, kt, 0, KEY_BITS[kt])
    v = make_values(rng, vt, 10000, True)
    ko, vo, in_first = prims.sort_pairs(kt, vt, k, v, be[0], be[1])
    assert in_first
    same(ko, k, "keys")
    if vt:
        same(vo, v, "values")


def test_sortPairs_u64_u64_n67108864_by_properties(prims):
    """2^26 pairs, all 64 key bits, values = input index.  Checked without an argsort by the three properties that together equal it:
    the output keys do not decrease; k_in[v_out] == k_out with v_out a permutation; v_out increases inside every run of equal keys.
    Keys are drawn from 2^22 distinct values so that runs of equal keys (stability) are everywhere."""
    n = 1 << 26
    rng = rng_for("sort-big")
    pool = rand_u64(rng, 1 << 22)
    k = pool[rng.integers(0, pool.size, n)]
    v = np.arange(n, dtype=np.uint64)
    ko, vo, in_first = prims.sort_pairs("u64", "u64", k, v, 0, 64)
    assert in_first
    assert np.all(ko[1:] >= ko[:-1]), "output keys decrease"
    assert vo.max() < n and np.all(np.bincount(vo.astype(np.int64), minlength=n) == 1), "the values are no permutation of the input indices"
    same(k[vo.astype(np.int64)], ko, "k_in[v_out] against k_out")
    eq = ko[1:] == ko[:-1]
    assert eq.any()
    assert np.all(vo[1:][eq] > vo[:-1][eq]), "equal keys left their input order"


# ====================================================================================================== compaction
COMPACT_N = [0, 1, CP_TILE - 1, CP_TILE, CP_TILE + 1, 70 * CP_TILE + 5, (1 << 22) + 1]
SHARES = ["none", "all", "1in1000", "half", "allbutone", "emptytile"]


@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("n", COMPACT_N, ids=lambda n: "n%d" % n)
@pytest.mark.parametrize("vt", ["u64", "u32", "u8"])
def test_compactPairs(prims, vt, n, share):
    """rx::compactPairs: the pairs whose key is not ~0, in order; total exact.  Only the first `total` outputs are compared."""
    rng = rng_for("compact", vt, n, share)
    k = rand_u64(rng, n) >> np.uint64(1)            # (never ~0)
    if share == "none":
        k[:] = EMPTY
    elif share == "1in1000":
        k[rng.random(n) >= 0.001] = EMPTY
    elif share == "half":
        k[rng.random(n) < 0.5] = EMPTY
    elif share == "allbutone" and n:
        k[rng.integers(0, n)] = EMPTY
    elif share == "emptytile":                      # a whole empty tile between full ones
        k[(np.arange(n) // CP_TILE) % 3 == 1] = EMPTY
    v = (rand_u64(rng, n) >> np.uint64(64 - 8 * np.dtype(primkit.DTYPES[vt]).itemsize)).astype(primkit.DTYPES[vt])
    ek, ev, etot = primkit.ref_compact(k, v)
    ko, vo, tot = prims.compact_pairs(vt, k, v)
    assert tot == etot, "total %d, expected %d" % (tot, etot)
    same(ko[:tot], ek, "keys")
    same(vo[:tot], ev, "values")


# ====================================================================================================== slot-key sort
def make_slot_keys(rng, n, top_bit, empty_share, digits="any"):
    head = min(primkit.RX_BITS, top_bit)
    shift = top_bit - head
    kmer = rng.integers(0, 1 << top_bit, n, dtype=np.uint64)
    if digits == "one":                             # every key in one head digit
        kmer = set_field(kmer, np.full(n, 137 % (1 << head), np.uint64), shift, top_bit)
    elif digits == "ends":                          # head digits 0 and 511 only
        kmer = set_field(kmer, np.array([0, (1 << head) - 1], np.uint64)[rng.integers(0, 2, n)], shift, top_bit)
    keys = kmer | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    if empty_share >= 1:
        keys[:] = EMPTY
    elif empty_share > 0:
        keys[rng.random(n) < empty_share] = EMPTY
    return keys


def slot_cases():
    geoms = [(40, 13), (40, 22), (40, 31), (9, 0), (12, 0)]        # two, one and no segment passes; head digit only; one pass of 3 bits
    cases = []
    for n in SORT_N + [1 << 24]:
        cases.append((40, 13, n, 0.5, "any", (0, 512), False))
    for tb, lb in geoms:
        for n in (RX_TILE + 1, 65 * RX_TILE + 1):
            for hist in (False, True):
                cases.append((tb, lb, n, 0.0, "any", (0, 512), hist))
        for share in (0.5, 0.999, 1.0):
            cases.append((tb, lb, (1 << 20) + 3, share, "any", (0, 512), False))
        for digits in ("one", "ends"):
            cases.append((tb, lb, 65 * RX_TILE + 1, 0.5, digits, (0, 512), True))
        for keep in ((17, 300), (511, 512), (5, 5)):
            for hist in (False, True):
                cases.append((tb, lb, 65 * RX_TILE + 1, 0.5, "any", keep, hist))
            cases.append((tb, lb, 65 * RX_TILE + 1, 0.5, "ends", keep, False))
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def slot_id(c):
    tb, lb, n, share, digits, keep, hist = c
    return "top%d-low%d-n%d-empty%g-%s-keep%d:%d-%s" % (tb, lb, n, share, digits, keep[0], keep[1], "hist" if hist else "nohist")


def check_slot_sort(prims, case):
    tb, lb, n, share, digits, keep, hist = case
    rng = rng_for("slot", case)
    keys = make_slot_keys(rng, n, tb, share, digits)
    elive, eseg, etup = primkit.ref_slot_tuples(keys, tb, lb, keep)
    live, seg, tup = prims.sort_slot_keys(keys, tb, lb, primkit.head_hist(keys, tb) if hist else None, keep)
    assert live == elive, "live %d, expected %d" % (live, elive)
    same(seg, eseg, "seg")
    same(tup, etup, "slot tuples")


@pytest.mark.parametrize("case", slot_cases(), ids=slot_id)
def test_sortSlotKeys(prims, case):
    """rx::sortSlotKeys (the metric's sort 1) against the model of the header's comment (primkit.ref_slot_tuples): live, all 513 seg
    words and the live tuples."""
    check_slot_sort(prims, case)


def test_sortSlotKeys_checks_a_callers_head_histogram(prims, monkeypatch):
    """CDM_SLOT_HIST=check: the caller's counts are compared with a count of the keys - right counts pass and give the same result"""
    monkeypatch.setenv("CDM_SLOT_HIST", "check")
    check_slot_sort(prims, (40, 13, 65 * RX_TILE + 1, 0.5, "any", (0, 512), True))
    check_slot_sort(prims, (40, 22, 65 * RX_TILE + 1, 0.5, "any", (17, 300), True))


@pytest.mark.parametrize("tb,lb", [(41, 13), (64, 31), (40, 12), (40, 0), (40, 32), (12, 4), (5, 1)], ids=lambda x: str(x))
def test_sortSlotKeys_refuses_geometry_it_cannot_take(prims, tb, lb):
    """more than 31 key bits below the head digit, more than 18 bits for the segment passes, lowBits above the head digit's shift:
    CDM_ERR_INVALID, before any launch"""
    assert primkit.slot_key_geometry(tb, lb) is None
    keys = make_slot_keys(rng_for("slot-refused", tb, lb), 1000, min(tb, 40), 0.5)
    with pytest.raises(primkit.PrimError) as ei:
        prims.sort_slot_keys(keys, tb, lb)
    assert ei.value.rc == primkit.CDM_ERR_INVALID


# ====================================================================================================== scans
SCAN_N = [0, 1, 255, 256, SC_TILE - 1, SC_TILE, SC_TILE + 1, SC_TILE ** 2 - 1, SC_TILE ** 2, SC_TILE ** 2 + 1, 20_000_000]


def scan_values(rng, t, n, kind):
    dt = primkit.DTYPES[t]
    if kind == "zeros":
        a = np.zeros(n, dt)
    elif kind == "ones":
        a = np.ones(n, dt)
    elif kind == "below2^20":       # (u32: the sums pass 2^32 from about 8 000 items on and wrap, on the device as in the reference)
        a = rng.integers(0, 1 << 20, n, dtype=dt)
    elif kind == "near2^63":        # carries through the two 32-bit halves of cdm_shfl_up_t; the u64 sums wrap modulo 2^64
        a = (np.uint64(1 << 63) - rng.integers(0, 1 << 33, n, dtype=np.uint64)).astype(dt)
    else:
        raise ValueError(kind)
    # the product scans n + 1 items for n counts: the last input is read, no output depends on it
    if n:
        a[-1] = np.iinfo(dt).max - 5
    return a


SCAN_CASES = [(t, n, kind) for t in ("u32", "u64") for n in SCAN_N for kind in ("zeros", "ones", "below2^20") + (("near2^63",) if t == "u64" else ())]


@pytest.mark.parametrize("t,n,kind", SCAN_CASES, ids=["%s-n%d-%s" % c for c in SCAN_CASES])
def test_exclusiveScan(prims, t, n, kind):
    """cdmscan::exclusiveScan<u32 / u64> = cumsum in the same unsigned width, shifted by one (u32 sums wrap modulo 2^32, u64 modulo
    2^64: so does the reference)"""
    a = scan_values(rng_for("scan", t, n, kind), t, n, kind)
    same(prims.excl_scan(t, a), primkit.ref_excl_scan(a), "scan")


@pytest.mark.parametrize("n", [SC_TILE + 1, SC_TILE ** 2 + 1], ids=lambda n: "n%d" % n)
@pytest.mark.parametrize("t", ["u32", "u64"])
def test_exclusiveScan_in_place(prims, t, n):
    a = scan_values(rng_for("scan-inplace", t, n), t, n, "below2^20")
    same(prims.excl_scan(t, a, in_place=True), primkit.ref_excl_scan(a), "scan in place")


def maxscan_values(rng, n, kind):
    if kind == "increasing":
        a = np.cumsum(rng.integers(0, 1 << 30, n, dtype=np.uint64))
    elif kind == "decreasing":
        a = np.uint64(1 << 63) + np.cumsum(rng.integers(0, 1 << 30, n, dtype=np.uint64))[::-1]
    elif kind == "constant":
        a = np.full(n, (1 << 63) + 12345, np.uint64)
    elif kind == "tilespike":       # one spike at the last item of a tile (every 5th tile), above 2^32 so that both halves travel
        a = rng.integers(0, 1 << 20, n, dtype=np.uint64)
        at = np.arange(SC_TILE - 1, n, 5 * SC_TILE)
        a[at] = np.uint64(1 << 40) + at.astype(np.uint64)
    elif kind == "random":
        a = rand_u64(rng, n) >> rng.integers(0, 64, n, dtype=np.uint64)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a, np.uint64)


@pytest.mark.parametrize("kind", ["increasing", "decreasing", "constant", "tilespike", "random"])
@pytest.mark.parametrize("n", SCAN_N, ids=lambda n: "n%d" % n)
def test_inclusiveMaxScan(prims, n, kind):
    """cdmscan::inclusiveMaxScanFn = np.maximum.accumulate"""
    a = maxscan_values(rng_for("maxscan", n, kind), n, kind)
    same(prims.incl_max_scan(a), primkit.ref_incl_max_scan(a), "max-scan")


def test_inclusiveMaxScan_in_place(prims):
    a = maxscan_values(rng_for("maxscan-inplace"), SC_TILE ** 2 + 1, "random")
    same(prims.incl_max_scan(a, in_place=True), primkit.ref_incl_max_scan(a), "max-scan in place")


# ====================================================================================================== bucket finish
def bucket_input(rng, sizes, shift_hi, ign, top, equal_from=5000):
    """keys stably sorted on [shiftHi, top) (made here: ascending bucket ids, one per entry of sizes); the compared low bits come from
    a small range, so that equal compared bits with different ignored bits (stability) are common; a bucket of equal_from or more
    elements holds one compared value only"""
    sizes = np.asarray(sizes, np.int64)
    ids = np.cumsum(rng.integers(1, 4, sizes.size)).astype(np.uint64)
    assert int(ids[-1]) < (1 << (top - shift_hi))
    hi = np.repeat(ids, sizes)
    n = int(sizes.sum())
    spread = rng.choice([3, 1 << 10, 1 << (shift_hi - ign)], sizes.size)
    low = (rng.random(n) * np.repeat(spread, sizes)).astype(np.uint64)
    low[np.repeat(sizes >= equal_from, sizes)] = 7
    k = (hi << np.uint64(shift_hi)) | (low << np.uint64(ign))
    if ign:
        k |= rng.integers(0, 1 << ign, n, dtype=np.uint64)
    return k


def small_buckets(rng, total):
    out = []
    while sum(out) < total:
        out.append(int(rng.integers(1, 40)))
    return out


def bucket_layouts():
    """name -> function(rng) giving the bucket sizes"""
    lay = {}
    for s in (1, 2, 255, 256, 257, 511, 512, 513):                 # around BK_GROUP and BK_MAXB (513: the big-bucket list)
        lay["size%d" % s] = lambda rng, s=s: sum(([s] + small_buckets(rng, int(rng.integers(1, 700))) for _ in range(12)), [])
    for s in (2, 300, 512, 600):                                    # a bucket that starts in the last slot of a wave's 256-slot range
        lay["lastslot-size%d" % s] = lambda rng, s=s: [100, 155, s] + small_buckets(rng, 1000) + [s, 77]
    for s in (767, 768, 769):                                       # spans a wave's whole window of WV_WIN slots, one less, one more
        lay["span%d" % s] = lambda rng, s=s: [3, s, 5] + small_buckets(rng, 300) + [s] + small_buckets(rng, 2000) + [s, 9]
    lay["equal5000"] = lambda rng: small_buckets(rng, 500) + [5000] + small_buckets(rng, 900) + [5000, 1]
    lay["single-bucket"] = lambda rng: [1237]
    lay["mixed"] = lambda rng: [int(x) for x in np.minimum(rng.geometric(0.02, 6000), 3000)] + [11]
    return lay


LAYOUTS = bucket_layouts()


@pytest.mark.parametrize("cap", [None, "5", "3,17"], ids=lambda c: "cap-" + (c or "default").replace(",", "_"))
@pytest.mark.parametrize("geom", [(30, 1, 61), (20, 0, 45)], ids=lambda g: "hi%d-ign%d-top%d" % g)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_bucketSortKeys(prims, monkeypatch, layout, geom, cap):
    """bucket::bucketSortKeys: input stably sorted on [shiftHi, top) -> stable sort on [ign, top).  (shiftHi, ign, top) = (30, 1, 61) is
    what sort 2 of kmermatcher passes for 26 id bits and 8 diagonal bits; CDM_BUCKET_CAP lowers the capacities so that the big-bucket
    list and the group limits are met on every layout."""
    shift_hi, ign, top = geom
    rng = rng_for("bucket", layout, geom)
    sizes = LAYOUTS[layout](rng)
    if sum(sizes) % 1024 == 0:
        sizes.append(1)
    k = bucket_input(rng, sizes, shift_hi, ign, top)
    assert k.size % 1024 != 0
    assert np.all(np.diff((k >> np.uint64(shift_hi)).astype(np.int64)) >= 0)
    if cap:
        monkeypatch.setenv("CDM_BUCKET_CAP", cap)
    else:
        monkeypatch.delenv("CDM_BUCKET_CAP", raising=False)
    same(prims.bucket_sort_keys(k, shift_hi, ign, top), primkit.ref_bucket_finish(k, ign, top), "keys")


# ====================================================================================================== x87
def p2(k):
    return float(np.ldexp(1.0, k))


A = 1.0 + p2(-52)       # a double with its last bit set
ONES = 2.0 - p2(-52)    # 53 ones


def directed_rows():
    """name -> terms, each named after the branch of x87_add / x87_acc / x87_round it reaches; every row also runs negated"""
    rows = {}
    for d in (0, 1, 63, 64, 65):
        rows["same-sign-gap%d" % d] = [A, A * p2(-d)]
        rows["same-sign-gap%d-odd-last-bit" % d] = [1.0, p2(-63), A * p2(-d)]
    for d in (0, 1, 2, 63, 64, 65, 66, 67):
        rows["opposite-gap%d" % d] = [A, -1.25 * p2(-d)]
        rows["opposite-gap%d-from-power-of-two" % d] = [1.0, -A * p2(-d)] if d else [1.75, -1.25]
        rows["opposite-gap%d-odd-last-bit" % d] = [1.0, p2(-63), -A * p2(-d)] if d else [1.0, p2(-63), -1.0 - p2(-40)]
    rows["pow2-minus-tiny-renormalise-by-1"] = [1.0, -0.25]
    rows["pow2-minus-tiny-renormalise-by-52"] = [1.0, -(1.0 - p2(-53))]
    rows["renormalise-by-63"] = [1.0, p2(-63), -1.0]
    rows["renormalise-by-more-than-64"] = [-1.0, p2(-64), 1.0]
    rows["renormalise-across-the-low-word"] = [1.0, -p2(-64), -(1.0 - p2(-30))]
    rows["exact-cancellation"] = [1.2345, -1.2345]
    rows["exact-cancellation-negative-first"] = [-1.2345, 1.2345]
    rows["cancel-then-add"] = [3.75, -3.75, p2(-70)]
    rows["cancel-after-rounding"] = [1.0, p2(-70), -1.0]
    rows["tie-odd-last-bit-rounds-up"] = [1.0, p2(-63), p2(-64)]
    rows["tie-even-last-bit-stays"] = [1.0, p2(-62), p2(-64)]
    rows["above-tie-rounds-up"] = [1.0, p2(-62), p2(-64) + p2(-100)]
    rows["below-tie-stays"] = [1.0, p2(-63), p2(-64) - p2(-110)]
    rows["all-ones-rounds-into-next-exponent-gap64"] = [-1.0, p2(-64), -p2(-65)]
    rows["all-ones-rounds-into-next-exponent-gap63"] = [-1.0, p2(-63), -1.5 * p2(-64)]
    rows["all-ones-plus-one-ulp-carries"] = [-1.0, p2(-64), -p2(-64)]
    for g in (0, 1):
        rows["carry-guard%d-sticky0" % g] = [1.5] + [p2(-63)] * g + [1.5]
        rows["carry-guard%d-sticky1" % g] = [ONES] + [p2(-63)] * g + [A * p2(-12)]
        rows["carry-guard%d-sticky-only-bit0" % g] = [ONES] + [p2(-63)] * g + [p2(-11) + p2(-63)] + [p2(-64)]
    rows["zero-terms"] = [0.0, -0.0, 1.5, -0.0, 0.0]
    rows["minus-zero-alone"] = [-0.0]
    rows["minus-zero-plus-zero"] = [-0.0, 0.0]
    rows["only-zeros"] = [0.0, 0.0]
    rows["subnormal-term-lost"] = [1.0, 5e-324]
    rows["subnormal-term-first"] = [5e-324, p2(-1040), p2(-1020)]
    rows["subnormal-term-exact"] = [p2(-1000), p2(-1060), -p2(-1063)]
    rows["running-log-sum"] = [-0.105360515657826, -2.30258509299405, -6.90775527898214, -0.0100503358535014] * 12
    out = {}
    for name, r in rows.items():
        out[name] = r
        out[name + "-negated"] = [-x for x in r]
    return out


DIRECTED = directed_rows()


def directed_matrix():
    cols = max(len(r) for r in DIRECTED.values())
    t = np.zeros((len(DIRECTED), cols), np.float64)        # (+0 terms to the right: x + 0 = x)
    for i, name in enumerate(sorted(DIRECTED)):
        t[i, :len(DIRECTED[name])] = DIRECTED[name]
    return t


def check_fold(prims, t, what, names=None):
    """both folds against the long double fold: (m, e, s) and the conversion to double, bit for bit"""
    primkit.require_x87()
    ref = primkit.x87_fold_ref(t)
    em, ee, es = primkit.x87_decode(ref)
    assert np.all(np.isfinite(ref))
    ed = ref.astype(np.float64)
    normal = (ed == 0) | (np.abs(ed) >= np.finfo(np.float64).tiny)
    assert normal.all(), "%s: a sum leaves the normal range of a double, which is all x87_to_double promises" % what
    results = {}
    for acc in (0, 1):
        fn = "x87_acc" if acc else "x87_add"
        m, e, s, d = prims.x87_fold(t, acc)
        results[acc] = (m, e, s, d)
        bad = np.flatnonzero((m != em) | (e != ee) | (s != es) | (d.view(np.uint64) != ed.view(np.uint64)))
        if bad.size:
            i = bad[0]
            raise AssertionError("%s, %s: %d of %d rows differ, first row %d%s: terms %r -> (m %#x, e %d, s %d, double %r), long double gives (m %#x, e %d, s %d, double %r)" % (
                what, fn, bad.size, t.shape[0], i, " (%s)" % names[i] if names else "", t[i].tolist(), m[i], e[i], s[i], d[i], em[i], ee[i], es[i], ed[i]))
    for a, b in zip(results[0], results[1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%s: x87_acc differs from x87_add" % what
    return ref, (em, ee, es)


def test_x87_reference_is_the_x87_format():
    """np.longdouble is the 80-bit format (64-bit significand, ties to even), and the decode reads it: two sums known by hand"""
    primkit.require_x87()
    ref = primkit.x87_fold_ref(np.array([[1.0, p2(-63), p2(-64)], [1.0, p2(-62), p2(-64)], [-1.0, p2(-64), -p2(-65)]]))
    m, e, s = primkit.x87_decode(ref)
    assert [int(x) for x in m] == [0x8000000000000002, 0x8000000000000002, 0x8000000000000000]
    assert e.tolist() == [0, 0, 0] and s.tolist() == [0, 0, 1]


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_x87_directed(prims, name):
    """one row per branch of x87_add / x87_acc / x87_round (the opposite-sign half has a single caller in the product)"""
    names = sorted(DIRECTED)
    i = names.index(name)
    t = directed_matrix()[i:i + 1]
    check_fold(prims, t, name, [name])


X87_ROWS, X87_COLS = 200_000, 64


def random_terms(rng, kind):
    shape = (X87_ROWS, X87_COLS)
    if kind == "negative":          # the callers' case: every term of one sign
        return -(1.0 + rng.random(shape)) * np.ldexp(1.0, rng.integers(-200, 201, shape))
    if kind == "mixed":
        return np.where(rng.random(shape) < 0.5, -1.0, 1.0) * (1.0 + rng.random(shape)) * np.ldexp(1.0, rng.integers(-200, 201, shape))
    if kind == "mixed-close-exponents":     # every exponent gap of a row within +-70: alignment, borrow and renormalisation at every distance
        base = rng.integers(-120, 121, (X87_ROWS, 1))
        return np.where(rng.random(shape) < 0.5, -1.0, 1.0) * (1.0 + rng.random(shape)) * np.ldexp(1.0, base + rng.integers(-70, 71, shape))
    if kind == "few-ulps-apart":    # terms a few ulps apart, signs at random: cancellation is common
        base = (1.0 + rng.random((X87_ROWS, 1))) * np.ldexp(1.0, rng.integers(-200, 201, (X87_ROWS, 1)))
        t = base * (1.0 + rng.integers(0, 8, shape) * p2(-52))
        return np.where(rng.random(shape) < 0.5, -t, t)
    if kind == "negative-logs":     # sums of log-likelihoods: x87_acc's fast path (same sign, gap 1 .. 63) on nearly every term
        return np.log(rng.random(shape) * 0.999 + 1e-4)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["negative", "mixed", "mixed-close-exponents", "few-ulps-apart", "negative-logs"])
def test_x87_random_rows(prims, kind):
    """200 000 rows x 64 terms, magnitudes 2^U(-200, 200) (no sum leaves the normal range of a double); x87_lt on neighbouring sums,
    on equal ones and against zero"""
    rng = rng_for("x87", kind)
    t = random_terms(rng, kind)
    t[:, 40:][rng.random(X87_ROWS) < 0.1] = 0.0         # (shorter rows as well)
    ref, (m, e, s) = check_fold(prims, t, kind)
    a = (m, e, s)
    for what, j in (("neighbour", np.roll(np.arange(X87_ROWS), 1)), ("itself", np.arange(X87_ROWS))):
        got = prims.x87_lt(a, (m[j], e[j], s[j]))
        same(got, ref < ref[j], "x87_lt with %s" % what)
    z = (np.zeros(X87_ROWS, np.uint64), np.zeros(X87_ROWS, np.int32), np.zeros(X87_ROWS, np.uint32))
    same(prims.x87_lt(a, z), ref < 0, "x87_lt(sum, 0)")
    same(prims.x87_lt(z, a), 0 < ref, "x87_lt(0, sum)")


def test_x87_lt_directed(prims):
    """x87_lt on every pair of the directed sums (both signs, equal magnitudes, zeros)"""
    primkit.require_x87()
    ref = primkit.x87_fold_ref(directed_matrix())
    m, e, s = primkit.x87_decode(ref)
    i, j = [x.reshape(-1) for x in np.meshgrid(np.arange(ref.size), np.arange(ref.size), indexing="ij")]
    same(prims.x87_lt((m[i], e[i], s[i]), (m[j], e[j], s[j])), ref[i] < ref[j], "x87_lt")


# ====================================================================================================== small device helpers
BLOCK_SIZES = [64, 128, 192, 256, 512, 1024]


@pytest.mark.parametrize("threads", BLOCK_SIZES, ids=lambda t: "block%d" % t)
@pytest.mark.parametrize("t", ["u32", "u64"])
def test_block_excl_sum(prims, t, threads):
    """cdm_block_excl_sum = cumsum inside the block, shifted by one; the total is the block's sum in every thread"""
    rng = rng_for("blocksum", t, threads)
    blocks = 37
    a = (rand_u64(rng, blocks * threads) >> np.uint64(1 if t == "u64" else 40)).astype(primkit.DTYPES[t])
    a[:threads] = 0
    a[threads:2 * threads] = 1
    out, tot = prims.block_excl_sum(t, a, threads)
    rows = a.reshape(blocks, threads)
    incl = np.cumsum(rows, axis=1, dtype=rows.dtype)
    same(out.reshape(blocks, threads), incl - rows, "exclusive sums")
    same(tot.reshape(blocks, threads), np.repeat(incl[:, -1:], threads, axis=1), "totals")


@pytest.mark.parametrize("pred", ["none", "all", "random", "onelane"])
@pytest.mark.parametrize("threads", BLOCK_SIZES, ids=lambda t: "block%d" % t)
@pytest.mark.parametrize("block", [False, True], ids=["wave", "block"])
def test_append(prims, block, threads, pred):
    """cdm_wave_append / cdm_block_append: the slots handed out are exactly 0 .. count-1, once each, and the counter ends at count;
    inside one wave (one block) they are consecutive and in lane (thread) order"""
    rng = rng_for("append", block, threads, pred)
    blocks = 53
    n = blocks * threads
    p = {"none": np.zeros(n, np.uint8), "all": np.ones(n, np.uint8), "random": (rng.random(n) < 0.3).astype(np.uint8)}.get(pred)
    if p is None:
        p = np.zeros(n, np.uint8)
        p[np.arange(0, n, 64) + rng.integers(0, 64, n // 64)] = 1
    slot, counter = prims.append(block, p, threads)
    count = int(p.sum())
    assert counter == count
    assert np.all(slot[p == 0] == 0xFFFFFFFF)
    same(np.sort(slot[p == 1]), np.arange(count, dtype=np.uint32), "slots handed out")
    unit = threads if block else 64
    for g, pg in zip(slot.reshape(-1, unit), p.reshape(-1, unit)):
        got = g[pg == 1]
        if got.size:
            same(got, got[0] + np.arange(got.size, dtype=np.uint32), "slots of one %s" % ("block" if block else "wave"))


def test_bit_helpers(prims):
    """cdm_revcomp16, cdm_spread16, cdm_squash16 against per-base / per-bit models"""
    rng = rng_for("bitops")
    x = np.concatenate([np.array([0, 1, 2, 3, 0xFFFFFFFF, 0x80000000, 0x55555555, 0xAAAAAAAA, 0x0000FFFF, 0xFFFF0000], np.uint32),
                        np.uint32(1) << np.arange(32, dtype=np.uint32), rng.integers(0, 1 << 32, 5000, dtype=np.uint32)])
    for op, model in (("revcomp16", primkit.revcomp16_model), ("spread16", primkit.spread16_model), ("squash16", primkit.squash16_model)):
        same(prims.bitop16(op, x), np.array([model(int(v)) for v in x], np.uint32), "cdm_" + op)
    same(prims.bitop16("squash16", prims.bitop16("spread16", x)), x & np.uint32(0xFFFF), "squash16(spread16(x))")


@pytest.mark.parametrize("L", [1, 15, 16, 17, 31, 32, 33, 100], ids=lambda L: "L%d" % L)
def test_windows16(prims, L):
    """cdm_window16 and cdm_oriented_window16 at every start position, both strands (the s < 0 branch of the reverse window for
    L < 16 + i), against a per-base model; the bases past the end of the sequence are not compared (garbage by contract), and the
    unused part of the last word holds ones or zeros"""
    rng = rng_for("windows", L)
    for pad in (0xFFFFFFFF, 0):
        seq = rng.integers(0, 4, L)
        codes = primkit.pack_bases(seq, pad)
        for mode, rc in (("plain", False), ("forward", False), ("reverse", True)):
            got = prims.windows16(codes, L, mode)
            model = [primkit.window_model(seq, rc, i) for i in range(L)]
            val = np.array([m[0] for m in model], np.uint32)
            mask = np.array([m[1] for m in model], np.uint32)
            same(got & mask, val, "%s windows" % mode)
