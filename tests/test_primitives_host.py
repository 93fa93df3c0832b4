"""Host-side checks of the primitives test kit (no GPU): the harness cross-compiles and exports what primkit binds; every type
combination of the radix sort, the compaction and the scans that the product instantiates has a harness entry point; the numpy
models agree with brute force on tiny inputs; the product library still exports the helpers the harness links against."""
import os
import re
import subprocess

import numpy as np

import primkit
from carpedeam_amd import build as pbuild

CSRC = pbuild.CSRC


def dynamic_symbols(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_harness_builds_and_exports_every_bound_entry_point():
    pbuild.build()
    lib = primkit.build()
    assert os.path.exists(lib)
    syms = dynamic_symbols(lib)
    missing = [n for n in primkit.SIGNATURES if n not in syms]
    assert not missing, missing
    extra = sorted(s for s in syms if s.startswith("prim_") and s not in primkit.SIGNATURES)
    assert not extra, "entry points without a binding in primkit.SIGNATURES: %s" % extra
    l = primkit.lib()          # loads on a machine without a GPU: nothing runs at load time
    assert all(hasattr(l, n) for n in primkit.SIGNATURES)


def test_product_library_still_exports_what_the_harness_links_against():
    """hiding these later is a decision, not an accident"""
    pbuild.build()
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", pbuild.LIB], check=True, capture_output=True, text=True).stdout
    for name in primkit.NEEDS:
        assert re.search(r"\b%s\b" % name, out), "libcarpedeam_hip.so no longer exports %s" % name


def test_header_constants_primkit_relies_on():
    radix = open(os.path.join(CSRC, "radix.h")).read()
    scan = open(os.path.join(CSRC, "scan.h")).read()
    assert re.search(r"#define CDM_RX_NT 512\b", radix) and re.search(r"#define CDM_RX_IPT 16\b", radix)
    assert primkit.RX_TILE == 512 * 16 and primkit.CP_TILE == 256 * 16
    assert re.search(r"BITS = %d, BINS = 1 << BITS, MAXPASS = %d;" % (primkit.RX_BITS, primkit.RX_MAXPASS), radix)
    assert "CP_NT = 256" in radix and "CP_TILE = CP_NT * IPT" in radix
    assert "SLOT_REM = %d, SLOT_IDX_SHIFT = 0, SLOT_STRAND_SHIFT = %d, SLOT_KEY_SHIFT = %d;" % (primkit.SLOT_REM, primkit.SLOT_STRAND_SHIFT, primkit.SLOT_KEY_SHIFT) in radix
    assert "SC_NT = 256, SC_ITEMS = 16, SC_TILE = SC_NT * SC_ITEMS;" in scan and primkit.SC_TILE == 256 * 16
    pub = open(os.path.join(os.path.dirname(pbuild.HERE), "include", "carpedeam_hip.h")).read()
    assert re.search(r"CDM_ERR_INVALID = %d," % primkit.CDM_ERR_INVALID, pub)


TYPE_NAMES = {"uint64_t": "u64", "u64": "u64", "unsigned long long": "u64", "uint32_t": "u32", "u32": "u32", "unsigned int": "u32", "uint8_t": "u8", "u8": "u8",
              "mx_t": "u64"}
LAYOUT_V = {"LayoutWideT": "u64", "LayoutHuge": "u64", "LayoutPacked": "u32", "LayoutSlot": "u32"}


def product_instantiations():
    """(primitive, types...) of every rx::sortPairs / sortKeys / compactPairs and cdmscan:: call with explicit template arguments in
    carpedeam_amd/csrc; a layout's `typedef ... V` stands for each of its types"""
    km = open(os.path.join(CSRC, "kmer_tuple.h")).read()
    vs = set()
    for name, v in re.findall(r"struct (Layout\w+) \{\s*typedef (\w+) V;", km):
        assert LAYOUT_V.get(name) == TYPE_NAMES[v], "layout %s has V = %s: tell LAYOUT_V, and cover the type" % (name, v)
        vs.add(TYPE_NAMES[v])
    assert len(vs) == 2
    found = set()
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith((".hip", ".h")):
            continue
        text = open(os.path.join(CSRC, fn)).read()
        for prim, args in re.findall(r"\b(?:rx|cdmscan)::(sortPairs|sortKeys|compactPairs|exclusiveScan|exclusiveScanFn)<([^<>()]*(?:<[^<>]*>)?[^<>()]*)>\s*\(", text):
            types = [a.strip() for a in args.split(",")]
            if prim.startswith("exclusiveScan"):
                types = types[:1]       # (the second argument of exclusiveScanFn is the load functor)
                prim = "exclusiveScan"
            expanded = [[]]
            for t in types:
                choices = sorted(vs) if t == "V" else [TYPE_NAMES[t]]
                expanded = [e + [c] for e in expanded for c in choices]
            for e in expanded:
                found.add((prim,) + tuple(e))
        if re.search(r"\bcdmscan::inclusiveMaxScanFn\s*\(", text):
            found.add(("inclusiveMaxScanFn",))
    return found


def test_every_product_instantiation_has_an_entry_point():
    """a new (K, V) of the sort, of the compaction or a new scan type in the product fails here until the harness covers it"""
    found = product_instantiations()
    assert {("sortPairs", "u64", "u64"), ("sortPairs", "u64", "u32"), ("sortPairs", "u32", "u32"), ("sortPairs", "u32", "u64"), ("sortKeys", "u64"),
            ("compactPairs", "u64", "u64"), ("compactPairs", "u64", "u32"), ("compactPairs", "u64", "u8"), ("exclusiveScan", "u32"), ("exclusiveScan", "u64"),
            ("inclusiveMaxScanFn",)} <= found, "the search lost instantiations it used to find: %s" % sorted(found)
    entry = {"sortPairs": "prim_sort_pairs_%s_%s", "sortKeys": "prim_sort_keys_%s", "compactPairs": "prim_compact_pairs_%s_%s", "exclusiveScan": "prim_excl_scan_%s",
             "inclusiveMaxScanFn": "prim_incl_max_scan"}
    for inst in sorted(found):
        name = entry[inst[0]] % inst[1:]
        assert name in primkit.SIGNATURES, "%s<%s> is instantiated in carpedeam_amd/csrc and has no harness entry point %s" % (inst[0], ", ".join(inst[1:]), name)


# ---------------------------------------------------------------------------------------------- the models against brute force
def test_slot_tuple_model_against_a_loop():
    rng = np.random.default_rng(5)
    for top_bit, low_bits, keep in ((40, 13, (0, 512)), (40, 31, (17, 300)), (12, 0, (0, 512)), (9, 0, (3, 200)), (40, 22, (5, 5))):
        head, shift, _ = primkit.slot_key_geometry(top_bit, low_bits)
        keys = rng.integers(0, 1 << top_bit, 200, dtype=np.uint64)
        keys[:100] &= np.uint64(((1 << head) - 1) << shift | 0x6000)       # few distinct keys: equal ones must stay in slot order
        keys |= rng.integers(0, 2, 200, dtype=np.uint64) << np.uint64(63)
        keys[rng.random(200) < 0.3] = primkit.EMPTY
        rows = []
        for i, k in enumerate(int(x) for x in keys):
            if k == 0xFFFFFFFFFFFFFFFF:
                continue
            d = (k >> shift) & ((1 << head) - 1)
            if not keep[0] <= d < keep[1]:
                continue
            low = k & ((1 << shift) - 1)
            rows.append((d, low >> low_bits, i, (low << 33) | ((k >> 63) << 32) | i))
        rows.sort(key=lambda r: r[:3])
        seg = [sum(1 for r in rows if r[0] < d) for d in range(513)]
        live, mseg, tup = primkit.ref_slot_tuples(keys, top_bit, low_bits, keep)
        assert live == len(rows)
        assert mseg.tolist() == seg
        assert [int(t) for t in tup] == [r[3] for r in rows]
        assert primkit.head_hist(keys, top_bit).sum() == (keys != primkit.EMPTY).sum()
    assert primkit.slot_key_geometry(41, 13) is None and primkit.slot_key_geometry(40, 12) is None and primkit.slot_key_geometry(12, 4) is None


def test_x87_decode_against_hand_written_values():
    primkit.require_x87()
    x = np.array([1.0, -1.5, 0.0], np.longdouble)
    x = np.append(x, np.longdouble(2.0) ** -63 + np.longdouble(1.0))
    m, e, s = primkit.x87_decode(x)
    assert [int(v) for v in m] == [0x8000000000000000, 0xC000000000000000, 0, 0x8000000000000001]
    assert e.tolist() == [0, 0, 0, 0]
    assert s.tolist() == [0, 1, 0, 0]
    m, e, s = primkit.x87_decode(np.array([-0.0, 2.0 ** -70, -3.0 * 2.0 ** 100], np.longdouble))
    assert [int(v) for v in m] == [0, 0x8000000000000000, 0xC000000000000000] and e.tolist() == [0, -70, 101] and s.tolist() == [0, 0, 1]


def test_x87_fold_reference_adds_term_by_term():
    """ties to even in the 64-bit significand, one add per term (a pairwise sum gives another last bit on the third row)"""
    primkit.require_x87()
    t = np.array([[1.0, 2.0 ** -63, 2.0 ** -64, 0.0], [1.0, 2.0 ** -62, 2.0 ** -64, 0.0], [1.0, 2.0 ** -64, 2.0 ** -64, 2.0 ** -64]])
    m, e, s = primkit.x87_decode(primkit.x87_fold_ref(t))
    assert [int(v) for v in m] == [0x8000000000000002, 0x8000000000000002, 0x8000000000000000]


def test_sort_scan_and_bucket_models_on_tiny_inputs():
    k = np.array([0x31, 0x10, 0x32, 0x11, 0x30], np.uint64)
    v = np.arange(5, dtype=np.uint32)
    ko, vo = primkit.ref_sort(k, v, 4, 8)
    assert ko.tolist() == [0x10, 0x11, 0x31, 0x32, 0x30] and vo.tolist() == [1, 3, 0, 2, 4]
    assert primkit.masked(np.array([0xFFFFFFFFFFFFFFFF], np.uint64), 0, 64).tolist() == [0xFFFFFFFFFFFFFFFF]
    assert primkit.masked(np.array([0xFF], np.uint64), 5, 5).tolist() == [0]
    a = np.array([0xFFFFFFFF, 2, 3, 99], np.uint32)
    assert primkit.ref_excl_scan(a).tolist() == [0, 0xFFFFFFFF, 1, 4]       # (wraps modulo 2^32)
    assert primkit.ref_excl_scan(np.zeros(0, np.uint64)).size == 0
    assert primkit.ref_incl_max_scan(np.array([3, 1, 7, 7, 2], np.uint64)).tolist() == [3, 3, 7, 7, 7]
    kk, vv, tot = primkit.ref_compact(np.array([5, 0xFFFFFFFFFFFFFFFF, 7], np.uint64), np.array([1, 2, 3], np.uint8))
    assert kk.tolist() == [5, 7] and vv.tolist() == [1, 3] and tot == 2
    b = np.array([(1 << 8) | 0x5, (1 << 8) | 0x4, (1 << 8) | 0x3, (2 << 8) | 0x1], np.uint64)      # ign 1: 0x5 and 0x4 compare equal
    assert primkit.ref_bucket_finish(b, 1, 12).tolist() == [(1 << 8) | 0x3, (1 << 8) | 0x5, (1 << 8) | 0x4, (2 << 8) | 0x1]


def test_packed_base_models():
    seq = [0, 1, 2, 3] * 5
    codes = primkit.pack_bases(seq, 0)
    assert codes.tolist() == [0xE4E4E4E4, 0xE4]
    assert primkit.pack_bases(seq)[1] == 0xFFFFFFE4
    assert primkit.window_model(seq, False, 18) == (0b1110, 0b1111)
    assert primkit.window_model(seq, True, 0)[0] & 0xFF == 0xE4          # (ACGT is its own reverse complement)
    assert primkit.revcomp16_model(0xE4E4E4E4) == 0xE4E4E4E4 and primkit.revcomp16_model(0) == 0xFFFFFFFF
    assert primkit.spread16_model(0xFFFF) == 0x55555555 and primkit.squash16_model(0xFFFFFFFF) == 0xFFFF and primkit.squash16_model(0xAAAAAAAA) == 0
