"""Test kit of the device primitives (csrc/radix.h, scan.h, bucket.h, devutil.h): builds the harness library
tests/csrc/primitives.hip -> tests/_build/libcdm_primitives.so, binds its entry points with ctypes (host arrays in, host arrays
out) and holds the exact numpy reference models the GPU tests compare with.  Test infrastructure only: nothing in carpedeam_amd/
or bench.py loads it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from carpedeam_amd import build as pbuild

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "primitives.hip")
OUT_DIR = os.path.join(HERE, "_build")
LIB = os.path.join(OUT_DIR, "libcdm_primitives.so")
NEEDS = ("cdmMallocRaw", "cdmFree", "cdm_set_error", "cdmGetenv", "cdm_seqdb_select", "cdm_seqdb_overlay")      # what the harness takes from libcarpedeam_hip.so

CDM_OK, CDM_ERR_INVALID = 0, -3        # include/carpedeam_hip.h

# constants of the headers the models and the case lists depend on (test_primitives_host.py checks them against the source)
RX_TILE, RX_BITS, RX_BINS, RX_MAXPASS, CP_TILE, SC_TILE = 8192, 9, 512, 8, 4096, 4096
SLOT_REM, SLOT_STRAND_SHIFT, SLOT_KEY_SHIFT = 31, 32, 33
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def build(verbose=False, csrc=None, src=None, out=None):
    """Cross-compile the harness for gfx950 (the mtime rule of carpedeam_amd/build.py: again when primitives.hip or any csrc/*.h is
    newer).  csrc / src / out: another header directory, harness source or output (scratch copies with a deliberate fault)."""
    csrc = csrc or pbuild.CSRC
    src = src or SRC
    out = out or LIB
    os.makedirs(os.path.dirname(out), exist_ok=True)
    headers = tuple(os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h"))
    if not os.path.exists(pbuild.LIB):
        raise RuntimeError("libcarpedeam_hip.so is not built: the harness links against it")
    if pbuild._newer(src, out, headers):
        cmd = [pbuild.HIPCC] + pbuild.HIP_FLAGS + ["-shared", "-I" + csrc, src, "-o", out, "-L" + pbuild.HERE, "-lcarpedeam_hip",
                                                   "-Wl,--no-undefined", "-Wl,-rpath," + pbuild.HERE, "-Wl,-rpath,$ORIGIN/../../carpedeam_amd"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if verbose or r.returncode:
            sys.stderr.write(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        if r.returncode:
            raise RuntimeError("primitives harness: compile failed")
    return out


_vp, _i, _u32, _u64 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64
_SORT = [_vp, _i, _vp, _vp, _u64, _i, _i, _vp, _vp, _vp]
_COMPACT = [_vp, _vp, _vp, _u64, _vp, _vp, _vp]
_SCAN = [_vp, _vp, _vp, _u64, _i]
_BLOCK = [_vp, _vp, _u32, _u32, _vp, _vp]
SIGNATURES = {
    "prim_sort_pairs_u64_u64": _SORT, "prim_sort_pairs_u64_u32": _SORT, "prim_sort_pairs_u32_u32": _SORT, "prim_sort_pairs_u32_u64": _SORT,
    "prim_sort_keys_u64": [_vp, _i, _vp, _u64, _i, _i, _vp, _vp],
    "prim_compact_pairs_u64_u64": _COMPACT, "prim_compact_pairs_u64_u32": _COMPACT, "prim_compact_pairs_u64_u8": _COMPACT,
    "prim_sort_slot_keys": [_vp, _i, _vp, _u64, _i, _i, _vp, _u32, _u32, _vp, _vp, _vp],
    "prim_excl_scan_u32": _SCAN, "prim_excl_scan_u64": _SCAN, "prim_incl_max_scan": _SCAN,
    "prim_bucket_sort_keys": [_vp, _vp, _vp, _u64, _i, _i, _i],
    "prim_x87_fold": [_vp, _vp, _u64, _i, _i, _vp, _vp, _vp, _vp],
    "prim_x87_lt": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp],
    "prim_block_excl_sum_u32": _BLOCK, "prim_block_excl_sum_u64": _BLOCK,
    "prim_wave_append": _BLOCK, "prim_block_append": _BLOCK,
    "prim_bitop16": [_vp, _vp, _u64, _i, _vp],
    "prim_windows16": [_vp, _vp, _u32, _i, _vp],
    "prim_seqdb_select": [_vp, _vp, _vp, _i, C.POINTER(_vp)], "prim_seqdb_overlay": [_vp, _vp, _vp, _vp, _vp, C.POINTER(_vp)],
}
DTYPES = {"u64": np.uint64, "u32": np.uint32, "u8": np.uint8}
_libs = {}


def lib(path=None):
    """the harness library (built on demand), every entry point bound.  CDM_PRIMITIVES_LIB=<path> names another build of it: a
    scratch copy with a deliberate fault, to see the tests bite (docs/NOTEBOOK.md)"""
    path = path or os.environ.get("CDM_PRIMITIVES_LIB") or build()
    if path not in _libs:
        from carpedeam_amd import capi
        capi.lib()                      # libcarpedeam_hip.so first, from the tree
        l = C.CDLL(path)
        for name, sig in SIGNATURES.items():
            f = getattr(l, name)
            f.argtypes, f.restype = sig, C.c_int
        _libs[path] = l
    return _libs[path]


class PrimError(RuntimeError):
    def __init__(self, rc, msg):
        RuntimeError.__init__(self, "primitive returned %d: %s" % (rc, msg))
        self.rc = rc


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _arr(a, dt):
    a = np.ascontiguousarray(a, dtype=dt)
    return a


class Prims:
    """The primitives on one context's stream.  Every call re-reads the CDM_* switches (capi.lib()) first."""

    CU = 256

    def __init__(self, ctx, path=None):
        from carpedeam_amd import capi
        self.capi, self.ctx, self.l = capi, ctx, lib(path)
        self.stream = capi.lib().cdm_ctx_stream(ctx.h)

    def _call(self, name, *args):
        self.capi.lib()
        rc = getattr(self.l, name)(self.stream, *args)
        if rc != 0:
            raise PrimError(rc, self.capi.lib().cdm_last_error().decode())

    def sort_pairs(self, kt, vt, k, v, b, e):
        """-> keys, values, inFirst (values None for vt None: rx::sortKeys)"""
        k = _arr(k, DTYPES[kt])
        ko, first = np.empty_like(k), C.c_int(-1)
        if vt is None:
            self._call("prim_sort_keys_%s" % kt, self.CU, _p(k), k.size, b, e, _p(ko), C.byref(first))
            return ko, None, bool(first.value)
        v = _arr(v, DTYPES[vt])
        assert v.size == k.size
        vo = np.empty_like(v)
        self._call("prim_sort_pairs_%s_%s" % (kt, vt), self.CU, _p(k), _p(v), k.size, b, e, _p(ko), _p(vo), C.byref(first))
        return ko, vo, bool(first.value)

    def compact_pairs(self, vt, k, v):
        k, v = _arr(k, np.uint64), _arr(v, DTYPES[vt])
        ko, vo, tot = np.empty_like(k), np.empty_like(v), C.c_uint64(0)
        self._call("prim_compact_pairs_u64_%s" % vt, _p(k), _p(v), k.size, _p(ko), _p(vo), C.byref(tot))
        return ko, vo, int(tot.value)

    def sort_slot_keys(self, keys, top_bit, low_bits, head_hist=None, keep=(0, 512)):
        """-> live, seg[513], tuples[live]"""
        keys = _arr(keys, np.uint64)
        hh = _arr(head_hist, np.uint64) if head_hist is not None else None
        assert hh is None or hh.size == RX_BINS
        seg, live, res = np.zeros(RX_BINS + 1, np.uint64), C.c_uint64(0), np.zeros(max(keys.size, 1), np.uint64)
        self._call("prim_sort_slot_keys", self.CU, _p(keys), keys.size, top_bit, low_bits, _p(hh), keep[0], keep[1], _p(seg), C.byref(live), _p(res))
        return int(live.value), seg, res[:int(live.value)]

    def _scan(self, name, dt, a, in_place):
        a = _arr(a, dt)
        out = np.empty_like(a)
        self._call(name, _p(a), _p(out), a.size, int(in_place))
        return out

    def excl_scan(self, t, a, in_place=False):
        return self._scan("prim_excl_scan_%s" % t, DTYPES[t], a, in_place)

    def incl_max_scan(self, a, in_place=False):
        return self._scan("prim_incl_max_scan", np.uint64, a, in_place)

    def bucket_sort_keys(self, keys, shift_hi, ign, top):
        keys = _arr(keys, np.uint64)
        out = np.empty_like(keys)
        self._call("prim_bucket_sort_keys", _p(keys), _p(out), keys.size, shift_hi, ign, top)
        return out

    def x87_fold(self, terms, acc):
        """terms [rows, cols] doubles -> m, e, s, as double"""
        t = _arr(terms, np.float64)
        rows, cols = t.shape
        m, e, s, d = np.empty(rows, np.uint64), np.empty(rows, np.int32), np.empty(rows, np.uint32), np.empty(rows, np.float64)
        self._call("prim_x87_fold", _p(t), rows, cols, int(acc), _p(m), _p(e), _p(s), _p(d))
        return m, e, s, d

    def x87_lt(self, a, b):
        """a, b: (m, e, s) triples of arrays -> bool array a < b"""
        am, ae, as_ = _arr(a[0], np.uint64), _arr(a[1], np.int32), _arr(a[2], np.uint32)
        bm, be, bs = _arr(b[0], np.uint64), _arr(b[1], np.int32), _arr(b[2], np.uint32)
        out = np.empty(am.size, np.uint8)
        self._call("prim_x87_lt", _p(am), _p(ae), _p(as_), _p(bm), _p(be), _p(bs), am.size, _p(out))
        return out.astype(bool)

    def block_excl_sum(self, t, a, threads):
        a = _arr(a, DTYPES[t])
        assert a.size % threads == 0
        out, tot = np.empty_like(a), np.empty_like(a)
        self._call("prim_block_excl_sum_%s" % t, _p(a), a.size // threads, threads, _p(out), _p(tot))
        return out, tot

    def append(self, block, pred, threads):
        """-> slots (0xFFFFFFFF where pred is clear), final counter"""
        pred = _arr(pred, np.uint8)
        assert pred.size % threads == 0
        slot, cnt = np.empty(pred.size, np.uint32), np.zeros(1, np.uint32)
        self._call("prim_block_append" if block else "prim_wave_append", _p(pred), pred.size // threads, threads, _p(slot), _p(cnt))
        return slot, int(cnt[0])

    def bitop16(self, op, a):
        a = _arr(a, np.uint32)
        out = np.empty_like(a)
        self._call("prim_bitop16", _p(a), a.size, {"revcomp16": 0, "spread16": 1, "squash16": 2}[op], _p(out))
        return out

    def windows16(self, codes, L, mode):
        codes = _arr(codes, np.uint32)
        assert codes.size == (L + 15) // 16
        out = np.empty(L, np.uint32)
        self._call("prim_windows16", _p(codes), L, {"plain": 0, "forward": 1, "reverse": 2}[mode], _p(out))
        return out

    def _seqdb(self, name, *args):
        """the two sequence DB constructors: the context itself, not its stream, goes in; -> capi.SeqDb"""
        self.capi.lib()
        h = C.c_void_p()
        rc = getattr(self.l, name)(self.ctx.h, *args, C.byref(h))
        if rc != 0:
            raise PrimError(rc, self.capi.lib().cdm_last_error().decode())
        return self.capi.SeqDb(self.ctx, h)

    def seqdb_select(self, db, sel, ext_value):
        """cdm_seqdb_select: sel[i] = 0xFFFFFFFF drops sequence i, else its first sel[i] letters stay"""
        sel = _arr(sel, np.uint32)
        assert sel.size == db.n
        return self._seqdb("prim_seqdb_select", db.h, _p(sel), int(ext_value))

    def seqdb_overlay(self, base, grown, idx, ext):
        """cdm_seqdb_overlay: base with sequence idx[j] replaced by grown's sequence j (grown None: none), wasExtended flags ext"""
        idx, ext = _arr(idx, np.uint32), _arr(ext, np.uint8)
        assert ext.size == base.n and idx.size == (grown.n if grown is not None else 0)
        return self._seqdb("prim_seqdb_overlay", base.h, grown.h if grown is not None else None, _p(idx) if grown is not None else None, _p(ext))


# ====================================================================================================== reference models
def masked(k, b, e):
    """key bits [b, e) as u64"""
    k = np.asarray(k).astype(np.uint64)
    w = e - b
    if w <= 0:
        return np.zeros(k.shape, np.uint64)
    m = np.uint64(0xFFFFFFFFFFFFFFFF) if w >= 64 else np.uint64((1 << w) - 1)
    return (k >> np.uint64(b)) & m


def ref_sort(k, v, b, e):
    """stable sort of the pairs on key bits [b, e): whole keys and values in that order"""
    order = np.argsort(masked(k, b, e), kind="stable")
    return k[order], (v[order] if v is not None else None)


def ref_compact(k, v):
    keep = k != EMPTY
    return k[keep], v[keep], int(keep.sum())


def slot_key_geometry(top_bit, low_bits):
    """(headBits, shift, segment passes) or None where rx::sortSlotKeys refuses"""
    head = min(RX_BITS, top_bit)
    shift = top_bit - head
    rem = shift - low_bits
    if shift > SLOT_REM or rem < 0 or (rem + RX_BITS - 1) // RX_BITS > 2:
        return None
    return head, shift, (rem + RX_BITS - 1) // RX_BITS


def ref_slot_tuples(keys, top_bit, low_bits, keep=(0, 512)):
    """rx::sortSlotKeys after the header's comment: -> live, seg[513], tuples[live]"""
    keys = np.asarray(keys, np.uint64)
    head, shift, _ = slot_key_geometry(top_bit, low_bits)
    idx = np.arange(keys.size, dtype=np.uint64)
    digit = (keys >> np.uint64(shift)) & np.uint64((1 << head) - 1)
    livemask = (keys != EMPTY) & (digit >= np.uint64(keep[0])) & (digit < np.uint64(keep[1]))
    k, i, d = keys[livemask], idx[livemask], digit[livemask]
    low = k & np.uint64((1 << shift) - 1)
    tup = (low << np.uint64(SLOT_KEY_SHIFT)) | ((k >> np.uint64(63)) << np.uint64(SLOT_STRAND_SHIFT)) | i
    # head digit first, then key bits [lowBits, shift), stable (slot order) among equals
    order = np.argsort((d << np.uint64(shift)) | ((low >> np.uint64(low_bits)) << np.uint64(low_bits)), kind="stable")
    seg = np.zeros(RX_BINS + 1, np.uint64)
    seg[1:] = np.cumsum(np.bincount(d.astype(np.int64), minlength=RX_BINS)).astype(np.uint64)
    return int(k.size), seg, tup[order]


def head_hist(keys, top_bit):
    """what a writer of the slot keys hands in as headHist: head digit counts of the real keys"""
    keys = np.asarray(keys, np.uint64)
    head = min(RX_BITS, top_bit)
    real = keys[keys != EMPTY]
    return np.bincount(((real >> np.uint64(top_bit - head)) & np.uint64((1 << head) - 1)).astype(np.int64), minlength=RX_BINS).astype(np.uint64)


def ref_excl_scan(a):
    """exclusive prefix sum in a's own unsigned width (u32 sums wrap modulo 2^32, as the device's do)"""
    out = np.zeros_like(a)
    if a.size > 1:
        np.cumsum(a[:-1], dtype=a.dtype, out=out[1:])
    return out


def ref_incl_max_scan(a):
    return np.maximum.accumulate(a) if a.size else a.copy()


def ref_bucket_finish(k, ign, top):
    """k is stably sorted on [shiftHi, top): stable sort on [ign, top)"""
    return k[np.argsort(masked(k, ign, top), kind="stable")]


# ---------------------------------------------------------------------------------------------- x87 (np.longdouble on x86-64)
def require_x87():
    """np.longdouble must be the x87 80-bit format: the reference of every x87 test.  Fails (never skips) otherwise."""
    fi = np.finfo(np.longdouble)
    assert fi.nmant == 63 and np.dtype(np.longdouble).itemsize == 16, "np.longdouble is not the x87 80-bit format on this machine (nmant %d)" % fi.nmant


def x87_decode(x):
    """longdouble array -> (m u64, e i32, s u32) as struct X87 holds them; zero is (0, 0, 0)"""
    x = np.ascontiguousarray(x, dtype=np.longdouble)
    raw = x.view(np.uint8).reshape(-1, 16)
    m = raw[:, 0:8].copy().view(np.uint64).reshape(-1)
    se = raw[:, 8:10].copy().view(np.uint16).reshape(-1)
    e = (se & 0x7FFF).astype(np.int32) - 16383
    s = (se >> 15).astype(np.uint32)
    zero = m == 0
    e[zero] = 0
    s[zero] = 0
    return m, e, s


def x87_fold_ref(terms):
    """left-to-right fold of every row, ONE elementwise long double add per term (np.sum adds pairwise)"""
    t = np.asarray(terms, np.float64)
    acc = np.zeros(t.shape[0], np.longdouble)
    for j in range(t.shape[1]):
        acc = acc + t[:, j].astype(np.longdouble)
    return acc


# ---------------------------------------------------------------------------------------------- packed bases
def pack_bases(seq, pad_bits=0xFFFFFFFF):
    """base codes 0..3 -> u32 words, 16 per word, little end first; the unused high part of the last word is filled from pad_bits"""
    L = len(seq)
    words = np.zeros((L + 15) // 16, np.uint32)
    for i, c in enumerate(seq):
        words[i >> 4] |= np.uint32(int(c) << (2 * (i & 15)))
    if L & 15:
        words[-1] |= np.uint32((pad_bits << (2 * (L & 15))) & 0xFFFFFFFF)
    return words


def window_model(seq, rc, i):
    """(value, mask) of the 16-base window at oriented position i: the bases that exist, per base; mask covers them"""
    L = len(seq)
    o = [3 - int(c) for c in reversed(seq)] if rc else [int(c) for c in seq]
    val = mask = 0
    for q in range(16):
        if i + q < L:
            val |= o[i + q] << (2 * q)
            mask |= 3 << (2 * q)
    return val, mask


def revcomp16_model(x):
    out = 0
    for q in range(16):
        out |= (3 - ((x >> (2 * (15 - q))) & 3)) << (2 * q)
    return out


def spread16_model(x):
    return sum(((x >> b) & 1) << (2 * b) for b in range(16))


def squash16_model(x):
    return sum(((x >> (2 * b)) & 1) << b for b in range(16))
