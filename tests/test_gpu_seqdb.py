"""The device-resident sequence DB container (carpedeam_amd/csrc/seqdb.hip) against its numpy model (seqdb_model.py), bit for bit:
upload, select (also through select_ext and select_assembled), overlay, concat, the packed round trips, the two downloads and the
generator's length statistics.  Every result is read back three ways - download() for the text, meta() for lengths, keys and
wasExtended flags, cdm_seqdb_export_packed for the code words, the 16-bit mask halves, the letter flags and the raw rows - and
compared with the model's planes.  cdm_seqdb_select and cdm_seqdb_overlay have no C-ABI entry: the test harness reaches them
(tests/csrc/primitives.hip, primkit.Prims.seqdb_select / seqdb_overlay).  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import primkit
import seqdb_model as M

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 1024, 1025, 2049]      # 1025: 65 code words, a wave's second trip through the copy loop
COUNTS = [1, 2, 255, 256, 257]                                    # the 256-thread kernels and their i == n sentinel thread
KINDS = ["plain", "n_ends", "n_before", "n_at", "lower_before", "lower_at", "iupac_before", "iupac_at"]
ACGT = np.frombuffer(b"ACGT", np.uint8)


def corpus(kinds, seed, repeat=1):
    """[(sequence, cut)]: every length x every cut on and beside a word boundary and the sequence's end x every kind of letter
    placed at cut - 1 (the last letter a select to `cut` keeps) or at cut (the first it drops), in a fixed shuffled order"""
    rng = np.random.default_rng(seed)
    rows = []
    for L in LENGTHS * repeat:
        for cut in sorted({c for c in (0, 1, 15, 16, 17, L - 1, L) if 0 <= c <= L}):
            for kind in kinds:
                s = ACGT[rng.integers(0, 4, L)].copy()
                at = cut - 1 if kind.endswith("_before") else cut
                if kind == "n_ends":
                    if L == 0:
                        continue
                    s[0] = s[L - 1] = ord("N")
                elif kind != "plain":
                    if not 0 <= at < L:
                        continue
                    s[at] = {"n": ord("N"), "lower": b"acgt"[at & 3], "iupac": b"RYKMSWBDHV"[at % 10]}[kind.split("_")[0]]
                rows.append((s.tobytes(), cut))
    return [rows[i] for i in rng.permutation(len(rows))]


MIXED = corpus(KINDS, 1)            # N, lower case and IUPAC letters: a raw plane
MIXED2 = corpus(KINDS, 2)
PLAIN = corpus(["plain"], 3, 6)        # no flag at all
ONLY_N = corpus(["plain", "n_ends", "n_before", "n_at"], 4, 2)      # a mask, no raw plane
CORPORA = {"mixed": MIXED, "plain": PLAIN, "only_n": ONLY_N}


@pytest.fixture(scope="module")
def kit():
    from carpedeam_amd import build, capi
    build.build()
    primkit.build()
    l = capi.lib()
    l.cdm_seqdb_export_packed.argtypes = [C.c_void_p] * 9
    l.cdm_seqdb_import_packed.argtypes = [C.c_void_p] * 8 + [C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]
    return primkit.Prims(capi.Ctx(0))


def make(kit, rows, n, first_key=5):
    """(device DB, model DB, cuts) of the first n rows: keys ascend with gaps, wasExtended alternates in runs of three"""
    assert 1 <= n <= len(rows)
    seqs, cuts = [r[0] for r in rows[:n]], np.array([r[1] for r in rows[:n]], np.uint32)
    keys, ext = [first_key + 3 * i for i in range(n)], [(i // 3) & 1 for i in range(n)]
    return kit.ctx.upload_seqs(seqs, keys, ext), M.upload(seqs, keys, ext), cuts


def same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, "%s: %s items, expected %s" % (what, got.shape, exp.shape)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %r, expected %r" % (what, bad.size, got.size, bad[0], got[bad[0]], exp[bad[0]])


def export(kit, dev):
    """-> codes, mask16, lengths, keys, ext, raw (words x 16 bytes, or None), letter flags"""
    n, w = dev.n, dev.words
    codes, mask, lens, keys = np.zeros(w, np.uint32), np.zeros(w, np.uint16), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    ext, flags, raw = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(w * 16, np.uint8) if dev.has_raw else None
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    rc = kit.capi.lib().cdm_seqdb_export_packed(kit.ctx.h, dev.h, p(codes), p(mask), p(lens), p(keys), p(ext), p(raw), p(flags))
    assert rc == 0, kit.capi.lib().cdm_last_error()
    return codes, mask, lens, keys, ext, raw, flags


def check(kit, dev, want, what):
    """the device DB against the model DB: counters, text, metadata and every packed plane"""
    p = M.planes(want)
    l = kit.capi.lib()
    assert (dev.n, dev.words, dev.residues, int(l.cdm_seqdb_max_len(dev.h))) == (len(want), p["words"], p["residues"], p["max_len"]), what
    assert dev.has_raw == want.raw_plane, what + ": raw plane"
    seqs, _, _ = dev.download()
    assert [bytes(s) for s in seqs] == [M.text(e) for e in want.entries], what + ": text"
    if dev.n:
        lens, keys, ext = dev.meta()
        same(lens, p["len"], what + ": meta lengths"); same(keys, p["key"], what + ": meta keys"); same(ext, p["ext"], what + ": meta ext")
    codes, mask, lens, keys, ext, raw, flags = export(kit, dev)
    same(codes, p["codes"], what + ": codes"); same(mask, p["mask16"], what + ": mask halves"); same(flags, p["hasN"], what + ": letter flags")
    same(lens, p["len"], what + ": lengths"); same(keys, p["key"], what + ": keys"); same(ext, p["ext"], what + ": ext")
    for i, e in enumerate(want.entries):
        if e.raw:
            at = 16 * int(p["woff"][i])
            assert raw[at:at + len(e.seq)].tobytes() == e.seq, "%s: raw row of entry %d" % (what, i)


# ====================================================================================================== upload
@pytest.mark.parametrize("name", sorted(CORPORA))
@pytest.mark.parametrize("n", COUNTS + [None])
def test_upload(kit, name, n):
    dev, want, _ = make(kit, CORPORA[name], n or len(CORPORA[name]))
    check(kit, dev, want, "upload")


# ====================================================================================================== select
def sel_patterns(want, cuts):
    lens = np.array([len(e.seq) for e in want.entries], np.uint32)
    i = np.arange(len(lens))
    return {"none": np.full(len(lens), M.DROP, np.uint32), "whole": lens, "zero": np.zeros(len(lens), np.uint32), "cuts": cuts,
            "cuts_and_drops": np.where(i % 3 == 1, np.uint32(M.DROP), cuts), "first": np.where(i == 0, lens, np.uint32(M.DROP)),
            "last": np.where(i == len(lens) - 1, cuts, np.uint32(M.DROP))}


@pytest.mark.parametrize("name", sorted(CORPORA))
@pytest.mark.parametrize("n", COUNTS + [None])
def test_select(kit, name, n):
    dev, want, cuts = make(kit, CORPORA[name], n or len(CORPORA[name]))
    for k, (pat, sel) in enumerate(sel_patterns(want, cuts).items()):
        for ext_value in (-1, 0, 1) if pat == "cuts" else ((-1, 0, 1)[k % 3],):
            out = kit.seqdb_select(dev, sel, ext_value)
            check(kit, out, M.select(want, sel, ext_value), "select %s ext %d" % (pat, ext_value))


def test_select_clears_a_dropped_n_and_keeps_a_kept_one(kit):
    """the flag rule itself, spelt out: an N at sel[i] is gone, one at sel[i] - 1 stays; a raw row stays a raw row either way"""
    seqs = [b"ACGTACGTACGTACGTN", b"ACGTACGTACGTACGNA", b"ACGTACGTACGTACGTr", b"ACGTACGTACGTACGyA"]
    dev, want = kit.ctx.upload_seqs(seqs), M.upload(seqs)
    out = kit.seqdb_select(dev, [16, 16, 16, 16], -1)
    assert export(kit, out)[6].tolist() == [0, 1, 3, 3]
    check(kit, out, M.select(want, [16, 16, 16, 16], -1), "select")
    ov = kit.seqdb_overlay(out, kit.seqdb_select(dev, [17, 17, M.DROP, M.DROP], -1), [0, 1], [0, 0, 0, 0])
    assert export(kit, ov)[6].tolist() == [1, 1, 3, 3]          # (an overlay carries whole sequences and their flags)


@pytest.mark.parametrize("n", [1, 2, 257])
def test_select_ext_and_select_assembled(kit, n):
    dev, want, cuts = make(kit, MIXED, n)
    check(kit, dev.select_ext(), M.select_ext(want), "select_ext")
    keep = [i for i in range(n) if i % 5 != 4] or [0]                    # the source lacks some keys, holds shorter, equal and empty entries
    src_seqs = [want.entries[i].seq[:int(cuts[i])] for i in keep]
    src_keys, src_ext = [want.entries[i].key for i in keep], [0] * len(keep)
    src_dev, src_want = kit.ctx.upload_seqs(src_seqs, src_keys, src_ext), M.upload(src_seqs, src_keys, src_ext)
    for min_len in (0, 17, 1025, 5000):
        check(kit, kit.ctx.select_assembled(dev, src_dev, min_len), M.select_assembled(want, src_want, min_len), "select_assembled %d" % min_len)
    idx = kit.ctx.index_copy(src_dev)                                     # (the source is read for its keys and lengths alone)
    check(kit, kit.ctx.select_assembled(dev, idx, 17), M.select_assembled(want, src_want, 17), "select_assembled on an index copy")


# ====================================================================================================== overlay
OVERLAY_PARTS = [("mixed", "mixed2"), ("plain", "mixed2"), ("mixed", "plain"), ("plain", "only_n")]      # raw plane in both, in grown only, in base only, in neither


@pytest.mark.parametrize("base_name,grown_name", OVERLAY_PARTS)
@pytest.mark.parametrize("n", COUNTS)
def test_overlay(kit, base_name, grown_name, n):
    rows = dict(CORPORA, mixed2=MIXED2)
    base, base_m, _ = make(kit, rows[base_name], n)
    rng = np.random.default_rng(n)
    ext = rng.integers(0, 2, n).astype(np.uint8)
    check(kit, kit.seqdb_overlay(base, None, [], ext), M.overlay(base_m, None, [], ext), "overlay of nothing")
    for what, idx in (("all", rng.permutation(n)), ("first", [0]), ("last", [n - 1]), ("some", np.flatnonzero(np.arange(n) % 3 == 1))):
        idx = np.asarray(idx, np.uint32)
        if idx.size == 0:
            continue
        grown, grown_m, _ = make(kit, rows[grown_name][7:], idx.size, first_key=1000)      # (other sequences than base's: shorter and longer ones)
        check(kit, kit.seqdb_overlay(base, grown, idx, ext), M.overlay(base_m, grown_m, idx, ext), "overlay %s" % what)


# ====================================================================================================== concat
@pytest.mark.parametrize("a_name,b_name", [("plain", "only_n"), ("mixed", "plain"), ("plain", "mixed"), ("mixed", "mixed")])
def test_concat(kit, a_name, b_name):
    for na, nb in ((1, 1), (2, 255), (256, 1), (257, 257)):
        a, a_m, _ = make(kit, CORPORA[a_name], na)
        b, b_m, _ = make(kit, CORPORA[b_name][11:], nb)
        check(kit, kit.ctx.concat(a, b, 1, 0), M.concat(a_m, b_m, 1, 0), "concat %d + %d" % (na, nb))
    none = np.full(na, M.DROP, np.uint32)
    empty, empty_m = kit.seqdb_select(a, none, -1), M.select(a_m, none, -1)
    assert empty.n == 0 and empty.words == 0
    check(kit, kit.ctx.concat(empty, b, 0, 1), M.concat(empty_m, b_m, 0, 1), "concat empty + b")
    check(kit, kit.ctx.concat(a, empty, 0, 1), M.concat(a_m, empty_m, 0, 1), "concat a + empty")


def test_concat_refuses_an_index_copy(kit):
    a, _, _ = make(kit, PLAIN, 5)
    idx = kit.ctx.index_copy(a)
    for x, y in ((idx, a), (a, idx)):
        with pytest.raises(kit.capi.CdmError, match=r"cdm error -3: cdm_seqdb_concat: a part holds no letters \(an index copy\)"):
            kit.ctx.concat(x, y, 0, 0)


# ====================================================================================================== packed round trips
class DevMem:
    """zeroed device memory straight from the HIP runtime (what a caller's own buffers are to the library)"""
    hip = None

    def __init__(self, nbytes):
        if DevMem.hip is None:
            DevMem.hip = C.CDLL("libamdhip64.so")
            DevMem.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            DevMem.hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
            DevMem.hip.hipFree.argtypes = [C.c_void_p]
        self.p = C.c_void_p()
        assert DevMem.hip.hipMalloc(C.byref(self.p), nbytes) == 0 and DevMem.hip.hipMemset(self.p, 0, nbytes) == 0

    def data_ptr(self):
        return self.p

    def __del__(self):
        if self.p:
            DevMem.hip.hipFree(self.p)
            self.p = None


def device_packed(dev):
    """the DB's packed planes in device buffers of their own (one spare, zeroed element each)"""
    n, w = dev.n, dev.words
    codes, mask, lens, keys, ext = DevMem(4 * w + 4), DevMem(2 * w + 2), DevMem(4 * n + 4), DevMem(4 * n + 4), DevMem(n + 1)
    dev.copy_packed(codes.data_ptr(), mask.data_ptr(), lens.data_ptr(), keys.data_ptr())
    dev.copy_ext(ext.data_ptr())
    return codes, mask, lens, keys, ext


@pytest.mark.parametrize("name", sorted(CORPORA))
@pytest.mark.parametrize("n", COUNTS)
def test_copy_packed_from_packed(kit, name, n):
    dev, want, _ = make(kit, CORPORA[name], n)
    codes, mask, lens, keys, ext = device_packed(dev)
    for ext_value in (0, 1):
        again = kit.ctx.from_packed(codes.data_ptr(), mask.data_ptr(), lens.data_ptr(), keys.data_ptr(), n, dev.words, ext_value)
        check(kit, again, M.from_packed(want, ext_value), "from_packed")
    again = kit.ctx.from_packed_ext(codes.data_ptr(), mask.data_ptr(), lens.data_ptr(), keys.data_ptr(), ext.data_ptr(), n, dev.words)
    check(kit, again, M.from_packed(want, [e.ext for e in want.entries]), "from_packed_ext")
    again = kit.ctx.from_packed_ext(codes.data_ptr(), mask.data_ptr(), lens.data_ptr(), keys.data_ptr(), None, n, dev.words)
    check(kit, again, M.from_packed(want, 0), "from_packed_ext without flags")


def test_from_packed_refuses_words_that_disagree_with_the_lengths(kit):
    dev, _, _ = make(kit, ONLY_N, 40)
    codes, mask, lens, keys, _ = device_packed(dev)
    need = dev.words
    for given in (need - 1, need + 1):
        with pytest.raises(kit.capi.CdmError, match=r"cdm error -3: cdm_seqdb_from_packed: lengths need %d code words, %d given" % (need, given)):
            kit.ctx.from_packed(codes.data_ptr(), mask.data_ptr(), lens.data_ptr(), keys.data_ptr(), 40, given, 0)


@pytest.mark.parametrize("name", sorted(CORPORA))
@pytest.mark.parametrize("n", COUNTS)
def test_export_import_packed(kit, name, n):
    dev, want, _ = make(kit, CORPORA[name], n)
    codes, mask, lens, keys, ext, raw, flags = export(kit, dev)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    for with_mask, with_raw in ((True, True), (True, False), (False, False)):
        if with_raw and raw is None:
            continue
        h = C.c_void_p()
        rc = kit.capi.lib().cdm_seqdb_import_packed(kit.ctx.h, p(codes), p(mask) if with_mask else None, p(lens), p(keys), p(ext), p(raw) if with_raw else None,
                                                    p(flags) if with_raw else None, n, dev.words, C.byref(h))
        assert rc == 0, kit.capi.lib().cdm_last_error()
        check(kit, kit.capi.SeqDb(kit.ctx, h), M.from_packed(want, [e.ext for e in want.entries], with_mask, with_raw), "import mask %d raw %d" % (with_mask, with_raw))


# ====================================================================================================== downloads
def test_download_stream_gives_the_bytes_of_download(kit):
    """pieces of 1 MiB (the smallest the call takes): an entry that a piece cuts in two, and empty entries whose '\\n' is a piece's
    last and first byte"""
    MB = 1 << 20
    seqs = [r[0] for r in MIXED[:60]] + [b"", b"", MIXED2[0][0] + b"ACGTNacgt" * 300, b"", b"ACGT"]
    dev = kit.ctx.upload_seqs(seqs)
    offs = np.zeros(len(seqs), np.uint64)
    offs[1:60] = np.cumsum([len(s) + 2 for s in seqs[:59]])            # (a spare byte between entries)
    assert int(offs[59]) + len(seqs[59]) + 1 < MB - 1
    offs[60], offs[61], offs[62], offs[63], offs[64] = MB - 1, MB, 2 * MB - 1000, 3 * MB - 1, 3 * MB
    assert len(seqs[62]) > 1000
    total = 3 * MB + 5
    whole, got, pieces = np.full(total, 7, np.uint8), np.full(total, 9, np.uint8), []
    dev.download_into(whole, offs)
    SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64)

    def sink(user, data, offset, nbytes):
        got[offset:offset + nbytes] = np.frombuffer(C.string_at(data, nbytes), np.uint8)
        pieces.append((int(offset), int(nbytes)))
        return 0

    fn = kit.capi.lib().cdm_seqdb_download_stream
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, SINK, C.c_void_p]
    assert fn(kit.ctx.h, dev.h, offs.ctypes.data, MB, SINK(sink), None) == 0
    assert pieces == [(0, MB), (MB, MB), (2 * MB, MB), (3 * MB, 5)]
    same(got, whole, "streamed bytes")
    for s, o in zip(seqs, offs):
        assert whole[int(o):int(o) + len(s) + 1].tobytes() == s + b"\n"
    assert whole[MB - 1] == 10 and whole[MB] == 10 and whole[3 * MB - 1] == 10


# ====================================================================================================== generator
@pytest.mark.parametrize("n,lo,hi", [(1, 100, 100), (257, 100, 100), (256, 17, 17), (1, 60, 150), (257, 60, 150), (1000, 1, 33)])
def test_synth_length_statistics(kit, n, lo, hi):
    db = kit.ctx.synth(n, lo, hi, 2)
    lens, keys, ext = db.meta()
    assert db.residues == int(lens.sum(dtype=np.uint64)) and int(kit.capi.lib().cdm_seqdb_max_len(db.h)) == int(lens.max())
    assert lens.min() >= lo and lens.max() <= hi and keys.tolist() == list(range(n)) and not ext.any() and not db.has_raw
    assert db.words == int(((lens.astype(np.uint64) + 15) // 16).sum())
