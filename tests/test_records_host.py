"""The record codecs of the host binary (carpedeam_amd/csrc/host/records.cpp: the text of the prefilter and alignment DBs to and from
the CSR record arrays, and the record side-cars) without a device: tests/cpu/records_driver.cpp links the unit with the DB reader,
the side-car unit and the built library (for cdm_evalue / cdm_bit_score only) and works on DB files this test writes.  The Python
codecs of carpedeam_amd.capi are the model; the goldens of tests/golden/synth2k (iteration 0) and tests/golden/hamming the texts.
Every case runs with one thread and with more threads than queries, where most of the record-balanced slices are empty."""
import os
import struct
import subprocess

import numpy as np
import pytest

from carpedeam_amd import capi, mmdb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "carpedeam_amd", "csrc", "host")
GOLD = os.path.join(ROOT, "tests", "golden")
PKG = os.path.join(ROOT, "carpedeam_amd")
SIDE_F_COMPACT = 1
BAD_ENTRY = "Invalid database read: the entry of key %d does not end where its index length says"


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    try:
        from carpedeam_amd import build
        build.build()
    except Exception as e:      # (no hipcc here)
        pytest.skip("libcarpedeam_hip.so can not be built here: %s" % e)
    exe = str(tmp_path_factory.mktemp("records") / "records_driver")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpu", "records_driver.cpp")] +
                       [os.path.join(HOST, f) for f in ("records.cpp", "mmdb.cpp", "sidecar.cpp")] + ["-L" + PKG, "-lcarpedeam_hip", "-Wl,-rpath," + PKG], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(threads, *args, status=0, env=None):
        r = subprocess.run([exe, str(threads)] + [str(a) for a in args], capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))
        assert r.returncode == status, (args, r.returncode, r.stderr[-2000:])
        return r
    return run


def dump(base, off, rec):
    np.ascontiguousarray(off, np.uint64).tofile(base + ".off")
    rec.tofile(base + ".rec")


def csr(base, dtype):
    return np.fromfile(base + ".off", np.uint64), np.fromfile(base + ".rec", dtype)


def same_records(got, want, ident=True):
    """field by field; seq_id as float32 bits"""
    assert len(got) == len(want)
    for f in want.dtype.names:
        if f == "seq_id":
            assert np.array_equal(got[f].view("<u4"), want[f].view("<u4")), f
        elif f != "ident" or ident:
            assert np.array_equal(got[f], want[f]), f


def seq_db(path, keyed):
    mmdb.write_from_keyed(path, keyed, mmdb.DBTYPE_NUCLEOTIDES)
    keys = sorted(keyed)
    return keys, [len(keyed[k][0]) - 1 for k in keys]


def aln_len(r):
    return max(abs(int(r["q_end"]) - int(r["q_start"])), abs(int(r["db_end"]) - int(r["db_start"]))) + 1


def columns(payload, cols):
    return [[l.split(b"\t")[c] for c in cols] for l in payload.split(b"\n") if l]


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    d = tmp_path_factory.mktemp("synth2k")
    g = {n: mmdb.load_keyed(os.path.join(GOLD, "synth2k", n + ".keyed.gz")) for n in ("reads", "pref_0", "aln_0")}
    keys, lens = seq_db(str(d / "reads"), g["reads"])
    mmdb.write_from_keyed(str(d / "pref_0"), g["pref_0"], mmdb.DBTYPE_PREFILTER_REV_RES)
    mmdb.write_from_keyed(str(d / "aln_0"), g["aln_0"], mmdb.DBTYPE_ALIGNMENT_RES)
    return {"dir": d, "keys": keys, "lens": lens, "gold": g, "many": len(keys) + 3,
            "pref": capi.parse_pref_db(g["pref_0"], keys), "aln": capi.parse_aln_db(g["aln_0"], keys)}


# ---------------------------------------------------------------------------------------------- the goldens
@pytest.mark.parametrize("many", [False, True])
def test_golden_texts_parse_as_the_model_parses_them(drv, synth, many, tmp_path):
    T, d = (synth["many"] if many else 1), synth["dir"]
    drv(T, "parse-pref", d / "reads", d / "pref_0", tmp_path / "p")
    off, rec = csr(str(tmp_path / "p"), capi.HIT_DTYPE)
    assert np.array_equal(off, synth["pref"][0])
    same_records(rec, synth["pref"][1])
    drv(T, "parse-aln", d / "reads", d / "aln_0", tmp_path / "a")
    off, rec = csr(str(tmp_path / "a"), capi.ALN_DTYPE)
    assert np.array_equal(off, synth["aln"][0])
    same_records(rec, synth["aln"][1])      # (raw_score: the integer the model derives from the bit score; ident: -1)


@pytest.mark.parametrize("many", [False, True])
def test_golden_prefilter_text_is_reproduced(drv, synth, many, tmp_path):
    T, d = (synth["many"] if many else 1), synth["dir"]
    drv(T, "parse-pref", d / "reads", d / "pref_0", tmp_path / "p")
    drv(T, "format-pref", d / "reads", tmp_path / "p", tmp_path / "out", 14)
    assert mmdb.read_db(str(tmp_path / "out")) == synth["gold"]["pref_0"]      # payloads and wasExtended flags
    assert mmdb.read_dbtype(str(tmp_path / "out")) == 14


@pytest.mark.parametrize("many", [False, True])
def test_golden_rescored_prefilter_text_is_reproduced(drv, many, tmp_path):
    g = {n: mmdb.load_keyed(os.path.join(GOLD, "hamming", n + ".keyed.gz")) for n in ("in", "pref", "res")}
    keys, _ = seq_db(str(tmp_path / "in"), g["in"])
    mmdb.write_from_keyed(str(tmp_path / "pref"), g["pref"], 7)
    mmdb.write_from_keyed(str(tmp_path / "res"), g["res"], 7)
    T = len(keys) + 3 if many else 1
    drv(T, "parse-pref", tmp_path / "in", tmp_path / "res", tmp_path / "r")
    drv(T, "format-resc", tmp_path / "in", tmp_path / "pref", tmp_path / "r", tmp_path / "out", 7)
    assert mmdb.read_db(str(tmp_path / "out")) == g["res"]
    # the golden's prefilter DB holds every query; one that lacks some: those get no entry, whatever records they have
    part = {k: v for k, v in g["pref"].items() if k % 7 != 3}
    mmdb.write_from_keyed(str(tmp_path / "part"), part, 7)
    drv(T, "format-resc", tmp_path / "in", tmp_path / "part", tmp_path / "r", tmp_path / "out2", 7)
    assert mmdb.read_db(str(tmp_path / "out2")) == {k: g["res"][k] for k in part}


def with_idents(rec, lens_text):
    """the records with an `ident` whose identity text (fast_seqid_text(ident / alnLen)) is the text's identity column"""
    rec = rec.copy()
    for j, (r, text) in enumerate(zip(rec, lens_text)):
        n = aln_len(r)
        guess = int(round(float(text) * n))
        fit = [i for i in range(max(0, guess - 2), min(n, guess + 2) + 1) if capi.fast_seqid_text(np.float32(i) / np.float32(n)) == text]
        assert fit, (text, n)
        rec["ident"][j] = fit[0]
    return rec


@pytest.mark.parametrize("many", [False, True])
def test_golden_alignment_records_format_as_the_model_formats_them(drv, synth, many, tmp_path):
    """formatAlnDb against capi.alns_to_text on the same records (parsed from aln_0, each with an ident that gives back the text's identity
    column).  The E-value and bit-score columns are checked against the Python model, not against the golden: the text does not hold
    ident, and the bit score does not fix the raw score.  The identity, coordinate and length columns are aln_0's.  Then the closure:
    parseAlnDb of the written text is the asParsed array formatAlnDb filled, and its seq_id is seqIdFrom1000(ident)."""
    T, d, keys, lens, gold = (synth["many"] if many else 1), synth["dir"], synth["keys"], synth["lens"], synth["gold"]["aln_0"]
    off, rec = synth["aln"]
    texts = [c[0].decode() for k in keys for c in columns(gold.get(k, (b"", 0))[0], [2])]
    rec = with_idents(rec, texts)
    dump(str(tmp_path / "in"), off, rec)
    residues = sum(lens)
    drv(T, "format-aln", d / "reads", "-", tmp_path / "in", residues, tmp_path / "out", tmp_path / "parsed")
    got, want = mmdb.read_db(str(tmp_path / "out")), capi.alns_to_text(off, rec, keys, lens, residues)
    assert {k: v[0] for k, v in got.items()} == want and all(v[1] == 0 for v in got.values())
    same = [2, 4, 5, 6, 7, 8, 9]
    for k, (payload, _) in gold.items():
        assert columns(got[k][0], same) == columns(payload, same)
    drv(T, "parse-aln", d / "reads", tmp_path / "out", tmp_path / "back")
    boff, back = csr(str(tmp_path / "back"), capi.ALN_DTYPE)
    parsed = np.fromfile(str(tmp_path / "parsed.rec"), capi.ALN_DTYPE)
    assert np.array_equal(boff, off)
    same_records(back, parsed, ident=False)
    assert np.array_equal(parsed["seq_id"].view("<u4"), (parsed["ident"].astype(np.float64) / 1000.0).astype(np.float32).view("<u4"))
    assert np.array_equal(parsed["ident"], [int(float(t) * 1000 + 0.5) for t in texts])


# ---------------------------------------------------------------------------------------------- directed edges
KEYS = [0, 1, 2, 5, 7, 8, 11, 20, 21, 30, 31, 40]       # (gaps: MmDb::idOf searches)
THREADS = [1, len(KEYS) + 4]


def tiny_seqs(keys=KEYS, extra=0):
    rng = np.random.RandomState(7)
    keyed = {k: (bytes(rng.choice(list(b"ACGT"), 30 + 3 * i)) + b"\n", i % 2) for i, k in enumerate(keys)}
    for j in range(extra):
        keyed[max(keys) + 1 + j] = (b"ACGTACGTAC\n", 0)
    return keyed


def short(d):
    return (int(d) + 32768) % 65536 - 32768


def hit_text(rows):
    return b"".join(b"%d\t%d\t%d\n" % r for r in rows)


PREF = {0: (hit_text([(KEYS[j % 12], 97 - 3 * j, j - 20) for j in range(50)]), 0),       # many records; negative scores and diagonals among them
        1: (b"", 0),                                                                     # an empty entry; key 2: no entry at all
        5: (hit_text([(40, -12, -32768)]), 0), 7: (hit_text([(0, 32767, 32767), (7, 0, 0)]), 0), 40: (hit_text([(5, -32768, -1)]), 1)}


@pytest.mark.parametrize("threads", THREADS)
def test_prefilter_edges(drv, threads, tmp_path):
    keys, _ = seq_db(str(tmp_path / "seq"), tiny_seqs())
    mmdb.write_from_keyed(str(tmp_path / "pref"), PREF, 14)
    drv(threads, "parse-pref", tmp_path / "seq", tmp_path / "pref", tmp_path / "p")
    off, rec = csr(str(tmp_path / "p"), capi.HIT_DTYPE)
    woff, wrec = capi.parse_pref_db(PREF, keys)
    assert np.array_equal(off, woff)
    same_records(rec, wrec)
    # formatting: one entry per query, the diagonal cast to a short, wasExtended 0 for more than one record and the sequence's flag otherwise
    rec["diagonal"][[3, 50]] = [40000, -40000]
    rec["score"][4] = -40000
    dump(str(tmp_path / "in"), off, rec)
    drv(threads, "format-pref", tmp_path / "seq", tmp_path / "in", tmp_path / "out", 14)
    seq = tiny_seqs()
    want = {}
    for i, k in enumerate(keys):
        rows = rec[int(off[i]):int(off[i + 1])]
        want[k] = (hit_text([(keys[r["target"]], int(r["score"]), short(r["diagonal"])) for r in rows]), 0 if len(rows) > 1 else seq[k][1])
    assert b"\t-25536\n" in want[0][0] and b"\t25536\n" in want[5][0]
    assert mmdb.read_db(str(tmp_path / "out")) == want
    # the rescored form: entries only for the queries of the prefilter DB, flag 0
    drv(threads, "format-resc", tmp_path / "seq", tmp_path / "pref", tmp_path / "in", tmp_path / "res", 7)
    assert mmdb.read_db(str(tmp_path / "res")) == {k: (want[k][0], 0) for k in PREF}


def aln_text(rows):
    return b"".join(b"%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % r for r in rows)


IDENTITIES = [b"1.00", b"0.999", b"0.10", b"0.099", b"0.01", b"0.009", b"0.000", b"0"]
ALN = {0: (aln_text([(KEYS[j % 12], 30 + j, IDENTITIES[j % 8], b"1.234E-05", j, 29 + j, 30, 29 + j, j, 33) for j in range(40)]), 0),    # forward and reverse coordinates
       2: (b"", 0),
       8: (aln_text([(8, -3, b"1.00", b"inf", -1, -1, 45, -1, -1, 45)]), 0),                   # the identity record of a sequence that scores 0 against itself
       40: (aln_text([(0, 7, b"0.5", b"0.000E+00", 3, 12, 63, 0, 9, 30), (40, 120, b"1.00", b"9.9E-31", 0, 62, 63, 0, 62, 63)]), 0)}


@pytest.mark.parametrize("threads", THREADS)
def test_alignment_edges(drv, threads, tmp_path):
    keys, lens = seq_db(str(tmp_path / "seq"), tiny_seqs())
    mmdb.write_from_keyed(str(tmp_path / "aln"), ALN, 5)
    drv(threads, "parse-aln", tmp_path / "seq", tmp_path / "aln", tmp_path / "a")
    off, rec = csr(str(tmp_path / "a"), capi.ALN_DTYPE)
    woff, wrec = capi.parse_aln_db(ALN, keys)
    assert np.array_equal(off, woff)
    same_records(rec, wrec)
    # formatting: identities on both sides of each branch of the identity text, over 10 000 columns; 100 / 10 000 is the float below 0.01
    idents = [10000, 9999, 9990, 1001, 1000, 999, 991, 101, 100, 99, 90, 1, 0]
    recs = np.zeros(len(idents), capi.ALN_DTYPE)
    recs["target"], recs["raw_score"], recs["ident"], recs["q_end"], recs["db_start"], recs["db_end"] = 3, 57, idents, 9999, 5, 10004
    foff = np.zeros(len(keys) + 1, np.uint64)
    foff[4:] = len(idents)
    dump(str(tmp_path / "in"), foff, recs)
    drv(threads, "format-aln", tmp_path / "seq", "-", tmp_path / "in", sum(lens), tmp_path / "out", tmp_path / "parsed")
    got = {k: v[0] for k, v in mmdb.read_db(str(tmp_path / "out")).items()}
    texts = [c[0] for c in columns(got[keys[3]], [2])]
    # Util::fastSeqIdToBuffer compares the float with the DOUBLES 0.10 and 0.01 (Util.cpp:296-300): float(0.01) lies below the double, so
    # 100 / 10 000 gets the third zero ("0.0010"), where capi.fast_seqid_text, which compares floats, writes "0.010"
    assert texts == [b"1.00", b"0.999", b"0.999", b"0.100", b"0.100", b"0.099", b"0.099", b"0.010", b"0.0010", b"0.009", b"0.009", b"0.000", b"0.000"]
    model = capi.alns_to_text(foff, recs, keys, lens, sum(lens))
    drop = idents.index(100)
    lines = lambda p: [l for j, l in enumerate(p.split(b"\n")) if j != drop]
    assert {k: lines(v) for k, v in got.items()} == {k: lines(v) for k, v in model.items()}
    # closure - without that record: its text reads back as 0.001, its asParsed record (seqIdTo1000) says 10 thousandths, as before this
    # unit was split off (docs/NOTEBOOK.md)
    drv(threads, "parse-aln", tmp_path / "seq", tmp_path / "out", tmp_path / "back")
    boff, back = csr(str(tmp_path / "back"), capi.ALN_DTYPE)
    parsed = np.fromfile(str(tmp_path / "parsed.rec"), capi.ALN_DTYPE)
    assert np.array_equal(boff, foff)
    same_records(np.delete(back, drop), np.delete(parsed, drop), ident=False)
    assert list(parsed["ident"]) == [1000, 999, 999, 100, 100, 99, 99, 10, 10, 9, 9, 0, 0]
    assert np.array_equal(parsed["seq_id"].view("<u4"), (parsed["ident"].astype(np.float64) / 1000.0).astype(np.float32).view("<u4"))


def test_decimal_reader_against_float(drv, tmp_path):
    table = ["0", "1", "1.00", "0.999", "0.10", "0.099", "0.01", "0.009", "0.000", ".5", ".001", "5.", "123456789012345", "1234567890.12345", "0.12345678901234",
             "1234567890123456", "0.123456789012345", "1234567890.123456", "0.1234567890123456789", "1.234E-05", "1e3", "2.5e+2", "9.999E+02", "inf", "nan", "-1.5", "+0.25",
             "0.30000000000000004", "4.35", "0.000001", "179769313486231", "00000000000000001.5"]
    open(str(tmp_path / "t"), "w").write("\n".join(table) + "\n")
    out = drv(1, "decimals", tmp_path / "t", "-").stdout.split("\n")[:-1]
    assert len(out) == len(table)
    fast = 0
    for text, line in zip(table, out):
        value, used = line.split()
        got, want = float.fromhex(value) if value not in ("inf", "nan") else float(value), float(text)
        assert (got == want or (got != got and want != want)) and int(used) == len(text), (text, line)
        digits = sum(c.isdigit() for c in text)
        fast += text.replace(".", "", 1).isdigit() and digits <= 15
    assert 0 < fast < len(table)        # both ways are taken: the exact division and strtod


@pytest.mark.parametrize("threads", THREADS)
def test_refused_texts(drv, threads, tmp_path):
    seq_db(str(tmp_path / "seq"), tiny_seqs())
    # a target key the sequence DB lacks
    for name, dbtype, text, cmd in (("pref", 14, hit_text([(0, 5, 1), (3, 5, 1)]), "parse-pref"), ("aln", 5, aln_text([(3, 30, b"1.00", b"1E-05", 0, 29, 30, 0, 29, 30)]), "parse-aln")):
        mmdb.write_db(str(tmp_path / name), [(1, hit_text([(1, 5, 0)]) if dbtype == 14 else b""), (7, text)], dbtype)
        r = drv(threads, cmd, tmp_path / "seq", tmp_path / name, tmp_path / "x", status=1)
        assert "Invalid database read for key 3\n" in r.stderr
    # an entry whose NUL comes before its index length says: a NUL inside the payload
    mmdb.write_db(str(tmp_path / "nul"), [(5, hit_text([(0, 5, 1)]) + b"\0" + hit_text([(1, 6, 1)])), (8, hit_text([(8, 9, 0)]))], 14)
    r = drv(threads, "parse-pref", tmp_path / "seq", tmp_path / "nul", tmp_path / "x", status=1)
    assert BAD_ENTRY % 5 in r.stderr
    # ... and an index length that reaches into the next entry
    mmdb.write_db(str(tmp_path / "long"), [(5, hit_text([(0, 5, 1)])), (8, hit_text([(8, 9, 0), (1, 2, 3)]))], 14)
    index = [l.split("\t") for l in open(str(tmp_path / "long.index")).read().split("\n") if l]
    index[0][2] = str(int(index[0][2]) + 9)
    open(str(tmp_path / "long.index"), "w").write("".join("\t".join(c) + "\n" for c in index))
    r = drv(threads, "parse-pref", tmp_path / "seq", tmp_path / "long", tmp_path / "x", status=1)
    assert BAD_ENTRY % 5 in r.stderr
    a = aln_text([(0, 30, b"1.00", b"1E-05", 0, 29, 30, 0, 29, 30)])
    mmdb.write_db(str(tmp_path / "anul"), [(5, a + b"\0" + a)], 5)
    r = drv(threads, "parse-aln", tmp_path / "seq", tmp_path / "anul", tmp_path / "x", status=1)
    assert BAD_ENTRY % 5 in r.stderr


# ---------------------------------------------------------------------------------------------- side-cars
def side_flags(db):
    magic, kind, flags = struct.unpack("<8sII", open(db + ".cdmbin", "rb").read(16))
    assert magic == b"CDMSIDE1"
    return flags


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("wide", [False, True])
def test_hit_side_car_round_trip(drv, threads, wide, tmp_path):
    keys, _ = seq_db(str(tmp_path / "seq"), tiny_seqs())
    off, rec = capi.parse_pref_db(PREF, keys)
    rec["diagonal"][3] = 40000              # (the text and the side-car hold it as a short)
    if wide:
        rec["score"][7] = 40000
    dump(str(tmp_path / "in"), off, rec)
    db = str(tmp_path / "pref")
    drv(threads, "format-pref", tmp_path / "seq", tmp_path / "in", db, 14)
    drv(threads, "hits-side-w", tmp_path / "seq", db, tmp_path / "in", 14)
    assert (side_flags(db) & SIDE_F_COMPACT) == (0 if wide else SIDE_F_COMPACT)
    assert drv(threads, "hits-side-r", tmp_path / "seq", db, tmp_path / "side").stdout == "14\n"
    drv(threads, "parse-pref", tmp_path / "seq", db, tmp_path / "text")
    soff, srec = csr(str(tmp_path / "side"), capi.HIT_DTYPE)
    toff, trec = csr(str(tmp_path / "text"), capi.HIT_DTYPE)
    assert np.array_equal(soff, toff) and np.array_equal(toff, off)
    same_records(srec, trec)
    assert trec["diagonal"][3] == 40000 - 65536 and (not wide or trec["score"][7] == 40000)


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("wide", [False, True])
def test_alignment_side_car_round_trip(drv, threads, wide, tmp_path):
    keys, lens = seq_db(str(tmp_path / "seq"), tiny_seqs())
    off, rec = capi.parse_aln_db(ALN, keys)
    rec["ident"] = [aln_len(r) * (j % 5) // 4 for j, r in enumerate(rec)]
    rec["raw_score"] = np.maximum(rec["raw_score"], 0)          # (a negative raw score alone would make the side-car wide)
    if wide:
        rec["raw_score"][5], rec["db_end"][9] = 70000, 40000
    dump(str(tmp_path / "in"), off, rec)
    db = str(tmp_path / "aln")
    drv(threads, "format-aln", tmp_path / "seq", "-", tmp_path / "in", sum(lens), db, tmp_path / "parsed")
    off.tofile(str(tmp_path / "parsed.off"))
    drv(threads, "alns-side-w", tmp_path / "seq", db, tmp_path / "parsed")
    assert (side_flags(db) & SIDE_F_COMPACT) == (0 if wide else SIDE_F_COMPACT)
    drv(threads, "alns-side-r", tmp_path / "seq", db, tmp_path / "side")
    drv(threads, "parse-aln", tmp_path / "seq", db, tmp_path / "text")
    soff, srec = csr(str(tmp_path / "side"), capi.ALN_DTYPE)
    toff, trec = csr(str(tmp_path / "text"), capi.ALN_DTYPE)
    assert np.array_equal(soff, toff) and np.array_equal(toff, off)
    same_records(srec, trec)
    assert not wide or (trec["raw_score"][5] > 65535 and trec["db_end"][9] == 40000)


def test_side_car_is_refused_for_other_files_and_not_written_when_switched_off(drv, tmp_path):
    keys, _ = seq_db(str(tmp_path / "seq"), tiny_seqs())
    off, rec = capi.parse_pref_db(PREF, keys)
    dump(str(tmp_path / "in"), off, rec)
    db = str(tmp_path / "pref")
    drv(1, "format-pref", tmp_path / "seq", tmp_path / "in", db, 14)
    drv(1, "hits-side-w", tmp_path / "seq", db, tmp_path / "in", 14, env={"CDM_SIDECAR": "0"})
    assert not os.path.exists(db + ".cdmbin") and not os.path.exists(db + ".cdmbin.tmp")
    drv(1, "hits-side-w", tmp_path / "seq", db, tmp_path / "in", 14)
    drv(1, "hits-side-r", tmp_path / "seq", db, tmp_path / "side")
    drv(1, "hits-side-r", tmp_path / "seq", db, tmp_path / "side", status=3, env={"CDM_SIDECAR": "0"})
    # a sequence DB with one key changed (the hash), one with another n
    seq_db(str(tmp_path / "seq_key"), tiny_seqs(KEYS[:-1] + [41]))
    drv(1, "hits-side-r", tmp_path / "seq_key", db, tmp_path / "side", status=3)
    seq_db(str(tmp_path / "seq_n"), tiny_seqs(extra=1))
    drv(1, "hits-side-r", tmp_path / "seq_n", db, tmp_path / "side", status=3)
    # the text DB's data file rewritten: the same bytes, another modification time (the stamp)
    data = open(db, "rb").read()
    st = os.stat(db)
    open(db, "wb").write(data)
    os.utime(db, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
    drv(1, "hits-side-r", tmp_path / "seq", db, tmp_path / "side", status=3)
