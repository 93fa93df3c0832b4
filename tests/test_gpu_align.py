"""`align` on the device (csrc/align.hip behind CDM_ALIGN=device): the alignment DB text and its dbtype must be byte for byte what the
reference's object code (oracle/_ref/carpedeam_full align --threads 1) and the host path (CDM_ALIGN=host) write.  Every case checks on
the module's CDM_TIMING line that the device path ran.  The legs against the reference need oracle/_ref; the device = host legs do not."""
import importlib.util
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from carpedeam_amd import mmdb
from stageflags import LINCLUST_K_FLAGS
from test_align_module import ALIGN_FLAGS, contig_set

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_FULL = os.path.join(ROOT, "oracle", "_ref", "carpedeam_full")
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
FRONT = os.path.join(ROOT, "carpedeam_amd", "carpedeam")
HAVE_REF = os.path.exists(REF_FULL)
needs_ref = pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref (the reference's object code) is not built here")
RUN_TIMEOUT = 900         # seconds for one run of a module: a hung process ends the test, not the session
LINE = re.compile(r"align: path=(\w+) hits=(\d+) slices=(\d+) rows=(\d+)")

_spec = importlib.util.spec_from_file_location("align_bench", os.path.join(ROOT, "scripts", "align_bench.py"))
align_bench = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(align_bench)


@pytest.fixture(scope="module")
def exe():
    from carpedeam_amd import build
    build.build()
    return EXE


def flags_for(wrapped, seqid, cov, covmode, threads=1):
    f = (ALIGN_FLAGS % (wrapped, seqid, cov, covmode)).split()
    f[f.index("--threads") + 1] = str(threads)
    return f


def align(binary, db, pref, out, flags, path=None, extra_env=None):
    """one run of the module -> (text DB, dbtype, (path, hits, slices, rows) of the CDM_TIMING line)"""
    env = dict(os.environ)
    env.pop("CDM_ALIGN", None)
    env.pop("CDM_ALIGN_TRACE_BUDGET", None)
    if path:
        env["CDM_ALIGN"] = path
        env["CDM_TIMING"] = "1"
    env.update(extra_env or {})
    r = subprocess.run([binary, "align", db, db, pref, out] + flags, capture_output=True, text=True, env=env, timeout=RUN_TIMEOUT)
    assert r.returncode == 0, (binary, path, r.stderr[-1500:])
    m = LINE.search(r.stderr)
    line = (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))) if m else None
    return mmdb.read_db(out), mmdb.read_dbtype(out), line


def differing(got, want):
    bad = [k for k in set(got) | set(want) if got.get(k) != want.get(k)]
    return [(k, got.get(k), want.get(k)) for k in sorted(bad)[:2]], len(bad)


@pytest.fixture(params=["host", pytest.param("reference", marks=needs_ref)])
def oracle(request):
    """what the device path is compared with: the host path (always there), the reference's object code (a leg of its own, skipped where
    oracle/_ref is not built)"""
    return request.param


def against(oracle, tmp_path, db, pref, flags, tag=""):
    """device = `oracle`, text and dbtype; returns the device's text and line"""
    t = lambda s: str(tmp_path / (s + tag))
    dev, dev_type, line = align(EXE, db, pref, t("dev"), flags, "device")
    assert line is not None and line[0] == "device", line
    if oracle == "host":
        want, want_type, hline = align(EXE, db, pref, t("host"), flags, "host")
        assert hline is not None and hline[0] == "host", hline
    else:
        want, want_type, _ = align(REF_FULL, db, pref, t("ref"), flags)
    assert differing(dev, want) == ([], 0)
    assert dev_type == want_type
    return dev, line


def records(db):
    """{query key: [the ten columns of a record]}"""
    return {k: [l.split(b"\t") for l in v[0].split(b"\n") if l] for k, v in db.items()}


# ---------------------------------------------------------------------------------------------------- 1. the reference generator
@pytest.mark.parametrize("case,wrapped,seqid,cov,covmode", [(0, 1, "0.97", "0.99", 1), (1, 1, "0.9", "0.8", 1), (2, 0, "0.9", "0.8", 0), (3, 1, "0.5", "0.3", 2), (4, 1, "0.97", "0.99", 1),
                                                          (5, 0, "0.95", "0.5", 1), (6, 1, "0.8", "0.9", 0), (7, 1, "0.97", "0.99", 1),
                                                          (8, 1, "0.97", "0.99", 1), (9, 0, "0.9", "0.8", 1), (10, 1, "0.9", "0.5", 1), (11, 1, "0.97", "0.9", 1), (12, 1, "0.6", "0.6", 0),
                                                          (13, 0, "0.97", "0.99", 1), (14, 1, "0.99", "0.99", 1), (15, 1, "0.3", "0.2", 2)])
def test_reference_generator(exe, tmp_path, oracle, case, wrapped, seqid, cov, covmode):
    """the sixteen contig sets of tests/test_align_module.py (case 8: contigs beyond 65 536 letters with wrapped scoring)"""
    rng = np.random.default_rng(100 + case)
    seqs = contig_set(rng, 4, 66000, 90000) if case in (8, 9) else contig_set(rng, 14, *([(60, 400), (200, 3000), (30, 900), (500, 6000)][case % 4]))
    t = lambda s: str(tmp_path / s)
    mmdb.write_seqdb(t("db"), seqs)
    kflags = [f if f != "0.99" else cov for f in LINCLUST_K_FLAGS]
    kflags[kflags.index("--cov-mode") + 1] = str(covmode)
    # the prefilter lists: the reference's kmermatcher where it is built, else the product's
    r = subprocess.run([REF_FULL if HAVE_REF else FRONT, "kmermatcher", t("db"), t("pref")] + kflags + ["--threads", "1", "-v", "0"], capture_output=True, text=True, timeout=RUN_TIMEOUT)
    assert r.returncode == 0, r.stderr[-1000:]
    dev, line = against(oracle, tmp_path, t("db"), t("pref"), flags_for(wrapped, seqid, cov, covmode))
    assert line[1] > 0 and line[3] > 0
    recs = records(dev)
    n_rec = sum(len(v) for v in recs.values())
    gapped = sum(1 for v in recs.values() for c in v if abs(int(c[5]) - int(c[4])) != abs(int(c[8]) - int(c[7])))
    assert n_rec > len(seqs) // 2
    if case in (1, 3):
        assert gapped > 0                               # (records whose two spans differ: alignments with gaps)


# ---------------------------------------------------------------------------------------------------- 2. directed extensions
def rnd(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def pair_db(tmp_path, seqs, hits, tag=""):
    """a sequence DB and a hand-made prefilter DB: hits = [(query, target, reverse, diagonal)]; every sequence gets its identity hit"""
    t = lambda s: str(tmp_path / (s + tag))
    mmdb.write_seqdb(t("db"), seqs)
    pref = []
    for k in range(len(seqs)):
        lines = ["%d\t100\t0\n" % k] + ["%d\t%d\t%d\n" % (tg, -100 if rev else 100, d) for q, tg, rev, d in hits if q == k]
        pref.append((k, "".join(lines).encode()))
    mmdb.write_db(t("pref"), pref, mmdb.DBTYPE_PREFILTER_REV_RES)
    return t("db"), t("pref")


LOOSE = dict(seqid="0.0", cov="0.0", covmode=0)


def test_zdrop_exit(exe, tmp_path, oracle):
    """a shared prefix followed by unrelated tails: the extension leaves by z-drop and the alignment ends near the prefix's end"""
    rng = np.random.default_rng(1)
    head = rnd(rng, 300)
    seqs = [head + rnd(rng, 700), head + rnd(rng, 700)]
    db, pref = pair_db(tmp_path, seqs, [(0, 1, False, 0), (1, 0, False, 0)])
    dev, line = against(oracle, tmp_path, db, pref, flags_for(0, **LOOSE))
    assert line[1] == 2
    assert line[3] < 2 * 3 * 1999                       # fewer rows than full matrices take: the search stopped
    for q, tg in ((0, 1), (1, 0)):
        c = [c for c in records(dev)[q] if int(c[0]) == tg][0]
        assert int(c[4]) == 0 and 290 <= int(c[5]) < 340 and int(c[7]) == 0 and 290 <= int(c[8]) < 340, c


def test_indel_longer_than_the_band(exe, tmp_path, oracle):
    rng = np.random.default_rng(2)
    x, y = rnd(rng, 400), rnd(rng, 400)
    seqs = [x + y, x + rnd(rng, 100) + y]
    db, pref = pair_db(tmp_path, seqs, [(0, 1, False, 0), (1, 0, False, 0)])
    dev, line = against(oracle, tmp_path, db, pref, flags_for(0, **LOOSE))
    assert line[1] == 2
    c = [c for c in records(dev)[0] if int(c[0]) == 1][0]
    assert int(c[5]) < 500 and int(c[8]) < 500, c      # the band of 64 does not reach over 100 inserted letters: the alignment ends at x


def test_n_runs_and_iupac(exe, tmp_path, oracle):
    rng = np.random.default_rng(3)
    a = rnd(rng, 150) + "N" * 40 + rnd(rng, 150) + "RYKM" * 5 + rnd(rng, 200) + "NNN"
    b = list(a)
    for p in (20, 95, 170, 260, 333, 400, 480):
        b[p] = "ACGT"[("ACGT".index(b[p]) + 1) % 4] if b[p] in "ACGT" else "A"
    b = "".join(b[:200]) + "N" * 7 + "".join(b[200:410]) + "".join(b[415:])
    c = "N" * 30 + a[30:300].lower() + "SWBDHV" + a[306:]
    seqs = [a, b, c]
    hits = [(i, j, False, 0) for i in range(3) for j in range(3) if i != j]
    db, pref = pair_db(tmp_path, seqs, hits)
    for wrapped in (0, 1):
        dev, line = against(oracle, tmp_path, db, pref, flags_for(wrapped, **LOOSE), tag="w%d" % wrapped)
        assert line[1] >= 6                             # (the identity hits of sequences with N are extended as well: N scores against itself)


def test_repeats_where_equal_row_maxima_decide(exe, tmp_path, oracle):
    """poly-A and dinucleotide repeats: many cells of a row share the best score, the order of the row maximum picks the end cell"""
    rng = np.random.default_rng(4)
    f1, f2 = rnd(rng, 60), rnd(rng, 60)
    seqs = ["A" * 200, "A" * 90 + "C" + "A" * 88, "AC" * 150, "AC" * 70 + "G" + "AC" * 75, f1 + "A" * 120 + f2, f1 + "A" * 131 + f2, f1 + "AC" * 60 + f2, f1 + "AC" * 66 + f2,
            "ACG" * 80 + "T" + "ACG" * 30, "ACG" * 100]
    hits = [(i, i ^ 1, False, 0) for i in range(10)] + [(0, 1, False, 5), (2, 3, False, 2), (3, 2, False, -4), (8, 9, False, 3)]
    db, pref = pair_db(tmp_path, seqs, hits)
    for wrapped in (0, 1):
        dev, line = against(oracle, tmp_path, db, pref, flags_for(wrapped, **LOOSE), tag="w%d" % wrapped)
        assert line[1] >= 10


def test_tiny_sequences(exe, tmp_path, oracle):
    """sequences of 1, 15, 16 and 17 letters: the 16-position blocks around the band with nothing, almost one, one and a little more to hold"""
    rng = np.random.default_rng(5)
    seqs, hits = [], []
    for n in (1, 15, 16, 17):
        base = rnd(rng, n)
        var = list(base)
        var[n // 2] = "ACGT"[("ACGT".index(var[n // 2]) + 1) % 4]
        k = len(seqs)
        seqs += [base, "".join(var), base + "ACGT"[int(rng.integers(0, 4))]]
        hits += [(k + i, k + j, False, 0) for i in range(3) for j in range(3) if i != j]
    # ... and each of them against longer ones
    longer = rnd(rng, 50)
    k = len(seqs)
    seqs += [longer, longer[:17], longer[3:19], longer[10:25]]
    hits += [(k, k + 1, False, 0), (k + 1, k, False, 0), (k, k + 2, False, 3), (k + 2, k, False, -3), (k, k + 3, False, 10), (k + 3, k, False, -10)]
    db, pref = pair_db(tmp_path, seqs, hits)
    dev, line = against(oracle, tmp_path, db, pref, flags_for(0, **LOOSE))
    assert line[1] > 0


def test_reverse_strand_hits(exe, tmp_path, oracle):
    rng = np.random.default_rng(6)
    seqs, hits = [], []
    for _ in range(6):
        base = rnd(rng, int(rng.integers(200, 900)))
        var = align_bench.mutate(rng, np.array(["ACGT".index(c) for c in base], np.uint8), 0.02, 0.01)
        rc = align_bench.revcomp(bytes(b"ACGT"[i] for i in var)).decode()
        k = len(seqs)
        seqs += [base, rc]
        for q, tg in ((k, k + 1), (k + 1, k)):
            for wrapped in (False, True):
                hit = align_bench.find_diagonal(seqs[q].encode(), seqs[tg].encode(), wrapped)
                assert hit is not None and hit[0]
                hits.append((q, tg, True, hit[1], wrapped))
    for wrapped in (0, 1):
        db, pref = pair_db(tmp_path, seqs, [h[:4] for h in hits if h[4] == bool(wrapped)], tag="w%d" % wrapped)
        dev, line = against(oracle, tmp_path, db, pref, flags_for(wrapped, **LOOSE), tag="w%d" % wrapped)
        assert line[1] >= 8                             # (a seed that spans both sequences needs no extension)
        recs = records(dev)
        assert sum(1 for v in recs.values() for c in v if int(c[7]) > int(c[8])) >= 10        # reverse-strand records: dbStart > dbEnd


@pytest.mark.parametrize("threads,oracle", [(1, "host"), (4, "host"), pytest.param(1, "reference", marks=needs_ref)])
def test_stale_letter_behind_a_shorter_sequence(exe, tmp_path, threads, oracle):
    """a seed that ends on the last letter of a sequence that follows a longer one in the same worker thread: the reverse extension's
    first letter is what the longer one left in the buffer.  Against the host path at the same thread count, and the reference at one"""
    rng = np.random.default_rng(7)
    seqs, hits = [], []
    for g in range(8):
        long_one = rnd(rng, 420 + 10 * g)
        short = rnd(rng, 200 + g)
        var = list(short)
        for p in (30, 90, 91, 150):
            var[p] = "ACGT"[("ACGT".index(var[p]) + 1) % 4]
        var = "".join(var[:60]) + "".join(var[62:])                # a deletion, so that the extension is needed
        k = len(seqs)
        seqs += [long_one, short, var, long_one[5:300]]
        # the long one first (its letters stay behind in the buffers), then hits whose seeds end on the last letter of query and target
        hits += [(k, k + 3, False, 5), (k + 1, k + 2, False, 2), (k + 2, k + 1, False, -2), (k + 1, k + 3, False, 0), (k + 3, k + 1, False, 0)]
    db, pref = pair_db(tmp_path, seqs, hits)
    for wrapped in (0, 1):
        dev, line = against(oracle, tmp_path, db, pref, flags_for(wrapped, threads=threads, **LOOSE), tag="w%d" % wrapped)
        assert line[1] > 0


def test_stale_letters_through_the_c_abi(exe):
    """cdm_align_hits called directly (capi.Ctx.align_hits) on pairs so short that the stale first column of the reverse extension decides.
    The seed ends on the last letter of both sequences, so the reversed arrays start with the stale letters (rev[0]) and go on with
    seq[L - 1], ... seq[1].  Expected values by hand from host/align.cpp:
      "A" / "A": the reverse extension is the one cell (stale_q, stale_t).  Equal letters below 4 score +2: end cell (0, 0), start 0, the
        forward run "A" / "A" gives score 2, one identity, one column.  Different letters score -3, a wildcard (4) scores 0: no cell above
        0, max_q = max_t = -1, the start is 1 - (0 - 1) - 1 = 1, the forward run is empty: score 0, start 1, end 0, nothing counted.
      "AC" / "AC": cells (stale, stale) and ('C', 'C').  Equal stale letters: 2 + 2 at (1, 1), start 0, forward "AC" / "AC" = 4, two
        identities.  Otherwise the best the second cell reaches is -3 + 2 (or 0 + 2 = 2 behind a wildcard, end cell (1, 1), start 0 as
        well); with a mismatch nothing is above 0: start 2, empty forward run."""
    from carpedeam_amd import capi
    ctx = capi.Ctx(0)
    db = ctx.upload_seqs(["A", "A", "AC", "AC"])
    hits = np.zeros(50, capi.ALIGN_HIT_DTYPE)
    want = []
    for pair, L in ((0, 1), (2, 2)):
        for sq in range(5):
            for st in range(5):
                h = hits[len(want)]
                h["query"], h["target"], h["q_len"], h["t_len"], h["q_end"], h["t_end"] = pair, pair + 1, L, L, L - 1, L - 1
                h["stale_q"], h["stale_t"] = sq, st
                if sq == st and sq < 4 or (L == 2 and 4 in (sq, st)):
                    want.append((2 * L, 0, L - 1, 0, L - 1, L, L))
                else:
                    want.append((0, L, L - 1, L, L - 1, 0, 0))
    res, stats = ctx.align_hits(db, hits)
    got = [tuple(int(r[f]) for f in ("score", "q_start", "q_end", "t_start", "t_end", "identities", "columns")) for r in res]
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:4]
    assert len(set(got)) == 4 and stats["slices"] == 1 and stats["rows"] > 0


# ---------------------------------------------------------------------------------------------------- 3. random campaign
def test_random_campaign(exe, tmp_path):
    """200 random small DBs of 30-400 letters: device = host at --threads 1"""
    def one(i):
        rng = np.random.default_rng(5000 + i)
        wrapped = bool(i & 1)
        seqs, pref = align_bench.make_db(9000 + i, int(rng.integers(1, 4)), 30, 400, variants=int(rng.integers(1, 4)), wrapped=wrapped, rate_scale=4.0)
        d = tmp_path / ("c%d" % i)
        d.mkdir()
        align_bench.write_db(str(d / "x"), seqs, pref)
        flags = flags_for(int(wrapped), ["0.0", "0.9", "0.97"][i % 3], ["0.0", "0.8"][i % 2], [0, 1, 2][i % 3])
        dev, _, line = align(EXE, str(d / "x_seq"), str(d / "x_pref"), str(d / "dev"), flags, "device")
        host, _, hline = align(EXE, str(d / "x_seq"), str(d / "x_pref"), str(d / "host"), flags, "host")
        return i, line, hline, differing(dev, host)

    with ThreadPoolExecutor(8) as pool:
        out = list(pool.map(one, range(200)))
    assert all(line is not None and line[0] == "device" and hline[0] == "host" for _, line, hline, _ in out)
    bad = [(i, d) for i, _, _, d in out if d[1]]
    assert not bad, bad[:2]
    assert sum(line[1] for _, line, _, _ in out) > 200            # hits that went through the kernel: more than one per DB


# ---------------------------------------------------------------------------------------------------- 4. slices
def test_slices(exe, tmp_path):
    seqs, pref = align_bench.make_db(77, 12, 300, 900)
    align_bench.write_db(str(tmp_path / "x"), seqs, pref)
    db, pf = str(tmp_path / "x_seq"), str(tmp_path / "x_pref")
    flags = flags_for(1, "0.9", "0.8", 1)
    whole, _, line = align(EXE, db, pf, str(tmp_path / "whole"), flags, "device")
    assert line[0] == "device" and line[2] == 1 and line[1] > 30
    cut, _, cline = align(EXE, db, pf, str(tmp_path / "cut"), flags, "device", {"CDM_ALIGN_TRACE_BUDGET": str(1 << 20)})
    assert cline[0] == "device" and cline[2] >= 3 and cline[1] == line[1] and cline[3] == line[3], cline
    assert differing(cut, whole) == ([], 0)
    # ... and in launches of a few hits each
    few, _, fline = align(EXE, db, pf, str(tmp_path / "few"), flags, "device", {"CDM_LAUNCH_SLICE": "7"})
    assert fline[0] == "device" and differing(few, whole) == ([], 0)


# ---------------------------------------------------------------------------------------------------- 5. a size a user would run
@needs_ref
def test_user_size_equals_reference(exe, tmp_path):
    """contigs of 1-5 kb, sized so that the reference's module needs about a minute at one thread: about 4 x 10^8 anti-diagonal rows (the host path counts
    90 000 rows per family of the generator: 4 800 families)"""
    seqs, pref = align_bench.make_db(2024, 4800, 1000, 5000)
    align_bench.write_db(str(tmp_path / "x"), seqs, pref)
    db, pf = str(tmp_path / "x_seq"), str(tmp_path / "x_pref")
    flags = flags_for(1, "0.9", "0.8", 1)
    dev, dev_type, line = align(EXE, db, pf, str(tmp_path / "dev"), flags, "device")
    assert line[0] == "device" and line[3] >= 4 * 10 ** 8, line
    want, want_type, _ = align(REF_FULL, db, pf, str(tmp_path / "ref"), flags)
    assert differing(dev, want) == ([], 0)
    assert dev_type == want_type
