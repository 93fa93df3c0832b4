"""The aggregation of sort 2 (aggvote.h) with wave-sized units in front of the block instances: the default, the block form alone
(CDM_AGG=block) and the vote on sorted tuples (CDM_KMER_VOTE=tuples, the independent path) give the same hit offsets and records,
array for array, on inputs built to stand on either side of every capacity of the new instance."""
import re

import numpy as np
import pytest

from carpedeam_amd import capi, synth

pytestmark = pytest.mark.gpu

PATHS = ({}, {"CDM_AGG": "block"}, {"CDM_KMER_VOTE": "tuples"})
U_CLASS_CAP = (1536, 2048, 3072)        # runsort.h
U_MAXSEG = 2048


@pytest.fixture(scope="module")
def ctx():
    return capi.Ctx(0)


@pytest.fixture(scope="module")
def bench_small(ctx):
    """30 000 reads of 100 bp at 20x coverage, as the benchmark generates them"""
    return ctx.synth(30_000, 100, 100, 7)


def random_reads(n, seed, lo=100, hi=100):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    return [letters[rng.integers(0, 4, int(rng.integers(lo, hi + 1)))].tobytes().decode() for _ in range(n)]


def run(ctx, db, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return ctx.kmermatch(db).download()
    finally:
        for k in env:
            monkeypatch.delenv(k)


def paths_agree(ctx, db, monkeypatch, extra=None):
    """the three paths under the same further switches; returns the default's arrays"""
    extra = extra or {}
    got = [run(ctx, db, monkeypatch, dict(extra, **p)) for p in PATHS]
    for p, g in zip(PATHS[1:], got[1:]):
        assert np.array_equal(got[0][0], g[0]) and np.array_equal(got[0][1], g[1]), (extra, p)
    return got[0]


def stats(ctx, db, monkeypatch, capfd, env=None):
    """what CDM_BUCKET_STATS=1 prints about one run: units per size class, units of the wave class and how many of them it handed on,
    segments no unit holds, hard units, records, entries written, the wave-sized instance's geometry"""
    capfd.readouterr()
    out = run(ctx, db, monkeypatch, dict(env or {}, CDM_BUCKET_STATS="1"))
    err = capfd.readouterr().err
    print(err)
    st = {"out": out}
    m = re.search(r"segmentedSortKeys \(units aggregated\): n (\d+), (\d+) records, (\d+) units \((\d+) / (\d+) / (\d+) by size class\): segments > (\d+): (\d+) \(<= \d+, block sort\), (\d+) longer.*; (\d+) hard units", err)
    if m:
        st.update(n=int(m[1]), records=int(m[2]), classes=tuple(int(m[i]) for i in (4, 5, 6)), long=int(m[8]) + int(m[9]), hard=int(m[10]))
    m = re.search(r"unit range (\d+): (\d+) units of at most (\d+) tuples in the wave class, (\d+) of them handed on", err)
    if m:
        st.update(range=int(m[1]), wave=int(m[2]), cap=int(m[3]), handed=int(m[4]))
    m = re.search(r"aggregate: (\d+) entries written", err)
    if m:
        st["written"] = int(m[1])
    m = re.search(r"wave-sized instance \d+: unit range \d+, (\d+) threads, table of (\d+) slots, distinct limit (\d+), (\d+) records a round", err)
    if m:
        st.update(threads=int(m[1]), table=int(m[2]), limit=int(m[3]), round=int(m[4]))
    return st


_GEOM = {}


@pytest.fixture
def geom(ctx, monkeypatch, capfd):
    """the wave-sized instance in use: tuple capacity, distinct limit, records per staging round (read from the statistics lines)"""
    if not _GEOM:
        st = stats(ctx, ctx.upload_seqs(random_reads(1, 1) * 2 + random_reads(50, 2)), monkeypatch, capfd)
        _GEOM.update(cap=st["cap"], limit=st["limit"], round=st["round"])
    return _GEOM


def test_bench_shaped_set(ctx, bench_small, monkeypatch, capfd):
    """2.4 M group tuples in 5 000 segments: most of the 9 400 unit ranges of 256 slots are crossed by a segment, and at least a thousand
    of them start a unit for the wave instance; no unit is finished twice: the wave form writes the entries the block form writes"""
    off, rec = paths_agree(ctx, bench_small, monkeypatch)
    assert len(rec) > 100_000
    wave, block = stats(ctx, bench_small, monkeypatch, capfd), stats(ctx, bench_small, monkeypatch, capfd, {"CDM_AGG": "block"})
    assert wave["wave"] >= 1000 and "wave" not in block
    assert wave["written"] == block["written"] > 0
    assert np.array_equal(wave["out"][1], rec)


def test_overflow_fallback(ctx, bench_small, monkeypatch):
    """an entry buffer of 10 entries: the run falls back to the tuple path"""
    paths_agree(ctx, bench_small, monkeypatch, {"CDM_AGG_CAP": "10"})


def copies_db(ctx, read, c, seed=3):
    return ctx.upload_seqs([read] * c + random_reads(2000, seed))


def tuples_of(length):
    """k-mer tuples of a random read of that many letters (a 100 bp read brings 82 of them, not 81)"""
    return length - 18


LOW_CAP = 768       # CDM_AGG_WAVE_CAP of the cases that want units for the block classes


def expected_route(m, wave_cap):
    """(units of the wave class, units per block class, segments no unit holds) for a DB whose one unit has m tuples in one segment"""
    if m > U_MAXSEG:
        return 0, (0, 0, 0), 1
    if m <= wave_cap:
        return 1, (0, 0, 0), 0
    return 0, tuple(int(m <= cap and (i == 0 or m > U_CLASS_CAP[i - 1])) for i, cap in enumerate(U_CLASS_CAP)), 0


@pytest.mark.parametrize("limit", [LOW_CAP, U_CLASS_CAP[0], U_CLASS_CAP[1]])
def test_copies_of_one_read_around_every_capacity(ctx, geom, monkeypatch, capfd, limit):
    """c copies of one 100 bp read: the representative's segment has 82 c tuples and is a unit of its own (the random reads next to
    it share no k-mer).  82 c one below and one above the wave instance's tuple capacity, the capacity of the first block class, and
    that of the second, which is U_MAXSEG as well; the statistics tell which instance took the unit.  The wave instance's own capacity
    is a range's last start plus U_MAXSEG, the largest unit there is - as the third class's 3072 it has no "above" - so its boundary
    is tested with the capacity lowered to 768 (CDM_AGG_WAVE_CAP), which also hands the larger units to the block classes; at the
    default capacity every unit is the wave instance's."""
    assert geom["cap"] >= U_MAXSEG + 255
    read = random_reads(1, 41)[0]
    t = tuples_of(100)
    for c in (limit // t, limit // t + 1):
        m = t * c
        db = copies_db(ctx, read, c)
        for cap, env in ((geom["cap"], {}), (LOW_CAP, {"CDM_AGG_WAVE_CAP": str(LOW_CAP)})):
            paths_agree(ctx, db, monkeypatch, env)
            st = stats(ctx, db, monkeypatch, capfd, env)
            blk = stats(ctx, db, monkeypatch, capfd, dict(env, CDM_AGG="block"))
            assert st["written"] == blk["written"] == c and st["n"] == m
            assert (st["wave"], st["classes"], st["long"]) == expected_route(m, cap) and st["handed"] == 0, (c, env, st)


def test_two_segments_fill_the_largest_class(ctx, geom, monkeypatch, capfd):
    """a segment shorter than the unit range and, starting in the same range, one just below U_MAXSEG: a unit beyond 2048 tuples - the
    wave instance's at the default capacity, the third block class's with the capacity lowered"""
    a, b = random_reads(2, 43)
    t = tuples_of(100)
    m = 3 * t + 24 * t
    assert 3 * t < 256 and 24 * t <= U_MAXSEG < m
    db = ctx.upload_seqs([a] * 3 + [b] * 24 + random_reads(2000, 5))
    for env, wave, classes in (({}, 1, (0, 0, 0)), ({"CDM_AGG_WAVE_CAP": str(LOW_CAP)}, 0, (0, 0, 1))):
        paths_agree(ctx, db, monkeypatch, env)
        st = stats(ctx, db, monkeypatch, capfd, env)
        assert (st["n"], st["wave"], st["classes"], st["long"], st["written"]) == (m, wave, classes, 0, 27), (env, st)


def test_distinct_limit(ctx, geom, bench_small, monkeypatch, capfd):
    """c copies of a 24 bp read are c distinct triples of 6 tuples each in one unit: exactly the wave instance's distinct limit (it takes
    the unit), one over it (handed on to the block instance), and with CDM_AGG_D at the limit, the limit minus one and 3 - the last puts
    every unit of the bench-shaped set on the hard list"""
    D = geom["limit"]
    read = random_reads(1, 47, 24, 24)[0]
    t = tuples_of(24)
    assert t * (D + 1) <= geom["cap"]
    for c, env, handed, hard in ((D, {}, 0, 0), (D + 1, {}, 1, 0), (D, {"CDM_AGG_D": str(D)}, 0, 0), (D, {"CDM_AGG_D": str(D - 1)}, 1, 1),
                                 (D - 1, {"CDM_AGG_D": str(D - 1)}, 0, 0)):
        db = copies_db(ctx, read, c)
        paths_agree(ctx, db, monkeypatch, env)
        st = stats(ctx, db, monkeypatch, capfd, env)
        assert (st["n"], st["wave"], st["handed"], st["hard"]) == (t * c, 1, handed, hard), (c, env, st)
        assert st["written"] == c
    for d in (D, D - 1, 40, 41, 3):
        paths_agree(ctx, bench_small, monkeypatch, {"CDM_AGG_D": str(d)})
    st = stats(ctx, bench_small, monkeypatch, capfd, {"CDM_AGG_D": "3"})
    blk = stats(ctx, bench_small, monkeypatch, capfd, {"CDM_AGG_D": "3", "CDM_AGG": "block"})
    assert st["handed"] > 1000 and st["written"] == blk["written"]


def test_staging_rounds(ctx, geom, monkeypatch, capfd):
    """c copies of a read of 18 + r letters are r run records of c tuples each - or one fewer where two of its k-mers are neighbours in
    k-mer order and their runs join, so the lengths around the target are all run and the statistics tell the records.  Wave form: one
    segment with as many records as a round holds, one fewer and one more (3 copies: the segment fills its unit range).  Block form (512
    records a round): four such segments of 2 copies in one range of 1024 slots, 511 / 512 / 513 records in all."""
    R = geom["round"]
    seen = set()
    for r in range(R - 2, R + 4):
        read = random_reads(1, 50 + r, 18 + r, 18 + r)[0]
        db = ctx.upload_seqs([read] * 3 + random_reads(2000, 9))
        paths_agree(ctx, db, monkeypatch)
        st = stats(ctx, db, monkeypatch, capfd)
        assert (st["n"], st["wave"], st["handed"]) == (3 * r, 1, 0) and r - 2 <= st["records"] <= r, st
        seen.add(st["records"])
    assert {R - 1, R, R + 1} <= seen
    seen = set()
    for last in range(126, 133):
        reads = random_reads(3, 60, 146, 146) + random_reads(1, 61, 18 + last, 18 + last)
        db = ctx.upload_seqs([x for x in reads for _ in range(2)] + random_reads(2000, 9))
        paths_agree(ctx, db, monkeypatch)
        st = stats(ctx, db, monkeypatch, capfd, {"CDM_AGG": "block"})
        assert (st["n"], st["classes"]) == (2 * (384 + last), (1, 0, 0)) and 380 + last <= st["records"] <= 384 + last, st
        seen.add(st["records"])
    assert {511, 512, 513} <= seen


def test_long_run_record(ctx, geom, monkeypatch, capfd):
    """70 copies of a 24 bp read: 6 run records of 70 tuples each - one record spans several gather batches of a wave"""
    db = copies_db(ctx, random_reads(1, 71, 24, 24)[0], 70)
    paths_agree(ctx, db, monkeypatch)
    st = stats(ctx, db, monkeypatch, capfd)
    assert (st["records"], st["n"], st["wave"], st["written"]) == (6, 420, 1, 70), st


def test_same_triple_in_two_runs(ctx, monkeypatch):
    """tandem repeats of a reverse-palindromic unit and their rotations: a member meets its representative on the same diagonal through
    k-mers of both strands, so one (representative, member, diagonal) triple is carried by runs of different strands - the strand of the
    last tuple in k-mer order is the entry's"""
    seqs = ["ACGTTGCA" * 12] * 3 + ["TGCAACGT" * 12] * 3 + ["TTGCAACG" * 11, "GTTGCAAC" * 12, "ACGTTGCA" * 9] + random_reads(500, 13)
    paths_agree(ctx, ctx.upload_seqs(seqs), monkeypatch)


def test_mixed_length_set(ctx, monkeypatch):
    """strings of 40-160 letters, copies of a low-complexity read, a dinucleotide repeat and an empty string: no slot layout"""
    seqs = synth.generate_strings(6000, seed=11, mixed=(40, 160)) + ["ACGTTGCA" * 12] * 40 + ["AC" * 50, ""]
    db = ctx.upload_seqs(seqs)
    for env in ({}, {"CDM_AGG_D": "40", "CDM_UNIT_CAP": "5"}, {"CDM_KMER_LAYOUT": "wide", "CDM_AGG_D": "7"}, {"CDM_FORCE_WIDE_WORD": "1"}):
        paths_agree(ctx, db, monkeypatch, env)


@pytest.mark.parametrize("seqs", [["ACGTTGCAAGGCTTAACGGATCCGATTACAGGCATCGA"], ["ACGTTGCAAGGCTTAACGGATCCGATTACAGGCATCGA"] * 2,
                                  ["ACGTTGCAAGGCTTAACGGA", "ACGTTGCAAGGCTTAACGGA", "TCCGTTAAGCCTTGCAACGT"], ["ACG", "TTGCA", "", "ACGTACGTAC"]])
def test_tiny_databases(ctx, monkeypatch, seqs):
    """one, two and three sequences, and a DB without a single k-mer tuple: the aggregation has no segment"""
    paths_agree(ctx, ctx.upload_seqs(seqs), monkeypatch)
