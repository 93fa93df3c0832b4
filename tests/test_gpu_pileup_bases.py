"""cdm_pileup_bases on the device against tests/bases_model.py: the directed and random alignment sets of tests/pileupcases.py, directed
sets of its own at the sizes where the column walk of a wave, the position tiles, the thresholds and the site order can go wrong, the
refusals, and the synth2k reads through cdm_kmermatch and cdm_rescore.  Every case is also held against cdm_pileup_depth on the same
handles.  Every comparison is between integers and exact."""
import numpy as np
import pytest

import bases_model as bm
import pileupcases as pc
from carpedeam_amd import capi
from gpuutil import gold
from pileup_model import codes_of, orient, unorient

pytestmark = pytest.mark.gpu

PAR = dict(bm.DEFAULTS)


@pytest.fixture(scope="module")
def ctx():
    return capi.Ctx(0)


def handles(ctx, c):
    db = ctx.upload_seqs(c["seqs"], ext=c["ext"])
    return db, ctx.upload_alns(db, c["off"], c["rec"])


def model(c, par, queries=None):
    return bm.bases(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"] if queries is None else queries, min_seq_id=c["min_seq_id"], skip=c["skip"], **par)


def read_n_columns(c, queries):
    """per listed query, how many counted records put an N of the read on each position"""
    thr = np.float32(c["min_seq_id"])
    out = []
    for q in queries:
        n = np.zeros(len(c["seqs"][q]), np.int64)
        for r in c["rec"][int(c["off"][q]):int(c["off"][q + 1])]:
            t = int(r["target"])
            if t == q or not (np.float32(r["seq_id"]) >= thr) or (c["skip"] and c["ext"][t]):
                continue
            tn = codes_of(c["seqs"][t])[1]
            qs, qe, ds, de, rev = orient(r, len(tn))
            op = ds + np.arange(qe - qs + 1)
            n[qs:qe + 1] += tn[len(tn) - 1 - op if rev else op]
        out.append(n)
    return out


def same_sites(got, want, what):
    assert got.dtype == bm.SITE_DTYPE and got.shape == want.shape, (what, got.shape, want.shape)
    for f in ("query", "pos", "info", "counts"):
        assert np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:5].tolist())


def check(ctx, c, par, queries=None, want=None, what="", h=None):
    """the device with and without each optional output against the model, and against cdm_pileup_depth; -> the model's results"""
    q = list(c["queries"] if queries is None else queries)
    db, alns = h or handles(ctx, c)
    w_stats, w_tables, w_sites = want or model(c, par, q)
    a = (db, alns, q, par["mask_ends"], par["min_depth"], par["min_alt_count"], par["min_alt_percent"], c["min_seq_id"], c["skip"])
    plain = ctx.pileup_bases(*a)
    s1, t1 = ctx.pileup_bases(*a, counts=True)
    s2, sites2 = ctx.pileup_bases(*a, sites=True)
    s3, t3, sites3 = ctx.pileup_bases(*a, counts=True, sites=True)
    for got in (plain, s1, s2, s3):
        assert got.dtype == np.uint64 and got.shape == (len(q), 8), what
        assert np.array_equal(got, w_stats), (what, par, np.argwhere(got != w_stats)[:5].tolist(), got.tolist()[:3], w_stats.tolist()[:3])
    for tables in (t1, t3):
        assert len(tables) == len(q)
        for k, (g, w) in enumerate(zip(tables, w_tables)):
            assert g.dtype == np.uint32 and g.shape == w.shape, (what, k)
            assert np.array_equal(g, w), (what, par, k, np.argwhere(g != w)[:5].tolist())
    for sites in (sites2, sites3):
        same_sites(sites, w_sites, what)
    # the cross-checks: reads and columns are the depth's; the flagged figure counts the query's site records; without a mask every
    # column of a counted record is either counted here or an N of its read
    d_stats, d_tracks = ctx.pileup_depth(db, alns, q, 0, c["min_seq_id"], c["skip"], track=True)
    assert np.array_equal(plain[:, 0:2], d_stats[:, 0:2]), what
    assert np.array_equal(plain[:, 7], np.bincount(sites2["query"], minlength=len(q)).astype(np.uint64)[:len(q)]), what
    if par["mask_ends"] == 0:
        for g, n, d in zip(t1, read_n_columns(c, q), d_tracks):
            assert np.array_equal(g.sum(axis=1, dtype=np.int64) + n, d.astype(np.int64)), what
    return w_stats, w_tables, w_sites


def with_par(**kw):
    p = dict(PAR)
    p.update(kw)
    return p


@pytest.mark.parametrize("mask_ends", [0, 3])
@pytest.mark.parametrize("name,make", pc.DIRECTED, ids=[n for n, _ in pc.DIRECTED])
def test_directed_cases(ctx, name, make, mask_ends):
    c = make()
    stats, _, _ = check(ctx, c, with_par(mask_ends=mask_ends), what=name)
    if name == "query_lists":           # the query with only its identity record: zeros
        assert stats[c["queries"].index(7)].tolist() == [0] * 8


# ------------------------------------------------------------------------------------------------ directed cases of these kernels
def test_column_steps_of_a_wave(ctx):
    """one contig of 300 letters under reads of 1, 63, 64, 65, 127, 128, 129 and 200 letters (N in some), each whole on both strands,
    and in part: overlaps that start mid-word on the read and cross its 16-base words, on both strands"""
    rng = np.random.default_rng(91)
    lens = (1, 63, 64, 65, 127, 128, 129, 200)
    seqs = [pc.rand_seq(rng, 300, 0.01)] + [pc.rand_seq(rng, n, 0.02) for n in lens]
    recs = [pc.identity(seqs, 0)]
    for t, n in enumerate(lens, start=1):
        recs.append(unorient(t, 7, 7 + n - 1, 0, n - 1, False, n))
        recs.append(unorient(t, 300 - n, 299, 0, n - 1, False, n))
        if n > 1:
            recs.append(unorient(t, 33, 33 + n - 1, 0, n - 1, True, n))
            for ds, m in ((7, n - 10), (17, min(40, n - 17)), (15, 2), (n - 33, 33)):
                for rev in (False, True):
                    recs.append(unorient(t, 50 + ds, 50 + ds + m - 1, ds, ds + m - 1, rev, n))
    c = pc.case(seqs, {0: recs}, [0])
    for mask in (0, 3, 64):
        stats, _, _ = check(ctx, c, with_par(mask_ends=mask, min_depth=1, min_alt_count=1), what="columns, mask %d" % mask)
        assert stats[0][0] == len(recs) - 1 and stats[0][2] > 0


LENGTHS = (1, 2, 2047, 2048, 300, 2049, 4097)       # adjacent contigs; the one of 300 letters has only its identity record
STEP = 512


def boundaries():
    """sequences 0..6: the contigs (N at 1 % of the letters); then one read of each contig's length, a read of 10 letters and one of 1.
    Per contig with records: the full-length read from its first letter to its last on both strands, one letter on the last position,
    and the 10-letter read around every multiple of STEP (the tile of 2048 positions among them) on both strands"""
    rng = np.random.default_rng(92)
    seqs = [pc.rand_seq(rng, n, 0.01) for n in LENGTHS]
    full = {}
    for q, n in enumerate(LENGTHS):
        if n != 300:
            full[q] = len(seqs)
            seqs.append(pc.rand_seq(rng, n))
    short, one = len(seqs), len(seqs) + 1
    seqs += [pc.rand_seq(rng, 10), pc.rand_seq(rng, 1)]
    per = {}
    for q, n in enumerate(LENGTHS):
        per[q] = [pc.identity(seqs, q)]
        if n == 300:
            continue
        per[q].append(unorient(full[q], 0, n - 1, 0, n - 1, False, n))
        if n > 1:
            per[q].append(unorient(full[q], 0, n - 1, 0, n - 1, True, n))
        per[q].append(unorient(one, n - 1, n - 1, 0, 0, False, 1))
        per[q].append(unorient(one, 0, 0, 0, 0, False, 1))
        for m in range(STEP, n, STEP):
            per[q].append(unorient(short, m - 10, m - 1, 0, 9, False, 10))
            if m + 10 <= n:
                per[q].append(unorient(short, m, m + 9, 0, 9, True, 10))
                per[q].append(unorient(short, m - 5, m + 4, 0, 9, False, 10))
                per[q].append(unorient(short, m - 1, m, 3, 4, True, 10))
    return pc.case(seqs, per, list(range(len(LENGTHS))))


BOUNDS_PAR = with_par(min_depth=2, min_alt_count=1)


@pytest.fixture(scope="module")
def bounds():
    c = boundaries()
    return c, model(c, BOUNDS_PAR)


def subset(want, q):
    """the model's results of boundaries() for the query list q"""
    stats, tables, sites = want
    parts = []
    for k, i in enumerate(q):
        s = sites[sites["query"] == i].copy()
        s["query"] = k
        parts.append(s)
    return stats[q], [tables[i] for i in q], np.concatenate(parts)


def test_adjacent_contigs_around_the_tile_size(ctx, bounds):
    c, want = bounds
    stats, tables, sites = check(ctx, c, BOUNDS_PAR, want=want, what="boundaries")
    k = LENGTHS.index(300)
    assert stats[k - 1][0] > 0 and stats[k + 1][0] > 0 and stats[k].tolist() == [0] * 8 and not tables[k].any()
    # the full-length reads reach the first and the last letter of every contig with records; sites exist on both sides of the empty one
    for q, n in enumerate(LENGTHS):
        if n != 300:
            assert tables[q][0].sum() >= 2 and tables[q][n - 1].sum() >= 2
    assert (sites["query"] == k).sum() == 0 and (sites["query"] == k - 1).sum() > 100 and (sites["query"] == k + 1).sum() > 100
    assert np.all(np.diff(sites["query"].astype(np.int64)) >= 0)        # listed order, then ascending positions
    assert all(np.all(np.diff(sites["pos"][sites["query"] == q].astype(np.int64)) > 0) for q in range(len(LENGTHS)))


def test_query_orders_and_subsets(ctx, bounds):
    c, want = bounds
    h = handles(ctx, c)
    n = len(LENGTHS)
    for q in (list(range(n))[::-1], [3, 6, 0, 5, 1, 4, 2], [5, 2], [6], [4]):
        check(ctx, c, BOUNDS_PAR, queries=q, want=subset(want, q), what=str(q), h=h)


def columns_case(columns):
    """columns: (contig letter, (nA, nC, nG, nT)) per position -> a contig under one-letter reads"""
    seqs = ["".join(ref for ref, _ in columns), "A", "C", "G", "T"]
    recs = [pc.identity(seqs, 0)]
    for i, (_, counts) in enumerate(columns):
        for b, n in enumerate(counts):
            recs += [unorient(1 + b, i, i, 0, 0, False, 1)] * n
    return pc.case(seqs, {0: recs}, [0])


def flags_by_pos(sites):
    return {int(s["pos"]): (int(s["info"]) >> 8, (int(s["info"]) >> 4) & 15, int(s["info"]) & 15) for s in sites}


def test_thresholds_at_equality(ctx):
    C, D, V = bm.CALLED, bm.DIFFERS, bm.VARIABLE
    cols = [("A", (3, 0, 0, 0)),        # 0: d = min_depth - 1: not called
            ("A", (4, 0, 0, 0)),        # 1: d = min_depth: called
            ("A", (6, 2, 0, 0)),        # 2: second = min_alt_count, second * 100 = 200 = 25 * 8: variable
            ("A", (7, 2, 0, 0)),        # 3: 200 < 25 * 9: not variable
            ("A", (3, 1, 0, 0)),        # 4: 100 = 25 * 4 but second = min_alt_count - 1: not variable
            ("C", (4, 4, 0, 0)),        # 5: a tie with the contig's letter among the tied: major is that letter, not DIFFERS
            ("T", (0, 4, 4, 0)),        # 6: a tie without it: major is the lowest code, not DIFFERS
            ("A", (1, 0, 5, 0)),        # 7: a strict winner that is not the contig's letter: DIFFERS
            ("N", (0, 0, 0, 5))]        # 8: a contig N under a strict winner: DIFFERS; no part of `mismatches`
    c = columns_case(cols)
    par = dict(mask_ends=0, min_depth=4, min_alt_count=2, min_alt_percent=25)
    stats, _, sites = check(ctx, c, par, what="equality")
    assert flags_by_pos(sites) == {2: (C | V, 0, 0), 5: (C | V, 1, 1), 6: (C | V, 1, 3), 7: (C | D, 2, 0), 8: (C | D, 3, 4)}
    assert stats[0].tolist() == [55, 55, 55, 2 + 2 + 1 + 4 + 8 + 5, 8, 2, 3, 5]
    # the percent rule one short: a second allele of 1 in 3 is variable at 33 % (100 >= 99) and not at 34 % (100 < 102)
    c = columns_case([("A", (2, 1, 0, 0))])
    for pct, n in ((33, 1), (34, 0)):
        stats, _, sites = check(ctx, c, dict(mask_ends=0, min_depth=3, min_alt_count=1, min_alt_percent=pct), what="percent %d" % pct)
        assert stats[0].tolist() == [3, 3, 3, 1, 1, 0, n, n] and len(sites) == n


def test_the_mask(ctx):
    rng = np.random.default_rng(93)
    seqs = [pc.rand_seq(rng, 200), pc.rand_seq(rng, 5), pc.rand_seq(rng, 100), pc.rand_seq(rng, 128), pc.rand_seq(rng, 129)]
    five = pc.case(seqs, {0: [pc.identity(seqs, 0), unorient(1, 20, 24, 0, 4, False, 5), unorient(1, 40, 44, 0, 4, True, 5)]}, [0])
    for mask, per_read in ((0, 5), (1, 3), (2, 1), (3, 0)):
        stats, tables, _ = check(ctx, five, with_par(mask_ends=mask, min_depth=1), what="five letters, mask %d" % mask)
        assert stats[0][:3].tolist() == [2, 10, 2 * per_read]
        if mask == 2:       # the middle letter of the read alone
            assert tables[0][22].sum() == 1 and tables[0][42].sum() == 1 and tables[0].sum() == 2
    # mask_ends = 64: a read shorter than 2 x 64 leaves nothing, one of 128 nothing either, one of 129 its middle letter
    recs = [pc.identity(seqs, 0)]
    for t, n in ((2, 100), (3, 128), (4, 129)):
        recs += [unorient(t, 30, 30 + n - 1, 0, n - 1, False, n), unorient(t, 60, 60 + n - 1, 0, n - 1, True, n)]
    c = pc.case(seqs, {0: recs}, [0])
    stats, tables, _ = check(ctx, c, with_par(mask_ends=64, min_depth=1), what="mask 64")
    assert stats[0][:3].tolist() == [6, 2 * (100 + 128 + 129), 2] and tables[0][30 + 64].sum() == 1 and tables[0][60 + 64].sum() == 1


def test_three_thousand_records_on_sixty_letters(ctx):
    """the hot cells: every column of every record falls on 60 positions"""
    rng = np.random.default_rng(94)
    seqs = [pc.rand_seq(rng, 60)] + [pc.rand_seq(rng, int(n)) for n in rng.integers(1, 61, size=8)]
    recs = [pc.identity(seqs, 0)]
    for i in range(3000):
        t = 1 + i % 8
        recs.append(pc.random_record(rng, 60, t, len(seqs[t])) if i % 3 else unorient(t, 0, len(seqs[t]) - 1, 0, len(seqs[t]) - 1, False, len(seqs[t])))
    c = pc.case(seqs, {0: recs}, [0])
    stats, tables, _ = check(ctx, c, PAR, what="3000 on 60")
    assert stats[0][0] == 3000 and tables[0].sum(axis=1).max() >= 1000


def test_one_record_more_than_a_chunk(ctx):
    """chunk + 1 records take two work items whose adds meet in the query's counters"""
    chunk = capi.pileup_chunk_records()
    assert 1 <= chunk <= 1 << 20
    c = pc.depth(chunk + 1)
    assert len(c["rec"]) == chunk + 2
    check(ctx, c, PAR, what="chunk + 1")


def test_small_chunks_slices_and_batches(ctx, bounds, monkeypatch):
    """the same figures and the same site order when a query's records are cut into items of 3, the items and tiles into launches of 5
    and the listed queries into batches of at most 3000 positions (the contig of 4097 letters goes alone)"""
    c, want = bounds
    q = pc.query_lists()
    want_q = model(q, PAR)
    before = capi.pileup_chunk_records()
    monkeypatch.setenv("CDM_PILEUP_CHUNK", "3")
    monkeypatch.setenv("CDM_LAUNCH_SLICE", "5")
    monkeypatch.setenv("CDM_BASES_POSITIONS", "3000")
    assert capi.pileup_chunk_records() == 3
    check(ctx, c, BOUNDS_PAR, want=want, what="boundaries, small switches")
    check(ctx, c, BOUNDS_PAR, queries=[6], want=subset(want, [6]), what="4097 alone")
    check(ctx, q, PAR, want=want_q, what="query_lists, small switches")
    monkeypatch.delenv("CDM_PILEUP_CHUNK")
    monkeypatch.delenv("CDM_LAUNCH_SLICE")
    monkeypatch.delenv("CDM_BASES_POSITIONS")
    assert capi.pileup_chunk_records() == before
    check(ctx, q, PAR, want=want_q, what="query_lists, switches restored")


def random_pars():
    rng = np.random.default_rng(95)
    return [dict(mask_ends=int(rng.choice([0, 1, 5, 64])), min_depth=int(rng.integers(1, 5)), min_alt_count=2, min_alt_percent=int(rng.choice([0, 20, 50]))) for _ in range(200)]


def test_random_sets(ctx):
    """200 random sets, per set a random subset of up to 4 queries in random order and random thresholds"""
    flagged = 0
    for seed, par in enumerate(random_pars()):
        c = pc.random_set(60_000 + seed, max_queries=4)
        flagged += int(check(ctx, c, par, what="seed %d" % seed)[0][:, 7].sum())
    assert flagged > 1_000


def test_refusals(ctx):
    c = pc.one_query_of_40()
    db = ctx.upload_seqs(c["seqs"])
    alns = ctx.upload_alns(db, c["off"], c["rec"])
    for kw, word in ((dict(mask_ends=-1), "mask_ends"), (dict(mask_ends=65), "mask_ends"), (dict(min_depth=0), "min_depth"), (dict(min_alt_count=0), "min_alt_count"),
                     (dict(min_alt_percent=-1), "min_alt_percent"), (dict(min_alt_percent=101), "min_alt_percent")):
        with pytest.raises(capi.CdmError, match="cdm error -3.*" + word):
            ctx.pileup_bases(db, alns, [0], sites=True, **kw)
    for extra in (dict(), dict(counts=True, sites=True)):
        with pytest.raises(capi.CdmError, match="cdm error -3.*query index 8"):
            ctx.pileup_bases(db, alns, [0, len(c["seqs"])], **extra)
        with pytest.raises(capi.CdmError, match="cdm error -3.*listed twice"):
            ctx.pileup_bases(db, alns, [1, 0, 1], **extra)
    stats = ctx.pileup_bases(db, alns, [0], mask_ends=64, min_depth=1, min_alt_count=1, min_alt_percent=100)          # (the handles are fine; the ends of the ranges)
    assert stats[0][:2].tolist() == [9, 126]


def test_a_set_with_the_minus_one_record_is_refused(ctx):
    """a sequence of more than 40 % N scores 0 against itself: cdm_rescore writes its identity record with the coordinates -1, and this
    call refuses the set as the profile and the depth do"""
    from carpedeam_amd import synth
    seqs = synth.generate_strings(300, seed=4, mixed=(40, 120))
    rng = np.random.default_rng(5)
    for i in (3, 77, 150, 299):
        s = list(seqs[i])
        for j in rng.choice(len(s), size=len(s) // 2 + 3, replace=False):
            s[j] = "N"
        seqs[i] = "".join(s)
    db = ctx.upload_seqs(seqs)
    alns = ctx.rescore(db, ctx.kmermatch(db))
    _, rec = alns.download()
    assert (rec["q_start"] == -1).any()                 # (the input does reach the case)
    with pytest.raises(capi.CdmError, match="coordinates -1"):
        ctx.pileup_bases(db, alns, [0])


def test_the_empty_query_list(ctx):
    c = pc.query_lists()
    db, alns = handles(ctx, c)
    stats = ctx.pileup_bases(db, alns, [])
    assert stats.shape == (0, 8) and stats.dtype == np.uint64
    stats, tables, sites = ctx.pileup_bases(db, alns, [], counts=True, sites=True)
    assert stats.shape == (0, 8) and tables == [] and sites.shape == (0,) and sites.dtype == bm.SITE_DTYPE


def test_no_flagged_position_gives_no_array(ctx):
    c = columns_case([("A", (5, 0, 0, 0)), ("C", (0, 5, 0, 0))])
    stats, sites = ctx.pileup_bases(*handles(ctx, c), [0], sites=True)          # (the binding asserts: no records, a NULL array)
    assert stats[0].tolist() == [10, 10, 10, 0, 2, 0, 0, 0] and len(sites) == 0


def test_kernel_time_is_reported(ctx):
    c = pc.depth(64)
    db, alns = handles(ctx, c)
    ctx.pileup_bases(db, alns, c["queries"], sites=True)
    assert ctx.bases_kernel_ms > 0 and ctx.last_kernel_ms(18) < 0


def test_synth2k_reads_through_kmermatch_and_rescore(ctx):
    """every query with at least two records against the model on the downloaded records"""
    keyed = gold("synth2k", "reads")
    db = ctx.upload_keyed_seqdb(keyed)
    seqs = [keyed[k][0].rstrip(b"\n").decode() for k in sorted(keyed)]
    alns = ctx.rescore(db, ctx.kmermatch(db))
    off, rec = alns.download()
    queries = [q for q in range(db.n) if off[q + 1] - off[q] >= 2]
    assert len(queries) > 100
    c = dict(seqs=seqs, ext=[0] * db.n, off=off, rec=rec, queries=queries, min_seq_id=0.0, skip=False)
    par = with_par(mask_ends=2, min_depth=2, min_alt_count=1)
    stats, _, sites = check(ctx, c, par, what="synth2k", h=(db, alns))
    assert stats[:, 0].sum() > 1000 and stats[:, 2].sum() > 1000 and len(sites) > 0
