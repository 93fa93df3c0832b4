"""cdm_pileup_breaks on the device against tests/breaks_model.py: the directed and random alignment sets of tests/pileupcases.py, directed
sets of its own at the sizes where the marks, the prefix sums, the classification tiles and the emission can go wrong, the refusals, and
the synth2k reads through cdm_kmermatch and cdm_rescore.  Every comparison is between integers and exact."""
import numpy as np
import pytest

import breaks_model as bm
import pileupcases as pc
from carpedeam_amd import capi
from gpuutil import gold
from pileup_model import unorient

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return capi.Ctx(0)


def handles(ctx, c):
    db = ctx.upload_seqs(c["seqs"], ext=c["ext"])
    return db, ctx.upload_alns(db, c["off"], c["rec"])


def model(c, anchor, edge, min_span=1, pct=0, queries=None):
    return bm.breaks_stats(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"] if queries is None else queries, anchor, edge, min_span, pct, c["min_seq_id"], c["skip"])


def check(ctx, c, anchor, edge, min_span=1, pct=0, queries=None, want=None, what="", h=None):
    """the device without extras, with the track, with the records and with both against the model; -> the model's results"""
    q = c["queries"] if queries is None else queries
    db, alns = h or handles(ctx, c)
    want_stats, want_tracks, want_breaks = want or model(c, anchor, edge, min_span, pct, q)
    a = (db, alns, q, anchor, edge, min_span, pct, c["min_seq_id"], c["skip"])
    plain = ctx.pileup_breaks(*a)
    s1, t1 = ctx.pileup_breaks(*a, track=True)
    s2, b2 = ctx.pileup_breaks(*a, breaks=True)
    s3, t3, b3 = ctx.pileup_breaks(*a, track=True, breaks=True)
    tag = (what, anchor, edge, min_span, pct)
    for got in (plain, s1, s2, s3):
        assert got.dtype == np.uint64 and got.shape == (len(q), 8), tag
        assert np.array_equal(got, want_stats), (tag, np.argwhere(got != want_stats)[:5].tolist(), got[got != want_stats][:5].tolist(), want_stats[got != want_stats][:5].tolist())
    for tracks in (t1, t3):
        assert len(tracks) == len(q)
        for k, (g, w) in enumerate(zip(tracks, want_tracks)):
            assert g.dtype == np.uint32 and g.shape == w.shape, (tag, k)
            assert np.array_equal(g, w), (tag, k, np.argwhere(g != w)[:5].tolist())
    for got in (b2, b3):
        assert got.dtype == capi.BREAK_DTYPE and got.shape == want_breaks.shape, (tag, len(got), len(want_breaks))
        assert np.array_equal(got, want_breaks), (tag, [r for r in zip(got.tolist(), want_breaks.tolist()) if r[0] != r[1]][:3])
    return want_stats, want_tracks, want_breaks


def test_the_binding_agrees_with_the_model_on_the_record():
    assert capi.BREAK_DTYPE == bm.BREAK_DTYPE and (capi.BREAK_JOIN, capi.BREAK_GAP) == (bm.JOIN, bm.GAP)


@pytest.mark.parametrize("anchor,edge", [(1, 1), (3, 5)])
@pytest.mark.parametrize("name,make", pc.DIRECTED, ids=[n for n, _ in pc.DIRECTED])
def test_directed_cases(ctx, name, make, anchor, edge):
    c = make()
    h = handles(ctx, c)
    want = check(ctx, c, anchor, edge, what=name, h=h)[0]
    depth = ctx.pileup_depth(h[0], h[1], c["queries"], 0, c["min_seq_id"], c["skip"])
    assert np.array_equal(want[:, :2], depth[:, :2])
    if name == "query_lists":           # the query with only its identity record: one gap over its whole window
        k = c["queries"].index(7)
        n = len(c["seqs"][7])
        assert want[k].tolist() == [0, 0, n + 1 - 2 * edge, n + 1 - 2 * edge, 1, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ directed cases of these kernels
LENGTHS = (1, 2, 2048, 2049, 4097, 8193)        # adjacent contigs; the one of 2049 letters has only its identity record
# With anchor 1 and edge 1 every boundary 1 .. len - 1 is in the window and a read qs..qe spans qs + 1 .. qe.  The contigs of 4097 and of
# 8193 letters carry a full-length read, so with min_span = 2 a boundary is weak exactly where no second read spans it:
WEAK = {4: [(1, 1),                 # the single boundary b = edge
            (63, 64),               # across two waves of a tile
            (100, 101), (103, 103),  # two runs with one boundary between them
            (2047, 2049),           # across the tile edge at 2048
            (4096, 4096)],          # the single boundary b = len - edge
        5: [(3000, 5500)]}          # longer than a tile of 2048 boundaries


def boundaries():
    """sequences 0..5: the contigs; behind them one target per read.  Contig 0: a read of one letter.  Contig 1: the full-length read.
    Contig 2: two reads that leave the positions 1000..1099 without a read.  Contigs 4 and 5: the full-length read, ending on the last
    letter (its -1 of the span plane lands on the closing cell at anchor 1), and short reads over every stretch between the WEAK runs;
    contig 5 also four reads of 20 letters on one place, which span nothing at anchor 16"""
    rng = np.random.default_rng(91)
    seqs = [pc.rand_seq(rng, n, 0.01) for n in LENGTHS]
    per = {q: [pc.identity(seqs, q)] for q in range(len(LENGTHS))}

    def read(q, qs, qe, rev=False):
        n = qe - qs + 1
        seqs.append(pc.rand_seq(rng, n))
        per[q].append(unorient(len(seqs) - 1, qs, qe, 0, n - 1, rev and n > 1, n))

    read(0, 0, 0)
    read(1, 0, 1)
    read(2, 0, 999)
    read(2, 1100, 2047, rev=True)
    for q, runs in WEAK.items():
        n = LENGTHS[q]
        read(q, 0, n - 1)
        at = 1                                      # the next boundary to be spanned a second time
        for first, last in runs + [(n, n)]:
            if first > at:
                read(q, at - 1, first - 1, rev=(first % 2 == 0))          # spans at .. first - 1
            at = last + 1
    for _ in range(4):              # depth 6, span 2 at anchor 16: weak by the percent rule alone
        read(5, 6000, 6019)
    return pc.case(seqs, per, list(range(len(LENGTHS))))


PARAMS = [(1, 1, 2, 0), (1, 1, 1, 0), (1, 1, 1, 50), (1, 1, 2, 100), (3, 5, 1, 0), (16, 50, 1, 50)]        # anchor, edge, min_span, min_span_percent


@pytest.fixture(scope="module")
def bounds():
    c = boundaries()
    return c, {p: model(c, *p) for p in PARAMS}


@pytest.mark.parametrize("par", PARAMS, ids=["a%d_e%d_s%d_p%d" % p for p in PARAMS])
def test_adjacent_contigs_around_the_tile_sizes(ctx, bounds, par):
    c, want = bounds
    stats, tracks, breaks = check(ctx, c, *par, want=want[par], what="boundaries")
    if par == (1, 1, 2, 0):
        for q, runs in WEAK.items():        # (the input does reach the cases: exactly the planned runs, all joins)
            mine = breaks[breaks["query"] == q]
            assert [(int(b["first"]), int(b["last"])) for b in mine] == runs and (mine["flags"] == bm.JOIN).all() and (mine["min_span"] == 1).all()
        assert stats[0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
        assert stats[1].tolist() == [1, 2, 1, 1, 1, 1, 1, 1]
        assert [tuple(int(x) for x in b) for b in breaks[breaks["query"] == 2]] == [(2, 1, 2047, 0, 100, 1, 1, bm.GAP)]
        assert [tuple(int(x) for x in b) for b in breaks[breaks["query"] == 3]] == [(3, 1, 2048, 0, 2047, 0, 0, bm.GAP)]       # nothing leaks in from the neighbours
        assert tracks[4][4096] == 1 and tracks[5][8192] == 2 and tracks[5][0] == 0
    if par == (16, 50, 1, 50):
        assert [tuple(int(x) for x in b)[1:] for b in breaks[breaks["query"] == 5]] == [(6001, 6019, 2, 0, 6, 6, bm.JOIN)]
    if par == (1, 1, 1, 0):
        assert stats[:, 4].tolist() == [0, 0, 1, 1, 0, 0] and stats[4].tolist()[2:4] == [4096, 0]
        assert [tuple(int(x) for x in b) for b in breaks[breaks["query"] == 2]] == [(2, 1000, 1100, 0, 100, 1, 1, bm.GAP)]


def test_query_orders_and_subsets(ctx, bounds):
    c, want = bounds
    h = handles(ctx, c)
    par = PARAMS[0]
    n = len(LENGTHS)
    for q in (list(range(n))[::-1], [3, 0, 5, 1, 4, 2], [5, 2], [4], [3]):
        check(ctx, c, *par, queries=q, what=str(q), h=h)


def test_small_chunks_slices_and_batches(ctx, bounds, monkeypatch):
    """the same results when a query's records are cut into items of 3, the items and tiles into launches of 5, and the listed queries
    into batches of at most 5000 cells over both planes (the contigs of 4097 and of 8193 letters go alone); the records come in listed
    order across the batches"""
    c, want = bounds
    q = pc.query_lists()
    want_q = model(q, 3, 5, 2, 50)
    before = capi.pileup_chunk_records()
    monkeypatch.setenv("CDM_PILEUP_CHUNK", "3")
    monkeypatch.setenv("CDM_LAUNCH_SLICE", "5")
    monkeypatch.setenv("CDM_DEPTH_CELLS", "5000")
    assert capi.pileup_chunk_records() == 3
    for par in (PARAMS[0], PARAMS[3], PARAMS[4]):
        breaks = check(ctx, c, *par, want=want[par], what="boundaries, small switches")[2]
        assert len(set(breaks["query"].tolist())) >= (4 if par == PARAMS[0] else 2)          # (records of several batches)
        order = [(int(b["query"]), int(b["first"])) for b in breaks]
        assert order == sorted(order) and len(set(order)) == len(order)
    check(ctx, c, *PARAMS[0], queries=[5, 3, 4], what="8193 first, small switches")
    check(ctx, q, 3, 5, 2, 50, want=want_q, what="query_lists, small switches")
    monkeypatch.delenv("CDM_PILEUP_CHUNK")
    monkeypatch.delenv("CDM_LAUNCH_SLICE")
    monkeypatch.delenv("CDM_DEPTH_CELLS")
    assert capi.pileup_chunk_records() == before
    check(ctx, q, 3, 5, 2, 50, want=want_q, what="query_lists, switches restored")


def test_one_record_more_than_a_chunk(ctx):
    """chunk + 1 records take two work items whose marks meet in the query's cells"""
    chunk = capi.pileup_chunk_records()
    c = pc.depth(chunk + 1)
    check(ctx, c, 3, 5, 200, 50, what="chunk + 1")


def test_random_sets(ctx):
    """120 random sets, (anchor, edge) in turn (1, 1) and (3, 5), min_span 1..3, min_span_percent of 0, 50, 100; per set a random subset
    of up to 4 queries in random order"""
    rng = np.random.default_rng(92)
    counted = runs = joins = 0
    for seed in range(120):
        c = pc.random_set(50_000 + seed, max_queries=4)
        anchor, edge = ((1, 1), (3, 5))[seed % 2]
        stats = check(ctx, c, anchor, edge, int(rng.integers(1, 4)), int(rng.choice([0, 50, 100])), what="seed %d" % seed)[0]
        counted += int(stats[:, 0].sum()); runs += int(stats[:, 4].sum()); joins += int(stats[:, 5].sum())
    assert counted > 5_000 and runs > 100 and 0 < joins < runs


def test_refusals(ctx):
    c = pc.one_query_of_40()
    db = ctx.upload_seqs(c["seqs"])
    alns = ctx.upload_alns(db, c["off"], c["rec"])
    bad = [(dict(anchor=0), "anchor"), (dict(anchor=1025, edge=2000), "anchor"), (dict(anchor=16, edge=15), "edge"), (dict(edge=1048577), "edge"),
           (dict(min_span=0), "min_span"), (dict(min_span=1000001), "min_span"), (dict(min_span_percent=-1), "min_span_percent"), (dict(min_span_percent=101), "min_span_percent")]
    for kw, word in bad:
        with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_breaks: %s = " % word):
            ctx.pileup_breaks(db, alns, [0], breaks=True, **kw)
    for extra in (dict(), dict(track=True), dict(breaks=True)):
        with pytest.raises(capi.CdmError, match="cdm error -3.*query index 8"):
            ctx.pileup_breaks(db, alns, [0, len(c["seqs"])], **extra)
        with pytest.raises(capi.CdmError, match="cdm error -3.*listed twice"):
            ctx.pileup_breaks(db, alns, [1, 0, 1], **extra)
    other = ctx.upload_seqs(c["seqs"][:3])
    with pytest.raises(capi.CdmError, match="cdm error -3.*alignment CSR has 8 queries, DB has 3"):
        ctx.pileup_breaks(other, alns, [0])
    # (the handles are fine; the ends of the ranges)
    want = bm.breaks_stats(c["seqs"], c["ext"], c["off"], c["rec"], [0], 1024, 1048576, 1000000, 100)[0]
    assert np.array_equal(ctx.pileup_breaks(db, alns, [0], 1024, 1048576, 1000000, 100), want) and want[0].tolist() == [9, 126, 0, 0, 0, 0, 0, 0]
    want = bm.breaks_stats(c["seqs"], c["ext"], c["off"], c["rec"], [0], 1, 1, 1, 0)[0]
    assert np.array_equal(ctx.pileup_breaks(db, alns, [0], 1, 1, 1, 0), want) and want[0][2] == 39


def test_a_set_with_the_minus_one_record_is_refused(ctx):
    """a sequence of more than 40 % N scores 0 against itself: cdm_rescore writes its identity record with the coordinates -1, and the
    break points refuse the set as the depth does"""
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
    with pytest.raises(capi.CdmError, match="cdm_pileup_breaks.*coordinates -1"):
        ctx.pileup_breaks(db, alns, [0])


def test_the_empty_query_list(ctx):
    c = pc.query_lists()
    db, alns = handles(ctx, c)
    stats = ctx.pileup_breaks(db, alns, [])
    assert stats.shape == (0, 8) and stats.dtype == np.uint64
    stats, tracks, breaks = ctx.pileup_breaks(db, alns, [], track=True, breaks=True)
    assert stats.shape == (0, 8) and tracks == [] and breaks.shape == (0,) and breaks.dtype == capi.BREAK_DTYPE


def test_no_break_gives_no_records_and_the_time_is_reported(ctx):
    c = pc.one_query_of_40()
    db, alns = handles(ctx, c)
    stats, breaks = ctx.pileup_breaks(db, alns, [0], 1, 12, 1, 0, breaks=True)          # (the binding asserts: no records, a NULL array)
    assert stats[0][4] == 0 and stats[0][2] == 17 and stats[0][6] >= 1 and len(breaks) == 0
    assert ctx.breaks_kernel_ms > 0


def test_synth2k_reads_through_kmermatch_and_rescore(ctx):
    """every query with at least two records against the model on the downloaded records"""
    keyed = gold("synth2k", "reads")
    db = ctx.upload_keyed_seqdb(keyed)
    seqs = [keyed[k][0].rstrip(b"\n").decode() for k in sorted(keyed)]
    alns = ctx.rescore(db, ctx.kmermatch(db))
    off, rec = alns.download()
    queries = [q for q in range(db.n) if off[q + 1] - off[q] >= 2]
    assert len(queries) > 100
    want_stats, want_tracks, want_breaks = bm.breaks_stats(seqs, [0] * db.n, off, rec, queries, 8, 10, 2, 50)
    stats, tracks, breaks = ctx.pileup_breaks(db, alns, queries, 8, 10, 2, 50, track=True, breaks=True)
    assert np.array_equal(stats, want_stats)
    assert all(np.array_equal(g, w) for g, w in zip(tracks, want_tracks))
    assert np.array_equal(breaks, want_breaks)
    depth = ctx.pileup_depth(db, alns, queries, edge=0)
    assert np.array_equal(stats[:, :2], depth[:, :2])
    assert want_stats[:, 0].sum() > 1000 and want_stats[:, 7].sum() > 1000 and len(want_breaks) > 10
