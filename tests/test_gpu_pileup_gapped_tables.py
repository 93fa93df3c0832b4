"""cdm_pileup_depth_gapped, cdm_pileup_bases_gapped and cdm_pileup_breaks_gapped on the device against tests/gapped_tables_model.py: the
hand-built records of tests/indelcases.py (62-letter gaps, 65 and 300 records on one place, reverse reads, N letters, clips, an unlisted
and extended target), the same in small batches, items and launches, random record sets with random thresholds, the two properties
(no gapped records: the ungapped call; a single-M record: the ungapped record), the refusals, and the chain kmermatch - rescore -
pileup_gapped - the three calls on the planted reads.  Every comparison is between integers and exact."""
import numpy as np
import pytest

import bases_model as bm
import breaks_model as brm
import gapped_tables_model as gt
import indelcases as ic
import indels_model as im
import pileupcases as pc
from carpedeam_amd import capi
from pileup_model import csr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return capi.Ctx(0)


def handles(ctx, c):
    db = ctx.upload_seqs(c["seqs"], ext=c["ext"])
    return db, ctx.upload_alns(db, c["off"], c["rec"])


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5].tolist())


def same_lists(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        same(g, w, (what, k))


DEFAULT = dict(edge=10, mask_ends=0, min_depth=3, min_alt_count=2, min_alt_percent=20, anchor=3, break_edge=5, min_span=1, min_span_percent=0, min_seq_id=0.0, skip=True)


def model(c, p):
    m = (c["seqs"], c["ext"], c["off"], c["rec"], c["queries"], c["grecs"], c["gops"])
    return dict(depth=gt.depth_stats(*m, p["edge"], p["min_seq_id"], p["skip"]),
                bases=gt.bases(*m, p["mask_ends"], p["min_depth"], p["min_alt_count"], p["min_alt_percent"], p["min_seq_id"], p["skip"]),
                breaks=gt.breaks_stats(*m, p["anchor"], p["break_edge"], p["min_span"], p["min_span_percent"], p["min_seq_id"], p["skip"]))


def check(ctx, c, p, want=None, what="", h=None):
    """the three calls without extras, with each optional output and with both, against the model; -> the model's results"""
    db, alns = h or handles(ctx, c)
    want = want or model(c, p)
    g = (c["grecs"], c["gops"])
    # depth
    a = (db, alns, c["queries"], p["edge"], p["min_seq_id"], p["skip"])
    same(ctx.pileup_depth(*a, gapped=g), want["depth"][0], (what, "depth"))
    stats, tracks = ctx.pileup_depth(*a, track=True, gapped=g)
    same(stats, want["depth"][0], (what, "depth, track"))
    same_lists(tracks, want["depth"][1], (what, "depth track"))
    # base counts
    a = (db, alns, c["queries"], p["mask_ends"], p["min_depth"], p["min_alt_count"], p["min_alt_percent"], p["min_seq_id"], p["skip"])
    ws, wt, wr = want["bases"]
    same(ctx.pileup_bases(*a, gapped=g), ws, (what, "bases"))
    s1, t1 = ctx.pileup_bases(*a, counts=True, gapped=g)
    s2, r2 = ctx.pileup_bases(*a, sites=True, gapped=g)
    s3, t3, r3 = ctx.pileup_bases(*a, counts=True, sites=True, gapped=g)
    for got in (s1, s2, s3):
        same(got, ws, (what, "bases, extras"))
    for got in (t1, t3):
        same_lists(got, wt, (what, "counts"))
    for got in (r2, r3):
        assert got.dtype == capi.SITE_DTYPE and got.shape == wr.shape and np.array_equal(got, wr), (what, "sites", len(got), len(wr))
    # break points
    a = (db, alns, c["queries"], p["anchor"], p["break_edge"], p["min_span"], p["min_span_percent"], p["min_seq_id"], p["skip"])
    ws, wt, wr = want["breaks"]
    same(ctx.pileup_breaks(*a, gapped=g), ws, (what, "breaks"))
    s1, t1 = ctx.pileup_breaks(*a, track=True, gapped=g)
    s2, r2 = ctx.pileup_breaks(*a, breaks=True, gapped=g)
    s3, t3, r3 = ctx.pileup_breaks(*a, track=True, breaks=True, gapped=g)
    for got in (s1, s2, s3):
        same(got, ws, (what, "breaks, extras"))
    for got in (t1, t3):
        same_lists(got, wt, (what, "span track"))
    for got in (r2, r3):
        assert got.dtype == capi.BREAK_DTYPE and got.shape == wr.shape and np.array_equal(got, wr), (what, "break records", got.tolist()[:3], wr.tolist()[:3])
    return want


def test_the_binding_agrees_with_the_models_on_the_records():
    assert capi.SITE_DTYPE == bm.SITE_DTYPE and capi.BREAK_DTYPE == brm.BREAK_DTYPE


@pytest.fixture(scope="module")
def directed():
    c = ic.directed()
    return c, model(c, DEFAULT)


def test_the_directed_case(ctx, directed):
    c, want = directed
    check(ctx, c, DEFAULT, want, "directed")
    assert ctx.depth_kernel_ms > 0 and ctx.bases_kernel_ms > 0 and ctx.breaks_kernel_ms > 0
    # the case is what it is built for: 300 reads on one place, a deleted stretch of 62 letters that reads span, sites and breaks
    depth, span = want["depth"][1][0], want["breaks"][1][0]
    assert int(depth.max()) >= 300 and not depth[200:262].any() and (span[200:263] == 3).all()
    assert len(want["bases"][2]) > 0 and len(want["breaks"][2]) > 0
    assert (depth >= want["bases"][1][0].sum(axis=1)).all() and int(want["depth"][0][0][1]) == int(depth.sum())
    for k in ("bases", "breaks"):
        assert np.array_equal(want[k][0][:, :2], want["depth"][0][:, :2])


def test_the_directed_case_with_masked_ends_and_other_thresholds(ctx, directed):
    c, _ = directed
    h = handles(ctx, c)
    check(ctx, c, dict(DEFAULT, edge=0, mask_ends=3, min_depth=1, min_alt_count=1, min_alt_percent=0, anchor=1, break_edge=1, min_span=2, min_span_percent=40), what="mask 3, anchor 1", h=h)
    check(ctx, c, dict(DEFAULT, edge=300, mask_ends=64, min_depth=4, anchor=16, break_edge=50, min_span=3, skip=False), what="mask 64, anchor 16, extended targets count", h=h)


def test_small_batches_chunks_and_slices(ctx, directed, monkeypatch):
    """the contig of 520 letters alone and the two small ones together in batches of at most 256 cells (depth: one batch of the two
    small; breaks: two planes, every query alone) and 256 positions, the ungapped records in items of 50, the items, tiles and blocks
    in launches of 7"""
    c, want = directed
    monkeypatch.setenv("CDM_DEPTH_CELLS", "256")
    monkeypatch.setenv("CDM_BASES_POSITIONS", "256")
    monkeypatch.setenv("CDM_PILEUP_CHUNK", "50")
    monkeypatch.setenv("CDM_LAUNCH_SLICE", "7")
    assert capi.pileup_chunk_records() == 50
    check(ctx, c, DEFAULT, want, "directed, small switches")
    monkeypatch.setenv("CDM_DEPTH_CELLS", "40")             # every query alone
    monkeypatch.setenv("CDM_BASES_POSITIONS", "40")
    monkeypatch.setenv("CDM_LAUNCH_SLICE", "1")
    check(ctx, c, DEFAULT, want, "directed, a query a batch, an item a launch")
    for name in ("CDM_DEPTH_CELLS", "CDM_BASES_POSITIONS", "CDM_PILEUP_CHUNK", "CDM_LAUNCH_SLICE"):
        monkeypatch.delenv(name)
    assert capi.pileup_chunk_records() != 50
    check(ctx, c, DEFAULT, want, "directed, switches restored")


def test_query_orders_and_subsets(ctx, directed):
    """the listed order turned round and a subset: the records' query field is the index into the list"""
    c, _ = directed
    h = handles(ctx, c)
    for queries in ([3, 2, 0], [2], [3, 0]):
        index = {c["queries"].index(q): k for k, q in enumerate(queries)}
        grecs = c["grecs"][np.isin(c["grecs"]["query"], list(index))].copy()
        grecs["query"] = [index[int(k)] for k in grecs["query"]]
        grecs = grecs[np.argsort(grecs["query"], kind="stable")]
        check(ctx, dict(c, queries=queries, grecs=grecs), DEFAULT, what=str(queries), h=h)


def test_random_sets(ctx):
    rng = np.random.default_rng(5150)
    sites = breaks = rescued = 0
    for seed in range(40):
        c, _ = ic.random_case(40_000 + seed)
        anchor = int(rng.choice([1, 2, 5]))
        p = dict(edge=int(rng.integers(0, 12)), mask_ends=int(rng.choice([0, 3])), min_depth=int(rng.integers(1, 5)), min_alt_count=int(rng.integers(1, 4)),
                 min_alt_percent=int(rng.choice([0, 20, 50, 100])), anchor=anchor, break_edge=anchor + int(rng.integers(0, 8)), min_span=int(rng.integers(1, 4)),
                 min_span_percent=int(rng.choice([0, 30, 100])), min_seq_id=0.0, skip=True)
        want = check(ctx, c, p, what="seed %d %r" % (seed, p))
        sites += len(want["bases"][2]); breaks += len(want["breaks"][2]); rescued += len(c["grecs"])
    assert sites > 50 and breaks > 20 and rescued > 100


def ungapped(ctx, db, alns, queries, p):
    return (ctx.pileup_depth(db, alns, queries, p["edge"], p["min_seq_id"], p["skip"], track=True),
            ctx.pileup_bases(db, alns, queries, p["mask_ends"], p["min_depth"], p["min_alt_count"], p["min_alt_percent"], p["min_seq_id"], p["skip"], counts=True, sites=True),
            ctx.pileup_breaks(db, alns, queries, p["anchor"], p["break_edge"], p["min_span"], p["min_span_percent"], p["min_seq_id"], p["skip"], track=True, breaks=True))


def gapped(ctx, db, alns, queries, p, g):
    return (ctx.pileup_depth(db, alns, queries, p["edge"], p["min_seq_id"], p["skip"], track=True, gapped=g),
            ctx.pileup_bases(db, alns, queries, p["mask_ends"], p["min_depth"], p["min_alt_count"], p["min_alt_percent"], p["min_seq_id"], p["skip"], counts=True, sites=True, gapped=g),
            ctx.pileup_breaks(db, alns, queries, p["anchor"], p["break_edge"], p["min_span"], p["min_span_percent"], p["min_seq_id"], p["skip"], track=True, breaks=True, gapped=g))


def same_results(got, want, what):
    for call, (g, w) in enumerate(zip(got, want)):
        same(g[0], w[0], (what, call, "stats"))
        same_lists(g[1], w[1], (what, call, "per position"))
        if len(g) > 2:
            assert g[2].dtype == w[2].dtype and np.array_equal(g[2], w[2]), (what, call, "records")


NONE = (np.empty(0, capi.GAP_DTYPE), np.empty(0, np.uint32))


def test_without_gapped_records_each_call_is_its_ungapped_counterpart(ctx, directed):
    c, _ = directed
    db, alns = handles(ctx, c)
    same_results(gapped(ctx, db, alns, c["queries"], DEFAULT, NONE), ungapped(ctx, db, alns, c["queries"], DEFAULT), "directed")
    s = pc.random_set(71_000)
    p = dict(DEFAULT, min_seq_id=s["min_seq_id"], skip=s["skip"])
    db, alns = handles(ctx, s)
    want = ungapped(ctx, db, alns, s["queries"], p)
    same_results(gapped(ctx, db, alns, s["queries"], p, NONE), want, "random set")
    assert int(want[0][0][:, 0].sum()) > 100
    # no listed query: CDM_OK and nothing comes back
    got = gapped(ctx, db, alns, [], p, NONE)
    assert got[0][0].shape == (0, 8) and got[0][1] == [] and got[1][2].shape == (0,) and got[2][2].shape == (0,)
    assert ctx.depth_kernel_ms == 0.0 and ctx.bases_kernel_ms == 0.0 and ctx.breaks_kernel_ms == 0.0


@pytest.mark.parametrize("seed", range(4))
def test_half_the_records_as_single_m_records(ctx, seed):
    """each call on a pile-up with every other counted record turned into a gapped record of one M operation equals the ungapped call on
    the whole set"""
    s = pc.random_set(70_000 + seed)
    p = dict(DEFAULT, edge=7, mask_ends=3 * (seed % 2), anchor=(1, 5)[seed % 2], break_edge=6, min_span=2, min_span_percent=30, min_seq_id=s["min_seq_id"], skip=s["skip"])
    off, rec, grecs, gops = gt.single_m(s["seqs"], s["ext"], s["off"], s["rec"], s["queries"], pick=lambda i: i % 2 == 0, min_seq_id=s["min_seq_id"], skip=s["skip"])
    assert len(grecs) > 50 and im.check_records(s["seqs"], s["queries"], grecs, gops) is None
    db = ctx.upload_seqs(s["seqs"], ext=s["ext"])
    whole, rest = ctx.upload_alns(db, s["off"], s["rec"]), ctx.upload_alns(db, off, rec)
    same_results(gapped(ctx, db, rest, s["queries"], p, (grecs, gops)), ungapped(ctx, db, whole, s["queries"], p), "seed %d" % seed)


def test_the_chain_on_the_device(ctx):
    """kmermatch, rescore, pileup_gapped and the three calls over the planted contig and its reads: the model is fed the device's
    alignment set and gapped records.  The rescued reads take the four false breaks away"""
    genome, contig, _ = ic.planted_genome(7)
    reads = [r for _, r, _ in ic.planted_reads(genome, strands="alternate")]
    seqs, ext, queries = [contig] + reads, [1] + [0] * len(reads), [0]
    both = ctx.concat(ctx.upload_seqs([contig]), ctx.upload_seqs(reads), 1, 0)
    hits = ctx.kmermatch(both, capi.KmerParams.reads_default())
    alns = ctx.rescore(both, hits, capi.RescoreParams.default())
    off, rec = alns.download()
    _, grecs, gops, _ = ctx.pileup_gapped(both, hits, alns, queries, capi.GapParams.default(0.0, True), records=True)
    # planted_case: 13 reads a plant carry it at least 20 letters from either end, 53 in all; the device's chain rescues more than half
    assert len(grecs) >= 30 and im.check_records(seqs, queries, grecs, gops) is None
    c = dict(seqs=seqs, ext=ext, off=off, rec=rec, queries=queries, grecs=grecs, gops=gops)
    p = dict(DEFAULT, edge=50, anchor=16, break_edge=50)
    want = check(ctx, c, p, what="planted chain", h=(both, alns))
    plain = ctx.pileup_breaks(both, alns, queries, 16, 50, 1, 0, 0.0, True, breaks=True)
    assert len(plain[1]) >= len(want["breaks"][2]) and int(want["depth"][0][0][5]) > int(ctx.pileup_depth(both, alns, queries, 50, 0.0, True)[0][5])


SEQS, REFUSALS = ic.refusals()


@pytest.fixture(scope="module")
def small(ctx):
    db = ctx.upload_seqs(SEQS)
    off, rec = csr(len(SEQS), {q: [pc.identity(SEQS, q)] for q in range(len(SEQS))})
    return db, ctx.upload_alns(db, off, rec)


@pytest.mark.parametrize("name,queries,recs,words,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_records_that_are_refused(ctx, small, name, queries, recs, words, message):
    """inputs each call must refuse on the host: CDM_ERR_INVALID naming the record under the call's own name, and no kernel has run"""
    g = ic.refusal_arrays(recs, words)
    for call, extras, ms in (("depth", dict(track=True), "depth_kernel_ms"), ("bases", dict(counts=True, sites=True), "bases_kernel_ms"), ("breaks", dict(track=True, breaks=True), "breaks_kernel_ms")):
        for extra in (dict(), extras):
            setattr(ctx, ms, -1.0)
            with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_%s_gapped: gapped %s" % (call, message)):
                getattr(ctx, "pileup_" + call)(*small, queries, gapped=g, **extra)
            assert getattr(ctx, ms) == 0.0


def test_the_record_the_refusals_start_from_passes(ctx, small):
    """pos 5, tstart 2, 10M 2I 10M: the positions 5..24 once each, the boundaries 5 + 3 .. 24 + 1 - 3 at anchor 3"""
    g = ic.refusal_arrays([dict(query=0, target=1, pos=5, span=20, tstart=2, tlen=30, columns=22, n_ops=3, ops=0)], [10 << 2, 2 << 2 | 1, 10 << 2])
    stats, tracks = ctx.pileup_depth(*small, [0], track=True, gapped=g)
    assert stats[0].tolist() == [1, 20, 20, 40, 20, 20, 20, 1] and tracks[0].tolist() == [0] * 5 + [1] * 20 + [0] * 15
    stats, tracks = ctx.pileup_breaks(*small, [0], 3, 3, track=True, gapped=g)
    assert stats[0][:2].tolist() == [1, 20] and tracks[0].tolist() == [0] * 8 + [1] * 15 + [0] * 17
    stats, counts = ctx.pileup_bases(*small, [0], counts=True, gapped=g)
    assert stats[0][:3].tolist() == [1, 20, 20] and counts[0].sum(axis=1).tolist() == [0] * 5 + [1] * 20 + [0] * 15 and not counts[0][:, 4:].any()
    read = SEQS[1][2:12] + SEQS[1][14:24]
    assert [int(np.argmax(row)) for row in counts[0][5:25]] == ["ACGT".index(x) for x in read]


def test_parameters_and_lists_are_refused_under_the_calls_own_names(ctx, small):
    db, alns = small
    with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_depth_gapped: edge = -1"):
        ctx.pileup_depth(db, alns, [0], edge=-1, gapped=NONE)
    with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_bases_gapped: mask_ends = 65"):
        ctx.pileup_bases(db, alns, [0], mask_ends=65, gapped=NONE)
    with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_breaks_gapped: anchor = 0"):
        ctx.pileup_breaks(db, alns, [0], anchor=0, gapped=NONE)
    for call in ("depth", "bases", "breaks"):
        with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_%s_gapped: query index 3" % call):
            getattr(ctx, "pileup_" + call)(db, alns, [0, 3], gapped=NONE)
        with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_%s_gapped: query index 1 is listed twice" % call):
            getattr(ctx, "pileup_" + call)(db, alns, [1, 0, 1], gapped=NONE)
