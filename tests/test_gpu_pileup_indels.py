"""cdm_pileup_indels on the device against tests/indels_model.py: the hand-built records of tests/indelcases.py at the sizes and ties
where the marks, the event sort, the segment scans, the place pass and the letter vote can go wrong, the same again in small batches,
items and launches, random record sets, the chain kmermatch - rescore - pileup_gapped - pileup_indels on the device, and the refusals.
Every comparison is between integers and exact."""
import numpy as np
import pytest

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


def device_params(p):
    return capi.IndelParams.default(p.min_depth, p.min_count, p.min_percent, p.min_seq_id, p.skip)


def model(c, par, queries=None, grecs=None):
    return im.indels_sorted(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"] if queries is None else queries, c["grecs"] if grecs is None else grecs, c["gops"], par)


def check(ctx, c, par, want=None, what="", h=None):
    """the device without extras, with the track, with the sites and with both against the model; -> the model's results"""
    db, alns = h or handles(ctx, c)
    want = want or model(c, par)
    a = (db, alns, c["queries"], c["grecs"], c["gops"], device_params(par))
    plain = ctx.pileup_indels(*a)
    s1, t1 = ctx.pileup_indels(*a, track=True)
    s2, r2, l2 = ctx.pileup_indels(*a, sites=True)
    s3, t3, r3, l3 = ctx.pileup_indels(*a, track=True, sites=True)
    for got in (plain, s1, s2, s3):
        assert got.dtype == np.uint64 and got.shape == want[0].shape, what
        assert np.array_equal(got, want[0]), (what, np.argwhere(got != want[0])[:5].tolist(), got[got != want[0]][:5].tolist(), want[0][got != want[0]][:5].tolist())
    for tracks in (t1, t3):
        assert len(tracks) == len(want[1])
        for k, (g, w) in enumerate(zip(tracks, want[1])):
            assert g.dtype == np.uint32 and g.shape == w.shape and np.array_equal(g, w), (what, k, np.argwhere(g != w)[:5].tolist())
    for recs, letters in ((r2, l2), (r3, l3)):
        assert recs.dtype == capi.INDEL_DTYPE and recs.shape == want[2].shape, (what, len(recs), len(want[2]))
        assert np.array_equal(recs, want[2]), (what, [r for r in zip(recs.tolist(), want[2].tolist()) if r[0] != r[1]][:3])
        assert letters.dtype == np.uint8 and np.array_equal(letters, want[3]), (what, letters[:40].tolist(), want[3][:40].tolist())
    return want


def test_the_binding_agrees_with_the_model_on_the_record():
    assert capi.INDEL_DTYPE == im.INDEL_DTYPE and capi.INDEL_DTYPE.itemsize == 40
    assert (capi.INDEL_INS, capi.INDEL_DEL, capi.INDEL_CALLED, capi.INDEL_SUPPORTED, capi.INDEL_MAJOR) == (im.INS, im.DEL, im.CALLED, im.SUPPORTED, im.MAJOR)


@pytest.fixture(scope="module")
def directed():
    c = ic.directed()
    par = im.Params(**ic.DIRECTED_PAR)
    return c, par, model(c, par)


def test_the_directed_case(ctx, directed):
    """tests/test_indels_model.py holds the model's answer on this case against the places worked out by hand"""
    c, par, want = directed
    check(ctx, c, par, want, "directed")
    assert ctx.indels_kernel_ms > 0
    assert int(want[0][0][8]) == 11 and len(want[3]) > 62


def test_small_batches_chunks_and_slices(ctx, directed, monkeypatch):
    """the contig of 520 letters alone and the two small ones together in batches of at most 256 cells, the ungapped records in items
    of 50, the items, tiles and blocks in launches of 7"""
    c, par, want = directed
    monkeypatch.setenv("CDM_INDEL_POSITIONS", "256")
    monkeypatch.setenv("CDM_PILEUP_CHUNK", "50")
    monkeypatch.setenv("CDM_LAUNCH_SLICE", "7")
    assert capi.pileup_chunk_records() == 50
    check(ctx, c, par, want, "directed, small switches")
    monkeypatch.setenv("CDM_INDEL_POSITIONS", "40")         # every query alone
    check(ctx, c, par, want, "directed, a query a batch")
    monkeypatch.delenv("CDM_INDEL_POSITIONS")
    monkeypatch.delenv("CDM_PILEUP_CHUNK")
    monkeypatch.delenv("CDM_LAUNCH_SLICE")
    assert capi.pileup_chunk_records() != 50
    check(ctx, c, par, want, "directed, switches restored")


def test_query_orders_and_subsets(ctx, directed):
    """the listed order turned round and a subset: the records' query field is the index into the list"""
    c, par, _ = directed
    h = handles(ctx, c)
    for queries in ([3, 2, 0], [2], [3, 0]):
        index = {c["queries"].index(q): k for k, q in enumerate(queries)}
        grecs = c["grecs"][np.isin(c["grecs"]["query"], list(index))].copy()
        grecs["query"] = [index[int(k)] for k in grecs["query"]]
        grecs = grecs[np.argsort(grecs["query"], kind="stable")]
        d = dict(c, queries=queries, grecs=grecs)
        check(ctx, d, par, what=str(queries), h=h)


def test_no_gapped_records_statistics_only_and_track_only(ctx, directed):
    c, par, want = directed
    h = handles(ctx, c)
    d = dict(c, grecs=c["grecs"][:0], gops=c["gops"][:0])
    none = check(ctx, d, par, what="n_recs == 0", h=h)
    assert len(none[2]) == 0 and not none[0][:, 2:].any() and none[0][0][0] > 20 and int(none[1][0][330]) == 8
    stats = ctx.pileup_indels(*h, c["queries"], c["grecs"], c["gops"], device_params(par))
    assert np.array_equal(stats, want[0])
    stats, tracks = ctx.pileup_indels(*h, c["queries"], c["grecs"], c["gops"], device_params(par), track=True)
    assert np.array_equal(stats, want[0]) and all(np.array_equal(g, w) for g, w in zip(tracks, want[1])) and tracks[0][0] == 0
    stats, tracks, recs, letters = ctx.pileup_indels(*h, [], c["grecs"][:0], c["gops"][:0], track=True, sites=True)
    assert stats.shape == (0, 10) and tracks == [] and recs.shape == (0,) and recs.dtype == capi.INDEL_DTYPE and letters.shape == (0,)


def test_random_sets(ctx):
    sites = letters = 0
    for seed in range(80):
        c, par = ic.random_case(12_000 + seed)
        want = check(ctx, c, par, what="seed %d" % seed)
        sites += len(want[2]); letters += len(want[3])
    assert sites > 100 and letters > 50


def test_the_chain_on_the_device(ctx):
    """kmermatch, rescore, pileup_gapped and pileup_indels on the corpus of tests/test_gpu_contig_gapped_cli.py: the model is fed the
    device's alignment set and gapped records"""
    from test_gpu_contig_gapped_cli import gapped_corpus
    c = gapped_corpus()
    nc = len(c["contigs"])
    seqs, ext = c["contigs"] + c["reads"], [1] * nc + [0] * len(c["reads"])
    both = ctx.concat(ctx.upload_seqs(c["contigs"]), ctx.upload_seqs(c["reads"]), 1, 0)
    hits = ctx.kmermatch(both, capi.KmerParams.reads_default())
    alns = ctx.rescore(both, hits, capi.RescoreParams.default())
    off, rec = alns.download()
    queries = list(range(nc))
    _, grecs, gops, _ = ctx.pileup_gapped(both, hits, alns, queries, capi.GapParams.default(0.0, True), records=True)
    assert len(grecs) >= 60 and im.check_records(seqs, queries, grecs, gops) is None
    for par in (im.Params(skip=True), im.Params(1, 1, 0, 0.0, True)):
        want = im.indels_sorted(seqs, ext, off, rec, queries, grecs, gops, par)
        stats, tracks, sites, letters = ctx.pileup_indels(both, alns, queries, grecs, gops, device_params(par), track=True, sites=True)
        assert np.array_equal(stats, want[0]) and all(np.array_equal(g, w) for g, w in zip(tracks, want[1]))
        assert np.array_equal(sites, want[2]) and np.array_equal(letters, want[3])
    assert len(want[2]) >= 20 and int(want[0][:, 3].sum()) > 10 and int(want[0][:, 4].sum()) > 10
    depth = ctx.pileup_depth(both, alns, queries, 0, 0.0, True)
    assert np.array_equal(stats[:, :2], depth[:, :2])


SEQS, REFUSALS = ic.refusals()


@pytest.fixture(scope="module")
def small(ctx):
    db = ctx.upload_seqs(SEQS)
    off, rec = csr(len(SEQS), {q: [pc.identity(SEQS, q)] for q in range(len(SEQS))})
    return db, ctx.upload_alns(db, off, rec)


@pytest.mark.parametrize("name,queries,recs,words,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_records_that_are_refused(ctx, small, name, queries, recs, words, message):
    """inputs the call must refuse on the host: CDM_ERR_INVALID naming the record, and no kernel has run"""
    grecs, gops = ic.refusal_arrays(recs, words)
    for extra in (dict(), dict(track=True, sites=True)):
        with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_indels: gapped " + message):
            ctx.pileup_indels(*small, queries, grecs, gops, **extra)
        assert ctx.indels_kernel_ms == 0.0


def test_the_record_the_refusals_start_from_passes(ctx, small):
    grecs, gops = ic.refusal_arrays([dict(query=0, target=1, pos=5, span=20, tstart=2, tlen=30, columns=22, n_ops=3, ops=0)], [10 << 2, 2 << 2 | 1, 10 << 2])
    stats, sites, letters = ctx.pileup_indels(*small, [0], grecs, gops, capi.IndelParams.default(1, 1, 0), sites=True)
    assert stats[0].tolist() == [0, 0, 1, 1, 0, 2, 0, 1, 1, 1] and len(sites) == 1 and int(sites[0]["pos"]) == 15 and len(letters) == 2


def test_parameters_and_lists_that_are_refused(ctx, small):
    db, alns = small
    none, no_ops = np.empty(0, capi.GAP_DTYPE), np.empty(0, np.uint32)
    for kw, word in ((dict(min_depth=0), "min_depth"), (dict(min_depth=1000001), "min_depth"), (dict(min_count=0), "min_count"), (dict(min_count=1000001), "min_count"),
                     (dict(min_percent=-1), "min_percent"), (dict(min_percent=101), "min_percent")):
        with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_indels: %s = " % word):
            ctx.pileup_indels(db, alns, [0], none, no_ops, capi.IndelParams.default(**kw), sites=True)
        assert ctx.indels_kernel_ms == 0.0
    with pytest.raises(capi.CdmError, match="cdm error -3.*query index 3"):
        ctx.pileup_indels(db, alns, [0, 3], none, no_ops)
    with pytest.raises(capi.CdmError, match="cdm error -3.*listed twice"):
        ctx.pileup_indels(db, alns, [1, 0, 1], none, no_ops)
    other = ctx.upload_seqs(SEQS[:2])
    with pytest.raises(capi.CdmError, match="cdm error -3.*alignment CSR has 3 queries, DB has 2"):
        ctx.pileup_indels(other, alns, [0], none, no_ops)
    stats = ctx.pileup_indels(db, alns, [0], none, no_ops, capi.IndelParams.default(1000000, 1000000, 100))        # (the ends of the ranges)
    assert stats.tolist() == [[0] * 10]
