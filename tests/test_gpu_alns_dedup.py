"""cdm_alns_dedup on the device against tests/dedup_model.py: the directed and random sets of tests/dedupcases.py with the default and with
small batch, query and chunk switches, permuted query lists, idempotence, the purine/pyrimidine counts, the reductions on the new set,
the empty query list and the refusals.  Every comparison is between integers and exact."""
import numpy as np
import pytest

import dedup_model as dm
import dedupcases as dc
import depth_model
import map_model
import pileup_model
import pileupcases as pc
from carpedeam_amd import capi

pytestmark = pytest.mark.gpu

SMALL = {"CDM_DEDUP_BATCH": "64", "CDM_DEDUP_QUERIES": "2", "CDM_PILEUP_CHUNK": "7"}


@pytest.fixture(scope="module")
def ctx():
    return capi.Ctx(0)


def handles(ctx, c):
    db = ctx.upload_seqs(c["seqs"], ext=c["ext"])
    return db, ctx.upload_alns(db, c["off"], c["rec"])


def model(c, queries=None):
    return dm.dedup(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"] if queries is None else queries, c["min_seq_id"], c["skip"])


def check(ctx, c, queries=None, want=None, what="", h=None):
    """the device with and without the keep flags against the model, then the device once more on its own output; -> the new set"""
    q = c["queries"] if queries is None else queries
    db, alns = h or handles(ctx, c)
    want_off, want_rec, want_keep, want_stats = want or model(c, q)
    out, stats, keep = ctx.alns_dedup(db, alns, q, c["min_seq_id"], c["skip"], keep=True)
    _, plain = ctx.alns_dedup(db, alns, q, c["min_seq_id"], c["skip"])
    for got in (stats, plain):
        assert got.dtype == np.uint64 and got.shape == (len(q), 4), what
        assert np.array_equal(got, want_stats), (what, np.argwhere(got != want_stats)[:5].tolist(), got[got != want_stats][:5].tolist(), want_stats[got != want_stats][:5].tolist())
    assert keep.dtype == np.uint8 and np.array_equal(keep, want_keep), (what, np.flatnonzero(keep != want_keep)[:5].tolist())
    off, rec = out.download()
    assert np.array_equal(off, want_off), (what, np.flatnonzero(off != want_off)[:5].tolist())
    assert rec.shape == want_rec.shape and rec.tobytes() == want_rec.tobytes(), what
    in_off, in_rec = alns.download()                # the input is untouched
    assert np.array_equal(in_off, c["off"]) and in_rec.tobytes() == c["rec"].tobytes(), what
    again, stats2, keep2 = ctx.alns_dedup(db, out, q, c["min_seq_id"], c["skip"], keep=True)
    off2, rec2 = again.download()
    assert np.array_equal(off2, off) and rec2.tobytes() == rec.tobytes() and keep2.all() and (stats2[:, 2] == 0).all() and np.array_equal(stats2[:, 0], stats[:, 1]), what
    return out


def test_the_binding_agrees_with_the_model_on_the_record():
    assert capi.ALN_DTYPE == pileup_model.ALN_DTYPE


@pytest.mark.parametrize("name,make", dc.DIRECTED, ids=[n for n, _ in dc.DIRECTED])
def test_directed_cases(ctx, name, make):
    c = make()
    want = model(c)
    if "keep" in c:
        assert want[2].tolist() == c["keep"]
    check(ctx, c, want=want, what=name)


@pytest.mark.parametrize("name,make", dc.DIRECTED, ids=[n for n, _ in dc.DIRECTED])
def test_directed_cases_in_small_batches_and_items(ctx, monkeypatch, name, make):
    """batches of at most 64 records and 2 queries, work items of 7 records: a long run crosses hundreds of items, and a query beyond the
    record bound goes alone"""
    c = make()
    want = model(c)
    before = capi.pileup_chunk_records()
    for k, v in SMALL.items():
        monkeypatch.setenv(k, v)
    assert capi.pileup_chunk_records() == 7
    check(ctx, c, want=want, what=name + ", small switches")
    for k in SMALL:
        monkeypatch.delenv(k)
    assert capi.pileup_chunk_records() == before
    check(ctx, c, want=want, what=name + ", switches restored")


def test_a_set_without_duplicates_comes_back_equal(ctx):
    c = pc.one_query_of_40()
    out = check(ctx, c, what="one_query_of_40")
    off, rec = out.download()
    assert np.array_equal(off, c["off"]) and rec.tobytes() == c["rec"].tobytes()


@pytest.mark.parametrize("group", range(4))
def test_random_sets(ctx, monkeypatch, group):
    """ten random sets a test: as drawn, with the query list reversed, and in small batches"""
    for seed in dc.RANDOM_SEEDS[group * 10:group * 10 + 10]:
        c = dc.random_set(seed)
        h = handles(ctx, c)
        want = model(c)
        check(ctx, c, want=want, what="seed %d" % seed, h=h)
        check(ctx, c, queries=c["queries"][::-1], what="seed %d reversed" % seed, h=h)
        for k, v in SMALL.items():
            monkeypatch.setenv(k, v)
        check(ctx, c, want=want, what="seed %d, small switches" % seed, h=h)
        for k in SMALL:
            monkeypatch.delenv(k)


def test_query_orders(ctx, monkeypatch):
    c = dc.query_lists()
    h = handles(ctx, c)
    lists = ([4, 11, 7, 29, 3, 17], [7], [11], [29, 7, 3], list(range(30)), list(range(29, -1, -1)))
    for q in lists:
        check(ctx, c, queries=q, what=str(q), h=h)
    for k, v in SMALL.items():
        monkeypatch.setenv(k, v)
    for q in lists:
        check(ctx, c, queries=q, what=str(q) + ", small switches", h=h)


def test_the_ry_counts_follow_their_records(ctx):
    """a set made by cdm_rescore on a small corpus with planted copies: the new set's counts are the input's at the kept records; an
    uploaded set has none before and none afterwards"""
    from carpedeam_amd import synth
    seqs = synth.generate_strings(400, seed=11, mixed=(40, 120))
    seqs += seqs[:150] + seqs[50:120]           # exact copies: every record of a copy on a longer sequence has a twin
    db = ctx.upload_seqs(seqs)
    alns = ctx.rescore(db, ctx.kmermatch(db))
    off, rec = alns.download()
    ry = alns.download_ry()
    q = list(range(len(seqs)))
    out, stats, keep = ctx.alns_dedup(db, alns, q, keep=True)
    want_off, want_rec, want_keep, want_stats = dm.dedup(seqs, [0] * len(seqs), off, rec, q)
    print("records", len(rec), "removed", int(stats[:, 2].sum()))
    assert stats[:, 2].sum() > 10 and (ry != 0xFFFF).any()          # (220 copies planted: a corpus whose copies make no group shows nothing)
    assert np.array_equal(keep, want_keep) and np.array_equal(stats, want_stats)
    got_off, got_rec = out.download()
    assert np.array_equal(got_off, want_off) and got_rec.tobytes() == want_rec.tobytes()
    assert np.array_equal(out.download_ry(), ry[keep == 1])
    empty, _ = ctx.alns_dedup(db, alns, [])
    assert np.array_equal(empty.download_ry(), ry)
    uploaded = ctx.upload_alns(db, off, rec)
    for queries in (q, []):
        plain, _ = ctx.alns_dedup(db, uploaded, queries)
        with pytest.raises(capi.CdmError, match="carries no purine/pyrimidine counts"):
            plain.download_ry()


@pytest.mark.parametrize("name,make", [("overhang", dc.overhang), ("not_counted_skip", lambda: dc.not_counted(True)), ("query_lists", dc.query_lists), ("random_3", lambda: dc.random_set(3)),
                                       ("random_8", lambda: dc.random_set(8))], ids=["overhang", "not_counted_skip", "query_lists", "random_3", "random_8"])
def test_the_reductions_on_the_new_set(ctx, name, make):
    """cdm_pileup_depth, cdm_pileup_profile and cdm_pileup_map on the device's output against their models on the model's output"""
    c = make()
    db, alns = handles(ctx, c)
    out, _ = ctx.alns_dedup(db, alns, c["queries"], c["min_seq_id"], c["skip"])
    off, rec, _, _ = model(c)
    args = (c["seqs"], c["ext"], off, rec, c["queries"])
    assert np.array_equal(ctx.pileup_depth(db, out, c["queries"], 0, c["min_seq_id"], c["skip"]), depth_model.depth_stats(*args, 0, c["min_seq_id"], c["skip"])[0]), name
    counts, reads, cols = ctx.pileup_profile(db, out, c["queries"], 16, c["min_seq_id"], c["skip"])
    want = pileup_model.profile(*args, 16, c["min_seq_id"], c["skip"])
    assert np.array_equal(counts, want[0]) and np.array_equal(reads, want[1]) and np.array_equal(cols, want[2]), name
    stats, recs, mism = ctx.pileup_map(db, out, c["queries"], c["min_seq_id"], c["skip"], records=True)
    want = map_model.map_records(*args, c["min_seq_id"], c["skip"])
    assert np.array_equal(stats, want[0]) and np.array_equal(recs, want[1]) and np.array_equal(mism, want[2]), name


def test_the_empty_query_list_and_the_time(ctx):
    c = dc.query_lists()
    db, alns = handles(ctx, c)
    out, stats, keep = ctx.alns_dedup(db, alns, [], keep=True)
    off, rec = out.download()
    assert stats.shape == (0, 4) and stats.dtype == np.uint64 and keep.all() and len(keep) == len(c["rec"])
    assert np.array_equal(off, c["off"]) and rec.tobytes() == c["rec"].tobytes() and ctx.dedup_kernel_ms == 0
    ctx.alns_dedup(db, alns, c["queries"])
    assert ctx.dedup_kernel_ms > 0


def test_refusals(ctx):
    c = dc.group_keys()
    db, alns = handles(ctx, c)
    n = len(c["seqs"])
    for keep in (False, True):
        with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_alns_dedup: query index %d" % n):
            ctx.alns_dedup(db, alns, [0, n], keep=keep)
        assert ctx.dedup_kernel_ms == 0
        with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_alns_dedup: query index 1 is listed twice"):
            ctx.alns_dedup(db, alns, [1, 0, 1], keep=keep)
        other = ctx.upload_seqs(c["seqs"][:3])
        with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_alns_dedup: alignment CSR has %d queries, DB has 3" % n):
            ctx.alns_dedup(other, alns, [0], keep=keep)
        assert ctx.dedup_kernel_ms == 0
    lib = capi.lib()
    par, h = capi.DedupParams(0.0, 0), capi.C.c_void_p()
    q, stats = np.zeros(1, np.uint32), np.zeros(4, np.uint64)
    ptr = lambda a: a.ctypes.data_as(capi.C.c_void_p)
    for args in ((None, db.h, alns.h, ptr(q), 1, capi.C.byref(par), capi.C.byref(h), ptr(stats)), (ctx.h, None, alns.h, ptr(q), 1, capi.C.byref(par), capi.C.byref(h), ptr(stats)),
                 (ctx.h, db.h, None, ptr(q), 1, capi.C.byref(par), capi.C.byref(h), ptr(stats)), (ctx.h, db.h, alns.h, None, 1, capi.C.byref(par), capi.C.byref(h), ptr(stats)),
                 (ctx.h, db.h, alns.h, ptr(q), 1, None, capi.C.byref(h), ptr(stats)), (ctx.h, db.h, alns.h, ptr(q), 1, capi.C.byref(par), None, ptr(stats)),
                 (ctx.h, db.h, alns.h, ptr(q), 1, capi.C.byref(par), capi.C.byref(h), None)):
        ms = capi.C.c_float(7.0)
        assert lib.cdm_alns_dedup(*args, None, capi.C.byref(ms)) == -3 and ms.value == 0 and not h.value
    check(ctx, c, what="the handles are fine", h=(db, alns))


def test_an_index_copy_of_the_db_is_refused(ctx):
    c = dc.group_keys()
    db, alns = handles(ctx, c)
    index = ctx.index_copy(db)
    with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_alns_dedup: the DB holds no letters"):
        ctx.alns_dedup(index, alns, [0])
    assert ctx.dedup_kernel_ms == 0


def test_a_set_with_the_minus_one_record_is_refused(ctx):
    """a sequence of more than 40 % N scores 0 against itself: cdm_rescore writes its identity record with the coordinates -1, and the
    call refuses the set as cdm_pileup_profile does"""
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
    with pytest.raises(capi.CdmError, match="cdm error -4.*cdm_alns_dedup.*coordinates -1"):
        ctx.alns_dedup(db, alns, [0])
    assert ctx.dedup_kernel_ms == 0
    # a NULL argument is CDM_ERR_INVALID whatever the set holds
    q, stats, h, ms = np.zeros(1, np.uint32), np.zeros(4, np.uint64), capi.C.c_void_p(), capi.C.c_float(7.0)
    assert capi.lib().cdm_alns_dedup(ctx.h, db.h, alns.h, q.ctypes.data_as(capi.C.c_void_p), 1, None, capi.C.byref(h), stats.ctypes.data_as(capi.C.c_void_p), None, capi.C.byref(ms)) == -3
    assert ms.value == 0 and not h.value


def test_a_db_with_a_sequence_of_4_m_letters_is_refused(ctx):
    """the group key holds tLen in 22 bits and u in 23: a DB whose longest sequence has 2^22 letters is refused before anything is
    launched (no upload refuses it), one of 2^22 - 1 letters is taken"""
    rng = np.random.default_rng(12)
    long = "".join(rng.choice(list("ACGT"), size=1 << 22))
    for seqs, ok in (([long, "ACGTACGTAC"], False), ([long[:-1], "ACGTACGTAC"], True)):
        db = ctx.upload_seqs(seqs)
        n = len(seqs[0])
        per = {0: [(0, 0, 0, 0, n - 1, 0, n - 1, 1.0), (1, 0, 9, n - 5, n - 1, 0, 4, 1.0), (1, 0, 7, n - 5, n - 1, 0, 4, 1.0)]}
        off, rec = pileup_model.csr(2, per)
        alns = ctx.upload_alns(db, off, rec)
        if ok:          # u = n - 5 uses all 23 bits of its field
            _, stats, keep = ctx.alns_dedup(db, alns, [0], keep=True)
            assert stats.tolist() == [[2, 1, 1, 2]] and keep.tolist() == [1, 1, 0]
            continue
        with pytest.raises(capi.CdmError, match="cdm error -4.*cdm_alns_dedup: the DB holds a sequence of 4194304 letters"):
            ctx.alns_dedup(db, alns, [0])
        assert ctx.dedup_kernel_ms == 0
        copy, stats = ctx.alns_dedup(db, alns, [])          # no key is built for an empty list: the copy
        assert copy.count == 3 and stats.shape == (0, 4)
