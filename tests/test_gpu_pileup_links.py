"""cdm_pileup_links on the device against tests/links_model.py: the directed and random sets of tests/linkcases.py with the default and
with small batch, query and chunk switches, statistics only, permuted query lists, the output of cdm_alns_dedup, the empty query list
and the refusals.  Every comparison is between integers and exact."""
import numpy as np
import pytest

import dedup_model
import linkcases as lc
import links_model as lm
import pileup_model
from carpedeam_amd import capi

pytestmark = pytest.mark.gpu

SMALL = {"CDM_LINKS_BATCH": "64", "CDM_LINKS_QUERIES": "2", "CDM_PILEUP_CHUNK": "7"}


@pytest.fixture(scope="module")
def ctx():
    return capi.Ctx(0)


def handles(ctx, c):
    db = ctx.upload_seqs(c["seqs"], ext=c["ext"])
    return db, ctx.upload_alns(db, c["off"], c["rec"])


def params(c, **over):
    p = dict(c["par"])
    p.update(over)
    return p


def model(c, queries=None, **over):
    return lm.links(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"] if queries is None else queries, min_seq_id=c["min_seq_id"], skip=c["skip"], **params(c, **over))


def check(ctx, c, queries=None, want=None, what="", h=None, **over):
    """the device with and without the links against the model, twice: two calls give byte-equal arrays; the input set is untouched"""
    q = c["queries"] if queries is None else queries
    db, alns = h or handles(ctx, c)
    want_stats, want_totals, want_links = want or model(c, q, **over)
    par = capi.LinksParams.default(min_seq_id=c["min_seq_id"], skip_extended_targets=c["skip"], **params(c, **over))
    stats, totals, found = ctx.pileup_links(db, alns, q, par, links=True)
    assert ctx.links_kernel_ms > 0 or not len(q), what
    assert stats.dtype == np.uint64 and stats.shape == (len(q), 6) and totals.dtype == np.uint64 and totals.shape == (5,) and found.dtype == capi.LINK_DTYPE, what
    assert np.array_equal(totals, want_totals), (what, totals.tolist(), want_totals.tolist())
    assert np.array_equal(stats, want_stats), (what, np.argwhere(stats != want_stats)[:5].tolist(), stats[stats != want_stats][:5].tolist(), want_stats[stats != want_stats][:5].tolist())
    assert len(found) == len(want_links), (what, len(found), len(want_links))
    differ = np.flatnonzero(found != want_links)
    assert not len(differ), (what, differ[:3].tolist(), found[differ[:3]].tolist(), want_links[differ[:3]].tolist())
    assert found.tobytes() == want_links.tobytes(), what
    only_stats, only_totals = ctx.pileup_links(db, alns, q, par)                # statistics only
    assert np.array_equal(only_stats, want_stats) and np.array_equal(only_totals, want_totals), what
    again = ctx.pileup_links(db, alns, q, par, links=True)
    assert again[0].tobytes() == stats.tobytes() and again[1].tobytes() == totals.tobytes() and again[2].tobytes() == found.tobytes(), what
    in_off, in_rec = alns.download()
    assert np.array_equal(in_off, c["off"]) and in_rec.tobytes() == c["rec"].tobytes(), what
    return stats, totals, found


def test_the_binding_agrees_with_the_model_on_the_records():
    assert capi.LINK_DTYPE == lm.LINK_DTYPE and capi.ALN_DTYPE == pileup_model.ALN_DTYPE


@pytest.mark.parametrize("name,make", lc.DIRECTED, ids=[n for n, _ in lc.DIRECTED])
def test_directed_cases(ctx, name, make):
    c = make()
    want = model(c)
    assert [tuple(int(k[f]) for f in lm.LINK_DTYPE.names if f != "reserved") for k in want[2]] == c["links"]
    check(ctx, c, want=want, what=name)


@pytest.mark.parametrize("name,make", lc.DIRECTED, ids=[n for n, _ in lc.DIRECTED])
def test_directed_cases_in_small_batches_and_items(ctx, monkeypatch, name, make):
    """batches of at most 64 records and 2 queries, work items of 7 records: a read's end records come from several batches, a link's
    pairs from hundreds of items"""
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


@pytest.mark.parametrize("name,over", [("thresholds", dict(overhang=2)), ("thresholds", dict(anchor=15)), ("thresholds", dict(overhang=4)), ("crowded", dict(max_ends=17)),
                                       ("crowded", dict(max_ends=15)), ("min_reads", dict(min_reads=1)), ("min_reads", dict(min_reads=3)), ("long_links", dict(min_reads=258)),
                                       ("chain", dict(anchor=1024)), ("chain", dict(max_ends=2, min_reads=1))])
def test_the_parameters_one_step_further(ctx, name, over):
    check(ctx, dict(lc.DIRECTED)[name](), what="%s %s" % (name, over), **over)


@pytest.mark.parametrize("group", range(3))
def test_random_sets(ctx, monkeypatch, group):
    """four random sets a test: as drawn, with the query list reversed, with every link returned, and in small batches"""
    for seed in lc.RANDOM_SEEDS[group * 4:group * 4 + 4]:
        c = lc.random_set(seed)
        h = handles(ctx, c)
        want = model(c)
        check(ctx, c, want=want, what="seed %d" % seed, h=h)
        check(ctx, c, queries=c["queries"][::-1], what="seed %d reversed" % seed, h=h)
        check(ctx, c, what="seed %d, min_reads 1" % seed, h=h, min_reads=1)
        for k, v in SMALL.items():
            monkeypatch.setenv(k, v)
        check(ctx, c, want=want, what="seed %d, small switches" % seed, h=h)
        for k in SMALL:
            monkeypatch.delenv(k)


def test_query_orders(ctx, monkeypatch):
    c = lc.four_edges()
    h = handles(ctx, c)
    rng = np.random.default_rng(3)
    lists = [list(range(8)), list(range(7, -1, -1)), [1, 0], [0], [5, 4, 1, 0, 7], [3, 2, 6]] + [[int(x) for x in rng.permutation(8)] for _ in range(3)]
    for q in lists:
        check(ctx, c, queries=q, what=str(q), h=h, min_reads=1)
    for k, v in SMALL.items():
        monkeypatch.setenv(k, v)
    for q in lists:
        check(ctx, c, queries=q, what=str(q) + ", small switches", h=h, min_reads=1)
    c = lc.permuted()
    assert [int(k["forward"]) for k in check(ctx, c, what="permuted")[2]] == [0, 2]


@pytest.mark.parametrize("name,make", [("mode_tie", lc.mode_tie), ("long_links", lc.long_links), ("random_0", lambda: lc.random_set(0)), ("random_3", lambda: lc.random_set(3))],
                         ids=["mode_tie", "long_links", "random_0", "random_3"])
def test_on_the_output_of_alns_dedup(ctx, name, make):
    """the set cdm_alns_dedup returns is a set like any other: the device on the device's set, the model on the model's"""
    c = make()
    db, alns = handles(ctx, c)
    out, dstats = ctx.alns_dedup(db, alns, c["queries"], c["min_seq_id"], c["skip"])
    off, rec, _, want_dstats = dedup_model.dedup(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"], c["min_seq_id"], c["skip"])
    assert np.array_equal(dstats, want_dstats) and int(dstats[:, 2].sum()) > 0, name
    d = dict(c, off=off, rec=rec)
    stats, totals, found = check(ctx, d, what=name + " without duplicates", h=(db, out), min_reads=1)
    before = int(model(c, min_reads=1)[1][3])
    assert int(totals[3]) <= before and (int(totals[3]) < before or name.startswith("random")), name            # (the copies made pairs)


def test_the_empty_query_list_and_the_time(ctx):
    c = lc.four_edges()
    db, alns = handles(ctx, c)
    stats, totals, found = ctx.pileup_links(db, alns, [], links=True)
    assert stats.shape == (0, 6) and totals.tolist() == [0] * 5 and found.shape == (0,) and found.dtype == capi.LINK_DTYPE and ctx.links_kernel_ms == 0
    stats, totals = ctx.pileup_links(db, alns, [])
    assert stats.shape == (0, 6) and totals.tolist() == [0] * 5 and ctx.links_kernel_ms == 0
    ctx.pileup_links(db, alns, c["queries"])
    assert ctx.links_kernel_ms > 0
    # a list without end records, and one without pairs
    assert check(ctx, c, queries=[0], what="one query")[1].tolist() == [2, 0, 0, 0, 0]
    none = lc.build([100, 100], [], 1)
    assert check(ctx, none, what="identity records alone")[1].tolist() == [0] * 5


def test_refusals(ctx):
    c = lc.four_edges()
    db, alns = handles(ctx, c)
    n = len(c["seqs"])
    for links in (False, True):
        with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_links: query index %d" % n):
            ctx.pileup_links(db, alns, [0, n], links=links)
        assert ctx.links_kernel_ms == 0
        with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_links: query index 1 is listed twice"):
            ctx.pileup_links(db, alns, [1, 0, 1], links=links)
        other = ctx.upload_seqs(c["seqs"][:3])
        with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_links: alignment CSR has %d queries, DB has 3" % n):
            ctx.pileup_links(other, alns, [0], links=links)
        for field, values in (("anchor", (0, 1025, -1)), ("overhang", (0, 1025)), ("max_ends", (1, 65)), ("min_reads", (0, 1000001))):
            for v in values:
                with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_links: %s = %d;" % (field, v)):
                    ctx.pileup_links(db, alns, [0, 1], capi.LinksParams.default(**{field: v}), links=links)
                assert ctx.links_kernel_ms == 0
        for field, v in (("anchor", 1), ("anchor", 1024), ("overhang", 1024), ("max_ends", 2), ("max_ends", 64), ("min_reads", 1000000)):
            ctx.pileup_links(db, alns, [0, 1], capi.LinksParams.default(**{field: v}), links=links)
    lib = capi.lib()
    par, ptr, n_links = capi.LinksParams.default(), capi.C.POINTER(capi.Link)(), capi.C.c_uint64(7)
    q, stats, totals = np.zeros(1, np.uint32), np.zeros(6, np.uint64), np.zeros(5, np.uint64)
    p = lambda a: a.ctypes.data_as(capi.C.c_void_p)
    good = [ctx.h, db.h, alns.h, p(q), 1, capi.C.byref(par), p(stats), p(totals), capi.C.byref(ptr), capi.C.byref(n_links)]
    for at in (0, 1, 2, 3, 5, 6, 7, 9):
        args = list(good)
        args[at] = None
        ms = capi.C.c_float(7.0)
        assert lib.cdm_pileup_links(*args, capi.C.byref(ms)) == -3 and ms.value == 0 and not ptr, at
    assert lib.cdm_pileup_links(*good, None) == 0 and n_links.value == 0 and not ptr            # (one query: no link; kernel_ms may be NULL)
    check(ctx, c, what="the handles are fine", h=(db, alns))


def test_an_index_copy_of_the_db_is_refused(ctx):
    c = lc.four_edges()
    db, alns = handles(ctx, c)
    index = ctx.index_copy(db)
    with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_links: the DB holds no letters"):
        ctx.pileup_links(index, alns, [0, 1])
    assert ctx.links_kernel_ms == 0


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
    with pytest.raises(capi.CdmError, match="cdm error -4.*cdm_pileup_links.*coordinates -1"):
        ctx.pileup_links(db, alns, [0, 1])
    assert ctx.links_kernel_ms == 0


def test_a_db_with_a_sequence_of_4_m_letters_is_refused(ctx):
    """an end record holds h in 22 bits and a pair its gap in 23: a DB whose longest sequence has 2^22 letters is refused before anything
    is launched, one of 2^22 - 1 letters is taken - a read of that length between two contigs, with the widest h and gap the fields hold"""
    rng = np.random.default_rng(12)
    long = "".join(rng.choice(list("ACGT"), size=1 << 22))
    contigs = ["".join(rng.choice(list("ACGT"), size=40)) for _ in range(2)]
    for read, ok in ((long, False), (long[:-1], True)):
        seqs = contigs + [read]
        T = len(read)
        db = ctx.upload_seqs(seqs)
        # the read's first 20 letters on the end of contig 0, its last 20 on the start of contig 1: h = T - 20 twice, gap = T - 40
        per = {0: [lc.tail_rec(2, T, 40, "+", T - 20)], 1: [lc.head_rec(2, T, 40, "+", T - 20)]}
        off, rec = pileup_model.csr(3, per)
        alns = ctx.upload_alns(db, off, rec)
        par = capi.LinksParams.default(min_reads=1)
        if ok:
            stats, totals, found = ctx.pileup_links(db, alns, [0, 1], par, links=True)
            want = lm.links(seqs, [0] * 3, off, rec, [0, 1], min_reads=1)
            assert np.array_equal(stats, want[0]) and np.array_equal(totals, want[1]) and found.tobytes() == want[2].tobytes()
            assert found["gap_mode"].tolist() == [T - 40] and T - 40 == (1 << 22) - 41
            stats, totals, found = ctx.pileup_links(db, alns, [1, 0], par, links=True)
            assert found.tobytes() == lm.links(seqs, [0] * 3, off, rec, [1, 0], min_reads=1)[2].tobytes() and found["info"].tolist() == [3]
            continue
        with pytest.raises(capi.CdmError, match="cdm error -4.*cdm_pileup_links: the DB holds a sequence of 4194304 letters"):
            ctx.pileup_links(db, alns, [0, 1], par)
        assert ctx.links_kernel_ms == 0
        stats, totals = ctx.pileup_links(db, alns, [], par)         # no key is built for an empty list
        assert stats.shape == (0, 6) and totals.tolist() == [0] * 5
