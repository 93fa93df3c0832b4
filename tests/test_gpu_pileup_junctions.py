"""cdm_pileup_junctions on the device against tests/join_model.py: the directed and random sets of tests/joincases.py with the default and
with small batch, query and chunk switches, subsets of the junctions, the output of cdm_alns_dedup, voters against the links' mode_reads,
the empty lists and the refusals; cdm_pileup_links on the same sets against its own model.  Every comparison is between integers and exact."""
import numpy as np
import pytest

import dedup_model
import join_model as jm
import joincases as jc
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


def par_of(c):
    return capi.LinksParams.default(min_seq_id=c["min_seq_id"], skip_extended_targets=c["skip"], min_reads=1, **jc.link_params(c))


def check(ctx, c, juncs=None, want=None, what="", h=None):
    """the device against the model on results, letters and counts, twice: two calls give byte-equal arrays; the input set is untouched"""
    j = jc.juncs_array(c["juncs"] if juncs is None else juncs)
    db, alns = h or handles(ctx, c)
    want_res, want_letters, want_counts = want or jc.model(c, juncs)
    res, letters, counts = ctx.pileup_junctions(db, alns, c["queries"], j, par_of(c), counts=True)
    assert ctx.junctions_kernel_ms > 0 or not len(j), what
    assert res.dtype == capi.JUNCTION_RES_DTYPE and letters.dtype == np.uint8 and counts.dtype == np.uint32 and counts.shape == (len(letters), 5), what
    differ = np.flatnonzero(res != want_res)
    assert not len(differ), (what, differ[:3].tolist(), res[differ[:3]].tolist(), want_res[differ[:3]].tolist())
    assert res.tobytes() == want_res.tobytes(), what
    assert letters.tobytes() == want_letters.tobytes(), (what, bytes(letters)[:80], bytes(want_letters)[:80])
    assert np.array_equal(counts, want_counts), (what, np.argwhere(counts != want_counts)[:5].tolist())
    again = ctx.pileup_junctions(db, alns, c["queries"], j, par_of(c), counts=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, (res, letters, counts))), what
    only = ctx.pileup_junctions(db, alns, c["queries"], j, par_of(c))         # without the counts
    assert len(only) == 2 and only[0].tobytes() == res.tobytes() and only[1].tobytes() == letters.tobytes(), what
    in_off, in_rec = alns.download()
    assert np.array_equal(in_off, c["off"]) and in_rec.tobytes() == c["rec"].tobytes(), what
    return res, letters, counts


def check_links(ctx, c, h):
    """cdm_pileup_links over the shared end-record stage is still its model's, and a junction made of a link has the link's mode_reads"""
    want = lm.links(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"], min_reads=1, min_seq_id=c["min_seq_id"], skip=c["skip"], **jc.link_params(c))
    stats, totals, found = ctx.pileup_links(h[0], h[1], c["queries"], par_of(c), links=True)
    assert np.array_equal(stats, want[0]) and np.array_equal(totals, want[1]) and found.tobytes() == want[2].tobytes()
    j = np.empty(len(found), capi.JUNCTION_DTYPE)
    for f in ("a", "b", "info"):
        j[f] = found[f]
    j["gap"] = found["gap_mode"]
    res, _ = ctx.pileup_junctions(h[0], h[1], c["queries"], j, par_of(c))
    assert res["voters"].tolist() == found["mode_reads"].tolist()
    return found


def test_the_binding_agrees_with_the_model_on_the_records():
    assert capi.JUNCTION_DTYPE == jm.JUNCTION_DTYPE and capi.JUNCTION_RES_DTYPE == jm.RES_DTYPE
    assert capi.JUNCTION_DTYPE.itemsize == capi.C.sizeof(capi.Junction) == 16 and capi.JUNCTION_RES_DTYPE.itemsize == capi.C.sizeof(capi.JunctionRes) == 40


@pytest.mark.parametrize("name,make", jc.DIRECTED, ids=[n for n, _ in jc.DIRECTED])
def test_directed_cases(ctx, monkeypatch, name, make):
    """as they stand, then in batches of at most 64 records and 2 queries with work items of 7 records"""
    c = make()
    h = handles(ctx, c)
    want = jc.model(c)
    if "want" in c:
        assert [tuple(int(r[f]) for f in ("columns", "matches", "voters", "flags", "fill_len", "fill_min", "fill_n")) for r in want[0]] == c["want"]
    check(ctx, c, want=want, what=name, h=h)
    for subset in c.get("subsets", []):
        check(ctx, c, juncs=[c["juncs"][i] for i in subset], what="%s %s" % (name, subset), h=h)
    check_links(ctx, c, h)
    for k, v in SMALL.items():
        monkeypatch.setenv(k, v)
    assert capi.pileup_chunk_records() == 7
    check(ctx, c, want=want, what=name + ", small switches", h=h)
    check_links(ctx, c, h)


@pytest.mark.parametrize("group", range(3))
def test_random_sets(ctx, monkeypatch, group):
    """four random sets a test: every link as a junction, every second one alone, and in small batches"""
    for seed in jc.RANDOM_SEEDS[group * 4:group * 4 + 4]:
        c = jc.random_set(seed)
        h = handles(ctx, c)
        want = jc.model(c)
        check(ctx, c, want=want, what="seed %d" % seed, h=h)
        check(ctx, c, juncs=c["juncs"][::2], what="seed %d, every second" % seed, h=h)
        check_links(ctx, c, h)
        for k, v in SMALL.items():
            monkeypatch.setenv(k, v)
        check(ctx, c, want=want, what="seed %d, small switches" % seed, h=h)
        for k in SMALL:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("name,make", [("fill_gaps", jc.fill_gaps), ("many_voters", jc.many_voters), ("random_0", lambda: jc.random_set(0))], ids=["fill_gaps", "many_voters", "random_0"])
def test_on_the_output_of_alns_dedup(ctx, name, make):
    """the set cdm_alns_dedup returns is a set like any other: the device on the device's set, the model on the model's"""
    c = make()
    db, alns = handles(ctx, c)
    out, _ = ctx.alns_dedup(db, alns, c["queries"], c["min_seq_id"], c["skip"])
    off, rec, _, _ = dedup_model.dedup(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"], c["min_seq_id"], c["skip"])
    d = dict(c, off=off, rec=rec)
    res = check(ctx, d, what=name + " without duplicates", h=(db, out))[0]
    assert int(res["voters"].sum()) <= int(jc.model(c)[0]["voters"].sum())


def test_empty_lists(ctx):
    c = jc.fill_gaps()
    db, alns = handles(ctx, c)
    res, letters, counts = ctx.pileup_junctions(db, alns, c["queries"], jc.juncs_array([]), counts=True)
    assert len(res) == 0 and len(letters) == 0 and counts.shape == (0, 5) and ctx.junctions_kernel_ms == 0
    res, letters = ctx.pileup_junctions(db, alns, [], jc.juncs_array([]))
    assert len(res) == 0 and len(letters) == 0 and ctx.junctions_kernel_ms == 0
    none = jc.build(c["seqs"][:2], [])          # identity records alone: no end record, a fill of N
    res, letters, counts = check(ctx, dict(none, juncs=[(0, 1, 0, 3)]), what="no end records")
    assert bytes(letters) == b"NNN" and res["fill_n"].tolist() == [3] and not counts.any()


def test_refusals(ctx):
    """Every refusal of the header with kernel_ms == 0, but three that no test can reach: more than 2^24 listed queries (a DB of more than
    16 M sequences; tests/test_gpu_pileup_links.py leaves the same bound out), 2^32 junctions or more (64 GB of input), and the two
    refusals that come once the records are counted (a query with 2^32 records, 2^32 end records).  The fill bound is held on the refusing
    side alone - 17 fills of 2^22 - 1 letters; that 16 of them stay within 2^26 is arithmetic here: the call would take 1.3 GB of counters."""
    c = jc.fill_gaps()
    db, alns = handles(ctx, c)
    n = len(c["seqs"])
    q = c["queries"]

    def refused(code, text, queries, juncs, par=None, d=db):
        with pytest.raises(capi.CdmError, match="cdm error %d.*cdm_pileup_junctions: %s" % (code, text)):
            ctx.pileup_junctions(d, alns, queries, jc.juncs_array(juncs), par)
        assert ctx.junctions_kernel_ms == 0

    refused(-3, "junction 0 joins list indices 1 and 1", q, [(1, 1, 0, 1)])
    refused(-3, "junction 0 joins list indices 2 and 1", q, [(2, 1, 0, 1)])
    refused(-3, "junction 1 joins list indices 0 and 8", q, [(0, 1, 0, 1), (0, 8, 0, 1)])
    refused(-3, "junction 0 joins list indices 0 and 1", [], [(0, 1, 0, 1)])
    refused(-3, "junction 0 has info = 4", q, [(0, 1, 4, 1)])
    refused(-3, "junction 1 does not follow junction 0", q, [(0, 1, 0, 1), (0, 1, 0, 2)])          # repeated
    refused(-3, "junction 1 does not follow junction 0", q, [(0, 1, 1, 1), (0, 1, 2, 1)])          # (0, -, 1, +) lies behind (0, +, 1, -)
    refused(-3, "junction 2 does not follow junction 1", q, [(0, 1, 0, 1), (2, 3, 0, 1), (1, 2, 0, 1)])
    refused(-3, "query index %d" % n, [0, n], [(0, 1, 0, 1)])
    refused(-3, "query index 1 is listed twice", [1, 0, 1], [(0, 1, 0, 1)])
    refused(-3, "alignment CSR has %d queries, DB has 3" % n, [0, 1], [(0, 1, 0, 1)], d=ctx.upload_seqs(c["seqs"][:3]))
    for field, values in (("anchor", (0, 1025)), ("overhang", (0, 1025)), ("max_ends", (1, 65))):
        for v in values:
            refused(-3, "%s = %d;" % (field, v), q, [(0, 1, 0, 1)], capi.LinksParams.default(**{field: v}))
    ctx.pileup_junctions(db, alns, q, jc.juncs_array([(0, 1, 0, 1)]), capi.LinksParams.default(min_reads=0))         # min_reads is ignored
    refused(-4, "junction 1 has gap = 4194304", q, [(0, 1, 0, 1), (0, 1, 2, 1 << 22)])
    refused(-4, "junction 0 has gap = -4194304", q, [(0, 1, 0, -(1 << 22))])
    edges = [(a, b, oa | ob << 1, (1 << 22) - 1) for a in range(3) for oa in (0, 1) for b in range(a + 1, 4) for ob in (0, 1)]        # ascending
    ctx_ok = 16 * ((1 << 22) - 1)
    assert ctx_ok <= 1 << 26 < ctx_ok + (1 << 22) - 1
    refused(-4, "the junctions ask for %d fill letters" % (17 * ((1 << 22) - 1)), q, edges[:17])
    lib = capi.lib()
    par, lp, cp = capi.LinksParams.default(), capi.C.POINTER(capi.C.c_uint8)(), capi.C.POINTER(capi.C.c_uint32)()
    qa, j, res = np.arange(8, dtype=np.uint32), jc.juncs_array([(0, 1, 0, 1)]), np.zeros(1, capi.JUNCTION_RES_DTYPE)
    p = lambda a: a.ctypes.data_as(capi.C.c_void_p)
    good = [ctx.h, db.h, alns.h, p(qa), 8, capi.C.byref(par), p(j), 1, p(res), capi.C.byref(lp)]
    for at in (0, 1, 2, 3, 5, 6, 8, 9):
        args = list(good)
        args[at] = None
        ms = capi.C.c_float(7.0)
        assert lib.cdm_pileup_junctions(*args, capi.C.byref(cp), capi.C.byref(ms)) == -3 and ms.value == 0 and not lp and not cp, at
    assert lib.cdm_pileup_junctions(*good, None, None) == 0 and bool(lp)           # (counts and kernel_ms may be NULL)
    lib.cdm_junction_free(lp, None)
    check(ctx, c, what="the handles are fine", h=(db, alns))


def test_an_index_copy_and_a_db_with_a_sequence_of_4_m_letters_are_refused(ctx):
    c = jc.fill_gaps()
    db, alns = handles(ctx, c)
    with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_junctions: the DB holds no letters"):
        ctx.pileup_junctions(ctx.index_copy(db), alns, [0, 1], jc.juncs_array([(0, 1, 0, 1)]))
    assert ctx.junctions_kernel_ms == 0
    rng = np.random.default_rng(12)
    seqs = ["".join(rng.choice(list("ACGT"), size=40)) for _ in range(2)] + ["".join(rng.choice(list("ACGT"), size=1 << 22))]
    big = ctx.upload_seqs(seqs)
    T = 1 << 22
    off, rec = pileup_model.csr(3, {0: [lc.tail_rec(2, T, 40, "+", T - 20)], 1: [lc.head_rec(2, T, 40, "+", T - 20)]})
    with pytest.raises(capi.CdmError, match="cdm error -4.*cdm_pileup_junctions: the DB holds a sequence of 4194304 letters"):
        ctx.pileup_junctions(big, ctx.upload_alns(big, off, rec), [0, 1], jc.juncs_array([(0, 1, 0, 1)]))
    assert ctx.junctions_kernel_ms == 0
