"""cdm_pileup_gapped on the device against tests/gapped_model.py through upload_hits / upload_alns: directed hit sets at the sizes and
ties where the rows, the trace, the walk back, the candidate rule and the primary rule can go wrong, the same again in small items,
launches and trace slices, a random corpus from kmermatch + rescore on the device, and the refusals.  Every comparison is between
integers and exact."""
import numpy as np
import pytest

import gapped_model as gm
import map_model as mm
import pileupcases as pc
from carpedeam_amd import capi
from pileup_model import csr, unorient

pytestmark = pytest.mark.gpu

COMP = mm.COMPLEMENT


@pytest.fixture(scope="module")
def ctx():
    return capi.Ctx(0)


class Builder:
    """sequences, a hit CSR and an alignment CSR by query"""

    def __init__(self, contigs):
        self.seqs, self.ext = list(contigs), [1] * len(contigs)
        self.hits, self.recs = {}, {q: [pc.identity(self.seqs, q)] for q in range(len(contigs))}
        for q in range(len(contigs)):
            self.hits[q] = [(q, 2 * len(contigs[q]), 0)]          # the self hit

    def read(self, q, oriented, Df, rev=False, ext=0, record=None):
        """a read whose letters in the contig's orientation are `oriented`, seeded on the contig-forward diagonal Df; record: the
        oriented (qs, qe, ds, de) of an ungapped record the set holds for the pair"""
        t = len(self.seqs)
        self.seqs.append(oriented.translate(COMP)[::-1] if rev else oriented)
        self.ext.append(ext)
        self.hits[q].append((t, -50 if rev else 50, gm.hit_diagonal(Df, len(self.seqs[q]), len(oriented), rev)))
        if record:
            self.recs[q].append(unorient(t, *record, rev, len(oriented)))
        return t

    def case(self, queries, par):
        n = len(self.seqs)
        off = np.zeros(n + 1, np.uint64)
        rows = []
        for q in range(n):
            rows += self.hits.get(q, [])
            off[q + 1] = len(rows)
        aoff, arec = csr(n, self.recs)
        return dict(seqs=self.seqs, ext=self.ext, hoff=off, hits=np.array(rows, capi.HIT_DTYPE), aoff=aoff, arec=arec, queries=list(queries), par=par)


def model(c, align=gm.align_pair):
    return gm.gapped_records(c["seqs"], c["ext"], c["hoff"], c["hits"], c["aoff"], c["arec"], c["queries"], c["par"], align)


def device_params(p):
    return capi.GapParams.default(p.min_seq_id, p.skip, p.band, p.min_columns, p.min_id_permille, p.match, p.mismatch, p.gap_open, p.gap_extend)


def check(ctx, c, want=None, what=""):
    want = want or model(c)
    db = ctx.upload_seqs(c["seqs"], ext=c["ext"])
    hits, alns = ctx.upload_hits(db, c["hoff"], c["hits"]), ctx.upload_alns(db, c["aoff"], c["arec"])
    par = device_params(c["par"])
    plain = ctx.pileup_gapped(db, hits, alns, c["queries"], par)
    stats, recs, ops, words = ctx.pileup_gapped(db, hits, alns, c["queries"], par, records=True)
    for got in (plain, stats):
        assert got.dtype == np.uint64 and got.shape == want[0].shape and np.array_equal(got, want[0]), (what, got.tolist(), want[0].tolist())
    assert recs.dtype == capi.GAP_DTYPE and recs.shape == want[1].shape, (what, len(recs), len(want[1]))
    assert np.array_equal(recs, want[1]), (what, [r for r in zip(recs.tolist(), want[1].tolist()) if r[0] != r[1]][:3])
    assert np.array_equal(ops, want[2]), (what, ops[:20].tolist(), want[2][:20].tolist())
    assert np.array_equal(words, want[3]), (what, np.flatnonzero(words != want[3])[:5].tolist() if words.shape == want[3].shape else (len(words), len(want[3])))
    return want


def other(c):
    return "ACGT"[("ACGT".find(c) + 1) % 4]


def substitute(s, at):
    s = list(s)
    for i in at:
        s[i] = other(s[i])
    return "".join(s)


def directed():
    """two contigs (the second not listed) and the reads of the issue's list; -> (case, {name: target})"""
    rng = np.random.default_rng(20261019)
    C = list(pc.rand_seq(rng, 520))
    C[122] = "N"
    C[300:305] = "AAAAA"
    C[299], C[305] = "C", "G"
    C = "".join(C)
    C2 = pc.rand_seq(rng, 200)
    b = Builder([C, C2])
    B = 8
    t = {}
    rnd = lambda n: pc.rand_seq(rng, n)
    t["ins1"] = b.read(0, C[50:90] + other(C[90]) + C[90:130], 50)
    t["del1"] = b.read(0, C[60:100] + C[101:141], 60, rev=True)
    t["gap3"] = b.read(0, C[130:170] + C[173:215], 130)
    t["two_gaps"] = b.read(0, C[150:180] + other(C[180]) + C[180:215] + C[217:250], 150, rev=True)
    t["del_B"] = b.read(0, C[200:240] + C[240 + B:290 + B], 200)
    t["del_B1"] = b.read(0, C[201:241] + C[241 + B + 1:291 + B + 1], 201)
    t["ins_B"] = b.read(0, C[330:370] + rnd(B) + C[370:420], 330, rev=True)
    t["left"] = b.read(0, rnd(10) + C[0:30] + C[31:70], -10)
    t["left_rev"] = b.read(0, rnd(7) + C[0:25] + other(C[25]) + C[25:60], -7, rev=True)
    t["right"] = b.read(0, C[460:490] + other(C[490]) + C[490:520] + rnd(12), 460)
    t["right_rev"] = b.read(0, C[450:480] + C[482:520] + rnd(5), 450, rev=True)
    r = C[100:121] + "N" + C[122:140] + C[141:165]          # an N over the contig's N, and one of the read's own
    t["n_both"] = b.read(0, r[:30] + "N" + r[31:], 100)
    t["neighbour"] = b.read(0, C[260:320], 262)              # the seed two diagonals off: no gap, XG 0
    t["neighbour_rev"] = b.read(0, C[380:440], 377, rev=True)
    t["has_record"] = b.read(0, C[400:440] + C[441:470], 400, record=(400, 439, 0, 39))
    a = 20
    t["id_at"] = b.read(0, substitute(C[a:a + 25] + C[a + 26:a + 50], (5, 10, 15, 40)), a)           # 45 matches of 49 columns and a deleted letter: 900 permille
    t["id_below"] = b.read(0, substitute(C[a + 200:a + 225] + C[a + 226:a + 250], (5, 10, 15, 35, 40)), a + 200)
    t["cols_at"] = b.read(0, C[70:86] + C[87:103], 70)       # 32 columns
    t["cols_below"] = b.read(0, C[270:286] + C[287:302], 270)
    t["too_long"] = b.read(0, rnd(4097), 3)
    t["flagged"] = b.read(0, C[340:380] + C[381:420], 340, ext=1)
    t["homo_del"] = b.read(0, C[270:300] + "AAAA" + C[305:340], 270)
    t["homo_ins"] = b.read(0, C[272:300] + "AAAAAA" + C[305:338], 272, rev=True)
    t["twice"] = b.read(0, C[10:50] + C[51:90], 10)         # the same read seeded twice: two candidates, one primary
    b.hits[0].append((t["twice"], 50, gm.hit_diagonal(11, len(C), 79, False)))
    t["unlisted"] = b.read(1, C2[20:60] + C2[61:100], 20)
    return b.case([0], gm.Params(skip=True, band=B)), t


@pytest.fixture(scope="module")
def directed_case():
    c, t = directed()
    return c, t, model(c)


def test_the_binding_agrees_with_the_model_on_the_record():
    assert capi.GAP_DTYPE == gm.GAP_DTYPE and (capi.GAP_OP_M, capi.GAP_OP_I, capi.GAP_OP_D) == (gm.OP_M, gm.OP_I, gm.OP_D)


def test_the_model_reaches_the_directed_cases(directed_case):
    """what the inputs are built for, asserted on the model's output before the device is asked"""
    c, t, (stats, recs, ops, words) = directed_case
    by = {}
    for r in recs:
        by.setdefault(int(r["target"]), []).append(r)
    opsof = lambda r: [(int(w) >> 2, int(w) & 3) for w in ops[int(r["ops"]):int(r["ops"]) + int(r["n_ops"])]]
    M, I, D = gm.OP_M, gm.OP_I, gm.OP_D
    assert opsof(by[t["ins1"]][0]) == [(40, M), (1, I), (40, M)] and opsof(by[t["del1"]][0]) == [(40, M), (1, D), (40, M)]
    assert [o for _, o in opsof(by[t["gap3"]][0])] == [M, D, M] and opsof(by[t["gap3"]][0])[1] == (3, D)
    assert sorted(o for _, o in opsof(by[t["two_gaps"]][0])) == [M, M, M, I, D]
    assert (8, D) in opsof(by[t["del_B"]][0]) and (8, I) in opsof(by[t["ins_B"]][0]) and t["del_B1"] not in by
    assert by[t["left"]][0]["tstart"] >= 10 and by[t["left"]][0]["pos"] == 0 and by[t["left_rev"]][0]["tstart"] >= 7
    for name in ("right", "right_rev"):
        r = by[t[name]][0]
        assert r["pos"] + r["span"] == 520 and r["tstart"] + r["columns"] < r["tlen"] and r["n_ops"] == 3
    r = by[t["n_both"]][0]
    w = words[int(r["words"]):int(r["words"]) + int(r["n_words"])]
    assert ((w >> 24) & 15 == 4).any() and ((w >> 28) == 4).any() and ((w >> 28) == gm.DELETED).any()
    assert opsof(by[t["neighbour"]][0]) == [(60, M)] and opsof(by[t["neighbour_rev"]][0]) == [(60, M)] and by[t["neighbour"]][0]["nm"] == 0
    assert t["has_record"] not in by and t["id_at"] in by and t["id_below"] not in by and t["cols_at"] in by and t["cols_below"] not in by
    assert by[t["cols_at"]][0]["columns"] == 32 and t["too_long"] not in by and t["flagged"] not in by and t["unlisted"] not in by
    assert opsof(by[t["homo_del"]][0]) == [(30, M), (1, D), (39, M)] and opsof(by[t["homo_ins"]][0]) == [(28, M), (1, I), (38, M)]
    assert sorted(int(r["flags"]) & gm.SECONDARY for r in by[t["twice"]]) == [0, gm.SECONDARY]
    n_hits = int(c["hoff"][1]) - 1
    assert stats.tolist() == [[n_hits - 3, len(recs), int(sum(gm.gap_letters(ops[int(r["ops"]):int(r["ops"]) + int(r["n_ops"])]) for r in recs)), 1]]
    assert (recs["flags"] & gm.REVERSE).sum() >= 7 and (np.diff(recs["pos"].astype(np.int64)) >= 0).all()


def test_directed_cases(ctx, directed_case):
    c, _, want = directed_case
    check(ctx, c, want, "directed")


def test_the_row_form_of_the_model_gives_the_same_records(directed_case):
    c, _, want = directed_case
    got = model(c, gm.align_rows)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_small_items_launches_and_trace_slices(ctx, directed_case, monkeypatch):
    """hits in items of 3, items in launches of 3, three candidates a launch of the alignment (CDM_LAUNCH_SLICE) and, with the budget of
    one trace slot, one: the trace buffer serves them in turn"""
    c, _, want = directed_case
    monkeypatch.setenv("CDM_PILEUP_CHUNK", "3")
    monkeypatch.setenv("CDM_LAUNCH_SLICE", "3")
    check(ctx, c, want, "small switches")
    monkeypatch.setenv("CDM_GAP_TRACE_BUDGET", "33000")          # 4096 rows of 16 lanes are 32 KB: one candidate a launch
    monkeypatch.delenv("CDM_LAUNCH_SLICE")
    check(ctx, c, want, "one trace slot")
    monkeypatch.setenv("CDM_GAP_TRACE_BUDGET", "200000")
    monkeypatch.setenv("CDM_MAP_BATCH", "5")
    b, t = both_queries()
    check(ctx, b, None, "several batches")
    monkeypatch.delenv("CDM_PILEUP_CHUNK")
    monkeypatch.delenv("CDM_GAP_TRACE_BUDGET")
    monkeypatch.delenv("CDM_MAP_BATCH")
    check(ctx, c, want, "switches restored")


def both_queries():
    """the directed case with both contigs listed, the second first, and a read seeded on both: the primary is chosen over the call"""
    c, t = directed()
    c["queries"] = [1, 0]
    return c, t


def test_two_listed_queries_and_a_read_on_both(ctx):
    rng = np.random.default_rng(5)
    A = pc.rand_seq(rng, 300)
    Bc = pc.rand_seq(rng, 100) + A[100:200] + pc.rand_seq(rng, 60)
    b = Builder([A, Bc])
    r = A[110:150] + A[151:190]
    t = b.read(0, r, 110)
    b.hits[1].append((t, 50, gm.hit_diagonal(110, len(Bc), len(r), False)))
    t2 = b.read(1, A[120:160] + "T" + A[160:195], 120, rev=True, record=None)
    b.hits[0].append((t2, -50, gm.hit_diagonal(120, len(A), 76, True)))
    b.recs[0].append(unorient(t2, 120, 159, 0, 39, True, 76))        # its ungapped record on the first contig: the rescued one on the second is secondary
    for queries in ([0, 1], [1, 0], [1]):
        c = b.case(queries, gm.Params(skip=True))
        stats, recs, _, _ = check(ctx, c, None, str(queries))
        if len(queries) == 2:
            assert sorted(recs["target"].tolist()) == [t, t, t2] and sorted((recs["flags"] & gm.SECONDARY).tolist()) == [0, 2, 2]
            assert (recs["flags"][recs["target"] == t2] & gm.SECONDARY).all() and (np.diff(recs["query"].astype(np.int64)) >= 0).all()
        else:
            assert sorted(recs["target"].tolist()) == [t, t2] and not (recs["flags"] & gm.SECONDARY).any()


def test_a_diagonal_that_wraps_the_sixteen_bits(ctx):
    rng = np.random.default_rng(70000)
    C = pc.rand_seq(rng, 70000)
    b = Builder([C])
    t1 = b.read(0, C[66000:66040] + C[66041:66090], 66000)
    t2 = b.read(0, C[65530:65570] + "G" + C[65570:65600], 65530, rev=True)
    t3 = b.read(0, C[69950:69980] + C[69982:70000] + pc.rand_seq(rng, 9), 69950)
    c = b.case([0], gm.Params(skip=True))
    assert int(c["hits"][1]["diagonal"]) == 66000 - 65536
    stats, recs, _, _ = check(ctx, c, None, "wrap")
    assert recs["target"].tolist() == [t2, t1, t3] and recs["pos"].tolist() == [65530, 66000, 69950] and stats[0].tolist() == [3, 3, 4, 0]


@pytest.mark.parametrize("B", [7, 8, 15, 16, 31])
def test_every_group_width_and_row_counts_around_the_wave(ctx, B):
    """reads of 1, 63, 64, 65 and 130 letters, each with a gap where it has room for one: G = 16 (band 7), 32 (8, 15) and 64 (16, 31),
    rows on either side of 64 and of the eight rows a trace word holds"""
    rng = np.random.default_rng(100 + B)
    C = pc.rand_seq(rng, 700)
    b = Builder([C])
    at = 20
    for i, L in enumerate((1, 63, 64, 65, 130)):
        g = min(B, 3 + i)
        if L == 1:
            b.read(0, C[at], at)
        elif i % 2:
            b.read(0, C[at:at + L // 2] + C[at + L // 2 + g:at + L + g], at, rev=bool(i & 2))
        else:
            b.read(0, (C[at:at + L // 2] + pc.rand_seq(rng, g) + C[at + L // 2:at + L])[:L], at + (1 if B > 7 else 0), rev=bool(i & 2))
        at += 110
    b.read(0, C[500:560] + C[560 + B:640 + B], 500)      # a deletion of B letters: the band's edge
    c = b.case([0], gm.Params(skip=True, band=B, min_columns=1, min_id_permille=700))
    stats, recs, ops, _ = check(ctx, c, None, "band %d" % B)
    assert len(recs) >= 5 and stats[0][2] >= 10 and (B << 2 | gm.OP_D) in ops.tolist() and 1 in recs["tlen"].tolist()


def test_other_scores_and_a_threshold_of_zero(ctx, directed_case):
    c, _, _ = directed_case
    for par in (gm.Params(skip=True, band=8, min_id_permille=0, min_columns=1), gm.Params(skip=True, band=5, gap_open=3, gap_extend=3, match=1, mismatch=-1),
                gm.Params(skip=False, band=12, min_seq_id=2.0)):
        d = dict(c, par=par)
        stats, recs, _, _ = check(ctx, d, None, "other parameters")
        assert len(recs) >= 15
    # min_seq_id 2: no record counts, so the pair with a record is a candidate too, and the flagged read is one without skip
    assert stats[0][0] == int(c["hoff"][1]) - 2


# ------------------------------------------------------------------------------------------------ a corpus from the device's own stages
def corpus():
    """three contigs and 420 reads of 60..100 letters on both strands; two in five carry one indel of 1..4 letters, one in seven a
    substitution.  Seed 11 was checked on the CPU, with the model on each read's true diagonal in place of the device's hits: about 40
    rescued reads with an insertion and 40 with a deletion on either strand; the test asserts 20 on the model's output for the
    device's own hits"""
    rng = np.random.default_rng(11)
    contigs = [pc.rand_seq(rng, 900) for _ in range(3)]
    reads = []
    for i in range(420):
        c = contigs[i % 3]
        L = int(rng.integers(60, 101))
        at = int(rng.integers(0, len(c) - L - 5))
        r = c[at:at + L + 5]
        kind = i % 5
        if kind in (0, 1):
            g, p = int(rng.integers(1, 5)), int(rng.integers(25, L - 25))
            r = r[:p] + (pc.rand_seq(rng, g) + r[p:] if kind == 0 else r[p + g:])
        r = r[:L]
        if i % 7 == 0:
            r = substitute(r, [int(rng.integers(0, L))])
        reads.append(r.translate(COMP)[::-1] if i % 2 else r)
    return contigs, reads


def test_a_random_corpus_from_kmermatch_and_rescore(ctx):
    contigs, reads = corpus()
    nc = len(contigs)
    seqs, ext = contigs + reads, [1] * nc + [0] * len(reads)
    db = ctx.upload_seqs(seqs, ext=ext)
    hits = ctx.kmermatch(db, capi.KmerParams.reads_default())
    alns = ctx.rescore(db, hits, capi.RescoreParams.default())
    hoff, hrec = hits.download()
    aoff, arec = alns.download()
    p = gm.Params(skip=True)
    queries = list(range(nc))
    want = gm.gapped_records(seqs, ext, hoff, hrec, aoff, arec, queries, p)
    stats, recs, ops, words = want
    kinds = {(rev, op): 0 for rev in (0, 1) for op in (gm.OP_I, gm.OP_D)}
    for r in recs:
        for w in ops[int(r["ops"]):int(r["ops"]) + int(r["n_ops"])]:
            if int(w) & 3:
                kinds[(int(r["flags"]) & gm.REVERSE, int(w) & 3)] += 1
    assert min(kinds.values()) >= 20, kinds
    got = ctx.pileup_gapped(db, hits, alns, queries, device_params(p), records=True)
    for g, w, name in zip(got, want, ("stats", "recs", "ops", "words")):
        assert np.array_equal(g, w), name
    assert ctx.gapped_kernel_ms > 0
    # band 0 of the model on the hits that do have a record is cdm_pileup_map's record (no letter of the corpus is beyond ACGT: the
    # set's trimming on the raw plane plays no part)
    _, mrecs, _ = ctx.pileup_map(db, alns, queries, 0.0, True, records=True)
    by = {(int(r["query"]), int(r["target"])): r for r in mrecs}
    assert len(by) == len(mrecs)
    p0, seen = gm.Params(band=0), 0
    for k, q in enumerate(queries):
        Q = mm.codes(seqs[q])
        for h in range(int(hoff[q]), int(hoff[q + 1])):
            tgt = int(hrec[h]["target"])
            if (k, tgt) not in by:
                continue
            rev = int(hrec[h]["score"]) < 0
            R = gm.oriented_codes(seqs[tgt], rev)
            a, _ = gm.best_alignment(Q, R, int(hrec[h]["diagonal"]), rev, p0)
            d = gm.describe(Q, R, a)
            m = by[(k, tgt)]
            assert (d["pos"], d["columns"], d["tstart"], len(d["words"])) == (int(m["pos"]), int(m["columns"]), int(m["tstart"]), int(m["nm"])), (q, tgt)
            assert bool(int(m["flags"]) & mm.REVERSE) == rev
            seen += 1
    assert seen == len(mrecs) >= 200


def test_refusals(ctx):
    c, _ = directed()
    db = ctx.upload_seqs(c["seqs"], ext=c["ext"])
    hits, alns = ctx.upload_hits(db, c["hoff"], c["hits"]), ctx.upload_alns(db, c["aoff"], c["arec"])
    bad = [dict(band=0), dict(band=32), dict(min_id_permille=1001), dict(match=0), dict(mismatch=0), dict(gap_extend=0), dict(gap_open=1, gap_extend=2)]
    for kw in bad:
        for records in (False, True):
            with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_gapped"):
                ctx.pileup_gapped(db, hits, alns, [0], capi.GapParams.default(**kw), records=records)
    with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_gapped: query index 1 is listed twice"):
        ctx.pileup_gapped(db, hits, alns, [1, 0, 1])
    with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_gapped: query index %d" % len(c["seqs"])):
        ctx.pileup_gapped(db, hits, alns, [len(c["seqs"])])
    small = ctx.upload_seqs(c["seqs"][:3])
    with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_gapped: hit CSR has"):
        ctx.pileup_gapped(small, hits, ctx.upload_alns(small, [0, 0, 0, 0], np.empty(0, capi.ALN_DTYPE)), [0])
    with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_gapped: alignment CSR has"):
        ctx.pileup_gapped(db, hits, ctx.upload_alns(small, [0, 0, 0, 0], np.empty(0, capi.ALN_DTYPE)), [0])
    stats, recs, ops, words = ctx.pileup_gapped(db, hits, alns, [], records=True)
    assert stats.shape == (0, 4) and len(recs) == 0 and len(ops) == 0 and len(words) == 0
    stats, recs, ops, words = ctx.pileup_gapped(db, hits, alns, [5], records=True)        # a read as the query: no hits
    assert stats.tolist() == [[0, 0, 0, 0]] and len(recs) == 0
