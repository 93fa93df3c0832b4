"""The pile-up of k_correct_fast split by damage class (csrc/correct.hip, SPLIT): interior columns counted in registers, the five
columns at each end of a target in the LDS counters with lane = record, records outside the stage through a loop of their own.
Piles built so that every border between the three meets a column on which one count too few or one too many turns the call:

  miss   self record + two records of one layout over a truth of C / G under a query of T / A: T (A) holds 1 of 3, the base is
         called; a column that one record fails to count is 1 of 2 and stays.
  dup    self record + four such records, one of which holds the query's letter: 2 of 5 and the base stays (the 0.4 rule); a
         column counted twice for another record is 2 of 6 and is called.  (Every seventh column of that record holds the truth, so
         that the group has called columns as well.)

Both are filled up to 17 records with records over other columns, so that the 16..64-record instance - the one with the split
loop - takes them under the default settings; CDM_CORRECT_VARIANT=0 sends every pile there.  Every case runs under both loops
(CDM_CORRECT_PILEUP), both pools of that instance, nothing staged and a pile staged in part, against the oracle's
ancient_correction on the same inputs and against what the reference's own object code answered
(tests/golden/correct_pileup_split/, written by tests/golden/make_correct_pileup_split.py)."""
import os

import numpy as np
import pytest

import correctcases as cc
from carpedeam_amd import mmdb
from gpuutil import GOLD, diff_keys, run_oracle, seqdb_to_keyed
from stageflags import A_FLAGS

DIR = os.path.join(GOLD, "correct_pileup_split")
SWITCHES = ("CDM_CORRECT_VARIANT", "CDM_CORRECT_BIGW", "CDM_CORRECT_STAGE_POOL", "CDM_CORRECT_STATS", "CDM_CORRECT_PILEUP", "CDM_CORRECT_GRID")
SETTINGS = [("default", {}), ("variant_0", {"CDM_CORRECT_VARIANT": "0"}), ("bigw_4", {"CDM_CORRECT_BIGW": "4"}),
            ("pool_0", {"CDM_CORRECT_STAGE_POOL": "0"}), ("pool_22", {"CDM_CORRECT_STAGE_POOL": "22"}),
            ("joint", {"CDM_CORRECT_PILEUP": "joint"}), ("split", {"CDM_CORRECT_PILEUP": "split"}),
            ("variant_0_pool_22", {"CDM_CORRECT_VARIANT": "0", "CDM_CORRECT_STAGE_POOL": "22"}),
            ("bigw_4_joint", {"CDM_CORRECT_BIGW": "4", "CDM_CORRECT_PILEUP": "joint"})]
CG = np.frombuffer(b"CG", np.uint8)


def probe_group(S, rs, name, qa, n, ds, tlen, rev, style, qlen=200, fill=None, with_n=False, records=17):
    """self + 2 (miss) or 4 (dup) records over the columns qa .. qa + n - 1 that start at oriented target position ds, every column
    a damage site; `fill`: the columns (first, last) of the records that fill the pile up to `records`, away from the probed ones.
    with_n: the second record's target holds an N off the span (it is not staged)"""
    core = bytes(bytearray(rs.choice(CG, size=qlen)))
    query = cc.damaged(rs, core, rate=1.0)
    q = S.seq(query)
    k = 2 if style == "miss" else 4
    for i in range(k):
        ed = None
        if style == "dup" and i == 1:
            def ed(mid, qa=qa):
                for j in range(len(mid)):
                    if j % 7 != 3:
                        mid[j] = query[qa + j]
        sed = None
        if with_n and i == 0:
            lo = tlen - ds - n if rev else ds                       # the span on the target as stored

            def sed(stored, lo=lo, n=n):
                stored[lo - 1 if lo else lo + n] = ord("N")
        cc.target(S, rs, q, core, qa, qa + n - 1, ds, tlen, rev, edit=ed, stored_edit=sed)
    if fill is None:
        fill = (qlen - 90, qlen - 1) if qa + n <= qlen - 90 else (0, 89)
    for i in range(records - 1 - k):
        assert fill[1] < qa or fill[0] >= qa + n, name
        m = fill[1] - fill[0] + 1
        cc.target(S, rs, q, core, fill[0], fill[1], int(rs.randint(0, 30)), m + 37, i % 2 == 1)
    S.group(name, q, True)
    return q


def build_cases(seed=41):
    rs = np.random.RandomState(seed)
    S = cc.CaseSet()
    rejected = set()

    # ---- class borders: a span of 60 columns that starts at oriented target position 0, 4, 5, 6 or ends at tLen - 7, tLen - 6,
    # tLen - 5, tLen - 1, both strands, both styles; the columns 10 .. 69 sit in both chunks
    for style in ("miss", "dup"):
        for o in "fr":
            for ds in (0, 4, 5, 6):
                probe_group(S, rs, "start_%d_%s_%s" % (ds, o, style), 10, 60, ds, 100, o == "r", style)
            for back in (7, 6, 5, 1):
                probe_group(S, rs, "end_m%d_%s_%s" % (back, o, style), 10, 60, 100 - back - 59, 100, o == "r", style)
            # tLen 30 under a span of 30 (ten end columns, twenty interior); a target of 40 inside the query; the query inside a target
            probe_group(S, rs, "tlen30_%s_%s" % (o, style), 50, 30, 0, 30, o == "r", style)
            probe_group(S, rs, "target_inside_%s_%s" % (o, style), 45, 40, 0, 40, o == "r", style)
            probe_group(S, rs, "query_inside_%s_%s" % (o, style), 0, 100, 50, 200, o == "r", style, qlen=100, fill=None, records=3 if style == "miss" else 5)
            # ---- chunk borders: class 4 on column 63 / 64 (the record starts on column 59 / 60 - with 60 its interior range is
            # empty in the first chunk), class 6 on column 63 / 64 (it ends on column 67 / 68 - with 67 empty in the second)
            for qa in (59, 60):
                probe_group(S, rs, "chunk_start_%d_%s_%s" % (qa, o, style), qa, 60, 0, 100, o == "r", style, fill=(130, 199))
            for qb in (67, 68):
                probe_group(S, rs, "chunk_end_%d_%s_%s" % (qb, o, style), qb - 59, 60, 40, 100, o == "r", style)
            # ---- the three paths on one set of columns: of the records of one layout one has an N in its target (off the span),
            # the others are staged (or past the pool under a small one); and spans of 200 columns (13 words: never staged)
            probe_group(S, rs, "with_n_%s_%s" % (o, style), 10, 60, 3, 100, o == "r", style, with_n=True)
            probe_group(S, rs, "long_%s_%s" % (o, style), 0, 200, 2, 205, o == "r", style, qlen=320, fill=(230, 319))

    # ---- query lengths around the chunk borders, 18 records, both ends of most targets inside the span (tLen = qLen + 7)
    for L in (63, 64, 65, 100, 128, 129):
        for o in "mr":
            cc.pile(S, rs, "qlen_%d_%s" % (L, o), L, 17, o, tlen=L + 7)

    # ---- counts: 15 and 64 records with one letter on every column, all reverse / all forward: the query is the prefix (right-only
    # records: columns 0 .. 4 are classes 0 .. 4) or the suffix (left-only: columns 35 .. 39 are classes 6 .. 10) of every oriented
    # target, no self record.  A field reaches 15 / 64, in the registers and in the counters
    for n in (15, 64):
        for o in "fr":
            for side, ds in (("prefix", 0), ("suffix", 60)):
                core = cc.core_with_probes(rs, 40)
                q = S.seq(cc.damaged(rs, core, force=cc.probe_cols(40)), self_record=False)
                for i in range(n):
                    cc.target(S, rs, q, core, 0, 39, ds, 100, o == "r")
                S.group("sat_%d_%s_%s" % (n, o, side), q, True)
    # forward and reverse on the same columns with different letters: extended queries of 30 T / A over a truth of C / G, of 18 (36)
    # records two (four) hold the damaged letter in a column - the call turns on the class ramps and on the strand of every record
    for gi in range(16):
        mult = (2, 4)[gi % 2]
        n = 9 * mult
        core = bytes(bytearray(rs.choice(CG, size=30)))
        q = S.seq(cc.damaged(rs, core, rate=1.0), 1)
        odd = np.array([rs.permutation(n)[:mult] for _ in range(30)])
        for i in range(n):
            tl = (30, 31, 100, 31, 100)[(i + gi) % 5]
            ds = {30: 0, 31: (i + gi) % 2}.get(tl, (0, 70, 1, 66, 35)[(i + gi // 5) % 5])

            def ed(mid, cols=np.nonzero((odd == i).any(1))[0]):
                for j in cols:
                    mid[j] = cc._DAMAGE[mid[j]]
            cc.target(S, rs, q, core, 0, 29, ds, tl, cc._rev_of("frm"[gi % 3], i), edit=ed, seq_id="0.966")
        S.group("strands_ext_%d_n%d" % (gi, n), q, None)

    # ---- pile sizes at the instances' borders, a rejected record in the middle of the wave
    for n in (2, 15, 16, 64):
        qlen, alen = (40, None) if n < 45 else (64, 32)
        core = cc.core_with_probes(rs, qlen)
        q = S.seq(cc.damaged(rs, core, force=cc.probe_cols(qlen)))
        for i in range(n - 1):
            m = qlen if alen is None else alen
            qa = 0 if i % 2 == 0 else qlen - m
            bad = i == (n - 1) // 2
            t = cc.target(S, rs, q, core, qa, qa + m - 1, int(rs.randint(1, 100 - m)), 100, i % 3 == 1, seq_id="0.899" if bad else "1.00")
            if bad:
                rejected.add((q, t))
        S.group("size_%d" % n, q, n >= 4)

    # ---- mixed paths in one deep pile: 100-column records (7 or 8 words; 60 of them overflow the pool of either deep instance), targets
    # with N, spans of 200 columns, a rejected record, all over the same columns of a 260-letter query
    core = cc.core_with_probes(rs, 260, probes=(0, 4, 5, 63, 64, 99, 100, 130, 199, 200, 254, 255, 259))
    q = S.seq(cc.damaged(rs, core, force=(0, 4, 5, 63, 64, 99, 100, 130, 199, 200, 254, 255, 259)), self_record=False)
    for i in range(64):
        rev = i % 2 == 1
        kind = ("plain", "plain", "withN", "plain", "long", "plain", "plain", "seqid")[i % 8]
        if kind == "long":
            cc.target(S, rs, q, core, 30, 229, int(rs.randint(0, 8)), 212, rev)
        elif kind == "withN":
            ds = int(rs.randint(0, 8))

            def sed(stored, lo=(150 - ds - 100) if rev else ds):
                stored[next(j for j in range(lo + 20, lo + 100) if stored[j] in b"AG")] = ord("N")
            cc.target(S, rs, q, core, 60, 159, ds, 150, rev, stored_edit=sed)
        elif kind == "seqid":
            rejected.add((q, cc.target(S, rs, q, core, 50, 149, 3, 150, rev, seq_id="0.899")))
        else:
            qa = (0, 60, 130, 160)[i // 8 % 4]
            cc.target(S, rs, q, core, qa, qa + 99, (0, 3, 7, 47)[i % 4], 150, rev)
    S.group("mixed_paths_64", q, True)
    return S.finish(), rejected


def fixture(what):
    return mmdb.load_keyed(os.path.join(DIR, what + ".keyed.gz"))


@pytest.fixture(scope="module")
def cases(oracle_bin, dhigh_prefix, tmp_path_factory):
    """the case set, its two DBs and the oracle's ancient_correction on them (computed once)"""
    S, rejected = build_cases()
    d = tmp_path_factory.mktemp("pileup_split")
    t = lambda s: str(d / s)
    seq_keyed, aln_keyed = S.seq_keyed(), S.aln_keyed()
    mmdb.write_from_keyed(t("in"), seq_keyed, mmdb.DBTYPE_NUCLEOTIDES)
    mmdb.write_from_keyed(t("aln"), aln_keyed, mmdb.DBTYPE_ALIGNMENT_RES)
    run_oracle(oracle_bin, "ancient_correction", t("in"), t("aln"), t("corr"), *A_FLAGS, "--ancient-damage", dhigh_prefix, "--threads", "4")
    return S, rejected, seq_keyed, aln_keyed, mmdb.read_db(t("corr"))


def test_cases_are_what_they_claim(cases):
    """no GPU: the generator gives the committed inputs, the oracle agrees with the reference's committed answer, every group has
    called columns, and the probed columns decide as the two styles say"""
    S, rejected, seq_keyed, aln_keyed, oracle = cases
    assert mmdb.canon(seq_keyed) == mmdb.canon(fixture("reads")) and mmdb.canon(aln_keyed) == mmdb.canon(fixture("aln_0"))
    assert not diff_keys(oracle, fixture("corr_0"))
    out = mmdb.canon(oracle)
    by_name = {g["name"]: g for g in S.groups}
    assert len(by_name) == len(S.groups)
    for g in S.groups:
        if g["calls"]:
            assert out[g["query"]][0] != S.seqs[g["query"]], g["name"] + ": the oracle leaves the query as it was"
    assert sum(out[g["query"]][0] != S.seqs[g["query"]] for g in S.groups if g["calls"] is None) >= 8
    # targets keep their letters (each has its self record alone)
    queries = {g["query"] for g in S.groups}
    assert all(out[k][0] == s for k, s in enumerate(S.seqs) if k not in queries)
    for g in S.groups:
        name, q = g["name"], g["query"]
        if not name.endswith(("_miss", "_dup")):
            continue
        f = S.recs[q][1].split("\t")
        lo, hi = sorted((int(f[4]), int(f[5])))
        got, was = out[q][0], S.seqs[q]
        called = [j for j in range(lo, hi + 1) if got[j] != was[j]]
        if name.endswith("_miss"):
            assert called == list(range(lo, hi + 1)), name
        else:
            assert called == [j for j in range(lo, hi + 1) if (j - lo) % 7 == 3], name
    # the instances: under the default settings the probed piles belong to the 16..64-record instance
    n = {g["name"]: g["records"] for g in S.groups}
    assert all(16 <= v <= 64 for k, v in n.items() if k.endswith(("_miss", "_dup")) and not k.startswith("query_inside"))
    assert [n["size_%d" % k] for k in (2, 15, 16, 64)] == [2, 15, 16, 64] and n["mixed_paths_64"] == 64 and len(rejected) == 4 + 8
    assert n["sat_15_f_prefix"] == 15 and n["sat_64_r_suffix"] == 64


@pytest.fixture(scope="module")
def ctx(dhigh_prefix):
    from carpedeam_amd import capi
    c = capi.Ctx(0)
    c.damage_load(dhigh_prefix)
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("setting,env", SETTINGS, ids=[s for s, _ in SETTINGS])
def test_split_pileup_matches_oracle_and_reference(ctx, cases, monkeypatch, setting, env):
    from carpedeam_amd import capi
    S, _, seq_keyed, aln_keyed, oracle = cases
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capi.lib()                                                   # the library reads its switches again
    db = ctx.upload_keyed_seqdb(seq_keyed)
    _, keys, _ = db.meta()
    off, rec = capi.parse_aln_db(aln_keyed, keys)
    got = seqdb_to_keyed(*ctx.correct(db, ctx.upload_alns(db, off, rec)).download())
    by_query = {g["query"]: g["name"] for g in S.groups}
    for what, exp in (("oracle", oracle), ("reference", fixture("corr_0"))):
        bad = diff_keys(got, exp)
        assert not bad, "%s: device differs from the %s in groups %s" % (setting, what, sorted({by_query.get(k, "target %d" % k) for k in bad}))
