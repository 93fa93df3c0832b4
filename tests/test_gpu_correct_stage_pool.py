"""The pooled target stage of k_correct_fast (csrc/correct.hip): piles built so that the pool overflows in the middle of a wave,
that it ends exactly on a record and one word short of it, that rejected records, targets with N and long spans sit between the
staged ones - every one under the default settings and under small pools (CDM_CORRECT_STAGE_POOL), against the oracle's
ancient_correction.  Which records land in the pool must never show in a result; that the pool is cut up as documented is read
from the kernel's own counters (CDM_CORRECT_STATS) and compared with the rule worked out here from the records."""
import re

import numpy as np
import pytest

import correctcases as cc
from carpedeam_amd import capi, mmdb
from gpuutil import diff_keys, run_oracle, seqdb_to_keyed
from stageflags import A_FLAGS

pytestmark = pytest.mark.gpu

STAGE_WORDS = 12
SWITCHES = ("CDM_CORRECT_VARIANT", "CDM_CORRECT_BIGW", "CDM_CORRECT_STAGE_POOL", "CDM_CORRECT_STATS")


def n_words(lo, n):
    """code words that hold n letters stored from letter lo on"""
    return ((lo + n - 1) >> 4) - (lo >> 4) + 1


def record(S, rs, q, core, qa, n, lo, tlen, rev, **kw):
    """a record over core[qa .. qa + n - 1] whose letters are stored from letter lo of the target on"""
    return cc.target(S, rs, q, core, qa, qa + n - 1, tlen - lo - n if rev else lo, tlen, rev, **kw)


def build_cases(seed=29):
    """the case set and the (query, target) pairs the gates turn away"""
    rs = np.random.RandomState(seed)
    S = cc.CaseSet()
    rejected = set()

    # ---- records per query (self included): the small instance, both ends of the deep one, the general kernel
    for n in (15, 16, 64, 65):
        cc.pile(S, rs, "count_%d" % n, 40 if n < 45 else 64, n - 1, "m", alen=None if n < 45 else 32)

    # ---- overflow in the middle of a wave: 64 accepted records of 100 columns, stored from letter 0 and from letter 15 of a word on
    # (7 and 8 words: 480 in all).  The 200-letter query keeps avCov at 32; there is no self record (it would be the 65th)
    core = cc.core_with_probes(rs, 200)
    q = S.seq(cc.damaged(rs, core, force=cc.probe_cols(200)), self_record=False)
    for i in range(64):
        record(S, rs, q, core, (0, 100)[i // 2 % 2], 100, 16 * int(rs.randint(0, 3)) + (0, 15)[i % 2], 170, i % 3 == 1)
    S.group("overflow_64", q, True)

    # ---- the same 7, 8, 7, 8 ... behind a self record of 7 words, for the small instance (6 records) and the deep one (20): the pool
    # ends are 7, 14, 22, 29, 37, 44 ... so that a pool of 22 (37) is filled exactly by the third (fifth) record
    for name, nt in (("ramp_small", 5), ("ramp_deep", 19)):
        core = cc.core_with_probes(rs, 100)
        q = S.seq(cc.damaged(rs, core, force=cc.probe_cols(100)))
        for i in range(nt):
            record(S, rs, q, core, 0, 100, 16 * int(rs.randint(0, 3)) + (0, 15)[i % 2], 170, i % 2 == 1)
        S.group(name, q, True)

    # ---- mixed: forward and reverse interleaved; records the RY gate and seqId turn away, targets with N, spans of 30 columns (the
    # shortest accepted), of 177 (12 words wherever they start) and of 178 from letter 15 on (13 words: never staged) in between
    for name, nt in (("mixed_small", 12), ("mixed_deep", 40)):
        core = cc.core_with_probes(rs, 240, probes=(0, 4, 5, 29, 120, 176, 177, 234, 235, 239))
        q = S.seq(cc.damaged(rs, core, force=(0, 4, 5, 29, 120, 176, 177, 234, 235, 239)))
        for i in range(nt):
            rev = i % 2 == 1
            kind = ("plain", "ry", "n30", "withN", "n177", "seqid", "plain", "n178", "n177_15", "plain")[i % 10]
            lo16 = 16 * int(rs.randint(0, 3))
            if kind == "plain":
                record(S, rs, q, core, (0, 140, 70)[i % 3], 100, lo16 + (0, 15, 9)[i % 3], 200, rev)
            elif kind == "ry":          # two purine <-> pyrimidine substitutions in 100 columns: below the rymer threshold
                rejected.add((q, record(S, rs, q, core, 60, 100, lo16 + 3, 200, rev, edit=cc.ry_edit(2), seq_id="0.980")))
            elif kind == "seqid":
                rejected.add((q, record(S, rs, q, core, 30, 100, lo16 + 15, 200, rev, seq_id="0.899")))
            elif kind == "n30":
                record(S, rs, q, core, (0, 210)[i // 10 % 2], 30, lo16 + (0, 15)[i // 10 % 2], 120, rev)
            elif kind == "withN":       # an N on a purine column of the span (N counts as A: the same RY class)
                lo = lo16 + 7

                def sed(stored, lo=lo):
                    stored[next(j for j in range(lo + 20, lo + 100) if stored[j] in b"AG")] = ord("N")
                record(S, rs, q, core, 100, 100, lo, 200, rev, stored_edit=sed)
            elif kind == "n177":
                record(S, rs, q, core, 0, 177, lo16, 260, rev)
            elif kind == "n177_15":
                record(S, rs, q, core, 63, 177, lo16 + 15, 260, rev)
            else:
                record(S, rs, q, core, 31, 178, lo16 + 15, 260, rev)
        S.group(name, q, True)
    return S.finish(), rejected


def model_counts(S, rejected, pool):
    """what CDM_CORRECT_STATS counts with a pool of `pool` words (below every compiled pool): accepted records of the queries with 2
    to 64 records, of them the ones with N in the target, the ones longer than STAGE_WORDS words, and the ones past the pool"""
    accepted = with_n = long_ = over = 0
    for q, lines in S.recs.items():
        if not 2 <= len(lines) <= 64:
            continue
        end = 0
        for l in lines:
            f = l.split("\t")
            t, ds, de = int(f[0]), int(f[7]), int(f[8])
            if (q, t) in rejected:
                continue
            accepted += 1
            nw = n_words(ds, de - ds + 1)                 # (ds .. de are letters of the target as stored)
            if b"N" in S.seqs[t]:
                with_n += 1
            elif nw > STAGE_WORDS:
                long_ += 1
            else:
                end += nw
                over += end > pool
    return accepted, with_n, long_, over


# pools: nothing; the first record alone (7 words) and 8; ended exactly by the third and the fifth record of the ramps, and one word short
POOLS = (0, 7, 8, 22, 21, 37, 36)
SETTINGS = [("default", {}), ("bigw_4", {"CDM_CORRECT_BIGW": "4"}), ("variant_0", {"CDM_CORRECT_VARIANT": "0"})] + [
    ("pool_%d" % p, {"CDM_CORRECT_STAGE_POOL": str(p)}) for p in POOLS] + [("pool_22_bigw_4", {"CDM_CORRECT_STAGE_POOL": "22", "CDM_CORRECT_BIGW": "4"})]


@pytest.fixture(scope="module")
def ctx(dhigh_prefix):
    c = capi.Ctx(0)
    c.damage_load(dhigh_prefix)
    return c


@pytest.fixture(scope="module")
def cases(oracle_bin, dhigh_prefix, tmp_path_factory):
    """the case set, its two DBs and the oracle's ancient_correction on them (computed once)"""
    S, rejected = build_cases()
    d = tmp_path_factory.mktemp("stage_pool")
    t = lambda s: str(d / s)
    seq_keyed, aln_keyed = S.seq_keyed(), S.aln_keyed()
    mmdb.write_from_keyed(t("in"), seq_keyed, mmdb.DBTYPE_NUCLEOTIDES)
    mmdb.write_from_keyed(t("aln"), aln_keyed, mmdb.DBTYPE_ALIGNMENT_RES)
    run_oracle(oracle_bin, "ancient_correction", t("in"), t("aln"), t("corr"), *A_FLAGS, "--ancient-damage", dhigh_prefix, "--threads", "4")
    return S, rejected, seq_keyed, aln_keyed, mmdb.read_db(t("corr"))


def device_correct(ctx, monkeypatch, env, seq_keyed, aln_keyed):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capi.lib()                                                   # the library reads its switches again
    db = ctx.upload_keyed_seqdb(seq_keyed)
    _, keys, _ = db.meta()
    off, rec = capi.parse_aln_db(aln_keyed, keys)
    return seqdb_to_keyed(*ctx.correct(db, ctx.upload_alns(db, off, rec)).download())


def test_cases_are_what_they_claim(cases):
    """the piles meet the shapes they were built for, and the oracle does correct them (no GPU work)"""
    S, rejected, seq_keyed, _, oracle = cases
    by_name = {g["name"]: g for g in S.groups}
    assert [by_name["count_%d" % n]["records"] for n in (15, 16, 64, 65)] == [15, 16, 64, 65]
    assert by_name["overflow_64"]["records"] == 64 and by_name["ramp_small"]["records"] == 6 and by_name["ramp_deep"]["records"] == 20
    assert by_name["mixed_small"]["records"] == 13 and by_name["mixed_deep"]["records"] == 41
    words = lambda name: [n_words(int(f[7]), int(f[8]) - int(f[7]) + 1) for f in (l.split("\t") for l in S.recs[by_name[name]["query"]])]
    assert words("overflow_64") == [7, 8] * 32 and sum(words("overflow_64")) > 352
    assert words("ramp_small") == [7, 7, 8, 7, 8, 7] and words("ramp_deep")[:6] == words("ramp_small")
    assert {12, 13, 2, 3} <= set(words("mixed_deep")) and rejected
    changed = set(diff_keys(oracle, seq_keyed))
    assert all(g["query"] in changed for g in S.groups), "the oracle leaves a query as it was"


@pytest.mark.parametrize("setting,env", SETTINGS, ids=[s for s, _ in SETTINGS])
def test_pool_settings_match_oracle(ctx, cases, monkeypatch, setting, env):
    S, _, seq_keyed, aln_keyed, oracle = cases
    got = device_correct(ctx, monkeypatch, env, seq_keyed, aln_keyed)
    bad = diff_keys(got, oracle)
    by_query = {g["query"]: g["name"] for g in S.groups}
    assert not bad, "%s: device differs from the oracle in groups %s" % (setting, sorted({by_query.get(k, "target %d" % k) for k in bad}))


def stats_of(err):
    m = re.search(r"accepted records (\d+), not staged \d+ \(target with N (\d+), more than \d+ words (\d+), past the pool (\d+)\)", err)
    assert m, "no stats line in %r" % err
    return tuple(int(x) for x in m.groups())


@pytest.mark.parametrize("pool", POOLS)
def test_pool_is_cut_up_by_the_rule(ctx, cases, monkeypatch, capfd, pool):
    """accepted records take their words in record order, rejected ones, targets with N and long spans take none, and a record is
    staged iff its words end inside the pool"""
    S, rejected, seq_keyed, aln_keyed, oracle = cases
    capfd.readouterr()
    got = device_correct(ctx, monkeypatch, {"CDM_CORRECT_STAGE_POOL": str(pool), "CDM_CORRECT_STATS": "1"}, seq_keyed, aln_keyed)
    counted = stats_of(capfd.readouterr().err)
    print("pool %d: device %s, rule %s" % (pool, counted, model_counts(S, rejected, pool)))
    assert counted == model_counts(S, rejected, pool)
    assert not diff_keys(got, oracle)


def test_default_pool_overflows_inside_a_wave(ctx, cases, monkeypatch, capfd):
    """with the compiled pool the 64-record pile is staged in part: some of its records are past the pool, most are not"""
    S, rejected, seq_keyed, aln_keyed, oracle = cases
    capfd.readouterr()
    got = device_correct(ctx, monkeypatch, {"CDM_CORRECT_STATS": "1"}, seq_keyed, aln_keyed)
    accepted, with_n, long_, over = stats_of(capfd.readouterr().err)
    print("default pool: accepted %d, with N %d, long %d, past the pool %d" % (accepted, with_n, long_, over))
    assert (accepted, with_n, long_) == model_counts(S, rejected, 0)[:3]
    # 480 words against a pool that cannot exceed 64 * STAGE_WORDS / 2 on the default instance and holds at least one record
    assert 0 < over < 64
    assert not diff_keys(got, oracle)
