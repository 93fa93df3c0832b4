"""The directed corrector cases (tests/correctcases.py) on the CPU: the oracle against what the reference's object code made of
them (tests/golden/correct_directed/), the generator against the committed inputs, and the conditions that keep the cases from
being vacuous - checked on the reference's output alone.  The call-level model (tests/callmodel.py) against the reference's
recorded answers, and the tie fixture against the model."""
import os

import numpy as np
import pytest

import callmodel
import correctcases
from carpedeam_amd import mmdb
from gpuutil import GOLD, diff_keys, run_oracle
from stageflags import A_FLAGS

DIR = os.path.join(GOLD, "correct_directed")
TIES = os.path.join(GOLD, "functions", "call_ties.tsv.gz")


def fixture(name, what):
    return mmdb.load_keyed(os.path.join(DIR if name == "main" else os.path.join(DIR, name), what + ".keyed.gz"))


@pytest.fixture(scope="module")
def sets():
    return {name: make() for name, make in correctcases.SETS}


def changed_groups(S, corr):
    corr = mmdb.canon(corr)
    return {g["name"] for g in S.groups if corr[g["query"]][0] != S.seqs[g["query"]]}


@pytest.mark.parametrize("name", [n for n, _ in correctcases.SETS])
def test_generator_reproduces_committed_inputs(sets, name):
    S = sets[name]
    assert mmdb.canon(S.seq_keyed()) == mmdb.canon(fixture(name, "reads"))
    assert mmdb.canon(S.aln_keyed()) == mmdb.canon(fixture(name, "aln_0"))
    # byte for byte: the dump of the generator's DBs is the committed text
    import gzip
    for keyed, fn, dbtype in ((S.seq_keyed(), "reads", mmdb.DBTYPE_NUCLEOTIDES), (S.aln_keyed(), "aln_0", mmdb.DBTYPE_ALIGNMENT_RES)):
        lines = []
        for k in sorted(keyed):
            lines += ["#%d\t%d" % (k, keyed[k][1]), keyed[k][0].decode("latin1").rstrip("\n")]
        path = os.path.join(DIR if name == "main" else os.path.join(DIR, name), fn + ".keyed.gz")
        assert ("\n".join(lines) + "\n").encode("latin1") == gzip.open(path, "rb").read(), fn


@pytest.mark.parametrize("name", [n for n, _ in correctcases.SETS])
def test_oracle_matches_reference_fixture(sets, oracle_bin, dhigh_prefix, tmp_path, name):
    t = lambda s: str(tmp_path / s)
    mmdb.write_from_keyed(t("in"), fixture(name, "reads"), mmdb.DBTYPE_NUCLEOTIDES)
    mmdb.write_from_keyed(t("aln"), fixture(name, "aln_0"), mmdb.DBTYPE_ALIGNMENT_RES)
    run_oracle(oracle_bin, "ancient_correction", t("in"), t("aln"), t("corr"), *A_FLAGS, "--ancient-damage", dhigh_prefix, "--threads", "4")
    bad = diff_keys(mmdb.read_db(t("corr")), fixture(name, "corr_0"))
    by_query = {g["query"]: g["name"] for g in sets[name].groups}
    assert not bad, "oracle differs from the reference in groups %s" % sorted({by_query.get(k, "target %d" % k) for k in bad})


def test_called_groups_change_a_base(sets):
    S, changed = sets["main"], changed_groups(sets["main"], fixture("main", "corr_0"))
    assert not [g["name"] for g in S.groups if g["calls"] is True and g["name"] not in changed]
    assert not [g["name"] for g in S.groups if g["calls"] is False and g["name"] in changed]
    for name in ("lonely", "single"):
        assert not changed_groups(sets[name], fixture(name, "corr_0"))
        assert mmdb.canon(fixture(name, "corr_0")) == mmdb.canon(fixture(name, "reads"))
    # targets are queries with their self record only: untouched
    corr, reads = mmdb.canon(fixture("main", "corr_0")), mmdb.canon(fixture("main", "reads"))
    queries = {g["query"] for g in S.groups}
    assert all(corr[k] == reads[k] for k in reads if k not in queries)


def test_gate_pairs_have_one_member_on_each_side(sets):
    S, changed = sets["main"], changed_groups(sets["main"], fixture("main", "corr_0"))
    names = {g["name"] for g in S.groups}
    for inside, outside in correctcases.GATE_PAIRS:
        assert inside in names and outside in names, (inside, outside)
        assert inside in changed and outside not in changed, (inside, outside)
    # at avCov 50 right-only and left-only records still correct
    assert {"avcov50_right", "avcov50_left", "avcov50_big_right", "avcov50_big_left"} <= changed
    # the query N under coverage >= 2 is called, the one under coverage 1 stays
    g = next(g for g in S.groups if g["name"] == "queryN")
    out = mmdb.canon(fixture("main", "corr_0"))[g["query"]][0]
    assert out[10:11] == b"N" and out[50:51] == b"G"


def test_every_instance_receives_groups(sets):
    S = sets["main"]
    n = np.array([g["records"] for g in S.groups])
    assert ((n >= 2) & (n <= 15)).sum() > 0 and ((n >= 16) & (n <= 64)).sum() > 0 and (n > 64).sum() > 0
    assert {1, 2, 15, 16, 64, 65, 66} <= set(n.tolist())
    raw = [g for g in S.groups if g["name"].startswith("raw_")]
    assert raw and {g["records"] <= 15 for g in raw} == {True, False}
    odd = lambda s: any(c not in b"ACGTN" for c in s)
    assert all(odd(S.seqs[g["query"]]) or any(odd(S.seqs[int(l.split("\t")[0])]) for l in S.recs[g["query"]]) for g in raw)
    # one record per (query, target) pair, every sequence has its self record unless the group says otherwise
    for q, recs in S.recs.items():
        ts = [int(l.split("\t")[0]) for l in recs]
        assert len(ts) == len(set(ts))


def test_ry_handoff_set_meets_its_conditions(oracle_bin, dhigh_prefix, tmp_path):
    """the hits of the RY hand-off test (tests/test_gpu_correct_directed.py), on the oracle's run alone"""
    correctcases.ry_handoff_oracle(oracle_bin, dhigh_prefix, tmp_path)


# ---------------------------------------------------------------------------------------------------------------- call level
needs_x87 = pytest.mark.skipif(not callmodel.usable(), reason="the model needs an x87 long double")


@needs_x87
def test_model_reproduces_known_answers():
    """the np.longdouble restatement of mostLikeliBaseRead gives the reference's answer on all 3000 recorded pile-ups"""
    head, cnt, rev, exp, _ = callmodel.parse_vectors(os.path.join(GOLD, "functions", "mostlikeli.tsv.gz"))
    ans, _, _ = callmodel.Model().call(head[:, 0], head[:, 1], head[:, 2], head[:, 3], cnt, rev)
    assert len(exp) == 3000 and (ans == exp).all()


def classify(model, head, cnt, rev):
    """(answers, kinds): a = exact tie of the top two long double sums, b = near tie (differ by less than 1e-12 relative), c = the
    arg-max of the sums folded in float64 is another one"""
    ans, s, early = model.call(head[:, 0], head[:, 1], head[:, 2], head[:, 3], cnt, rev)
    ans64, _, _ = model.call(head[:, 0], head[:, 1], head[:, 2], head[:, 3], cnt, rev, dtype=np.float64)
    top = np.sort(s, 1)
    t1, t2 = top[:, 3], top[:, 2]
    kinds = []
    for i in range(len(ans)):
        k = ""
        if not early[i]:
            if t1[i] == t2[i]:
                k += "a"
            elif t1[i] - t2[i] < np.longdouble(1e-12) * (abs(t1[i]) + abs(t2[i])):
                k += "b"
            if ans64[i] != ans[i]:
                k += "c"
        kinds.append(k)
    return ans, kinds


@needs_x87
def test_tie_fixture_holds_what_the_search_found():
    """every vector of call_ties.tsv.gz is of the kind it is filed under and carries the model's answer; the counts are those of
    the search (scripts/find_call_ties.py, docs/NOTEBOOK.md)"""
    head, cnt, rev, exp, kinds = callmodel.parse_vectors(TIES)
    ans, got = classify(callmodel.Model(), head, cnt, rev)
    assert (ans == exp).all()
    assert got == kinds
    n = {k: sum(k in x for x in kinds) for k in "abc"}
    heavy = {k: sum(k in x and c.max() >= 45000 for x, c in zip(kinds, cnt)) for k in "abc"}
    assert n == {"a": 935, "b": 749, "c": 99}, n                       # all that the search found
    assert heavy["a"] >= 86 and heavy["b"] >= 83 and heavy["c"] >= 5, heavy
    assert cnt.max() <= 65535 and (rev <= cnt).all() and (cnt.reshape(len(cnt), -1).sum(1) >= 2).all()
    pairs = {tuple(sorted(np.argsort(-s)[:2])) for s in callmodel.Model().call(head[:, 0], head[:, 1], head[:, 2], head[:, 3], cnt, rev)[1][[("a" in k) for k in kinds]]}
    assert pairs == {(1, 2)}, pairs                                    # C against G: the one pair of candidates that ties under this profile
