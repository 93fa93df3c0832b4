"""ancient_read_assemble on the device against the directed cases (tests/extendcases.py): every set through the three forms of the
kernel - sequences and ext flags against the oracle and against the reference's committed output, the set of scored records and
every likelihood score against the oracle's, bit for bit - and the main set in --unsafe 1 against the oracle."""
import numpy as np
import pytest

import extendcases
from carpedeam_amd import capi, mmdb
from extendcases import fixture, run_oracle_on_fixture
from gpuutil import diff_keys, run_oracle, seqdb_to_keyed

pytestmark = pytest.mark.gpu

FORMS = [("records", {}), ("records-wide-margins", {"CDM_EXTEND_MARGIN": "3e11"}), ("queries", {"CDM_EXTEND": "queries"})]


@pytest.fixture(scope="module")
def ctx(dhigh_prefix):
    c = capi.Ctx(0)
    c.damage_load(dhigh_prefix)
    return c


@pytest.fixture(scope="module")
def expected(oracle_bin, dhigh_prefix, tmp_path_factory):
    """per set: the case set, the oracle's output and score log on the committed inputs, the reference's committed output (once)"""
    d = tmp_path_factory.mktemp("gpu_extend_directed")
    out = {}
    for name, make, max_seq_len in extendcases.SETS:
        asm, scores = run_oracle_on_fixture(oracle_bin, dhigh_prefix, d, name, max_seq_len)
        out[name] = (make(), asm, scores, fixture(name, "asm"), max_seq_len)
    return out


def set_form(monkeypatch, env):
    for k in ("CDM_EXTEND", "CDM_EXTEND_MARGIN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capi.lib()                                                   # the library reads its switches again


def broken_groups(S, bad_keys):
    by_key = {g["key"]: g["name"] for g in S.groups}
    return sorted({by_key.get(k, "target %d of no group" % k) for k in bad_keys})


def device_extend(ctx, seq_keyed, aln_keyed, par, want_scores):
    db = ctx.upload_keyed_seqdb(seq_keyed)
    _, keys, _ = db.meta()
    off, rec = capi.parse_aln_db(aln_keyed, keys)
    res = ctx.extend(db, ctx.upload_alns(db, off, rec), par, want_scores=want_scores)
    if not want_scores:
        return seqdb_to_keyed(*res.download()), None
    asm, scores = res
    got = {}
    for i, k in enumerate(keys):
        for r in range(int(off[i]), int(off[i + 1])):
            if not np.isnan(scores[r]):
                got[(int(k), int(keys[rec[r]["target"]]))] = float(scores[r])
    return seqdb_to_keyed(*asm.download()), got


@pytest.mark.parametrize("form,env", FORMS, ids=[f for f, _ in FORMS])
@pytest.mark.parametrize("name", [n for n, _, _ in extendcases.SETS])
def test_directed_cases_match_oracle_and_reference(ctx, expected, monkeypatch, name, form, env):
    set_form(monkeypatch, env)
    S, oracle, oracle_scores, reference, max_seq_len = expected[name]
    par = capi.AncientParams.default()
    par.max_seq_len = max_seq_len
    seq_keyed, aln_keyed = fixture(name, "corr"), fixture(name, "aln")
    # without the scores: the form as it runs in production (the record form takes the plain-double likelihoods where they decide)
    got, _ = device_extend(ctx, seq_keyed, aln_keyed, par, False)
    bad = diff_keys(got, oracle)
    assert not bad, "%s: device differs from the oracle in groups %s" % (form, broken_groups(S, bad))
    bad = diff_keys(got, reference)
    assert not bad, "%s: device differs from the reference in groups %s" % (form, broken_groups(S, bad))
    # with the scores: the same sequences, the oracle's set of scored records, every score bit-equal
    got, scores = device_extend(ctx, seq_keyed, aln_keyed, par, True)
    bad = diff_keys(got, reference)
    assert not bad, "%s, scores asked for: device differs from the reference in groups %s" % (form, broken_groups(S, bad))
    exp = {k: v[0] for k, v in oracle_scores.items()}
    odd = set(scores) ^ set(exp)
    assert not odd, "%s: scored records differ from the oracle's in groups %s" % (form, broken_groups(S, {q for q, _ in odd}))
    bad = [k for k in exp if scores[k] != exp[k]]
    assert not bad, "%s: likelihood scores differ in groups %s, e.g. %s" % (form, broken_groups(S, {q for q, _ in bad}), [(k, scores[k], exp[k]) for k in bad[:3]])


@pytest.mark.parametrize("min_cov", [1, 2, 5])
def test_main_set_unsafe_mode_matches_oracle(ctx, oracle_bin, dhigh_prefix, tmp_path, monkeypatch, min_cov):
    """--unsafe 1 on the main set, against the oracle (whose unsafe mode is pinned to the reference in tests/test_oracle_golden.py).  The
    groups the device refuses - a target that overhangs the query by more than the query's length - and the queries too deep for a mode
    that is quadratic in a query's records are taken out by the generator's own filter; together they are fewer than a quarter."""
    set_form(monkeypatch, {})
    S = extendcases.main_set()
    seq_keyed, aln_keyed, refused, deep = extendcases.without_unsupported(S)
    assert refused + deep < len(S.groups) / 4
    t = lambda s: str(tmp_path / s)
    mmdb.write_from_keyed(t("corr"), seq_keyed, mmdb.DBTYPE_NUCLEOTIDES)
    mmdb.write_from_keyed(t("aln"), aln_keyed, mmdb.DBTYPE_ALIGNMENT_RES)
    run_oracle(oracle_bin, "ancient_read_assemble", t("corr"), t("aln"), t("asm"), *extendcases.flags_for(200000, 1, min_cov), "--ancient-damage", dhigh_prefix, "--threads", "4")
    par = capi.AncientParams.default()
    par.unsafe, par.min_cov_safe = 1, min_cov
    got, _ = device_extend(ctx, seq_keyed, aln_keyed, par, False)
    exp = mmdb.read_db(t("asm"))
    bad = diff_keys(got, exp)
    assert not bad, "unsafe, min-cov-safe %d: device differs from the oracle in groups %s" % (min_cov, broken_groups(S, bad))
    assert sum(v[1] for v in exp.values()) > 50
