"""ancient_correction on the device against the directed cases (tests/correctcases.py): every kernel instance on the hand-built
alignment sets, the RY counts handed over by cdm_rescore, and the call path on exact and near ties."""
import ctypes
import os

import numpy as np
import pytest

import callmodel
import correctcases
from carpedeam_amd import capi, mmdb
from gpuutil import GOLD, diff_keys, run_oracle, seqdb_to_keyed
from stageflags import A_FLAGS

pytestmark = pytest.mark.gpu

DIR = os.path.join(GOLD, "correct_directed")
SETTINGS = [("default", {}), ("variant_0", {"CDM_CORRECT_VARIANT": "0"}), ("variant_s5", {"CDM_CORRECT_VARIANT": "s5"}),
            ("variant_s8", {"CDM_CORRECT_VARIANT": "s8"}), ("bigw_4", {"CDM_CORRECT_BIGW": "4"}), ("bigw_6", {"CDM_CORRECT_BIGW": "6"})]


@pytest.fixture(scope="module")
def ctx(dhigh_prefix):
    c = capi.Ctx(0)
    c.damage_load(dhigh_prefix)
    return c


def fixture(name, what):
    return mmdb.load_keyed(os.path.join(DIR if name == "main" else os.path.join(DIR, name), what + ".keyed.gz"))


@pytest.fixture(scope="module")
def expected(oracle_bin, dhigh_prefix, tmp_path_factory):
    """per set: the case set, the oracle's output on the committed inputs and the reference's committed output (computed once)"""
    out = {}
    for name, make in correctcases.SETS:
        d = tmp_path_factory.mktemp("directed_" + name)
        t = lambda s: str(d / s)
        mmdb.write_from_keyed(t("in"), fixture(name, "reads"), mmdb.DBTYPE_NUCLEOTIDES)
        mmdb.write_from_keyed(t("aln"), fixture(name, "aln_0"), mmdb.DBTYPE_ALIGNMENT_RES)
        run_oracle(oracle_bin, "ancient_correction", t("in"), t("aln"), t("corr"), *A_FLAGS, "--ancient-damage", dhigh_prefix, "--threads", "4")
        out[name] = (make(), mmdb.read_db(t("corr")), fixture(name, "corr_0"))
    return out


def broken_groups(S, bad_keys):
    by_query = {g["query"]: g["name"] for g in S.groups}
    return sorted({by_query.get(k, "target %d of no group" % k) for k in bad_keys})


@pytest.mark.parametrize("setting,env", SETTINGS, ids=[s for s, _ in SETTINGS])
@pytest.mark.parametrize("name", [n for n, _ in correctcases.SETS])
def test_directed_cases_match_oracle_and_reference(ctx, expected, monkeypatch, name, setting, env):
    for k in ("CDM_CORRECT_VARIANT", "CDM_CORRECT_BIGW"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capi.lib()                                                   # the library reads its switches again
    S, oracle, reference = expected[name]
    seq_keyed, aln_keyed = fixture(name, "reads"), fixture(name, "aln_0")
    db = ctx.upload_keyed_seqdb(seq_keyed)
    _, keys, _ = db.meta()
    off, rec = capi.parse_aln_db(aln_keyed, keys)
    got = seqdb_to_keyed(*ctx.correct(db, ctx.upload_alns(db, off, rec)).download())
    bad = diff_keys(got, oracle)
    assert not bad, "%s: device differs from the oracle in groups %s" % (setting, broken_groups(S, bad))
    bad = diff_keys(got, reference)
    assert not bad, "%s: device differs from the reference in groups %s" % (setting, broken_groups(S, bad))


# ---------------------------------------------------------------------------------------------------------------- RY hand-off
def test_ry_counts_handed_from_rescore(ctx, oracle_bin, dhigh_prefix, tmp_path):
    """hand-built hits -> cdm_rescore -> cdm_correct (the RY counts of rescore, compacted beside the records) against the same
    alignments downloaded and uploaded again (counted in the corrector) and against the oracle's rescorediagonal + ancient_correction"""
    seqs, info, pref, aln, corr = correctcases.ry_handoff_oracle(oracle_bin, dhigh_prefix, tmp_path)

    db = ctx.upload_seqs(seqs)
    lens, keys, _ = db.meta()
    off, rec = capi.parse_pref_db(dict((q, (p, 0)) for q, p in pref), keys)
    alns = ctx.rescore(db, ctx.upload_hits(db, off, rec))
    aoff, arec = alns.download()
    bad = diff_keys({k: (v, 0) for k, v in capi.alns_to_text(aoff, arec, keys, lens, db.residues).items()}, aln)
    assert not bad, "rescore differs from the oracle for queries %s" % [info.get(k, {"name": k})["name"] for k in bad]
    name_of = lambda bad: sorted({info[k]["name"] if k in info else "sequence %d" % k for k in bad})
    handed = seqdb_to_keyed(*ctx.correct(db, alns).download())
    counted = seqdb_to_keyed(*ctx.correct(db, ctx.upload_alns(db, aoff, arec)).download())
    bad = diff_keys(handed, corr)
    assert not bad, "RY counts handed over by rescore: the corrector differs from the oracle for %s" % name_of(bad)
    bad = diff_keys(counted, corr)
    assert not bad, "RY counted in the corrector: it differs from the oracle for %s" % name_of(bad)
    assert not diff_keys(handed, counted)


# ---------------------------------------------------------------------------------------------------------------- call level
def test_call_bases_on_ties(ctx):
    """cdm_debug_call_bases on the vectors scripts/find_call_ties.py found - (a) exact ties of the top two sums, where the first
    maximum wins, (b) near ties inside the kernel's own 1e-12 margin, (c) vectors on which sums folded in float64 pick another
    base - against the long double model (tests/callmodel.py, itself checked against the reference's 3000 answers)"""
    head, cnt, rev, exp, kinds = callmodel.parse_vectors(os.path.join(GOLD, "functions", "call_ties.tsv.gz"))
    vec = callmodel.device_vectors(head, cnt, rev)
    out = np.zeros(len(vec), np.uint8)
    l = capi.lib()
    l.cdm_debug_call_bases.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_uint32, ctypes.c_void_p]
    rc = l.cdm_debug_call_bases(ctx.h, vec.ctypes.data_as(ctypes.c_void_p), len(vec), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, l.cdm_last_error()
    bad = np.nonzero(out != exp)[0]
    per_kind = {k: sum(k in kinds[i] for i in bad) for k in "abc"}
    assert bad.size == 0, "wrong calls by kind (a exact tie, b near tie, c float64 picks another): %s; first vectors %s" % (per_kind, bad[:10].tolist())
