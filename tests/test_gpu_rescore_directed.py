"""cdm_rescore on the directed cases (tests/rescorecases.py): per set and parameter row the offsets, every field of every record bit
for bit, the purine/pyrimidine counts, the record count and the count of identity records with the coordinates -1 against the
model (tests/rescore_model.py, computed in this process), and the records' text against what the reference's object code wrote
(tests/golden/rescore_directed/).  Then the two-pass form (CDM_RESCORE=twopass, read once: a fresh child process runs this file
as a script), the module's path from flags to cdm_rescore_params, and the refusal of a -e that lets a score of 0 pass.

The prefilter text may spell one diagonal in several ways; cdm_hits_upload takes the 16-bit value only, so the hits go up as
the text's reader narrows them (rescorecases.short, as host/records.cpp and the reference's QueryMatcher.h:88 do)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "carpedeam_amd", "carpedeam")
pytestmark = pytest.mark.gpu
TWOPASS_SETS = ("gates", "letters")
MODULE_ROWS = ("cov0_c0.8", "alnlen30", "sid0.97_e1e-05")


def run_set(ctx, S):
    """every row of a set on the device -> {row: (off, rec, ry, count, undefined records)}"""
    db = ctx.upload_seqs(S.seqs)
    assert db.residues == S.residues
    hits = ctx.upload_hits(db, *S.csr())
    out = {}
    for row, par in S.rows:
        alns = ctx.rescore(db, hits, par.capi())
        off, rec = alns.download()
        out[row] = (off, rec, alns.download_ry(), int(alns.count), int(alns.undefined_records))
    return out


def child(out_path):
    sys.path.insert(0, ROOT)
    import rescorecases
    from carpedeam_amd import capi
    ctx = capi.Ctx(0)
    res = {}
    for name, make in rescorecases.SETS:
        if name in TWOPASS_SETS:
            for row, (off, rec, ry, count, undefined) in run_set(ctx, make()).items():
                res.update({"%s/%s/off" % (name, row): off, "%s/%s/rec" % (name, row): rec, "%s/%s/ry" % (name, row): ry,
                            "%s/%s/n" % (name, row): np.array([count, undefined], np.int64)})
    np.savez(out_path, **res)


if __name__ == "__main__":
    child(sys.argv[1])
    sys.exit(0)

import rescore_model  # noqa: E402
import rescorecases  # noqa: E402
from carpedeam_amd import capi, mmdb  # noqa: E402
from gpuutil import diff_keys  # noqa: E402
from rescorecases import fixture, records  # noqa: E402

NAMES = [n for n, _ in rescorecases.SETS]


@pytest.fixture(scope="module")
def ctx():
    return capi.Ctx(0)


@pytest.fixture(scope="module")
def expected():
    """per set: the case set and the model's answer for every row (computed once)"""
    out = {}
    for name, make in rescorecases.SETS:
        S = make()
        assert [S.digest(), str(len(S.groups))] == rescorecases.fixture_digest(name)
        hits = S.hit_list()
        scored = rescore_model.score_set(S.seqs, hits)[1]
        out[name] = (S, {row: rescore_model.apply(S.seqs, hits, scored, par) for row, par in S.rows})
    return out


def broken_groups(S, got, want):
    """the groups whose record (with its purine/pyrimidine count) differs between two (off, rec, ry) results"""
    def by_pair(off, rec, ry):
        out = {}
        for q in range(len(off) - 1):
            for r in range(int(off[q]), int(off[q + 1])):
                out[(q, int(rec[r]["target"]))] = (rec[r].tobytes(), int(ry[r]))
        return out
    if int(got[0][-1]) != len(got[1]) or len(got[1]) != len(got[2]):
        return ["offsets, records and counts of different lengths"]
    a, b, names = by_pair(*got), by_pair(*want), S.by_pair()
    return sorted(names.get(k, "pair %s of no group" % (k,)) for k in set(a) | set(b) if a.get(k) != b.get(k))[:12]


def compare(S, name, got_rows, want_rows, form):
    failures = []
    for row, _ in S.rows:
        off, rec, ry, count, undefined = got_rows[row]
        w_off, w_rec, w_ry, w_undefined = want_rows[row]
        same = (np.array_equal(off, w_off) and rec.dtype.itemsize == 32 and rec.tobytes() == w_rec.tobytes() and np.array_equal(ry, w_ry)
                and count == len(w_rec) and undefined == w_undefined)
        if not same:
            failures.append("%s: differs from the model in groups %s (count %d | %d, undefined records %d | %d)"
                            % (row, broken_groups(S, (off, rec, ry), (w_off, w_rec, w_ry)), count, len(w_rec), undefined, w_undefined))
        lens = np.array([len(s) for s in S.seqs], np.int64)
        text = {k: (v, 0) for k, v in capi.alns_to_text(off, rec, np.arange(len(S.seqs)), lens, S.residues).items()}
        exp = fixture(name, row)
        if diff_keys(text, exp):
            a, b = records(text), records(exp)
            failures.append("%s: text differs from the reference in groups %s" % (row, sorted(S.by_pair().get(k, str(k)) for k in set(a) | set(b) if a.get(k) != b.get(k))[:12]))
    assert not failures, "%s, %s:\n%s" % (name, form, "\n".join(failures))


@pytest.mark.parametrize("name", NAMES)
def test_directed_cases_match_model_and_reference(ctx, expected, name):
    S, want = expected[name]
    compare(S, name, run_set(ctx, S), want, "one-pass")


def test_two_pass_form_matches_model_and_reference(expected, tmp_path):
    out = str(tmp_path / "twopass.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("CDM_RESCORE", "CDM_RESCORE_BLOCKS")}
    env["CDM_RESCORE"] = "twopass"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    got = dict(np.load(out))
    for name in TWOPASS_SETS:
        S, want = expected[name]
        rows = {row: (got["%s/%s/off" % (name, row)], got["%s/%s/rec" % (name, row)], got["%s/%s/ry" % (name, row)], *(int(x) for x in got["%s/%s/n" % (name, row)]))
                for row, _ in S.rows}
        compare(S, name, rows, want, "two-pass")


def test_module_flags_reach_the_kernel(expected, tmp_path):
    """`carpedeam rescorediagonal` on the gates set under three rows of flags that are not the defaults: text and dbtype"""
    S, _ = expected["gates"]
    t = lambda s: str(tmp_path / s)
    S.write(t("db"), t("pref"))
    rows = dict(S.rows)
    for row in MODULE_ROWS:
        r = subprocess.run([BIN, "rescorediagonal", t("db"), t("db"), t("pref"), t(row)] + rows[row].flags() + ["--threads", "1"], capture_output=True, text=True)
        assert r.returncode == 0, (row, r.stderr[-2000:])
        got, exp = mmdb.read_db(t(row)), fixture("gates", row)
        a, b = records(got), records(exp)
        assert not diff_keys(got, exp), "%s: the module differs from the reference in groups %s" % (row, sorted(S.by_pair().get(k, str(k)) for k in set(a) | set(b) if a.get(k) != b.get(k))[:12])
        assert mmdb.read_dbtype(t(row)) == mmdb.DBTYPE_ALIGNMENT_RES


def unrelated_pair():
    rs = np.random.RandomState(7)
    S = rescorecases.RSet("refusal", 7)
    S.hit("unrelated", S.seq(rescorecases.rnd(rs, 60)), S.seq(rescorecases.rnd(rs, 60)), False, 0)
    S.hits.sort()
    return S


def test_an_e_that_lets_score_zero_pass_is_refused(ctx):
    """-e 1e9 on two unrelated sequences: the score 0 would pass, the reference's record for it is undefined - CDM_ERR_UNSUPPORTED, the
    message names -e; the largest -e below the E-value of score 0 is taken, and drops the hit"""
    S = unrelated_pair()
    db = ctx.upload_seqs(S.seqs)
    hits = ctx.upload_hits(db, *S.csr())
    with pytest.raises(capi.CdmError, match=r"cdm error -4: .*-e ") as e:
        ctx.rescore(db, hits, rescore_model.Params(e=1e9, min_seq_id=0.0).capi())
    assert "score of 0" in str(e.value)
    e0 = capi.lib().cdm_evalue(0.0, 60.0, 120)
    with pytest.raises(capi.CdmError, match=r"cdm error -4: .*-e "):
        ctx.rescore(db, hits, rescore_model.Params(e=e0, min_seq_id=0.0).capi())
    alns = ctx.rescore(db, hits, rescore_model.Params(e=np.nextafter(e0, 0.0), min_seq_id=0.0).capi())
    assert alns.count == 0 and alns.undefined_records == 0


def test_the_module_refuses_such_an_e(tmp_path):
    S = unrelated_pair()
    t = lambda s: str(tmp_path / s)
    S.write(t("db"), t("pref"))
    r = subprocess.run([BIN, "rescorediagonal", t("db"), t("db"), t("pref"), t("aln")] + rescore_model.Params(e=1e9, min_seq_id=0.0).flags() + ["--threads", "1"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "-e " in r.stderr and "score of 0" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(t("aln"))
