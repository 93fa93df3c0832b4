"""The directed rescorer cases (tests/rescorecases.py) on the CPU: the model (tests/rescore_model.py) = `cdm_oracle rescorediagonal` =
what the reference's object code wrote (tests/golden/rescore_directed/), byte for byte, for every set and parameter row - and the
conditions that keep the cases from being vacuous, read from the reference's text alone."""
import collections

import pytest

import rescore_model
import rescorecases
from carpedeam_amd import capi, mmdb
from gpuutil import diff_keys, run_oracle
from rescorecases import fixture, record_diagonal, records

NAMES = [n for n, _ in rescorecases.SETS]


@pytest.fixture(scope="module")
def sets():
    return {name: make() for name, make in rescorecases.SETS}


@pytest.fixture(scope="module")
def scored(sets):
    return {name: rescore_model.score_set(S.seqs, S.hit_list())[1] for name, S in sets.items()}


def differing_groups(S, got, exp):
    """the groups whose record differs between two keyed alignment DBs"""
    a, b, by = records(got), records(exp), S.by_pair()
    return sorted(by.get(k, "pair %s of no group" % (k,)) for k in set(a) | set(b) if a.get(k) != b.get(k))[:12]


@pytest.mark.parametrize("name", NAMES)
def test_generator_matches_the_goldens_digest(sets, name):
    """the groups and inputs regenerated from the seed are the ones the reference ran on: no group left or changed silently"""
    S = sets[name]
    digest, n_groups = rescorecases.fixture_digest(name)
    assert len(S.groups) == int(n_groups) and S.digest() == digest
    assert len(S.groups) == len(S.hits) == len(S.by_pair())
    for where, group, reason in rescorecases.DROPPED:
        assert reason and all(group not in T.groups for T in sets.values())


@pytest.mark.parametrize("name", NAMES)
def test_model_matches_reference(sets, scored, name):
    S, hits = sets[name], sets[name].hit_list()
    for row, par in S.rows:
        off, rec, ry, undefined = rescore_model.apply(S.seqs, hits, scored[name], par)
        got, exp = rescore_model.to_text(S.seqs, off, rec), fixture(name, row)
        assert not diff_keys(got, exp), "%s: the model differs from the reference in groups %s" % (row, differing_groups(S, got, exp))
        assert undefined == (rescorecases.UNDEFINED_RECORDS.get(name, 0)), row
        assert undefined == sum(f[4] == "-1" for f in records(exp).values())
        assert int(off[-1]) == len(rec) == len(ry)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference(sets, oracle_bin, tmp_path, name):
    S = sets[name]
    t = lambda s: str(tmp_path / s)
    S.write(t("db"), t("pref"))
    for row, par in S.rows:
        run_oracle(oracle_bin, "rescorediagonal", t("db"), t("db"), t("pref"), t(row), *par.flags(), "--threads", "1")
        got, exp = mmdb.read_db(t(row)), fixture(name, row)
        assert not diff_keys(got, exp), "%s: the oracle differs from the reference in groups %s" % (row, differing_groups(S, got, exp))


def test_every_e_keeps_score_zero_out(sets):
    """no row lets a score of 0 pass its -e at any length present (RSet.finish asserts it while it builds; here on the finished sets)"""
    ev = capi.lib().cdm_evalue
    for S in sets.values():
        for _, par in S.rows:
            assert all(ev(0.0, float(L), S.residues) > par.e for L in {len(s) for s in S.seqs})


def test_gate_pairs_have_one_member_on_each_side(sets):
    """read from the reference's text: the passing member of every gate pair is there, the failing one is not"""
    rows_with_both = set()
    for name, S in sets.items():
        for row, present, absent in S.expect:
            have = {S.by_pair()[k] for k in records(fixture(name, row))}
            assert not [g for g in present if g not in have], (name, row, [g for g in present if g not in have])
            assert not [g for g in absent if g in have], (name, row, [g for g in absent if g in have])
            if present and absent:
                rows_with_both.add((name, row))
    S = sets["gates"]
    # every gate row has a member on each side, but the thresholds no positive score can fail: an identity of 0.6 or less scores 0
    no_failing_side = {"sid0.0", "sid0.5"}
    assert {r for r, _ in S.rows} - {r for n, r in rows_with_both if n == "gates"} == no_failing_side
    # ... and on both strands
    for row, present, absent in S.expect:
        for side in (present, absent):
            named = [g for g in side if g.endswith(("_fwd", "_rev"))]
            if named and not row.startswith("strict"):
                assert {g[-3:] for g in named} >= ({"fwd", "rev"} if len(named) > 1 else set()), (row, named)
    # the E-value pairs sit on the boundary by the host's arithmetic: the model's smallest passing score, and that score less 1
    for rn, e in rescorecases.EVALUE_ROWS:
        for L in rescorecases.EVALUE_LENGTHS:
            smin = rescore_model.min_passing_score(L, S.residues, e)
            for sn in ("fwd", "rev"):
                assert S.groups["ev_%s_L%d_min_%s" % (rn, L, sn)]["score"] == smin and S.groups["ev_%s_L%d_below_%s" % (rn, L, sn)]["score"] == smin - 1
                f = records(fixture("gates", rn))[(S.groups["ev_%s_L%d_min_%s" % (rn, L, sn)]["query"], S.groups["ev_%s_L%d_min_%s" % (rn, L, sn)]["target"])]
                assert float(f[3]) <= e


def test_geometry_classes_leave_records_on_both_strands(sets):
    """every length x diagonal class leaves a record on each strand under the loose -e - every member of the one-length sets does,
    the one-column overlaps on the largest diagonals and the overlaps of 2, 3, 4 and 8 columns included - and every member beyond
    the last diagonal leaves none; in the mixed-length set every class and every length, as query and as target, leaves records on
    each strand, and the three spellings of one diagonal give one answer"""
    pairs = 0
    for L in rescorecases.LENGTHS:
        T = sets["geometry_L%d" % L]
        got = {T.by_pair()[k] for k in records(fixture(T.name, "loose"))}
        strict = {T.by_pair()[k] for k in records(fixture(T.name, "e0.001"))}
        classes = {c for c, d in rescorecases.length_classes(L) if rescorecases.overlap(L, L, d)}
        assert classes >= {"d0", "dmax+", "dmax-"} and {g["cls"] for g in T.groups.values() if g["columns"]} == classes
        for n, g in T.groups.items():
            assert (n in got) == (g["columns"] > 0), n
            assert g["columns"] > 0 or n not in strict, n
            pairs += n in got
        # (a one-column overlap does depend on the loose -e: under -e 0.001 it is gone)
        assert not any(n in strict for n, g in T.groups.items() if g["columns"] == 1)
        assert {g["columns"] for g in T.groups.values()} >= {c for c in (1,) + rescorecases.FEW_COLUMNS if c < L or c == 1}
    assert pairs == sum(2 * len([1 for c, d in rescorecases.length_classes(L) if rescorecases.overlap(L, L, d)]) for L in rescorecases.LENGTHS)
    S = sets["geometry"]
    have = records(fixture("geometry", "loose"))
    got = {S.by_pair()[k] for k in have}
    seen = collections.defaultdict(bool)
    for n, g in S.groups.items():
        if g["cls"].startswith("beyond"):
            assert n not in got, n
            continue
        for key in (("query", g["qlen"], g["strand"]), ("target", g["tlen"], g["strand"]), (g["cls"], g["strand"])):
            seen[key] |= n in got
    assert all(seen.values()), sorted(k for k in seen if not seen[k])
    beyond = [n for n, g in S.groups.items() if g["cls"].startswith("beyond")]
    assert len(beyond) > 200 and not set(beyond) & {S.by_pair()[k] for k in records(fixture("geometry", "e0.001"))}
    n = 0
    for name, g in S.groups.items():
        if "same_as" in g:
            b = S.groups[g["same_as"]]
            mine, base = have.get((g["query"], g["target"])), have.get((b["query"], b["target"]))
            assert (mine is None) == (base is None) and (mine is None or mine[1:] == base[1:]), name
            n += mine is not None
    assert n >= 100
    # a transition and its transversion twin: one score (the reference's text has no purine/pyrimidine column)
    for name, g in S.groups.items():
        t = S.groups.get(name[:-3] + "_tv")
        if name.endswith("_ts") and t and (g["query"], g["target"]) in have:
            assert have[(g["query"], g["target"])][1:4] == have[(t["query"], t["target"])][1:4], name


def test_sweep_pins_every_quotient(sets):
    """the sweep's records carry (L - k) / L as the reference cuts it to three decimals, for every passing (L, k)"""
    S = sets["gates_sweep"]
    have = records(fixture("gates_sweep", "sid0.0"))
    quotients = set()
    for n, g in S.groups.items():
        f = have.get((g["query"], g["target"]))
        if f:
            assert int(f[8]) - int(f[7]) + 1 == g["columns"]
            quotients.add((g["columns"] - g["mismatches"], g["columns"]))
    assert len(quotients) > 4000 and {L for _, L in quotients} >= set(range(4, 151))


def test_letters_reach_their_cases(sets):
    S = sets["letters"]
    have = records(fixture("letters", "loose"))
    rec = lambda n: have[(S.groups[n]["query"], S.groups[n]["target"])]
    for n in ("star_only_identity", "heavy_n_identity"):
        assert rec(n)[4:6] == ["-1", "-1"] and rec(n)[7:9] == ["-1", "-1"] and rec(n)[2] == "1.00"
    # N over N: an identity on the forward strand, none on the reverse strand (the reversed query spells it X)
    assert rec("n_both_fwd")[2] == "1.00" and rec("n_both_rev")[2] == "0.983"
    # letters that score as a match and are different letters, and the other way round
    assert rec("iupac_R_over_G_fwd")[1] == rec("iupac_R_over_R_fwd")[1] and rec("iupac_R_over_G_fwd")[2] == "0.983" and rec("iupac_R_over_R_fwd")[2] == "1.00"
    assert rec("x_over_x_fwd")[2] == "1.00" and int(rec("x_over_x_fwd")[1]) < int(rec("iupac_R_over_R_fwd")[1])
    assert rec("lower_all_q_fwd")[2] == "1.00" and rec("lower_all_t_rev")[2] == "1.00"
    # '*' at an end of the overlap is left out of the coordinates; inside, or spelled X on the reverse strand, it is not
    assert rec("star_first_q_fwd")[4] == "1" and rec("star_last_t_fwd")[8] == "58" and rec("star_ends_t_rev")[7:9] == ["1", "58"]
    assert rec("star_inside_q_fwd")[7:9] == ["0", "59"] and rec("star_first_q_rev")[7:9] == ["0", "59"]
    assert rec("star_overlap_end_d-7_fwd")[7:9] == ["8", "58"] and rec("star_off_overlap_d5_fwd")[4:6] == ["5", "59"]
    # the N far from the overlap changes nothing (per-base path against the twin's word path)
    for n in S.groups:
        if n.startswith("far_n_"):
            assert rec(n)[1:3] == rec(n.replace("far_n_", "far_plain_"))[1:3] and rec(n)[2] == "1.00", n


def test_wrap_members_lie_on_their_diagonals(sets):
    """every wrap member leaves a record on its true diagonal; the repeats pick the probe their name says"""
    S = sets["wrap"]
    have = records(fixture("wrap", "sid0"))
    n_repeats = 0
    for n, g in S.groups.items():
        f = have[(g["query"], g["target"])]
        assert record_diagonal(f) == g["true_diagonal"], (n, record_diagonal(f), g["true_diagonal"])
        n_repeats += n.startswith("repeat_")
    assert n_repeats == 12
    assert {abs(g["true_diagonal"]) for n, g in S.groups.items() if n.startswith("wrap_")} == set(rescorecases.WRAP_DIAGONALS)
    lens = {len(s) for s in S.seqs}
    assert lens >= set(rescorecases.WRAP_LENGTHS)
    # the identity gate sees the saturating pair: 0.600 passes 0.0 and fails 0.9
    default = {S.by_pair()[k] for k in records(fixture("wrap", "default"))}
    assert "ry_saturates_65536" not in default and "ry_counts_60000" not in default and "wrap_d+131000_fwd" in default


def test_model_counts_purine_pyrimidine_mismatches(sets, scored):
    """the side-car's count on the members that carry transversions by construction"""
    S = sets["wrap"]
    by = {g: al for (_, _, _, _, g), al in zip(S.hits, scored["wrap"])}
    assert by["ry_saturates_65536"]["ry"] == 0xFFFF and by["ry_counts_60000"]["ry"] == 60000 and by["wrap_d+65536_fwd"]["ry"] == 1
    S = sets["geometry"]
    by = {g: al for (_, _, _, _, g), al in zip(S.hits, scored["geometry"])}
    for n, al in by.items():
        if al is not None:
            want = {"first_tv": 1, "last_tv": 1, "c15ts_c16tv": 1, "c15tv_c16ts": 1, "three_tv": 3}.get(S.groups[n].get("variant"), 0)
            assert al["ry"] == want, n
    S = sets["letters"]
    assert all(al is None or al["ry"] == (0 if n.startswith("far_plain") else 0xFFFF) for (_, _, _, _, n), al in zip(S.hits, scored["letters"]))
