"""The directed extender cases (tests/extendcases.py) on the CPU: the generator against the committed inputs, the oracle against what
the reference's object code made of them (tests/golden/extend_directed/), and the conditions that keep the cases from being
vacuous - checked on the reference's output alone (the record and candidate counts of the deep groups on the generator and on
the oracle's score log)."""
import collections
import gzip
import os

import pytest

import extendcases
from carpedeam_amd import mmdb
from extendcases import DIR, fixture, run_oracle_on_fixture
from gpuutil import diff_keys

NAMES = [n for n, _, _ in extendcases.SETS]


@pytest.fixture(scope="module")
def sets():
    return {name: make() for name, make, _ in extendcases.SETS}


def outcome(S, asm):
    """group name -> (side, output length, letters added left, letters added right) in a keyed assembly DB"""
    asm = mmdb.canon(asm)
    return {g["name"]: extendcases.sides(S, g, *asm[g["key"]]) for g in S.groups}


@pytest.fixture(scope="module")
def reference(sets):
    return {name: outcome(sets[name], fixture(name, "asm")) for name in NAMES}


@pytest.fixture(scope="module")
def oracle_runs(oracle_bin, dhigh_prefix, tmp_path_factory):
    d = tmp_path_factory.mktemp("extend_directed")
    return {name: run_oracle_on_fixture(oracle_bin, dhigh_prefix, d, name, msl) for name, _, msl in extendcases.SETS}


@pytest.mark.parametrize("name", NAMES)
def test_generator_reproduces_committed_inputs(sets, name):
    S = sets[name]
    for keyed, fn in ((S.seq_keyed(), "corr"), (S.aln_keyed(), "aln")):
        lines = []
        for k in sorted(keyed):
            lines += ["#%d\t%d" % (k, keyed[k][1]), keyed[k][0].decode("latin1").rstrip("\n")]
        assert ("\n".join(lines) + "\n").encode("latin1") == gzip.open(os.path.join(DIR, name, fn + ".keyed.gz"), "rb").read(), fn


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_fixture(sets, oracle_runs, name):
    asm, scores = oracle_runs[name]
    bad = diff_keys(asm, fixture(name, "asm"))
    by_key = {g["key"]: g["name"] for g in sets[name].groups}
    assert not bad, "oracle differs from the reference in groups %s" % sorted({by_key.get(k, "target %d" % k) for k in bad})
    # the score log: finite sums, ratios in [0, 1], queries and targets of the set
    keys = set(sets[name].keys)
    for (q, t), (s, r) in scores.items():
        assert q in keys and t in keys and s <= 0.0 and 0.0 <= r <= 1.0, (q, t, s, r)
    assert (len(scores) > 0) == (name != "lonely")


def test_domain_rules(sets):
    for name, S in sets.items():
        keys = S.keys
        assert sorted(set(keys)) == sorted(keys)
        for q, recs in S.recs.items():
            ts = [int(l.split("\t")[0]) for l in recs]
            assert len(ts) == len(set(ts)), (name, q)                     # one record per (query, target) pair
            qlen = len(S.seqs[q])
            for l in recs:
                f = l.split("\t")
                t, qs, qe, ql, ds, de, tl = int(f[0]), int(f[4]), int(f[5]), int(f[6]), int(f[7]), int(f[8]), int(f[9])
                assert min(qs, qe, ds, de) >= 0 and ql == qlen and tl == len(S.seqs[t]) and abs(qe - qs) == de - ds and max(qs, qe) < ql and de < tl
                assert tl - (de - ds + 1) <= qlen or qs > qe              # the overhang never exceeds the query
        run = next((g for g in S.groups if g["name"] == "gap_run"), None)
        no_self = {q for q, recs in S.recs.items() if not any(int(l.split("\t")[0]) == q for l in recs)}
        allowed = set(range(run["query"], run["query"] + run["run"])) if run else set()
        assert no_self <= allowed | (set(S.recs) if name == "lonely" else set()), (name, sorted(no_self - allowed)[:5])
    # ids are ranks of keys: in the two keys sets the lying target's id is its query's key
    for name in ("keys_plus1", "keys_sparse"):
        S = sets[name]
        keys = S.keys
        rank = {k: i for i, k in enumerate(sorted(keys))}
        assert S.lies and all(rank[keys[t]] == keys[q] for q, t in S.lies), name
        assert keys != sorted(keys) or name == "keys_plus1"
    assert sum(len(S.seqs) for S in sets.values()) < 6000


def test_groups_come_out_as_stated(sets, reference):
    unstated = []
    for name in NAMES:
        S, out = sets[name], reference[name]
        wrong = [(g["name"], g["expect"], out[g["name"]][0]) for g in S.groups if g["expect"] is not None and out[g["name"]][0] != g["expect"]]
        assert not wrong, (name, wrong)
        wrong = [(g["name"], g["length"], out[g["name"]][1]) for g in S.groups if g["length"] is not None and out[g["name"]][1] != g["length"]]
        assert not wrong, (name, wrong)
        unstated += [(name, g["name"]) for g in S.groups if g["expect"] is None]
        # a sequence that is no group's query is a target with its self record alone: untouched
        asm, corr = mmdb.canon(fixture(name, "asm")), mmdb.canon(fixture(name, "corr"))
        queries = {g["key"] for g in S.groups}
        assert all(asm[k] == corr[k] for k in corr if k not in queries), name
    assert sorted(unstated) == [("keys_plus1", "lie_high"), ("keys_plus1", "lie_low"), ("keys_sparse", "lie_high"), ("keys_sparse", "lie_low")]
    # what the reference does on the lying pair: it takes the text value where the target's id is the query's key.  lie_low (perfect
    # letters under the text 0.500) is turned away; lie_high (32/40 under 1.000) is let in and its 40 columns cost the honest 30-column
    # candidate beside it ten columns of excess - neither extends, where either would by its letters
    for name in ("keys_plus1", "keys_sparse"):
        assert reference[name]["lie_low"][0] == "none" and reference[name]["lie_high"][0] == "none"
    assert reference["main"]["text_low_letters_good"][0] == "right"
    # ... and where it is not, the letters decide: the 32/40 candidate under the text 1.000 stays out, so the honest 30-column
    # candidate beside it pays no excess and donates its own letters
    g = next(g for g in sets["main"].groups if g["name"] == "text_good_letters_low")
    assert reference["main"]["text_good_letters_low"][3] == g["honest"]
    for name in ("lonely",):
        assert mmdb.canon(fixture(name, "asm")) == mmdb.canon(fixture(name, "corr"))
    assert len([g for g in sets["single"].groups]) == 1 and sum(len(v) > 1 for v in sets["single"].recs.values()) == 1
    assert all(len(v) <= 1 for v in sets["lonely"].recs.values())


def test_gate_pairs_have_one_member_on_each_side(sets, reference):
    out = reference["main"]
    for inside, outside in extendcases.GATE_PAIRS:
        assert inside in out and outside in out, (inside, outside)
        assert out[inside][0] != "none" and out[outside][0] == "none", (inside, outside)
    for name in ("keys_plus1", "keys_sparse"):
        for inside, outside in extendcases.GATE_PAIRS:
            if inside in reference[name] and outside in reference[name]:
                assert reference[name][inside][0] != "none" and reference[name][outside][0] == "none", (name, inside, outside)
    # --max-seq-len: at the bound the second piece is refused, one letter below it is taken
    m = reference["maxlen"]
    assert m["maxlen_at"][:2] == ("right", 100) and m["maxlen_below"][:2] == ("both", extendcases.MAXLEN_BOUND - 1)
    assert m["maxlen_first_at"][0] == "none" and m["maxlen_first_below"][1] == extendcases.MAXLEN_BOUND - 1


def test_tie_groups_show_the_heap_order(sets, reference):
    """the donating target (the overhang found in the output) differs between at least two sibling record orders of every family"""
    seen = 0
    for name in ("main", "keys_plus1", "keys_sparse"):
        fam = collections.defaultdict(dict)
        for g in sets[name].groups:
            if "tie" in g:
                side, _, l, r = reference[name][g["name"]]
                added = r if g["tie"][0] == "right" else l
                assert added in g["tails"], g["name"]
                fam[g["name"].rsplit("_", 1)[0]][g["name"]] = g["tails"].index(added)
        for f, donors in fam.items():
            assert len(donors) >= 2 and len(set(donors.values())) >= 2, (name, f, donors)
            seen += 1
        if name == "main":
            assert {2, 3, 5, 9} <= {g["tie"][1] for g in sets[name].groups if "tie" in g}
            # the better pair of tie_top2 donates, never one of the three with a substitution
            assert all(d in (1, 3) for n, d in fam["tie_top2"].items())
    assert seen >= 11


def test_near_tie_groups_tie_exactly(sets, oracle_runs):
    """the two candidates of every near-tie group have bit-equal scores in the oracle's (the reference's) long double arithmetic"""
    scores, n = oracle_runs["main"][1], 0
    for g in sets["main"].groups:
        if g["name"].startswith("near_tie_"):
            mine = [v[0] for (q, _), v in scores.items() if q == g["key"]]
            assert len(mine) == 2 and mine[0] == mine[1], (g["name"], mine)
            n += 1
    assert n == 2 * len(extendcases.NEAR_TIE_COLUMNS)


def test_parked_groups_outgrow_their_first_round(sets, reference):
    by = {g["name"]: g for g in sets["main"].groups}
    for n in extendcases.PARKED:
        assert reference["main"][n][1] > by[n]["round1"], n
    # a third round: two candidates parked behind the first
    assert reference["main"]["parked3_right"][1] == by["parked3_right"]["round1"] + 40
    # the twins: dropped at an overhang equal to the piece, and where the re-aligned identity fails
    for side in ("right", "left"):
        assert reference["main"]["skip_off_eq_" + side][1] == by["skip_off_eq_" + side]["round1"]
        # 62/70 after re-alignment: not queued again; 63/70 = 0.9f: queued and used
        assert reference["main"]["parked_fail_id_" + side][1] == by["parked_fail_id_" + side]["round1"]
        assert reference["main"]["parked_pass_id_" + side][1] == by["parked_pass_id_" + side]["round1"] + 20


def test_deep_groups_have_their_counts(sets, oracle_runs):
    S = sets["main"]
    by = {g["name"]: g for g in S.groups}
    for n, records in extendcases.DEEP_RECORDS.items():
        assert by[n]["records"] == records, n
    scored = collections.Counter(q for q, _ in oracle_runs["main"][1])
    assert scored[by["deep_lcap"]["key"]] > 1024                       # beyond the LDS list of the record kernel
    assert scored[by["deep_32"]["key"]] == 32 and scored[by["deep_33"]["key"]] == 33 and scored[by["deep_100"]["key"]] == 99
    # ... and all of them enter the queue (sRatio above the threshold 0.5): 32 | 33 straddle the record form's all-pairs switch
    queued = collections.Counter(q for (q, _), (_, ratio) in oracle_runs["main"][1].items() if ratio > 0.5)
    assert queued[by["deep_32"]["key"]] == 32 and queued[by["deep_33"]["key"]] == 33
    assert scored[by["deep_449"]["key"]] == 448 and scored[by["deep_900"]["key"]] == 899
    # the last length bin starts at 248 columns
    for n in (247, 248, 400):
        recs = S.recs[by["bin_%d" % n]["query"]]
        assert sorted(int(l.split("\t")[8]) - int(l.split("\t")[7]) + 1 for l in recs)[:2] == [n, n]
    # the run without records: more than 512 sequences, starting inside a window of 448 records that also holds an active query
    run = by["gap_run"]
    assert run["run"] > 512 and all(not S.recs[q] for q in range(run["query"], run["query"] + run["run"]))
    first_rec = lambda q: sum(len(S.recs[i]) for i in range(q))
    assert first_rec(by["gap_before"]["query"]) // 448 == first_rec(run["query"]) // 448 and first_rec(run["query"]) % 448 != 0
    # record ranges on word boundaries of the push bits
    ends = set()
    for g in S.groups:
        if g["name"].startswith("bits_"):
            assert first_rec(g["query"]) == g["r0"]
            ends.add((g["r0"] % 32, (g["r0"] + g["records"]) % 32))
    assert {(0, 0), (0, 31), (0, 1), (1, 0), (31, 0), (31, 31)} <= ends, ends


def test_unsafe_filter_keeps_most_of_the_set(sets):
    """the device refuses --unsafe 1 where a target overhangs the query by more than the query's length, and the run leaves out the
    queries of more than 128 records: from the geometry alone, the filter takes out less than a quarter of the main set's groups - no
    group for its overhang, the three deepest for their depth"""
    S = sets["main"]
    _, aln, refused, deep = extendcases.without_unsupported(S)
    assert refused == 0 and deep == 3 and refused + deep < len(S.groups) / 4
    assert sum(1 for v in aln.values() if v[0]) == sum(1 for v in S.recs.values() if v) - refused - deep
