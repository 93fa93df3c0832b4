"""The directed contig-merge cases (tests/contigcases.py) on the CPU: the generator against the committed inputs, the oracle against what
the reference's object code made of them (tests/golden/contig_directed/), and the conditions that keep the cases from being vacuous -
the outcomes on the reference's output alone, what happened on the way (heap sizes, middle-zone comparisons, rounds, skips,
re-alignments) on the oracle's event log (ORACLE_CONTIG_LOG), which is only read where the oracle's output equals the reference's."""
import collections
import gzip
import os

import pytest

import contigcases as cc
from carpedeam_amd import mmdb
from contigcases import DIR, fixture
from correctcases import revcomp
from gpuutil import diff_keys

NAMES = [n for n, _, _ in cc.SETS]
REF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "carpedeam_ref")
needs_ref = pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref (the reference's object code) is not built here")


@pytest.fixture(scope="module")
def sets():
    return {name: make() for name, make, _ in cc.SETS}


def outcome(S, db):
    """group name -> (side, output length, letters added left, letters added right) in a keyed DB"""
    db = mmdb.canon(db)
    return {g["name"]: cc.sides(S, g, *db[g["key"]]) for g in S.groups}


@pytest.fixture(scope="module")
def reference(sets):
    return {name: outcome(sets[name], fixture(name, "cmerge")) for name in NAMES}


@pytest.fixture(scope="module")
def oracle_runs(oracle_bin, dhigh_prefix, tmp_path_factory):
    d = tmp_path_factory.mktemp("contig_directed")
    return {name: cc.run_oracle_on_fixture(oracle_bin, dhigh_prefix, d, name, msl) for name, _, msl in cc.SETS}


def events_of(sets, oracle_runs, name):
    """group name -> Events of its query"""
    ev = oracle_runs[name][1]
    return {g["name"]: ev.get(g["key"], cc.Events()) for g in sets[name].groups}


@pytest.mark.parametrize("name", NAMES)
def test_generator_reproduces_committed_inputs(sets, name):
    S = sets[name]
    for keyed, fn in ((S.seq_keyed(), "corr"), (S.aln_keyed(), "aln")):
        lines = []
        for k in sorted(keyed):
            lines += ["#%d\t%d" % (k, keyed[k][1]), keyed[k][0].decode("latin1").rstrip("\n")]
        assert ("\n".join(lines) + "\n").encode("latin1") == gzip.open(os.path.join(DIR, name, fn + ".keyed.gz"), "rb").read(), fn


def test_fixture_files_are_small():
    total = 0
    for name in NAMES:
        assert sorted(os.listdir(os.path.join(DIR, name))) == ["aln.keyed.gz", "cmerge.keyed.gz", "corr.keyed.gz"], name
        for fn in os.listdir(os.path.join(DIR, name)):
            size = os.path.getsize(os.path.join(DIR, name, fn))
            assert size < 100_000, (name, fn, size)
            total += size
    assert total < 600_000 and sorted(os.listdir(DIR)) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_fixture(sets, oracle_runs, name):
    out, events = oracle_runs[name]
    bad = diff_keys(out, fixture(name, "cmerge"))
    by_key = {g["key"]: g["name"] for g in sets[name].groups}
    assert not bad, "oracle differs from the reference in groups %s" % sorted({by_key.get(k, "target %d" % k) for k in bad})
    # the event log: queries of the set's groups alone (a target's only record is its own), every gated record a record of the query
    S = sets[name]
    assert set(events) <= set(by_key), sorted(set(events) - set(by_key))[:5]
    for g in S.groups:
        targets = {int(l.split("\t")[0]) for l in S.recs[g["query"]]}
        e = events.get(g["key"], cc.Events())
        assert {t for t, _, _ in e.gated} <= targets and {t for _, t in e.pops} <= targets, g["name"]
        # (every gated record is popped unless --max-seq-len ends the loop on a queue that is not empty)
        assert (len(e.pops) >= len(e.gated) or any(b[3] > 0 for b in e.breaks)) and [r[0] for r in e.rounds] == list(range(len(e.rounds))), g["name"]


def aligned_columns(S, line, q):
    """a record's columns as the reference walks them: [(query letter, target letter)] with a reverse target reverse-complemented"""
    f = line.split("\t")
    t, qs, qe, ds, de, tlen = int(f[0]), int(f[4]), int(f[5]), int(f[7]), int(f[8]), int(f[9])
    target = S.seqs[t]
    if qs > qe:
        qs, qe, ds, de, target = qe, qs, tlen - de - 1, tlen - ds - 1, revcomp(target)
    return [(S.seqs[q][qs + i], target[ds + i]) for i in range(qe - qs + 1)]


def test_domain_rules(sets):
    extra = [("handback", cc.handback_set()), ("refusal_0", cc.refusal_set(0)), ("tables", cc.tables_set())]
    for name, S in list(sets.items()) + extra:
        keys = S.keys
        assert sorted(set(keys)) == sorted(keys)
        twice = {(g["query"], g["twice"]) for g in S.groups if "twice" in g}
        for q, recs in S.recs.items():
            ts = [int(l.split("\t")[0]) for l in recs]
            assert q in ts, (name, q)                                      # every sequence has its self record
            dup = {t for t, n in collections.Counter(ts).items() if n > 1}
            assert {(q, t) for t in dup} <= twice, (name, q)               # one record per (query, target) pair but for use_reverse_last
            qlen = len(S.seqs[q])
            for l in recs:
                f = l.split("\t")
                t, qs, qe, ql, ds, de, tl = int(f[0]), int(f[4]), int(f[5]), int(f[6]), int(f[7]), int(f[8]), int(f[9])
                assert min(qs, qe, ds, de) >= 0 and ql == qlen and tl == len(S.seqs[t]) and abs(qe - qs) == de - ds and max(qs, qe) < ql and de < tl
            assert not cc.overhang_beyond_query(S, q), (name, q)           # the overhang never exceeds the query
    assert cc.overhang_beyond_query(cc.refusal_set(1), 0)                  # ... but for the one case made for it, by one letter
    S0, S1 = cc.refusal_set(0), cc.refusal_set(1)
    assert len(S0.seqs[1]) - 100 == len(S0.seqs[0]) and len(S1.seqs[1]) - 100 == len(S1.seqs[0]) + 1
    assert sum(len(S.seqs) for S in sets.values()) < 6000
    assert sum(1 for v in sets["wide"].recs.values() if len(v) > 1) == cc.WIDE_QUERIES and cc.WIDE_QUERIES % 64 != 0
    # parked counts of the wide set differ within every wave of 64 consecutive active queries
    parked = [g["parked"] for g in sets["wide"].groups]
    assert all(set(parked[w:w + 64]) == {0, 1, 5} for w in range(0, cc.WIDE_QUERIES, 64))
    # the tables set: both overlaps beyond 2^18 columns, so the comparator's xHit + yHit leaves lgammaf's table [1, 2^19)
    T = cc.tables_set()
    cols = sorted(int(l.split("\t")[8]) - int(l.split("\t")[7]) + 1 for l in T.recs[0] if int(l.split("\t")[0]) != 0)
    assert len(cols) == 2 and cols[0] > 1 << 18 and len(T.seqs[0]) + 40 < cc.TABLES_MAX_SEQ_LEN


def test_groups_come_out_as_stated(sets, reference):
    for name in NAMES:
        S, out = sets[name], reference[name]
        wrong = [(g["name"], g["expect"], out[g["name"]][0]) for g in S.groups if g["expect"] is not None and out[g["name"]][0] != g["expect"]]
        assert not wrong, (name, wrong)
        wrong = [(g["name"], g["length"], out[g["name"]][1]) for g in S.groups if g["length"] is not None and out[g["name"]][1] != g["length"]]
        assert not wrong, (name, wrong)
        assert not [g["name"] for g in S.groups if g["expect"] is None and "order_family" not in g], name
        # a sequence that is no group's query is a target with its self record alone: untouched
        res, corr = mmdb.canon(fixture(name, "cmerge")), mmdb.canon(fixture(name, "corr"))
        queries = {g["key"] for g in S.groups}
        assert all(res[k] == corr[k] for k in corr if k not in queries), name
    # useReverse from the LAST record of the target: the fragment is the reverse complement of the target's first 25 letters
    S = sets["letters"]
    g = next(g for g in S.groups if g["name"] == "use_reverse_last")
    assert reference["letters"]["use_reverse_last"][3] == revcomp(S.seqs[g["twice"]][:25]) != S.seqs[g["twice"]][-25:]


def test_gate_pairs_have_one_member_on_each_side(sets, reference):
    """every `in` member grows by more letters than every `out` member of its pair, on the reference's output"""
    seen = 0
    for name in NAMES:
        S, out = sets[name], reference[name]
        qlen = {g["name"]: len(S.seqs[g["query"]]) for g in S.groups}
        for pair, m in cc.gate_pairs(S).items():
            assert m["in"] and m["out"], (name, pair)
            for i in m["in"]:
                for o in m["out"]:
                    assert out[i][0] != "none" and out[i][1] - qlen[i] > out[o][1] - qlen[o], (name, pair, i, o)
            seen += 1
    # stats: 4 paths x 2 sides x 8 lengths less the reverse record of one column, and the two mirrored-N pairs
    assert len(cc.gate_pairs(sets["stats"])) == 4 * 2 * 8 - 2 + 2 and seen == 64 + 9 + 5 + 2


def test_stats_siblings_differ_in_the_intended_column(sets, oracle_runs):
    """the mismatching columns of `out` are those of `in` and the one intended column (the last, or column 0); the N-free column count of
    every `in` member as the oracle logs it"""
    S = sets["stats"]
    events = events_of(sets, oracle_runs, "stats")
    by = {g["name"]: g for g in S.groups}

    def mismatches(g):
        line = next(l for l in S.recs[g["query"]] if int(l.split("\t")[0]) != g["query"])
        cols = aligned_columns(S, line, g["query"])
        return {i for i, (a, b) in enumerate(cols) if a != b}, sum(1 for a, b in cols if a == ord("N") or b == ord("N")), len(cols)

    n_pairs = 0
    for pair, m in cc.gate_pairs(S).items():
        if pair.startswith("stats_rev_n"):
            continue
        (i,) = m["in"]
        mm_in, n_in, cols = mismatches(by[i])
        assert len(mm_in) == cc.kmax(cols) and not ({0, cols - 1} & mm_in) or cols == 1, i
        for o in m["out"]:
            mm_out, _, cols_out = mismatches(by[o])
            assert cols_out == cols and mm_out - mm_in == {0 if o.endswith("out0") else cols - 1} and mm_in <= mm_out, (pair, o)
        gated = events[i].gated
        assert len(gated) == 1 and gated[0][1] == cols - n_in, (i, gated)
        assert not events[m["out"][0]].gated
        n_pairs += 1
    assert n_pairs == 62
    paths = collections.Counter(g["pair"][0].split("_")[1] for g in S.groups if g.get("pair"))
    assert set(paths) == {"fast", "qn", "tn", "rev"}
    # overlaps that end on the last letter of sequences whose lengths are 0, 1 and 15 mod 16, on the fast path
    ends = set()
    for g in S.groups:
        if g["name"].startswith("stats_fast_") and g["name"].endswith("_in"):
            side = g["name"].split("_")[2]
            t = next(int(l.split("\t")[0]) for l in S.recs[g["query"]] if int(l.split("\t")[0]) != g["query"])
            ends.add((side, len(S.seqs[g["query"] if side == "right" else t]) % 16))
    assert {("right", 0), ("right", 1), ("right", 15)} <= ends and len({r for s, r in ends if s == "left"}) >= 3, ends


def test_damage_columns_decide_the_donor(sets, reference):
    """C over T and G over A count, their converses do not: the donor changes with one column, and with the kind of the two"""
    S, out = sets["stats"], reference["stats"]
    donor = {}
    for g in S.groups:
        if "damage" in g:
            donor[g["damage"]] = g["tails"].index(out[g["name"]][3])
    pairs = sorted({(c1, c2) for c1, c2, _ in donor})
    assert pairs == [(0, 15), (0, 199), (15, 16), (16, 199)]
    for c1, c2 in pairs:
        d = {tag: donor[(c1, c2, tag)] for tag in ("dmg", "conv1", "conv2", "none", "ctct", "gaga")}
        assert d["dmg"] != d["conv1"] and d["dmg"] != d["conv2"] and d["ctct"] != d["gaga"], (c1, c2, d)


def test_heap_families_show_the_heap_order(sets, reference, oracle_runs):
    """the donating target differs between at least two sibling record orders of every family; every stated queue length occurs, and the
    comparator meets the middle zone with alnLengthCons smaller, equal and larger"""
    seen = 0
    for name in ("heap", "gates"):
        fam = collections.defaultdict(dict)
        for g in sets[name].groups:
            if "tie" in g:
                side, _, l, r = reference[name][g["name"]]
                added = [r, l] if g["tie"][0] == "both" else [r] if g["tie"][0] == "right" else [l]
                assert all(x in g["tails"] for x in added), g["name"]
                fam[g["name"].rsplit("_", 1)[0]][g["name"]] = tuple(g["tails"].index(x) for x in added)
        for f, donors in fam.items():
            if len(donors) > 1:
                assert len(set(donors.values())) >= 2, (name, f, donors)
                seen += 1
    # sizes 2 .. 8 on both sides, 33 and 200 on the right, the families of both sides in one queue, the family with zero keys
    assert seen == 2 * 6 + 2 + len(cc.MIXED_SIZES) + 1
    events = events_of(sets, oracle_runs, "heap")
    sizes = collections.Counter(len(e.gated) for e in events.values())
    assert set(cc.HEAP_SIZES) <= set(sizes), sizes
    for g in sets["heap"].groups:
        assert len(events[g["name"]].gated) == g["heap"] == len(events[g["name"]].pops), g["name"]
    zone = collections.Counter("<" if a < b else "=" if a == b else ">" for e in events.values() for a, b, _ in e.zone)
    assert min(zone["<"], zone["="], zone[">"]) >= 10, zone
    assert all(0.45 <= p <= 0.55 for e in events.values() for _, _, p in e.zone)
    # the records with a zero key are in the queue of the `neither` family and popped
    ev = events_of(sets, oracle_runs, "gates")
    for g in sets["gates"].groups:
        if g["name"].startswith("neither_mixed"):
            assert sorted(c for _, c, _ in ev[g["name"]].gated)[:4] == [0, 0, 0, 0] and len(ev[g["name"]].pops) == 7, g["name"]


def test_rounds_as_stated(sets, reference, oracle_runs):
    for name in ("rounds", "letters", "maxlen", "wide"):
        S, out, events = sets[name], reference[name], events_of(sets, oracle_runs, name)
        for g in S.groups:
            e = events[g["name"]]
            if "rounds" in g:
                assert len(e.rounds) == g["rounds"], (g["name"], len(e.rounds))
            if "round1" in g:
                # a parked group outgrows its first round - or its parked hit provably fails its re-alignment
                first = e.rounds[0]
                assert len(S.seqs[g["query"]]) + first[1] + first[2] == g["round1"], g["name"]
                if g.get("parked_fails"):
                    assert out[g["name"]][1] == g["round1"] and e.realigned and not any(a[-1] for a in e.realigned), g["name"]
                elif g.get("rounds", 1) > 1 or g.get("parked_fails") is False:
                    assert out[g["name"]][1] > g["round1"] and any(a[-1] for a in e.realigned), g["name"]
            if "neither" in g:
                assert len(e.neither) == g["neither"], g["name"]
    events = events_of(sets, oracle_runs, "rounds")
    assert len(events["ladder"].rounds) >= 20 and all(r[1] + r[2] == 5 for r in events["ladder"].rounds)
    # each skip rule at equality, and one letter beyond it parked
    for side, tag in (("right", "R"), ("left", "L")):
        assert [(s[2], s[3] == s[4]) for s in events["skip_eq_" + side].skips] == [(tag, True)]
        assert not events["skip_plus1_" + side].skips and len(events["skip_plus1_" + side].realigned) == 1
    # re-alignment on a negative diagonal (left) and on a positive one that holds leftOff (right, after growth on both sides)
    diags = {a[1]: a[2] for a in events["parked_both"].realigned}
    assert len(diags) == 2 and min(diags.values()) < 0 < max(diags.values()) and events["parked_both"].rounds[0][1] > 0
    assert max(diags.values()) == 180 - 100 + events["parked_both"].rounds[0][1]
    # the pass at exactly 0.99f, the two-column overlap (identity over one column), 1024 and 1025 columns
    for side in ("right", "left"):
        (a,) = events["realign_pass_" + side].realigned
        assert a[4] - a[3] == 100 and abs(a[7] - 0.99) < 1e-6 and a[-1] == 1
        (a,) = events["realign_fail_" + side].realigned
        assert a[4] - a[3] == 100 and abs(a[7] - 0.98) < 1e-6 and a[-1] == 0
    (a,) = events["realign_2col"].realigned
    assert a[4] - a[3] == 1 and a[7] == 1.0
    assert sorted(a[4] - a[3] + 1 for n in ("realign_1024", "realign_1025", "realign_1024_left") for a in events[n].realigned) == [1024, 1024, 1025]
    # the last column decides for the RY classes, not for the letters: 99/100 both, 100/101 against 99/101
    (a,), (b,) = events["ry_last_in_right"].realigned, events["ry_last_out_right"].realigned
    assert a[7] == b[7] and abs(a[7] - 0.99) < 1e-6 and a[8] > 0.99 > b[8] and (a[-1], b[-1]) == (1, 0)
    # --max-seq-len: the break with the queue not empty and on the last element
    events = events_of(sets, oracle_runs, "maxlen")
    assert [b[3] > 0 for b in events["break_queue_not_empty"].breaks] == [True] and not events["break_queue_not_empty"].realigned
    assert [b[3] > 0 for b in events["grow_then_break_not_empty"].breaks] == [True] and events["grow_then_break_not_empty"].rounds[0][3] == 1
    assert not events["grow_then_break_not_empty"].realigned
    assert [b[3] for b in events["grow_then_break_last"].breaks] == [0] and len(events["grow_then_break_last"].realigned) == 1
    assert [b[0] for b in events["parked_at_bound"].breaks] == [1] and not events["no_break"].breaks
    # the break_order families: every member breaks on the left candidate, and the orders of a family end at more than one length
    by_family = collections.defaultdict(set)
    for g in sets["maxlen"].groups:
        if "order_family" in g:
            assert [b[2] for b in events[g["name"]].breaks] == ["L"] and len(events[g["name"]].gated) == g["order_family"], g["name"]
            by_family[g["order_family"]].add(reference["maxlen"][g["name"]][1])
    assert sorted(by_family) == list(cc.BREAK_ORDER_SIZES) and sum(len(v) > 1 for v in by_family.values()) >= 4, by_family
    # the wide set: parked counts as stated, more than one round count
    events = events_of(sets, oracle_runs, "wide")
    assert all(events[g["name"]].rounds[0][3] == g["parked"] for g in sets["wide"].groups)
    assert len({len(e.rounds) for e in events.values()}) >= 3
    # a query without N gains one and its parked hit is re-aligned across it
    events = events_of(sets, oracle_runs, "letters")
    for g in sets["letters"].groups:
        if g["name"].startswith("gains_n_"):
            assert b"N" not in sets["letters"].seqs[g["query"]] and b"N" in reference["letters"][g["name"]][2 if g["name"].endswith("left") else 3]
            (a,) = events[g["name"]].realigned
            # (an N over a letter differs; an N over the parked target's own N is an equal letter)
            assert a[-1] == 1 and (a[7] < 1.0) == ("_letter_" in g["name"]), g["name"]


def test_unsafe_filter_keeps_the_set(sets):
    """the --unsafe 1 rows run the `main` sets less what the device refuses - a target that overhangs its query by more than the query's
    length: from the geometry alone, nothing of these sets"""
    for name in cc.MAIN:
        S = sets[name]
        _, aln, refused = cc.without_unsupported(S)
        assert refused == 0 and refused < len(S.groups) / 4
        assert sum(1 for v in aln.values() if v[0]) == sum(1 for v in S.recs.values() if v)


@needs_ref
def test_oracle_matches_live_reference_on_handback_and_unsafe_rows(sets, oracle_bin, dhigh_prefix, tmp_path):
    S = cc.handback_set()
    o, _ = cc.run_oracle_on(oracle_bin, dhigh_prefix, tmp_path, "handback", S.seq_keyed(), S.aln_keyed(), 200000)
    r, _ = cc.run_oracle_on(REF, dhigh_prefix, tmp_path, "handback", S.seq_keyed(), S.aln_keyed(), 200000, exe_name="ref")
    assert not diff_keys(o, r)
    assert all(v[0] == "right" for v in outcome(S, r).values())
    differ = 0
    for name in cc.MAIN:
        seq, aln, _ = cc.without_unsupported(sets[name])
        for min_cov in (1, 2, 5):
            o, _ = cc.run_oracle_on(oracle_bin, dhigh_prefix, tmp_path, "%s_%d" % (name, min_cov), seq, aln, 200000, 1, min_cov)
            r, _ = cc.run_oracle_on(REF, dhigh_prefix, tmp_path, "%s_%d" % (name, min_cov), seq, aln, 200000, 1, min_cov, exe_name="ref")
            by_key = {g["key"]: g["name"] for g in sets[name].groups}
            bad = diff_keys(o, r)
            assert not bad, (name, min_cov, sorted(by_key.get(k, k) for k in bad))
            differ += len(diff_keys(r, fixture(name, "cmerge")))
    assert differ > 0                       # (the mode changes something on these sets)
