"""tests/links_model.py against the links, totals and statistics that tests/linkcases.py writes out by hand, against a second, literal
restatement of the pairing on the random sets, and its three file writers against lines written by hand.  No device."""
import numpy as np
import pytest

import linkcases as lc
import links_model as lm

FIELDS = ("a", "b", "info", "reads", "forward", "mode_reads", "gap_mode", "gap_min", "gap_max", "gap_sum")


def model(c, queries=None, **par):
    p = dict(c["par"])
    p.update(par)
    return lm.links(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"] if queries is None else queries, min_seq_id=c["min_seq_id"], skip=c["skip"], **p)


def as_tuples(found):
    return [tuple(int(k[f]) for f in FIELDS) for k in found]


def test_the_record_has_48_bytes():
    assert lm.LINK_DTYPE.itemsize == 48 and lm.LINK_DTYPE.fields["gap_sum"][1] == 40 and lm.LINK_DTYPE.fields["gap_mode"][1] == 24


@pytest.mark.parametrize("name,make", lc.DIRECTED, ids=[n for n, _ in lc.DIRECTED])
def test_directed_cases(name, make):
    c = make()
    stats, totals, found = model(c)
    assert as_tuples(found) == c["links"]
    assert (found["reserved"] == 0).all() and found.dtype == lm.LINK_DTYPE
    if "totals" in c:
        assert totals.tolist() == c["totals"]
    for x, cols in c.get("stats", {}).items():
        for col, v in cols.items():
            assert int(stats[x, col]) == v, (name, x, col)
    # what holds of every result
    assert int(totals[0]) == int(stats[:, 2:4].sum()) and int(totals[4]) >= len(found) and int(totals[3]) >= int(found["reads"].sum())
    assert int(stats[:, 5].sum()) == 2 * len(found)
    assert ((found["gap_min"] <= found["gap_mode"]) & (found["gap_mode"] <= found["gap_max"]) & (found["a"] < found["b"]) & (found["forward"] <= found["reads"])).all()


def test_a_read_and_its_reverse_complement_land_on_one_link():
    c = lc.four_edges()
    _, _, found = model(c)
    assert found["reads"].tolist() == [2] * 4 and found["forward"].tolist() == [1] * 4 and found["info"].tolist() == [0, 2, 1, 3]


def test_the_thresholds_one_step_further():
    """thresholds() at overhang 2 and at anchor 15: the read that was a letter or a column short makes its pair"""
    c = lc.thresholds()
    assert as_tuples(model(c, overhang=2)[2]) == [(0, 1, 0, 2, 2, 1, -14, -14, -13, -27)]
    assert as_tuples(model(c, anchor=15)[2]) == [(0, 1, 0, 2, 2, 1, -13, -13, -12, -25)]
    assert len(model(c, overhang=4)[2]) == 0 and len(model(c, anchor=17)[2]) == 0


def test_max_ends_one_step_either_way():
    c = lc.crowded()
    _, totals, found = model(c, max_ends=17)
    assert totals.tolist() == [33, 0, 0, 64 + 72, 1] and int(found[0]["reads"]) == 136
    _, totals, found = model(c, max_ends=15)
    assert totals.tolist() == [33, 2, 0, 0, 0] and len(found) == 0


def test_min_reads_only_filters():
    c = lc.min_reads()
    _, totals, found = model(c, min_reads=1)
    assert totals.tolist() == c["totals"] and as_tuples(found) == c["links"] + [(2, 3, 0, 1, 1, 1, 3, 3, 3, 3)]
    assert len(model(c, min_reads=3)[2]) == 0


def test_the_query_list_permuted():
    """a and b follow the list: every permutation of four_edges' list gives the same links once its indices are mapped back to contigs and
    the flipped ones are flipped back"""
    c = lc.four_edges()
    want = {(int(k["a"]), int(k["info"]) & 1, int(k["b"]), int(k["info"]) >> 1): (int(k["reads"]), int(k["gap_sum"])) for k in model(c)[2]}
    rng = np.random.default_rng(5)
    for _ in range(5):
        q = [int(x) for x in rng.permutation(8)]
        stats, totals, found = model(c, queries=q)
        got = {}
        for k in found:
            a, oa, b, ob = q[int(k["a"])], int(k["info"]) & 1, q[int(k["b"])], int(k["info"]) >> 1
            key = (a, oa, b, ob) if a < b else (b, 1 - ob, a, 1 - oa)
            got[key] = (int(k["reads"]), int(k["gap_sum"]))
        assert got == want and totals.tolist() == c["totals"]
        assert (found["a"] < found["b"]).all()


def literal(c):
    """the pairing once more, record pair by record pair over the whole set, without the per-read lists: {(a, oA, b, oB): sorted gaps}"""
    thr = np.float32(c["min_seq_id"])
    p = c["par"]
    ends = []
    for x, q in enumerate(c["queries"]):
        for r in c["rec"][int(c["off"][q]):int(c["off"][q + 1])]:
            got = lm.counted(c["seqs"], c["ext"], q, r, thr, c["skip"])
            if got is None:
                continue
            qs, qe, ds, de, rev, t_len = got
            start, end = qs - ds, qs - ds + t_len               # the read on the query: [start, end)
            over_left, over_right = max(0, -start), max(0, end - len(c["seqs"][q]))
            if qe - qs + 1 >= p["anchor"] and (over_left >= p["overhang"]) != (over_right >= p["overhang"]):
                right = over_right >= p["overhang"]
                ends.append((int(r["target"]), x, "-" if rev else "+", right != rev, over_right if right else over_left))
    per_read = {}
    for e in ends:
        per_read[e[0]] = per_read.get(e[0], 0) + 1
    out = {}
    for t, x, ox, tail_x, hx in ends:
        for t2, y, oy, tail_y, hy in ends:
            if t != t2 or not tail_x or tail_y or x == y or per_read[t] > p["max_ends"]:
                continue
            flip = {"+": "-", "-": "+"}
            key = (x, ox, y, oy) if x < y else (y, flip[oy], x, flip[ox])
            out.setdefault(key, []).append(hx + hy - len(c["seqs"][t]))
    return {k: sorted(v) for k, v in out.items()}


@pytest.mark.parametrize("seed", lc.RANDOM_SEEDS)
def test_random_sets(seed):
    c = lc.random_set(seed)
    stats, totals, found = model(c, min_reads=1)
    want = literal(c)
    assert int(totals[4]) == len(want) == len(found) and int(totals[3]) == sum(len(v) for v in want.values())
    for k, key in zip(found, sorted(want, key=lambda k: (k[0], k[1] == "-", k[2], k[3] == "-"))):
        gaps = want[key]
        assert (int(k["a"]), "-" if int(k["info"]) & 1 else "+", int(k["b"]), "-" if int(k["info"]) & 2 else "+") == key
        assert (int(k["reads"]), int(k["gap_min"]), int(k["gap_max"]), int(k["gap_sum"])) == (len(gaps), gaps[0], gaps[-1], sum(gaps))
        assert int(k["mode_reads"]) == max(gaps.count(g) for g in set(gaps)) == gaps.count(int(k["gap_mode"]))
        assert all(gaps.count(g) < int(k["mode_reads"]) for g in set(gaps) if g < int(k["gap_mode"]))
    kept = model(c)[2]
    assert kept.tobytes() == found[found["reads"] >= c["par"]["min_reads"]].tobytes()


def test_the_random_sets_reach_what_they_are_for():
    """taken together the random sets hold crowded reads, self pairs, both-end records, links of more than 64 pairs and negative and positive gaps
    (three_gaps has the zero)"""
    seen = np.zeros(5, np.uint64)
    both = most = 0
    signs = set()
    for seed in lc.RANDOM_SEEDS:
        c = lc.random_set(seed)
        assert 1500 <= len(c["rec"]) <= 4500
        stats, totals, found = model(c, min_reads=1)
        seen += totals
        both += int(stats[:, 4].sum())
        most = max(most, int(found["reads"].max()) if len(found) else 0)
        signs |= {int(np.sign(g)) for g in found["gap_mode"]}
    assert seen[1] > 0 and seen[2] > 0 and both > 0 and most > 64 and {-1, 1} <= signs


def test_the_three_files():
    c = lc.min_reads()
    stats, _, found = model(c, min_reads=1)
    names = ["c%d" % i for i in range(4)]
    assert lm.links_tsv(names, found) == "c0\t+\tc1\t-\t2\t2\t3\t1\t3\t4\t7\nc2\t+\tc3\t+\t1\t1\t3\t1\t3\t3\t3\n"
    assert lm.links_tsv(names, found[:0]) == ""
    text = lm.ends_tsv(names, [10, 11, 12, 13], [100] * 4, stats)
    assert text.splitlines()[0] == "c0\t10\t100\t2\t59\t0\t2\t0\t1" and text.count("\n") == 4
    c = lc.three_gaps()
    found = model(c)[2]
    names, letters = ["n%d" % i for i in range(6)], ["ACGT" * (i + 1) for i in range(6)]
    want = "H\tVN:Z:1.0\n" + "".join("S\tn%d\t%s\tLN:i:%d\n" % (i, letters[i], 4 * (i + 1)) for i in range(6)) + "L\tn0\t+\tn1\t+\t5M\tRC:i:1\nL\tn2\t+\tn3\t+\t0M\tRC:i:1\n"
    assert lm.gfa(names, letters, found) == want          # the link with 7 letters between its contigs has no L line
