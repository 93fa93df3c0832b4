"""tests/dedup_model.py against keep vectors written by hand (the first four cases of tests/dedupcases.py), and the properties the header
states for cdm_alns_dedup: idempotence, identity on a set without duplicates, counted = kept + removed, sum(keep) against the offsets."""
import numpy as np
import pytest

import dedup_model as dm
import dedupcases as dc


def run(c, queries=None):
    return dm.dedup(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"] if queries is None else queries, c["min_seq_id"], c["skip"])


def properties(c, off, rec, keep, stats, queries=None):
    q = c["queries"] if queries is None else queries
    assert keep.dtype == np.uint8 and len(keep) == len(c["rec"]) and stats.shape == (len(q), 4)
    assert int(keep.sum()) == int(off[-1]) == len(rec) and np.array_equal(rec, c["rec"][keep == 1])
    assert (stats[:, 0] == stats[:, 1] + stats[:, 2]).all() and (stats[:, 3] <= stats[:, 0]).all() and ((stats[:, 3] > 0) == (stats[:, 0] > 0)).all()
    for k, row in enumerate(q):
        lo, hi = int(c["off"][row]), int(c["off"][row + 1])
        assert int(off[row + 1]) - int(off[row]) == int(keep[lo:hi].sum()) == hi - lo - int(stats[k][2])
    for row in set(range(len(c["off"]) - 1)) - set(q):          # rows that are not listed are copied whole
        assert keep[int(c["off"][row]):int(c["off"][row + 1])].all()
    again = dict(c, off=off, rec=rec)
    off2, rec2, keep2, stats2 = run(again, q)
    assert np.array_equal(off2, off) and np.array_equal(rec2, rec) and keep2.all() and (stats2[:, 2] == 0).all() and np.array_equal(stats2[:, 0], stats[:, 1])


@pytest.mark.parametrize("name,make", dc.HAND + [("not_counted_skip_misfit", lambda: dc.not_counted(True, True)), ("not_counted_keep_misfit", lambda: dc.not_counted(False, True))],
                         ids=[n for n, _ in dc.HAND] + ["not_counted_skip_misfit", "not_counted_keep_misfit"])
def test_keep_vectors_written_by_hand(name, make):
    c = make()
    off, rec, keep, stats = run(c)
    assert keep.tolist() == c["keep"], name
    properties(c, off, rec, keep, stats)


def test_statistics_written_by_hand():
    assert run(dc.group_keys())[3].tolist() == [[7, 4, 3, 3]]
    assert run(dc.overhang())[3].tolist() == [[8, 6, 2, 2]]
    assert run(dc.reverse_strand())[3].tolist() == [[4, 2, 2, 2]]
    assert run(dc.not_counted(True, True))[3].tolist() == [[2, 1, 1, 2]] and run(dc.not_counted(False, True))[3].tolist() == [[4, 1, 3, 4]]


@pytest.mark.parametrize("name,make", dc.DIRECTED[len(dc.HAND):], ids=[n for n, _ in dc.DIRECTED[len(dc.HAND):]])
def test_directed_cases(name, make):
    c = make()
    off, rec, keep, stats = run(c)
    properties(c, off, rec, keep, stats)
    if "keep" in c:
        assert keep.tolist() == c["keep"]
    if name.startswith("long_runs"):
        assert stats.tolist() == [[10000, 5001, 4999, 5000]] and keep[c["survivor"]] == 1 and keep[1::2].sum() == 1 and keep[2::2].all()
    if name == "all_duplicates":
        best = max(range(1, 301), key=lambda r: (int(c["rec"][r]["ident"]), -r))
        assert stats.tolist() == [[300, 1, 299, 300]] and np.flatnonzero(keep).tolist() == [0, best]
    if name == "query_lists":
        k7, k11 = c["queries"].index(7), c["queries"].index(11)
        assert stats[k7].tolist() == [0, 0, 0, 0] and stats[k11].tolist() == [0, 0, 0, 0] and (stats[:, 2] > 0).sum() >= 3
        unlisted = dm.dedup(c["seqs"], c["ext"], c["off"], c["rec"], [q for q in range(30) if q not in c["queries"]])[3]
        assert unlisted[:, 2].sum() > 0          # the rows that are not listed do hold duplicates


def test_a_set_without_duplicates_comes_back_equal():
    import pileupcases as pc
    c = pc.one_query_of_40()
    off, rec, keep, stats = run(c)
    assert np.array_equal(off, c["off"]) and rec.tobytes() == c["rec"].tobytes() and keep.all() and stats.tolist() == [[9, 9, 0, 1]]


@pytest.mark.parametrize("seed", dc.RANDOM_SEEDS)
def test_random_sets(seed):
    c = dc.random_set(seed)
    properties(c, *run(c))


def test_the_random_sets_hold_groups_and_records_that_do_not_count():
    removed = counted = records = 0
    for seed in dc.RANDOM_SEEDS:
        c = dc.random_set(seed)
        stats = run(c)[3]
        removed += int(stats[:, 2].sum()); counted += int(stats[:, 0].sum())
        records += sum(int(c["off"][q + 1]) - int(c["off"][q]) for q in c["queries"])
    assert removed > 1000 and counted - removed > 300 and records > counted


def test_the_table():
    c = dc.group_keys()
    off, _, _, stats = run(c)
    assert dm.table(["c1"], [5], [60], c["off"], stats) == dm.HEADER + "c1\t5\t60\t8\t7\t4\t3\t3\n"
