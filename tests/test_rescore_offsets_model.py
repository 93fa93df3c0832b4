"""The offset rule of the one-pass k_rescore (carpedeam_amd/csrc/rescore.hip), in numpy: the thread of hit h knows `rank[h]`, the
number of surviving hits in front of h, and writes it to off[q'] for every query q' in (owner[h - 1], owner[h]] - [0, owner[0]] for
h = 0; the last tile writes the total to off[owner[nHits - 1] + 1 .. n]; without hits off is zero.  Against the definition of the
CSR offsets: the exclusive cumulative sum of the surviving hits per query."""
import numpy as np
import pytest


def offsets_by_rule(n, owner, valid):
    off = np.full(n + 1, -1, np.int64)          # -1: never written
    if len(owner) == 0:
        return np.zeros(n + 1, np.int64)
    rank = np.cumsum(valid) - valid
    for h in range(len(owner)):
        first = 0 if h == 0 else owner[h - 1] + 1
        assert np.all(off[first:owner[h] + 1] == -1)          # every entry has one writer
        off[first:owner[h] + 1] = rank[h]
    assert np.all(off[owner[-1] + 1:] == -1)
    off[owner[-1] + 1:] = valid.sum()
    return off


def offsets_by_definition(n, owner, valid):
    per_query = np.bincount(owner[valid.astype(bool)], minlength=n) if len(owner) else np.zeros(n, np.int64)
    return np.concatenate([[0], np.cumsum(per_query)]).astype(np.int64)


def case(hits_per_query, valid=None, seed=0):
    hits_per_query = np.asarray(hits_per_query, np.int64)
    owner = np.repeat(np.arange(len(hits_per_query)), hits_per_query)
    if valid is None:
        valid = np.random.default_rng(seed).integers(0, 2, len(owner))
    return len(hits_per_query), owner, np.asarray(valid, np.int64)


DIRECTED = {
    "no_hits": case([0, 0, 0]),
    "no_queries": case([]),
    "one_hit": case([1], [1]),
    "one_invalid_hit": case([1], [0]),
    "first_query_empty": case([0, 3, 2]),
    "middle_query_empty": case([3, 0, 2]),
    "last_query_empty": case([3, 2, 0]),
    "several_empty_in_a_row": case([0, 0, 2, 0, 0, 0, 4, 0, 0]),
    "a_query_all_invalid": case([2, 3, 2], [1, 1, 0, 0, 0, 1, 0]),
    "everything_invalid": case([2, 0, 3], [0] * 5),
    "everything_valid": case([2, 0, 3], [1] * 5),
    "one_deep_query": case([0, 700, 1]),
}


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_rule_on_directed_owner_patterns(name):
    n, owner, valid = DIRECTED[name]
    got = offsets_by_rule(n, owner, valid)
    assert np.all(got >= 0)                                    # every entry is written
    assert np.array_equal(got, offsets_by_definition(n, owner, valid))


def test_rule_on_random_owner_patterns():
    rng = np.random.default_rng(7)
    for i in range(1000):
        n = int(rng.integers(0, 40))
        per = rng.integers(0, 6, n) * (rng.random(n) < rng.random())      # from no empty queries to mostly empty ones
        n, owner, valid = case(per, (rng.random(int(per.sum())) < rng.random()).astype(np.int64))
        got = offsets_by_rule(n, owner, valid)
        assert np.all(got >= 0), i
        assert np.array_equal(got, offsets_by_definition(n, owner, valid)), i
