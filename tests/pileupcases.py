"""Directed and random inputs of cdm_pileup_profile, shared by the model's own tests (CPU) and the device's (GPU).  A case is a dict:
seqs (ASCII), ext (wasExtended per sequence), off / rec (the alignment set, CSR by query), queries, ends, min_seq_id, skip."""
import random

import numpy as np

from pileup_model import csr, unorient


class PyRng:
    """the two calls random_record makes, on Python's generator (a numpy call per integer costs more than the rest of a random set)"""

    def __init__(self, seed):
        self.r = random.Random(seed)

    def integers(self, lo, hi):
        return self.r.randrange(lo, hi)


def rand_seq(rng, n, n_frac=0.0):
    s = rng.choice(list("ACGT"), size=n)
    if n_frac:
        s[rng.random(n) < n_frac] = "N"
    return "".join(s)


def case(seqs, per_query, queries, ends=16, ext=None, min_seq_id=0.0, skip=False):
    off, rec = csr(len(seqs), per_query)
    return dict(seqs=list(seqs), ext=list(ext) if ext is not None else [0] * len(seqs), off=off, rec=rec, queries=list(queries), ends=ends,
                min_seq_id=min_seq_id, skip=skip)


def identity(seqs, q):
    return (q, 0, 0, 0, len(seqs[q]) - 1, 0, len(seqs[q]) - 1, 1.0)


def one_query_of_40(ends=16):
    """a forward read inside the query, a reverse read, reads overhanging either end, a read of 5 letters (both tables at once with
    ends = 16), reads of exactly `ends` and of 2 * ends - 1 letters"""
    rng = np.random.default_rng(40)
    seqs = [rand_seq(rng, 40)] + [rand_seq(rng, n) for n in (20, 20, 20, 20, 5, ends, 2 * ends - 1)]
    L = [len(s) for s in seqs]
    recs = [identity(seqs, 0),
            unorient(1, 10, 29, 0, 19, False, L[1]),                   # forward, inside
            unorient(2, 5, 24, 0, 19, True, L[2]),                     # reverse, inside
            unorient(3, 0, 11, 8, 19, False, L[3]),                    # overhangs the query's left end
            unorient(4, 30, 39, 0, 9, False, L[4]),                    # overhangs its right end
            unorient(4, 0, 6, 13, 19, True, L[4]),                     # the same read reversed over the left end
            unorient(5, 17, 21, 0, 4, False, L[5]),                    # 5 letters
            unorient(5, 30, 34, 0, 4, True, L[5]),
            unorient(6, 3, 3 + ends - 1, 0, ends - 1, False, L[6]),    # exactly `ends` letters
            unorient(7, 2, 2 + 2 * ends - 2, 0, 2 * ends - 2, True, L[7])]
    return case(seqs, {0: recs}, [0], ends)


def n_columns():
    """an N in a query column and an N in a target column: those columns count in `columns` only"""
    rng = np.random.default_rng(41)
    q = list(rand_seq(rng, 50)); q[12] = "N"; q[33] = "N"
    t1 = list(rand_seq(rng, 30)); t1[3] = "N"; t1[28] = "N"
    t2 = rand_seq(rng, 25)
    seqs = ["".join(q), "".join(t1), t2]
    recs = [identity(seqs, 0), unorient(1, 5, 34, 0, 29, False, 30), unorient(1, 10, 39, 0, 29, True, 30), unorient(2, 8, 32, 0, 24, False, 25), unorient(2, 20, 44, 0, 24, True, 25)]
    return case(seqs, {0: recs}, [0], 16)


def word_boundaries():
    """queries and targets that cross the 16-base word boundaries at 16 and 32; target overlaps that start mid-word"""
    rng = np.random.default_rng(42)
    seqs = [rand_seq(rng, 70), rand_seq(rng, 48), rand_seq(rng, 33), rand_seq(rng, 17)]
    L = [len(s) for s in seqs]
    recs = [identity(seqs, 0)]
    for t, qs, ds, n in ((1, 10, 5, 40), (1, 15, 15, 33), (1, 31, 0, 2), (2, 16, 0, 33), (2, 1, 7, 26), (3, 15, 0, 17), (3, 32, 15, 2), (1, 0, 16, 32), (1, 22, 31, 17)):
        for rev in (False, True):
            recs.append(unorient(t, qs, qs + n - 1, ds, ds + n - 1, rev, L[t]))
    return case(seqs, {0: recs}, [0], 16)


def depth(n_records, ends=16):
    """n_records records on one query (a handful of reads, many records each)"""
    rng = np.random.default_rng(1000 + n_records)
    seqs = [rand_seq(rng, 120)] + [rand_seq(rng, int(n)) for n in rng.integers(1, 90, size=12)]
    recs = [identity(seqs, 0)]
    while len(recs) < n_records + 1:
        t = int(rng.integers(1, len(seqs)))
        recs.append(random_record(rng, len(seqs[0]), t, len(seqs[t])))
    return case(seqs, {0: recs}, [0], ends)


def random_record(rng, q_len, t, t_len, seq_id=1.0):
    n = int(rng.integers(1, min(q_len, t_len) + 1))
    qs, ds = int(rng.integers(0, q_len - n + 1)), int(rng.integers(0, t_len - n + 1))
    rev = bool(rng.integers(0, 2)) and n > 1
    return unorient(t, qs, qs + n - 1, ds, ds + n - 1, rev, t_len, seq_id)


def query_lists():
    """a DB of 30 sequences: non-contiguous, unsorted indices; query 7 has only its identity record"""
    rng = np.random.default_rng(43)
    seqs = [rand_seq(rng, int(n)) for n in rng.integers(20, 120, size=30)]
    per = {}
    for q in range(30):
        per[q] = [identity(seqs, q)]
        if q != 7:
            for _ in range(int(rng.integers(1, 20))):
                t = int(rng.integers(0, 30))
                if t != q:
                    per[q].append(random_record(rng, len(seqs[q]), t, len(seqs[t])))
    return case(seqs, per, [17, 3, 29, 7, 4], 16)


def mixed_flags(skip):
    """skip_extended_targets on a DB with mixed wasExtended flags"""
    c = query_lists()
    c["ext"] = [1 if i % 3 == 0 else 0 for i in range(30)]
    c["skip"] = skip
    return c


def threshold():
    """min_seq_id: a record whose seq_id equals the threshold exactly is counted, the float below it is not"""
    rng = np.random.default_rng(44)
    seqs = [rand_seq(rng, 60), rand_seq(rng, 30), rand_seq(rng, 30), rand_seq(rng, 30)]
    thr = np.float32(0.9)
    below = np.nextafter(thr, np.float32(0))
    recs = [identity(seqs, 0), unorient(1, 0, 29, 0, 29, False, 30, thr), unorient(2, 10, 39, 0, 29, True, 30, below), unorient(3, 30, 59, 0, 29, False, 30, np.float32(0.95))]
    return case(seqs, {0: recs}, [0], 16, min_seq_id=float(thr))


def long_reads(ends):
    """ends = 1 and ends = 64 on reads longer than 2 * 64 letters and shorter than 64"""
    rng = np.random.default_rng(45)
    seqs = [rand_seq(rng, 260), rand_seq(rng, 150), rand_seq(rng, 64), rand_seq(rng, 63), rand_seq(rng, 127), rand_seq(rng, 1)]
    recs = [identity(seqs, 0)]
    for t in range(1, 6):
        for _ in range(6):
            recs.append(random_record(rng, 260, t, len(seqs[t])))
        if len(seqs[t]) > 1:
            recs.append(unorient(t, 100, 100 + len(seqs[t]) - 1, 0, len(seqs[t]) - 1, True, len(seqs[t])))
        recs.append(unorient(t, 2, 2 + len(seqs[t]) - 1, 0, len(seqs[t]) - 1, False, len(seqs[t])))
    return case(seqs, {0: recs}, [0], ends)


def raw_plane():
    """lower-case and IUPAC letters: the sequences get a row in the raw plane; mapped codes and N bits are what counts"""
    rng = np.random.default_rng(46)
    alphabet = list("ACGTacgtNnRYKMSWBDHVUuXx")
    seqs = ["".join(rng.choice(alphabet, size=int(n))) for n in (80, 40, 33, 20)] + [rand_seq(rng, 50)]
    recs = {0: [identity(seqs, 0)], 4: [identity(seqs, 4)]}
    for q in (0, 4):
        for t in range(5):
            if t != q:
                for _ in range(5):
                    recs[q].append(random_record(rng, len(seqs[q]), t, len(seqs[t])))
    return case(seqs, recs, [0, 4], 16)


DIRECTED = [("one_query_of_40", one_query_of_40), ("n_columns", n_columns), ("word_boundaries", word_boundaries), ("query_lists", query_lists),
            ("mixed_flags_skip", lambda: mixed_flags(True)), ("mixed_flags_keep", lambda: mixed_flags(False)), ("threshold", threshold),
            ("ends_1", lambda: long_reads(1)), ("ends_64", lambda: long_reads(64)), ("raw_plane", raw_plane),
            ("depth_1", lambda: depth(1)), ("depth_64", lambda: depth(64)), ("depth_65", lambda: depth(65)), ("depth_129", lambda: depth(129))]


def random_set(seed, max_queries=None):
    """a DB of 2..40 sequences of 1..300 letters (N at 2 % of them), 0..150 valid random records per query on both strands (identity
    records among them); the query list: a random subset in random order, every query with max_queries=None"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 41))
    seqs = [rand_seq(rng, int(rng.integers(1, 301)), 0.02) for _ in range(n)]
    ext = [int(x) for x in rng.integers(0, 2, size=n)]
    per = {}
    fast = PyRng(seed)
    ids = [float(np.float32(x)) for x in (0.8, 0.85, 0.9, 0.95, 1.0)]
    for q in range(n):
        per[q] = []
        for _ in range(fast.integers(0, 151)):
            t = fast.integers(0, n)
            per[q].append(identity(seqs, q) if t == q else random_record(fast, len(seqs[q]), t, len(seqs[t]), ids[fast.integers(0, 5)]))
    k = n if max_queries is None else int(rng.integers(1, min(n, max_queries) + 1))
    queries = [int(x) for x in rng.permutation(n)[:k]]
    return case(seqs, per, queries, int(rng.choice([1, 5, 16, 64])), ext=ext, min_seq_id=float(rng.choice([0.0, 0.9])), skip=bool(rng.integers(0, 2)))
