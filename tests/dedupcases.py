"""Directed and random inputs of cdm_alns_dedup, shared by the model's own tests (CPU) and the device's (GPU): the smallest shapes at
which the kernels can go wrong.  A case is the dict of tests/pileupcases.py (seqs, ext, off / rec, queries, min_seq_id, skip); the first
four carry the keep vector written by hand ("keep")."""
import numpy as np

import pileupcases as pc
from pileup_model import unorient


def placed(t, t_len, q_len, u, rev, ident=0, seq_id=1.0, clip=(0, 0)):
    """the record of read t (t_len letters) whose unclipped start on a query of q_len letters is u: the whole overlap, less clip[0]
    columns at its left and clip[1] at its right end"""
    qs, qe = max(u, 0) + clip[0], min(u + t_len - 1, q_len - 1) - clip[1]
    assert 0 <= qs <= qe < q_len
    r = unorient(t, qs, qe, qs - u, qe - u, rev, t_len, seq_id)
    return r[:2] + (int(ident),) + r[3:]


def _one_query(q_len, reads, seed, **kw):
    """reads: (t_len, u, rev, ident[, seq_id[, clip]]) in set order, every read a sequence of its own -> the case, identity record first"""
    rng = np.random.default_rng(seed)
    seqs = [pc.rand_seq(rng, q_len)] + [pc.rand_seq(rng, r[0]) for r in reads]
    recs = [pc.identity(seqs, 0)]
    for i, r in enumerate(reads):
        recs.append(placed(1 + i, r[0], q_len, r[1], r[2], r[3], *r[4:]))
    return pc.case(seqs, {0: recs}, [0], **kw)


def group_keys():
    """three forward reads of one length on one diagonal (ident 18, 20, 20: the second stays), the same coordinates reversed (a group of
    their own), the same u with another tLen, the same tLen with u + 1"""
    c = _one_query(60, [(20, 10, False, 18), (20, 10, False, 20), (20, 10, False, 20), (20, 10, True, 20), (20, 10, True, 18), (21, 10, False, 1), (20, 11, False, 1)], 501)
    c["keep"] = [1, 0, 1, 0, 1, 0, 1, 1]
    return c


def overhang():
    """u = -1 (a pair), u = -(tLen - 1), u = qLen - 1; two reads of 20 and 25 letters clipped to the same 0..14 (both stay); two reads of
    20 letters at u = -5 (the one with the smaller ident goes); a read at u = -3 clipped to the same 0..14"""
    c = _one_query(50, [(20, -1, False, 5), (20, -1, False, 5), (20, -19, False, 1), (20, 49, False, 1), (20, -5, False, 3), (25, -10, False, 3), (20, -5, False, 9),
                        (20, -3, False, 3, 1.0, (0, 2))], 502)
    r = c["rec"]
    assert [(int(x["q_start"]), int(x["q_end"])) for x in r[[5, 6, 7, 8]]] == [(0, 14)] * 4 and (int(r[3]["q_start"]), int(r[3]["q_end"])) == (0, 0) and int(r[4]["q_start"]) == 49
    c["keep"] = [1, 1, 0, 1, 1, 0, 1, 1, 1]
    return c


def reverse_strand():
    """a forward read of 24 letters at u = 10 (raw target columns 2..19) and two reverse reads whose raw target columns are 4..23 and
    0..19 but which orient to u = 10 as well: the reverse pair is a group, the forward record none of it; a second forward copy goes"""
    c = _one_query(60, [(24, 10, False, 7, 1.0, (2, 4)), (24, 10, True, 4, 1.0, (0, 4)), (24, 10, True, 6, 1.0, (4, 0)), (24, 10, False, 7)], 503)
    r = c["rec"]
    assert [(int(x["db_start"]), int(x["db_end"])) for x in r[1:4]] == [(2, 19), (4, 23), (0, 19)] and int(r[2]["q_start"]) > int(r[2]["q_end"])
    c["keep"] = [1, 1, 0, 1, 0]
    return c


def not_counted(skip, misfit=False):
    """one group key (forward, u = 5, 20 letters) throughout, min_seq_id 0.9: A counted, ident 10; B below the threshold with the largest
    ident; C counted, ident 9; D and E on extended targets, ident 99 and 98; with misfit M, whose two spans differ (cdm_alns_upload refuses
    such a record, so only the model sees it), ident 100.  B, M and - under skip - D and E stay and displace nothing"""
    reads = [(20, 5, False, 10, 0.95), (20, 5, False, 50, 0.5), (20, 5, False, 9, 0.95), (20, 5, False, 99), (20, 5, False, 98)] + ([(20, 5, False, 100)] if misfit else [])
    c = _one_query(60, reads, 504, ext=[1, 0, 0, 0, 1, 1] + [0] * misfit, min_seq_id=0.9, skip=skip)
    if misfit:
        c["rec"][6]["db_end"] -= 1
    c["keep"] = ([1, 1, 1, 0, 1, 1] if skip else [1, 0, 1, 0, 1, 0]) + [1] * misfit
    return c


def same_target_twice():
    """one read with two records at one place (the second goes), and a third on the other strand"""
    rng = np.random.default_rng(505)
    seqs = [pc.rand_seq(rng, 60), pc.rand_seq(rng, 20)]
    recs = [pc.identity(seqs, 0), placed(1, 20, 60, 7, False, 3), placed(1, 20, 60, 7, False, 3), placed(1, 20, 60, 7, True, 3)]
    c = pc.case(seqs, {0: recs}, [0])
    c["keep"] = [1, 1, 0, 1]
    return c


def wide_fields():
    """a query of 70 000 letters, reads of 66 000 and of 464 letters: pairs of keys that differ in bit 16 of u or of tLen alone, u on both
    sides of 0"""
    c = _one_query(70_000, [(66_000, 1000, False, 1), (66_000, 1000 + 65_536, False, 9), (464, 1000, False, 9), (66_000, 1000, False, 2), (66_000, -65_000, True, 4),
                            (66_000, -65_000 + 65_536, True, 9), (66_000, -65_000, True, 4)], 506)
    c["keep"] = [1, 0, 1, 1, 1, 1, 1, 0]
    return c


def long_runs(peak):
    """one group of 5 000 records interleaved in set order with 5 000 singletons: more than a work item of 1 024 records, a block and a
    radix tile.  peak: where the largest ident sits (first, middle, last), or equal: every ident the same"""
    rng = np.random.default_rng(507)
    n, q_len = 5000, 6000
    seqs = [pc.rand_seq(rng, q_len)] + [pc.rand_seq(rng, 30) for _ in range(7)]
    at = {"first": 0, "middle": n // 2 + 1, "last": n - 1, "equal": -1}[peak]
    recs = [pc.identity(seqs, 0)]
    for i in range(n):
        recs.append(placed(1 + i % 7, 30, q_len, 50, False, 90 if i == at else 10))
        recs.append(placed(1 + (i + 3) % 7, 30, q_len, 100 + i, bool(i % 2), 10))
    c = pc.case(seqs, {0: recs}, [0])
    c["survivor"] = 1 + 2 * max(at, 0)
    return c


def all_duplicates():
    """every counted record of the query in one group"""
    rng = np.random.default_rng(508)
    seqs = [pc.rand_seq(rng, 80)] + [pc.rand_seq(rng, 33) for _ in range(5)]
    recs = [pc.identity(seqs, 0)] + [placed(1 + i % 5, 33, 80, 20, True, int(rng.integers(0, 40))) for i in range(300)]
    return pc.case(seqs, {0: recs}, [0])


def _few_keys(rng, seqs, q, n_recs, ids=(1.0,)):
    """n_recs records on query q whose (rev, u, tLen) come from a handful of values: groups abound"""
    q_len = len(seqs[q])
    targets = [int(t) for t in rng.integers(0, len(seqs), size=4) if int(t) != q and len(seqs[int(t)]) >= 2]
    starts = [int(u) for u in rng.integers(-8, max(q_len - 2, 1), size=3)]
    out = []
    while targets and len(out) < n_recs:
        t, u, rev = targets[int(rng.integers(0, len(targets)))], starts[int(rng.integers(0, 3))], bool(rng.integers(0, 2))
        t_len = len(seqs[t])
        lo, hi = max(u, 0), min(u + t_len - 1, q_len - 1)
        if hi - lo < 1:
            u = 0
            lo, hi = 0, min(t_len, q_len) - 1
            if hi < 1:
                continue
        left = int(rng.integers(0, (hi - lo) // 2 + 1))
        right = int(rng.integers(0, hi - lo - left))
        out.append(placed(t, t_len, q_len, u, rev, int(rng.integers(0, 4)), float(ids[int(rng.integers(0, len(ids)))]), (left, right)))
    return out


def query_lists():
    """a DB of 30 sequences, an unsorted, non-contiguous list; rows that are not listed hold duplicates; query 7 has only its identity
    record, query 11 no record at all"""
    rng = np.random.default_rng(509)
    seqs = [pc.rand_seq(rng, int(n)) for n in rng.choice([20, 25, 40, 90], size=30)]
    per = {}
    for q in range(30):
        if q == 11:
            continue
        per[q] = [pc.identity(seqs, q)] + ([] if q == 7 else _few_keys(rng, seqs, q, int(rng.integers(5, 40))))
    return pc.case(seqs, per, [17, 3, 29, 7, 11, 4])


def random_set(seed):
    """2..20 sequences of a few lengths, 0..120 records per query from a handful of keys each, random ident, identity threshold, flags and
    query list"""
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.integers(2, 21))
    seqs = [pc.rand_seq(rng, int(l), 0.02) for l in rng.choice([2, 17, 30, 31, 64, 150], size=n)]
    ids = [float(np.float32(x)) for x in (0.8, 0.9, 0.95, 1.0)]
    per = {}
    for q in range(n):
        per[q] = ([pc.identity(seqs, q)] if rng.integers(0, 4) else []) + (_few_keys(rng, seqs, q, int(rng.integers(0, 121)), ids) if len(seqs[q]) >= 2 else [])
    k = int(rng.integers(1, n + 1))
    return pc.case(seqs, per, [int(x) for x in rng.permutation(n)[:k]], ext=[int(x) for x in rng.integers(0, 2, size=n)], min_seq_id=float(rng.choice([0.0, 0.9])),
                   skip=bool(rng.integers(0, 2)))


HAND = [("group_keys", group_keys), ("overhang", overhang), ("reverse_strand", reverse_strand), ("not_counted_skip", lambda: not_counted(True)),
        ("not_counted_keep", lambda: not_counted(False))]
DIRECTED = HAND + [("same_target_twice", same_target_twice), ("wide_fields", wide_fields), ("long_runs_first", lambda: long_runs("first")),
                   ("long_runs_middle", lambda: long_runs("middle")), ("long_runs_last", lambda: long_runs("last")), ("long_runs_equal", lambda: long_runs("equal")),
                   ("all_duplicates", all_duplicates), ("query_lists", query_lists)]
RANDOM_SEEDS = range(40)
