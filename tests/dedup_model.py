"""cdm_alns_dedup (include/carpedeam_hip.h) in plain numpy / Python, written from the header text: the counted records of a listed query
with equal (reverse, u = qs - ds, tLen) form a group, the record with the largest ident stays, among equals the earliest in the set.
dedup() returns the new set, the keep flags and the four statistics; table() is the file `carpedeam contig_dedup` writes.
tests/test_dedup_model.py holds the model against hand-written keep vectors; the device and the commands are held against it."""
import numpy as np

from pileup_model import orient

NAMES = ("counted", "kept", "removed", "largest")
HEADER = "name\tkey\tlength\trecords\tcounted\tkept\tduplicates\tlargest\n"


def counted(seqs, ext, q, r, thr, skip):
    """None, or (rev, u, tLen) of record r on query q: the rule of the reductions over the pile-up (countedRecord, csrc/pileup.h)"""
    t = int(r["target"])
    if t == q or t >= len(seqs) or not (np.float32(r["seq_id"]) >= thr):
        return None
    if skip and ext[t]:
        return None
    t_len, q_len = len(seqs[t]), len(seqs[q])
    qs, qe, ds, de, rev = orient(r, t_len)
    if qs < 0 or ds < 0 or qe < qs or qe >= q_len or de >= t_len or qe - qs != de - ds:
        return None         # a record that does not fit its two sequences
    return rev, qs - ds, t_len


def dedup(seqs, ext, off, rec, queries, min_seq_id=0.0, skip=False):
    """-> (off', rec', keep: uint8 per record of rec, stats[nq, 4] uint64)"""
    thr = np.float32(min_seq_id)
    keep = np.ones(len(rec), np.uint8)
    stats = np.zeros((len(queries), 4), np.uint64)
    for k, q in enumerate(queries):
        q = int(q)
        groups = {}         # (rev, u, tLen) -> the indices of its records, ascending
        for r in range(int(off[q]), int(off[q + 1])):
            key = counted(seqs, ext, q, rec[r], thr, skip)
            if key is not None:
                groups.setdefault(key, []).append(r)
        n = sum(len(g) for g in groups.values())
        for g in groups.values():
            best = max(g, key=lambda r: (int(rec[r]["ident"]), -r))
            for r in g:
                if r != best:
                    keep[r] = 0
        stats[k] = (n, len(groups), n - len(groups), max((len(g) for g in groups.values()), default=0))
    new_off = np.zeros(len(off), np.uint64)
    new_off[1:] = np.cumsum([int(keep[int(off[q]):int(off[q + 1])].sum()) for q in range(len(off) - 1)])
    return new_off, rec[keep == 1], keep, stats


def table(names, keys, lengths, off, stats):
    """the table `carpedeam contig_dedup` writes: one line per contig (the first len(names) sequences of the joint DB, listed in order)"""
    out = [HEADER]
    for i, name in enumerate(names):
        f = [name, int(keys[i]), int(lengths[i]), int(off[i + 1]) - int(off[i]), int(stats[i][0]), int(stats[i][1]), int(stats[i][2]), int(stats[i][3])]
        out.append("\t".join(str(x) for x in f) + "\n")
    return "".join(out)
