"""cdm_pileup_links (include/carpedeam_hip.h) in plain numpy / Python, written from the header text: a counted record whose read hangs
over exactly one end of a listed query is an end record, a read's tail record on one list index and its head record on another are a
pair, the pairs with equal canonical (a, oA, b, oB) are a link.  links() returns the statistics, the totals and the links;
links_tsv(), ends_tsv() and gfa() are the three files `carpedeam contig_links` writes.  tests/test_links_model.py holds the model
against links written out by hand; the device and the command are held against it."""
from collections import Counter

import numpy as np

from pileup_model import orient

LINK_DTYPE = np.dtype([(n, "<u4") for n in ("a", "b", "info", "reads", "forward", "mode_reads")] + [(n, "<i4") for n in ("gap_mode", "gap_min", "gap_max", "reserved")] + [
    ("gap_sum", "<i8")])
STATS = ("reads", "columns", "left_ends", "right_ends", "both_ends", "links")
TOTALS = ("end_records", "crowded", "self_pairs", "pairs", "links")
DEFAULTS = dict(anchor=16, overhang=1, max_ends=16, min_reads=2)


def counted(seqs, ext, q, r, thr, skip):
    """None, or (qs, qe, ds, de, rev, tLen) of record r on query q: the rule of the reductions over the pile-up (tests/pileup_model.py
    profile(); a record that does not fit its two sequences is left out, countedRecord in csrc/pileup.h)"""
    t = int(r["target"])
    if t == q or t >= len(seqs) or not (np.float32(r["seq_id"]) >= thr):
        return None
    if skip and ext[t]:
        return None
    t_len, q_len = len(seqs[t]), len(seqs[q])
    qs, qe, ds, de, rev = orient(r, t_len)
    if qs < 0 or ds < 0 or qe < qs or qe >= q_len or de >= t_len or qe - qs != de - ds:
        return None
    return qs, qe, ds, de, rev, t_len


def links(seqs, ext, off, rec, queries, anchor=16, overhang=1, max_ends=16, min_reads=2, min_seq_id=0.0, skip=False):
    """-> (stats[nq, 6] uint64, totals[5] uint64, links: LINK_DTYPE, ascending by (a, oA, b, oB))"""
    thr = np.float32(min_seq_id)
    stats = np.zeros((len(queries), 6), np.uint64)
    totals = np.zeros(5, np.uint64)
    ends = {}               # read -> [(list index, tail, rev, h)]
    for x, q in enumerate(queries):
        q = int(q)
        q_len = len(seqs[q])
        for r in rec[int(off[q]):int(off[q + 1])]:
            c = counted(seqs, ext, q, r, thr, skip)
            if c is None:
                continue
            qs, qe, ds, de, rev, t_len = c
            stats[x, 0] += 1
            stats[x, 1] += qe - qs + 1
            u = qs - ds
            L, R = max(0, -u), max(0, u + t_len - q_len)
            if qe - qs + 1 < anchor:
                continue
            left, right = L >= overhang, R >= overhang
            if left and right:
                stats[x, 4] += 1
            elif left or right:
                stats[x, 2 if left else 3] += 1
                ends.setdefault(int(r["target"]), []).append((x, right != rev, rev, L if left else R))
    gaps = {}               # (a, oA, b, oB) -> [(gap, forward)]
    for t, e in ends.items():
        totals[0] += len(e)
        if len(e) > max_ends:
            totals[1] += 1
            continue
        for x, tail_x, rev_x, h_x in e:
            if not tail_x:
                continue
            for y, tail_y, rev_y, h_y in e:
                if tail_y:
                    continue
                if x == y:
                    totals[2] += 1
                    continue
                gap = h_x + h_y - len(seqs[t])
                key = (x, int(rev_x), y, int(rev_y)) if x < y else (y, int(not rev_y), x, int(not rev_x))
                gaps.setdefault(key, []).append((gap, x < y))
    totals[3] = sum(len(g) for g in gaps.values())
    totals[4] = len(gaps)
    out = []
    for key in sorted(gaps):
        g = gaps[key]
        if len(g) < min_reads:
            continue
        values = [v for v, _ in g]
        count = Counter(values)
        mode = min(count, key=lambda v: (-count[v], v))
        a, o_a, b, o_b = key
        out.append((a, b, o_a | o_b << 1, len(g), sum(1 for _, f in g if f), count[mode], mode, min(values), max(values), 0, sum(values)))
        stats[a, 5] += 1
        stats[b, 5] += 1
    return stats, totals, (np.array(out, LINK_DTYPE) if out else np.empty(0, LINK_DTYPE))


def links_tsv(names, found):
    """the table `carpedeam contig_links` writes: one line per returned link, no header"""
    out = []
    for k in found:
        f = [names[int(k["a"])], "-" if int(k["info"]) & 1 else "+", names[int(k["b"])], "-" if int(k["info"]) & 2 else "+"]
        f += [int(k[n]) for n in ("reads", "forward", "gap_mode", "mode_reads", "gap_min", "gap_max", "gap_sum")]
        out.append("\t".join(str(x) for x in f) + "\n")
    return "".join(out)


def ends_tsv(names, keys, lengths, stats):
    """its --ends file: one line per contig, no header"""
    return "".join("\t".join([names[i], str(int(keys[i])), str(int(lengths[i]))] + [str(int(v)) for v in stats[i]]) + "\n" for i in range(len(names)))


def gfa(names, letters, found):
    """its --gfa file: GFA 1, a segment per contig in input order, an L line per returned link whose most frequent gap is an overlap or 0"""
    out = ["H\tVN:Z:1.0\n"]
    for name, s in zip(names, letters):
        out.append("S\t%s\t%s\tLN:i:%d\n" % (name, s, len(s)))
    for k in found:
        if int(k["gap_mode"]) <= 0:
            out.append("L\t%s\t%s\t%s\t%s\t%dM\tRC:i:%d\n" % (names[int(k["a"])], "-" if int(k["info"]) & 1 else "+", names[int(k["b"])], "-" if int(k["info"]) & 2 else "+",
                                                             -int(k["gap_mode"]), int(k["reads"])))
    return "".join(out)
