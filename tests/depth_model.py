"""The statistic of cdm_pileup_depth (include/carpedeam_hip.h) in numpy, written from its definition: every counted record of a listed
query adds one to the depth of the positions qs..qe it covers, and the eight figures are read off the depth vector.
tests/test_depth_model.py holds it against a loop over positions and a hand-computed answer; the device is held against it."""
import numpy as np

from pileup_model import codes_of, csr, orient  # noqa: F401  (codes_of, csr: for the users of this module)

NAMES = ("reads", "columns", "breadth", "window", "covered", "sum", "sumsq", "max")
PER_SAMPLE = ("reads", "columns", "breadth", "covered", "sum", "sumsq", "max")


def window_of(length, edge):
    """(first, last) position of the statistics window: the whole contig when length <= 2 * edge"""
    if length <= 2 * edge:
        return 0, length - 1
    return edge, length - 1 - edge


def counted(seqs, ext, off, rec, q, min_seq_id, skip):
    """the oriented (qs, qe) of the records that count on query q, in record order"""
    thr = np.float32(min_seq_id)
    out = []
    for r in rec[int(off[q]):int(off[q + 1])]:
        t = int(r["target"])
        if t == q or not (np.float32(r["seq_id"]) >= thr):
            continue
        if skip and ext[t]:
            continue
        qs, qe, _, _, _ = orient(r, len(seqs[t]))
        out.append((qs, qe))
    return out


def stats_of(depth, n_reads, n_columns, edge):
    """the eight figures of one query from its depth vector"""
    length = len(depth)
    w0, w1 = window_of(length, edge)
    w = depth[w0:w1 + 1].astype(np.uint64)    # (exact while sumsq < 2^64: any input a test can hold)
    return [n_reads, n_columns, int((depth >= 1).sum()), len(w), int((w >= 1).sum()), int(w.sum()), int((w * w).sum()), int(w.max()) if len(w) else 0]


def depth_stats(seqs, ext, off, rec, queries, edge, min_seq_id=0.0, skip=False):
    """-> (stats[nq, 8] uint64, tracks: one uint32 depth vector per listed query)"""
    stats = np.zeros((len(queries), 8), np.uint64)
    tracks = []
    for k, q in enumerate(queries):
        q = int(q)
        depth = np.zeros(len(seqs[q]), np.uint32)
        recs = counted(seqs, ext, off, rec, q, min_seq_id, skip)
        for qs, qe in recs:
            depth[qs:qe + 1] += 1
        stats[k] = stats_of(depth, len(recs), sum(qe - qs + 1 for qs, qe in recs), int(edge))
        tracks.append(depth)
    return stats, tracks


def tsv_header(samples=1):
    cols = ["name", "key", "length", "window"]
    for s in range(1, samples + 1):
        cols += ["%s_%d" % (c, s) for c in PER_SAMPLE]
    return "\t".join(cols) + "\n"


def tsv(names, keys, lengths, stats_per_sample):
    """the table `carpedeam contig_depth` writes: stats_per_sample is one stats[nq, 8] per read set"""
    out = [tsv_header(len(stats_per_sample))]
    for i, name in enumerate(names):
        f = [name, str(int(keys[i])), str(int(lengths[i])), str(int(stats_per_sample[0][i][3]))]
        for st in stats_per_sample:
            f += [str(int(st[i][c])) for c in (0, 1, 2, 4, 5, 6, 7)]
        out.append("\t".join(f) + "\n")
    return "".join(out)


def bedgraph(names, tracks):
    """the runs of equal depth, zero runs included: name, start, end (0-based, half-open), depth"""
    out = []
    for name, d in zip(names, tracks):
        start = 0
        for i in range(1, len(d) + 1):
            if i == len(d) or d[i] != d[start]:
                out.append("%s\t%d\t%d\t%d\n" % (name, start, i, int(d[start])))
                start = i
    return "".join(out)
