"""The statistic of cdm_pileup_breaks (include/carpedeam_hip.h) in numpy, integers only, written from its definition: span[b] counts the
counted records with at least `anchor` columns on either side of boundary b, a window boundary is weak where too few span it, and a
break is a maximal run of weak boundaries.  tests/test_breaks_model.py holds it against hand-computed answers; the device is held
against it.  The text writers give what `carpedeam contig_breaks` writes for these results."""
import numpy as np

from depth_model import counted

NAMES = ("reads", "columns", "window", "weak", "breaks", "joins", "min_span", "sum_span")
FIELDS = ("query", "first", "last", "min_span", "uncovered", "depth_left", "depth_right", "flags")
BREAK_DTYPE = np.dtype([(n, "<u4") for n in FIELDS])
JOIN, GAP = 1, 2


def arrays_of(length, recs, anchor):
    """(depth[length], span[length]) of one query from the oriented (qs, qe) of its counted records; span[0] = 0"""
    depth = np.zeros(length, np.int64)
    span = np.zeros(length + 1, np.int64)
    w = int(anchor)
    for qs, qe in recs:
        depth[qs:qe + 1] += 1
        if qe - qs + 1 >= 2 * w:
            span[qs + w:qe + 2 - w] += 1          # boundaries qs + w .. qe + 1 - w
    return depth, span[:length]


def weak_of(depth, span, edge, min_span, min_span_percent):
    """(in_window[length], weak[length]) per boundary b; b = 0 is no boundary"""
    length = len(depth)
    b = np.arange(length)
    in_window = (b >= edge) & (b <= length - edge) & (b >= 1)
    weak = np.zeros(length, bool)
    if length >= 2:
        low = np.minimum(depth[:-1], depth[1:])       # min(depth[b - 1], depth[b]) for b = 1 ..
        weak[1:] = span[1:] < min_span
        if min_span_percent > 0:
            weak[1:] |= span[1:] * 100 < int(min_span_percent) * low      # (int64: exact for any input a test can hold)
    return in_window, weak & in_window


def runs_of(weak):
    """[(first, last)] of the maximal runs of True"""
    w = np.concatenate(([False], weak, [False])).astype(np.int8)
    d = np.diff(w)
    return list(zip(np.flatnonzero(d == 1).tolist(), (np.flatnonzero(d == -1) - 1).tolist()))


def breaks_stats(seqs, ext, off, rec, queries, anchor, edge, min_span=1, min_span_percent=0, min_seq_id=0.0, skip=False):
    """-> (stats[nq, 8] uint64, tracks: one uint32 span vector per listed query, breaks: BREAK_DTYPE in listed query order, then first)"""
    stats = np.zeros((len(queries), 8), np.uint64)
    tracks, out = [], []
    for k, q in enumerate(queries):
        q = int(q)
        recs = counted(seqs, ext, off, rec, q, min_seq_id, skip)
        depth, span = arrays_of(len(seqs[q]), recs, anchor)
        in_window, weak = weak_of(depth, span, int(edge), int(min_span), int(min_span_percent))
        runs = runs_of(weak)
        joins = 0
        for first, last in runs:
            uncovered = int((depth[first:last] == 0).sum())
            joins += uncovered == 0
            out.append((k, first, last, int(span[first:last + 1].min()), uncovered, int(depth[first - 1]), int(depth[last]), GAP if uncovered else JOIN))
        ws = span[in_window]
        stats[k] = [len(recs), sum(qe - qs + 1 for qs, qe in recs), len(ws), int(weak.sum()), len(runs), joins, int(ws.min()) if len(ws) else 0, int(ws.sum())]
        tracks.append(span.astype(np.uint32))
    return stats, tracks, np.array(out, BREAK_DTYPE)


# ------------------------------------------------------------------------------------------------ the texts of `carpedeam contig_breaks`
HEADER = "name\tkey\tlength\treads\tcolumns\twindow\tweak\tbreaks\tjoins\tmin_span\tsum_span\n"


def tsv(names, keys, lengths, stats, breaks):
    """the header, one line per contig in input order, behind each its breaks: #break name first last min_span uncovered depth_left
    depth_right J|G (1-based boundaries)"""
    out = [HEADER]
    for i, name in enumerate(names):
        out.append("\t".join([name, str(int(keys[i])), str(int(lengths[i]))] + [str(int(v)) for v in stats[i]]) + "\n")
        for b in breaks[breaks["query"] == i]:
            out.append("#break\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (name, int(b["first"]) + 1, int(b["last"]) + 1, int(b["min_span"]), int(b["uncovered"]), int(b["depth_left"]),
                                                                  int(b["depth_right"]), "G" if int(b["flags"]) & GAP else "J"))
    return "".join(out)


def bedgraph(names, tracks):
    """the runs of equal span: name, start, end (0-based, half-open), span"""
    out = []
    for name, d in zip(names, tracks):
        start = 0
        for i in range(1, len(d) + 1):
            if i == len(d) or d[i] != d[start]:
                out.append("%s\t%d\t%d\t%d\n" % (name, start, i, int(d[start])))
                start = i
    return "".join(out)


def split(names, seqs, breaks, min_piece=1):
    """the FASTA of the contigs cut at their breaks: a piece ends at position first - 1, the next begins at position last; an unbroken
    contig keeps its name, pieces are name_1, name_2, ...; pieces shorter than min_piece are left out"""
    out = []
    for i, (name, s) in enumerate(zip(names, seqs)):
        mine = breaks[breaks["query"] == i]
        pieces, at = [], 0
        for b in mine:
            pieces.append(s[at:int(b["first"])])
            at = int(b["last"])
        pieces.append(s[at:])
        for k, p in enumerate(pieces):
            if len(p) >= min_piece:
                out.append(">%s\n%s\n" % (name if not len(mine) else "%s_%d" % (name, k + 1), p))
    return "".join(out)
