"""The statistics of cdm_pileup_depth_gapped, cdm_pileup_bases_gapped and cdm_pileup_breaks_gapped (include/carpedeam_hip.h) in numpy,
integers only, written from their definition: the ungapped records count as in depth_model, bases_model and breaks_model, and every
gapped record adds its M columns - found by walking its operations from pos and tstart - to the same depth, span and counters; the
figures are then read off the sums exactly as the three models read them.  tests/test_gapped_tables_model.py holds it against a
hand-worked record, the single-M property and the planted case; the device is held against it."""
import numpy as np

import bases_model as bm
import breaks_model as brm
import depth_model as dm
import gapped_model as gm
from pileup_model import codes_of, orient


def segments(r, gops):
    """the M operations of a gapped record as [(p, o, g)]: g columns, column j on query position p + j with the read's oriented offset
    o + j.  I advances the offset, D the position"""
    p, o, out = int(r["pos"]), int(r["tstart"]), []
    for w in gops[int(r["ops"]):int(r["ops"]) + int(r["n_ops"])]:
        g, op = int(w) >> 2, int(w) & 3
        if op == gm.OP_M:
            out.append((p, o, g))
            p += g
            o += g
        elif op == gm.OP_I:
            o += g
        else:
            p += g
    return out


def columns_of(segs):
    """the query positions m_1 < .. < m_C of a record's M columns"""
    return [p + j for p, _, g in segs for j in range(g)]


def spanned(segs, anchor):
    """(first, last) boundary a record spans with `anchor` M columns on either side, or None: m_w + 1 .. m_(C - w + 1)"""
    m, w = columns_of(segs), int(anchor)
    if len(m) < 2 * w:
        return None
    return m[w - 1] + 1, m[len(m) - w]


def of_query(grecs, k):
    return grecs[grecs["query"] == k]


def add_depth(depth, segs):
    for p, _, g in segs:
        depth[p:p + g] += 1


def depth_stats(seqs, ext, off, rec, queries, grecs, gops, edge, min_seq_id=0.0, skip=False):
    """-> (stats[nq, 8] uint64, tracks: one uint32 depth vector per listed query)"""
    stats = np.zeros((len(queries), 8), np.uint64)
    tracks = []
    for k, q in enumerate(queries):
        q = int(q)
        depth = np.zeros(len(seqs[q]), np.uint32)
        recs = dm.counted(seqs, ext, off, rec, q, min_seq_id, skip)
        for qs, qe in recs:
            depth[qs:qe + 1] += 1
        reads, columns = len(recs), sum(qe - qs + 1 for qs, qe in recs)
        for r in of_query(grecs, k):
            segs = segments(r, gops)
            add_depth(depth, segs)
            reads += 1
            columns += sum(g for _, _, g in segs)
        stats[k] = dm.stats_of(depth, reads, columns, int(edge))
        tracks.append(depth)
    return stats, tracks


def breaks_stats(seqs, ext, off, rec, queries, grecs, gops, anchor, edge, min_span=1, min_span_percent=0, min_seq_id=0.0, skip=False):
    """-> (stats[nq, 8] uint64, tracks: one uint32 span vector per listed query, breaks: BREAK_DTYPE in listed query order, then first)"""
    stats = np.zeros((len(queries), 8), np.uint64)
    tracks, out = [], []
    for k, q in enumerate(queries):
        q = int(q)
        length = len(seqs[q])
        recs = dm.counted(seqs, ext, off, rec, q, min_seq_id, skip)
        depth, span = brm.arrays_of(length, recs, anchor)
        span = np.concatenate((span, [0]))
        reads, columns = len(recs), sum(qe - qs + 1 for qs, qe in recs)
        for r in of_query(grecs, k):
            segs = segments(r, gops)
            add_depth(depth, segs)
            reads += 1
            columns += sum(g for _, _, g in segs)
            s = spanned(segs, anchor)
            if s:
                span[s[0]:s[1] + 1] += 1
        span = span[:length]
        in_window, weak = brm.weak_of(depth, span, int(edge), int(min_span), int(min_span_percent))
        runs = brm.runs_of(weak)
        joins = 0
        for first, last in runs:
            uncovered = int((depth[first:last] == 0).sum())
            joins += uncovered == 0
            out.append((k, first, last, int(span[first:last + 1].min()), uncovered, int(depth[first - 1]), int(depth[last]), brm.GAP if uncovered else brm.JOIN))
        ws = span[in_window]
        stats[k] = [reads, columns, len(ws), int(weak.sum()), len(runs), joins, int(ws.min()) if len(ws) else 0, int(ws.sum())]
        tracks.append(span.astype(np.uint32))
    return stats, tracks, np.array(out, brm.BREAK_DTYPE)


def bases(seqs, ext, off, rec, queries, grecs, gops, mask_ends=0, min_depth=3, min_alt_count=2, min_alt_percent=20, min_seq_id=0.0, skip=False):
    """-> (stats[nq, 8] uint64, counts: one uint32 [length, 8] array per listed query, sites: SITE_DTYPE records)"""
    packed = {}

    def view(i):
        if i not in packed:
            packed[i] = codes_of(seqs[i])
        return packed[i]

    m = int(mask_ends)
    stats = np.zeros((len(queries), 8), np.uint64)
    tables, sites = [], []
    for k, q in enumerate(queries):
        q = int(q)
        counts, reads, columns = bm.count_query(seqs, ext, off, rec, q, m, min_seq_id, skip, view)
        for r in of_query(grecs, k):
            tc, tn = view(int(r["target"]))
            t_len, rev = int(r["tlen"]), bool(int(r["flags"]) & gm.REVERSE)
            reads += 1
            for p, o, g in segments(r, gops):
                columns += g
                for j in range(g):
                    at = t_len - 1 - (o + j) if rev else o + j           # the position in the read's own orientation
                    if tn[at] or (m > 0 and (at < m or t_len - 1 - at < m)):
                        continue
                    b = int(tc[at])
                    counts[p + j][4 * rev + (3 - b if rev else b)] += 1
        qc, qn = view(q)
        ref = np.where(qn != 0, 4, qc).astype(np.int64)
        major, flags, d, t = bm.classify(counts, ref, min_depth, min_alt_count, min_alt_percent)
        rows = np.arange(len(ref))
        at_ref = t[rows, np.minimum(ref, 3)]
        flagged = (flags & (bm.DIFFERS | bm.VARIABLE)) != 0
        stats[k] = [reads, columns, int(d.sum()), int((d - at_ref)[ref != 4].sum()), int((flags & bm.CALLED != 0).sum()), int((flags & bm.DIFFERS != 0).sum()),
                    int((flags & bm.VARIABLE != 0).sum()), int(flagged.sum())]
        tables.append(counts)
        for p in np.flatnonzero(flagged):
            sites.append((k, int(p), int(ref[p]) | int(major[p]) << 4 | int(flags[p]) << 8, counts[p]))
    out = np.zeros(len(sites), bm.SITE_DTYPE)
    for i, s in enumerate(sites):
        out[i] = s
    return stats, tables, out


def single_m(seqs, ext, off, rec, queries, pick, min_seq_id=0.0, skip=False):
    """The single-M property's input: every record i of a listed query that the ungapped rule counts and for which pick(i) holds
    leaves the set and comes back as a gapped record of one M operation -> (off, rec, grecs, gops)"""
    thr = np.float32(min_seq_id)
    rows, stay = [], np.ones(len(rec), bool)
    for k, q in enumerate(queries):
        q = int(q)
        for i in range(int(off[q]), int(off[q + 1])):
            r = rec[i]
            t = int(r["target"])
            if t == q or not (np.float32(r["seq_id"]) >= thr) or (skip and ext[t]) or not pick(i):
                continue
            t_len = len(seqs[t])
            qs, qe, ds, _, rev = orient(r, t_len)
            n = qe - qs + 1
            rows.append((k, qs, i, (k, t, qs, n, ds, t_len, n, 0, gm.REVERSE if rev else 0, 1, 0, 0)))
            stay[i] = False
    rows.sort(key=lambda x: x[:3])
    grecs = np.zeros(len(rows), gm.GAP_DTYPE)
    for j, (_, _, _, f) in enumerate(rows):
        grecs[j] = f + (j, 0)
    gops = np.array([int(f[3]) << 2 | gm.OP_M for _, _, _, f in rows], np.uint32)
    kept = np.concatenate(([0], np.cumsum(stay)))
    return kept[off.astype(np.int64)].astype(np.uint64), rec[stay], grecs, gops
