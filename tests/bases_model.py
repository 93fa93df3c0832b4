"""The statistic of cdm_pileup_bases (include/carpedeam_hip.h) in numpy, written from its definition: every counted record of a listed
query adds its columns, as one vector, to the query's [position][8] counters; the flags and the eight figures are read off that table.
tests/test_bases_model.py holds it against a literal per-column implementation on strings and a hand-counted case; the device is held
against it.  The three text writers give what `carpedeam contig_variants` writes for these results."""
import numpy as np

from pileup_model import codes_of, csr, orient, unorient  # noqa: F401  (csr, unorient: for the users of this module)

NAMES = ("reads", "columns", "bases", "mismatches", "called", "differs", "variable", "flagged")
CALLED, DIFFERS, VARIABLE = 1, 2, 4
SITE_DTYPE = np.dtype([("query", "<u4"), ("pos", "<u4"), ("info", "<u4"), ("counts", "<u4", (8,))])
DEFAULTS = dict(mask_ends=0, min_depth=3, min_alt_count=2, min_alt_percent=20)


def count_query(seqs, ext, off, rec, q, mask_ends, min_seq_id, skip, view):
    """-> (counts[len, 8] uint32, reads, columns) of query q"""
    counts = np.zeros((len(seqs[q]), 8), np.uint32)
    reads = columns = 0
    thr = np.float32(min_seq_id)
    for r in rec[int(off[q]):int(off[q + 1])]:
        t = int(r["target"])
        if t == q or not (np.float32(r["seq_id"]) >= thr):
            continue
        if skip and ext[t]:
            continue
        tc, tn = view(t)
        t_len = len(tc)
        qs, qe, ds, de, rev = orient(r, t_len)
        reads += 1
        columns += qe - qs + 1
        c = np.arange(qe - qs + 1)
        op = ds + c
        p = t_len - 1 - op if rev else op           # the position in the read's own orientation
        ok = tn[p] == 0
        if mask_ends > 0:
            ok &= (p >= mask_ends) & (t_len - 1 - p >= mask_ends)
        b = tc[p].astype(np.int64)
        if rev:
            b = 3 - b                               # the read base as the contig's strand sees it
        np.add.at(counts, ((qs + c)[ok], (4 * int(rev) + b)[ok]), 1)
    return counts, reads, columns


def classify(counts, ref, min_depth, min_alt_count, min_alt_percent):
    """-> (major, flags, depth, t) per position; ref: the contig's code, 4 for N"""
    t = counts[:, :4].astype(np.int64) + counts[:, 4:].astype(np.int64)
    n = len(t)
    d = t.sum(axis=1)
    rows = np.arange(n)
    major = np.argmax(t, axis=1) if n else np.zeros(0, np.int64)      # (the lowest code among equal largest)
    safe = np.minimum(ref, 3)
    take_ref = (ref < 4) & (t[rows, safe] == t[rows, major])
    major = np.where(take_ref, safe, major)
    rest = t.copy()
    rest[rows, major] = -1
    second = rest.max(axis=1) if n else np.zeros(0, np.int64)
    called = d >= min_depth
    differs = called & (major != ref) & (t[rows, major] > second)
    variable = called & (second >= min_alt_count) & (second * 100 >= min_alt_percent * d)
    flags = called * CALLED + differs * DIFFERS + variable * VARIABLE
    return major, flags.astype(np.int64), d, t


def bases(seqs, ext, off, rec, queries, mask_ends=0, min_depth=3, min_alt_count=2, min_alt_percent=20, min_seq_id=0.0, skip=False):
    """-> (stats[nq, 8] uint64, counts: one uint32 [length, 8] array per listed query, sites: SITE_DTYPE records)"""
    packed = {}

    def view(i):
        if i not in packed:
            packed[i] = codes_of(seqs[i])
        return packed[i]

    stats = np.zeros((len(queries), 8), np.uint64)
    tables, sites = [], []
    for k, q in enumerate(queries):
        q = int(q)
        counts, reads, columns = count_query(seqs, ext, off, rec, q, int(mask_ends), min_seq_id, skip, view)
        qc, qn = view(q)
        ref = np.where(qn != 0, 4, qc).astype(np.int64)
        major, flags, d, t = classify(counts, ref, min_depth, min_alt_count, min_alt_percent)
        rows = np.arange(len(ref))
        at_ref = t[rows, np.minimum(ref, 3)]
        flagged = (flags & (DIFFERS | VARIABLE)) != 0
        stats[k] = [reads, columns, int(d.sum()), int((d - at_ref)[ref != 4].sum()), int((flags & CALLED != 0).sum()), int((flags & DIFFERS != 0).sum()),
                    int((flags & VARIABLE != 0).sum()), int(flagged.sum())]
        tables.append(counts)
        for p in np.flatnonzero(flagged):
            sites.append((k, int(p), int(ref[p]) | int(major[p]) << 4 | int(flags[p]) << 8, counts[p]))
    out = np.zeros(len(sites), SITE_DTYPE)
    for i, s in enumerate(sites):
        out[i] = s
    return stats, tables, out


# ------------------------------------------------------------------------------------------------ the texts of `carpedeam contig_variants`
SUMMARY_HEADER = "\t".join(("name", "key", "length") + NAMES[:7]) + "\n"
LETTERS = "ACGTN"


def summary_tsv(names, keys, lengths, stats):
    out = [SUMMARY_HEADER]
    for i, name in enumerate(names):
        out.append("\t".join([name, str(int(keys[i])), str(int(lengths[i]))] + [str(int(stats[i][c])) for c in range(7)]) + "\n")
    return "".join(out)


def sites_tsv(names, sites):
    """name pos(1-based) ref major flags depth A C G T a c g t"""
    out = []
    for s in sites:
        info = int(s["info"])
        fl = info >> 8
        c = [int(x) for x in s["counts"]]
        out.append("\t".join([names[int(s["query"])], str(int(s["pos"]) + 1), LETTERS[info & 15], LETTERS[(info >> 4) & 15],
                              ("D" if fl & DIFFERS else "") + ("V" if fl & VARIABLE else ""), str(sum(c))] + [str(x) for x in c]) + "\n")
    return "".join(out)


def consensus_fasta(names, seqs, sites):
    """the input's own letters, the upper-case major at the DIFFERS positions"""
    letters = [list(s) for s in seqs]
    for s in sites:
        info = int(s["info"])
        if (info >> 8) & DIFFERS:
            letters[int(s["query"])][int(s["pos"])] = LETTERS[(info >> 4) & 15]
    return "".join(">%s\n%s\n" % (n, "".join(l)) for n, l in zip(names, letters))
