"""The statistic of cdm_pileup_profile (include/carpedeam_hip.h) in numpy, written from its definition: a loop over the records of
every listed query, the columns of a record as one vector, on ASCII sequences.  tests/test_pileup_model.py holds it against
hand-counted tables and against a second, literal implementation on strings; the device is held against it."""
import numpy as np

ALN_DTYPE = np.dtype([("target", "<u4"), ("raw_score", "<i4"), ("ident", "<i4"), ("q_start", "<i4"), ("q_end", "<i4"),
                      ("db_start", "<i4"), ("db_end", "<i4"), ("seq_id", "<f4")])

# what the sequence DB holds for a letter (NucleotideMatrix::setupLetterMapping as cdm_seqdb_upload packs it): a code A,C,G,T = 0..3
# for the letter, its upper case or the base an IUPAC code stands for first, and the N bit for everything else
_TO = {}
for _group, _code in (("A", 0), ("CMYH", 1), ("GKBDVRS", 2), ("TUW", 3)):
    for _c in _group:
        _TO[_c] = _TO[_c.lower()] = _code


def letter(c):
    """(code, isN) of one ASCII letter"""
    if isinstance(c, int):
        c = chr(c)
    return (_TO[c], 0) if c in _TO else (0, 1)


def codes_of(seq):
    """(codes, nbits) of a sequence as uint8 arrays"""
    if isinstance(seq, bytes):
        seq = seq.decode()
    pairs = [letter(c) for c in seq]
    return np.array([p[0] for p in pairs], np.uint8), np.array([p[1] for p in pairs], np.uint8)


def orient(r, t_len):
    """correction.cpp:229-242: (qs, qe, ds, de, rev) of a record on a target of t_len letters"""
    if int(r["q_start"]) > int(r["q_end"]):
        return int(r["q_end"]), int(r["q_start"]), t_len - int(r["db_end"]) - 1, t_len - int(r["db_start"]) - 1, True
    return int(r["q_start"]), int(r["q_end"]), int(r["db_start"]), int(r["db_end"]), False


def unorient(target, qs, qe, ds, de, rev, t_len, seq_id=1.0):
    """the record whose oriented form is (qs, qe, ds, de, rev): the inverse of orient() (a reverse record needs qe > qs)"""
    if rev:
        assert qe > qs
        return (target, 0, 0, qe, qs, t_len - 1 - de, t_len - 1 - ds, seq_id)
    return (target, 0, 0, qs, qe, ds, de, seq_id)


def csr(n, per_query):
    """per_query: {query: [record tuples]} -> (offsets[n + 1], records)"""
    off = np.zeros(n + 1, np.uint64)
    recs = []
    for q in range(n):
        recs += per_query.get(q, [])
        off[q + 1] = len(recs)
    return off, (np.array(recs, ALN_DTYPE) if recs else np.empty(0, ALN_DTYPE))


def profile(seqs, ext, off, rec, queries, ends, min_seq_id=0.0, skip_extended_targets=False):
    """-> (counts[nq, 2, ends, 4, 4], reads[nq], columns[nq]) as uint64"""
    packed = {}

    def view(i):
        if i not in packed:
            packed[i] = codes_of(seqs[i])
        return packed[i]

    P = int(ends)
    nq = len(queries)
    counts = np.zeros((nq, 2, P, 4, 4), np.uint64)
    reads, columns = np.zeros(nq, np.uint64), np.zeros(nq, np.uint64)
    thr = np.float32(min_seq_id)
    for k, q in enumerate(queries):
        q = int(q)
        qc, qn = view(q)
        for r in rec[int(off[q]):int(off[q + 1])]:
            t = int(r["target"])
            if t == q or not (np.float32(r["seq_id"]) >= thr):
                continue
            if skip_extended_targets and ext[t]:
                continue
            tc, tn = view(t)
            t_len = len(tc)
            qs, qe, ds, de, rev = orient(r, t_len)
            reads[k] += 1
            columns[k] += qe - qs + 1
            c = np.arange(qe - qs + 1)
            qpos, op = qs + c, ds + c
            p = t_len - 1 - op if rev else op           # the position in the read's own orientation
            y = tc[p].astype(np.int64)
            x = qc[qpos].astype(np.int64)
            if rev:
                x = 3 - x                               # the contig base as the read's strand sees it
            ok = (qn[qpos] == 0) & (tn[p] == 0)
            d5, d3 = p, t_len - 1 - p
            m5, m3 = ok & (d5 < P), ok & (d3 < P)
            np.add.at(counts[k, 0], (d5[m5], x[m5], y[m5]), 1)
            np.add.at(counts[k, 1], (d3[m3], x[m3], y[m3]), 1)
    return counts, reads, columns


def tsv_header(ends):
    cols = ["name", "key", "length", "reads", "columns"]
    for d in range(1, ends + 1):
        cols += ["5p_C_%d" % d, "5p_CT_%d" % d, "3p_G_%d" % d, "3p_GA_%d" % d]
    return "\t".join(cols) + "\n"


def tsv(names, keys, lengths, counts, reads, columns):
    """the table `carpedeam contig_damage` writes for these counts"""
    ends = counts.shape[2]
    out = [tsv_header(ends)]
    for i, name in enumerate(names):
        f = [name, str(int(keys[i])), str(int(lengths[i])), str(int(reads[i])), str(int(columns[i]))]
        for d in range(ends):
            c5, c3 = counts[i, 0, d], counts[i, 1, d]
            f += [str(int(c5[1].sum())), str(int(c5[1, 3])), str(int(c3[2].sum())), str(int(c3[2, 0]))]
        out.append("\t".join(f) + "\n")
    return "".join(out)
