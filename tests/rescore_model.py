"""rescorediagonal --rescore-mode 3 (query DB == target DB) restated in numpy, exactly: what tests/test_rescore_directed.py holds to
the reference's committed text and tests/test_gpu_rescore_directed.py holds cdm_rescore to, field by field.

Written from the reference's rules, not from csrc/rescore.hip: DistanceCalculator.h:93-175, 204-220 (probing of the 16-bit
diagonal, the end-to-end score), rescorediagonal.cpp:145-356 (strand, identity count, gates, reverse-strand coordinates),
Util.cpp:533-598 (canBeCovered, hasCoverage, computeSeqId), StripedSmithWaterman.cpp:1055-1057 (computeCov) and
NucleotideMatrix.cpp:17-61 (the letter mapping).  Integers are Python integers, the float32 steps are numpy float32 scalars.

Input: the letters as the DB holds them (bytes per sequence, index = id), hits (query, target, prefilter score, diagonal) in
query order, and the six parameters.  Output per surviving hit, in hit order: the eight fields of capi.ALN_DTYPE, the
purine/pyrimidine mismatch count as Alns.download_ry returns it, the per-query offsets and the number of identity records with
the coordinates -1.

The E-value gate goes through capi.lib().cdm_evalue: host code that tests/golden/evalue.tsv holds to the reference, not the
kernel's table of smallest passing scores.

A hit that is not an identity hit, scores 0 on every probe and still passes the E-value gate makes the reference count the byte in
front of both sequences: `Undefined` is raised for it (cdm_rescore refuses such a threshold)."""
import numpy as np

from carpedeam_amd import capi

FLT_EPSILON = np.float32(np.finfo(np.float32).eps)
U32 = 0xFFFFFFFF
STAR = ord("*")

# nucleotide.out orders the alphabet A C T G X (NucleotideMatrix.cpp:17-61: toupper, IUPAC codes to one base, the rest to X)
_CODE = np.full(256, 4, np.uint8)
for _letters, _v in (("A", 0), ("CMYH", 1), ("TUW", 2), ("GKBDVRS", 3)):
    for _c in _letters:
        _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _v
_NUM2AA = np.frombuffer(b"ACTGX", np.uint8)
_REVERSE = np.array([2, 3, 0, 1, 4], np.uint8)          # NucleotideMatrix.cpp:9-13
_PYRIMIDINE = np.array([0, 1, 1, 0, 0], np.uint8)       # C and T


class Undefined(Exception):
    """the reference reads outside a sequence for this hit"""


class Params:
    def __init__(self, e=0.001, min_seq_id=0.9, c=0.0, cov_mode=1, min_aln_len=0):
        self.e, self.min_seq_id, self.c, self.cov_mode, self.min_aln_len = float(e), np.float32(min_seq_id), np.float32(c), int(cov_mode), int(min_aln_len)

    def capi(self):
        return capi.RescoreParams(float(self.min_seq_id), self.e, self.cov_mode, float(self.c), 0, self.min_aln_len)

    def flags(self):
        return ["--rescore-mode", "3", "-e", repr(self.e), "--min-seq-id", repr(float(self.min_seq_id)), "--seq-id-mode", "0", "--sort-results", "0", "-a", "0",
                "--filter-hits", "0", "--cov-mode", str(self.cov_mode), "-c", repr(float(self.c)), "--min-aln-len", str(self.min_aln_len)]


class Seq:
    """one sequence: its bytes, mapped codes and case-folded bytes, and the reversed query as rescorediagonal.cpp:173-179 spells it"""

    def __init__(self, letters):
        self.raw = np.frombuffer(bytes(letters), np.uint8)
        self.code = _CODE[self.raw]
        self.plain = bool(np.all(np.isin(self.raw, np.frombuffer(b"ACGT", np.uint8))))
        self._rev = None

    def __len__(self):
        return len(self.raw)

    def strand(self, reverse):
        if not reverse:
            return self.raw, self.code
        if self._rev is None:
            code = _REVERSE[self.code[::-1]]
            self._rev = (_NUM2AA[code], code)
        return self._rev


def can_be_covered(thr, mode, ql, tl):
    ql, tl, one = np.float32(ql), np.float32(tl), np.float32(1.0)
    if mode == 0:
        return bool(ql / tl >= thr and tl / ql >= thr)
    if mode == 1:
        return bool(ql / tl >= thr)
    if mode == 2:
        return bool(tl / ql >= thr)
    if mode == 3:
        return bool(tl / ql >= thr and tl / ql <= one)
    if mode == 4:
        return bool(ql / tl >= thr and ql / tl <= one)
    if mode == 5:
        return bool(min(tl, ql) / max(tl, ql) >= thr)
    return True


def has_coverage(thr, mode, qc, tc):
    if mode == 0:
        return bool(qc >= thr and tc >= thr)
    if mode == 1:
        return bool(tc >= thr)
    if mode == 2:
        return bool(qc >= thr)
    return True


def compute_cov(s, e, length):
    """computeCov(unsigned, unsigned, unsigned): the numerator in 32-bit unsigned arithmetic"""
    s, e = s & U32, e & U32
    return np.float32(np.float32((min(length, max(s, e)) - min(s, e) + 1) & U32) / np.float32(length))


def _one_diagonal(q_raw, q_code, t_raw, t_code, diagonal):
    """ungappedAlignmentByDiagonal in mode 3 -> (score, first, last, query offset, target offset, columns) or None without an overlap"""
    md, q_len, t_len = abs(diagonal), len(q_raw), len(t_raw)
    if diagonal >= 0 and md < q_len:
        qo, to, m = md, 0, min(t_len, q_len - md)
    elif diagonal < 0 and md < t_len:
        qo, to, m = 0, md, min(t_len - md, q_len)
    else:
        return None
    first = 1 if (q_raw[qo] == STAR or t_raw[to] == STAR) else 0
    last = m - 1
    if last > 0 and (q_raw[qo + m - 1] == STAR or t_raw[to + m - 1] == STAR):
        last -= 1
    a, b = q_code[qo + first:qo + last + 1], t_code[to + first:to + last + 1]
    match = int(np.count_nonzero((a == b) & (a != 4)))
    return max(0, 2 * match - 3 * (len(a) - match)), first, last, qo, to, m


def score_hit(q, t, reverse, diagonal):
    """computeUngappedAlignment on the 16-bit diagonal plus what the gates need of the winning probe: None where every probe scores 0,
    else a dict (score, start, end, dist, diagonal, ident, ry)"""
    u = diagonal & 0xFFFF
    q_raw, q_code = q.strand(reverse)
    best = None
    probes = [-d * 65536 + u for d in range(1, 1 + len(t) // 32768 + 1)] + [d * 65536 + u for d in range(0, len(q) // 65536 + 1)]
    for real in probes:
        r = _one_diagonal(q_raw, q_code, t.raw, t.code, real)
        if r is not None and r[0] > (best[0][0] if best else 0):
            best = (r, real)
    if best is None:
        return None
    (score, first, last, qo, to, m), real = best
    # the identity count of rescorediagonal.cpp:278-282, on the case-folded bytes
    a, b = q_raw[qo + first:qo + last + 1] & 0xDF, t.raw[to + first:to + last + 1] & 0xDF
    ry = 0xFFFF
    if q.plain and t.plain:
        ry = min(0xFFFF, int(np.count_nonzero(_PYRIMIDINE[q_code[qo:qo + m]] != _PYRIMIDINE[t.code[to:to + m]])))
    return {"score": score, "start": first, "end": last, "dist": abs(real), "diagonal": real, "ident": int(np.count_nonzero(a == b)), "ry": ry}


def score_set(seqs, hits):
    """the parameter-free part, once per case set: [score_hit] in hit order"""
    S = [Seq(s) for s in seqs]
    return S, [score_hit(S[q], S[t], sc < 0, d) for q, t, sc, d in hits]


def stored_seq_id(seq_id):
    """what a reader of the text record gets back (Util.cpp:278-307): three decimals, cut"""
    if seq_id == np.float32(1.0):
        return np.float32(1.0)
    return np.float32(float(int(np.float32(seq_id * np.float32(1000)))) / 1000.0)


def min_passing_score(q_len, residues, e):
    """the smallest score whose E-value passes, None where 2 * q_len does not"""
    ev = capi.lib().cdm_evalue
    for s in range(0, 2 * q_len + 1):
        if ev(float(s), float(q_len), residues) <= e:
            return s
    return None


def apply(seqs, hits, scored, par):
    """the gates of rescorediagonal.cpp:204-314 on the scored hits -> (off, rec, ry, undefined identity records)"""
    ev = capi.lib().cdm_evalue
    lens = [len(s) for s in seqs]
    residues = sum(lens)
    off = np.zeros(len(seqs) + 1, np.uint64)
    recs, rys, undefined = [], [], 0
    pass_cache = {}
    for (q, t, sc, _), al in zip(hits, scored):
        q_len, t_len, reverse, identity = lens[q], lens[t], sc < 0, q == t
        if not can_be_covered(par.c, par.cov_mode, q_len, t_len):
            continue
        score = al["score"] if al else 0
        key = (score, q_len)
        if key not in pass_cache:
            pass_cache[key] = ev(float(score), float(q_len), residues) <= par.e
        has_evalue = pass_cache[key]
        if al is None:
            if not identity:
                if has_evalue:
                    raise Undefined("hit (%d, %d): score 0 passes -e %g" % (q, t, par.e))
                continue
            if reverse:
                raise Undefined("identity hit of %d on the reverse strand scores 0" % q)
            # the alignment's constructor values: start = end = -1, one compared byte in front of the sequence, equal to itself
            recs.append((t, 0, 1, -1, -1, -1, -1, np.float32(1.0)))
            rys.append(0xFFFF)
            off[q + 1] += 1
            undefined += 1
            continue
        start, end, dist = al["start"], al["end"], al["dist"]
        aln_len = end - start + 1
        if al["diagonal"] >= 0:
            qs, qe, ds, de = start + dist, end + dist, start, end
        else:
            qs, qe, ds, de = start, end, start + dist, end + dist
        seq_id = np.float32(0.0)
        if has_evalue or identity:
            seq_id = np.float32(np.float32(al["ident"]) / np.float32(aln_len))
        q_cov, t_cov = compute_cov(qs, qe, q_len), compute_cov(ds, de, t_len)
        if reverse:
            qs, qe = q_len - qs - 1, q_len - qe - 1
        has_cov = has_coverage(par.c, par.cov_mode, q_cov, t_cov)
        has_seq_id = float(seq_id) >= float(np.float32(par.min_seq_id - FLT_EPSILON))
        has_aln_len = aln_len >= par.min_aln_len
        if identity or (has_aln_len and has_cov and has_seq_id and has_evalue):
            recs.append((t, al["score"], al["ident"], qs, qe, ds, de, stored_seq_id(seq_id)))
            rys.append(al["ry"])
            off[q + 1] += 1
    off = np.cumsum(off).astype(np.uint64)
    rec = np.array(recs, capi.ALN_DTYPE) if recs else np.empty(0, capi.ALN_DTYPE)
    return off, rec, np.array(rys, np.uint16), undefined


def to_text(seqs, off, rec):
    """the model's records as the alignment DB's text, keyed by sequence id"""
    lens = np.array([len(s) for s in seqs], np.int64)
    keys = np.arange(len(seqs))
    return {k: (v, 0) for k, v in capi.alns_to_text(off, rec, keys, lens, int(lens.sum())).items()}
