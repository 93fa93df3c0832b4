"""cdm_pileup_gapped (include/carpedeam_hip.h) in plain Python / numpy, integers only: the banded affine-gap overlap alignment of a
read on a contig, written twice - align_pair() is the textbook three-matrix form with explicit traceback, the yardstick; align_rows()
is the row-by-row form of the kernel (a lane per diagonal of the band, the deletion as a prefix maximum along the row) - then the
candidates, records, primary rule and statistics of the call, the text `carpedeam contig_map --gapped 1` writes (sam_text_gapped) and
a check of such a text from the contigs alone (sam_check_gapped).  The reference project has nothing like it: this file is the
specification, tests/test_gapped_model.py holds its two halves against each other and against hand-computed answers."""
import re
from itertools import accumulate

import numpy as np

import map_model as mm
from pileup_model import orient

NAMES = ("candidates", "rescued", "gap_letters", "too_long")
FIELDS = ("query", "target", "pos", "span", "tstart", "tlen", "columns", "nm", "flags", "n_ops", "n_words")
GAP_DTYPE = np.dtype([(n, "<u4") for n in FIELDS] + [("score", "<i4"), ("ops", "<u8"), ("words", "<u8")])
REVERSE, SECONDARY = mm.REVERSE, mm.SECONDARY
OP_M, OP_I, OP_D = 0, 1, 2
DELETED = 15                # the `read` field of the word of a deleted contig letter
MAX_TLEN = 4096
NEG = -(1 << 28)            # "no path": below every score a path can have


class Params:
    """cdm_gap_params with the command's values"""

    def __init__(self, min_seq_id=0.0, skip=False, band=8, min_columns=32, min_id_permille=900, match=2, mismatch=-3, gap_open=5, gap_extend=2):
        self.min_seq_id, self.skip, self.band, self.min_columns, self.min_id_permille = min_seq_id, skip, band, min_columns, min_id_permille
        self.match, self.mismatch, self.gap_open, self.gap_extend = match, mismatch, gap_open, gap_extend


def real_diagonals(diagonal, n, L, rev):
    """the contig-forward diagonals i - j of a hit's 16-bit diagonal, in the order k_rescore probes them, those with an overlap"""
    u = int(diagonal) & 0xFFFF
    probes = [u - 65536 * d for d in range(1, 2 + L // 32768)] + [u + 65536 * d for d in range(0, n // 65536 + 1)]
    return [(n - L - D if rev else D) for D in probes if (0 <= D < n) or (D < 0 and -D < L)]


def hit_diagonal(Df, n, L, rev):
    """the 16-bit diagonal a hit carries (a signed short, as kmermatcher writes it) for the contig-forward diagonal Df: the inverse of
    real_diagonals, for the tests' inputs"""
    return ((((n - L - Df) if rev else Df) & 0xFFFF) ^ 0x8000) - 0x8000


def column_score(a, b, p):
    return p.match if a < 4 and b < 4 and a == b else p.mismatch


# ------------------------------------------------------------------------------------------------ the yardstick
def align_pair(Q, R, Df, B, p):
    """Q: the contig's codes (0..3, 4 = N), R: the read's in the contig's orientation.  Cells (i, j) with |i - j - Df| <= B.
    H/E/F as explicit arrays; E: the read letter j stands alone (insertion), F: the contig letter i stands alone (deletion).
    -> None (no end cell in the band) or dict(score, start=(i, j), end=(i, j), ops=[(op, length)] first to last)"""
    n, L = len(Q), len(R)
    go, ge = p.gap_open, p.gap_extend
    base, top = max(0, Df - B), min(n - 1, L - 1 + Df + B)      # the contig letters the band reaches: row i of the arrays is letter base + i
    if top < base:
        return None
    Q = Q[base:top + 1]
    Df, n = Df - base, top - base + 1
    a = align_band(Q, R, Df, B, n, L, go, ge, p)
    if a is not None:
        a["start"], a["end"] = (a["start"][0] + base, a["start"][1]), (a["end"][0] + base, a["end"][1])
    return a


def align_band(Q, R, Df, B, n, L, go, ge, p):
    """align_pair's arrays over the stretch of the contig the band reaches (n letters here).  Where the stretch is cut short of the
    contig's first letter its row 0 holds the one cell with j = 0, where it is cut short of the last its row n - 1 the one cell with
    j = L - 1: `i == 0` and `i == n - 1` below then add nothing to `j == 0` and `j == L - 1`, and mean the contig's ends otherwise"""
    M = [[NEG] * L for _ in range(n)]
    H = [[NEG] * L for _ in range(n)]
    E = [[NEG] * L for _ in range(n)]
    F = [[NEG] * L for _ in range(n)]
    best = None
    for j in range(L):
        for i in range(max(0, j + Df - B), min(n - 1, j + Df + B) + 1):
            off = i - j - Df        # the cell's diagonal within the band, -B .. B
            m = column_score(Q[i], R[j], p) + (H[i - 1][j - 1] if i > 0 and j > 0 else 0)
            e = f = NEG
            if j > 0 and off + 1 <= B:          # (i, j - 1) is a cell of the band
                e = max(H[i][j - 1] - go, E[i][j - 1] - ge)
            if i > 0 and off - 1 >= -B:         # (i - 1, j) is
                f = max(H[i - 1][j] - go, F[i - 1][j] - ge)
            M[i][j], E[i][j], F[i][j], H[i][j] = m, e, f, max(m, e, f)
            if (j == L - 1 or i == n - 1) and (best is None or (m, -i, -j) > best):
                best = (m, -i, -j)
    if best is None:
        return None
    score, i, j = best[0], -best[1], -best[2]
    end = (i, j)
    steps, state = [], OP_M
    while True:
        steps.append(state)
        if state == OP_M:
            if i == 0 or j == 0:
                break
            i, j = i - 1, j - 1
            nxt = None
        elif state == OP_D:
            nxt = OP_D if F[i - 1][j] - ge >= H[i - 1][j] - go else None
            i -= 1
        else:
            nxt = OP_I if E[i][j - 1] - ge >= H[i][j - 1] - go else None
            j -= 1
        if nxt is None:         # the state H[i][j] came from: M, then D, then I
            nxt = OP_M if M[i][j] >= E[i][j] and M[i][j] >= F[i][j] else OP_D if F[i][j] >= E[i][j] else OP_I
        state = nxt
    return dict(score=score, start=(i, j), end=end, ops=merge(reversed(steps)))


def merge(steps):
    ops = []
    for s in steps:
        if ops and ops[-1][0] == s:
            ops[-1][1] += 1
        else:
            ops.append([s, 1])
    return [(o, l) for o, l in ops]


# ------------------------------------------------------------------------------------------------ the kernel's form
def group_width(B):
    return 16 if 2 * B + 1 <= 16 else 32 if 2 * B + 1 <= 32 else 64


def align_rows(Q, R, Df, B, p):
    """the same alignment a row per read letter: lane k of G holds the cell i = j + Df + k - B.  M reads the lane's own previous row, E
    the previous row's lane k + 1; F = max over k' < k of H0[k'] - open - extend (k - k' - 1), H0 = max(M, E), as one inclusive prefix
    maximum of H0[k'] + extend k' in log2 G shuffle steps (exact for open >= extend); four trace bits per cell, taken after the scan from
    the neighbour lane's final H and F: bits 0-1 the state H came from (0 M, 1 D, 2 I), bit 2 E extended, bit 3 F extended"""
    n, L = len(Q), len(R)
    go, ge = p.gap_open, p.gap_extend
    G, W = group_width(B), 2 * B + 1
    j0, j1 = max(0, -Df - B), min(L - 1, n - 1 - Df + B)
    if j1 < j0:
        return None
    Hp, Ep = [NEG] * G, [NEG] * G
    trace = []
    best = [None] * G
    for j in range(j0, j1 + 1):
        Mv, Ev, Fv, Hv, eext, row = [NEG] * G, [NEG] * G, [NEG] * G, [NEG] * G, [0] * G, [0] * G
        lo, hi = max(0, B - j - Df), min(W - 1, n - 1 - j - Df + B)        # the lanes whose cell lies on the contig
        for k in range(lo, hi + 1):
            i = j + Df + k - B
            Mv[k] = column_score(Q[i], R[j], p) + (Hp[k] if i > 0 and j > 0 else 0)
            hu, eu = Hp[k + 1], Ep[k + 1]           # (W is odd, G even: lane k + 1 exists, and holds NEG beyond the band)
            Ev[k] = max(hu - go, eu - ge)
            eext[k] = 1 if eu - ge >= hu - go else 0
            if (j == L - 1 or i == n - 1) and (best[k] is None or Mv[k] > best[k][0]):       # (i and j ascend in a lane: the first of equals stays)
                best[k] = (Mv[k], -i, -j)
        # inclusive prefix maximum over the lanes (the kernel: log2 G shuffle steps), then every lane reads its left neighbour's
        scan = list(accumulate((max(Mv[k], Ev[k]) + ge * k if lo <= k <= hi else NEG for k in range(G)), max))
        for k in range(lo, hi + 1):
            if k > 0:
                Fv[k] = scan[k - 1] - go - ge * (k - 1)
            Hv[k] = max(Mv[k], Ev[k], Fv[k])
        for k in range(lo, hi + 1):
            src = 0 if Mv[k] >= Ev[k] and Mv[k] >= Fv[k] else 1 if Fv[k] >= Ev[k] else 2
            fext = 1 if k > 0 and Fv[k - 1] - ge >= Hv[k - 1] - go else 0
            row[k] = src | eext[k] << 2 | fext << 3
        trace.append(row)
        Hp, Ep = Hv, Ev
    found = [b for b in best if b is not None]
    if not found:
        return None
    score, i, j = max(found)
    i, j = -i, -j
    end = (i, j)
    steps, state = [], OP_M
    while True:
        steps.append(state)
        bits = trace[j - j0][i - j - Df + B]
        if state == OP_M:
            if i == 0 or j == 0:
                break
            i, j, ext = i - 1, j - 1, False
        elif state == OP_D:
            ext = bool(bits & 8)
            i -= 1
        else:
            ext = bool(bits & 4)
            j -= 1
        if not ext:
            state = (OP_M, OP_D, OP_I)[trace[j - j0][i - j - Df + B] & 3]
    return dict(score=score, start=(i, j), end=end, ops=merge(reversed(steps)))


# ------------------------------------------------------------------------------------------------ from an alignment to a record
def describe(Q, R, a):
    """the counts and words of an alignment: dict(pos, span, tstart, columns, matches, inserted, deleted, ops words, mismatch words)"""
    i, j = a["start"]
    pos, words, matches, ins, dele = i, [], 0, 0, 0
    for op, length in a["ops"]:
        for _ in range(length):
            if op == OP_M:
                if Q[i] < 4 and R[j] < 4 and Q[i] == R[j]:
                    matches += 1
                else:
                    words.append((i - pos) | int(Q[i]) << 24 | int(R[j]) << 28)
                i, j = i + 1, j + 1
            elif op == OP_I:
                ins += 1
                j += 1
            else:
                words.append((i - pos) | int(Q[i]) << 24 | DELETED << 28)
                dele += 1
                i += 1
    assert (i - 1, j - 1) == a["end"] and a["ops"][0][0] == OP_M and a["ops"][-1][0] == OP_M
    m_cols = sum(l for o, l in a["ops"] if o == OP_M)
    return dict(pos=pos, span=i - pos, tstart=a["start"][1], columns=j - a["start"][1], matches=matches, m_cols=m_cols, inserted=ins, deleted=dele,
                ops=[l << 2 | o for o, l in a["ops"]], words=words, score=a["score"])


def accepted(d, p):
    return d["score"] > 0 and d["columns"] >= p.min_columns and d["matches"] * 1000 >= p.min_id_permille * (d["m_cols"] + d["inserted"] + d["deleted"])


def best_alignment(Q, R, diagonal, rev, p, align=align_pair):
    """over the hit's real diagonals: the greatest score, among equals the first in probe order -> (alignment, Df) or None"""
    best = None
    for Df in real_diagonals(diagonal, len(Q), len(R), rev):
        a = align(Q, R, Df, p.band, p)
        if a is not None and (best is None or a["score"] > best[0]["score"]):
            best = (a, Df)
    return best


def oriented_codes(seq, rev):
    c = mm.codes(seq)
    return np.where(c[::-1] == 4, 4, 3 - c[::-1]) if rev else c


def gapped_records(seqs, ext, hoff, hits, aoff, arec, queries, p, align=align_pair):
    """-> (stats[nq, 4] uint64, recs: GAP_DTYPE, ops: uint32, words: uint32)"""
    thr = np.float32(p.min_seq_id)
    counted_pairs, counted_targets = set(), set()
    for q in queries:
        q = int(q)
        for r in range(int(aoff[q]), int(aoff[q + 1])):
            a = arec[r]
            t = int(a["target"])
            if t == q or t >= len(seqs) or not (np.float32(a["seq_id"]) >= thr) or (p.skip and ext[t]):
                continue
            qs, qe, ds, de, _ = orient(a, len(seqs[t]))
            if qs < 0 or ds < 0 or qe < qs or qe >= len(seqs[q]) or de >= len(seqs[t]) or qe - qs != de - ds:
                continue
            counted_pairs.add((q, t))
            counted_targets.add(t)
    stats = np.zeros((len(queries), 4), np.uint64)
    rows = []
    for k, q in enumerate(queries):
        q = int(q)
        Q = mm.codes(seqs[q])
        for h in range(int(hoff[q]), int(hoff[q + 1])):
            t, rev = int(hits[h]["target"]), int(hits[h]["score"]) < 0
            if t == q or t >= len(seqs) or (p.skip and ext[t]) or (q, t) in counted_pairs:
                continue
            if len(seqs[t]) > MAX_TLEN:
                stats[k][3] += 1
                continue
            stats[k][0] += 1
            R = oriented_codes(seqs[t], rev)
            best = best_alignment(Q, R, int(hits[h]["diagonal"]), rev, p, align)
            if best is None:
                continue
            d = describe(Q, R, best[0])
            if not accepted(d, p):
                continue
            stats[k][1] += 1
            stats[k][2] += d["inserted"] + d["deleted"]
            rows.append(dict(d, k=k, h=h, target=t, tlen=len(seqs[t]), rev=rev))
    best = {}
    for row in rows:
        key = (row["columns"], -row["h"])
        if row["target"] not in counted_targets and (row["target"] not in best or key > best[row["target"]]):
            best[row["target"]] = key
    rows.sort(key=lambda row: (row["k"], row["pos"], row["h"]))
    recs = np.zeros(len(rows), GAP_DTYPE)
    ops, words = [], []
    for i, row in enumerate(rows):
        primary = best.get(row["target"]) == (row["columns"], -row["h"])
        flags = (REVERSE if row["rev"] else 0) | (0 if primary else SECONDARY)
        recs[i] = (row["k"], row["target"], row["pos"], row["span"], row["tstart"], row["tlen"], row["columns"], len(row["words"]) + row["inserted"], flags,
                   len(row["ops"]), len(row["words"]), row["score"], len(ops), len(words))
        ops += row["ops"]
        words += row["words"]
    return stats, recs, np.array(ops, np.uint32), np.array(words, np.uint32)


# ------------------------------------------------------------------------------------------------ the text of `contig_map --gapped 1`
def cigar_of(ops, tstart, tlen):
    read = sum(int(w) >> 2 for w in ops if int(w) & 3 != OP_D)
    right = tlen - tstart - read
    return ("%dS" % tstart if tstart else "") + "".join("%d%s" % (int(w) >> 2, "MID"[int(w) & 3]) for w in ops) + ("%dS" % right if right else "")


def md_gapped(words, span):
    """match-run length, then the contig's letter of a mismatch or ^ and the contig's letters of a deletion; a deleted letter joins
    the ^ in front of it when it follows a deleted letter on the contig"""
    out, at, in_del = [], 0, False
    for w in words:
        w = int(w)
        c, ref, deleted = w & 0xFFFFFF, mm.LETTERS[(w >> 24) & 15], (w >> 28) == DELETED
        if deleted and in_del and c == at:
            out.append(ref)
        else:
            out.append("%d%s%s" % (c - at, "^" if deleted else "", ref))
        at, in_del = c + 1, deleted
    return "".join(out) + str(span - at)


def gap_letters(ops):
    return sum(int(w) >> 2 for w in ops if int(w) & 3 != OP_M)


def sam_text_gapped(contig_names, contig_lengths, read_name, read_seq, recs, mism, grecs, gops, gwords, read_group=None, primary_only=False):
    """the merged file: the lines of map_model.sam_text() and the rescued lines, by (contig, pos), the ungapped first on equal keys"""
    plain = mm.sam_text(contig_names, contig_lengths, read_name, read_seq, recs, mism, read_group=read_group).split("\n")[:-1]
    head = [l for l in plain if l.startswith("@")]
    body = [l for l in plain if not l.startswith("@")]
    assert len(body) == len(recs)
    lines = []
    for r, l in zip(recs, body):
        if not (primary_only and int(r["flags"]) & SECONDARY):
            lines.append(((int(r["query"]), int(r["pos"]), 0), l))
    for r in grecs:
        flags = int(r["flags"])
        if primary_only and flags & SECONDARY:
            continue
        t = int(r["target"])
        seq = mm.mapped(read_seq(t))
        if flags & REVERSE:
            seq = seq.translate(mm.COMPLEMENT)[::-1]
        ops = gops[int(r["ops"]):int(r["ops"]) + int(r["n_ops"])]
        words = gwords[int(r["words"]):int(r["words"]) + int(r["n_words"])]
        f = [read_name(t), str((16 if flags & REVERSE else 0) | (256 if flags & SECONDARY else 0)), contig_names[int(r["query"])], str(int(r["pos"]) + 1), "255",
             cigar_of(ops, int(r["tstart"]), int(r["tlen"])), "*", "0", "0", seq, "*", "NM:i:%d" % int(r["nm"]), "MD:Z:" + md_gapped(words, int(r["span"]))]
        if read_group is not None:
            f.append("RG:Z:" + read_group)
        f.append("XG:i:%d" % gap_letters(ops))
        lines.append(((int(r["query"]), int(r["pos"]), 1), "\t".join(f)))
    lines.sort(key=lambda x: x[0])          # (stable: either stream keeps its own order)
    return "\n".join(head + [l for _, l in lines]) + "\n"


CIGAR = re.compile(r"^(?:(\d+)S)?((?:\d+[MID])+)(?:(\d+)S)?$")
MD = re.compile(r"^\d+(?:(?:[ACGTN]|\^[ACGTN]+)\d+)*$")


def sam_check_gapped(text, contigs):
    """contigs: {name: ASCII letters}.  Raises ValueError naming the first line that does not hold: CIGAR's S, M and I sum to len(SEQ), its
    first and last operation inside the clips is M; SEQ, CIGAR and MD rebuild the contig's mapped letters at POS..; a match column holds no
    N, a mismatch column differs or holds an N; NM is the mismatches plus the inserted and deleted letters; XG, where a line has it, the
    inserted plus deleted letters, and a line without it has neither; the lines are sorted by (@SQ order, POS); every QNAME has exactly
    one line without 256.  -> (reads with lines, lines with XG)"""
    order, primaries, last, rescued = {}, {}, (-1, -1), 0
    for no, line in enumerate(text.split("\n")[:-1], 1):
        def fail(what):
            raise ValueError("line %d: %s: %s" % (no, what, line[:200]))
        f = line.split("\t")
        if line.startswith("@"):
            if f[0] == "@SQ":
                name = f[1][3:]
                if name in order:
                    fail("@SQ twice")
                if name not in contigs or int(f[2][3:]) != len(contigs[name]):
                    fail("@SQ names no contig of that length")
                order[name] = len(order)
            continue
        if len(f) < 13:
            fail("fewer than 13 fields")
        qname, flag, rname, pos, cigar, seq = f[0], int(f[1]), f[2], int(f[3]), f[5], f[9]
        tags = dict((t[:5], t[5:]) for t in f[11:])
        m = CIGAR.match(cigar)
        if not m or rname not in order or "NM:i:" not in tags or "MD:Z:" not in tags or not MD.match(tags["MD:Z:"]):
            fail("malformed")
        left, right = (int(x) if x else 0 for x in (m.group(1), m.group(3)))
        ops = [(int(l), o) for l, o in re.findall(r"(\d+)([MID])", m.group(2))]
        if ops[0][1] != "M" or ops[-1][1] != "M" or any(l == 0 for l, _ in ops) or any(a[1] == b[1] for a, b in zip(ops, ops[1:])):
            fail("the operations do not begin and end with M, or are empty or not merged")
        if left + right + sum(l for l, o in ops if o != "D") != len(seq):
            fail("the clips, M and I do not sum to len(SEQ)")
        span = sum(l for l, o in ops if o != "I")
        ref = mm.mapped(contigs[rname])
        if pos < 1 or pos - 1 + span > len(ref):
            fail("beyond the contig")
        # MD as one item per contig letter: a match ("="), a mismatch (its letter) or a deleted letter ("^" + letter)
        items = []
        for run, dele, letter in re.findall(r"(\d+)(?:\^([ACGTN]+)|([ACGTN]))?", tags["MD:Z:"]):
            items += ["="] * int(run) + ["^" + c for c in dele] + ([letter] if letter else [])
        if len(items) != span:
            fail("MD does not cover the contig letters of CIGAR")
        at, on, rebuilt, mismatches = left, 0, [], 0
        for l, o in ops:
            for _ in range(l):
                if o == "I":
                    at += 1
                    continue
                item = items[on]
                on += 1
                if o == "D":
                    if item[0] != "^":
                        fail("a D column that MD does not show as deleted")
                    rebuilt.append(item[1])
                    continue
                if item[0] == "^":
                    fail("an M column that MD shows as deleted")
                if item == "=":
                    if seq[at] == "N":
                        fail("an N in a match run")
                    rebuilt.append(seq[at])
                else:
                    if item == seq[at] and item != "N":
                        fail("a mismatch column that matches")
                    rebuilt.append(item)
                    mismatches += 1
                at += 1
        if "".join(rebuilt) != ref[pos - 1:pos - 1 + span]:
            fail("SEQ, CIGAR and MD do not rebuild the contig")
        gaps = sum(l for l, o in ops if o != "M")
        if int(tags["NM:i:"]) != mismatches + gaps:
            fail("NM is not the mismatches plus the gap letters")
        if "XG:i:" in tags:
            rescued += 1
            if int(tags["XG:i:"]) != gaps:
                fail("XG is not the number of gap letters")
        elif gaps:
            fail("a gap on a line without XG")
        if (order[rname], pos) < last:
            fail("not sorted by (@SQ order, POS)")
        last = (order[rname], pos)
        primaries[qname] = primaries.get(qname, 0) + (0 if flag & 256 else 1)
    for qname, n in primaries.items():
        if n != 1:
            raise ValueError("%s has %d lines without 256" % (qname, n))
    return len(primaries), rescued
