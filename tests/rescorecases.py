"""Hand-built prefilter sets for rescorediagonal --rescore-mode 3 (rescorediagonal.cpp:145-356, DistanceCalculator.h:93-220): every
window, mask, gate and probe of csrc/rescore.hip met on purpose instead of by what kmermatcher happens to emit.  Deterministic
(RandomState), no GPU.

A case set is one sequence DB (keys = ids = 0..n-1) plus one prefilter DB of type DBTYPE_PREFILTER_REV_RES (a negative score = the
reverse strand), and its parameter rows.  Every hit is one named group with a (query, target) pair of its own, so a record of the
reference's text belongs to exactly one group.  Random sequences score 0 off their true diagonal: a hit that is meant to pass has
a target cut from its query (or from the query's reverse complement) at a known offset, and carries that offset as its
diagonal.  Mismatches are substitutions: a transition keeps the purine/pyrimidine class, a transversion (`TV`) flips it.

The E-value depends on the DB's residue total.  A set is therefore complete - every sequence has its final length - before
`finish` works out the loose threshold (half the smallest E-value a score of 0 has at any length present: score 0 still fails,
which keeps the reference defined) and the members that sit on the E-value boundary (their letters change, their lengths do not).

Sets: geometry (no N: the 2-bit word path; lengths mixed), geometry_L1 .. geometry_L129 (one length each, so that the loose
threshold is that length's own and the one-column overlaps on the largest diagonals pass it), gates, gates_sweep (every overlap length with every affordable mismatch count; a set
of its own so that its thousands of records are written for one row, not for thirty), letters (the per-base path and the raw
plane), wrap (diagonals beyond 16 bits on sequences cut from one seeded genome).

Groups dropped because the reference reads outside a sequence for them (undefined there), by name, in `DROPPED`.
"""
import functools
import hashlib
import os

import numpy as np

from carpedeam_amd import capi, mmdb
from rescore_model import Params, min_passing_score

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rescore_directed")
ALPHA = np.frombuffer(b"ACGT", np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
TS = bytes.maketrans(b"ACGT", b"GTAC")           # transition: same purine/pyrimidine class
TV = bytes.maketrans(b"ACGT", b"CATG")           # transversion: the class flips
LENGTHS = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 129]
WRAP_LENGTHS = [32767, 32768, 32769, 65535, 65536, 65537, 98304, 131073]
WRAP_DIAGONALS = [1, 32767, 32768, 65535, 65536, 65537, 98000, 131000]
IDENTITY_THRESHOLDS = [0.0, 0.5, 0.9, 0.97, 0.99, 1.0]
EPSILON_THRESHOLD = 0.9000001      # the float two steps above 0.9f: 9/10 passes it only through the gate's `- FLT_EPSILON`
EVALUE_ROWS = [("e1e-05", 1e-5), ("e0.001", 0.001), ("e10", 10.0)]
EVALUE_LENGTHS = [40, 75, 100, 150]

# what left the generator because the reference's behaviour is undefined for it: (set, group, reason)
DROPPED = [
    ("letters", "heavy_n_identity_rev", "an identity hit on the reverse strand that scores 0: the identity loop compares the byte in front of the reversed "
                                        "query's malloc block with the byte in front of the sequence"),
    ("letters", "star_only_identity_rev", "the same, for the sequence `*`"),
    ("any", "score_0_passes_e", "a hit that is no identity hit, scores 0 and passes -e: the -1 record of a non-identity hit (cdm_rescore refuses such a -e)"),
]


def rnd(rs, n):
    return bytes(bytearray(ALPHA[rs.randint(0, 4, size=n)]))


def revcomp(s):
    return s.translate(_COMP)[::-1]


def short(d):
    """the diagonal as the prefilter text's reader narrows it (QueryMatcher.h:88: fast_atoi<short>)"""
    return ((int(d) + 32768) & 0xFFFF) - 32768


def overlap(q_len, t_len, d):
    """(query offset, target offset, columns) of diagonal d, None without an overlap (DistanceCalculator.h:119-150)"""
    md = abs(d)
    if d >= 0 and md < q_len:
        return md, 0, min(t_len, q_len - md)
    if d < 0 and md < t_len:
        return 0, md, min(t_len - md, q_len)
    return None


def plant(rs, oriented, t_len, d, subs=()):
    """a random target of t_len letters that holds the oriented query's letters on diagonal d, with substitutions (column of the
    overlap - negative from its end -, table)"""
    t = bytearray(rnd(rs, t_len))
    ov = overlap(len(oriented), t_len, d)
    if ov:
        qo, to, m = ov
        t[to:to + m] = oriented[qo:qo + m]
        cols = [c if c >= 0 else m + c for c, _ in subs]
        assert len(set(cols)) == len(cols) and all(0 <= c < m for c in cols), (cols, m)
        for c, (_, table) in zip(cols, subs):
            t[to + c] = bytes([t[to + c]]).translate(table)[0]
    return bytes(t)


class RSet:
    def __init__(self, name, seed):
        self.name, self.rs = name, np.random.RandomState(seed)
        self.seqs, self.hits, self.groups, self.rows, self.expect, self.pending = [], [], {}, [], [], []
        self._pairs, self._cache, self._by_pair = set(), {}, {}
        self.loose = None

    # ---- building
    def seq(self, s, cache_key=None):
        if cache_key is not None and cache_key in self._cache:
            return self._cache[cache_key]
        self.seqs.append(bytes(s))
        if cache_key is not None:
            self._cache[cache_key] = len(self.seqs) - 1
        return len(self.seqs) - 1

    def hit(self, group, q, t, rev, diag, **meta):
        assert group not in self.groups, group
        assert (q, t) not in self._pairs, group
        self._pairs.add((q, t))
        self.groups[group] = dict(query=q, target=t, reverse=bool(rev), diagonal=int(diag), **meta)
        self.hits.append((q, t, -100 if rev else 100, int(diag), group))

    def planted(self, group, q_len, t_len, d, rev, subs=(), q=None, text=None, **meta):
        """a query (new unless given) and a new target that holds it on diagonal d"""
        if q is None:
            q = self.seq(rnd(self.rs, q_len))
        oriented = revcomp(self.seqs[q]) if rev else self.seqs[q]
        t = self.seq(plant(self.rs, oriented, t_len, d, subs))
        self.hit(group, q, t, rev, d if text is None else text, **meta)
        return q, t

    def row(self, name, **par):
        self.rows.append((name, par))

    def expecting(self, row, present, absent):
        self.expect.append((row, list(present), list(absent)))

    # ---- finishing
    def finish(self):
        ev = capi.lib().cdm_evalue
        self.residues = sum(len(s) for s in self.seqs)
        lens = sorted({len(s) for s in self.seqs})
        self.loose = min(ev(0.0, float(L), self.residues) for L in lens) / 2.0
        for group, e, q, t, which, rev in self.pending:       # the E-value boundary: target t gets its letters now
            L = len(self.seqs[q])
            s = min_passing_score(L, self.residues, e) - (0 if which == "min" else 1)
            assert s >= 0, group
            b = next(b for b in range(6) if (s + 5 * b) % 2 == 0 and (s + 5 * b) // 2 >= max(1, b))
            m = (s + 5 * b) // 2
            assert 1 <= m <= L, (group, s, m)
            oriented = revcomp(self.seqs[q]) if rev else self.seqs[q]
            self.seqs[t] = plant(self.rs, oriented, L, L - m, [(2 * i, TV) for i in range(b)])
            self.hit(group, q, t, rev, L - m, score=s)
        self.pending = []
        self.hits.sort(key=lambda h: h[0])
        self.rows = [(n, Params(**{k: (self.loose if v == "loose" else v) for k, v in p.items()})) for n, p in self.rows]
        # keep the reference defined: score 0 fails every -e of the set, at every length present
        for n, p in self.rows:
            assert all(ev(0.0, float(L), self.residues) > p.e for L in lens), (self.name, n)
        names = set(self.groups)
        for row, present, absent in self.expect:
            assert set(present) <= names and set(absent) <= names and row in dict(self.rows), row
        return self

    def hit_list(self):
        """(query, target, score, diagonal as the text's reader narrows it) in query order"""
        return [(q, t, sc, short(d)) for q, t, sc, d, _ in self.hits]

    def csr(self):
        off = np.zeros(len(self.seqs) + 1, np.uint64)
        off[1:] = np.cumsum(np.bincount([h[0] for h in self.hits], minlength=len(self.seqs)))
        return off, np.array([h[1:] for h in self.hit_list()], capi.HIT_DTYPE)

    def seq_keyed(self):
        return {k: (s + b"\n", 0) for k, s in enumerate(self.seqs)}

    def pref_keyed(self):
        """every sequence has an entry, the ones without hits an empty one; the diagonal stands as the group wrote it"""
        lines = {k: [] for k in range(len(self.seqs))}
        for q, t, sc, d, _ in self.hits:
            lines[q].append("%d\t%d\t%d\n" % (t, sc, d))
        return {k: ("".join(v).encode(), 0) for k, v in lines.items()}

    def write(self, seq_path, pref_path):
        mmdb.write_from_keyed(seq_path, self.seq_keyed(), mmdb.DBTYPE_NUCLEOTIDES)
        mmdb.write_from_keyed(pref_path, self.pref_keyed(), mmdb.DBTYPE_PREFILTER_REV_RES)

    def by_pair(self):
        if len(self._by_pair) != len(self.groups):
            self._by_pair = {(g["query"], g["target"]): n for n, g in self.groups.items()}
        return self._by_pair

    def digest(self):
        h = hashlib.sha256()
        h.update(self.name.encode())
        for s in self.seqs:
            h.update(s + b"\n")
        for q, t, sc, d, g in self.hits:
            h.update(("%d %d %d %d %s\n" % (q, t, sc, d, g)).encode())
        for n, p in self.rows:
            h.update((n + " " + " ".join(p.flags()) + "\n").encode())
        return h.hexdigest()


def strands():
    return (("fwd", False), ("rev", True))


# ---------------------------------------------------------------------------------------------------------------- geometry
GEOMETRY_SUBS = [("first_ts", [(0, TS)]), ("first_tv", [(0, TV)]), ("last_ts", [(-1, TS)]), ("last_tv", [(-1, TV)]),
                 ("c15ts_c16tv", [(15, TS), (16, TV)]), ("c15tv_c16ts", [(15, TV), (16, TS)]),
                 ("three_ts", [(0, TS), (15, TS), (-1, TS)]), ("three_tv", [(0, TV), (16, TV), (-1, TV)])]


def geometry_classes(q_len, t_len):
    return [("d0", 0), ("d+1", 1), ("d-1", -1), ("d+15", 15), ("d-15", -15), ("d+16", 16), ("d-16", -16), ("d+17", 17), ("d-17", -17),
            ("dmax+", q_len - 1), ("dmax-", -(t_len - 1)), ("beyond+", q_len), ("beyond-", -t_len)]


def geometry_set():
    S = RSet("geometry", 101)
    for i, q_len in enumerate(LENGTHS):
        q = S.seq(rnd(S.rs, q_len))
        for t_len in sorted({q_len, LENGTHS[(i + 4) % 15], LENGTHS[(i + 9) % 15], 129, 1}):
            for cls, d in geometry_classes(q_len, t_len):
                ov = overlap(q_len, t_len, d)
                beyond = cls.startswith("beyond")
                if (ov is None) != beyond:
                    continue
                for sn, rev in strands():
                    base = "q%d_t%d_%s_%s" % (q_len, t_len, cls, sn)
                    meta = dict(cls=cls, qlen=q_len, tlen=t_len, strand=sn, columns=ov[2] if ov else 0)
                    S.planted(base, q_len, t_len, d, rev, q=q, **meta)
                    if beyond:
                        continue
                    if t_len in (q_len, 129) and cls in ("d0", "d+1", "d-1", "d+16", "d-17"):
                        for vn, subs in GEOMETRY_SUBS:
                            cols = [c if c >= 0 else ov[2] + c for c, _ in subs]
                            if len(set(cols)) == len(cols) and all(0 <= c < ov[2] for c in cols):
                                S.planted(base + "_" + vn, q_len, t_len, d, rev, subs, q=q, variant=vn, **meta)
                    if t_len == q_len and cls in ("d+1", "d-1", "d+16", "d-16"):
                        # the same true diagonal as a value 65536 above and 65536 below: one of the two is the 16-bit truncation
                        for vn, text in (("enc_plus", d + 65536), ("enc_minus", d - 65536)):
                            S.planted(base + "_" + vn, q_len, t_len, d, rev, q=q, text=text, same_as=base, **meta)
    S.row("e0.001", e=0.001)
    S.row("loose", e="loose", min_seq_id=0.0)
    return S.finish()


FEW_COLUMNS = (2, 3, 4, 8)


def length_classes(L):
    """the classes of `geometry` for a query and a target of L letters each, and overlaps of a few columns at either end"""
    return geometry_classes(L, L) + [("cols%d%s" % (c, sg), s * (L - c)) for c in FEW_COLUMNS if L > c for sg, s in (("+", 1), ("-", -1))]


def geometry_length_set(L):
    """One length for query and target.  The loose -e of the mixed set above is set by its 1-letter sequences, where an overlap of one
    or two columns passes for a query of one letter only; here it is half the E-value of score 0 at L itself, which the score 2 of a
    single column passes (E falls by 0.28 with it): the largest diagonals, one column in the last word, are compared at every length."""
    S = RSet("geometry_L%d" % L, 1000 + L)
    q = S.seq(rnd(S.rs, L))
    for cls, d in length_classes(L):
        ov = overlap(L, L, d)
        if (ov is None) != cls.startswith("beyond"):
            continue
        for sn, rev in strands():
            S.planted("L%d_%s_%s" % (L, cls, sn), L, L, d, rev, q=q, cls=cls, qlen=L, tlen=L, strand=sn, columns=ov[2] if ov else 0)
    S.row("e0.001", e=0.001)
    S.row("loose", e="loose", min_seq_id=0.0)
    return S.finish()


# ---------------------------------------------------------------------------------------------------------------- gates
def _id_members(S):
    for L, k in ((30, 3), (30, 4), (10, 1), (10, 2), (1000, 100), (1000, 101), (100, 3), (100, 4), (100, 1), (100, 2), (1000, 10), (1000, 11), (100, 0), (1000, 1)):
        for sn, rev in strands():
            cols = S.rs.choice(L, k, replace=False)
            S.planted("id_%dof%d_%s" % (L - k, L, sn), L, L, 0, rev, [(int(c), TV if i % 2 else TS) for i, c in enumerate(cols)])


def _cov_expect(mode, c):
    """(present, absent) member stems of the canBeCovered / hasCoverage pairs at -c c, from the length ratios alone"""
    if c == 1.0:
        return {0: (["100_100"], ["99_100", "100_99"]), 1: (["100_100", "100_99"], ["99_100"]), 2: (["100_100", "99_100"], ["100_99"]),
                3: (["100_100"], ["100_99", "99_100"]), 4: (["100_100"], ["99_100", "100_99"]), 5: (["100_100"], ["99_100", "100_99"])}[mode]
    s = int(round(100 * c))
    a, b, a1, b1 = "%d_100" % s, "100_%d" % s, "%d_100" % (s - 1), "100_%d" % (s - 1)
    return {0: ([a, b, "100_100"], [a1, b1]), 1: ([a, b], [a1]), 2: ([b, a], [b1]),
            3: ([b, "100_100"], [b1, a]),          # a = (s, 100): tLen / qLen > 1, refused by mode 3's `<= 1.0` alone
            4: ([a, "100_100"], [a1, b]),          # b = (100, s): qLen / tLen > 1, refused by mode 4's `<= 1.0` alone
            5: ([a, b], [a1, b1])}[mode]


def gates_set():
    S = RSet("gates", 202)
    both = lambda stems: [s + "_" + sn for s in stems for sn, _ in strands()]
    # ---- identity
    _id_members(S)
    for thr in IDENTITY_THRESHOLDS + [EPSILON_THRESHOLD]:
        S.row("sid%s" % thr, e="loose", min_seq_id=thr)
    S.expecting("sid0.5", both(["id_27of30", "id_26of30", "id_8of10"]), [])
    S.expecting("sid0.9", both(["id_27of30", "id_9of10", "id_900of1000"]), both(["id_26of30", "id_8of10", "id_899of1000"]))
    S.expecting("sid0.97", both(["id_97of100"]), both(["id_96of100"]))
    S.expecting("sid0.99", both(["id_99of100", "id_990of1000"]), both(["id_98of100", "id_989of1000"]))
    S.expecting("sid1.0", both(["id_100of100"]), both(["id_999of1000", "id_99of100"]))
    S.expecting("sid%s" % EPSILON_THRESHOLD, both(["id_9of10", "id_27of30"]), both(["id_26of30"]))
    # ---- E-value: the smallest passing score of the query's length and that score less 1; the targets get their letters in finish()
    for rn, e in EVALUE_ROWS:
        S.row(rn, e=e, min_seq_id=0.0)
        for L in EVALUE_LENGTHS:
            for sn, rev in strands():
                q, names = S.seq(rnd(S.rs, L)), []
                for which in ("min", "below"):
                    names.append("ev_%s_L%d_%s_%s" % (rn, L, which, sn))
                    S.pending.append((names[-1], e, q, S.seq(rnd(S.rs, L)), which, rev))
                S.expect.append((rn, names[:1], names[1:]))
    # ---- --min-aln-len 30: 30 | 29 columns, with a '*' on one end (alnLen = m - 1) and on both (alnLen = m - 2)
    S.row("alnlen30", e="loose", min_seq_id=0.0, min_aln_len=30)
    for stem, m, stars in (("al_plain_30", 30, ()), ("al_plain_29", 29, ()), ("al_star1_31", 31, (-1,)), ("al_star1_30", 30, (-1,)),
                           ("al_starfirst_31", 31, (0,)), ("al_starfirst_30", 30, (0,)), ("al_star2_32", 32, (0, -1)), ("al_star2_31", 31, (0, -1))):
        for sn, rev in strands():
            oriented = rnd(S.rs, m)
            t = bytearray(oriented)
            for p in stars:
                t[p] = ord("*")
            S.hit(stem + "_" + sn, S.seq(revcomp(oriented) if rev else oriented), S.seq(t), rev, 0)
    # (forward only: the reversed query spells its '*' as X, which is not trimmed)
    for stem, m in (("al_qstar_31", 31), ("al_qstar_30", 30)):
        oriented = rnd(S.rs, m)
        S.hit(stem + "_fwd", S.seq(oriented[:-1] + b"*"), S.seq(oriented), False, 0)
    S.expecting("alnlen30", both(["al_plain_30", "al_star1_31", "al_starfirst_31", "al_star2_32"]) + ["al_qstar_31_fwd"],
                both(["al_plain_29", "al_star1_30", "al_starfirst_30", "al_star2_31"]) + ["al_qstar_30_fwd"])
    # ---- canBeCovered / hasCoverage on the length ratio: the shorter sequence lies in the longer on diagonal 0
    for ql, tl in ((100, 100), (80, 100), (79, 100), (100, 80), (100, 79), (50, 100), (49, 100), (100, 50), (100, 49), (99, 100), (100, 99)):
        for sn, rev in strands():
            S.planted("cc_%d_%d_%s" % (ql, tl, sn), ql, tl, 0, rev)
    # ---- hasCoverage on the overlap: exactly the share asked, and one column less
    for d in (0, 1, -1, 20, 21, -20, -21, 50, 51, -50, -51):
        for sn, rev in strands():
            S.planted("hc_eq_d%+d_%s" % (d, sn), 100, 100, d, rev)
    for d in (-100, -101):
        for sn, rev in strands():
            S.planted("hc_t200_d%+d_%s" % (d, sn), 100, 200, d, rev)
    for d in (100, 101):
        for sn, rev in strands():
            S.planted("hc_q200_d%+d_%s" % (d, sn), 200, 100, d, rev)
    # 200 | 250: four fifths of the longer sequence, the whole of the shorter - the query's share and the target's apart at -c 0.8
    for d in (-50, -51):
        for sn, rev in strands():
            S.planted("hc_t250_d%+d_%s" % (d, sn), 200, 250, d, rev)
    for d in (50, 51):
        for sn, rev in strands():
            S.planted("hc_q250_d%+d_%s" % (d, sn), 250, 200, d, rev)
    for mode in range(6):
        for c in (0.5, 0.8, 1.0):
            rn = "cov%d_c%s" % (mode, c)
            S.row(rn, e="loose", min_seq_id=0.0, c=c, cov_mode=mode)
            present, absent = _cov_expect(mode, c)
            present, absent = ["cc_" + s for s in present], ["cc_" + s for s in absent]
            if mode in (0, 1, 2):
                edge = {0.5: 50, 0.8: 20, 1.0: 0}[c]
                present += ["hc_eq_d%+d" % edge] + (["hc_eq_d%+d" % -edge] if edge else [])
                absent += ["hc_eq_d%+d" % (edge + 1), "hc_eq_d%+d" % -(edge + 1)]
                if c == 0.5 and mode in (0, 1):
                    present, absent = present + ["hc_t200_d-100"], absent + ["hc_t200_d-101"]
                if c == 0.5 and mode in (0, 2):
                    present, absent = present + ["hc_q200_d+100"], absent + ["hc_q200_d+101"]
                if c == 0.8 and mode in (0, 1):          # target share 200 / 250 | 199 / 250, query share 1
                    present, absent = present + ["hc_t250_d-50"], absent + ["hc_t250_d-51"]
                if c == 0.8 and mode in (0, 2):          # query share 200 / 250 | 199 / 250, target share 1
                    present, absent = present + ["hc_q250_d+50"], absent + ["hc_q250_d+51"]
                if c == 1.0 and mode == 1:               # the whole target | one column less, half of the query either way
                    present, absent = present + ["hc_q200_d+100"], absent + ["hc_q200_d+101"]
                if c == 1.0 and mode == 2:
                    present, absent = present + ["hc_t200_d-100"], absent + ["hc_t200_d-101"]
            S.expecting(rn, both(present), both(absent))
    # ---- identity hits: written whatever their gates say
    S.row("sid0.97_e1e-05", e=1e-5, min_seq_id=0.97)
    S.expecting("sid0.97_e1e-05", both(["id_97of100", "id_990of1000"]), both(["id_96of100", "id_9of10"]))
    S.row("strict", e=1e-5, min_seq_id=0.97, c=0.8, cov_mode=0, min_aln_len=30)
    s = bytearray(b"ACG" * 4)
    s[11] = ord("T")                       # diagonal 3: nine columns, eight identities, score 13
    k = S.seq(s)
    S.hit("identity_fails_all", k, k, False, 3)
    k = S.seq(rnd(S.rs, 50))
    S.hit("identity_plain", k, k, False, 0)
    x = rnd(S.rs, 30)
    k = S.seq(x + revcomp(x))
    S.hit("identity_rev_palindrome", k, k, True, 0)
    for rn, _ in list(S.rows):
        S.expecting(rn, ["identity_fails_all", "identity_plain", "identity_rev_palindrome"], [])
    S.expecting("strict", ["cc_100_100_fwd"], ["id_27of30_fwd", "al_plain_29_fwd"])
    # ---- the text's diagonal: -5 as -5, as 65531; 5 as 65541 and as -65531 (the module reads them as the reference does)
    for stem, d, text in (("enc_m5", -5, -5), ("enc_m5_trunc", -5, 65531), ("enc_p5", 5, 5), ("enc_p5_plus", 5, 65541), ("enc_p5_minus", 5, -65531)):
        for sn, rev in strands():
            S.planted(stem + "_" + sn, 60, 60, d, rev, text=text)
    S.expecting("sid0.9", both(["enc_m5", "enc_m5_trunc", "enc_p5", "enc_p5_plus", "enc_p5_minus"]), [])
    return S.finish()


def sweep_set():
    """every overlap length 1..150 with every mismatch count that still scores above 0 (2 (L - k) > 3 k): pins ident and the stored
    seq_id of every quotient"""
    S = RSet("gates_sweep", 303)
    for L in range(1, 151):
        q = S.seq(rnd(S.rs, L))
        for sn, rev in strands():
            if rev and L % 7:
                continue
            k = 0
            while 2 * (L - k) - 3 * k > 0:
                cols = S.rs.choice(L, k, replace=False)
                S.planted("sweep_L%d_k%d_%s" % (L, k, sn), L, L, 0, rev, [(int(c), TV if i % 2 else TS) for i, c in enumerate(cols)], q=q, columns=L, mismatches=k)
                k += 1
    S.row("sid0.0", e="loose", min_seq_id=0.0)
    return S.finish()


# ---------------------------------------------------------------------------------------------------------------- letters
def _letters_member(S, name, L, q_cols, t_cols, rev, d=0, t_len=None):
    """an oriented plain query O and a target cut from it on diagonal d; then letters set at columns of the oriented query (stored at
    L - 1 - column on the reverse strand) and at positions of the target.  "lower" lower-cases the letter that is there."""
    O = rnd(S.rs, L)
    t = bytearray(plant(S.rs, O, L if t_len is None else t_len, d))
    q = bytearray(revcomp(O) if rev else O)

    def put(buf, pos, letter):
        buf[pos] = ord(chr(buf[pos]).lower()) if letter == "lower" else ord(letter)
    for c, letter in q_cols.items():
        put(q, (L - 1 - c) if rev else c, letter)
    for p, letter in t_cols.items():
        put(t, p, letter)
    S.hit(name, S.seq(q), S.seq(t), rev, d)


def letters_set():
    S = RSet("letters", 404)
    run = lambda a, b, ch: {c: ch for c in range(a, b)}
    cases = [("n_q", {10: "N"}, {}), ("n_t", {}, {10: "N"}), ("n_both", {10: "N"}, {10: "N"}),
             ("nrun_q", run(20, 25, "N"), {}), ("nrun_t", {}, run(20, 25, "N")), ("nrun_both", run(20, 25, "N"), run(20, 25, "N")),
             ("nrun_shifted", run(20, 25, "N"), run(23, 28, "N")),
             # score as a match, different letters - and the other way round
             ("iupac_R_over_G", {10: "R"}, {10: "G"}), ("iupac_R_over_R", {10: "R"}, {10: "R"}), ("iupac_R_over_C", {10: "R"}, {10: "C"}),
             ("iupac_R_over_Y", {10: "R"}, {10: "Y"}), ("iupac_W_over_U", {10: "W"}, {10: "U"}), ("iupac_Y_over_T", {10: "Y"}, {10: "T"}),
             ("iupac_S_over_S", {10: "S"}, {10: "S"}), ("iupac_M_over_K", {10: "M"}, {10: "K"}), ("iupac_lower_r_over_G", {10: "r"}, {10: "G"}),
             ("x_over_x", {10: "X"}, {10: "X"}), ("n_over_x", {10: "N"}, {10: "X"}), ("iupac_every_letter", dict(zip(range(5, 18), "UWKBDVRSMYHXN")), {}),
             ("iupac_every_letter_t", {}, dict(zip(range(5, 18), "UWKBDVRSMYHXN"))),
             # lower case on either side
             ("lower_q", {5: "lower"}, {}), ("lower_t", {}, {5: "lower"}), ("lower_both", {5: "lower"}, {5: "lower"}),
             ("lower_all_q", run(0, 60, "lower"), {}), ("lower_all_t", {}, run(0, 60, "lower")),
             # '*': first, last, inside
             ("star_first_q", {0: "*"}, {}), ("star_last_q", {59: "*"}, {}), ("star_inside_q", {30: "*"}, {}), ("star_first_t", {}, {0: "*"}),
             ("star_last_t", {}, {59: "*"}), ("star_inside_t", {}, {30: "*"}), ("star_ends_t", {}, {0: "*", 59: "*"}), ("star_first_q_last_t", {0: "*"}, {59: "*"}),
             ("star_over_star_inside", {30: "*"}, {30: "*"}), ("star_over_star_first", {0: "*"}, {0: "*"}), ("star_second_q", {1: "*"}, {})]
    for name, q_cols, t_cols in cases:
        for sn, rev in strands():
            _letters_member(S, "%s_%s" % (name, sn), 60, q_cols, t_cols, rev)
    for sn, rev in strands():
        # off the main diagonal: the '*' that ends the overlap is not the one that ends the sequence
        _letters_member(S, "n_both_d5_" + sn, 60, {10: "N"}, {5: "N"}, rev, d=5)
        _letters_member(S, "star_overlap_end_d-7_" + sn, 60, {}, {7: "*", 59: "*"}, rev, d=-7)
        _letters_member(S, "star_off_overlap_d5_" + sn, 60, {0: "*", 4: "*"}, {}, rev, d=5)
        # an N far from an overlap that is itself N-free: the per-base path against the word path of the twin
        for stem, q_cols, t_cols in (("far_n_q", {90: "N"}, {}), ("far_plain_q", {}, {})):
            _letters_member(S, "%s_%s" % (stem, sn), 100, q_cols, t_cols, rev, t_len=50)
            _letters_member(S, "%s_d7_%s" % (stem, sn), 100, q_cols, t_cols, rev, d=7, t_len=50)
        for stem, t_cols in (("far_n_t", {90: "N"}), ("far_plain_t", {})):
            _letters_member(S, "%s_%s" % (stem, sn), 50, {}, t_cols, rev, t_len=100)
            _letters_member(S, "%s_d-7_%s" % (stem, sn), 50, {}, t_cols, rev, d=-7, t_len=100)
    # '*' as the only letter; more than 40 % N: the identity hit becomes the -1 record (forward strand: DROPPED has the reverse one)
    k = S.seq(b"*")
    S.hit("star_only_identity", k, k, False, 0)
    S.hit("star_only_pair", S.seq(b"*"), S.seq(b"*"), False, 0)
    s = bytearray(rnd(S.rs, 50))
    for p in S.rs.choice(50, 25, replace=False):
        s[p] = ord("N")
    k = S.seq(s)
    S.hit("heavy_n_identity", k, k, False, 0)
    s = bytearray(rnd(S.rs, 50))
    s[7] = ord("N")
    k = S.seq(s)
    S.hit("light_n_identity", k, k, False, 0)
    S.row("loose", e="loose", min_seq_id=0.0)
    S.row("default", e=0.001)
    S.expecting("loose", ["star_only_identity", "heavy_n_identity", "light_n_identity"], ["star_only_pair"])
    return S.finish()


UNDEFINED_RECORDS = {"letters": 2}       # star_only_identity and heavy_n_identity; no other set has a -1 record


# ---------------------------------------------------------------------------------------------------------------- wrap
def wrap_set():
    S = RSet("wrap", 505)
    G = rnd(S.rs, 400000)

    def cut(start, n, rev):
        s = G[start:start + n]
        assert len(s) == n
        return S.seq(revcomp(s) if rev else s, cache_key=(start, n, rev))
    W = WRAP_LENGTHS
    for i, ad in enumerate(WRAP_DIAGONALS):
        need = next(L for L in W if L >= ad + 50) if ad > 1 else W[i]
        for sign in (1, -1):
            other = W[(2 * i + (sign < 0) + 1) % len(W)]
            d = sign * ad
            for sn, rev in strands():
                if d > 0:
                    q_len, t_len, q, t = need, other, cut(1000, need, rev), None
                    target = bytearray(G[1000 + d:1000 + d + t_len])
                else:
                    q_len, t_len = other, need
                    q = cut(2000 + ad, q_len, rev)
                    target = bytearray(G[2000:2000 + t_len])
                qo, to, m = overlap(q_len, t_len, d)
                for c, table in ((0, TV), (m - 1, TS)):
                    target[to + c] = bytes([target[to + c]]).translate(table)[0]
                S.hit("wrap_d%+d_%s" % (d, sn), q, S.seq(target), rev, short(d), true_diagonal=d, columns=m, qlen=q_len, tlen=t_len)
    # a query that holds the target twice, 65536 letters apart: probes 100 and 65636; strict '>' keeps the first of two equal ones
    T = rnd(S.rs, 1000)
    for name, subs_first, subs_second, want in (("repeat_equal_picks_first", 0, 0, 100), ("repeat_second_better", 2, 0, 65636), ("repeat_first_better", 0, 2, 100)):
        for sn, rev in strands():
            Q = bytearray(rnd(S.rs, 131073))
            for at, k in ((100, subs_first), (65636, subs_second)):
                Q[at:at + 1000] = T
                for c in range(k):
                    Q[at + 10 * c] = bytes([Q[at + 10 * c]]).translate(TV)[0]
            S.hit("%s_%s" % (name, sn), S.seq(revcomp(bytes(Q)) if rev else bytes(Q)), S.seq(T), rev, 100, true_diagonal=want)
    # a target that holds the query on -65436 (1000 columns) and its tail on +100 (900 columns): the negative probes come first
    for name, k, want in (("repeat_negpos_equal_picks_negative", 40, -65436), ("repeat_negpos_positive_better", 41, 100), ("repeat_negpos_negative_better", 0, -65436)):
        for sn, rev in strands():
            O = rnd(S.rs, 1000)
            t = bytearray(rnd(S.rs, 70000))
            t[65436:66436] = O
            for c in range(k):
                t[65436 + 20 * c] = bytes([t[65436 + 20 * c]]).translate(TS)[0]
            t[0:900] = O[100:]
            S.hit("%s_%s" % (name, sn), S.seq(revcomp(O) if rev else O), S.seq(t), rev, 100, true_diagonal=want)
    # 164 000 columns with 65 536 transversions: the score stays above the gate, the purine/pyrimidine count saturates
    for name, k in (("ry_saturates_65536", 65536), ("ry_counts_60000", 60000)):
        A = G[200000:364000]
        B = bytearray(A)
        for p in range(0, 2 * k, 2):
            B[p] = bytes([B[p]]).translate(TV)[0]
        S.hit(name, cut(200000, 164000, False), S.seq(B), False, 0, true_diagonal=0, transversions=k)
    S.row("default", e=0.001)
    S.row("sid0", e=0.001, min_seq_id=0.0)
    return S.finish()


SETS = [("geometry", geometry_set), ("gates", gates_set), ("gates_sweep", sweep_set), ("letters", letters_set), ("wrap", wrap_set)]
SETS += [("geometry_L%d" % L, functools.partial(geometry_length_set, L)) for L in LENGTHS]


# ---------------------------------------------------------------------------------------------------------------- fixtures
def fixture(name, row):
    return mmdb.load_keyed(os.path.join(DIR, name, row + ".keyed.gz"))


def fixture_digest(name):
    with open(os.path.join(DIR, name, "digest.txt")) as f:
        return f.read().split()


def records(keyed):
    """alignment DB text -> {(query key, target key): the record's columns}"""
    out = {}
    for q, (payload, _) in keyed.items():
        for line in payload.decode().split("\n"):
            if line:
                f = line.split("\t")
                out[(q, int(f[0]))] = f
    return out


def record_diagonal(f):
    """the diagonal a record lies on: forward q_start - db_start; reverse (q_start > q_end) the oriented start q_len - 1 - q_start"""
    qs, qe, ql, ds = int(f[4]), int(f[5]), int(f[6]), int(f[7])
    return (qs - ds) if qs <= qe else (ql - 1 - qs) - ds
