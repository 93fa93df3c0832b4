"""Hand-built alignment sets for ancient_contig_merge (src/assembler/ancientContigsResults.cpp, nuclassembleUtil.cpp): the column counts
of csrc/contig.hip, the two gates, the heap, the rounds, the letters of a grown query and the wave-level lists of csrc/contigqueue.hip met
on purpose instead of by what random reads grown into contigs happen to reach.  Deterministic (RandomState), no GPU.  Shape and
helpers as tests/extendcases.py: a set is one sequence DB plus one alignment DB as text records, built from groups (one query with its
targets); a group carries its name, its query and - where it follows from the geometry - what the reference is meant to do with it:
"right" / "left" / "both" / "none", None = whatever comes out, and the length of the output.

Geometry.  A right candidate of n columns with an overhang of o letters is a target  query[qLen-n:] + tail(o): record
(qs, qe, ds, de) = (qLen-n, qLen-1, 0, n-1).  A left candidate is  head(o) + query[:n]: (0, n-1, o, o+n-1).  A reverse candidate is
stored reverse-complemented: the record holds qs > qe and the coordinates of the target as stored.

Arithmetic used for the expectations (AC_FLAGS: --min-merge-seq-id 0.99, --min-ryseq-id-corr-reads 0.99).
  * First gate: identical letters / alnLength >= 0.99f and the same for the RY classes, both over the record's columns; an N over a
    letter differs, an N over an N is equal.  kmax(n) is the largest number of mismatches n columns take.
  * Second gate: the same two ratios over the columns in which neither side holds an N, and alnLength >= min(500, unsigned(0.2 dbLen))
    for records shorter than 500 columns.  Records that are neither right- nor left-starting keep their first ratios and a zero key.
  * Queue: the comparator's sum for two clean overlaps of m1 and m2 columns is (m1 + 1) / (m1 + m2 + 2): below 0.45 the first is the
    worse one whatever else holds, so a clean overlap 1.3 times as long as another is popped first ("leader": 160 before 100, 250
    before 160, 1300 before 1015).  Between 0.45 and 0.55 the longer alnLengthCons wins, so overlaps within a tenth of one another
    are popped longest first (the ladder), and equal ones in whatever order libstdc++'s heap leaves them (the tie families).
  * A round takes the first right and the first left candidate it pops; a later one whose overhang is at most what was added is
    dropped, one that reaches further is parked, re-aligned on the grown query (identical letters over all columns but the last,
    divided by their number; RY classes over all columns) and queued again with its old key.

The domain: records ungapped and in range, every sequence has its self record, a left- or right-starting target never overhangs its
query by more than the query's length (the reference pads the target with qLen - overhang letters 'N': a negative count is
undefined - the `refusal` pair, which has no golden, holds the one case beyond).

Not built, with the reason:
  * a re-aligned overlap of one column: a right hit is parked only behind a right growth (rightOff >= 1), and its new overlap is
    qLen - qs + rightOff >= 2 columns; on the left it is alnLength + leftOff >= 2.  `realign_2col` has the two-column overlap, whose
    identity is taken over one column.
  * a record that fails the RY gate alone in the first gate: two letters of different RY classes are different letters.
  * a reverse record of one column: qs == qe cannot say that it is reversed.
  * a target with letters beyond ACGTN that the device meets in a later round only: cqRound looks at a target's flag when it pops
    the hit, before it parks it, and every record is popped in the round that first queues it (docs/NOTEBOOK.md); the `handback` set
    holds such a target all the same, used by the reference in its second round.
  * heap families of ties that see the even-length branch of libstdc++'s __adjust_heap: with equal keys the comparator answers
    `worse` to everything and the branch's move is undone by the sift that follows it; the `break_keys` families (keys that differ,
    every pop visible through the --max-seq-len break) are what holds that branch.
  * a case for the comparator's 1e-12 hand-back band: CDM_CONTIG_HAND_BACK_EVERY covers that path.

Groups dropped because the reference's binary ended on a signal for them: none.
"""
import os
import subprocess

import numpy as np

from correctcases import revcomp, rnd
from extendcases import ExtSet, _RYFLIP, _TRANSITION, put, sides  # noqa: F401

MAXLEN_BOUND = 400
BREAK_ORDER_SIZES = (4, 5, 6, 7, 8, 9)
F32 = np.float32


def kmax(n):
    """the most mismatches n columns may hold: float(n - k) / n >= 0.99f"""
    k = 0
    while k + 1 <= n and F32(n - k - 1) / F32(n) >= F32(0.99):
        k += 1
    return k


def ts(*cols):
    """a transition under the query's letter: another letter of the same RY class"""
    def f(mid):
        for p in cols:
            mid[p] = bytes([mid[p]]).translate(_TRANSITION)[0]
    return f


def tv(*cols):
    """a transversion: the RY class differs too"""
    def f(mid):
        for p in cols:
            mid[p] = bytes([mid[p]]).translate(_RYFLIP)[0]
    return f


def both(*fs):
    def f(mid):
        for g in fs:
            if g:
                g(mid)
    return f


def spread(n, k, avoid=()):
    """k interior columns of n, evenly spread, none of `avoid`, none at either end"""
    out, used = [], set(avoid) | {0, n - 1}
    for i in range(k):
        c = (i + 1) * n // (k + 1)
        while c in used:
            c += 1
        assert 0 < c < n - 1
        used.add(c)
        out.append(c)
    return out


def no_n(mid):
    """the target holds a letter where the query holds an N"""
    for j in range(len(mid)):
        if mid[j] == ord("N"):
            mid[j] = ord("A")


def mk(S, rs, q, side, n, over, ext=None, edit=None, sedit=None, rev=False):
    """the target of a candidate and the arguments of its record.  `edit` works on the overlap's letters, `sedit` on the whole target,
    both as aligned (before a reverse target is stored reverse-complemented); `ext` are the overhang's letters"""
    query = S.seqs[q]
    L = len(query)
    assert 0 < n <= L and over <= L, "a target never overhangs its query by more than the query's length"
    mid = bytearray(query[L - n:] if side == "right" else query[:n])
    if edit:
        edit(mid)
    ext = rnd(rs, over) if ext is None else ext
    assert len(ext) == over
    t = bytearray(bytes(mid) + ext if side == "right" else ext + bytes(mid))
    if sedit:
        sedit(t)
    k = S.seq(revcomp(bytes(t)) if rev else bytes(t))
    qs, qe, ds, de = (L - n, L - 1, 0, n - 1) if side == "right" else (0, n - 1, over, over + n - 1)
    if rev:
        qs, qe, ds, de = qe, qs, len(t) - 1 - de, len(t) - 1 - ds
    return k, (q, k, qs, qe, ds, de)


def cand(S, rs, q, side, n, over, **kw):
    k, args = mk(S, rs, q, side, n, over, **kw)
    S.rec(*args)
    return k


# ------------------------------------------------------------------------------------------------------------------ stats
STATS_N = (1, 15, 16, 17, 1023, 1024, 1025, 1040)
STATS_PATHS = ("fast", "qn", "tn", "rev")
# query lengths of the right candidates: the overlap ends on the query's last letter (lengths = 0, 1, 15 and 7 mod 16; qs takes
# whatever residue qLen - n has); overhangs of the left candidates: the overlap ends on the target's last letter, ds = the overhang
_STATS_QLEN = (48, 49, 63, 55)
_STATS_OVER = {1: 8, 15: 13, 16: 32, 17: 23}


def stats_groups(S, rs):
    """every overlap length twice on every path and side: `in` holds kmax(n) mismatches, `out` one more - in the LAST column, the one a
    tail mask or an end coordinate one off loses (n = 17 and 1025: a third member with the extra mismatch in column 0).  The slow paths:
    an N in the query or in the target (beyond the overlap where it is shorter than 100 columns, inside it - one of the kmax mismatches -
    where it is longer), a reverse target"""
    i = 0
    for path in STATS_PATHS:
        for side in ("right", "left"):
            for n in STATS_N:
                if path == "rev" and n == 1:
                    continue                                        # (qs == qe: a record of one column cannot say that it is reversed)
                long_ = n > 100
                members = [("in", None), ("out", n - 1)] + ([("out0", 0)] if n in (17, 1025) else [])
                for tag, extra in members:
                    i += 1
                    over = 20 + i % 13 if long_ else _STATS_OVER[n]
                    qlen = (n + 16 * (1 + i % 2) + (0, 1, 15, 7)[i % 4] - n % 16) if long_ else max(_STATS_QLEN[i % 4], over)
                    assert qlen >= n and qlen >= over
                    query = bytearray(rnd(rs, qlen))
                    k = kmax(n)
                    ncol = n // 2                                   # the column of the N, as aligned
                    if path == "qn":
                        # inside a long overlap; beyond a short one (two columns off its end, which every n here leaves room for)
                        pos = (qlen - n + ncol if side == "right" else ncol) if long_ else (qlen - n - 2 if side == "right" else n + 1)
                        assert 0 <= pos < qlen
                        query[pos] = ord("N")
                    q = S.seq(bytes(query))
                    inside_n = long_ and path in ("qn", "tn")
                    cols = spread(n, k - 1 if inside_n else k, avoid=(ncol,)) if n > 2 else []
                    ed = both(no_n, ts(*cols), ts(extra) if extra is not None else None)
                    sed = None
                    if path == "tn":
                        tpos = ((ncol if side == "right" else over + ncol) if long_ else (n + 1 if side == "right" else over - 2))
                        sed = put((tpos, "N"))
                    cand(S, rs, q, side, n, over, edit=ed, sedit=sed, rev=path == "rev")
                    grows = tag == "in"
                    S.group("stats_%s_%s_%d_%s" % (path, side, n, tag), q, side if grows else "none", qlen + over if grows else None,
                            pair=("stats_%s_%s_%d" % (path, side, n), tag))
    # a reverse target's N, inside the overlap and at the mirrored place of the stored sequence (which lies in the overhang as aligned)
    for tag, tpos in (("in", 5), ("mirror", 64)):
        q = S.seq(rnd(rs, 60))
        cand(S, rs, q, "right", 40, 30, sedit=put((tpos, "N")), rev=True)
        S.group("stats_rev_n_%s" % tag, q, "right" if tag == "mirror" else "none", 90 if tag == "mirror" else None, pair=("stats_rev_n", "in" if tag == "mirror" else "out"))
    for tag, tpos in (("in", 65), ("mirror", 70 - 1 - 65)):
        q = S.seq(rnd(rs, 60))
        cand(S, rs, q, "left", 40, 30, sedit=put((tpos, "N")), rev=True)
        S.group("stats_rev_n_left_%s" % tag, q, "left" if tag == "mirror" else "none", 90 if tag == "mirror" else None, pair=("stats_rev_n_left", "in" if tag == "mirror" else "out"))


# the damage columns: see damage_groups
DAMAGE_COLS = (("c0", 0), ("c15", 15), ("c16", 16), ("last", None))


def damage_groups(S, rs, lead=None, lead_swap=None):
    """C over T and G over A (query letter over target letter) count towards deamMatch, T over C and A over G do not.  Two right
    candidates: `a`, clean and short, and `b`, 200 columns with two mismatches (all that 200 columns may hold, and the gates count a
    damage column as a mismatch like any other) out of the columns 0, 15, 16 and the last: (0, 15), (16, last), (0, last), (15, 16).
    `dmg`: the first is C over T, the second G over A; `conv1` / `conv2`: the first / the second is its converse (T over C, A over G);
    `none`: both are.  With `a` of DAMAGE_LEAD columns the comparator's sum for (a, b) lies inside the middle zone with both columns
    counted - `b`, the longer one, donates - and above 0.55 with one or none: `a` donates.
    `ctct` / `gaga`: both columns C over T / both G over A, beside an `a` of DAMAGE_LEAD_SWAP columns, where the two posteriors (the
    profile's C>T and G>A rates differ) fall on different sides of 0.55: counts taken for one another show."""
    lead, lead_swap = lead or DAMAGE_LEAD, lead_swap or DAMAGE_LEAD_SWAP
    letters = {"dmg": (b"CT", b"GA"), "conv1": (b"TC", b"GA"), "conv2": (b"CT", b"AG"), "none": (b"TC", b"AG"), "ctct": (b"CT", b"CT"), "gaga": (b"GA", b"GA")}
    for c1, c2 in ((0, 15), (16, 199), (0, 199), (15, 16)):
        base = bytearray(rnd(rs, 300))
        tails = [rnd(rs, 20), rnd(rs, 20)]
        for tag in ("dmg", "conv1", "conv2", "none", "ctct", "gaga"):
            query = bytearray(base)
            o = 300 - 200
            l1, l2 = letters[tag]
            query[o + c1], query[o + c2] = l1[0], l2[0]
            q = S.seq(bytes(query))
            cand(S, rs, q, "right", lead_swap if tag in ("ctct", "gaga") else lead, 20, ext=tails[0])
            cand(S, rs, q, "right", 200, 20, ext=tails[1], edit=put((c1, l1[1]), (c2, l2[1])))
            S.group("damage_%d_%d_%s" % (c1, c2, tag), q, "right", 320, tails=tails, damage=(c1, c2, tag))


def stats_set(seed=61):
    rs = np.random.RandomState(seed)
    S = ExtSet()
    stats_groups(S, rs)
    damage_groups(S, rs)
    return S.finish()


# the columns of the clean competitor in the damage groups (found by running the oracle over a range of lengths: 61 .. 97 do for the
# first, docs/NOTEBOOK.md)
DAMAGE_LEAD, DAMAGE_LEAD_SWAP = 80, 80


# ------------------------------------------------------------------------------------------------------------------ gates
def gate_groups(S, rs):
    def one(name, n, over, edit=None, exp=True, qlen=None, side="right", pair=None, qedit=None, **kw):
        query = bytearray(rnd(rs, qlen or max(n + 20, over)))
        if qedit:
            qedit(query)
        q = S.seq(bytes(query))
        cand(S, rs, q, side, n, over, edit=edit, **kw)
        S.group(name, q, side if exp else "none", len(query) + over if exp else None, pair=pair)
        return q
    # 99/100 == 0.99f; 98/99 is below
    one("id_99of100", 100, 25, ts(50), True, pair=("id", "in"))
    one("id_98of99", 99, 25, ts(50), False, pair=("id", "out"))
    one("id_99of100_left", 100, 25, ts(50), True, side="left", pair=("id_left", "in"))
    one("id_98of99_left", 99, 25, ts(50), False, side="left", pair=("id_left", "out"))
    one("ry_99of100", 100, 25, tv(50), True, pair=("ry", "in"))
    one("ry_98of99", 99, 25, tv(50), False, pair=("ry", "out"))
    # two mismatches on 200 columns pass; as transversions too
    one("id_198of200", 200, 25, ts(50, 150), True, pair=("id200", "in"))
    one("id_197of200", 200, 25, ts(50, 100, 150), False, pair=("id200", "out"))
    one("ry_198of200", 200, 25, tv(50, 150), True, pair=("ry200", "in"))
    one("ry_197of200", 200, 25, both(tv(50, 150), tv(100)), False, pair=("ry200", "out"))
    # the self record alone, and beside a candidate
    q = S.seq(rnd(rs, 120))
    S.group("self_alone", q, "none")
    one("self_beside", 100, 25, None, True)
    # alnLength >= min(500, unsigned(0.2 dbLen)) for records below 500 columns
    for dblen, exp in ((2500, False), (2495, True), (2499, True)):
        one("alnlen_499_db%d" % dblen, 499, dblen - 499, None, exp, qlen=2001 + dblen % 7, pair=("alnlen_499", "in" if exp else "out"))
    one("alnlen_500_db3000", 500, 2500, None, True, qlen=2503, pair=("alnlen_499", "in"))
    one("alnlen_20_db100", 20, 80, None, True, qlen=90, pair=("alnlen_short", "in"))
    one("alnlen_20_db105", 20, 85, None, False, qlen=90, pair=("alnlen_short", "out"))
    # the recount without the N columns.  100 columns of which 50 hold N over N: with one mismatch 99/100, then 49/50; the sibling holds
    # an N over that letter instead - 99/100, then 49/49
    nn = list(range(20, 70))
    def n_over_n(query):
        for c in nn:
            query[len(query) - 100 + c] = ord("N")
    keep_n = lambda mid: None
    one("recount_nn_clean", 100, 25, keep_n, True, qlen=130, qedit=n_over_n, pair=("recount_nn", "in"))
    one("recount_nn_mismatch", 100, 25, ts(80), False, qlen=130, qedit=n_over_n, pair=("recount_nn", "out"))
    one("recount_nn_n_over_letter", 100, 25, put((80, "N")), True, qlen=130, qedit=n_over_n, pair=("recount_n_letter", "in"))
    # ... and with the letter under the query's N: N over a letter is a mismatch for the first gate only
    def n_at_80(query):
        n_over_n(query)
        query[len(query) - 100 + 80] = ord("N")
    one("recount_nn_letter_under_n", 100, 25, put((80, "A")), True, qlen=130, qedit=n_at_80, pair=("recount_n_letter", "in"))
    one("recount_two_n_over_letters", 100, 25, put((80, "N"), (81, "N")), False, qlen=130, qedit=n_over_n, pair=("recount_n_letter", "out"))
    # (1 - seqId) cons + 0.5: k mismatches on cons columns, beside a clean candidate a tenth longer
    for cons, k in ((100, 1), (200, 2), (300, 3), (1000, 10), (700, 7), (1001, 10)):
        q = S.seq(rnd(rs, cons + 150))
        tails = [rnd(rs, 20), rnd(rs, 20)]
        cand(S, rs, q, "right", cons, 20, ext=tails[0], edit=ts(*spread(cons, k)))
        cand(S, rs, q, "right", cons + cons // 10, 20, ext=tails[1])
        S.group("round_cons_%d_%d" % (cons, k), q, "right", cons + 170, tails=tails)
    # records that are neither left- nor right-starting - contained (the whole target inside the query) and interior (both ends inside
    # both sequences) - pass both gates on their first ratios and enter the heap with a zero key
    for fam in range(2):
        query = rnd(rs, 200)
        tails = [rnd(rs, 25) for _ in range(3)]
        orders = {"a": [0, 1, 2, 3, 4, 5, 6], "b": [6, 5, 4, 3, 2, 1, 0], "c": [3, 0, 5, 1, 6, 2, 4], "d": [5, 6, 0, 3, 1, 4, 2]}
        for o, order in sorted(orders.items()):
            q = S.seq(query)
            made = [mk(S, rs, q, "right", 100 + fam * 2 * j, 25, ext=tails[j]) for j in range(3)]
            for j in range(2):                                      # contained: query[30 + j .. 90 + j) is the whole target
                k = S.seq(query[30 + j:90 + j])
                made.append((k, (q, k, 30 + j, 89 + j, 0, 59)))
            for j in range(2):                                      # interior: 60 columns between 10 other letters on either side
                k = S.seq(rnd(rs, 10) + query[50 + j:110 + j] + rnd(rs, 10))
                made.append((k, (q, k, 50 + j, 109 + j, 10, 69)))
            for j in order:
                S.rec(*made[j][1])
            S.group("neither_mixed_%d_%s" % (fam, o), q, "right", 225, tails=tails, **({"tie": ("right", "neither")} if fam == 0 else {}))


def gates_set(seed=67):
    rs = np.random.RandomState(seed)
    S = ExtSet()
    gate_groups(S, rs)
    return S.finish()


# ------------------------------------------------------------------------------------------------------------------- heap
HEAP_SIZES = (1, 2, 3, 4, 5, 7, 8, 33, 200)
ZONE_COLUMNS = (100, 100, 104, 110, 96, 130, 160, 118)
MIXED_SIZES = (4, 5, 6, 7, 8, 9)


def heap_groups(S, rs):
    """k right candidates with the same 40 overlap letters and overhangs of 25 other letters each: equal keys, so the comparator says
    `worse` whichever way it is asked, and libstdc++'s sift order decides which target donates; the siblings hold the same candidates
    under other record orders.  The first donor's 25 letters are all any of them has: the others are dropped at `overhang <= rightOff`"""
    for k in HEAP_SIZES:
        for side in ("right", "left") if k <= 8 else ("right",):
            query, tails = rnd(rs, 70), [rnd(rs, 25) for _ in range(k)]
            assert len(set(tails)) == k
            orders = {"a": list(range(k)), "b": list(range(k))[::-1], "c": list(range(1, k)) + [0], "d": [int(x) for x in rs.permutation(k)]}
            for o, order in sorted(orders.items()):
                if k == 1 and o != "a":
                    continue
                q = S.seq(query)
                made = [mk(S, rs, q, side, 40, 25, ext=t) for t in tails]
                for j in order:
                    S.rec(*made[j][1])
                S.group("tie_%s_%d_%s" % (side, k, o), q, side, 95, tails=tails, tie=(side, k), heap=k)
    # overlaps of other lengths: sums below, inside and above the middle zone, alnLengthCons smaller, equal and larger
    query, tails = rnd(rs, 200), [rnd(rs, 25) for _ in ZONE_COLUMNS]
    k = len(ZONE_COLUMNS)
    orders = {"a": list(range(k)), "b": list(range(k))[::-1], "c": [3, 0, 5, 1, 6, 2, 7, 4], "d": [5, 6, 0, 3, 7, 1, 4, 2], "e": [2, 4, 7, 6, 5, 3, 1, 0]}
    for o, order in sorted(orders.items()):
        q = S.seq(query)
        made = [mk(S, rs, q, "right", n, 25, ext=t) for n, t in zip(ZONE_COLUMNS, tails)]
        for j in order:
            S.rec(*made[j][1])
        S.group("zone_%s" % o, q, "right", 225, tails=tails, zone=True, heap=k)
    # candidates of both sides in one queue: the first right one and the first left one popped both donate, so the output shows two
    # places of the pop order - equal keys (40 columns each), and the overlaps of ZONE_COLUMNS dealt out to the two sides
    for k in MIXED_SIZES:
        query, exts = rnd(rs, 70), [rnd(rs, 25) for _ in range(k)]
        orders = {"a": list(range(k)), "b": list(range(k))[::-1], "c": list(range(1, k)) + [0], "d": [int(x) for x in rs.permutation(k)]}
        for o, order in sorted(orders.items()):
            q = S.seq(query)
            made = [mk(S, rs, q, ("right", "left")[j % 2], 40, 25, ext=t) for j, t in enumerate(exts)]
            for j in order:
                S.rec(*made[j][1])
            S.group("tie_mixed_%d_%s" % (k, o), q, "both", 120, tails=exts, tie=("both", k), heap=k)
    query, exts = rnd(rs, 200), [rnd(rs, 25) for _ in ZONE_COLUMNS]
    k = len(ZONE_COLUMNS)
    orders = {"a": list(range(k)), "b": list(range(k))[::-1], "c": [3, 0, 5, 1, 6, 2, 7, 4], "d": [5, 6, 0, 3, 7, 1, 4, 2]}
    for o, order in sorted(orders.items()):
        q = S.seq(query)
        made = [mk(S, rs, q, ("right", "left")[j % 2], n, 25, ext=t) for j, (n, t) in enumerate(zip(ZONE_COLUMNS, exts))]
        for j in order:
            S.rec(*made[j][1])
        S.group("zone_mixed_%s" % o, q, "both", 250, tails=exts, zone=True, heap=k)
    # ... and with one or two mismatches in some of them (keys that differ in deamMatch at equal alnLengthCons)
    query, tails = rnd(rs, 260), [rnd(rs, 25) for _ in range(6)]
    edits = [None, ts(50), ts(50, 120), None, tv(70), ts(30)]
    cols = [200, 200, 200, 210, 200, 190]
    for o, order in (("a", [0, 1, 2, 3, 4, 5]), ("b", [5, 4, 3, 2, 1, 0]), ("c", [2, 0, 4, 1, 5, 3]), ("d", [1, 2, 4, 5, 0, 3])):
        q = S.seq(query)
        made = [mk(S, rs, q, "right", n, 25, ext=t, edit=e) for n, t, e in zip(cols, tails, edits)]
        for j in order:
            S.rec(*made[j][1])
        S.group("keys_%s" % o, q, "right", 285, tails=tails, heap=6)


def heap_set(seed=71):
    rs = np.random.RandomState(seed)
    S = ExtSet()
    heap_groups(S, rs)
    return S.finish()


# ----------------------------------------------------------------------------------------------------------------- rounds
def chain(S, rs, name, side, cols, overs, qlen, genome=None, edits=None, exp=None, exp_len=None, **more):
    """candidates of one side whose overhangs are prefixes (right) / suffixes (left) of one `genome`, nearest letter first.  cols[0] leads
    (module text: `leader`), the others are parked behind it"""
    q = S.seq(rnd(rs, qlen))
    genome = rnd(rs, max(overs)) if genome is None else genome
    for i, (n, o) in enumerate(zip(cols, overs)):
        g = bytearray(genome[:o])
        if edits and edits[i]:
            edits[i](g)
        cand(S, rs, q, side, n, o, ext=bytes(g) if side == "right" else bytes(g[::-1]))
    S.group(name, q, side if exp is None else exp, exp_len, round1=qlen + overs[0], **more)
    return q


def round_groups(S, rs):
    q = S.seq(rnd(rs, 130)); cand(S, rs, q, "right", 100, 25)
    S.group("right_only", q, "right", 155)
    q = S.seq(rnd(rs, 130)); cand(S, rs, q, "left", 100, 25)
    S.group("left_only", q, "left", 155)
    q = S.seq(rnd(rs, 130)); cand(S, rs, q, "right", 100, 25); cand(S, rs, q, "left", 90, 31)
    S.group("both_one_round", q, "both", 186)
    for side in ("right", "left"):
        chain(S, rs, "parked_%s" % side, side, (160, 100), (10, 30), 180, exp_len=210, rounds=2)
        chain(S, rs, "chain3_%s" % side, side, (250, 160, 100), (10, 30, 50), 270, exp_len=320, rounds=3)
        chain(S, rs, "chain4_%s" % side, side, (400, 250, 160, 100), (10, 30, 50, 70), 420, exp_len=490, rounds=4)
        # the parked hit on the grown query: 91 + 10 = 101 columns, identity over the first 100.  The letters the leader gave are the
        # genome's; the parked target holds another letter in one (99/100 == 0.99f: queued again and used) or two of them
        g = lambda *cols: (lambda t: [t.__setitem__(c, bytes([t[c]]).translate(_TRANSITION)[0]) for c in cols])
        chain(S, rs, "realign_pass_%s" % side, side, (160, 91), (10, 30), 180, edits=(None, g(3)), exp_len=210, pair=("realign_%s" % side, "in"), parked_fails=False)
        chain(S, rs, "realign_fail_%s" % side, side, (160, 91), (10, 30), 180, edits=(None, g(3, 6)), exp_len=190, pair=("realign_%s" % side, "out"), parked_fails=True)
        # the skip rules: an overhang equal to what was added is dropped, one more letter is parked and used
        chain(S, rs, "skip_eq_%s" % side, side, (160, 100), (20, 20), 180, exp_len=200, pair=("skip_%s" % side, "out"), skip=side)
        chain(S, rs, "skip_plus1_%s" % side, side, (160, 100), (20, 21), 180, exp_len=201, pair=("skip_%s" % side, "in"))
    # the last column of a re-aligned overlap counts for the RY identity alone.  Right: the last column is the last letter the leader gave
    # (genome[9]); left: the columns run from the target's start, the last one is the query's old column 90.  One transversion elsewhere
    # in both members (99/100 and 100/101); the last column's transversion leaves the identity alone and makes the RY ratio 99/101
    tvg = lambda *cols: (lambda t: [t.__setitem__(c, bytes([t[c]]).translate(_RYFLIP)[0]) for c in cols])
    chain(S, rs, "ry_last_in_right", "right", (160, 91), (10, 30), 180, edits=(None, tvg(3)), exp_len=210, pair=("ry_last_right", "in"), parked_fails=False)
    chain(S, rs, "ry_last_out_right", "right", (160, 91), (10, 30), 180, edits=(None, tvg(3, 9)), exp_len=190, pair=("ry_last_right", "out"), parked_fails=True)
    # both sides in one round with a parked hit on each: the left one is re-aligned on a negative diagonal, the right one on a positive
    # diagonal that holds leftOff
    q = S.seq(rnd(rs, 180))
    gr, gl = rnd(rs, 30), rnd(rs, 35)
    cand(S, rs, q, "right", 160, 10, ext=gr[:10]); cand(S, rs, q, "right", 100, 30, ext=gr)
    cand(S, rs, q, "left", 150, 15, ext=gl[20:]); cand(S, rs, q, "left", 95, 35, ext=gl)
    S.group("parked_both", q, "both", 245, round1=205, rounds=2)
    # left growth alone, a right hit parked?  No: a right hit is parked behind a right growth only.  Left growth in round 1 beside a parked
    # right hit whose leader is on the right as well, the left candidate being the best of all
    q = S.seq(rnd(rs, 300))
    gr = rnd(rs, 30)
    cand(S, rs, q, "left", 280, 17); cand(S, rs, q, "right", 160, 10, ext=gr[:10]); cand(S, rs, q, "right", 100, 30, ext=gr)
    S.group("left_first_parked_right", q, "both", 347, round1=327, rounds=2)
    # ds == 0 and qs == 0: the whole query on the target's prefix is never taken from the queue
    q = S.seq(rnd(rs, 100))
    k = S.seq(S.seqs[q] + rnd(rs, 25)); S.rec(q, k, 0, 99, 0, 99)
    S.group("both_zero", q, "none")
    # a right-starting record without an overhang: the target is the query's suffix
    q = S.seq(rnd(rs, 100))
    k = S.seq(S.seqs[q][40:]); S.rec(q, k, 40, 99, 0, 59)
    S.group("no_overhang", q, "none")
    # a popped hit that fits neither branch: it starts the target (or the query) but ends inside both sequences; alone, and behind a
    # candidate that the round takes first (100 clean columns against 60) - its 25 letters then drop the right-starting one of the two
    # at the offset rule (20 letters beyond its overlap), the other one still falls through
    for beside in (False, True):
        q = S.seq(rnd(rs, 130))
        k = S.seq(S.seqs[q][10:70] + rnd(rs, 20)); S.rec(q, k, 10, 69, 0, 59)
        k = S.seq(rnd(rs, 20) + S.seqs[q][0:60] + rnd(rs, 9)); S.rec(q, k, 0, 59, 20, 79)
        if beside:
            cand(S, rs, q, "right", 100, 25)
        S.group("neither_branch%s" % ("_beside" if beside else ""), q, "right" if beside else "none", 155 if beside else None, neither=1 if beside else 2)
    # a two-column re-aligned overlap: the parked target holds one column and five letters more; the leader gives one letter
    q = S.seq(rnd(rs, 120))
    g = rnd(rs, 5)
    cand(S, rs, q, "right", 100, 1, ext=g[:1]); cand(S, rs, q, "right", 1, 5, ext=g)
    S.group("realign_2col", q, "right", 125, round1=121, rounds=2)
    # re-aligned overlaps of 1024 and 1025 columns (a wave step is 64 lanes x 16 columns)
    for n2 in (1014, 1015):
        chain(S, rs, "realign_%d" % (n2 + 10), "right", (1300, n2), (10, 30), 1310 + n2 % 7, exp_len=1310 + n2 % 7 + 30, rounds=2)
    chain(S, rs, "realign_1024_left", "left", (1300, 1014), (10, 30), 1311, exp_len=1341, rounds=2)
    # the ladder: 40 clean overlaps of 300 .. 261 columns (every pair inside the middle zone: popped longest first), each reaching
    # five letters beyond the one before - one growth a round
    q = S.seq(rnd(rs, 320))
    genome = rnd(rs, 200)
    for i in range(40):
        cand(S, rs, q, "right", 300 - i, 5 * (i + 1), ext=genome[:5 * (i + 1)])
    S.group("ladder", q, "right", 520, round1=325, rounds=40)


def rounds_set(seed=73):
    rs = np.random.RandomState(seed)
    S = ExtSet()
    round_groups(S, rs)
    return S.finish()


# ---------------------------------------------------------------------------------------------------------------- letters
FRAGMENTS = (1, 15, 16, 17, 31, 33)


def letter_groups(S, rs):
    i = 0
    for rev in (False, True):
        for f in FRAGMENTS:
            for side in ("right", "left"):
                i += 1
                q = S.seq(rnd(rs, 50 + i % 17))
                cand(S, rs, q, side, 40, f, rev=rev)
                S.group("frag_%s_%d_%s" % (side, f, "rev" if rev else "fwd"), q, side, len(S.seqs[q]) + f)
            i += 1
            q = S.seq(rnd(rs, 50 + i % 17))
            cand(S, rs, q, "right", 40, f, rev=rev)
            cand(S, rs, q, "left", 40, FRAGMENTS[(FRAGMENTS.index(f) + 2) % 6], rev=not rev)
            S.group("frag_both_%d_%s" % (f, "rev" if rev else "fwd"), q, "both", len(S.seqs[q]) + f + FRAGMENTS[(FRAGMENTS.index(f) + 2) % 6])
    # one 16-letter word holds the left fragment, the query and the start of the right fragment
    for rev in (False, True):
        q = S.seq(rnd(rs, 8))
        cand(S, rs, q, "left", 5, 3, rev=rev)
        cand(S, rs, q, "right", 5, 4, rev=rev)
        S.group("three_pieces_%s" % ("rev" if rev else "fwd"), q, "both", 15)
    # N at the first and the last letter of a fragment shorter than 16
    for rev in (False, True):
        for side in ("right", "left"):
            q = S.seq(rnd(rs, 57))
            cand(S, rs, q, side, 40, 7, ext=b"N" + rnd(rs, 5) + b"N", rev=rev)
            S.group("frag_n_ends_%s_%s" % (side, "rev" if rev else "fwd"), q, side, 64)
            q = S.seq(rnd(rs, 61))
            cand(S, rs, q, side, 40, 12, ext=b"N" + rnd(rs, 11) if side == "right" else rnd(rs, 11) + b"N", rev=rev)
            S.group("frag_n_joint_%s_%s" % (side, "rev" if rev else "fwd"), q, side, 73)
    # a query without N gains one from the leader; the parked hit is re-aligned across it (108 of 109 letters, 109 or 110 of 110 classes)
    for tag, under in (("letter_c", "C"), ("letter_a", "A"), ("n", "N")):
        for side in ("right", "left"):
            q = S.seq(rnd(rs, 180))
            genome = bytearray(rnd(rs, 30))
            lead = bytearray(genome[:10]); lead[3] = ord("N")
            genome[3] = ord(under)
            if side == "right":
                cand(S, rs, q, side, 160, 10, ext=bytes(lead)); cand(S, rs, q, side, 100, 30, ext=bytes(genome))
            else:
                cand(S, rs, q, side, 160, 10, ext=bytes(lead[::-1])); cand(S, rs, q, side, 100, 30, ext=bytes(genome[::-1]))
            S.group("gains_n_%s_%s" % (tag, side), q, side, 210, round1=190, rounds=2)
    # useReverse is the strand of the query's LAST record with the target: a forward candidate, then a second record of the same target
    # on the other strand, which fails the first gate - the fragment is then cut from the reverse-complemented target
    q = S.seq(rnd(rs, 130))
    k = cand(S, rs, q, "right", 100, 25)
    S.recs[q].append("%d\t%d\t%s\t1.000E-20\t%d\t%d\t%d\t%d\t%d\t%d" % (k, 80, "1.00", 129, 90, 130, 10, 49, 125))
    S.group("use_reverse_last", q, "right", 155, twice=k)


def letters_set(seed=79):
    rs = np.random.RandomState(seed)
    S = ExtSet()
    letter_groups(S, rs)
    return S.finish()


# ----------------------------------------------------------------------------------------------------------------- maxlen
def maxlen_set(seed=83):
    """--max-seq-len 400: the loop breaks where the query's length + the fragment's >= 400"""
    rs = np.random.RandomState(seed)
    S = ExtSet()
    B = MAXLEN_BOUND
    for name, over, exp in (("maxlen_at", 100, "none"), ("maxlen_below", 99, "right")):
        q = S.seq(rnd(rs, 300)); cand(S, rs, q, "right", 100, over)
        S.group(name, q, exp, 399 if exp == "right" else None, pair=("maxlen", "in" if exp == "right" else "out"))
    # the break leaves the queue non-empty: the loop ends, and the left candidate behind the refused one is never tried (alone it fits)
    q = S.seq(rnd(rs, 300)); cand(S, rs, q, "right", 250, 100); cand(S, rs, q, "left", 160, 20)
    S.group("break_queue_not_empty", q, "none", pair=("break_left", "out"))
    q = S.seq(rnd(rs, 300)); cand(S, rs, q, "right", 250, 79); cand(S, rs, q, "left", 160, 20)
    S.group("no_break", q, "both", 399, pair=("break_left", "in"))
    # growth to the right, then the break on the left with the queue non-empty (a third candidate behind): the loop ends, the parked
    # right hit is never re-aligned
    q = S.seq(rnd(rs, 300)); g = rnd(rs, 30)
    cand(S, rs, q, "right", 280, 10, ext=g[:10]); cand(S, rs, q, "right", 200, 30, ext=g); cand(S, rs, q, "left", 150, 90); cand(S, rs, q, "left", 100, 5)
    S.group("grow_then_break_not_empty", q, "right", 310, round1=310)
    # ... on the last element: the queue is empty, the round goes on to its parked hit
    q = S.seq(rnd(rs, 300)); g = rnd(rs, 30)
    cand(S, rs, q, "right", 280, 10, ext=g[:10]); cand(S, rs, q, "right", 200, 30, ext=g); cand(S, rs, q, "left", 150, 90)
    S.group("grow_then_break_last", q, "right", 330, round1=310, rounds=2)
    # the parked hit's own fragment reaches the bound in round 2
    q = S.seq(rnd(rs, 300)); g = rnd(rs, 100)
    cand(S, rs, q, "right", 280, 10, ext=g[:10]); cand(S, rs, q, "right", 200, 100, ext=g)
    S.group("parked_at_bound", q, "right", 310, round1=310)
    q = S.seq(rnd(rs, 300)); g = rnd(rs, 99)
    cand(S, rs, q, "right", 280, 10, ext=g[:10]); cand(S, rs, q, "right", 200, 99, ext=g)
    S.group("parked_below_bound", q, "right", 399, round1=310, rounds=2)
    # the whole pop order of a queue of equal keys, seen through the break: k - 1 right candidates of 100 clean columns that reach 10, 20,
    # ... letters into one genome, and one left candidate of 100 columns whose 100 letters the bound refuses wherever it is popped.  The
    # first right candidate popped donates; popped last, the left one leaves the queue empty and the parked hits go on to the longest
    # overhang; popped earlier, it ends the loop at what the first one gave
    for k in BREAK_ORDER_SIZES:
        query, genome, head = rnd(rs, 300), rnd(rs, 10 * (k - 1)), rnd(rs, 100)
        orders = {"a": list(range(k)), "b": list(range(k))[::-1], "c": list(range(1, k)) + [0], "d": [int(x) for x in rs.permutation(k)]}
        for o, order in sorted(orders.items()):
            q = S.seq(query)
            made = [mk(S, rs, q, "right", 100, 10 * (j + 1), ext=genome[:10 * (j + 1)]) for j in range(k - 1)] + [mk(S, rs, q, "left", 100, 100, ext=head)]
            for j in order:
                S.rec(*made[j][1])
            S.group("break_order_%d_%s" % (k, o), q, None, None, order_family=k)     # (the heap's: nothing, where the left one is popped first)
    # ... and of a queue of keys that differ, every pair inside the middle zone (118, 116, ... columns on the right, 100 on the left): the
    # longer overlap is popped first whatever the record order, the left one last - the parked hits go on to the longest overhang
    for k in BREAK_ORDER_SIZES:
        query, genome, head = rnd(rs, 300), rnd(rs, 10 * (k - 1)), rnd(rs, 100)
        orders = {"a": list(range(k)), "b": list(range(k))[::-1], "c": list(range(1, k)) + [0], "d": [int(x) for x in rs.permutation(k)]}
        for o, order in sorted(orders.items()):
            q = S.seq(query)
            made = [mk(S, rs, q, "right", 118 - 2 * j, 10 * (j + 1), ext=genome[:10 * (j + 1)]) for j in range(k - 1)] + [mk(S, rs, q, "left", 100, 100, ext=head)]
            for j in order:
                S.rec(*made[j][1])
            S.group("break_keys_%d_%s" % (k, o), q, "right", 300 + 10 * (k - 1), round1=310, rounds=k - 1)
    assert max(len(s) for s in S.seqs) < B
    return S.finish()


# ------------------------------------------------------------------------------------------------------------------- wide
WIDE_QUERIES = 150


def wide_set(seed=89):
    """150 active queries (two full waves and 22 lanes) with 0, 1 and 5 parked hits, interleaved so that the counts differ within a
    wave; the five parked hits have equal keys and reach 10 .. 50 letters beyond the leader: how many rounds they take is the heap's"""
    rs = np.random.RandomState(seed)
    S = ExtSet()
    for i in range(WIDE_QUERIES):
        q = S.seq(rnd(rs, 90 + i % 5))
        genome = rnd(rs, 60)
        cand(S, rs, q, "right", 80, 10, ext=genome[:10])
        parked = (0, 1, 5)[i % 3]
        for j in range(parked):
            cand(S, rs, q, "right", 48, 20 + 10 * j, ext=genome[:20 + 10 * j])
        S.group("wide_%d_p%d" % (i, parked), q, "right", len(S.seqs[q]) + (10, 20, 60)[i % 3], round1=len(S.seqs[q]) + 10, parked=parked)
    return S.finish()


# --------------------------------------------------------------------------------------------------------------- handback
def handback_set(seed=97):
    """letters beyond ACGTN: the device hands such a query back to the host code - at once where the query holds them, in the round
    that meets them where a target does"""
    rs = np.random.RandomState(seed)
    S = ExtSet()
    for name, letters in (("iupac", b"RYKM"), ("lower", b"acgt")):
        query = bytearray(rnd(rs, 180))
        for j, c in enumerate(letters):
            query[5 + 3 * j] = c                                    # outside the overlap
        q = S.seq(bytes(query)); cand(S, rs, q, "right", 100, 25)
        S.group("query_%s" % name, q, None)
        # a target with such letters in its overhang, parked in round 1 and met again in round 2
        q = S.seq(rnd(rs, 180)); g = bytearray(rnd(rs, 30))
        cand(S, rs, q, "right", 160, 10, ext=bytes(g[:10]))
        g[20], g[25] = letters[0], letters[1]
        cand(S, rs, q, "right", 100, 30, ext=bytes(g))
        S.group("target_round2_%s" % name, q, None)
    q = S.seq(rnd(rs, 130)); cand(S, rs, q, "right", 100, 25)
    S.group("plain_beside", q, "right", 155)
    return S.finish()


# ---------------------------------------------------------------------------------------------------------------- refusal
def refusal_set(beyond, seed=101):
    """one right candidate that overhangs its query of 120 letters by 120 (`beyond` = 0: the last defined case) or 121 letters"""
    rs = np.random.RandomState(seed)
    S = ExtSet()
    q = S.seq(rnd(rs, 120))
    query = S.seqs[q]
    k = S.seq(query[20:] + rnd(rs, 120 + beyond)); S.rec(q, k, 20, 119, 0, 99)
    S.group("overhang_qlen_plus_%d" % beyond, q, "right" if beyond == 0 else None, 240 if beyond == 0 else None)
    return S.finish()


# ----------------------------------------------------------------------------------------------------------------- tables
TABLES_QLEN, TABLES_OVERLAP = 270000, (1 << 18) + 1000


def tables_set(seed=103):
    """made at run time, no golden: one query of 270 000 letters and two right candidates that overlap it by more than 2^18 columns
    each - the comparator's lgammaf argument xHit + yHit leaves the device's table, the query goes back to the host"""
    rs = np.random.RandomState(seed)
    S = ExtSet()
    q = S.seq(rnd(rs, TABLES_QLEN))
    g = rnd(rs, 40)
    cand(S, rs, q, "right", TABLES_OVERLAP + 3000, 20, ext=g[:20]); cand(S, rs, q, "right", TABLES_OVERLAP, 40, ext=g)
    S.group("beyond_tables", q, "right", None)
    q = S.seq(rnd(rs, 130)); cand(S, rs, q, "right", 100, 25)
    S.group("plain_beside", q, "right", 155)
    return S.finish()


TABLES_MAX_SEQ_LEN = 600000

# (name, maker, --max-seq-len); the goldens hold these
SETS = (("stats", stats_set, 200000), ("gates", gates_set, 200000), ("heap", heap_set, 200000), ("rounds", rounds_set, 200000),
        ("letters", letters_set, 200000), ("maxlen", maxlen_set, MAXLEN_BOUND), ("wide", wide_set, 200000))
# `main`: the sets whose groups the --unsafe 1 rows and the hand-back rows run again
MAIN = ("gates", "rounds", "letters")


def flags_for(max_seq_len, unsafe=0, min_cov=5):
    from carpedeam_amd.stageflags import AC_FLAGS
    return (" ".join(AC_FLAGS).replace("--max-seq-len 200000", "--max-seq-len %d" % max_seq_len).replace("--unsafe 0", "--unsafe %d" % unsafe)
            .replace("--min-cov-safe 5", "--min-cov-safe %d" % min_cov).split())


def gate_pairs(S):
    """pair name -> {"in": [group names], "out": [group names]}"""
    out = {}
    for g in S.groups:
        if g.get("pair"):
            out.setdefault(g["pair"][0], {"in": [], "out": []})["out" if g["pair"][1].startswith("out") else "in"].append(g["name"])
    return out


def overhang_beyond_query(S, q):
    """the device (and the host code) refuses a left- or right-starting target that overhangs the query by more than the query's length"""
    qlen = len(S.seqs[q])
    for l in S.recs[q]:
        f = l.split("\t")
        t, qs, qe, ds, de, tlen = int(f[0]), int(f[4]), int(f[5]), int(f[7]), int(f[8]), int(f[9])
        if t != q and tlen - (max(abs(qe - qs), de - ds) + 1) > qlen:
            return True
    return False


def without_unsupported(S):
    """The set for the --unsafe 1 rows: (sequences, alignments, number of groups taken out).  What the device refuses - a query with a
    target that overhangs it by more than its length - loses its records"""
    refused = {g["query"] for g in S.groups if overhang_beyond_query(S, g["query"])}
    seq, aln = S.seq_keyed(), S.aln_keyed()
    keys = S.keys
    for q in refused:
        aln[keys[q]] = (b"", 0)
    return seq, aln, len(refused)


# ------------------------------------------------------------------------------------- the committed fixtures and the oracle on them
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contig_directed")


def fixture(name, what):
    from carpedeam_amd import mmdb
    return mmdb.load_keyed(os.path.join(DIR, name, what + ".keyed.gz"))


def run_oracle_on(oracle_bin, dhigh_prefix, tmp, name, seq_keyed, aln_keyed, max_seq_len, unsafe=0, min_cov=5, exe_name="oracle"):
    """ancient_contig_merge of `oracle_bin` on a keyed sequence DB and alignment DB: (merged DB, event log)"""
    from carpedeam_amd import mmdb
    from gpuutil import OracleCrash
    t = lambda s: os.path.join(str(tmp), "%s_%s_%s" % (exe_name, name, s))
    mmdb.write_from_keyed(t("corr"), seq_keyed, mmdb.DBTYPE_NUCLEOTIDES)
    mmdb.write_from_keyed(t("aln"), aln_keyed, mmdb.DBTYPE_ALIGNMENT_RES)
    r = subprocess.run([oracle_bin, "ancient_contig_merge", t("corr"), t("aln"), t("cmerge")] + flags_for(max_seq_len, unsafe, min_cov) + ["--ancient-damage", dhigh_prefix, "--threads", "4"],
                       capture_output=True, text=True, env=dict(os.environ, ORACLE_CONTIG_LOG=t("events.tsv")))
    if r.returncode < 0:
        raise OracleCrash("ancient_contig_merge of %s ended with signal %d on set %s" % (os.path.basename(oracle_bin), -r.returncode, name))
    assert r.returncode == 0, r.stderr[-2000:]
    return mmdb.read_db(t("cmerge")), (parse_event_log(t("events.tsv")) if os.path.exists(t("events.tsv")) else None)


def run_oracle_on_fixture(oracle_bin, dhigh_prefix, tmp, name, max_seq_len):
    return run_oracle_on(oracle_bin, dhigh_prefix, tmp, name, fixture(name, "corr"), fixture(name, "aln"), max_seq_len)


class Events:
    """ORACLE_CONTIG_LOG, per query key: gated = [(target, alnLengthCons, deamMatch bits)] in the order pushed; zone = [(cons1, cons2, sum)]
    for every comparator call whose sum lies in [0.45, 0.55]; pops = [(round, target)]; skips = [(round, target, side, overhang, offset)];
    neither = [(round, target)]; breaks = [(round, target, side, queue size)]; rounds = [(round, leftOff, rightOff, parked, queue size)];
    realigned = [(round, target, diag, qs, qe, ds, de, seqId, rySeqId, queued again)]"""

    def __init__(self):
        self.gated, self.zone, self.pops, self.skips, self.neither, self.breaks, self.rounds, self.realigned = [], [], [], [], [], [], [], []


def parse_event_log(path):
    out = {}
    for line in open(path):
        f = line.rstrip("\n").split("\t")
        e = out.setdefault(int(f[1]), Events())
        if f[0] == "G":
            e.gated.append((int(f[2]), int(f[3]), int(f[4], 16)))
        elif f[0] == "C":
            e.zone.append((int(f[2]), int(f[3]), float.fromhex(f[4])))
        elif f[0] == "P":
            e.pops.append((int(f[2]), int(f[3])))
        elif f[0] == "S":
            e.skips.append((int(f[2]), int(f[3]), f[4], int(f[5]), int(f[6])))
        elif f[0] == "X":
            e.neither.append((int(f[2]), int(f[3])))
        elif f[0] == "B":
            e.breaks.append((int(f[2]), int(f[3]), f[4], int(f[5])))
        elif f[0] == "R":
            e.rounds.append(tuple(int(x) for x in f[2:7]))
        elif f[0] == "A":
            e.realigned.append((int(f[2]), int(f[3])) + tuple(int(x) for x in f[4:9]) + (float.fromhex(f[9]), float.fromhex(f[10]), int(f[11])))
        else:
            raise AssertionError(line)
    return out


def device_totals(events):
    """What CDM_TIMING's summary line of the device queue must read, from the oracle's events, for queries that are not handed back:
    (rounds, growths, parked hits re-aligned).
      rounds   the device runs k_cq_round while a query is active; a query stays active while its round ends with the queue empty and
               parked hits (cqRound: parked = np), whether or not any of them passes its re-alignment.  The oracle's loop ends where none
               passes.  So a query's device rounds are its logged rounds, plus one where its last logged round parked hits with the
               queue empty; the line holds the maximum over the queries.
      growths  one per query and round with leftOff > 0 or rightOff > 0 (the `grown` list of a round).
      parked   the parked hits of every round that ends with the queue empty (only those are re-aligned, by both)."""
    rounds = growths = parked = 0
    for e in events.values():
        if not e.rounds:
            continue
        last = e.rounds[-1]
        rounds = max(rounds, len(e.rounds) + (1 if last[3] > 0 and last[4] == 0 else 0))
        growths += sum(1 for r in e.rounds if r[1] > 0 or r[2] > 0)
        parked += sum(r[3] for r in e.rounds if r[4] == 0)
    return rounds, growths, parked
