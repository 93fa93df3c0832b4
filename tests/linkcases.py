"""Directed and random inputs of cdm_pileup_links, shared by the model's own tests (CPU) and the device's (GPU): the smallest shapes at
which the kernels can go wrong.  A case is the dict of tests/pileupcases.py (seqs, ext, off / rec, queries, min_seq_id, skip) with "par"
(anchor, overhang, max_ends, min_reads); the directed ones carry their links written out by hand ("links": tuples in the order of the
record's fields without `reserved`) and, where the case is about them, "totals" and "stats" ({list index: {column: value}}).

The contigs come first in a case's DB, the reads behind them.  A bridge (T, x, oX, hX, y, oY, hY) is a read of T letters with a tail
record on contig x in orientation oX, hX of its letters beyond that contig's end, and a head record on contig y in orientation oY with
hY letters beyond: the edge (x, oX) -> (y, oY) with gap hX + hY - T."""
import numpy as np

import pileupcases as pc
from dedupcases import placed

FLIP = {"+": "-", "-": "+"}


def end_rec(t, t_len, q_len, right, h, rev, seq_id=1.0, clip=(0, 0)):
    """the record of read t whose h letters hang over the right (else the left) end of a query of q_len letters"""
    return placed(t, t_len, q_len, q_len - t_len + h if right else -h, rev, 0, seq_id, clip)


def tail_rec(t, t_len, q_len, o, h, **kw):
    """tail: (hangs right) != rev, so on a + contig the read leaves over the right end, on a - contig over the left"""
    return end_rec(t, t_len, q_len, o == "+", h, o == "-", **kw)


def head_rec(t, t_len, q_len, o, h, **kw):
    return end_rec(t, t_len, q_len, o == "-", h, o == "-", **kw)


def other_strand(b):
    """the bridge as the read's reverse complement shows it"""
    T, x, ox, hx, y, oy, hy = b
    return (T, y, FLIP[oy], hy, x, FLIP[ox], hx)


def build(contig_lens, bridges, seed, queries=None, par=None, extra=None, **kw):
    """extra: {contig: [lambda t: record]} - further records, each of a read of its own (t_len, make); a bridge may carry an eighth field,
    {"tail": kwargs, "head": kwargs} for end_rec (seq_id, clip)"""
    rng = np.random.default_rng(seed)
    nc = len(contig_lens)
    seqs = [pc.rand_seq(rng, n) for n in contig_lens]
    per = {q: [pc.identity(seqs, q)] for q in range(nc)}
    for b in bridges:
        T, x, ox, hx, y, oy, hy = b[:7]
        opt = b[7] if len(b) > 7 else {}
        t = len(seqs)
        seqs.append(pc.rand_seq(rng, T))
        per[x].append(tail_rec(t, T, contig_lens[x], ox, hx, **opt.get("tail", {})))
        per[y].append(head_rec(t, T, contig_lens[y], oy, hy, **opt.get("head", {})))
    for q, makers in (extra or {}).items():
        for t_len, make in makers:
            t = len(seqs)
            seqs.append(pc.rand_seq(rng, t_len))
            per[q].append(make(t))
    c = pc.case(seqs, per, list(range(nc)) if queries is None else queries, **kw)
    c["par"] = dict(anchor=16, overhang=1, max_ends=16, min_reads=2)
    c["par"].update(par or {})
    c["contigs"] = nc
    return c


def four_edges():
    """every edge type between a contig pair of its own, each seen by a read and by its reverse complement: one link of 2 pairs, 1 forward"""
    bridges = []
    for k, (oa, ob) in enumerate(("++", "+-", "-+", "--")):
        b = (60, 2 * k, oa, 30, 2 * k + 1, ob, 35)
        bridges += [b, other_strand(b)]
    c = build([100] * 8, bridges, 601)
    c["links"] = [(0, 1, 0, 2, 1, 2, 5, 5, 5, 10), (2, 3, 2, 2, 1, 2, 5, 5, 5, 10), (4, 5, 1, 2, 1, 2, 5, 5, 5, 10), (6, 7, 3, 2, 1, 2, 5, 5, 5, 10)]
    c["totals"] = [16, 0, 0, 8, 4]
    return c


def three_gaps():
    """an overlap of 5 letters, two contigs that abut, 7 letters between two contigs"""
    c = build([100] * 6, [(60, 0, "+", 25, 1, "+", 30), (60, 2, "+", 30, 3, "+", 30), (60, 4, "+", 37, 5, "+", 30)], 602, par=dict(min_reads=1))
    c["links"] = [(0, 1, 0, 1, 1, 1, -5, -5, -5, -5), (2, 3, 0, 1, 1, 1, 0, 0, 0, 0), (4, 5, 0, 1, 1, 1, 7, 7, 7, 7)]
    return c


def thresholds():
    """overhang 3, anchor 16: a read with 3 letters beyond contig 0 and 16 columns on contig 1 makes the link; one with 2 letters beyond
    and one with 15 columns make none, but their other record is an end record all the same"""
    c = build([100, 100], [(40, 0, "+", 3, 1, "+", 24), (40, 0, "+", 2, 1, "+", 24), (40, 0, "+", 3, 1, "+", 25)], 603, par=dict(overhang=3, min_reads=1))
    c["links"] = [(0, 1, 0, 1, 1, 1, -13, -13, -13, -13)]
    c["totals"] = [4, 0, 0, 1, 1]
    c["stats"] = {0: {0: 3, 1: 37 + 38 + 37, 2: 0, 3: 2, 5: 1}, 1: {0: 3, 1: 16 + 16 + 15, 2: 2, 3: 0, 5: 1}}
    return c


def both_ends():
    """a read of 60 letters over the whole of a contig of 20: counted in both_ends, no end record; its two outer records link 0 and 2"""
    c = build([100, 20, 100], [(60, 0, "+", 40, 2, "+", 40)], 604, par=dict(min_reads=1),
              extra={1: [(60, lambda t: placed(t, 60, 20, -18, False))]})
    # the spanning read is a read of its own: the bridge and it share no end record
    c["links"] = [(0, 2, 0, 1, 1, 1, 20, 20, 20, 20)]
    c["totals"] = [2, 0, 0, 1, 1]
    c["stats"] = {1: {0: 1, 1: 20, 2: 0, 3: 0, 4: 1, 5: 0}}
    return c


def self_pair():
    """a read that leaves contig 0 over its right end and enters it over its left: a self pair, no link"""
    c = build([100, 100], [(60, 0, "+", 30, 0, "+", 35), (60, 0, "+", 30, 1, "+", 35)], 605, par=dict(min_reads=1))
    c["links"] = [(0, 1, 0, 1, 1, 1, 5, 5, 5, 5)]
    c["totals"] = [4, 0, 1, 1, 1]
    return c


def crowded():
    """max_ends 16: a read with 8 tail records on contig 0 and 8 head records on contig 1 makes 64 pairs; one with 9 and 8 makes none"""
    rng = np.random.default_rng(606)
    seqs = [pc.rand_seq(rng, 100), pc.rand_seq(rng, 100), pc.rand_seq(rng, 60), pc.rand_seq(rng, 60)]
    per = {0: [pc.identity(seqs, 0)], 1: [pc.identity(seqs, 1)]}
    for t, tails in ((2, 8), (3, 9)):
        per[0] += [tail_rec(t, 60, 100, "+", 20 + i) for i in range(tails)]
        per[1] += [head_rec(t, 60, 100, "+", 20 + i) for i in range(8)]
    c = pc.case(seqs, per, [0, 1])
    c["par"] = dict(anchor=16, overhang=1, max_ends=16, min_reads=1)
    c["contigs"] = 2
    # gaps hX + hY - 60 over 20..27 x 20..27: -20 .. -6, the sum 47 eight times
    c["links"] = [(0, 1, 0, 64, 64, 8, -13, -20, -6, 64 * -60 + 2 * 8 * sum(range(20, 28)))]
    c["totals"] = [33, 1, 0, 64, 1]
    return c


def not_counted():
    """min_seq_id 0.9 and skip: of three bridges one has its tail record below the threshold and one is an extended sequence"""
    c = build([100, 100], [(60, 0, "+", 30, 1, "+", 35), (60, 0, "+", 30, 1, "+", 36, {"tail": {"seq_id": 0.5}}), (60, 0, "+", 30, 1, "+", 37)], 607, par=dict(min_reads=1),
              ext=[1, 1, 0, 0, 1], min_seq_id=0.9, skip=True)
    c["links"] = [(0, 1, 0, 1, 1, 1, 5, 5, 5, 5)]
    c["totals"] = [3, 0, 0, 1, 1]
    return c


def mode_tie():
    """gaps 4, 2, 4, 2: two values with two pairs each, the smaller is the mode"""
    c = build([100, 100], [(60, 0, "+", 30, 1, "+", 30 + g) for g in (4, 2, 4, 2)], 608)
    c["links"] = [(0, 1, 0, 4, 4, 2, 2, 2, 4, 12)]
    return c


def min_reads():
    """min_reads 2: a link of two pairs is returned, one of a single pair is counted in totals[4] alone"""
    c = build([100] * 4, [(60, 0, "+", 30, 1, "-", 33), (60, 0, "+", 31, 1, "-", 33), (60, 2, "+", 30, 3, "+", 33)], 609)
    c["links"] = [(0, 1, 2, 2, 2, 1, 3, 3, 4, 7)]
    c["totals"] = [6, 0, 0, 3, 2]
    c["stats"] = {2: {3: 1, 5: 0}, 3: {2: 1, 5: 0}, 0: {5: 1}, 1: {5: 1}}
    return c


def unlisted():
    """contig 2 is not listed: the bridges from 0 to 2 make no link, their records on 0 are end records"""
    c = build([100] * 3, [(60, 0, "+", 30, 2, "+", 33), (60, 0, "+", 30, 2, "+", 33), (60, 0, "-", 30, 1, "+", 33), (60, 0, "-", 30, 1, "+", 33)], 610, queries=[0, 1])
    c["links"] = [(0, 1, 1, 2, 2, 2, 3, 3, 3, 6)]
    c["totals"] = [6, 0, 0, 2, 1]
    return c


def permuted():
    """the list [2, 0, 1]: contig 0 is list index 1, contig 1 index 2, contig 2 index 0.  The edge (contig 0, +) -> (contig 1, -) stays as it
    stands, (1, +) -> (2, -); the edge (contig 1, +) -> (contig 2, +) goes from index 2 to 0 and is flipped: (0, -) -> (2, -), not forward"""
    c = build([100] * 3, [(60, 0, "+", 30, 1, "-", 31)] * 2 + [(60, 1, "+", 30, 2, "+", 38)] * 3, 611, queries=[2, 0, 1])
    c["links"] = [(0, 2, 3, 3, 0, 3, 8, 8, 8, 24), (1, 2, 2, 2, 2, 2, 1, 1, 1, 2)]
    return c


def long_links():
    """links of 65, 257 and 2050 pairs, the gaps 0, 1, 2 in turn: runs across a wave, a tile of 256 and a tile of 2048 places"""
    bridges, want = [], []
    for k, n in enumerate((65, 257, 2050)):
        bridges += [(40, 2 * k, "+", 20, 2 * k + 1, "+", 20 + i % 3) for i in range(n)]
        per_gap = [(n + 2 - g) // 3 for g in range(3)]
        want.append((2 * k, 2 * k + 1, 0, n, n, per_gap[0], 0, 0, 2, per_gap[1] + 2 * per_gap[2]))
    c = build([100] * 6, bridges, 612)
    c["links"] = want
    return c


def chain():
    """200 contigs, each linked to its neighbour by two reads, every second junction seen from the other strand"""
    bridges = []
    for i in range(199):
        b = (50, i, "+", 25, i + 1, "+", 25 + i % 7)
        bridges += [b, other_strand(b) if i % 2 else b]
    c = build([60] * 200, bridges, 613)
    c["links"] = [(i, i + 1, 0, 2, 1 if i % 2 else 2, 2, i % 7, i % 7, i % 7, 2 * (i % 7)) for i in range(199)]
    c["totals"] = [796, 0, 0, 398, 199]
    return c


DIRECTED = [("four_edges", four_edges), ("three_gaps", three_gaps), ("thresholds", thresholds), ("both_ends", both_ends), ("self_pair", self_pair), ("crowded", crowded),
            ("not_counted", not_counted), ("mode_tie", mode_tie), ("min_reads", min_reads), ("unlisted", unlisted), ("permuted", permuted), ("long_links", long_links),
            ("chain", chain)]


def random_set(seed):
    """3..12 contigs and some 1000 reads with 0..5 records each (a few with up to 24), two or three thousand records in all: over either
    end, over both, inside; both strands, clipped, some below the identity threshold, some reads extended; random parameters and a random
    query list"""
    rng = np.random.default_rng(8000 + seed)
    fast = pc.PyRng(8000 + seed)
    dense = seed % 3 == 0           # few contigs, one strand for most records: links of a hundred pairs and more
    nc = 3 if dense else fast.integers(3, 13)
    lens = [int(x) for x in rng.choice([30, 64, 150], size=nc)] + [int(x) for x in rng.integers(20, 81, size=fast.integers(500, 900) if dense else fast.integers(600, 1200))]
    seqs = [pc.rand_seq(rng, n) for n in lens]
    ids = [float(np.float32(x)) for x in (0.8, 0.9, 0.95, 1.0)]
    per = {q: ([pc.identity(seqs, q)] if fast.integers(0, 4) else []) for q in range(nc)}
    for t in range(nc, len(seqs)):
        T = lens[t]
        for _ in range(fast.integers(0, 25) if fast.integers(0, 40) == 0 else fast.integers(2 if dense else 0, 6)):
            q = fast.integers(0, nc)
            kind = fast.integers(0, 8)
            if kind == 0:           # anywhere
                per[q].append(pc.random_record(fast, lens[q], t, T, ids[fast.integers(0, 4)]))
                continue
            h = fast.integers(1, min(T - 1, 6) + 1) if fast.integers(0, 3) == 0 else fast.integers(1, T)
            u = lens[q] - T + h if kind & 1 else -h
            lo, hi = max(u, 0), min(u + T - 1, lens[q] - 1)
            left = fast.integers(0, 3) if hi - lo >= 4 else 0
            rev = fast.integers(0, 8 if dense else 2) == 1 and hi - lo - left >= 1
            per[q].append(placed(t, T, lens[q], u, rev, 0, ids[fast.integers(0, 4)], (left, 0)))
    k = fast.integers(1, nc + 1)
    c = pc.case(seqs, per, [int(x) for x in rng.permutation(nc)[:k]], ext=[1] * nc + [int(fast.integers(0, 8) == 0) for _ in range(len(seqs) - nc)],
                min_seq_id=float(rng.choice([0.0, 0.9])), skip=bool(fast.integers(0, 2)))
    c["par"] = dict(anchor=[1, 8, 16][fast.integers(0, 3)], overhang=[1, 3][fast.integers(0, 2)], max_ends=[2, 4, 16][fast.integers(0, 3)], min_reads=fast.integers(1, 4))
    c["contigs"] = nc
    return c


RANDOM_SEEDS = range(12)
