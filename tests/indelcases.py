"""Inputs of cdm_pileup_indels, shared by the model's own tests (CPU) and the device's (GPU): hand-built gapped records with the reads
they lie on, random record sets, one record per refusal, and the planted-indel corpus.  A case is a dict: seqs (ASCII), ext, off / rec
(the ungapped set, CSR by query), queries, grecs (GAP_DTYPE) and gops (uint32), in the layout cdm_pileup_gapped returns them."""
import numpy as np

import gapped_model as gm
import indels_model as im
import map_model as mm
import pileupcases as pc
from pileup_model import csr, unorient

M, I, D = gm.OP_M, gm.OP_I, gm.OP_D


def revcomp(s):
    return s.translate(mm.COMPLEMENT)[::-1]


class Builder:
    """sequences 0 .. n_contigs - 1 are the contigs (wasExtended 1); every record brings a read of its own behind them"""

    def __init__(self, rng, contigs):
        self.rng, self.seqs, self.ext = rng, list(contigs), [1] * len(contigs)
        self.per = {q: [pc.identity(self.seqs, q)] for q in range(len(contigs))}
        self.rows = []

    def read(self, letters, rev):
        self.seqs.append(revcomp(letters) if rev else letters)
        self.ext.append(0)
        return len(self.seqs) - 1

    def plain(self, q, qs, qe, rev=False, target=None, ds=0):
        """an ungapped record of query q over qs..qe; target: an existing sequence instead of a new read"""
        n = qe - qs + 1
        t = self.read(pc.rand_seq(self.rng, n), rev) if target is None else target
        self.per[q].append(unorient(t, qs, qe, ds, ds + n - 1, rev and n > 1, len(self.seqs[t])))

    def gapped(self, k, pos, ops, rev=False, inserted=None, tstart=0, tail=0):
        """a gapped record of listed query k at pos with the operations [(op, length)]; inserted: the letters of its insertions, in the
        query's orientation, one str per I (random where None); tstart / tail: clipped letters in front and behind"""
        letters, given = [pc.rand_seq(self.rng, tstart)], list(inserted or [])
        for op, g in ops:
            if op == I:
                letters.append(given.pop(0) if given else pc.rand_seq(self.rng, g))
                assert len(letters[-1]) == g
            elif op == M:
                letters.append(pc.rand_seq(self.rng, g))
        letters.append(pc.rand_seq(self.rng, tail))
        letters = "".join(letters)
        t = self.read(letters, rev)
        span, columns = sum(g for op, g in ops if op != I), sum(g for op, g in ops if op != D)
        self.rows.append((k, pos, len(self.rows), (k, t, pos, span, tstart, len(letters), columns, 0, gm.REVERSE if rev else 0, len(ops), 0, 0), [g << 2 | op for op, g in ops]))

    def case(self, queries, **kw):
        """the records in the order of cdm_pileup_gapped: listed query, pos, then as they were added"""
        off, rec = csr(len(self.seqs), self.per)
        grecs, gops = np.zeros(len(self.rows), gm.GAP_DTYPE), []
        for i, (_, _, _, fields, words) in enumerate(sorted(self.rows, key=lambda r: r[:3])):
            grecs[i] = fields + (len(gops), 0)
            gops += words
        return dict(seqs=self.seqs, ext=self.ext, off=off, rec=rec, queries=list(queries), grecs=grecs, gops=np.array(gops, np.uint32), **kw)


def indel(a, op, g, b):
    return [(M, a), (op, g), (M, b)]


# ------------------------------------------------------------------------------------------------ the directed case
DIRECTED_PAR = dict(min_depth=3, min_count=2, min_percent=20, skip=True)
# (p, kind) -> (g, count, cross, others, flags) of the places of contig 0 the case is built for, worked out by hand
S, SM = im.CALLED | im.SUPPORTED, im.CALLED | im.SUPPORTED | im.MAJOR
DIRECTED_PLACES = {
    (20, im.INS): (1, 3, 3, 0, SM), (40, im.DEL): (1, 3, 3, 0, SM),
    (60, im.INS): (8, 2, 4, 0, S), (60, im.DEL): (8, 2, 4, 0, S),          # an I and a D at one position; 2 * count == cross: not major
    (100, im.INS): (62, 4, 4, 0, SM), (200, im.DEL): (62, 3, 3, 0, SM),
    (300, im.INS): (2, 2, 4, 2, S),                                         # two lengths with equal counts: the smaller
    (330, im.DEL): (1, 2, 10, 0, S),                                        # exactly min_count and exactly min_percent of cross
    (350, im.DEL): (1, 2, 11, 0, im.CALLED),                                # below the percentage
    (370, im.INS): (1, 1, 5, 0, im.CALLED),                                 # below the count
    (385, im.DEL): (1, 2, 2, 0, 0),                                         # below the depth
    (400, im.INS): (1, 3, 3, 0, SM),                                        # events at p = pos + 1 and at p = pos + span - 1
    (430, im.DEL): (1, 65, 65, 0, SM), (460, im.INS): (1, 300, 300, 0, SM)}
DIRECTED_LETTERS = {20: "C", 60: "ACGTNACG", 300: "AC", 400: "G", 460: "T"}       # and (100, INS) below


def directed():
    """listed: contig 0 of 520 letters, contig 2 of 60 and contig 3 of 30; contig 1 is not listed and lies on contig 0 as an extended
    target, which skip_extended_targets leaves out"""
    rng = np.random.default_rng(620)
    b = Builder(rng, [pc.rand_seq(rng, n, 0.01) for n in (520, 100, 60, 30)])
    for _ in range(3):
        b.gapped(0, 10, indel(10, I, 1, 10), inserted=["C"])
        b.gapped(0, 30, indel(10, D, 1, 10))
    # p = 60: two insertions of 8 (the second reverse, its letters on the read's stored positions 10..17, across a code word; an N of its
    # own at offset 4, where the first has one too) and two deletions of 8
    b.gapped(0, 50, indel(10, I, 8, 10), inserted=["ACGTNACG"])
    b.gapped(0, 50, indel(10, I, 8, 10), rev=True, inserted=["ACGTNACG"])
    b.gapped(0, 50, indel(10, D, 8, 10))
    b.gapped(0, 50, indel(10, D, 8, 10), rev=True)
    # p = 100: four insertions of 62, two of them reverse: ties at the offsets 0 (A A C C -> A), 1 (G T T G -> G) and 3 (N N T C -> C), N
    # in all four at offset 2
    common = pc.rand_seq(rng, 58)
    for k, head in enumerate(("AGNN", "ATNN", "CTNT", "CGNC")):
        b.gapped(0, 88, indel(12, I, 62, 9), rev=k % 2 == 1, inserted=[head + common], tstart=k, tail=3 - k)
    for k in range(3):
        b.gapped(0, 190, indel(10, D, 62, 10), rev=k == 1)
    for g in (2, 3, 3, 2):
        b.gapped(0, 290, indel(10, I, g, 10), inserted=["ACG"[:g]])
    # p = 330, 350, 370, 385: the thresholds; ungapped records crossing, ending at (qe = p - 1) and starting at (qs = p) the place
    for _ in range(2):
        b.gapped(0, 325, indel(5, D, 1, 5))
        b.gapped(0, 345, indel(5, D, 1, 5))
        b.gapped(0, 380, indel(5, D, 1, 5))
    b.gapped(0, 365, indel(5, I, 1, 5))
    for k in range(8):
        b.plain(0, 329 - k, 330 + k, rev=k % 2 == 1)         # qs < 330 <= qe, down to the two-letter record 329..330
    b.plain(0, 320, 329)
    b.plain(0, 330, 339)
    b.plain(0, 320, 340, target=1, ds=7)                        # the extended target: not counted
    for k in range(9):
        b.plain(0, 346 - k, 352)
    for k in range(4):
        b.plain(0, 366, 372 + k)
    b.gapped(0, 399, indel(1, I, 1, 10), inserted=["G"])
    b.gapped(0, 399, indel(1, I, 1, 10), inserted=["G"], rev=True)
    b.gapped(0, 390, indel(10, I, 1, 1), inserted=["T"])
    for k in range(65):         # past a wave
        b.gapped(0, 420, indel(10, D, 1, 10), rev=k % 3 == 0)
    for k in range(300):        # past a block: 120 T, 100 A, 80 G
        b.gapped(0, 450, indel(10, I, 1, 10), rev=k % 2 == 1, inserted=["T" if k < 120 else "A" if k < 220 else "G"])
    # the two small contigs: listed queries 1 and 2
    for _ in range(3):
        b.gapped(1, 22, indel(8, I, 1, 8), rev=True, inserted=["A"])
    for _ in range(2):
        b.gapped(1, 40, indel(5, D, 2, 5))
    b.plain(2, 1, 40)
    b.plain(3, 3, 20)
    b.plain(1, 0, 50)           # a record of the contig that is not listed
    return b.case([0, 2, 3], common=common)


# ------------------------------------------------------------------------------------------------ random record sets
def random_case(seed):
    """one or two listed contigs of 30..70 letters, a few ungapped records and up to a dozen gapped records a contig with one to three
    gaps each at positions drawn from a few, so that places collect several events and several lengths"""
    rng = np.random.default_rng(seed)
    nq = int(rng.integers(1, 3))
    b = Builder(rng, [pc.rand_seq(rng, int(rng.integers(30, 71)), 0.02) for _ in range(nq)])
    for k in range(nq):
        L = len(b.seqs[k])
        for _ in range(int(rng.integers(0, 6))):
            qs = int(rng.integers(0, L - 1))
            b.plain(k, qs, int(rng.integers(qs, L)), rev=bool(rng.integers(0, 2)))
        for _ in range(int(rng.integers(0, 13))):
            pos = int(rng.integers(0, 6))
            ops = []
            for j in range(int(rng.integers(1, 4))):
                ops += [(M, int(rng.choice([1, 4, 7]))), (int(rng.choice([I, D])), int(rng.choice([1, 1, 2, 5])))]
            ops.append((M, int(rng.integers(1, 5))))
            if pos + sum(g for op, g in ops if op != I) > L:
                continue
            letters = [pc.rand_seq(rng, g, 0.2) if rng.integers(0, 2) else "ACGTA"[:g] for op, g in ops if op == I]
            b.gapped(k, pos, ops, rev=bool(rng.integers(0, 2)), inserted=letters, tstart=int(rng.integers(0, 3)), tail=int(rng.integers(0, 3)))
    par = im.Params(int(rng.integers(1, 5)), int(rng.integers(1, 4)), int(rng.choice([0, 20, 50, 100])), 0.0, True)
    order = list(range(nq))[::-1] if seed % 3 == 0 else list(range(nq))
    if order != list(range(nq)):        # the listed order turned round: the records' query is the index into the list
        for i in range(len(b.rows)):
            k, pos, n, fields, words = b.rows[i]
            b.rows[i] = (nq - 1 - k, pos, n, (nq - 1 - k,) + fields[1:], words)
    return b.case(order), par


# ------------------------------------------------------------------------------------------------ one record per refusal
def refusals():
    """-> (seqs, [(name, queries, records [(fields without ops)], operation words, the message's words)]); sequence 0: a contig of 40
    letters, 1: a read of 30, 2: a read of 100"""
    rng = np.random.default_rng(621)
    seqs = [pc.rand_seq(rng, 40), pc.rand_seq(rng, 30), pc.rand_seq(rng, 100)]
    good = dict(query=0, target=1, pos=5, span=20, tstart=2, tlen=30, columns=22, n_ops=3, ops=0)
    words = [10 << 2 | M, 2 << 2 | I, 10 << 2 | M]

    def one(name, message, words=words, second=None, **change):
        recs = [dict(good, **change)] + ([dict(good, **second)] if second else [])
        return name, [0], recs, list(words), message

    return seqs, [
        one("query", "record 0: its query is not an index", query=1),
        one("target", "record 0: its target is not a sequence", target=99),
        one("tlen", "record 0: tlen is not the length", tlen=29),
        one("order", "record 1: the records do not ascend", second=dict(pos=4)),
        one("pool", "record 0: its operations are not words of the pool", ops=1),
        one("no_ops", "record 0: its operations are not words of the pool", n_ops=0),
        one("code", "record 0: an operation that is not M, I or D", words=[10 << 2 | M, 2 << 2 | 3, 10 << 2 | M]),
        one("empty_op", "record 0: an operation that is not M, I or D", words=[10 << 2 | M, 0 << 2 | I, 10 << 2 | M]),
        one("first", "record 0: its first or last operation is not M", words=[2 << 2 | I, 20 << 2 | M], n_ops=2),
        one("last", "record 0: its first or last operation is not M", words=[18 << 2 | M, 2 << 2 | D], n_ops=2, columns=18),
        one("neighbours", "record 0: two neighbouring operations of one code", words=[5 << 2 | M, 5 << 2 | M, 2 << 2 | I, 10 << 2 | M], n_ops=4),
        one("span", "record 0: its operations do not sum", span=21),
        one("columns", "record 0: its operations do not sum", columns=21),
        one("beyond_query", "record 0: pos \\+ span lies beyond its query", pos=21),
        one("beyond_target", "record 0: tstart \\+ columns lies beyond its target", tstart=9),
        one("long_gap", "record 0: an insertion or deletion of more than 62", words=[5 << 2 | M, 63 << 2 | I, 5 << 2 | M], target=2, tlen=100, span=10, columns=73)]


def refusal_arrays(recs, words):
    grecs = np.zeros(len(recs), gm.GAP_DTYPE)
    for i, r in enumerate(recs):
        for name, v in r.items():
            grecs[i][name] = v
    return grecs, np.array(words, np.uint32)


# ------------------------------------------------------------------------------------------------ the planted corpus
PLANTS = (("missing", 150, 1), ("extra", 290, 2), ("homopolymer", 430, 1), ("missing", 560, 3))


def planted_genome(seed, length=700):
    """-> (genome, contig, ends): the genome with a five-letter homopolymer at 430, the contig with the four planted errors - genome
    letter 150 missing, two letters too many in front of 290, the homopolymer one letter short, 560..562 missing - and, per plant, the
    genome stretch [from, to) that the contig lacks (from == to for the extra letters)"""
    rng = np.random.default_rng(seed)
    g = list(pc.rand_seq(rng, length))
    g[430:435] = "AAAAA"
    g[429], g[435] = "C", "G"
    genome = "".join(g)
    contig, at, ends = [], 0, []
    for kind, p, n in PLANTS:
        contig.append(genome[at:p])
        if kind == "extra":
            contig.append("GT"[:n])
            at = p
            ends.append((p, p))
        else:
            at = p + n
            ends.append((p, p + n))
    contig.append(genome[at:])
    return genome, "".join(contig), ends


def planted_reads(genome, read_len=80, step=3, strands="forward", first=0):
    """error-free reads every `step` positions -> [(genome start, stored letters, reverse)]"""
    out = []
    for i, s in enumerate(range(first, len(genome) - read_len + 1, step)):
        rev = strands == "reverse" or (strands == "alternate" and i % 2 == 1)
        r = genome[s:s + read_len]
        out.append((s, revcomp(r) if rev else r, rev))
    return out


def planted_case(seed=7, strands="forward", margin=20):
    """the experiment on the CPU with the model's own alignment: a read without a plant lies ungapped on the contig, a read with a plant
    within `margin` letters of an end keeps the ungapped record of its longer side, clipped at the plant, and every other read goes
    through gapped_model.align_pair on its left side's diagonal.  -> (case, genome, rescued)"""
    genome, contig, ends = planted_genome(seed)
    to_contig, shift = {}, 0           # genome position -> contig position, for the letters the contig has
    for gi in range(len(genome)):
        for (kind, p, n), (lo, hi) in zip(PLANTS, ends):
            if gi == p and kind == "extra":
                shift += n
        if any(lo <= gi < hi for lo, hi in ends):
            shift -= 1
            continue
        to_contig[gi] = gi + shift
    rng = np.random.default_rng(seed + 1)
    b = Builder(rng, [contig])
    Q, p, rescued = mm.codes(contig), gm.Params(0.0, True), 0
    for s, stored, rev in planted_reads(genome, strands=strands):
        n = len(stored)
        hit = [(lo, hi) for lo, hi in ends if ((lo < s + n and hi > s) if lo < hi else (s < lo < s + n))]      # (extra letters: between two letters of the read)
        t = b.read(revcomp(stored) if rev else stored, rev)
        assert b.seqs[t] == stored
        if not hit:
            b.per[0].append(unorient(t, to_contig[s], to_contig[s + n - 1], 0, n - 1, rev, n))
            continue
        (lo, hi), = hit
        x, x_end = max(lo - s, 0), min(hi - s, n)       # the read letters [x, x_end) have no contig letter (none: x == x_end)
        if min(x, n - x_end) < margin:
            if x >= n - x_end:
                b.per[0].append(unorient(t, to_contig[s], to_contig[s + x - 1], 0, x - 1, rev, n))
            else:
                b.per[0].append(unorient(t, to_contig[s + x_end], to_contig[s + n - 1], x_end, n - 1, rev, n))
            continue
        R = gm.oriented_codes(stored, rev)
        a = gm.align_pair(Q, R, to_contig[s], p.band, p)
        d = gm.describe(Q, R, a)
        if not gm.accepted(d, p):
            continue
        rescued += 1
        b.rows.append((0, d["pos"], len(b.rows), (0, t, d["pos"], d["span"], d["tstart"], n, d["columns"], 0, gm.REVERSE if rev else 0, len(d["ops"]), 0, d["score"]), d["ops"]))
    return b.case([0]), genome, rescued
