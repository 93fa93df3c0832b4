"""Directed and random inputs of cdm_pileup_junctions and of the host rules of contig_join, shared by the model's own tests (CPU), the
host unit's (CPU) and the device's (GPU): the smallest shapes at which the kernels and the rules can go wrong.  A device case is the dict
of tests/linkcases.py with "juncs" (a, b, info, gap) and, where written out by hand, "want": per junction (columns, matches, voters,
flags, fill_len, fill_min, fill_n) and "letters": the voted fills back to back.  The records are hand-built (tests/linkcases.py) and need
not agree with the letters: contig ends and read letters are chosen.  A host case (DECISIONS) is names, contigs, links, what the device
would say about the fills, and the decisions and paths written out by hand."""
import numpy as np

import join_model as jm
import linkcases as lc
import links_model as lm
import pileupcases as pc

PAIRS = ("++", "+-", "-+", "--")


def info_of(oa, ob):
    return (oa == "-") | (ob == "-") << 1


def build(contigs, bridges, queries=None, par=None, extra=None):
    """contigs: letters; a bridge (read letters, x, oX, hX, y, oY, hY): tests/linkcases.py's bridge with the read's letters chosen;
    extra: [(read letters, [(contig, lambda t: record)])] - reads with records of their own"""
    seqs, nc = list(contigs), len(contigs)
    per = {q: [pc.identity(seqs, q)] for q in range(nc)}
    for read, x, ox, hx, y, oy, hy in bridges:
        t = len(seqs)
        seqs.append(read)
        per[x].append(lc.tail_rec(t, len(read), len(contigs[x]), ox, hx))
        per[y].append(lc.head_rec(t, len(read), len(contigs[y]), oy, hy))
    for read, recs in extra or []:
        t = len(seqs)
        seqs.append(read)
        for q, make in recs:
            per[q].append(make(t))
    c = pc.case(seqs, per, list(range(nc)) if queries is None else queries)
    c["par"] = dict(anchor=16, overhang=1, max_ends=16)
    c["par"].update(par or {})
    c["contigs"] = nc
    return c


def bridge(read, x, ox, y, oy, gap, left=20):
    """`left` columns on x, then gap letters (or an overlap), the rest on y: between the contigs lie read[left : left + gap]"""
    return (read, x, ox, len(read) - left, y, oy, gap + left)


def seen_from_the_other_strand(b):
    read, x, ox, hx, y, oy, hy = b
    return (jm.rc(read), y, lc.FLIP[oy], hy, x, lc.FLIP[ox], hx)


def overlap_pair(rng, k, oa, ob, len_a=70, len_b=70, edit=None):
    """two contigs whose oriented forms overlap by k letters; edit(tail of oriented A, head of oriented B) -> the two with letters changed"""
    fa, fb = pc.rand_seq(rng, len_a), pc.rand_seq(rng, len_b)
    head = fa[len_a - k:]
    tail = head
    if edit:
        tail, head = edit(list(tail), list(head))
        tail, head = "".join(tail), "".join(head)
    fa, fb = fa[:len_a - k] + tail, head + fb[k:]
    return (jm.rc(fa) if oa == "-" else fa), (jm.rc(fb) if ob == "-" else fb)


def other(ch):
    return "ACGT"[("ACGT".index(ch) + 1) % 4]


def overlap_lengths():
    """every length around the 16-letter code word and the wave, in each of the four orientation pairs: all columns agree"""
    rng = np.random.default_rng(701)
    contigs, juncs, want = [], [], []
    for k in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65):
        for oa, ob in PAIRS:
            juncs.append((len(contigs), len(contigs) + 1, info_of(oa, ob), -k))
            contigs += overlap_pair(rng, k, oa, ob)
            want.append((k, k, 0, 0, 0, 0, 0))
    c = build(contigs, [])
    c.update(juncs=juncs, want=want, letters="")
    return c


def overlap_mismatches():
    """33 and 65 columns in each orientation pair: a mismatch in the first column only and in the last only; N on one side, on both sides,
    and N over an A (the N is stored as the code of A under its N bit)"""
    rng = np.random.default_rng(702)
    contigs, juncs, want = [], [], []

    def first(a, b):
        b[0] = other(a[0])
        return a, b

    def last(a, b):
        a[-1] = other(b[-1])
        return a, b

    def n_one(a, b):
        a[5] = "N"
        return a, b

    def n_both(a, b):
        a[7] = b[7] = "N"
        return a, b

    def n_over_a(a, b):
        a[9], b[9] = "N", "A"
        a[11], b[11] = "A", "N"
        return a, b

    for k in (33, 65):
        for oa, ob in PAIRS:
            for edit, miss in ((first, 1), (last, 1), (n_one, 1), (n_both, 1), (n_over_a, 2)):
                juncs.append((len(contigs), len(contigs) + 1, info_of(oa, ob), -k))
                contigs += overlap_pair(rng, k, oa, ob, edit=edit)
                want.append((k, k - miss, 0, 0, 0, 0, 0))
    c = build(contigs, [])
    c.update(juncs=juncs, want=want, letters="")
    return c


def contained():
    """contigs of 40 and 30 letters: an overlap of 30 is the whole of B, one of 31 is contained (no read can show either: a read that
    leaves A over its end has no end record on a B that ends inside A)"""
    rng = np.random.default_rng(703)
    a, b = overlap_pair(rng, 30, "+", "+", 40, 30)
    c = build([a, b], [])
    c.update(juncs=[(0, 1, 0, -30), (0, 1, 2, -31), (0, 1, 1, -40), (0, 1, 3, -4194303)],
             want=[(30, 30, 0, 0, 0, 0, 0), (0, 0, 0, jm.CONTAINED, 0, 0, 0), (0, 0, 0, jm.CONTAINED, 0, 0, 0), (0, 0, 0, jm.CONTAINED, 0, 0, 0)], letters="")
    return c


def fill_gaps():
    """gaps of 1, 63, 64 and 65 letters, each voted by a read, the same read seen from the other strand, and a read that differs in the
    last letter: forward and flipped pairs land on the same offsets"""
    rng = np.random.default_rng(704)
    contigs = [pc.rand_seq(rng, 60) for _ in range(8)]
    bridges, juncs, want, letters = [], [], [], ""
    for i, gap in enumerate((1, 63, 64, 65)):
        oa, ob = PAIRS[i]
        read = pc.rand_seq(rng, 20 + gap + 20)
        odd = read[:20 + gap - 1] + other(read[20 + gap - 1]) + read[20 + gap:]
        b = bridge(read, 2 * i, oa, 2 * i + 1, ob, gap)
        bridges += [b, seen_from_the_other_strand(b), bridge(odd, 2 * i, oa, 2 * i + 1, ob, gap)]
        juncs.append((2 * i, 2 * i + 1, info_of(oa, ob), gap))
        want.append((0, 0, 3, 0, gap, 2, 0))
        letters += read[20:20 + gap]
    c = build(contigs, bridges)
    c.update(juncs=juncs, want=want, letters=letters)
    return c


def fill_votes():
    """six offsets, four voters: a 2:2 tie of C and G (C), N alone (N), A beside N (A), a 2:2 tie of A and T (A), four G, a 2:2 tie of A and C
    (A).  A fifth read of the same edge has 7 letters between the contigs and a sixth is crowded (max_ends 2, three end records): neither votes"""
    rng = np.random.default_rng(705)
    contigs = [pc.rand_seq(rng, 60) for _ in range(3)]
    left, right = pc.rand_seq(rng, 20), pc.rand_seq(rng, 20)
    bridges = [bridge(left + f + right, 0, "+", 1, "+", 6) for f in ("CNATGA", "CNATGC", "GNNAGC", "GNNAGA")]
    bridges.append(bridge(left + "TTTTTTT" + right, 0, "+", 1, "+", 7))
    # the crowded read: the two records of a bridge with 6 letters between the contigs, and a tail record on contig 2
    crowd = (left + "TTTTTT" + right, [(0, lambda t: lc.tail_rec(t, 46, 60, "+", 26)), (1, lambda t: lc.head_rec(t, 46, 60, "+", 26)), (2, lambda t: lc.tail_rec(t, 46, 60, "+", 10))])
    c = build(contigs, bridges, par=dict(max_ends=2), extra=[crowd])
    c.update(juncs=[(0, 1, 0, 6)], want=[(0, 0, 4, 0, 6, 0, 1)], letters="CNAAGA", counts=[[0, 2, 2, 0, 0], [0, 0, 0, 0, 4], [2, 0, 0, 0, 2], [2, 0, 0, 2, 0], [0, 0, 4, 0, 0], [2, 2, 0, 0, 0]])
    return c


def junction_lists():
    """three edges with pairs - a fill of 4 (two reads), an overlap of 5 (three reads), two contigs that abut (two reads) - and one without
    any pair; `subsets` are junction lists of their own"""
    rng = np.random.default_rng(706)
    contigs = list(overlap_pair(rng, 5, "+", "-")) + [pc.rand_seq(rng, 60) for _ in range(4)]
    reads = [pc.rand_seq(rng, 50) for _ in range(7)]
    bridges = [bridge(reads[i], 0, "+", 1, "-", -5) for i in range(3)] + [bridge(reads[3][:20] + "ACGT" + reads[3][24:], 2, "-", 3, "+", 4) for _ in range(2)]
    bridges += [bridge(reads[5 + i], 3, "+", 4, "+", 0) for i in range(2)]
    c = build(contigs, bridges)
    c.update(juncs=[(0, 1, 2, -5), (2, 3, 1, 4), (3, 4, 0, 0), (4, 5, 0, 3)], want=[(5, 5, 3, 0, 0, 0, 0), (0, 0, 2, 0, 4, 2, 0), (0, 0, 2, 0, 0, 0, 0), (0, 0, 0, 0, 3, 0, 3)], letters="ACGTNNN",
             subsets=[[0], [1], [3], [1, 3], [0, 2]])
    return c


def permuted_list():
    """the list [2, 0, 1]: the edge (contig 1, +) -> (contig 2, +) goes from list index 2 to 0 and is (0, -) -> (2, -): its letters are the
    reverse complement of what the read shows"""
    rng = np.random.default_rng(707)
    contigs = [pc.rand_seq(rng, 60) for _ in range(3)]
    read = pc.rand_seq(rng, 20) + "AACCG" + pc.rand_seq(rng, 20)
    c = build(contigs, [bridge(read, 1, "+", 2, "+", 5)] * 2, queries=[2, 0, 1])
    c.update(juncs=[(0, 2, 3, 5)], want=[(0, 0, 2, 0, 5, 2, 0)], letters="CGGTT")
    return c


def many_voters():
    """one junction with 2050 voters of three letters: every third read says T at the second offset"""
    rng = np.random.default_rng(708)
    contigs = [pc.rand_seq(rng, 60) for _ in range(2)]
    left, right = pc.rand_seq(rng, 20), pc.rand_seq(rng, 20)
    c = build(contigs, [bridge(left + ("GTA" if i % 3 == 0 else "GCA") + right, 0, "+", 1, "+", 3) for i in range(2050)])
    c.update(juncs=[(0, 1, 0, 3)], want=[(0, 0, 2050, 0, 3, 2050 - 684, 0)], letters="GCA")
    return c


def chain():
    """tests/linkcases.py's chain of 200 contigs: 199 junctions with gaps 0..6, every second seen from the other strand"""
    c = lc.chain()
    c["par"] = dict(anchor=16, overhang=1, max_ends=16)
    c["juncs"] = [(i, i + 1, 0, i % 7) for i in range(199)]
    return c


DIRECTED = [("overlap_lengths", overlap_lengths), ("overlap_mismatches", overlap_mismatches), ("contained", contained), ("fill_gaps", fill_gaps), ("fill_votes", fill_votes),
            ("junction_lists", junction_lists), ("permuted_list", permuted_list), ("many_voters", many_voters), ("chain", chain)]


def juncs_array(juncs):
    return np.array(juncs, jm.JUNCTION_DTYPE) if len(juncs) else np.empty(0, jm.JUNCTION_DTYPE)


def link_params(c):
    return {k: c["par"][k] for k in ("anchor", "overhang", "max_ends")}


def model_links(c, min_reads=1):
    return lm.links(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"], min_reads=min_reads, min_seq_id=c["min_seq_id"], skip=c["skip"], **link_params(c))[2]


def model(c, juncs=None):
    return jm.junctions(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"], juncs_array(c["juncs"] if juncs is None else juncs), min_seq_id=c["min_seq_id"], skip=c["skip"], **link_params(c))


def random_set(seed):
    """tests/linkcases.py's random set (two to four thousand records) with N letters in some reads; the junctions are every link with its
    most frequent gap - for every third link its smallest gap instead"""
    c = lc.random_set(seed)
    rng = np.random.default_rng(9000 + seed)
    for t in range(c["contigs"], len(c["seqs"])):
        if rng.integers(0, 4) == 0:
            s = list(c["seqs"][t])
            for p in rng.integers(0, len(s), size=3):
                s[p] = "N"
            c["seqs"][t] = "".join(s)
    c["par"] = link_params(c)
    links = model_links(c)
    c["juncs"] = [(int(k["a"]), int(k["b"]), int(k["info"]), int(k["gap_min"] if i % 3 == 2 else k["gap_mode"])) for i, k in enumerate(links)]
    return c


RANDOM_SEEDS = range(12)


# ------------------------------------------------------------------------------------------------------ the host rules
def link(a, oa, b, ob, reads, gap, mode_reads=None):
    return (a, b, info_of(oa, ob), reads, reads, reads if mode_reads is None else mode_reads, gap, gap, gap, 0, gap * reads)


def host_case(contigs, links, dec, paths, fills=None, names=None, **par):
    """fills: {link index: the fill letters the device would vote}; paths: [[(contig, o, trim, fill)]] written out by hand"""
    return dict(names=names or ["c%d" % i for i in range(len(contigs))], contigs=list(contigs), links=np.array(links, lm.LINK_DTYPE), fills=fills or {}, dec=dec, paths=paths, par=par)


def synthetic_junctions(c):
    """what cdm_pileup_junctions would say about the case's junctions: the overlaps from the contigs' letters, the fills as the case states them"""
    def run(juncs):
        n = len(c["contigs"])
        res, _, _ = jm.junctions(c["contigs"], [0] * n, np.zeros(n + 1, np.uint64), np.empty(0, lm_aln_dtype()), list(range(n)), juncs)
        by_edge = {(int(k["a"]), int(k["b"]), int(k["info"])): c["fills"].get(i, "") for i, k in enumerate(c["links"])}
        letters = ""
        for j, r in zip(juncs, res):
            f = by_edge[(int(j["a"]), int(j["b"]), int(j["info"]))] if int(j["gap"]) > 0 else ""
            assert len(f) == int(r["fill_len"])
            r["fill_off"], r["fill_min"], r["fill_n"], r["voters"] = len(letters), (2 if f else 0), f.count("N"), 2
            letters += f
        return res, np.frombuffer(letters.encode(), np.uint8).copy()
    return run


def lm_aln_dtype():
    import pileup_model
    return pileup_model.ALN_DTYPE


def decisions():
    rng = np.random.default_rng(720)
    r = lambda n: pc.rand_seq(rng, n)
    out = {}
    # A: two links at the right end of c0; the third link touches c2's right end and c3's left end, which are its own
    out["A"] = host_case([r(50), r(50), r(50), r(50)], [link(0, "+", 1, "+", 5, 2), link(0, "+", 2, "+", 4, 2), link(2, "+", 3, "+", 4, 0)], "AAJ",
                         [[(2, "+", 0, ""), (3, "+", 0, "")]], fills={0: "AC", 1: "GT"})
    out["W"] = host_case([r(50), r(50)], [link(0, "+", 1, "+", 5, 2, mode_reads=1)], "W", [])
    out["C"] = host_case([r(40), r(60)], [link(0, "+", 1, "+", 5, -41)], "C", [])
    a, b = overlap_pair(rng, 10, "+", "+", 50, 50, edit=lambda x, y: (x, [other(ch) if i < 2 else ch for i, ch in enumerate(y)]))
    out["X"] = host_case([a, b], [link(0, "+", 1, "+", 5, -10)], "X", [])                       # 8 of 10 columns: 800 < 900
    out["X_at_80"] = host_case([a, b], [link(0, "+", 1, "+", 5, -10)], "J", [[(0, "+", 0, ""), (1, "+", 10, "")]], overlap_percent=80)
    # S: c1 of 20 letters overlaps c0 by 15 and c2 by 10; the link with 3 reads goes.  The letters agree: c0's last 15 are c1's first 15,
    # c1's last 10 are c2's first 10
    c1 = r(20)
    out["S"] = host_case([r(30) + c1[:15], c1, c1[10:] + r(30)], [link(0, "+", 1, "+", 5, -15), link(1, "+", 2, "+", 3, -10)], "JS", [[(0, "+", 0, ""), (1, "+", 15, "")]])
    out["S_equal"] = host_case([r(30) + c1[:15], c1, c1[10:] + r(30)], [link(0, "+", 1, "+", 3, -15), link(1, "+", 2, "+", 3, -10)], "JS", [[(0, "+", 0, ""), (1, "+", 15, "")]])
    # O: a circle of three; the link at c0's left end, (0, -) -> (2, -), is the one that is opened
    out["O"] = host_case([r(40), r(40), r(40)], [link(0, "+", 1, "+", 4, 1), link(0, "-", 2, "-", 4, 2), link(1, "+", 2, "+", 4, 0)], "JOJ",
                         [[(0, "+", 0, ""), (1, "+", 0, "G"), (2, "+", 0, "")]], fills={0: "G", 1: "TT"})
    # J: c1 starts in -, its link to c0 is walked against the canonical direction (the fill's reverse complement), then c0's other link as it stands
    out["J"] = host_case(["acgtRYKMBVDHSWNxACGT" + r(30), r(40), r(40)], [link(0, "+", 1, "+", 4, 3), link(0, "-", 2, "+", 4, 2)], "JJ",
                         [[(1, "-", 0, ""), (0, "-", 0, "TGG"), (2, "+", 0, "AN")]], fills={0: "CCA", 1: "AN"})
    # a - start contig on a canonical walk, with an overlap in front of the second contig
    a, b = overlap_pair(rng, 6, "-", "-", 40, 40)
    out["minus_start"] = host_case([a, b, r(30)], [link(0, "-", 1, "-", 4, -6)], "J", [[(0, "-", 0, ""), (1, "-", 6, "")]])
    return out


DECISIONS = decisions()
