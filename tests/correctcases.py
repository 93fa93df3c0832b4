"""Hand-built alignment sets for ancient_correction (src/assembler/correction.cpp): every gate, counter width, staging bound
and damage-class step of csrc/correct.hip met on purpose instead of by what kmermatcher -> rescorediagonal happen to emit.
Deterministic (RandomState), no GPU.

A case set is one sequence DB (sequences, keys = 0..n-1, ext flags) plus one alignment DB as text records, built from independent
groups: one query with its targets.  Each group carries a name, the query's key, the number of records of the query and whether
the reference is meant to change a base of it ("calls": True / False / None = whatever comes out).

The domain: one record per (query, target) pair.  The reference takes a target's orientation from the query's LAST record with
that target (useReverse) while the device takes it per record; two records of one pair are outside the stage's domain
and no group has them.  Every sequence also has its self record (except where a sparse group says otherwise), records are
ungapped and in range (cdm_alns_upload checks both).

Where a base is meant to be called the substitution is damage-like - the query holds T where the targets hold C, or A where they
hold G: transversions are never corrected for reads (the other base costs log(0.001) per record).  By default half of a query's
C / G columns are damaged that way, so that nearly every target letter decides an output letter.

Groups dropped because the reference's binary ended on a signal for them: none.
"""
import numpy as np

ALPHA = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGTacgtN", b"TGCAtgcaN")
_DAMAGE = {ord("C"): ord("T"), ord("G"): ord("A")}
_RYFLIP = bytes.maketrans(b"ACGT", b"CATG")          # purine <-> pyrimidine


def revcomp(s):
    return s.translate(_COMP)[::-1]


def rnd(rs, n):
    return bytes(bytearray(ALPHA[rs.randint(0, 4, size=n)]))


class CaseSet:
    def __init__(self):
        self.seqs, self.ext, self.recs, self.groups = [], [], {}, []

    @property
    def keys(self):
        return list(range(len(self.seqs)))

    def seq(self, s, ext=0, self_record=True):
        k = len(self.seqs)
        self.seqs.append(bytes(s))
        self.ext.append(int(ext))
        self.recs[k] = []
        if self_record:
            self.rec(k, k, 0, len(s) - 1, 0, len(s) - 1)
        return k

    def rec(self, q, t, qs, qe, ds, de, seq_id="1.00", at=None):
        """one alignment record as Matcher::resultToBuffer writes it; reverse: qs > qe, ds <= de on the target as stored"""
        n = abs(qe - qs) + 1
        assert ds <= de and de - ds + 1 == n and max(qs, qe) < len(self.seqs[q]) and de < len(self.seqs[t]) and min(qs, qe, ds) >= 0
        assert all(int(l.split("\t")[0]) != t for l in self.recs[q]), "one record per (query, target) pair"
        line = "%d\t%d\t%s\t1.000E-20\t%d\t%d\t%d\t%d\t%d\t%d" % (t, 2 * n, seq_id, qs, qe, len(self.seqs[q]), ds, de, len(self.seqs[t]))
        self.recs[q].insert(len(self.recs[q]) if at is None else at, line)

    def group(self, name, q, calls):
        self.groups.append({"name": name, "query": q, "calls": calls})

    def finish(self):
        for g in self.groups:
            g["records"] = len(self.recs[g["query"]])
        return self

    def seq_keyed(self):
        return {k: (s + b"\n", e) for k, (s, e) in enumerate(zip(self.seqs, self.ext))}

    def aln_keyed(self):
        return {k: (("\n".join(v) + "\n").encode() if v else b"", 0) for k, v in self.recs.items()}


def damaged(rs, core, rate=0.5, force=(), spare=()):
    """the query of a true sequence: C -> T, G -> A at `rate`, always at the columns `force`, never at `spare`"""
    b = bytearray(core)
    hit = rs.random_sample(len(b)) < rate
    for i, c in enumerate(core):
        if c in _DAMAGE and i not in spare and (hit[i] or i in force):
            b[i] = _DAMAGE[c]
    return bytes(b)


def probe_cols(qlen):
    return sorted({0, 4, 5, qlen // 2, qlen - 6, qlen - 5, qlen - 1})


def core_with_probes(rs, qlen, probes=None, letters=b"CG"):
    """a true sequence that holds C or G (a damage site) at every probed column"""
    b = bytearray(rnd(rs, qlen))
    for i, p in enumerate(probe_cols(qlen) if probes is None else probes):
        b[p] = letters[i % len(letters)]
    return bytes(b)


def target(S, rs, q, core, qa, qb, ds, tlen, rev, edit=None, ext=0, seq_id="1.00", at=None, stored_edit=None):
    """a target whose oriented letters ds .. ds + (qb - qa) are core[qa .. qb], random flanks around them; stored reverse
    complemented when rev.  edit(bytearray of the aligned letters) changes them before the flanks go on."""
    n = qb - qa + 1
    mid = bytearray(core[qa: qb + 1])
    if edit:
        edit(mid)
    w = rnd(rs, ds) + bytes(mid) + rnd(rs, tlen - ds - n)
    assert len(w) == tlen
    stored = bytearray(revcomp(w) if rev else w)
    if stored_edit:
        stored_edit(stored)
    t = S.seq(bytes(stored), ext)
    if rev:
        S.rec(q, t, qb, qa, tlen - 1 - (ds + n - 1), tlen - 1 - ds, seq_id, at)
    else:
        S.rec(q, t, qa, qb, ds, ds + n - 1, seq_id, at)
    return t


def _rev_of(orient, i):
    return {"f": False, "r": True, "m": i % 2 == 1}[orient]


def pile(S, rs, name, qlen, ntargets, orient="f", tlen=100, calls=True, qext=0, core=None, query=None, seq_id="1.00",
         self_at=0, edit=None, alen=None):
    """query + self record + ntargets inside records: the query (or, with alen, alternately its first and its last alen columns)
    somewhere within each target"""
    core = core_with_probes(rs, qlen) if core is None else core
    query = damaged(rs, core, force=probe_cols(qlen)) if query is None else query
    q = S.seq(query, qext)
    for i in range(ntargets):
        tl = tlen[i % len(tlen)] if isinstance(tlen, (tuple, list)) else tlen
        n = qlen if alen is None else alen
        qa = 0 if i % 2 == 0 else qlen - n
        ds = int(rs.randint(1, tl - n)) if tl > n + 1 else 0
        target(S, rs, q, core, qa, qa + n - 1, ds, tl, _rev_of(orient, i // 2 if alen else i), edit=edit, seq_id=seq_id)
    if self_at:
        S.recs[q].insert(min(self_at, len(S.recs[q]) - 1), S.recs[q].pop(0))
    S.group(name, q, calls)
    return q


def ry_edit(k):
    """k purine <-> pyrimidine substitutions in the aligned letters, away from the ends"""
    def f(mid):
        step = max(1, (len(mid) - 16) // max(k, 1))
        for j in range(k):
            p = 8 + j * step
            mid[p] = bytes([mid[p]]).translate(_RYFLIP)[0]
    return f


def main_set(seed=17):
    rs = np.random.RandomState(seed)
    S = CaseSet()

    # ---- record counts (self included) around the three instance boundaries, all forward / all reverse / mixed
    for n in (1, 2, 15, 16, 64, 65, 66):
        for o in "frm":
            # (64 and more full-length records would put avCov past 50: those cover half of a 64-letter query each)
            pile(S, rs, "count_%d_%s" % (n, o), 40 if n < 45 else 64, n - 1, o, calls=n >= 3, self_at=0 if o != "m" else n // 2, alen=None if n < 45 else 32)
    # two records, extended query: no 2/5 rule, whatever the likelihoods give
    pile(S, rs, "count_2_ext", 40, 1, "f", qext=1, calls=None)

    # ---- counter saturation: every non-self record reverse with the same base in the same class: 0xF|0xF in a byte at 15 records,
    # 0x40|0x40 in a half word and 64 in a cov4 byte at 64 (65 records with the self one belong to the general kernel, so 64
    # reverse records need a query whose self record is absent).  The query is the prefix of every oriented target: right-only
    # records, which avCov >= 50 does not turn away
    for n, name in ((15, "sat_15"), (16, "sat_16"), (64, "sat_64"), (65, "sat_65")):
        core = core_with_probes(rs, 40)
        q = S.seq(damaged(rs, core, force=probe_cols(40)))
        for i in range(n - 1):
            target(S, rs, q, core, 0, 39, 0, 100, True)
        S.group(name, q, True)
    for n, name in ((15, "sat_15_noself"), (64, "sat_64_noself")):
        core = core_with_probes(rs, 40)
        q = S.seq(damaged(rs, core, force=probe_cols(40)), self_record=False)
        for i in range(n):
            target(S, rs, q, core, 0, 39, 0, 100, True)
        S.group(name, q, True)

    # ---- query lengths: last code word, last chunk of 64
    for L in (30, 31, 47, 48, 49, 63, 64, 65, 127, 128, 129, 200):
        for o, n in (("m", 3), ("r", 20)):
            pile(S, rs, "qlen_%d_%s%d" % (L, o, n), L, n, o, tlen=L + 37)

    # ---- staging: 12 words hold 177 columns wherever they start; span x letter offset of the stored span within a word
    for span in (176, 177, 178, 192, 193):
        for woff in (0, 1, 15):
            for rev in (False, True):
                for withN in (False, True):
                    core = core_with_probes(rs, span, probes=(0, 15, 16, span // 2, span - 17, span - 16, span - 1))
                    query = damaged(rs, core, force=(0, 15, 16, span // 2, span - 17, span - 16, span - 1))
                    q = S.seq(query)
                    for i in range(3):
                        tl = (400, 333, span + 48)[i]
                        lo = 16 * int(rs.randint(0, (tl - span - 15) // 16 + 1)) + woff      # stored start of the span
                        ds = tl - lo - span if rev else lo
                        sed = None
                        if withN and i == 1:
                            def sed(stored, lo=lo, span=span):        # an N on a purine column of the span: same RY class
                                p = next(j for j in range(lo + 20, lo + span) if stored[j] in b"AG")
                                stored[p] = ord("N")
                        target(S, rs, q, core, 0, span - 1, ds, tl, rev, stored_edit=sed)
                    S.group("stage_%d_w%d_%s%s" % (span, woff, "r" if rev else "f", "_N" if withN else ""), q, True)

    # ---- RY gates (the in member first)
    def ry_group(name, alen, mism, calls, n=3):
        pile(S, rs, name, alen if n < 45 else 2 * alen, n, "m", tlen=alen + 23, calls=calls, edit=ry_edit(mism) if mism else None,
             seq_id="0.950" if mism else "1.00", alen=None if n < 45 else alen)
    for alen, calls in ((30, True), (29, False)):
        # aLen 29 | 30: a 40-letter query of which the records cover the last 29 / 30 columns
        core = core_with_probes(rs, 40, probes=(20, 34, 35, 39))
        q = S.seq(damaged(rs, core, force=(20, 34, 35, 39)))
        for i in range(4):
            target(S, rs, q, core, 40 - alen, 39, 11 + i, 80, i % 2 == 1)
        S.group("alen_%d" % alen, q, calls)
    for alen, ok, bad in ((100, 1, 2), (101, 1, 2), (200, 2, 3), (300, 3, 4), (700, 7, 8)):
        ry_group("ry_%d_m%d" % (alen, ok), alen, ok, True)
        ry_group("ry_%d_m%d" % (alen, bad), alen, bad, False)
    ry_group("ry_100_m0", 100, 0, True)
    ry_group("ry_101_m0", 101, 0, True)
    # the same decision with 16..64 records and with more than 64
    for n in (20, 70):
        ry_group("ry_100_m1_n%d" % n, 100, 1, True, n=n)
        ry_group("ry_100_m2_n%d" % n, 100, 2, False, n=n)

    # ---- seqId text at the threshold, a target that is an extended sequence
    pile(S, rs, "seqid_0.900", 40, 3, "m", seq_id="0.900")
    pile(S, rs, "seqid_0.899", 40, 3, "m", seq_id="0.899", calls=False)
    for nm, e, calls in (("ext_target_0", 0, True), ("ext_target_1", 1, False)):
        core = core_with_probes(rs, 40)
        q = S.seq(damaged(rs, core, force=probe_cols(40)))
        for i in range(3):
            target(S, rs, q, core, 0, 39, 7 + i, 100, i == 1, ext=e)
        S.group(nm, q, calls)

    # ---- avCov just below and at 50: inside records leave at 50, right-only and left-only ones stay.
    # 16..64 records: a 40-letter query and 40-column records, 48 | 49 of them; more than 64: a 60-letter query and 30-column
    # records, 97 | 98 of them (60 + 30 * 98 = 50 * 60)
    def cov_group(name, qlen, alen, n, kind, calls):
        qa = qlen - alen if kind != "left" else 0
        pr = (qa, qa + 4, qa + 5, qa + alen // 2, qa + alen - 6, qa + alen - 5, qa + alen - 1)
        core = core_with_probes(rs, qlen, probes=pr)
        q = S.seq(damaged(rs, core, force=pr))
        for i in range(n):
            tl = 100
            ds = {"inside": 1 + i % (tl - alen - 1), "right": 0, "left": tl - alen}[kind]
            target(S, rs, q, core, qa, qa + alen - 1, ds, tl, i % 3 == 1)
        S.group(name, q, calls)
    for kind in ("inside", "right", "left"):
        cov_group("avcov49_%s" % kind, 40, 40, 48, kind, True)
        cov_group("avcov50_%s" % kind, 40, 40, 49, kind, kind != "inside")
        cov_group("avcov49.5_big_%s" % kind, 60, 30, 97, kind, True)
        cov_group("avcov50_big_%s" % kind, 60, 30, 98, kind, kind != "inside")

    # ---- the 2/5 rule: T (or A, or A made of target N's) holds exactly 2 of 5, 4 of 10 -> kept; 2 of 6, 3 of 8 -> called
    for letter in ("T", "A", "N"):
        for have, total in ((2, 5), (4, 10), (2, 6), (3, 8)):
            true = b"C" if letter == "T" else b"G"
            core = bytearray(rnd(rs, 40)); core[20:21] = true
            core = bytes(core)
            query = bytearray(damaged(rs, core, rate=0.0, force=(20,)))
            q = S.seq(bytes(query))
            for i in range(total - 1):
                ed = None
                if i < have - 1:
                    ed = lambda mid, c=ord(letter): mid.__setitem__(20, c)
                target(S, rs, q, core, 0, 39, 3 + 5 * i, 100, i % 2 == 1 and letter != "N", edit=ed)
            S.group("rule_%s_%dof%d" % (letter, have, total), q, 5 * have < 2 * total)

    # ---- damage classes.  With a read query the steps sit on probed columns of targets of 30, 31 and 100 letters; a wrong class
    # shows there only where it tips a call, which for reads it never does (the 2/5 rule leaves no close calls).  The competitions
    # are the extended queries: 30 letters, all T (A) over a truth of C (G); of nine or ten full-length records exactly one holds
    # T (A) in a column.  Eight or nine times log P(C -> C) + log 1000 of the records' classes against log P(C -> T) of the odd
    # one's class and the sequencing error of the query: the winner turns on the 5' and 3' class ramps of the targets.  (In the
    # dhigh profile classes 4, 5 and 6 share one row, so a step misplaced between them alone is invisible; a ramp shifted by one
    # class is not.)
    for tl in (30, 31, 100):
        for o in "fr":
            core = core_with_probes(rs, 60)
            q = S.seq(damaged(rs, core, force=probe_cols(60)))
            for i in range(6):
                alen = 30 if tl < 100 else 40
                target(S, rs, q, core, (0, 60 - alen, 15)[i % 3], (0, 60 - alen, 15)[i % 3] + alen - 1, (0, tl - alen, (tl - alen) // 2)[i // 2 % 3], tl, o == "r")
            S.group("class_t%d_%s" % (tl, o), q, True)
    # the same proportion at 18 records (two odd ones per column) for the 16..64 instance and at 72 (eight) for the general
    # kernel, where avCov >= 50 admits right-only and left-only records alone
    for gi in range(36):
        mult = (1, 1, 2, 8)[gi % 4]
        n = (9 + gi % 2) if mult == 1 else 9 * mult
        core = bytes(bytearray(rs.choice(np.frombuffer(b"CG", np.uint8), size=30)))
        q = S.seq(damaged(rs, core, rate=1.0), 1)
        odd = np.array([rs.permutation(n)[:mult] for _ in range(30)])       # which records hold the damaged letter in a column
        for i in range(n):
            tl = (30, 31, 100, 31, 100)[(i + gi) % 5]
            ds = {30: 0, 31: (i + gi) % 2}.get(tl, (0, 70, 1, 66, 35)[(i + gi // 5) % 5] if mult < 8 else (0, 70)[i % 2])
            def ed(mid, cols=np.nonzero((odd == i).any(1))[0]):
                for j in cols:
                    mid[j] = _DAMAGE[mid[j]]
            target(S, rs, q, core, 0, 29, ds, tl, _rev_of("frm"[gi % 3], i), edit=ed, seq_id="0.966")
        S.group("class_ext_%d_n%d" % (gi, n), q, None)
    # query class steps p 4 | 5 and qLen-6 | qLen-5 are probed columns of every pile above; here with an extended query
    for o in "fr":
        pile(S, rs, "qclass_ext_%s" % o, 40, 14, o, qext=1, calls=None)

    # ---- N: a query N with coverage <= 1 is kept, with coverage >= 2 it is called (N counts as A: put it where the truth is G)
    core = bytearray(rnd(rs, 80)); core[10:11] = b"G"; core[50:51] = b"G"; core = bytes(core)
    query = bytearray(damaged(rs, core, force=(40, 79))); query[10] = ord("N"); query[50] = ord("N")
    q = S.seq(bytes(query))
    for i in range(4):
        target(S, rs, q, core, 30, 79, 0, 100, i % 2 == 1)
    S.group("queryN", q, True)
    # a target N off and on the aligned columns, 2..15 and 16..64 records
    for n in (4, 20):
        core = core_with_probes(rs, 60)
        pu = next(j for j in range(20, 60) if core[j] in b"AG")
        q = S.seq(damaged(rs, core, force=probe_cols(60)))
        for i in range(n):
            target(S, rs, q, core, 0, 59, 5 + i, 100, i % 2 == 1, edit=(lambda mid, pu=pu: mid.__setitem__(pu, ord("N"))) if i % 3 == 0 else None)
        S.group("targetN_n%d" % n, q, True)

    # ---- letters beyond ACGTN (lower case, IUPAC) in the query, in one target, in both: the general kernel takes these queries
    for where in ("query", "target", "both"):
        for n in (4, 20):
            for odd in (b"a", b"g", b"R", b"t", b"Y"):
                core = core_with_probes(rs, 60)
                col = next(j for j in range(25, 60) if core[j] in (b"AG" if odd in (b"a", b"g", b"R") else b"CT"))
                query = bytearray(damaged(rs, core, force=probe_cols(60), spare=(col,)))
                if where != "target":
                    query[col] = odd[0]
                q = S.seq(bytes(query))
                for i in range(n):
                    sed = None
                    rev = i % 2 == 1
                    ds = 5 + i
                    if where != "query" and i == 1:
                        def sed(stored, p=(100 - 1 - (ds + col)) if rev else ds + col, c=odd[0]):
                            stored[p] = c
                    target(S, rs, q, core, 0, 59, ds, 100, rev, stored_edit=sed)
                S.group("raw_%s_n%d_%s" % (where, n, odd.decode()), q, True)

    # ---- sparse: a query with no record at all, a query with only a non-self record
    S.group("no_record", S.seq(rnd(rs, 50), self_record=False), False)
    core = core_with_probes(rs, 40)
    q = S.seq(damaged(rs, core, force=probe_cols(40)), self_record=False)
    target(S, rs, q, core, 0, 39, 9, 100, False)
    S.group("only_nonself", q, False)
    return S.finish()


def lonely_set(seed=5):
    """a DB in which no query has two records (the kernels' lists are all empty)"""
    rs = np.random.RandomState(seed)
    S = CaseSet()
    for i in range(40):
        S.group("lonely_%d" % i, S.seq(rnd(rs, int(rs.randint(30, 130))), ext=i % 7 == 0, self_record=i % 5 != 0), False)
    return S.finish()


def single_set(seed=3):
    """a DB of one sequence"""
    rs = np.random.RandomState(seed)
    S = CaseSet()
    S.group("single", S.seq(rnd(rs, 77)), False)
    return S.finish()


SETS = (("main", main_set), ("lonely", lonely_set), ("single", single_set))

# the in / out pairs of every gate: (changed, unchanged)
GATE_PAIRS = [("avcov49_inside", "avcov50_inside"), ("avcov49.5_big_inside", "avcov50_big_inside"), ("alen_30", "alen_29"),
              ("ry_100_m1", "ry_100_m2"), ("ry_101_m1", "ry_101_m2"), ("ry_200_m2", "ry_200_m3"), ("ry_300_m3", "ry_300_m4"),
              ("ry_700_m7", "ry_700_m8"), ("ry_100_m1_n20", "ry_100_m2_n20"), ("ry_100_m1_n70", "ry_100_m2_n70"),
              ("seqid_0.900", "seqid_0.899"), ("ext_target_0", "ext_target_1"),
              ("rule_T_2of6", "rule_T_2of5"), ("rule_T_3of8", "rule_T_4of10"), ("rule_A_2of6", "rule_A_2of5"), ("rule_A_3of8", "rule_A_4of10"),
              ("rule_N_2of6", "rule_N_2of5"), ("rule_N_3of8", "rule_N_4of10")]


# --------------------------------------------------------------------------------------------------------- the RY hand-off
def ry_handoff_set(seed=23):
    """Prefilter hits for cdm_rescore -> cdm_correct: rescore counts the purine/pyrimidine mismatches of every record, compacts them
    beside the records (k_scatter up to 256 hits per query, k_scatter_big beyond) and the corrector trusts them.  Returns
    (seqs, hits, info): hits[q] = [(target, score, diagonal)] (score < 0: reverse strand), info[q] = {"name", "one": targets that are
    accepted with 1 RY mismatch, "two": targets accepted by rescore with 2 (the corrector turns them away), "junk": rejected hits}.

    Every query is damaged at a few C / G columns.  Its targets with at most one RY mismatch hold the truth there, those with two
    hold the damaged letter: were one of them let in (a count that slid by one record in the compaction), T or A would reach 2/5
    of the column and the base would stay.  Rejected hits (unrelated sequences) are interleaved with the accepted ones.
    The first sequence is a query with few hits: the deep queries' hits do not start the hit array."""
    rs = np.random.RandomState(seed)
    seqs, hits, info = [], {}, {}

    def add(s):
        seqs.append(bytes(s))
        hits[len(seqs) - 1] = [(len(seqs) - 1, 2 * len(s), 0)]        # the identity hit
        return len(seqs) - 1
    pool = [add(rnd(rs, 100)) for _ in range(320)]

    def flips(mid, k, cols):
        for j in range(k):
            p = next(c for c in range(6 + 13 * j, len(mid)) if c not in cols)
            mid[p] = bytes([mid[p]]).translate(_RYFLIP)[0]

    def query(name, qlen, layouts, n_junk, withN=None):
        """layouts: (reverse, diagonal, tlen) per accepted target"""
        dcols = [c for c in (3, qlen // 2, qlen - 4)]
        core = core_with_probes(rs, qlen, probes=dcols)
        qseq = bytearray(damaged(rs, core, rate=0.0, force=dcols))
        if withN == "query":
            qseq[next(c for c in range(10, qlen) if core[c] in b"AG" and c not in dcols)] = ord("N")
        q = add(bytes(qseq))
        inf = info[q] = {"name": name, "one": [], "two": [], "junk": []}
        acc = []
        for i, (rev, d, tlen) in enumerate(layouts):
            src = revcomp(core) if rev else core
            dq = [qlen - 1 - c for c in dcols] if rev else dcols
            if d >= 0:
                q0, t0, m = d, 0, min(tlen, qlen - d)
            else:
                q0, t0, m = 0, -d, min(tlen + d, qlen)
            mid = bytearray(src[q0: q0 + m])
            local = {c - q0 for c in dq if q0 <= c < q0 + m}
            kind = ("zero", "one", "two", "one", "two")[i % 5]
            if kind == "two":                                     # holds the damaged letter where the query is damaged
                for c in local:
                    mid[c] = _DAMAGE[mid[c]] if not rev else {ord("G"): ord("A"), ord("C"): ord("T")}[mid[c]]
            flips(mid, {"zero": 0, "one": 1, "two": 2}[kind], local)
            t = bytearray(rnd(rs, t0) + bytes(mid) + rnd(rs, tlen - t0 - m))
            if withN == "target" and i == 0:
                t[t0 + next(c for c in range(8, m) if mid[c] in b"AG" and c not in local)] = ord("N")
            tk = add(bytes(t))
            inf["one" if kind != "two" else "two"].append(tk)
            acc.append((tk, -60 if rev else 60, d))
        junk = [(pool[j], 40 if j % 3 else -40, int(rs.randint(-20, 20))) for j in rs.permutation(len(pool))[:n_junk]]
        inf["junk"] = [j[0] for j in junk]
        order = []                                                # junk first, then interleaved
        ai, ji = 0, 0
        while ai < len(acc) or ji < len(junk):
            take_junk = ji < len(junk) and (ai >= len(acc) or (ai + ji) % 3 != 2 or ji * len(acc) < ai * len(junk))
            if take_junk:
                order.append(junk[ji]); ji += 1
            else:
                order.append(acc[ai]); ai += 1
        hits[q] = order[: len(order) // 2] + hits[q] + order[len(order) // 2:]
        return q

    # overlaps m % 16 in {0, 1, 15}, diagonals of both signs, both strands, query lengths that are no multiple of 16 on the reverse strand
    for m in (48, 49, 47):
        for qlen in (m + 22, 77):
            lay = []
            for i in range(10):
                rev = i % 2 == 1
                lay.append((rev, qlen - m, 100) if i % 4 < 2 else (rev, -(90 - m), 90))
            query("m%d_q%d" % (m, qlen), qlen, lay, 7)
    query("N_query", 75, [(i % 2 == 1, 75 - 50, 100) for i in range(10)], 5, withN="query")
    query("N_target", 75, [(i % 2 == 1, -(90 - 50), 90) for i in range(10)], 5, withN="target")
    # 255 | 256 | 257 and 300 hits (identity included): full-length records of 100 columns, where one RY mismatch passes and two do not
    for nh in (255, 256, 257, 300):
        n_acc = 60
        query("deep_%d" % nh, 100, [(i % 3 == 1, 0, 100) for i in range(n_acc)], nh - 1 - n_acc)
    return seqs, hits, info


def ry_handoff_oracle(oracle_bin, dhigh_prefix, tmpdir):
    """the oracle's rescorediagonal and ancient_correction on ry_handoff_set(), and the conditions on the input checked on that run
    alone: in every query both kinds of accepted record follow a rejected hit, every query is corrected, the deep queries sit on
    both sides of the 256-hit split.  Returns (seqs, info, prefilter entries, alignment DB, corrected DB)."""
    import os
    from carpedeam_amd import mmdb
    from gpuutil import run_oracle
    from stageflags import A_FLAGS, R_FLAGS
    seqs, hits, info = ry_handoff_set()
    t = lambda s: os.path.join(str(tmpdir), s)
    mmdb.write_seqdb(t("in"), seqs)
    pref = [(q, "".join("%d\t%d\t%d\n" % h for h in hits[q]).encode()) for q in sorted(hits)]
    mmdb.write_db(t("pref"), pref, mmdb.DBTYPE_PREFILTER_REV_RES)
    run_oracle(oracle_bin, "rescorediagonal", t("in"), t("in"), t("pref"), t("aln"), *R_FLAGS, "--threads", "4")
    run_oracle(oracle_bin, "ancient_correction", t("in"), t("aln"), t("corr"), *A_FLAGS, "--ancient-damage", dhigh_prefix, "--threads", "4")
    aln, corr = mmdb.read_db(t("aln")), mmdb.read_db(t("corr"))
    for q, inf in info.items():
        kept = [int(l.split("\t")[0]) for l in aln[q][0].decode().split("\n") if l]
        order = [h[0] for h in hits[q]]
        first_rejected = min(order.index(j) for j in inf["junk"] if j not in kept)
        for kind in ("one", "two"):
            assert any(k in kept and order.index(k) > first_rejected for k in inf[kind]), (inf["name"], kind)
        assert mmdb.canon(corr)[q][0] != seqs[q], inf["name"]
    assert sorted(len(hits[q]) for q, inf in info.items() if inf["name"].startswith("deep")) == [255, 256, 257, 300]
    assert min(q for q, inf in info.items() if inf["name"].startswith("deep")) > 0 and len(hits[0]) <= 256
    return seqs, info, pref, aln, corr
