"""tests/gapped_model.py against itself and against hand-computed answers: the row form the kernel uses equals the three-matrix
yardstick cell for cell in what leaves them (score, end and start cell, operations), the tie rules on directed cases, band 0 is the
ungapped overlap, and the SAM check refuses broken lines.  No device."""
import random
import re

import numpy as np
import pytest

import gapped_model as gm
import map_model as mm

P = gm.Params()
M, I, D = gm.OP_M, gm.OP_I, gm.OP_D


def codes(s):
    return [int(c) for c in mm.codes(s)]


def random_pair(rng, B):
    """a contig, a read copied from it with substitutions, N letters and indels of 1..6 letters, hanging over either contig end in some
    pairs, and a diagonal within the band's reach of where the read starts"""
    L = rng.randrange(20, 151)
    n = rng.randrange(max(10, L // 2), L + 60)
    contig = [rng.choice("ACGT") for _ in range(n)]
    start = rng.randrange(-L // 3, n - L // 2)
    src = [contig[i] if 0 <= i < n else rng.choice("ACGT") for i in range(start, start + L + 12)]
    read = []
    i = 0
    gaps = rng.randrange(0, 3)
    at = sorted(rng.randrange(3, L) for _ in range(gaps))
    while len(read) < L and i < len(src):
        if at and len(read) >= at[0]:
            at.pop(0)
            g = rng.randrange(1, 7)
            if rng.random() < 0.5:
                i += g                                           # the read lacks g contig letters
            else:
                read += [rng.choice("ACGT") for _ in range(g)]   # the read has g letters of its own
            continue
        c = src[i]
        r = rng.random()
        read.append("N" if r < 0.01 else rng.choice("ACGT") if r < 0.05 else c)
        i += 1
    read = read[:L] + [rng.choice("ACGT") for _ in range(L - len(read))]
    if rng.random() < 0.1:
        contig[rng.randrange(n)] = "N"
    if rng.random() < 0.3:         # homopolymer stretches: ties
        a = rng.randrange(0, n - 5)
        contig[a:a + 5] = contig[a] * 5
    Df = start + rng.randrange(-B - 2, B + 3)
    return "".join(contig), "".join(read), Df


@pytest.mark.parametrize("B", [1, 2, 8, 31])
def test_the_row_form_equals_the_three_matrices(B):
    """2200 random pairs in all, 550 a band"""
    rng = random.Random(20261019 + B)
    seen = {"I": 0, "D": 0, "none": 0, "left": 0, "right": 0, "N": 0}
    p = gm.Params(band=B)
    for _ in range(550):
        contig, read, Df = random_pair(rng, B)
        Q, R = codes(contig), codes(read)
        a, b = gm.align_pair(Q, R, Df, B, p), gm.align_rows(Q, R, Df, B, p)
        assert a == b, (B, contig, read, Df, a, b)
        if a is None:
            seen["none"] += 1
            continue
        d = gm.describe(Q, R, a)
        assert d["span"] == a["end"][0] - a["start"][0] + 1 and d["columns"] == a["end"][1] - a["start"][1] + 1
        assert a["start"][0] == 0 or a["start"][1] == 0
        assert a["end"][0] == len(Q) - 1 or a["end"][1] == len(R) - 1
        assert abs(a["start"][0] - a["start"][1] - Df) <= B and abs(a["end"][0] - a["end"][1] - Df) <= B
        seen["I"] += d["inserted"] > 0
        seen["D"] += d["deleted"] > 0
        seen["left"] += a["start"][1] > 0
        seen["right"] += a["end"][1] < len(R) - 1
        seen["N"] += "N" in read or "N" in contig
    assert min(seen["I"], seen["D"], seen["left"], seen["right"], seen["N"]) >= 25, seen


@pytest.mark.parametrize("open_,extend", [(5, 2), (2, 2), (7, 1)])
def test_the_row_form_with_other_gap_costs(open_, extend):
    """open == extend is the bound at which the one-pass row form is still exact (and every gap tie between opening and extending shows)"""
    rng = random.Random(open_ * 10 + extend)
    p = gm.Params(band=8, gap_open=open_, gap_extend=extend)
    for _ in range(150):
        contig, read, Df = random_pair(rng, 8)
        Q, R = codes(contig), codes(read)
        assert gm.align_pair(Q, R, Df, 8, p) == gm.align_rows(Q, R, Df, 8, p), (contig, read, Df)


FLANK_A, FLANK_B = "GATTACAGCTCAGGTC", "CTGACCATGCTAGGCA"


@pytest.mark.parametrize("align", [gm.align_pair, gm.align_rows], ids=["pair", "rows"])
def test_ties_in_a_homopolymer(align):
    """a read that lacks one A of a run of five: the five places score the same.  The walk back from the end prefers M at every tie, so
    the read's four A pair with the run's LAST four contig letters and the deletion takes the run's first letter (by hand)"""
    contig = FLANK_A + "AAAAA" + FLANK_B
    read = FLANK_A + "AAAA" + FLANK_B
    a = align(codes(contig), codes(read), 0, 2, P)
    n_match = len(read)
    assert a["score"] == 2 * n_match - 5
    assert a["ops"] == [(M, 16), (D, 1), (M, 20)]
    # one A more than the contig: the insertion likewise at the left end of the run
    a = align(codes(read), codes(contig), 0, 2, P)
    assert a["score"] == 2 * n_match - 5 and a["ops"] == [(M, 16), (I, 1), (M, 20)]


@pytest.mark.parametrize("align", [gm.align_pair, gm.align_rows], ids=["pair", "rows"])
def test_a_gap_that_could_open_at_two_places(align):
    """the contig holds CG twice where the read holds it once: deleting either copy scores the same; the walk back prefers M, so the
    read's CG pairs with the RIGHT copy and the deletion takes the left one"""
    contig = FLANK_A + "TCGCGA" + FLANK_B
    read = FLANK_A + "TCGA" + FLANK_B
    a = align(codes(contig), codes(read), 0, 3, P)
    assert a["score"] == 2 * len(read) - 7 and a["ops"] == [(M, 17), (D, 2), (M, 19)]
    d = gm.describe(codes(contig), codes(read), a)
    assert [w & 0xFFFFFF for w in d["words"]] == [17, 18] and all(w >> 28 == gm.DELETED for w in d["words"])
    assert [(w >> 24) & 15 for w in d["words"]] == [1, 2]          # C, G


def test_a_substitution_is_not_a_deletion_beside_an_insertion():
    """a contig letter without a read letter beside a read letter without a contig letter costs 10, the mismatch column 3"""
    a = gm.align_pair(codes("ACGTACGTAAGTACGTACGT"), codes("ACGTACGTACGTACGTACGT"), 0, 2, gm.Params(band=2))
    assert a["ops"] == [(M, 20)] and a["score"] == 2 * 19 - 3


def test_band_zero_is_the_ungapped_overlap():
    rng = random.Random(77)
    for _ in range(300):
        L, n = rng.randrange(20, 100), rng.randrange(30, 160)
        contig = "".join(rng.choice("ACGTN") if rng.random() < 0.02 else rng.choice("ACGT") for _ in range(n))
        Df = rng.randrange(-L + 1, n)
        read = "".join(contig[i] if 0 <= i < n and rng.random() < 0.9 else rng.choice("ACGT") for i in range(Df, Df + L))
        Q, R = codes(contig), codes(read)
        p = gm.Params(band=0)
        a, b = gm.align_pair(Q, R, Df, 0, p), gm.align_rows(Q, R, Df, 0, p)
        assert a == b
        i0, j0 = max(Df, 0), max(-Df, 0)
        cols = min(n - i0, L - j0)
        mism = sum(1 for c in range(cols) if Q[i0 + c] == 4 or R[j0 + c] == 4 or Q[i0 + c] != R[j0 + c])
        d = gm.describe(Q, R, a)
        assert a["start"] == (i0, j0) and a["ops"] == [(M, cols)] and len(d["words"]) == mism and d["score"] == 2 * (cols - mism) - 3 * mism


def test_real_diagonals_and_their_inverse():
    assert gm.real_diagonals(5, 100, 40, False) == [5] and gm.real_diagonals(-5 & 0xFFFF, 100, 40, False) == [-5]
    assert gm.real_diagonals(464, 70000, 100, False) == [464, 66000]
    for n, L, Df, rev in ((70000, 100, 66000, False), (70000, 100, 66000, True), (100, 40, -7, True), (100, 40, 93, False), (300, 4096, -4000, False)):
        assert Df in gm.real_diagonals(gm.hit_diagonal(Df, n, L, rev), n, L, rev)


def small_case():
    """one contig, three reads: one with a deleted letter (rescued, primary), one that also has an ungapped record (no candidate), one
    reverse with an inserted letter"""
    rng = np.random.default_rng(9)
    contig = "".join(rng.choice(list("ACGT"), size=200))
    r1 = contig[20:50] + contig[51:90]
    r2 = contig[100:150]
    r3 = (contig[120:150] + "T" + contig[150:185]).translate(mm.COMPLEMENT)[::-1]
    seqs = [contig, r1, r2, r3]
    hits = np.array([(0, 400, 0), (1, 50, gm.hit_diagonal(20, 200, len(r1), False)), (2, 60, gm.hit_diagonal(100, 200, 50, False)),
                     (3, -50, gm.hit_diagonal(120, 200, len(r3), True))], [("target", "<u4"), ("score", "<i4"), ("diagonal", "<i4")])
    hoff = np.array([0, 4, 4, 4, 4], np.uint64)
    from pileupcases import case, identity
    from pileup_model import unorient
    c = case(seqs, {0: [identity(seqs, 0), unorient(2, 100, 149, 0, 49, False, 50)]}, [0])
    return seqs, hoff, hits, c["off"], c["rec"]


def records_words_and_the_text():
    seqs, hoff, hits, aoff, arec = small_case()
    gone = 50           # the deleted contig letter: the leftmost of a run of equal letters that ends at 50 (M is preferred on the walk back)
    while seqs[0][gone - 1] == seqs[0][gone]:
        gone -= 1
    for align in (gm.align_pair, gm.align_rows):
        stats, recs, ops, words = gm.gapped_records(seqs, [1, 0, 0, 0], hoff, hits, aoff, arec, [0], gm.Params(skip=True), align)
        assert stats.tolist() == [[2, 2, 2, 0]]
        assert recs["target"].tolist() == [1, 3] and recs["pos"].tolist() == [20, 120] and recs["span"].tolist() == [70, 65] and recs["columns"].tolist() == [69, 66]
        assert recs["flags"].tolist() == [0, gm.REVERSE] and recs["nm"].tolist() == [1, 1] and recs["n_words"].tolist() == [1, 0]
        assert [[(int(w) >> 2, int(w) & 3) for w in ops[int(r["ops"]):int(r["ops"]) + int(r["n_ops"])]] for r in recs] == [[(gone - 20, M), (1, D), (89 - gone, M)], [(30, M), (1, I), (35, M)]]
    _, mrecs, mism = mm.map_records(seqs, [1, 0, 0, 0], aoff, arec, [0], 0.0, True)
    text = gm.sam_text_gapped(["c"], [200], lambda t: "r%d" % t, lambda t: seqs[t], mrecs, mism, recs, ops, words)
    lines = [l.split("\t") for l in text.split("\n") if l and l[0] != "@"]
    assert [l[0] for l in lines] == ["r1", "r2", "r3"] and [l[5] for l in lines] == ["%dM1D%dM" % (gone - 20, 89 - gone), "50M", "30M1I35M"]
    assert lines[0][12] == "MD:Z:%d^%s%d" % (gone - 20, seqs[0][50], 89 - gone) and lines[0][-1] == "XG:i:1" and lines[2][12] == "MD:Z:65" and lines[2][11] == "NM:i:1"
    assert gm.sam_check_gapped(text, {"c": seqs[0]}) == (3, 2)
    return text


def test_records_words_and_the_text():
    records_words_and_the_text()


def test_sam_check_rejects_a_hand_broken_line():
    text = records_words_and_the_text()
    contigs = {"c": small_case()[0][0]}
    cigar = [l.split("\t")[5] for l in text.split("\n") if l.startswith("r1\t")][0]
    a, b = (int(x) for x in re.findall(r"(\d+)M", cigar))
    for old, new, what in ((cigar, "%dM1D%dM" % (a, b - 1), "sum to len"), ("XG:i:1", "XG:i:2", "XG"), ("NM:i:1\tMD:Z:%d^" % a, "NM:i:2\tMD:Z:%d^" % a, "NM"), (cigar, "%dM1D%dM" % (a + 1, b - 1), "rebuild|deleted|match"),
                           ("30M1I35M", "30M1D35M", "sum to len|cover"), ("\t121\t", "\t19\t", "sorted|rebuild")):
        assert old in text
        with pytest.raises(ValueError, match=what):
            gm.sam_check_gapped(text.replace(old, new, 1), contigs)
    dup = text + [l for l in text.split("\n") if l.startswith("r1\t")][0].replace("\t21\t", "\t21\t", 1) + "\n"
    with pytest.raises(ValueError, match="sorted|lines without 256"):
        gm.sam_check_gapped(dup, contigs)
