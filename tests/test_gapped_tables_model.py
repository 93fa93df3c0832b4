"""tests/gapped_tables_model.py against answers that do not come from it: a forward and a reverse gapped record worked out by hand,
the span rule against its literal reading, the single-M property (an ungapped record turned into a gapped record of one M operation
changes no output of the three models) and the planted corpus, where the ungapped records alone give one false break per planted
indel and the rescued reads take all four away."""
import numpy as np
import pytest

import bases_model as bm
import breaks_model as brm
import depth_model as dm
import gapped_model as gm
import gapped_tables_model as gt
import indelcases as ic
import pileupcases as pc
from pileup_model import csr

M, I, D = gm.OP_M, gm.OP_I, gm.OP_D


def hand_case():
    """a contig of 40 letters without N and two reads, given in the contig's orientation:
    F forward at pos 5: 2 clipped, 6M 2I 4M 3D 5M, 1 clipped   M columns on 5..10, 11..14 and 18..22 with the offsets 2..7, 10..13, 14..18
    R reverse at pos 12: 1 clipped, 3M 1D 2M 1I 3M, 2 clipped  M columns on 12..14, 16..17 and 18..20 with the offsets 1..3, 4..5, 7..9"""
    rng = np.random.default_rng(40)
    contig = pc.rand_seq(rng, 40)
    f = "TT" + "ACGTAC" + "GG" + "NACG" + "TTTTT" + "A"
    r = "C" + "GGA" + "CN" + "T" + "ACC" + "GT"
    seqs = [contig, f, ic.revcomp(r)]
    off, rec = csr(3, {0: [pc.identity(seqs, 0)]})
    grecs = np.zeros(2, gm.GAP_DTYPE)
    grecs[0] = (0, 1, 5, 18, 2, 20, 17, 0, 0, 5, 0, 0, 0, 0)
    grecs[1] = (0, 2, 12, 9, 1, 12, 9, 0, gm.REVERSE, 5, 0, 0, 5, 0)
    gops = np.array([6 << 2 | M, 2 << 2 | I, 4 << 2 | M, 3 << 2 | D, 5 << 2 | M, 3 << 2 | M, 1 << 2 | D, 2 << 2 | M, 1 << 2 | I, 3 << 2 | M], np.uint32)
    return dict(seqs=seqs, ext=[1, 0, 0], off=off, rec=rec, queries=[0], grecs=grecs, gops=gops)


def args(c):
    return c["seqs"], c["ext"], c["off"], c["rec"], c["queries"], c["grecs"], c["gops"]


def hand_depth():
    d = np.zeros(40, np.uint32)
    d[5:15] += 1; d[18:23] += 1                         # F: a deleted letter (15, 16, 17) gets no depth
    d[12:15] += 1; d[16:18] += 1; d[18:21] += 1         # R: 15 is deleted
    return d


def test_the_hand_worked_records_depth():
    c = hand_case()
    stats, tracks = gt.depth_stats(*args(c), edge=0, skip=True)
    want = hand_depth()
    assert want.tolist()[10:24] == [1, 1, 2, 2, 2, 0, 1, 1, 2, 2, 2, 1, 1, 0]
    assert np.array_equal(tracks[0], want)
    # reads 2, columns 15 + 8, breadth 17, window 40, covered 17, sum 23, sumsq 11 x 1 + 6 x 4, max 2
    assert stats[0].tolist() == [2, 23, 17, 40, 17, 23, 35, 2]
    stats, _ = gt.depth_stats(*args(c), edge=10, skip=True)          # the window 10..29: 1 1 2 2 2 0 1 1 2 2 2 1 1 and zeros
    assert stats[0].tolist() == [2, 23, 17, 20, 12, 18, 30, 2]


def test_the_hand_worked_records_span_at_anchor_3():
    """F: C = 15, m_3 = 7 and m_13 = 20, the boundaries 8..20; R: C = 8, m_3 = 14 and m_6 = 18, the boundaries 15..18"""
    c = hand_case()
    stats, tracks, breaks = gt.breaks_stats(*args(c), anchor=3, edge=3, skip=True)
    want = np.zeros(40, np.uint32)
    want[8:21] += 1; want[15:19] += 1
    assert np.array_equal(tracks[0], want) and want[15] == 2 and want[19] == 1
    # window: the boundaries 3..37; weak where span is 0: 3..7 and 21..37, two runs, both with uncovered positions
    assert stats[0].tolist() == [2, 23, 35, 22, 2, 0, 0, 17]
    assert breaks.tolist() == [(0, 3, 7, 0, 2, 0, 1, brm.GAP), (0, 21, 37, 0, 14, 2, 0, brm.GAP)]
    # edge 8 keeps the boundaries 8..32.  The deleted position 15 has depth 0 and a span of 2: the boundaries 15 and 16 are not weak
    # and give no break; 21..32 are weak, one run
    stats, _, breaks = gt.breaks_stats(*args(c), anchor=3, edge=8, skip=True)
    assert stats[0].tolist() == [2, 23, 25, 12, 1, 0, 0, 17]
    assert breaks.tolist() == [(0, 21, 32, 0, 9, 2, 0, brm.GAP)]
    # at two spanning reads only 15..18 hold; with the percent rule at 100 the boundaries 15 and 16 hold all the same: min(depth) = 0
    stats, _, breaks = gt.breaks_stats(*args(c), anchor=3, edge=8, min_span=2, skip=True)
    assert [(int(b["first"]), int(b["last"])) for b in breaks] == [(8, 14), (19, 32)]
    stats, _, breaks = gt.breaks_stats(*args(c), anchor=3, edge=8, min_span=1, min_span_percent=100, skip=True)
    assert [(int(b["first"]), int(b["last"])) for b in breaks] == [(13, 14), (19, 32)]
    # anchor 8: R (C = 8 < 16) spans nothing, F spans m_8 + 1 = 13 .. m_8 = 12: C = 15 < 16, nothing either
    _, tracks, _ = gt.breaks_stats(*args(c), anchor=8, edge=8, skip=True)
    assert not tracks[0].any()
    # anchor 4: R has C = 8 = 2 x 4: m_4 + 1 = 17 .. m_5 = 17, the one boundary between its fourth and fifth column
    _, tracks, _ = gt.breaks_stats(*args(c), anchor=4, edge=4, skip=True)
    want = np.zeros(40, np.uint32)
    want[9:20] += 1; want[17] += 1                      # F: m_4 + 1 = 9 .. m_12 = 19
    assert np.array_equal(tracks[0], want)


def hand_counts(mask):
    want = np.zeros((40, 8), np.uint32)
    fwd = {5: "A", 6: "C", 7: "G", 8: "T", 9: "A", 10: "C", 12: "A", 13: "C", 14: "G", 18: "T", 19: "T", 20: "T", 21: "T", 22: "T"}       # 11: the read's N
    rev = {12: "G", 13: "G", 14: "A", 16: "C", 18: "A", 19: "C", 20: "C"}                                                                # 17: the read's N
    if mask == 3:       # F: the read positions 0..2 and 17..19, its offsets 2, 17 and 18; R: r = 11 - offset, the offsets 9, 1 and 2
        for p in (5, 21, 22):
            del fwd[p]
        for p in (20, 12, 13):
            del rev[p]
    for p, l in fwd.items():
        want[p]["ACGT".index(l)] += 1
    for p, l in rev.items():
        want[p][4 + "ACGT".index(l)] += 1
    return want


@pytest.mark.parametrize("mask", [0, 3])
def test_the_hand_worked_records_counters(mask):
    c = hand_case()
    stats, tables, sites = gt.bases(*args(c), mask_ends=mask, min_depth=1, min_alt_count=1, min_alt_percent=0, skip=True)
    want = hand_counts(mask)
    assert np.array_equal(tables[0], want)
    assert stats[0][:3].tolist() == [2, 23, int(want.sum())] and int(want.sum()) == (21 if mask == 0 else 15)
    assert (hand_depth() >= want.sum(axis=1)).all()          # depth[i] >= the sum of position i's eight counters
    # the sites are read off the table as bases_model reads them
    ref = np.array(["ACGT".index(x) for x in c["seqs"][0]], np.int64)
    _, flags, _, _ = bm.classify(want, ref, 1, 1, 0)
    assert sites["pos"].tolist() == np.flatnonzero(flags & (bm.DIFFERS | bm.VARIABLE)).tolist() and all(np.array_equal(s["counts"], want[int(s["pos"])]) for s in sites)


def test_the_span_rule_against_its_literal_reading():
    """b is spanned iff at least w M columns lie strictly left of it and at least w at or right of it; the set is one interval inside
    pos + 1 .. pos + span - 1"""
    n = 0
    for seed in range(40):
        c, _ = ic.random_case(30_000 + seed)
        for r in c["grecs"]:
            segs = gt.segments(r, c["gops"])
            m = np.array(gt.columns_of(segs))
            assert len(m) == sum(g for _, _, g in segs) and (np.diff(m) > 0).all()
            for w in (1, 2, 5):
                literal = [b for b in range(0, 80) if (m < b).sum() >= w and (m >= b).sum() >= w]
                got = gt.spanned(segs, w)
                assert (got is None) == (len(m) < 2 * w) == (not literal)
                if got:
                    assert literal == list(range(got[0], got[1] + 1)) and int(r["pos"]) + 1 <= got[0] and got[1] <= int(r["pos"]) + int(r["span"]) - 1
                    n += 1
    assert n > 300


@pytest.mark.parametrize("seed", range(6))
def test_a_single_m_record_changes_nothing(seed):
    """every other counted record of a random pile-up as a gapped record of one M operation: the three models' outputs stay"""
    c = pc.random_set(70_000 + seed)
    u = (c["seqs"], c["ext"], c["off"], c["rec"], c["queries"])
    off, rec, grecs, gops = gt.single_m(*u, pick=lambda i: i % 2 == 0, min_seq_id=c["min_seq_id"], skip=c["skip"])
    g = (c["seqs"], c["ext"], off, rec, c["queries"], grecs, gops)
    kw = dict(min_seq_id=c["min_seq_id"], skip=c["skip"])
    assert len(grecs) > 0 and len(rec) + len(grecs) == len(c["rec"])
    want, got = dm.depth_stats(*u, 7, **kw), gt.depth_stats(*g, 7, **kw)
    assert np.array_equal(want[0], got[0]) and all(np.array_equal(a, b) for a, b in zip(want[1], got[1]))
    for anchor in (1, 5):
        want, got = brm.breaks_stats(*u, anchor, 6, 2, 30, **kw), gt.breaks_stats(*g, anchor, 6, 2, 30, **kw)
        assert np.array_equal(want[0], got[0]) and all(np.array_equal(a, b) for a, b in zip(want[1], got[1])) and np.array_equal(want[2], got[2])
    for mask in (0, 3):
        want, got = bm.bases(*u, mask, 2, 1, 10, **kw), gt.bases(*g, mask, 2, 1, 10, **kw)
        assert np.array_equal(want[0], got[0]) and all(np.array_equal(a, b) for a, b in zip(want[1], got[1])) and np.array_equal(want[2], got[2])


def test_without_gapped_records_the_models_are_the_ungapped_ones():
    c = ic.directed()
    u = (c["seqs"], c["ext"], c["off"], c["rec"], c["queries"])
    g = u + (c["grecs"][:0], c["gops"][:0])
    assert np.array_equal(dm.depth_stats(*u, 5, 0.0, True)[0], gt.depth_stats(*g, 5, 0.0, True)[0])
    assert np.array_equal(brm.breaks_stats(*u, 4, 10, skip=True)[2], gt.breaks_stats(*g, 4, 10, skip=True)[2])
    assert np.array_equal(bm.bases(*u, skip=True)[0], gt.bases(*g, skip=True)[0])


@pytest.mark.parametrize("strands", ["forward", "alternate"])
def test_the_planted_corpus(strands):
    """planted_case(7): four planted indels on a contig of 700 letters, reads of 80 letters every 3 positions.  At anchor 16 and edge 50
    the ungapped records alone give one break on every plant; with the 53 rescued records no boundary of the window is weak"""
    c, _, rescued = ic.planted_case(7, strands)
    assert rescued == len(c["grecs"]) == 53
    u = (c["seqs"], c["ext"], c["off"], c["rec"], c["queries"])
    for min_span in (1, 3):
        stats, _, breaks = brm.breaks_stats(*u, 16, 50, min_span, 0, 0.0, True)
        assert [(int(b["first"]), int(b["last"]), "JG"[int(b["flags"]) - 1]) for b in breaks] == [(135, 165, "J"), (274, 306, "G"), (416, 446, "J"), (545, 575, "J")]
        assert int(stats[0][6]) == 0
        stats, _, breaks = gt.breaks_stats(*args(c), 16, 50, min_span, 0, 0.0, True)
        assert len(breaks) == 0 and int(stats[0][3]) == 0 and int(stats[0][6]) == 9
    # every break sits on its plant: the contig position of the planted error lies inside the run
    at, shift = [], 0
    for kind, p, n in ic.PLANTS:
        at.append(p + shift)
        shift += n if kind == "extra" else -n
    _, _, breaks = brm.breaks_stats(*u, 16, 50, 1, 0, 0.0, True)
    assert all(int(b["first"]) <= x <= int(b["last"]) for b, x in zip(breaks, at))
    # the depth around the plants rises, and depth >= the counters everywhere
    du, dg = dm.depth_stats(*u, 50, 0.0, True), gt.depth_stats(*args(c), 50, 0.0, True)
    assert int(dg[0][0][5]) > int(du[0][0][5]) and (dg[1][0] >= du[1][0]).all()
    _, tables, _ = gt.bases(*args(c), skip=True)
    assert (dg[1][0] >= tables[0].sum(axis=1)).all()
    assert np.array_equal(dg[0][0][:2], gt.bases(*args(c), skip=True)[0][0][:2])
