"""tests/breaks_model.py on hand-computed cases: the definition of cdm_pileup_breaks (include/carpedeam_hip.h) one property at a time."""
import numpy as np

import breaks_model as bm
import depth_model as dm
import pileupcases as pc
from pileup_model import unorient

J, G = bm.JOIN, bm.GAP


def one(length, reads, extra=()):
    """a contig of `length` letters as query 0 with its identity record and one forward read per (qs, qe), each a target of its own"""
    rng = np.random.default_rng(length * 1000 + len(reads))
    seqs = [pc.rand_seq(rng, length)] + [pc.rand_seq(rng, qe - qs + 1) for qs, qe in reads]
    recs = [pc.identity(seqs, 0)] + [unorient(1 + i, qs, qe, 0, qe - qs, False, qe - qs + 1) for i, (qs, qe) in enumerate(reads)] + list(extra)
    return pc.case(seqs, {0: recs}, [0])


def run(c, anchor, edge, min_span=1, pct=0):
    return bm.breaks_stats(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"], anchor, edge, min_span, pct, c["min_seq_id"], c["skip"])


def rows(breaks):
    return [tuple(int(b[f]) for f in bm.FIELDS) for b in breaks]


def test_twelve_letters_four_reads():
    c = one(12, [(0, 5), (2, 9), (6, 11), (4, 7)])
    stats, tracks, breaks = run(c, 2, 2)
    # (0,5) spans 2..4, (2,9) spans 4..8, (6,11) spans 8..10, (4,7) spans 6
    assert tracks[0].tolist() == [0, 0, 1, 1, 2, 1, 2, 1, 2, 1, 1, 0] and tracks[0].dtype == np.uint32
    assert stats[0].tolist() == [4, 24, 9, 0, 0, 0, 1, 12] and len(breaks) == 0
    stats, tracks, breaks = run(c, 2, 2, min_span=2)
    assert stats[0].tolist() == [4, 24, 9, 6, 4, 4, 1, 12]
    assert rows(breaks) == [(0, 2, 3, 1, 0, 1, 2, J), (0, 5, 5, 1, 0, 3, 3, J), (0, 7, 7, 1, 0, 3, 3, J), (0, 9, 10, 1, 0, 2, 1, J)]
    assert breaks.dtype == bm.BREAK_DTYPE and breaks.dtype.itemsize == 32
    # a reverse record spans as its oriented form does
    rev = one(12, [(0, 5), (6, 11), (4, 7)], extra=[unorient(2, 2, 9, 0, 7, True, 8)])
    rev["seqs"][2] = "ACGTACGT"
    assert run(rev, 2, 2)[1][0].tolist() == [0, 0, 1, 1, 2, 1, 2, 1, 2, 1, 1, 0]


def test_the_shortest_spanning_read():
    w = 3
    short = one(20, [(5, 5 + 2 * w - 2)])              # L = 2 w - 1
    assert run(short, w, w)[1][0].sum() == 0
    exact = one(20, [(5, 5 + 2 * w - 1)])              # L = 2 w: boundary qs + w alone
    span = run(exact, w, w)[1][0]
    assert span.sum() == 1 and span[5 + w] == 1


def test_a_run_at_each_end_of_the_window():
    # one read 2..17 on 20 letters, anchor 1, edge 2: it spans 3..17; the window 2..18 is weak at 2 and at 18
    c = one(20, [(2, 17)])
    stats, tracks, breaks = run(c, 1, 2)
    assert tracks[0].tolist() == [0, 0, 0] + [1] * 15 + [0, 0]
    assert stats[0].tolist() == [1, 16, 17, 2, 2, 2, 0, 15]
    # a run of one boundary has no position first .. last - 1 to be uncovered: J, with the depth 0 on its outer side
    assert rows(breaks) == [(0, 2, 2, 0, 0, 0, 1, J), (0, 18, 18, 0, 0, 1, 0, J)]


def test_empty_windows():
    edge = 4
    for length in (1, 2 * edge - 1):
        c = one(length, [(0, length - 1)])
        stats, tracks, breaks = run(c, 1, edge)
        assert stats[0].tolist() == [1, length, 0, 0, 0, 0, 0, 0] and len(breaks) == 0 and len(tracks[0]) == length
    c = one(2 * edge, [(0, 2 * edge - 1)])             # 2 x edge letters: the one boundary b = edge
    assert run(c, 1, edge)[0][0].tolist() == [1, 8, 1, 0, 0, 0, 1, 1]
    assert run(one(2, [(0, 1)]), 1, 1)[0][0].tolist() == [1, 2, 1, 0, 0, 0, 1, 1]
    assert run(one(1, []), 1, 1)[0][0].tolist() == [0] * 8


def test_a_gap():
    # reads 0..9 and 14..29 on 30 letters: positions 10..13 have no read
    c = one(30, [(0, 9), (14, 29)])
    stats, tracks, breaks = run(c, 2, 2)
    # spans 2..8 and 16..28: weak 9..15; positions 9..14 of the run, of them 10..13 uncovered
    assert rows(breaks) == [(0, 9, 15, 0, 4, 1, 1, G)]
    assert stats[0].tolist() == [2, 26, 27, 7, 1, 0, 0, 20]


def test_adjacent_flanks_without_a_spanning_read():
    # reads 0..14 and 15..29 meet at boundary 15: every position covered, nothing spans 14..16 with two columns on either side
    c = one(30, [(0, 14), (15, 29)])
    stats, tracks, breaks = run(c, 2, 2)
    assert rows(breaks) == [(0, 14, 16, 0, 0, 1, 1, J)]
    assert stats[0].tolist() == [2, 30, 27, 3, 1, 1, 0, 24]
    # overlapping flanks that do not reach the anchor across the boundary are a join as well
    c = one(30, [(0, 16), (14, 29)])
    assert rows(run(c, 4, 4)[2]) == [(0, 14, 17, 0, 0, 1, 1, J)]


def test_the_percent_rule_at_equality():
    # depth 4 on 0..19 by four reads of which two span boundary 10 with anchor 5: span[10] * 100 == 50 * 4
    c = one(20, [(0, 19), (0, 19), (0, 12), (8, 19)])
    stats, tracks, breaks = run(c, 5, 10, 1, 50)
    assert tracks[0][10] == 2 and stats[0].tolist() == [4, 65, 1, 0, 0, 0, 2, 2]
    stats, tracks, breaks = run(c, 5, 10, 1, 51)
    assert stats[0].tolist() == [4, 65, 1, 1, 1, 1, 2, 2] and rows(breaks) == [(0, 10, 10, 2, 0, 4, 4, J)]
    assert run(c, 5, 10, 1, 0)[0][0][3] == 0 and run(c, 5, 10, 3, 0)[0][0][3] == 1
    # the smaller of the two depths counts: depth 2 | 1 at boundary 10, one record spans it
    c = one(20, [(0, 19), (0, 9)])
    assert run(c, 5, 10, 1, 100)[0][0][3] == 0


def test_reads_and_columns_are_the_depth_models():
    for name, make in pc.DIRECTED:
        c = make()
        stats, tracks, breaks = run(c, 3, 5)
        want, depth = dm.depth_stats(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"], 0, c["min_seq_id"], c["skip"])
        assert np.array_equal(stats[:, :2], want[:, :2]), name
        assert int(stats[:, 4].sum()) == len(breaks) and int(stats[:, 5].sum()) == int((breaks["flags"] == J).sum())
        for k, (s, d) in enumerate(zip(tracks, depth)):
            assert len(s) == len(d) and s[0] == 0
            if len(d) > 1:
                assert (s[1:] <= np.minimum(d[:-1], d[1:])).all(), (name, k)           # a spanning read covers both neighbours


def test_the_texts():
    c = one(30, [(0, 9), (14, 29)])
    stats, tracks, breaks = run(c, 2, 2)
    assert bm.tsv(["c1"], [7], [30], stats, breaks) == bm.HEADER + "c1\t7\t30\t2\t26\t27\t7\t1\t0\t0\t20\n#break\tc1\t10\t16\t0\t4\t1\t1\tG\n"
    assert bm.bedgraph(["c1"], tracks) == "c1\t0\t2\t0\nc1\t2\t9\t1\nc1\t9\t16\t0\nc1\t16\t29\t1\nc1\t29\t30\t0\n"
    s = c["seqs"][0]
    assert bm.split(["c1"], [s], breaks) == ">c1_1\n%s\n>c1_2\n%s\n" % (s[:9], s[15:])
    assert bm.split(["c1"], [s], breaks, min_piece=10) == ">c1_2\n%s\n" % s[15:]
    assert bm.split(["c1"], [s], breaks[:0]) == ">c1\n%s\n" % s
