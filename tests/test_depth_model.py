"""tests/depth_model.py against a brute-force loop over positions (every position asks every record whether it covers it) on the
directed and random inputs of tests/pileupcases.py, and against one answer computed by hand."""
import numpy as np
import pytest

import depth_model as dm
import pileup_model as pm
import pileupcases as pc


def brute(c, edge):
    """position by position: depth[i] = the number of counted records with qs <= i <= qe, then the figures by their definitions"""
    thr = np.float32(c["min_seq_id"])
    stats, tracks = [], []
    for q in c["queries"]:
        length = len(c["seqs"][q])
        spans = []
        for r in c["rec"][int(c["off"][q]):int(c["off"][q + 1])]:
            t = int(r["target"])
            if t == q or not (np.float32(r["seq_id"]) >= thr) or (c["skip"] and c["ext"][t]):
                continue
            qs, qe = sorted((int(r["q_start"]), int(r["q_end"])))         # orient() swaps a reverse record's query coordinates
            spans.append((qs, qe))
        depth = [sum(1 for qs, qe in spans if qs <= i <= qe) for i in range(length)]
        inside = [i for i in range(length) if length <= 2 * edge or edge <= i <= length - 1 - edge]
        stats.append([len(spans), sum(qe - qs + 1 for qs, qe in spans), sum(1 for d in depth if d >= 1), len(inside), sum(1 for i in inside if depth[i] >= 1),
                      sum(depth[i] for i in inside), sum(depth[i] ** 2 for i in inside), max([depth[i] for i in inside], default=0)])
        tracks.append(depth)
    return stats, tracks


def model(c, edge):
    return dm.depth_stats(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"], edge, c["min_seq_id"], c["skip"])


def check(c, edge, what):
    stats, tracks = model(c, edge)
    want_stats, want_tracks = brute(c, edge)
    assert stats.dtype == np.uint64 and stats.shape == (len(c["queries"]), 8)
    assert stats.tolist() == want_stats, what
    assert [t.tolist() for t in tracks] == want_tracks, what
    assert all(t.dtype == np.uint32 for t in tracks)
    # reads and columns are the profile's, and the depth of the whole contig adds up to columns
    _, reads, columns = pm.profile(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"], 1, c["min_seq_id"], c["skip"])
    assert np.array_equal(stats[:, 0], reads) and np.array_equal(stats[:, 1], columns), what
    assert [int(t.sum()) for t in tracks] == columns.tolist(), what
    return stats


@pytest.mark.parametrize("edge", [0, 5])
@pytest.mark.parametrize("name,make", pc.DIRECTED, ids=[n for n, _ in pc.DIRECTED])
def test_directed_cases(name, make, edge):
    check(make(), edge, name)


@pytest.mark.parametrize("edge", [0, 5])
def test_random_sets(edge):
    counted = 0
    for seed in range(50):
        c = pc.random_set(20_000 + seed, max_queries=3)
        counted += int(check(c, edge, "seed %d" % seed)[:, 0].sum())
    assert counted > 1000


def test_the_known_answer():
    c = pc.one_query_of_40()
    depth = [2, 2, 3, 4, 4, 5, 5, 4, 4, 4, 5, 5, 4, 4, 4, 4, 4, 5, 5, 4, 4, 4, 3, 3, 3, 2, 2, 2, 2, 2, 3, 3, 3, 2, 2, 1, 1, 1, 1, 1]
    stats, tracks = model(c, 0)
    assert tracks[0].tolist() == depth
    assert dict(zip(dm.NAMES, stats[0].tolist())) == dict(reads=9, columns=126, breadth=40, window=40, covered=40, sum=126, sumsq=462, max=5)
    stats, tracks = model(c, 5)
    assert tracks[0].tolist() == depth
    assert dict(zip(dm.NAMES, stats[0].tolist())) == dict(reads=9, columns=126, breadth=40, window=30, covered=30, sum=106, sumsq=408, max=5)


def test_the_window_rule():
    assert dm.window_of(10, 5) == (0, 9) and dm.window_of(11, 5) == (5, 5) and dm.window_of(9, 5) == (0, 8) and dm.window_of(1, 0) == (0, 0)
    assert dm.window_of(40, 5) == (5, 34)


def test_tsv_and_bedgraph_text():
    st1 = np.array([[9, 126, 40, 30, 30, 106, 408, 5], [0, 0, 0, 7, 0, 0, 0, 0]], np.uint64)
    st2 = st1 + np.uint64(1)
    assert dm.tsv_header(1) == "name\tkey\tlength\twindow\treads_1\tcolumns_1\tbreadth_1\tcovered_1\tsum_1\tsumsq_1\tmax_1\n"
    assert dm.tsv_header(2).rstrip("\n").split("\t")[11:] == ["reads_2", "columns_2", "breadth_2", "covered_2", "sum_2", "sumsq_2", "max_2"]
    text = dm.tsv(["a", "b"], [3, 4], [40, 7], [st1, st2])
    assert text.split("\n")[1] == "a\t3\t40\t30\t9\t126\t40\t30\t106\t408\t5\t10\t127\t41\t31\t107\t409\t6"
    assert text.split("\n")[2].split("\t")[:5] == ["b", "4", "7", "7", "0"]
    bg = dm.bedgraph(["a", "b"], [np.array([0, 0, 2, 2, 2, 1], np.uint32), np.array([3], np.uint32)])
    assert bg == "a\t0\t2\t0\na\t2\t5\t2\na\t5\t6\t1\nb\t0\t1\t3\n"
