"""tests/indels_model.py against itself and against planted answers: its two forms on random record sets, the planted-indel experiment
with the alignment of tests/gapped_model.py, the consensus rule on overlapping sites, one record per refusal, and the hand-computed
places of the directed case the device is held against."""
import numpy as np
import pytest

import indelcases as ic
import indels_model as im


def both(c, par):
    a = (c["seqs"], c["ext"], c["off"], c["rec"], c["queries"], c["grecs"], c["gops"], par)
    return im.indels_brute(*a), im.indels_sorted(*a)


def same(got, want):
    return (np.array_equal(got[0], want[0]) and len(got[1]) == len(want[1]) and all(np.array_equal(g, w) for g, w in zip(got[1], want[1]))
            and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]))


def test_the_two_forms_agree_on_random_record_sets():
    events = places = sites = shared = ties = 0
    for seed in range(300):
        c, par = ic.random_case(9000 + seed)
        assert im.check_records(c["seqs"], c["queries"], c["grecs"], c["gops"]) is None
        brute, fast = both(c, par)
        assert same(brute, fast), seed
        stats, _, recs, _ = brute
        events += int(stats[:, 3:5].sum()); places += int(stats[:, 7].sum()); sites += len(recs)
        shared += int((recs["count"] > 1).sum()); ties += int((recs["others"] > 0).sum())
        order = [(int(r["query"]), int(r["pos"]), int(r["info"]) & 15) for r in recs]
        assert order == sorted(order) and len(set(order)) == len(order)
        assert all(int(r["count"]) <= int(r["cross"]) for r in recs) and int(stats[:, 8].sum()) == len(recs)
    assert events > 2000 and places > 1000 and sites > 300 and shared > 100 and ties > 50


@pytest.mark.parametrize("strands", ["forward", "alternate"])
def test_the_planted_indels_give_back_the_genome(strands):
    c, genome, rescued = ic.planted_case(7, strands)
    contig = c["seqs"][0]
    assert contig != genome and len(contig) == len(genome) - 3 and rescued >= 40
    assert im.check_records(c["seqs"], c["queries"], c["grecs"], c["gops"]) is None
    stats, tracks, sites, letters = im.indels_sorted(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"], c["grecs"], c["gops"], im.Params(skip=True))
    major = sites[(sites["info"] >> 16) & im.MAJOR != 0]
    assert [(int(s["info"]) & 15, (int(s["info"]) >> 4) & 0xFFF) for s in major] == [(im.INS, 1), (im.DEL, 2), (im.INS, 1), (im.INS, 3)]
    assert all(2 * int(s["count"]) > int(s["cross"]) for s in major) and int(stats[0][9]) == 4
    if strands == "alternate":
        assert {int(r["flags"]) & 1 for r in c["grecs"]} == {0, 1}
    polished, applied = im.apply_consensus(contig, sites, letters)
    assert applied == 4 and polished == genome
    text = im.summary_tsv(["c"], [0], [contig], stats, sites, letters)
    assert text.split("\n")[1].split("\t")[-2:] == ["4", str(len(genome))]


def site(pos, kind, g, flags, letters_at=0):
    return (0, pos, kind | g << 4 | flags << 16, 5, 6, 0, g if kind == im.INS else 0, 0, letters_at)


def test_the_consensus_rule_on_overlapping_sites():
    SM, S = im.CALLED | im.SUPPORTED | im.MAJOR, im.CALLED | im.SUPPORTED
    contig = "acgtACGTNNacgtACGT"
    letters = np.array([3, 4, 0, 1], np.uint8)
    # a D inside a D is skipped, a D that begins where the first ends is taken, a supported site that is not major is left alone
    sites = np.array([site(2, im.DEL, 4, SM), site(4, im.DEL, 3, SM), site(6, im.DEL, 2, SM), site(12, im.DEL, 1, S)], im.INDEL_DTYPE)
    assert im.apply_consensus(contig, sites, letters) == ("ac" + "NNacgtACGT", 2)
    # an I at the cursor: right behind a deletion, and at a position with a deletion of its own (the I comes first)
    sites = np.array([site(2, im.DEL, 2, SM), site(4, im.INS, 2, SM, 0), site(8, im.INS, 2, SM, 2), site(8, im.DEL, 2, SM)], im.INDEL_DTYPE)
    assert im.apply_consensus(contig, sites, letters) == ("ac" + "TN" + "ACGT" + "AC" + "acgtACGT", 4)
    # an I inside a removed stretch is skipped; the first and the last position; every other byte as in the input
    sites = np.array([site(0, im.DEL, 3, SM), site(1, im.INS, 2, SM, 0), site(17, im.DEL, 1, SM)], im.INDEL_DTYPE)
    assert im.apply_consensus(contig, sites, letters) == ("tACGTNNacgtACG", 2)
    assert im.apply_consensus(contig, sites[:0], letters) == (contig, 0)
    assert im.consensus_fasta(["x"], [contig], sites, letters) == ">x\ntACGTNNacgtACG\n"
    assert im.sites_tsv(["x"], [contig], sites[1:2], letters) == "x\t2\tI\t2\tTN\t5\t6\t0\tSM\n"
    assert im.sites_tsv(["x"], [contig], sites[:1], letters) == "x\t1\tD\t3\tACG\t5\t6\t0\tSM\n"


SEQS, REFUSALS = ic.refusals()


def test_the_refusal_cases_start_from_a_record_that_passes():
    grecs, gops = ic.refusal_arrays([dict(query=0, target=1, pos=5, span=20, tstart=2, tlen=30, columns=22, n_ops=3, ops=0)], [10 << 2, 2 << 2 | 1, 10 << 2])
    assert im.check_records(SEQS, [0], grecs, gops) is None
    assert im.events_of(grecs[0], gops) == [(15, im.INS, 2, 12)]


@pytest.mark.parametrize("name,queries,recs,words,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_refusal_has_a_one_record_example(name, queries, recs, words, message):
    import re
    grecs, gops = ic.refusal_arrays(recs, words)
    got = im.check_records(SEQS, queries, grecs, gops)
    assert got is not None and re.search(message, "record %d: %s" % got), got


def test_the_directed_case_reaches_its_places():
    c = ic.directed()
    assert im.check_records(c["seqs"], c["queries"], c["grecs"], c["gops"]) is None
    par = im.Params(**ic.DIRECTED_PAR)
    stats, tracks, sites, letters = im.indels_sorted(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"], c["grecs"], c["gops"], par)
    by_place = {(int(s["pos"]), int(s["info"]) & 15): s for s in sites if int(s["query"]) == 0}
    for (p, kind), (g, count, cross, others, flags) in ic.DIRECTED_PLACES.items():
        assert int(tracks[0][p]) == cross, (p, int(tracks[0][p]))
        if not flags & im.SUPPORTED:
            assert (p, kind) not in by_place
            continue
        s = by_place[(p, kind)]
        assert (int(s["info"]) >> 4 & 0xFFF, int(s["count"]), int(s["cross"]), int(s["others"]), int(s["info"]) >> 16) == (g, count, cross, others, flags), (p, kind)
    assert len(by_place) == sum(1 for v in ic.DIRECTED_PLACES.values() if v[4] & im.SUPPORTED) and int(stats[0][7]) == len(ic.DIRECTED_PLACES)
    for p, want in list(ic.DIRECTED_LETTERS.items()) + [(100, "AGNC" + c["common"])]:
        assert im.letters_of(by_place[(p, im.INS)], letters) == want, p
    assert stats[1].tolist()[2:] == [5, 3, 2, 3, 4, 2, 1, 1] and stats[2].tolist() == [1, 18, 0, 0, 0, 0, 0, 0, 0, 0]
    assert len(c["seqs"][0]) == 520 and 1 not in c["queries"]
    # the extended target is what keeps the place at 330 at exactly min_percent
    loose = im.indels_sorted(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"], c["grecs"], c["gops"], im.Params(3, 2, 20, 0.0, False))
    assert int(loose[1][0][330]) == 11 and (330, im.DEL) not in {(int(s["pos"]), int(s["info"]) & 15) for s in loose[2] if int(s["query"]) == 0}
