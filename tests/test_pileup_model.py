"""tests/pileup_model.py, the statistic cdm_pileup_profile is held against: hand-counted tables, and a second implementation that is
literal on purpose - it builds the reverse complement of a read as a string and looks positions up in lists, with no index arithmetic."""
import numpy as np
import pytest

import pileup_model as pm
import pileupcases as pc


def literal(c):
    """the same tables from strings: the mapped view of every sequence as a string over ACGTN, the oriented target as the read or its
    reverse complement, the position of every oriented letter in the read looked up in a list"""
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    idx = {"A": 0, "C": 1, "G": 2, "T": 3}
    canon = ["".join("N" if pm.letter(ch)[1] else "ACGT"[pm.letter(ch)[0]] for ch in s) for s in c["seqs"]]
    P = c["ends"]
    counts = np.zeros((len(c["queries"]), 2, P, 4, 4), np.uint64)
    reads, columns = np.zeros(len(c["queries"]), np.uint64), np.zeros(len(c["queries"]), np.uint64)
    for k, q in enumerate(c["queries"]):
        for r in c["rec"][int(c["off"][q]):int(c["off"][q + 1])]:
            t = int(r["target"])
            if t == q or r["seq_id"] < np.float32(c["min_seq_id"]) or (c["skip"] and c["ext"][t]):
                continue
            read = canon[t]
            from_5p = list(range(len(read)))                # distance of every letter of the read from its 5' end
            from_3p = from_5p[::-1]
            rev = r["q_start"] > r["q_end"]
            if rev:                                         # the query's window against the reverse complement of the read
                window = canon[q][r["q_end"]:r["q_start"] + 1]
                oriented = "".join(comp[ch] for ch in reversed(read))
                d5_of, d3_of = from_5p[::-1], from_3p[::-1]
                first = len(read) - 1 - r["db_end"]
            else:
                window = canon[q][r["q_start"]:r["q_end"] + 1]
                oriented, d5_of, d3_of, first = read, from_5p, from_3p, r["db_start"]
            reads[k] += 1
            columns[k] += len(window)
            for j, qch in enumerate(window):
                tch = oriented[first + j]
                if qch == "N" or tch == "N":
                    continue
                # in the read's own orientation: its own letter, and the query letter as its strand sees it
                y, x = (comp[tch], comp[qch]) if rev else (tch, qch)
                d5, d3 = d5_of[first + j], d3_of[first + j]
                if d5 < P:
                    counts[k, 0, d5, idx[x], idx[y]] += 1
                if d3 < P:
                    counts[k, 1, d3, idx[x], idx[y]] += 1
    return counts, reads, columns


def run_model(c):
    return pm.profile(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"], c["ends"], c["min_seq_id"], c["skip"])


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_forward_read_by_hand():
    """query ACGTACGTAC, read GTTC on query positions 2..5 (GTAC), ends = 2"""
    c = pc.case(["ACGTACGTAC", "GTTC"], {0: [(0, 0, 0, 0, 9, 0, 9, 1.0), (1, 0, 0, 2, 5, 0, 3, 1.0)]}, [0], ends=2)
    counts, reads, columns = run_model(c)
    want = np.zeros((1, 2, 2, 4, 4), np.uint64)
    want[0, 0, 0, 2, 2] = 1         # 5' distance 0: query G under read G
    want[0, 0, 1, 3, 3] = 1         # 5' distance 1: T under T
    want[0, 1, 0, 1, 1] = 1         # 3' distance 0: C under C
    want[0, 1, 1, 0, 3] = 1         # 3' distance 1: query A under read T
    assert np.array_equal(counts, want) and reads[0] == 1 and columns[0] == 4


def test_reverse_read_by_hand():
    """the read TGTA is the reverse complement of TACA; on the query's TACG (positions 3..6) its strand sees the query as CGTA:
    read position 0 (T) stands over query position 6 (G, seen as C): a C->T at the read's 5' end"""
    c = pc.case(["ACGTACGTAC", "TGTA"], {0: [(0, 0, 0, 0, 9, 0, 9, 1.0), pm.unorient(1, 3, 6, 0, 3, True, 4)]}, [0], ends=3)
    assert tuple(c["rec"][1])[3:7] == (6, 3, 0, 3)
    counts, reads, columns = run_model(c)
    want = np.zeros((1, 2, 3, 4, 4), np.uint64)
    # read positions 0..3 = T G T A over the query as its strand sees it, C G T A
    want[0, 0, 0, 1, 3] = 1
    want[0, 0, 1, 2, 2] = 1
    want[0, 0, 2, 3, 3] = 1
    want[0, 1, 0, 0, 0] = 1         # 3' distance 0: read position 3
    want[0, 1, 1, 3, 3] = 1
    want[0, 1, 2, 2, 2] = 1
    assert np.array_equal(counts, want) and reads[0] == 1 and columns[0] == 4


def test_n_columns_and_gates_by_hand():
    """an N on either side counts in `columns` only; the identity record, a record below the threshold and an extended target count
    nowhere; a lower-case letter and an IUPAC code count as what they map to"""
    seqs = ["ACNTAcGT", "ACGN", "AYG", "ACGT", "ACGT"]
    recs = [(0, 0, 0, 0, 7, 0, 7, 1.0), (1, 0, 0, 0, 3, 0, 3, 1.0), (2, 0, 0, 4, 6, 0, 2, 0.95), (3, 0, 0, 0, 3, 0, 3, 0.5), (4, 0, 0, 0, 3, 0, 3, 1.0)]
    c = pc.case(seqs, {0: recs}, [0], ends=4, ext=[1, 0, 0, 0, 1], min_seq_id=0.9, skip=True)
    counts, reads, columns = run_model(c)
    want = np.zeros((1, 2, 4, 4, 4), np.uint64)
    for d5, d3, x, y in ((0, 3, 0, 0), (1, 2, 1, 1)):       # ACGN on ACNT: columns 2 (query N) and 3 (read N) are left out
        want[0, 0, d5, x, y] += 1
        want[0, 1, d3, x, y] += 1
    for d5, d3, x, y in ((0, 2, 0, 0), (1, 1, 1, 1), (2, 0, 2, 2)):      # AYG on AcG: c is C, Y is C
        want[0, 0, d5, x, y] += 1
        want[0, 1, d3, x, y] += 1
    assert np.array_equal(counts, want) and reads[0] == 2 and columns[0] == 7


def test_short_read_lands_in_both_tables():
    c = pc.one_query_of_40()
    counts, _, _ = run_model(pc.case(c["seqs"], {0: [pm.unorient(5, 17, 21, 0, 4, False, 5)]}, [0], 16))
    assert counts[0, 0].sum() == 5 and counts[0, 1].sum() == 5
    assert [int(counts[0, 0, d].sum()) for d in range(16)] == [1] * 5 + [0] * 11 == [int(counts[0, 1, d].sum()) for d in range(16)]


@pytest.mark.parametrize("name,make", pc.DIRECTED, ids=[n for n, _ in pc.DIRECTED])
def test_model_against_the_literal_implementation(name, make):
    c = make()
    got = run_model(c)
    assert same(got, literal(c))
    if name not in ("query_lists", "mixed_flags_skip", "mixed_flags_keep"):
        assert got[1].sum() > 0 and got[0].sum() > 0          # (the case counts something)


def test_a_query_with_only_its_identity_record_is_all_zeros():
    c = pc.query_lists()
    counts, reads, columns = run_model(c)
    k = c["queries"].index(7)
    assert counts[k].sum() == 0 and reads[k] == 0 and columns[k] == 0 and reads.sum() > 0


def test_the_threshold_takes_the_record_that_equals_it():
    counts, reads, columns = run_model(pc.threshold())
    assert reads[0] == 2 and columns[0] == 60


def test_random_sets_against_the_literal_implementation():
    for seed in range(12):
        c = pc.random_set(seed, max_queries=3)
        assert same(run_model(c), literal(c)), seed


def test_tsv_layout():
    counts = np.zeros((1, 2, 2, 4, 4), np.uint64)
    counts[0, 0, 0, 1] = [1, 2, 3, 4]
    counts[0, 1, 1, 2] = [5, 6, 7, 8]
    text = pm.tsv(["c1"], [7], [400], counts, [9], [99])
    assert text == "name\tkey\tlength\treads\tcolumns\t5p_C_1\t5p_CT_1\t3p_G_1\t3p_GA_1\t5p_C_2\t5p_CT_2\t3p_G_2\t3p_GA_2\nc1\t7\t400\t9\t99\t10\t4\t0\t0\t0\t0\t26\t5\n"
