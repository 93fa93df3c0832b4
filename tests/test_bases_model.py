"""tests/bases_model.py against a second, literal implementation of cdm_pileup_bases' definition (one column at a time, on strings) and
against a case counted by hand.  No device is involved: the model is what the device is held against."""
import numpy as np
import pytest

import bases_model as bm
import pileupcases as pc
from pileup_model import letter, orient, unorient


def literal(c, queries, mask_ends, min_depth, min_alt_count, min_alt_percent):
    """the definition, column by column -> (stats rows, counts per query, site tuples)"""
    seqs, ext, off, rec = c["seqs"], c["ext"], c["off"], c["rec"]
    thr = np.float32(c["min_seq_id"])
    stats, tables, sites = [], [], []
    for k, q in enumerate(queries):
        counts = [[0] * 8 for _ in seqs[q]]
        reads = columns = 0
        for r in rec[int(off[q]):int(off[q + 1])]:
            t = int(r["target"])
            if t == q or not (np.float32(r["seq_id"]) >= thr) or (c["skip"] and ext[t]):
                continue
            read = seqs[t]
            t_len = len(read)
            qs, qe, ds, de, rev = orient(r, t_len)
            reads += 1
            for i in range(qs, qe + 1):
                columns += 1
                op = ds + (i - qs)
                p = t_len - 1 - op if rev else op
                b, is_n = letter(read[p])
                if is_n:
                    continue
                if mask_ends > 0 and (p < mask_ends or t_len - 1 - p < mask_ends):
                    continue
                counts[i][(4 if rev else 0) + (3 - b if rev else b)] += 1
        row = [reads, columns, 0, 0, 0, 0, 0, 0]
        for i, cnt in enumerate(counts):
            t4 = [cnt[b] + cnt[4 + b] for b in range(4)]
            d = sum(t4)
            code, is_n = letter(seqs[q][i])
            ref = 4 if is_n else code
            top = max(t4)
            tied = [b for b in range(4) if t4[b] == top]
            major = ref if ref in tied else tied[0]
            others = [t4[b] for b in range(4) if b != major]
            second = max(others)
            flags = 0
            if d >= min_depth:
                flags |= bm.CALLED
                if major != ref and all(t4[major] > o for o in others):
                    flags |= bm.DIFFERS
                if second >= min_alt_count and second * 100 >= min_alt_percent * d:
                    flags |= bm.VARIABLE
            row[2] += d
            if ref != 4:
                row[3] += d - t4[ref]
            row[4] += bool(flags & bm.CALLED)
            row[5] += bool(flags & bm.DIFFERS)
            row[6] += bool(flags & bm.VARIABLE)
            if flags & (bm.DIFFERS | bm.VARIABLE):
                row[7] += 1
                sites.append((k, i, ref | major << 4 | flags << 8, list(cnt)))
        stats.append(row)
        tables.append(counts)
    return stats, tables, sites


def compare(c, queries, mask_ends, min_depth, min_alt_count, min_alt_percent, what):
    stats, tables, sites = bm.bases(c["seqs"], c["ext"], c["off"], c["rec"], queries, mask_ends, min_depth, min_alt_count, min_alt_percent, c["min_seq_id"], c["skip"])
    w_stats, w_tables, w_sites = literal(c, queries, mask_ends, min_depth, min_alt_count, min_alt_percent)
    assert stats.dtype == np.uint64 and stats.tolist() == w_stats, what
    assert len(tables) == len(w_tables)
    for g, w in zip(tables, w_tables):
        assert g.dtype == np.uint32 and g.shape == (len(w), 8) and g.tolist() == w, what
    assert [(int(s["query"]), int(s["pos"]), int(s["info"]), s["counts"].tolist()) for s in sites] == w_sites, what
    return stats


@pytest.mark.parametrize("mask_ends", [0, 3])
@pytest.mark.parametrize("name,make", pc.DIRECTED, ids=[n for n, _ in pc.DIRECTED])
def test_directed_cases(name, make, mask_ends):
    c = make()
    compare(c, c["queries"], mask_ends, 3, 2, 20, name)


def test_random_sets():
    rng = np.random.default_rng(90)
    flagged = 0
    for seed in range(50):
        c = pc.random_set(50_000 + seed, max_queries=2)
        mask = int(rng.choice([0, 1, 5, 64]))
        stats = compare(c, c["queries"], mask, int(rng.integers(1, 5)), int(rng.integers(1, 3)), int(rng.choice([0, 20, 50])), "seed %d" % seed)
        flagged += int(stats[:, 7].sum())
    assert flagged > 300


def hand_case():
    """ACGTNACGTACG under four reads: two forward from the left end, one reverse across the N, one with an N of its own on the contig's N"""
    seqs = ["ACGTNACGTACG", "ACGTT", "CGTAA", "GGTAAC", "TNAC"]
    recs = [pc.identity(seqs, 0),
            unorient(1, 0, 4, 0, 4, False, 5),          # A C G T T on 0..4
            unorient(2, 1, 5, 0, 4, False, 5),          # C G T A A on 1..5
            unorient(3, 2, 7, 0, 5, True, 6),           # reversed: G T T A C C on 2..7 (C against the contig's G at 7)
            unorient(4, 3, 6, 0, 3, False, 4)]          # T N A C on 3..6
    return pc.case(seqs, {0: recs}, [0])


def test_the_hand_counted_case():
    c = hand_case()
    stats, tables, sites = bm.bases(c["seqs"], c["ext"], c["off"], c["rec"], [0], 0, 3, 1, 20)
    #            A  C  G  T  a  c  g  t
    want = [[1, 0, 0, 0, 0, 0, 0, 0],        # 0
            [0, 2, 0, 0, 0, 0, 0, 0],        # 1
            [0, 0, 2, 0, 0, 0, 1, 0],        # 2
            [0, 0, 0, 3, 0, 0, 0, 1],        # 3
            [1, 0, 0, 1, 0, 0, 0, 1],        # 4: the contig's N; the fourth read's N is left out
            [2, 0, 0, 0, 1, 0, 0, 0],        # 5
            [0, 1, 0, 0, 0, 1, 0, 0],        # 6
            [0, 0, 0, 0, 0, 1, 0, 0]] + [[0] * 8] * 4
    assert tables[0].tolist() == want
    # reads, columns 5 + 5 + 6 + 4, bases = columns - the read's N, mismatches: the C on G at 7 (the N position is excluded),
    # called: 2, 3, 4, 5; the N position differs (T 2 > A 1) and is variable (1 >= 1, 100 >= 20 * 3)
    assert stats[0].tolist() == [4, 20, 19, 1, 4, 1, 1, 1]
    assert len(sites) == 1
    s = sites[0]
    assert (int(s["query"]), int(s["pos"]), int(s["info"])) == (0, 4, 4 | 3 << 4 | 7 << 8) and s["counts"].tolist() == want[4]
    assert compare(c, [0], 0, 3, 1, 20, "hand").tolist() == stats.tolist()
    # a second allele of 1 in 3 is 33 %: not variable at 34 %, nor with a count of 2 asked for
    assert bm.bases(c["seqs"], c["ext"], c["off"], c["rec"], [0], 0, 3, 1, 34)[0][0].tolist() == [4, 20, 19, 1, 4, 1, 0, 1]
    assert bm.bases(c["seqs"], c["ext"], c["off"], c["rec"], [0], 0, 3, 2, 20)[0][0].tolist() == [4, 20, 19, 1, 4, 1, 0, 1]
    # mask_ends 1 takes the first and last letter of every read: 8 columns, the mismatch at 7 among them
    st1, t1, _ = bm.bases(c["seqs"], c["ext"], c["off"], c["rec"], [0], 1, 3, 1, 20)
    assert st1[0][:4].tolist() == [4, 20, 11, 0]
    assert t1[0][4].tolist() == [1, 0, 0, 0, 0, 0, 0, 1] and t1[0][0].tolist() == [0] * 8 and t1[0][7].tolist() == [0] * 8


def test_the_texts():
    c = hand_case()
    stats, _, sites = bm.bases(c["seqs"], c["ext"], c["off"], c["rec"], [0], 0, 3, 1, 20)
    assert bm.summary_tsv(["ctg"], [7], [12], stats) == "name\tkey\tlength\treads\tcolumns\tbases\tmismatches\tcalled\tdiffers\tvariable\nctg\t7\t12\t4\t20\t19\t1\t4\t1\t1\n"
    assert bm.sites_tsv(["ctg"], sites) == "ctg\t5\tN\tT\tDV\t3\t1\t0\t0\t1\t0\t0\t0\t1\n"
    assert bm.consensus_fasta(["ctg"], ["ACGTNACGTACG"], sites) == ">ctg\nACGTTACGTACG\n"
    assert bm.sites_tsv(["ctg"], sites[:0]) == "" and bm.summary_tsv([], [], [], stats[:0]) == bm.SUMMARY_HEADER
