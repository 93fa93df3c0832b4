"""tests/map_model.py against hand-computed answers, one property each: the MD strings, N columns, a reverse record's SEQ and clips,
the primary rules, and what sam_check has to reject."""
import pytest

import map_model as mm
from pileup_model import unorient
from pileupcases import case, identity

#    0         1         2
#    012345678901234567890123456789
Q = "ACGTTGCAAGGCTATCCGATTGACCTAGGA"
COMP = str.maketrans("ACGT", "TGCA")


def run(seqs, per_query, queries, **kw):
    c = case(seqs, per_query, queries)
    return mm.map_records(c["seqs"], c["ext"], c["off"], c["rec"], queries, **kw)


def single(read, qs, ds=0, n=None, rev=False, query=Q):
    """one read with one record on one query -> (stats row, record, its words)"""
    n = len(read) - ds if n is None else n
    seqs = [query, read]
    stats, recs, mism = run(seqs, {0: [identity(seqs, 0), unorient(1, qs, qs + n - 1, ds, ds + n - 1, rev, len(read))]}, [0])
    assert len(recs) == 1 and int(recs[0]["mm"]) == 0 and len(mism) == int(recs[0]["nm"])
    return stats[0].tolist(), recs[0], mism.tolist()


def word(c, ref, read):
    return c | "ACGTN".index(ref) << 24 | "ACGTN".index(read) << 28


def test_the_record_layout():
    assert mm.MAP_DTYPE.itemsize == 40 and mm.MAP_DTYPE.names == ("query", "target", "pos", "columns", "tstart", "tlen", "nm", "flags", "mm")


def test_md_of_a_perfect_match():
    stats, r, words = single(Q[5:15], 5)
    assert tuple(int(x) for x in r) == (0, 1, 5, 10, 0, 10, 0, 0, 0) and words == [] and stats == [1, 10, 0, 1]
    assert mm.md_of(words, 10) == "10"


def test_md_of_a_mismatch_in_the_first_column():
    stats, r, words = single("C" + Q[1:10], 0)
    assert words == [word(0, "A", "C")] and int(r["nm"]) == 1 and mm.md_of(words, 10) == "0A9" and stats == [1, 10, 1, 1]


def test_md_of_a_mismatch_in_the_last_column():
    _, r, words = single(Q[4:13] + "C", 4)
    assert words == [word(9, "A", "C")] and mm.md_of(words, 10) == "9A0"


def test_md_of_two_adjacent_mismatches():
    _, r, words = single(Q[19:22] + "GT" + Q[24:29], 19)
    assert words == [word(3, "A", "G"), word(4, "C", "T")] and int(r["nm"]) == 2 and mm.md_of(words, 10) == "3A0C5"


def test_md_of_an_all_mismatch_record():
    _, r, words = single("CGTA", 0)          # on ACGT
    assert words == [word(0, "A", "C"), word(1, "C", "G"), word(2, "G", "T"), word(3, "T", "A")] and int(r["nm"]) == 4
    assert mm.md_of(words, 4) == "0A0C0G0T0"


def test_an_n_on_either_side_is_a_mismatch_and_shows_as_the_ref_letter():
    q = Q[:7] + "N" + Q[8:]
    _, r, words = single(Q[5:15], 5, query=q)                   # the query's N under the read's A
    assert words == [word(2, "N", "A")] and mm.md_of(words, 10) == "2N7"
    _, r, words = single(Q[5:8] + "N" + Q[9:15], 5)             # the read's N over the query's A
    assert words == [word(3, "A", "N")] and mm.md_of(words, 10) == "3A6"
    _, r, words = single(Q[5:7] + "N" + Q[8:15], 5, query=q)    # an N over an N matches nothing either
    assert words == [word(2, "N", "N")] and int(r["nm"]) == 1
    _, r, words = single(Q[5:7] + "x" + Q[8:10] + "r" + Q[11:15], 5)       # letters beyond ACGTN: x is an N, r stands for G
    assert words == [word(2, "A", "N")] and mm.mapped("xrYn") == "NGCN"


def sam_lines(seqs, names, recs, mism, n_contigs, **kw):
    text = mm.sam_text(names[:n_contigs], [len(s) for s in seqs[:n_contigs]], lambda t: names[t], lambda t: seqs[t], recs, mism, **kw)
    return text, [l.split("\t") for l in text.split("\n")[:-1] if not l.startswith("@")]


def test_a_reverse_record_seq_and_clips():
    oriented = "GGG" + Q[5:9] + "T" + Q[10:13] + "T"              # 3 clipped, 8 columns with a mismatch in column 4, 1 clipped
    read = oriented.translate(COMP)[::-1]
    seqs = [Q, read]
    stats, recs, mism = run(seqs, {0: [identity(seqs, 0), unorient(1, 5, 12, 3, 10, True, 12)]}, [0])
    assert tuple(int(x) for x in recs[0]) == (0, 1, 5, 8, 3, 12, 1, mm.REVERSE, 0) and mism.tolist() == [word(4, "G", "T")]
    text, lines = sam_lines(seqs, ["ctg", "r1"], recs, mism, 1, read_group="lib1")
    assert text.startswith("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:ctg\tLN:30\n@RG\tID:lib1\n@PG\tID:carpedeam\tPN:carpedeam\n")
    assert lines == [["r1", "16", "ctg", "6", "255", "3S8M1S", "*", "0", "0", oriented, "*", "NM:i:1", "MD:Z:4G3", "RG:Z:lib1"]]
    assert mm.sam_check(text, {"ctg": Q}) == 1


def two_records(first, second, queries=(0,)):
    """read 2 with the records `first` and `second` (query, qs, columns) in that order in the set -> the flags in output order"""
    seqs = [Q, Q[::-1], Q[3:15]]
    per = {0: [identity(seqs, 0)], 1: [identity(seqs, 1)]}
    for q, qs, n in (first, second):
        per[q].append(unorient(2, qs, qs + n - 1, 0, n - 1, False, 12))
    stats, recs, _ = run(seqs, per, list(queries))
    return [(int(r["query"]), int(r["pos"]), int(r["flags"])) for r in recs], stats[:, 3].tolist()


def test_primary_more_columns_wins():
    assert two_records((0, 3, 8), (0, 1, 10)) == ([(0, 1, 0), (0, 3, mm.SECONDARY)], [1])          # the later, longer record; output by pos


def test_primary_equal_columns_gives_the_earlier_record():
    assert two_records((0, 6, 8), (0, 2, 8)) == ([(0, 2, mm.SECONDARY), (0, 6, 0)], [1])


def test_primary_of_a_read_on_two_contigs():
    assert two_records((0, 3, 8), (1, 0, 9), queries=(0, 1)) == ([(0, 3, mm.SECONDARY), (1, 0, 0)], [0, 1])
    assert two_records((0, 3, 8), (1, 0, 9), queries=(1, 0)) == ([(0, 0, 0), (1, 3, mm.SECONDARY)], [1, 0])       # query: the index into the list


def test_primary_of_a_read_twice_on_one_contig_at_one_position():
    assert two_records((0, 3, 8), (0, 3, 8)) == ([(0, 3, 0), (0, 3, mm.SECONDARY)], [1])            # stable: the set's order


def test_an_unlisted_query_takes_no_part_in_the_choice():
    assert two_records((0, 3, 8), (1, 0, 12), queries=(0,)) == ([(0, 3, 0)], [1])


def test_filters_are_those_of_the_other_reductions():
    seqs = [Q, Q[3:15], Q[5:20]]
    per = {0: [identity(seqs, 0), unorient(1, 3, 14, 0, 11, False, 12, 0.8), unorient(2, 5, 19, 0, 14, False, 15, 0.95)]}
    c = case(seqs, per, [0], ext=[1, 0, 1])
    assert len(mm.map_records(c["seqs"], c["ext"], c["off"], c["rec"], [0])[1]) == 2
    assert mm.map_records(c["seqs"], c["ext"], c["off"], c["rec"], [0], min_seq_id=0.9)[1]["target"].tolist() == [2]
    assert mm.map_records(c["seqs"], c["ext"], c["off"], c["rec"], [0], skip=True)[1]["target"].tolist() == [1]


@pytest.fixture(scope="module")
def good():
    """two contigs, three reads, four lines: mismatches, a reverse record, a secondary line"""
    c2 = Q[::-1]
    r3 = (c2[4:10] + "A" + c2[11:16]).translate(COMP)[::-1]       # reverse on the second contig, a mismatch in column 6 (ref T)
    seqs = [Q, c2, Q[2:6] + "A" + Q[7:14], Q[10:22], r3]
    assert c2[10] == "T"
    per = {0: [identity(seqs, 0), unorient(3, 10, 21, 0, 11, False, 12), unorient(2, 2, 13, 0, 11, False, 12), unorient(3, 12, 19, 2, 9, False, 12)],
           1: [identity(seqs, 1), unorient(4, 4, 15, 0, 11, True, 12)]}
    stats, recs, mism = run(seqs, per, [0, 1])
    text, lines = sam_lines(seqs, ["c1", "c2", "ra", "rb", "rc"], recs, mism, 2)
    assert [l[0] for l in lines] == ["ra", "rb", "rb", "rc"] and [l[1] for l in lines] == ["0", "0", "256", "16"] and [l[3] for l in lines] == ["3", "11", "13", "5"]
    assert [l[5] for l in lines] == ["12M", "12M", "2S8M2S", "12M"] and [l[12] for l in lines] == ["MD:Z:4C7", "MD:Z:12", "MD:Z:8", "MD:Z:6T5"]
    assert stats.tolist() == [[3, 32, 1, 2], [1, 12, 1, 1]]
    return text, {"c1": Q, "c2": c2}, (seqs, recs, mism)


def test_sam_check_accepts_the_model_text(good):
    text, contigs, (seqs, recs, mism) = good
    assert mm.sam_check(text, contigs) == 3
    only, lines = sam_lines(seqs, ["c1", "c2", "ra", "rb", "rc"], recs, mism, 2, primary_only=True)
    assert len(lines) == 3 and mm.sam_check(only, contigs) == 3


def test_sam_check_rejects_a_changed_md_letter(good):
    text, contigs, _ = good
    assert text.count("MD:Z:4C7") == 1
    with pytest.raises(ValueError, match="line 5: SEQ and MD do not rebuild"):
        mm.sam_check(text.replace("MD:Z:4C7", "MD:Z:4G7"), contigs)
    with pytest.raises(ValueError, match="line 5: a mismatch column that matches"):
        mm.sam_check(text.replace("MD:Z:4C7", "MD:Z:4A7"), contigs)
    with pytest.raises(ValueError, match="line 5: NM is not"):
        mm.sam_check(text.replace("NM:i:1\tMD:Z:4C7", "NM:i:2\tMD:Z:4C7"), contigs)


def test_sam_check_rejects_two_swapped_lines(good):
    text, contigs, _ = good
    lines = text.split("\n")
    lines[5], lines[6] = lines[6], lines[5]
    with pytest.raises(ValueError, match="line 7: not sorted"):
        mm.sam_check("\n".join(lines), contigs)


def test_sam_check_rejects_a_second_primary(good):
    text, contigs, _ = good
    assert text.count("\t256\t") == 1
    with pytest.raises(ValueError, match="rb has 2 lines without 256"):
        mm.sam_check(text.replace("\t256\t", "\t0\t"), contigs)
    with pytest.raises(ValueError, match="rc has 0 lines without 256"):
        mm.sam_check(text.replace("rc\t16\t", "rc\t272\t"), contigs)


def test_sam_check_rejects_wrong_clips(good):
    text, contigs, _ = good
    with pytest.raises(ValueError, match="do not sum to len"):
        mm.sam_check(text.replace("2S8M2S", "2S8M1S"), contigs)
