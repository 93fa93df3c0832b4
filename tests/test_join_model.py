"""tests/join_model.py against expectations written out by hand: the junction results, letters and counts of the directed cases of
tests/joincases.py, the decisions and paths of its host cases, and the three files on a small example.  No device."""
import numpy as np
import pytest

import join_model as jm
import joincases as jc

FIELDS = ("columns", "matches", "voters", "flags", "fill_len", "fill_min", "fill_n")
WRITTEN = [(n, m) for n, m in jc.DIRECTED if n != "chain"]


@pytest.mark.parametrize("name,make", WRITTEN, ids=[n for n, _ in WRITTEN])
def test_directed_junctions(name, make):
    c = make()
    res, letters, counts = jc.model(c)
    assert [tuple(int(r[f]) for f in FIELDS) for r in res] == c["want"]
    assert bytes(letters).decode() == c["letters"] and counts.shape == (len(c["letters"]), 5)
    assert res["fill_off"].tolist() == np.concatenate([[0], np.cumsum(res["fill_len"])[:-1]]).tolist()
    if "counts" in c:
        assert counts.tolist() == c["counts"]
    for o, row in enumerate(counts):        # every voter has one letter at every offset of its junction
        j = int(np.searchsorted(res["fill_off"] + res["fill_len"], o, side="right"))
        assert int(row.sum()) == int(res[j]["voters"])


def test_subsets_of_the_junctions_say_the_same():
    c = jc.junction_lists()
    whole = jc.model(c)
    for subset in c["subsets"]:
        res, letters, _ = jc.model(c, [c["juncs"][i] for i in subset])
        assert [tuple(int(r[f]) for f in FIELDS) for r in res] == [c["want"][i] for i in subset]
        assert bytes(letters).decode() == "".join(bytes(whole[1][int(whole[0][i]["fill_off"]):][:int(whole[0][i]["fill_len"])]).decode() for i in subset)


def test_voters_are_the_mode_reads_of_the_links():
    for make in (jc.fill_gaps, jc.junction_lists, jc.chain, lambda: jc.random_set(1)):
        c = make()
        links = jc.model_links(c)
        res = jc.model(c, [(int(k["a"]), int(k["b"]), int(k["info"]), int(k["gap_mode"])) for k in links])[0]
        assert len(links) and res["voters"].tolist() == links["mode_reads"].tolist()


def test_reverse_complements():
    assert jm.rc("ACGTN") == "NACGT" and jm.device_letters("acgRn-T") == "ACGNNNT"
    assert jm.rc_bytes("ACGTacgtRYKMBVDHrykmbvdhSWNswn*x") == "x*nwsNWSdhbvkmryDHBVKMRYacgtACGT"


@pytest.mark.parametrize("name", sorted(jc.DECISIONS))
def test_decisions_and_paths(name):
    c = jc.DECISIONS[name]
    got = jm.join(c["names"], c["contigs"], c["links"], jc.synthetic_junctions(c), **c["par"])
    assert "".join(got["dec"]) == c["dec"]
    assert got["paths"] == c["paths"]
    assert got["joins"].count("\n") == len(c["links"])
    inside = {m[0] for p in got["paths"] for m in p}
    assert got["joined"].count(">") == len(c["contigs"]) - len(inside) + len(got["paths"])


def test_the_three_files():
    c = jc.DECISIONS["J"]
    got = jm.join(c["names"], c["contigs"], c["links"], jc.synthetic_junctions(c))
    c0, c1, c2 = c["contigs"]
    joined = jm.rc_bytes(c1) + "TGG" + jm.rc_bytes(c0) + "AN" + c2
    assert jm.rc_bytes(c0).endswith("ACGTxNWSDHBVKMRYacgt")
    assert got["joined"] == ">c1_join3\n%s\n" % joined          # c0 and c2 are inside the path that starts at c1
    assert got["joins"] == "c0\t+\tc1\t+\t4\t3\t4\t0\t0\t2\t0\tJ\tc1_join3\nc0\t-\tc2\t+\t4\t2\t4\t0\t0\t2\t1\tJ\tc1_join3\n"
    assert got["paths_tsv"] == "c1_join3\t1\tc1\t-\t1\t40\t0\t0\nc1_join3\t2\tc0\t-\t44\t50\t0\t3\nc1_join3\t3\tc2\t+\t96\t40\t0\t2\n"
    c = jc.DECISIONS["S"]
    got = jm.join(c["names"], c["contigs"], c["links"], jc.synthetic_junctions(c))
    assert got["joined"] == ">c0_join2\n%s\n>c2\n%s\n" % (c["contigs"][0] + c["contigs"][1][15:], c["contigs"][2])
    assert got["paths_tsv"] == "c0_join2\t1\tc0\t+\t1\t45\t0\t0\nc0_join2\t2\tc1\t+\t46\t20\t15\t0\n"
    assert got["joins"] == "c0\t+\tc1\t+\t5\t-15\t5\t15\t15\t0\t0\tJ\tc0_join2\nc1\t+\tc2\t+\t3\t-10\t3\t10\t10\t0\t0\tS\t-\n"
    c = jc.DECISIONS["O"]
    got = jm.join(c["names"], c["contigs"], c["links"], jc.synthetic_junctions(c))
    assert got["joined"] == ">c0_join3\n%s\n" % (c["contigs"][0] + "G" + c["contigs"][1] + c["contigs"][2])
    c = jc.DECISIONS["W"]
    got = jm.join(c["names"], c["contigs"], c["links"], jc.synthetic_junctions(c))
    assert got["joined"] == ">c0\n%s\n>c1\n%s\n" % tuple(c["contigs"]) and got["paths_tsv"] == "" and got["joins"] == "c0\t+\tc1\t+\t5\t2\t1\t0\t0\t0\t0\tW\t-\n"
