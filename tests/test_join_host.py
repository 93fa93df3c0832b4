"""host/contig_join.cpp against tests/join_model.py through tests/cpu/join_driver.cpp, built with g++: the junctions, decisions, paths and
the three files on the host cases of tests/joincases.py - one per decision letter, a circle, a walk against a link's canonical direction,
a - start contig, lower-case and IUPAC contig bytes - and on random link graphs.  No device."""
import os
import subprocess

import numpy as np
import pytest

import join_model as jm
import joincases as jc
import links_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "carpedeam_amd", "csrc", "host")


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    d = tmp_path_factory.mktemp("join")
    exe = str(d / "join_driver")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpu", "join_driver.cpp"),
                        os.path.join(HOST, "contig_join.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(c, n=[0]):
        """the case through the model and through the driver -> (model's dict, driver's dict)"""
        par = dict(jm.DEFAULTS, **c["par"])
        lens = [len(s) for s in c["contigs"]]
        dec, juncs, at = jm.first_decisions(c["links"], lens, par["min_link_reads"])
        res, letters = jc.synthetic_junctions(c)(juncs) if len(juncs) else (np.zeros(0, jm.RES_DTYPE), np.zeros(0, np.uint8))
        want = jm.join(c["names"], c["contigs"], c["links"], jc.synthetic_junctions(c), min_link_reads=par["min_link_reads"], overlap_percent=par["overlap_percent"])
        lines = ["%d %d" % (par["overlap_percent"], par["min_link_reads"]), str(len(lens))] + ["%s %s" % (n_, s) for n_, s in zip(c["names"], c["contigs"])] + [str(len(c["links"]))]
        lines += [" ".join(str(int(k[f])) for f in lm.LINK_DTYPE.names if f != "reserved") for k in c["links"]] + [str(len(at))]
        for i, r_ in zip(at, res):
            f = bytes(letters[int(r_["fill_off"]):int(r_["fill_off"]) + int(r_["fill_len"])]).decode()
            lines.append(" ".join([str(i)] + [str(int(r_[k])) for k in ("columns", "matches", "voters", "flags", "fill_len", "fill_min", "fill_n")] + [f or "-"]))
        n[0] += 1
        path = d / ("case%d.txt" % n[0])
        path.write_text("\n".join(lines) + "\n")
        out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr[-2000:]
        head, rest = out.stdout.split("==joins\n")
        joins, rest = rest.split("==joined\n")
        joined, rest = rest.split("==paths\n")
        got = dict(joins=joins, joined=joined, paths_tsv=rest[:-len("==end\n")], juncs=[], paths=[], dec=None)
        assert rest.endswith("==end\n")
        for line in head.splitlines():
            f = line.split()
            if f[0] == "junc":
                got["juncs"].append(tuple(int(x) for x in f[1:]))
            elif f[0] == "dec":
                got["dec"] = f[1] if len(f) > 1 else ""
            else:
                k = int(f[1])
                if k == len(got["paths"]):
                    got["paths"].append([])
                got["paths"][k].append((int(f[2]), f[3], int(f[4]), "" if f[5] == "-" else f[5]))
        return want, got
    return run


def same(want, got):
    assert got["juncs"] == [tuple(int(x) for x in j) for j in want["juncs"]]
    assert got["dec"] == "".join(want["dec"])
    assert got["paths"] == want["paths"]
    assert got["joins"] == want["joins"] and got["joined"] == want["joined"] and got["paths_tsv"] == want["paths_tsv"]


@pytest.mark.parametrize("name", sorted(jc.DECISIONS))
def test_the_host_cases(drv, name):
    c = jc.DECISIONS[name]
    want, got = drv(c)
    assert got["dec"] == c["dec"] and got["paths"] == c["paths"]
    same(want, got)


def test_lower_case_and_iupac_bytes_are_complemented_in_place(drv):
    c = jc.DECISIONS["J"]
    want, got = drv(c)
    record = got["joined"].splitlines()[1]
    assert record[40 + 3:][:50].endswith("ACGTxNWSDHBVKMRYacgt") and record.startswith(jm.rc_bytes(c["contigs"][1]))
    same(want, got)


def random_graph(seed):
    """5 to 40 contigs of 12 to 80 bytes (a few lower-case and IUPAC), links over a random choice of end pairs: overlaps up to 25 with planted
    agreement for some, fills up to 6, 1 to 6 reads; dense enough for A, sparse enough for paths; every fourth set has a circle of its own"""
    rng = np.random.default_rng(9100 + seed)
    nc = int(rng.integers(5, 41))
    contigs = ["".join(rng.choice(list("ACGTACGTACGTacgtRYKMSWN"), size=int(rng.integers(12, 81)))) for _ in range(nc)]
    edges = set()
    for _ in range(int(nc * rng.choice([0.5, 0.9, 1.3]))):
        a, b = sorted(int(x) for x in rng.choice(nc, size=2, replace=False))
        edges.add((a, int(rng.integers(0, 2)), b, int(rng.integers(0, 2))))
    if seed % 4 == 0:           # a circle of three or four contigs of their own, with reads enough for any threshold
        m = int(rng.integers(3, 5))
        contigs += ["".join(rng.choice(list("ACGT"), size=30)) for _ in range(m)]
        edges.update((nc + i, 0, nc + i + 1, 0) for i in range(m - 1))
        edges.add((nc, 1, nc + m - 1, 1))
    links, fills = [], {}
    for i, (a, oa, b, ob) in enumerate(sorted(edges)):
        ring = a >= nc
        gap = int(rng.integers(0, 4)) if ring else int(rng.integers(-25, 7))
        if gap < 0 and rng.integers(0, 3) and -gap <= min(len(contigs[a]), len(contigs[b])):          # make the two ends agree: B's oriented head := A's oriented tail
            tail = (jm.rc_bytes(contigs[a]) if oa else contigs[a])[gap:]
            ob_form = jm.rc_bytes(contigs[b]) if ob else contigs[b]
            ob_form = tail + ob_form[-gap:]
            contigs[b] = jm.rc_bytes(ob_form) if ob else ob_form
        reads = 6 if ring else int(rng.integers(1, 7))
        links.append(jc.link(a, "-" if oa else "+", b, "-" if ob else "+", reads, gap, mode_reads=reads if ring else int(rng.integers(1, reads + 1))))
        if gap > 0:
            fills[i] = "".join(rng.choice(list("ACGTN"), size=gap))
    return jc.host_case(contigs, links, None, None, fills=fills, overlap_percent=int(rng.choice([0, 60, 90, 100])), min_link_reads=int(rng.integers(1, 4)))


@pytest.mark.parametrize("group", range(4))
def test_random_link_graphs(drv, group):
    seen = set()
    for seed in range(group * 25, group * 25 + 25):
        want, got = drv(random_graph(seed))
        same(want, got)
        seen.update(got["dec"])
    assert {"A", "J"} <= seen


def test_random_graphs_reach_every_decision(drv):
    seen = set()
    for seed in range(100):
        seen.update(drv(random_graph(seed))[1]["dec"])
    assert seen == set("AWCXSOJ"), seen
