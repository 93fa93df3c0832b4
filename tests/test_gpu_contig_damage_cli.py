"""`carpedeam contig_damage` and `carpedeam ancient_assemble_fused --damage-report` on the device: the TSV against the tables of
tests/pileup_model.py on the records the same four library calls give, formatted the same way - integers, compared as text."""
import json
import os
import subprocess

import numpy as np
import pytest

import pileup_model as pm
from carpedeam_amd import capi
from stageflags import K_FLAGS, R_FLAGS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT = os.path.join(ROOT, "carpedeam_amd", "carpedeam")
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
GOLD = os.path.join(ROOT, "tests", "golden")
COMP = str.maketrans("ACGT", "TGCA")


@pytest.fixture(scope="module", autouse=True)
def built():
    from carpedeam_amd import build
    build.build()


def run(exe, args, **env):
    e = {k: v for k, v in os.environ.items() if k != "CARPEDEAM_REF_BIN"}
    e.update(env)
    return subprocess.run([exe] + args, capture_output=True, text=True, env=e, timeout=300)


def createdb_order(n):
    """createdb's --shuffle 1: entry i goes to split i % 32, the splits back to back (how the loop and contig_damage lay reads out)"""
    return [i for s in range(32) for i in range(s, n, 32)]


def expected_tsv(names, contigs, reads, ends, k=20, min_seq_id=0.9):
    """the four steps of contig_damage through the Python binding, the counting done by the model"""
    assert K_FLAGS[-2:] == ["-k", "20"] and "--min-seq-id 0.9" in " ".join(R_FLAGS)
    ctx = capi.Ctx(0)
    reads = [reads[i] for i in createdb_order(len(reads))]
    both = ctx.concat(ctx.upload_seqs(contigs), ctx.upload_seqs(reads), 1, 0)
    kp = capi.KmerParams.reads_default()
    kp.kmer_size = k
    rp = capi.RescoreParams.default()
    rp.seq_id_thr = min_seq_id
    alns = ctx.rescore(both, ctx.kmermatch(both, kp), rp)
    off, rec = alns.download()
    queries = list(range(len(contigs)))
    ext = [1] * len(contigs) + [0] * len(reads)
    counts, nreads, columns = pm.profile(contigs + reads, ext, off, rec, queries, ends, 0.0, True)
    got = ctx.pileup_profile(both, alns, queries, ends, 0.0, True)
    assert all(np.array_equal(g, w) for g, w in zip(got, (counts, nreads, columns)))
    return pm.tsv(names, queries, [len(c) for c in contigs], counts, nreads, columns), counts, nreads


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """three contigs of 400 letters, 300 reads of 40..80 letters cut from them on both strands; every third read whose first letter
    is a C gets it replaced by T (C->T at 5' position 1), no other difference"""
    rng = np.random.default_rng(2024)
    contigs = ["".join(rng.choice(list("ACGT"), size=400)) for _ in range(3)]
    reads, forced = [], 0
    for i in range(300):
        c = contigs[i % 3]
        n = int(rng.integers(40, 81))
        at = int(rng.integers(0, 400 - n + 1))
        r = c[at:at + n]
        if rng.integers(0, 2):
            r = r.translate(COMP)[::-1]
        if r[0] == "C" and forced * 3 <= i:
            r = "T" + r[1:]
            forced += 1
        reads.append(r)
    d = tmp_path_factory.mktemp("contig_damage")
    with open(d / "contigs.fa", "w") as f:
        for i, c in enumerate(contigs):
            f.write(">ctg%d some comment\n%s\n%s\n" % (i + 1, c[:250], c[250:]))
    with open(d / "reads.fq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    assert forced >= 20
    return dict(dir=d, contigs=contigs, reads=reads, forced=forced, names=["ctg1", "ctg2", "ctg3"])


def test_contig_damage_tsv(corpus):
    d = corpus["dir"]
    log = str(d / "dispatch.log")
    r = run(FRONT, ["contig_damage", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "out.tsv"), "--threads", "4"], CARPEDEAM_DISPATCH_LOG=log)
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(log).read() == "gpu contig_damage\n"
    want, counts, nreads = expected_tsv(corpus["names"], corpus["contigs"], corpus["reads"], 16)
    got = open(d / "out.tsv").read()
    assert got == want
    rows = [l.split("\t") for l in got.split("\n")[1:] if l]
    head = got.split("\n")[0].split("\t")
    assert [r[0] for r in rows] == corpus["names"] and [r[1] for r in rows] == ["0", "1", "2"] and [r[2] for r in rows] == ["400"] * 3
    ct1 = sum(int(r[head.index("5p_CT_1")]) for r in rows)
    # the forced substitutions show: a read of 40+ letters with one mismatch keeps 97.5 % identity and k-mers of 20 behind it, so at least
    # half of the forced reads are found; no other column of these reads differs from its contig
    assert ct1 >= corpus["forced"] // 2
    assert all(int(r[head.index("5p_CT_%d" % p)]) == 0 for r in rows for p in range(2, 17))
    assert all(int(r[head.index("3p_GA_%d" % p)]) == 0 for r in rows for p in range(1, 17))
    assert sum(int(r[3]) for r in rows) >= 150


def test_contig_damage_flags(corpus):
    d = corpus["dir"]
    r = run(EXE, ["contig_damage", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "e4.tsv"), "--damage-ends", "4", "--min-seq-id", "0.99", "-k", "22"])
    assert r.returncode == 0, r.stderr[-1500:]
    want, _, _ = expected_tsv(corpus["names"], corpus["contigs"], corpus["reads"], 4, k=22, min_seq_id=0.99)
    assert open(d / "e4.tsv").read() == want
    assert len(want.split("\n")[0].split("\t")) == 5 + 4 * 4


@pytest.mark.parametrize("ends", ["0", "65"])
def test_damage_ends_out_of_range(corpus, ends):
    d = corpus["dir"]
    out = str(d / ("refused_%s.tsv" % ends))
    r = run(EXE, ["contig_damage", str(d / "contigs.fa"), str(d / "reads.fq"), out, "--damage-ends", ends])
    assert r.returncode == 77 and "--damage-ends " + ends in r.stderr
    assert not os.path.exists(out)


def test_unknown_flag(corpus):
    d = corpus["dir"]
    r = run(EXE, ["contig_damage", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "x.tsv"), "--shuffle", "0"])
    assert r.returncode == 1 and 'Unrecognized parameter "--shuffle"' in r.stderr


def test_an_empty_fasta_gives_the_header_alone(corpus):
    d = corpus["dir"]
    open(d / "empty.fa", "w").close()
    r = run(EXE, ["contig_damage", str(d / "empty.fa"), str(d / "reads.fq"), str(d / "empty.tsv"), "--damage-ends", "2"])
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(d / "empty.tsv").read() == pm.tsv_header(2)


def test_fused_damage_report(tmp_path, dhigh_prefix):
    """ancient_assemble_fused on the smallest single-file input of tests/test_gpu_assemble_fused.py: the FASTA is byte-identical with and
    without --damage-report, and the TSV is what contig_damage writes for that FASTA and those reads"""
    c = json.load(open(os.path.join(GOLD, "fused", "cases.json")))["circ"]
    reads = os.path.join(GOLD, c["inputs"][0])
    base = [reads, None, None, "--ancient-damage", dhigh_prefix, "--threads", "8"] + c["flags"]

    def fused(tag, extra):
        a = list(base)
        a[1], a[2] = str(tmp_path / (tag + ".fasta")), str(tmp_path / (tag + "_tmp"))
        r = run(FRONT, ["ancient_assemble_fused"] + a + extra)
        assert r.returncode == 0, r.stderr[-1500:]
        return open(a[1], "rb").read()

    plain = fused("plain", [])
    tsv = str(tmp_path / "report.tsv")
    with_report = fused("report", ["--damage-report", tsv, "--damage-ends", "12"])
    assert with_report == plain == open(os.path.join(GOLD, c["fasta"]), "rb").read()
    r = run(FRONT, ["contig_damage", str(tmp_path / "report.fasta"), reads, str(tmp_path / "cli.tsv"), "--damage-ends", "12"])
    assert r.returncode == 0, r.stderr[-1500:]
    got = open(tsv).read()
    assert got == open(tmp_path / "cli.tsv").read()
    lines = got.split("\n")
    assert lines[0] == pm.tsv_header(12).rstrip("\n") and len(lines) - 2 == plain.count(b">")
    assert sum(int(l.split("\t")[3]) for l in lines[1:] if l) > 0             # reads were counted on the contigs
