"""`carpedeam contig_breaks` and `carpedeam ancient_assemble_fused --break-report` on the device: the summary with its `#break` lines, the
span track and the split FASTA against the text tests/breaks_model.py writes for the records the same four library calls give -
compared as text - and a planted chimeric join that the defaults have to find."""
import json
import os
import subprocess

import numpy as np
import pytest

import breaks_model as bm
from carpedeam_amd import capi
from stageflags import K_FLAGS, R_FLAGS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT = os.path.join(ROOT, "carpedeam_amd", "carpedeam")
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
GOLD = os.path.join(ROOT, "tests", "golden")
COMP = str.maketrans("ACGT", "TGCA")
NAMES = ["ctg1", "ctg2", "ctg3"]
HOLE, LOWER, IUPAC = (180, 230), (100, 140), {60: "R", 250: "y", 251: "N"}       # on ctg2: no read touches it; on ctg3; on ctg3
DEFAULTS = dict(anchor=16, edge=50, min_span=1, min_span_percent=0)


@pytest.fixture(scope="module", autouse=True)
def built():
    from carpedeam_amd import build
    build.build()


def run(exe, args, **env):
    e = {k: v for k, v in os.environ.items() if k != "CARPEDEAM_REF_BIN"}
    e.update(env)
    return subprocess.run([exe] + args, capture_output=True, text=True, env=e, timeout=300)


def createdb_order(n):
    """createdb's --shuffle 1: entry i goes to split i % 32, the splits back to back (how the loop and contig_breaks lay reads out)"""
    return [i for s in range(32) for i in range(s, n, 32)]


def expected(contigs, reads, k=20, min_seq_id=0.9, **par):
    """the four steps of contig_breaks through the Python binding, the statistic by the model -> (stats, tracks, breaks)"""
    assert K_FLAGS[-2:] == ["-k", "20"] and "--min-seq-id 0.9" in " ".join(R_FLAGS)
    p = dict(DEFAULTS)
    p.update(par)
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
    stats, tracks, breaks = bm.breaks_stats(contigs + reads, ext, off, rec, queries, p["anchor"], p["edge"], p["min_span"], p["min_span_percent"], 0.0, True)
    got, got_tracks, got_breaks = ctx.pileup_breaks(both, alns, queries, p["anchor"], p["edge"], p["min_span"], p["min_span_percent"], 0.0, True, track=True, breaks=True)
    assert np.array_equal(got, stats) and np.array_equal(got_breaks, breaks) and all(np.array_equal(g, w) for g, w in zip(got_tracks, tracks))
    return stats, tracks, breaks


def write_fasta(path, names, seqs):
    with open(path, "w") as f:
        for name, seq in zip(names, seqs):
            f.write(">%s\n%s\n" % (name, seq))


def write_fastq(path, reads):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))


def build_corpus():
    """three contigs of 400 letters, 330 reads of 40..80 letters cut from them on both strands; no read touches ctg2[HOLE]; ctg3 is
    written with a lower-case stretch and three IUPAC letters"""
    rng = np.random.default_rng(2025)
    original = ["".join(rng.choice(list("ACGT"), size=400)) for _ in range(3)]
    reads = []
    while len(reads) < 330:
        i = len(reads)
        n = int(rng.integers(40, 81))
        at = int(rng.integers(0, 400 - n + 1))
        if i % 3 == 1 and at < HOLE[1] and at + n > HOLE[0]:
            at = 0 if at < HOLE[0] else 400 - n
        r = original[i % 3][at:at + n]
        if rng.integers(0, 2):
            r = r.translate(COMP)[::-1]
        reads.append(r)
    contigs = list(original)
    c3 = list(original[2][:LOWER[0]] + original[2][LOWER[0]:LOWER[1]].lower() + original[2][LOWER[1]:])
    for at, letter in IUPAC.items():
        c3[at] = letter
    contigs[2] = "".join(c3)
    return dict(contigs=contigs, reads=reads)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    c = build_corpus()
    c["dir"] = d = tmp_path_factory.mktemp("contig_breaks")
    write_fasta(d / "contigs.fa", NAMES, c["contigs"])
    write_fastq(d / "reads.fq", c["reads"])
    return c


def summary_of(contigs, stats, breaks):
    return bm.tsv(NAMES, list(range(len(contigs))), [len(c) for c in contigs], stats, breaks)


def test_contig_breaks_files(corpus):
    d = corpus["dir"]
    stats, tracks, breaks = expected(corpus["contigs"], corpus["reads"])
    log = str(d / "dispatch.log")
    out, split, bed = str(d / "out.tsv"), str(d / "split.fa"), str(d / "span.bedgraph")
    r = run(FRONT, ["contig_breaks", str(d / "contigs.fa"), str(d / "reads.fq"), out, "--split", split, "--span-track", bed, "--threads", "4"], CARPEDEAM_DISPATCH_LOG=log)
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(log).read() == "gpu contig_breaks\n"
    text = open(out).read()
    assert text == summary_of(corpus["contigs"], stats, breaks)
    assert open(bed).read() == bm.bedgraph(NAMES, tracks)
    fasta = open(split).read()
    assert fasta == bm.split(NAMES, corpus["contigs"], breaks)
    rows = [l.split("\t") for l in text.split("\n")[1:] if l and not l.startswith("#")]
    assert [r[0] for r in rows] == NAMES and [r[1] for r in rows] == ["0", "1", "2"] and [r[2] for r in rows] == ["400"] * 3
    assert sum(int(r[3]) for r in rows) >= 150 and [r[5] for r in rows] == ["301"] * 3
    # the stretch without reads: one gap on ctg2 that holds it, and its two flanks in the split FASTA
    marks = [l.split("\t") for l in text.split("\n") if l.startswith("#break\tctg2\t")]
    assert len(marks) == 1 and marks[0][8] == "G" and int(marks[0][2]) - 1 <= HOLE[0] and int(marks[0][3]) - 1 >= HOLE[1] and int(marks[0][5]) >= HOLE[1] - HOLE[0]
    first, last = int(marks[0][2]) - 1, int(marks[0][3]) - 1
    assert ">ctg2_1\n%s\n>ctg2_2\n%s\n" % (corpus["contigs"][1][:first], corpus["contigs"][1][last:]) in fasta
    # an unbroken contig is unchanged, lower case and IUPAC bytes included
    assert not [l for l in text.split("\n") if l.startswith("#break\tctg3\t")]
    assert ">ctg3\n%s\n" % corpus["contigs"][2] in fasta and any(c.islower() for c in corpus["contigs"][2]) and "R" in corpus["contigs"][2]


def test_contig_breaks_flags(corpus):
    """thresholds that break the contigs in many places; the pieces of ctg3 keep its lower case and IUPAC bytes; --min-piece drops the
    short ones"""
    d = corpus["dir"]
    flags = ["--break-anchor", "8", "--break-edge", "10", "--min-span", "4", "--min-span-percent", "60", "-k", "22", "--min-seq-id", "0.95"]
    stats, tracks, breaks = expected(corpus["contigs"], corpus["reads"], k=22, min_seq_id=0.95, anchor=8, edge=10, min_span=4, min_span_percent=60)
    r = run(EXE, ["contig_breaks", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "f.tsv"), "--split", str(d / "f_split.fa"), "--span-track", str(d / "f.bedgraph")] + flags)
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(d / "f.tsv").read() == summary_of(corpus["contigs"], stats, breaks)
    assert open(d / "f.bedgraph").read() == bm.bedgraph(NAMES, tracks)
    fasta = open(d / "f_split.fa").read()
    assert fasta == bm.split(NAMES, corpus["contigs"], breaks)
    assert len(breaks) > 6 and (breaks["flags"] == bm.JOIN).any() and (breaks["flags"] == bm.GAP).any() and (breaks["query"] == 2).any()
    assert any(c.islower() for c in fasta) and "R" in fasta
    r = run(EXE, ["contig_breaks", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "p.tsv"), "--split", str(d / "p_split.fa"), "--min-piece", "50"] + flags)
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(d / "p.tsv").read() == open(d / "f.tsv").read()
    pieces = open(d / "p_split.fa").read()
    assert pieces == bm.split(NAMES, corpus["contigs"], breaks, min_piece=50)
    assert 0 < pieces.count(">") < fasta.count(">") and all(len(l) >= 50 for l in pieces.split("\n") if l and not l.startswith(">"))


def test_an_empty_fasta_gives_the_header_alone(corpus):
    d = corpus["dir"]
    open(d / "empty.fa", "w").close()
    r = run(EXE, ["contig_breaks", str(d / "empty.fa"), str(d / "reads.fq"), str(d / "empty.tsv"), "--split", str(d / "empty_split.fa"), "--span-track", str(d / "empty.bedgraph")])
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(d / "empty.tsv").read() == bm.HEADER
    assert open(d / "empty_split.fa").read() == "" and open(d / "empty.bedgraph").read() == ""


def test_reads_without_sequences_are_an_error(corpus):
    d = corpus["dir"]
    open(d / "none.fq", "w").close()
    r = run(EXE, ["contig_breaks", str(d / "contigs.fa"), str(d / "none.fq"), str(d / "none.tsv")])
    assert r.returncode == 1 and "holds no reads" in r.stderr
    assert not os.path.exists(d / "none.tsv")


# ------------------------------------------------------------------------------------------------ a planted join
JOIN_AT, JOIN_LEN, READ_LEN, READ_STEP, JOIN_SEED = 600, 1200, 60, 3, 611


def planted_join():
    """Two unrelated random sequences A and B of 1200 letters: the contig `joined` is A[0:600] + B[600:1200]; the contig `control` is an
    unrelated C.  The reads are error-free, 60 letters, every 3 letters, from all of A, B and C.

    The conditions of test_a_planted_join were established without a device before the first run on one: kmermatcher and rescorediagonal
    of the CPU oracle (oracle/cdm_oracle.cpp) on the concatenated DB in createdb's read order with the flags of tests/stageflags.py, then
    tests/breaks_model.py with the defaults: `joined` has exactly one break, a join with first <= 600 <= last, and `control` has none.
    The read tiling and the seed are the first ones tried; no threshold was changed."""
    rng = np.random.default_rng(JOIN_SEED)
    a, b, c = ("".join(rng.choice(list("ACGT"), size=JOIN_LEN)) for _ in range(3))
    contigs = [a[:JOIN_AT] + b[JOIN_AT:], c]
    reads = [s[at:at + READ_LEN] for s in (a, b, c) for at in range(0, JOIN_LEN - READ_LEN + 1, READ_STEP)]
    return ["joined", "control"], contigs, reads


def test_a_planted_join(tmp_path):
    names, contigs, reads = planted_join()
    write_fasta(tmp_path / "contigs.fa", names, contigs)
    write_fastq(tmp_path / "reads.fq", reads)
    out, split = str(tmp_path / "out.tsv"), str(tmp_path / "split.fa")
    r = run(EXE, ["contig_breaks", str(tmp_path / "contigs.fa"), str(tmp_path / "reads.fq"), out, "--split", split])
    assert r.returncode == 0, r.stderr[-1500:]
    lines = [l.split("\t") for l in open(out).read().split("\n") if l]
    rows = {l[0]: l for l in lines[1:] if l[0] != "#break"}
    marks = [l for l in lines if l[0] == "#break"]
    assert rows["joined"][7:9] == ["1", "1"] and rows["control"][6:9] == ["0", "0", "0"] and int(rows["control"][3]) > 100
    assert len(marks) == 1 and marks[0][1] == "joined" and marks[0][8] == "J" and marks[0][5] == "0"
    first, last = int(marks[0][2]) - 1, int(marks[0][3]) - 1
    assert first <= JOIN_AT <= last
    assert open(split).read() == ">joined_1\n%s\n>joined_2\n%s\n>control\n%s\n" % (contigs[0][:first], contigs[0][last:], contigs[1])


def test_fused_break_report(tmp_path, dhigh_prefix):
    """ancient_assemble_fused on the `circ` case: the FASTA is the golden one with the new flags; the break report is what contig_breaks
    writes for that FASTA and those reads; the other three reports beside it are byte-equal to those of a run without it"""
    c = json.load(open(os.path.join(GOLD, "fused", "cases.json")))["circ"]
    reads = os.path.join(GOLD, c["inputs"][0])
    base = [reads, None, None, "--ancient-damage", dhigh_prefix, "--threads", "8"] + c["flags"]
    thresholds = ["--break-anchor", "10", "--break-edge", "20", "--min-span", "2", "--min-span-percent", "30"]

    def others(tag):
        return ["--variant-report", str(tmp_path / (tag + "_var.tsv")), "--variant-sites", str(tmp_path / (tag + "_sites.tsv")), "--depth-report", str(tmp_path / (tag + "_depth.tsv")),
                "--depth-edge", "30", "--damage-report", str(tmp_path / (tag + "_damage.tsv")), "--damage-ends", "12"]

    def fused(tag, extra):
        a = list(base)
        a[1], a[2] = str(tmp_path / (tag + ".fasta")), str(tmp_path / (tag + "_tmp"))
        r = run(FRONT, ["ancient_assemble_fused"] + a + extra)
        assert r.returncode == 0, r.stderr[-1500:]
        return open(a[1], "rb").read()

    golden = open(os.path.join(GOLD, c["fasta"]), "rb").read()
    brk = str(tmp_path / "with_breaks.tsv")
    assert fused("with", ["--break-report", brk] + thresholds + others("with")) == golden
    r = run(FRONT, ["contig_breaks", str(tmp_path / "with.fasta"), reads, str(tmp_path / "cli_breaks.tsv")] + thresholds)
    assert r.returncode == 0, r.stderr[-1500:]
    got = open(brk).read()
    assert got == open(tmp_path / "cli_breaks.tsv").read()
    lines = [l for l in got.split("\n") if l]
    assert lines[0] + "\n" == bm.HEADER and len([l for l in lines[1:] if not l.startswith("#")]) == golden.count(b">")
    assert sum(int(l.split("\t")[3]) for l in lines[1:] if not l.startswith("#")) > 0           # reads were counted on the contigs
    assert fused("without", others("without")) == golden
    for name in ("_var.tsv", "_sites.tsv", "_depth.tsv", "_damage.tsv"):
        assert open(tmp_path / ("with" + name), "rb").read() == open(tmp_path / ("without" + name), "rb").read(), name
    assert not os.path.exists(tmp_path / "without_breaks.tsv")
