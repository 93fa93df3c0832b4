"""`carpedeam contig_depth` and `carpedeam ancient_assemble_fused --depth-report` on the device: the TSV and the bedGraph against the
text tests/depth_model.py writes for the records the same four library calls give - integers, compared as text."""
import json
import os
import subprocess

import numpy as np
import pytest

import depth_model as dm
from carpedeam_amd import capi
from stageflags import K_FLAGS, R_FLAGS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT = os.path.join(ROOT, "carpedeam_amd", "carpedeam")
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
GOLD = os.path.join(ROOT, "tests", "golden")
COMP = str.maketrans("ACGT", "TGCA")
NAMES = ["ctg1", "ctg2", "ctg3"]


@pytest.fixture(scope="module", autouse=True)
def built():
    from carpedeam_amd import build
    build.build()


def run(exe, args, **env):
    e = {k: v for k, v in os.environ.items() if k != "CARPEDEAM_REF_BIN"}
    e.update(env)
    return subprocess.run([exe] + args, capture_output=True, text=True, env=e, timeout=300)


def createdb_order(n):
    """createdb's --shuffle 1: entry i goes to split i % 32, the splits back to back (how the loop and contig_depth lay reads out)"""
    return [i for s in range(32) for i in range(s, n, 32)]


def expected(contigs, reads, edge, k=20, min_seq_id=0.9):
    """the four steps of contig_depth through the Python binding, the counting done by the model -> (stats, tracks)"""
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
    stats, tracks = dm.depth_stats(contigs + reads, ext, off, rec, queries, edge, 0.0, True)
    got, got_tracks = ctx.pileup_depth(both, alns, queries, edge, 0.0, True, track=True)
    assert np.array_equal(got, stats) and all(np.array_equal(g, w) for g, w in zip(got_tracks, tracks))
    return stats, tracks


def text_of(contigs, stats_per_sample):
    return dm.tsv(NAMES, list(range(len(contigs))), [len(c) for c in contigs], stats_per_sample)


def write_fastq(path, reads):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """the corpus of tests/test_gpu_contig_damage_cli.py: three contigs of 400 letters, 300 reads of 40..80 letters cut from them on both
    strands; every third read whose first letter is a C gets it replaced by T, no other difference"""
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
    d = tmp_path_factory.mktemp("contig_depth")
    with open(d / "contigs.fa", "w") as f:
        for i, c in enumerate(contigs):
            f.write(">ctg%d some comment\n%s\n%s\n" % (i + 1, c[:250], c[250:]))
    write_fastq(d / "reads.fq", reads)
    write_fastq(d / "even.fq", reads[0::2])
    write_fastq(d / "odd.fq", reads[1::2])
    return dict(dir=d, contigs=contigs, reads=reads)


@pytest.fixture(scope="module")
def one_sample(corpus):
    return expected(corpus["contigs"], corpus["reads"], 0)


def test_contig_depth_tsv(corpus, one_sample):
    d = corpus["dir"]
    log = str(d / "dispatch.log")
    r = run(FRONT, ["contig_depth", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "out.tsv"), "--threads", "4"], CARPEDEAM_DISPATCH_LOG=log)
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(log).read() == "gpu contig_depth\n"
    got = open(d / "out.tsv").read()
    assert got == text_of(corpus["contigs"], [one_sample[0]])
    head = got.split("\n")[0].split("\t")
    assert head == dm.tsv_header(1).rstrip("\n").split("\t")
    rows = [dict(zip(head, l.split("\t"))) for l in got.split("\n")[1:] if l]
    assert [r["name"] for r in rows] == NAMES and [r["key"] for r in rows] == ["0", "1", "2"] and [r["length"] for r in rows] == ["400"] * 3
    assert sum(int(r["reads_1"]) for r in rows) >= 150
    assert all(int(r["breadth_1"]) <= 400 for r in rows)
    assert all(r["sum_1"] == r["columns_1"] and r["window"] == "400" for r in rows)          # edge 0: the window is the contig


def test_two_samples_give_two_column_groups(corpus):
    d = corpus["dir"]
    r = run(EXE, ["contig_depth", str(d / "contigs.fa"), str(d / "even.fq"), str(d / "odd.fq"), str(d / "two.tsv"), "--depth-edge", "20"])
    assert r.returncode == 0, r.stderr[-1500:]
    got = open(d / "two.tsv").read()
    assert got.split("\n")[0] + "\n" == dm.tsv_header(2)
    groups = []
    for name in ("even", "odd"):
        r = run(EXE, ["contig_depth", str(d / "contigs.fa"), str(d / (name + ".fq")), str(d / (name + ".tsv")), "--depth-edge", "20"])
        assert r.returncode == 0, r.stderr[-1500:]
        groups.append([l.split("\t") for l in open(d / (name + ".tsv")).read().split("\n")[1:] if l])
    rows = [l.split("\t") for l in got.split("\n")[1:] if l]
    assert len(rows) == 3
    for i, row in enumerate(rows):
        assert row[:4] == groups[0][i][:4] == groups[1][i][:4] and row[3] == "360"
        assert row[4:11] == groups[0][i][4:] and row[11:] == groups[1][i][4:]
    assert sum(int(r[4]) for r in rows) > 0 and sum(int(r[11]) for r in rows) > 0
    # each group against the model on its own reads
    stats = [expected(corpus["contigs"], corpus["reads"][k::2], 20)[0] for k in (0, 1)]
    assert got == text_of(corpus["contigs"], stats)


def test_contig_depth_flags(corpus):
    d = corpus["dir"]
    r = run(EXE, ["contig_depth", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "e50.tsv"), "--depth-edge", "50", "-k", "22", "--min-seq-id", "0.99"])
    assert r.returncode == 0, r.stderr[-1500:]
    stats, _ = expected(corpus["contigs"], corpus["reads"], 50, k=22, min_seq_id=0.99)
    assert open(d / "e50.tsv").read() == text_of(corpus["contigs"], [stats])
    assert stats[:, 3].tolist() == [300] * 3 and stats[:, 0].sum() > 0


def test_depth_track(corpus, one_sample):
    d = corpus["dir"]
    r = run(EXE, ["contig_depth", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "t.tsv"), "--depth-track", str(d / "t.bedgraph")])
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(d / "t.tsv").read() == text_of(corpus["contigs"], [one_sample[0]])
    got = open(d / "t.bedgraph").read()
    assert got == dm.bedgraph(NAMES, one_sample[1])
    for name in NAMES:          # the intervals tile 0..400
        iv = [(int(f[1]), int(f[2])) for f in (l.split("\t") for l in got.split("\n") if l) if f[0] == name]
        assert iv[0][0] == 0 and iv[-1][1] == 400 and all(a[1] == b[0] for a, b in zip(iv, iv[1:])) and all(a < b for a, b in iv)


def test_an_empty_fasta_gives_the_header_alone(corpus):
    d = corpus["dir"]
    open(d / "empty.fa", "w").close()
    r = run(EXE, ["contig_depth", str(d / "empty.fa"), str(d / "reads.fq"), str(d / "empty.tsv"), "--depth-edge", "2"])
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(d / "empty.tsv").read() == dm.tsv_header(1)


def test_reads_without_sequences_are_an_error(corpus):
    d = corpus["dir"]
    open(d / "none.fq", "w").close()
    r = run(EXE, ["contig_depth", str(d / "contigs.fa"), str(d / "none.fq"), str(d / "none.tsv")])
    assert r.returncode == 1 and "holds no reads" in r.stderr
    assert not os.path.exists(d / "none.tsv")


def test_fused_depth_report(tmp_path, dhigh_prefix):
    """ancient_assemble_fused on the `circ` case: the FASTA is byte-identical with and without --depth-report and equals the golden; the
    report is what contig_depth writes for that FASTA and those reads; with --damage-report as well, both tables equal their stand-alone
    commands' output"""
    c = json.load(open(os.path.join(GOLD, "fused", "cases.json")))["circ"]
    reads = os.path.join(GOLD, c["inputs"][0])
    base = [reads, None, None, "--ancient-damage", dhigh_prefix, "--threads", "8"] + c["flags"]

    def fused(tag, extra):
        a = list(base)
        a[1], a[2] = str(tmp_path / (tag + ".fasta")), str(tmp_path / (tag + "_tmp"))
        r = run(FRONT, ["ancient_assemble_fused"] + a + extra)
        assert r.returncode == 0, r.stderr[-1500:]
        return open(a[1], "rb").read()

    golden = open(os.path.join(GOLD, c["fasta"]), "rb").read()
    plain = fused("plain", [])
    depth = str(tmp_path / "depth.tsv")
    assert fused("depth", ["--depth-report", depth, "--depth-edge", "30"]) == plain == golden
    r = run(FRONT, ["contig_depth", str(tmp_path / "depth.fasta"), reads, str(tmp_path / "cli_depth.tsv"), "--depth-edge", "30"])
    assert r.returncode == 0, r.stderr[-1500:]
    want = open(tmp_path / "cli_depth.tsv").read()
    got = open(depth).read()
    assert got == want
    lines = got.split("\n")
    assert lines[0] + "\n" == dm.tsv_header(1) and len(lines) - 2 == plain.count(b">")
    assert sum(int(l.split("\t")[4]) for l in lines[1:] if l) > 0             # reads were counted on the contigs
    # both reports from one alignment set
    depth2, damage2 = str(tmp_path / "depth2.tsv"), str(tmp_path / "damage2.tsv")
    assert fused("both", ["--depth-report", depth2, "--depth-edge", "30", "--damage-report", damage2, "--damage-ends", "12"]) == golden
    r = run(FRONT, ["contig_damage", str(tmp_path / "both.fasta"), reads, str(tmp_path / "cli_damage.tsv"), "--damage-ends", "12"])
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(depth2).read() == want
    assert open(damage2).read() == open(tmp_path / "cli_damage.tsv").read()
