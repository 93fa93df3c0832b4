"""`carpedeam contig_variants` and `carpedeam ancient_assemble_fused --variant-report` on the device: the summary, the sites file and the
consensus FASTA against the text tests/bases_model.py writes for the records the same four library calls give - compared as text."""
import json
import os
import subprocess

import numpy as np
import pytest

import bases_model as bm
from carpedeam_amd import capi
from stageflags import K_FLAGS, R_FLAGS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT = os.path.join(ROOT, "carpedeam_amd", "carpedeam")
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
GOLD = os.path.join(ROOT, "tests", "golden")
COMP = str.maketrans("ACGT", "TGCA")
NAMES = ["ctg1", "ctg2", "ctg3"]
ALLELE_AT, CHANGED_AT, LOWER = 200, 150, (100, 140)        # on ctg1, on ctg2, on ctg3


@pytest.fixture(scope="module", autouse=True)
def built():
    from carpedeam_amd import build
    build.build()


def run(exe, args, **env):
    e = {k: v for k, v in os.environ.items() if k != "CARPEDEAM_REF_BIN"}
    e.update(env)
    return subprocess.run([exe] + args, capture_output=True, text=True, env=e, timeout=300)


def createdb_order(n):
    """createdb's --shuffle 1: entry i goes to split i % 32, the splits back to back (how the loop and contig_variants lay reads out)"""
    return [i for s in range(32) for i in range(s, n, 32)]


def expected(contigs, reads, k=20, min_seq_id=0.9, **par):
    """the four steps of contig_variants through the Python binding, the counting done by the model -> (stats, sites)"""
    assert K_FLAGS[-2:] == ["-k", "20"] and "--min-seq-id 0.9" in " ".join(R_FLAGS)
    p = dict(bm.DEFAULTS)
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
    stats, _, sites = bm.bases(contigs + reads, ext, off, rec, queries, min_seq_id=0.0, skip=True, **p)
    got, got_sites = ctx.pileup_bases(both, alns, queries, p["mask_ends"], p["min_depth"], p["min_alt_count"], p["min_alt_percent"], 0.0, True, sites=True)
    assert np.array_equal(got, stats) and all(np.array_equal(got_sites[f], sites[f]) for f in ("query", "pos", "info", "counts"))
    return stats, sites


def summary_of(contigs, stats):
    return bm.summary_tsv(NAMES, list(range(len(contigs))), [len(c) for c in contigs], stats)


def write_fastq(path, reads):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))


def build_corpus():
    """the corpus of tests/test_gpu_contig_depth_cli.py - three contigs of 400 letters, 300 reads of 40..80 letters cut from them on both
    strands, every third read whose first letter is a C gets it replaced by T - with three things planted: of the reads over
    ctg1[ALLELE_AT] two in five carry another base; ctg2[CHANGED_AT] is changed AFTER the reads were cut; ctg3 is written with a
    lower-case stretch"""
    rng = np.random.default_rng(2024)
    original = ["".join(rng.choice(list("ACGT"), size=400)) for _ in range(3)]
    alt = "ACGT"[("ACGT".index(original[0][ALLELE_AT]) + 2) % 4]
    reads, forced, covering = [], 0, 0
    for i in range(300):
        c = original[i % 3]
        n = int(rng.integers(40, 81))
        at = int(rng.integers(0, 400 - n + 1))
        r = list(c[at:at + n])
        if i % 3 == 0 and at + 3 <= ALLELE_AT < at + n - 3:         # (not on a read's ends: --mask-ends leaves the allele alone)
            if covering % 5 in (1, 3):
                r[ALLELE_AT - at] = alt
            covering += 1
        r = "".join(r)
        if rng.integers(0, 2):
            r = r.translate(COMP)[::-1]
        if r[0] == "C" and forced * 3 <= i:
            r = "T" + r[1:]
            forced += 1
        reads.append(r)
    contigs = list(original)
    was = original[1][CHANGED_AT]
    contigs[1] = original[1][:CHANGED_AT] + "ACGT"[("ACGT".index(was) + 1) % 4] + original[1][CHANGED_AT + 1:]
    contigs[2] = original[2][:LOWER[0]] + original[2][LOWER[0]:LOWER[1]].lower() + original[2][LOWER[1]:]
    assert covering >= 10 and forced >= 20
    return dict(contigs=contigs, original=original, reads=reads, alt=alt)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    c = build_corpus()
    c["dir"] = d = tmp_path_factory.mktemp("contig_variants")
    with open(d / "contigs.fa", "w") as f:
        for name, seq in zip(NAMES, c["contigs"]):
            f.write(">%s\n%s\n" % (name, seq))
    write_fastq(d / "reads.fq", c["reads"])
    return c


@pytest.fixture(scope="module")
def defaults(corpus):
    return expected(corpus["contigs"], corpus["reads"])


def test_contig_variants_files(corpus, defaults):
    d = corpus["dir"]
    stats, sites = defaults
    log = str(d / "dispatch.log")
    out, sites_file, cons = str(d / "out.tsv"), str(d / "sites.tsv"), str(d / "cons.fa")
    r = run(FRONT, ["contig_variants", str(d / "contigs.fa"), str(d / "reads.fq"), out, "--sites", sites_file, "--consensus", cons, "--threads", "4"], CARPEDEAM_DISPATCH_LOG=log)
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(log).read() == "gpu contig_variants\n"
    assert open(out).read() == summary_of(corpus["contigs"], stats)
    assert open(sites_file).read() == bm.sites_tsv(NAMES, sites)
    fasta = open(cons).read()
    assert fasta == bm.consensus_fasta(NAMES, corpus["contigs"], sites)
    rows = [l.split("\t") for l in open(out).read().split("\n")[1:] if l]
    assert [r[0] for r in rows] == NAMES and [r[1] for r in rows] == ["0", "1", "2"] and [r[2] for r in rows] == ["400"] * 3
    assert sum(int(r[3]) for r in rows) >= 150
    by_pos = {(int(s["query"]), int(s["pos"])): int(s["info"]) >> 8 for s in sites}
    # the second allele: variable, and the contig's letter keeps the majority
    assert by_pos[(0, ALLELE_AT)] == bm.CALLED | bm.VARIABLE
    line = [l.split("\t") for l in open(sites_file).read().split("\n") if l.startswith("ctg1\t%d\t" % (ALLELE_AT + 1))]
    assert len(line) == 1 and line[0][2] == line[0][3] == corpus["original"][0][ALLELE_AT] and line[0][4] == "V"
    counts = dict(zip("ACGT", (int(a) + int(b) for a, b in zip(line[0][6:10], line[0][10:14]))))
    assert counts[corpus["alt"]] >= 2 and counts[corpus["alt"]] < counts[line[0][2]] and int(line[0][5]) == sum(counts.values())
    # the changed contig letter: the reads differ from it, and the consensus has the letter the reads were cut from
    assert by_pos[(1, CHANGED_AT)] & bm.DIFFERS
    want = list(corpus["contigs"])
    want[1] = corpus["original"][1]
    assert fasta == "".join(">%s\n%s\n" % (n, c) for n, c in zip(NAMES, want))          # every other byte as in the input, lower case included
    assert [k for k, fl in by_pos.items() if fl & bm.DIFFERS] == [(1, CHANGED_AT)]


def test_the_mask_takes_the_end_damage_out(corpus, defaults):
    d = corpus["dir"]
    r = run(EXE, ["contig_variants", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "m1.tsv"), "--mask-ends", "1", "--sites", str(d / "m1_sites.tsv")])
    assert r.returncode == 0, r.stderr[-1500:]
    stats, sites = expected(corpus["contigs"], corpus["reads"], mask_ends=1)
    assert open(d / "m1.tsv").read() == summary_of(corpus["contigs"], stats)
    assert open(d / "m1_sites.tsv").read() == bm.sites_tsv(NAMES, sites)
    # the C->T on the first letter of a read counts as a mismatch at --mask-ends 0 and not at 1; what stays are the two planted columns
    m0, m1 = defaults[0][:, 3].astype(np.int64), stats[:, 3].astype(np.int64)
    assert (m0 - m1).sum() >= 10 and np.all(m1 <= m0) and m1[2] == 0 and m1[0] >= 2 and m1[1] >= 3
    assert np.array_equal(defaults[0][:, 0:2], stats[:, 0:2])             # reads and columns do not depend on the mask


def test_contig_variants_flags(corpus):
    d = corpus["dir"]
    r = run(EXE, ["contig_variants", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "f.tsv"), "--sites", str(d / "f_sites.tsv"), "--min-depth", "1", "--min-alt-count", "1",
                  "--min-alt-percent", "5", "-k", "22", "--min-seq-id", "0.95"])
    assert r.returncode == 0, r.stderr[-1500:]
    stats, sites = expected(corpus["contigs"], corpus["reads"], k=22, min_seq_id=0.95, min_depth=1, min_alt_count=1, min_alt_percent=5)
    assert open(d / "f.tsv").read() == summary_of(corpus["contigs"], stats)
    assert open(d / "f_sites.tsv").read() == bm.sites_tsv(NAMES, sites)
    assert len(sites) > 10 and stats[:, 0].sum() > 0


def test_an_empty_fasta_gives_the_header_alone(corpus):
    d = corpus["dir"]
    open(d / "empty.fa", "w").close()
    r = run(EXE, ["contig_variants", str(d / "empty.fa"), str(d / "reads.fq"), str(d / "empty.tsv"), "--sites", str(d / "empty_sites.tsv"), "--consensus", str(d / "empty_cons.fa")])
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(d / "empty.tsv").read() == bm.SUMMARY_HEADER
    assert open(d / "empty_sites.tsv").read() == "" and open(d / "empty_cons.fa").read() == ""


def test_reads_without_sequences_are_an_error(corpus):
    d = corpus["dir"]
    open(d / "none.fq", "w").close()
    r = run(EXE, ["contig_variants", str(d / "contigs.fa"), str(d / "none.fq"), str(d / "none.tsv")])
    assert r.returncode == 1 and "holds no reads" in r.stderr
    assert not os.path.exists(d / "none.tsv")


def test_fused_variant_report(tmp_path, dhigh_prefix):
    """ancient_assemble_fused on the `circ` case: the FASTA is the golden one with the new flags; the two files are what contig_variants
    writes for that FASTA and those reads; with --damage-report and --depth-report as well, all three sets of reports equal their
    stand-alone commands' output"""
    c = json.load(open(os.path.join(GOLD, "fused", "cases.json")))["circ"]
    reads = os.path.join(GOLD, c["inputs"][0])
    base = [reads, None, None, "--ancient-damage", dhigh_prefix, "--threads", "8"] + c["flags"]
    thresholds = ["--min-depth", "2", "--min-alt-count", "1", "--min-alt-percent", "10", "--mask-ends", "1"]

    def fused(tag, extra):
        a = list(base)
        a[1], a[2] = str(tmp_path / (tag + ".fasta")), str(tmp_path / (tag + "_tmp"))
        r = run(FRONT, ["ancient_assemble_fused"] + a + extra)
        assert r.returncode == 0, r.stderr[-1500:]
        return open(a[1], "rb").read()

    def alone(command, fasta, out, extra):
        r = run(FRONT, [command, str(tmp_path / fasta), reads, str(tmp_path / out)] + extra)
        assert r.returncode == 0, r.stderr[-1500:]
        return open(tmp_path / out).read()

    golden = open(os.path.join(GOLD, c["fasta"]), "rb").read()
    var, sites = str(tmp_path / "var.tsv"), str(tmp_path / "sites.tsv")
    assert fused("var", ["--variant-report", var, "--variant-sites", sites] + thresholds) == golden
    want = alone("contig_variants", "var.fasta", "cli_var.tsv", ["--sites", str(tmp_path / "cli_sites.tsv")] + thresholds)
    want_sites = open(tmp_path / "cli_sites.tsv").read()
    got = open(var).read()
    assert got == want and open(sites).read() == want_sites
    lines = got.split("\n")
    assert lines[0] + "\n" == bm.SUMMARY_HEADER and len(lines) - 2 == golden.count(b">")
    assert sum(int(l.split("\t")[3]) for l in lines[1:] if l) > 0             # reads were counted on the contigs
    # the three reports from one alignment set
    var3, sites3, depth3, damage3 = (str(tmp_path / n) for n in ("var3.tsv", "sites3.tsv", "depth3.tsv", "damage3.tsv"))
    assert fused("all", ["--variant-report", var3, "--variant-sites", sites3, "--depth-report", depth3, "--depth-edge", "30", "--damage-report", damage3, "--damage-ends", "12"] + thresholds) == golden
    assert open(var3).read() == want and open(sites3).read() == want_sites
    assert open(depth3).read() == alone("contig_depth", "all.fasta", "cli_depth.tsv", ["--depth-edge", "30"])
    assert open(damage3).read() == alone("contig_damage", "all.fasta", "cli_damage.tsv", ["--damage-ends", "12"])
