"""`carpedeam contig_depth`, `contig_variants` and `contig_breaks` with --gapped 1 on the device: every file a command writes against the
text the models' writers give for the results of the command's own library calls through the Python binding - compared as bytes - on
a corpus with planted contig errors, where the ungapped tables call a break at every plant and the rescued reads take them away.

The corpus (planted_corpus): one genome of 700 letters (seed 7) with a five-letter homopolymer; ctg1 is the genome with the four plants
of tests/indelcases.py (a letter missing at 150, two letters too many in front of 290, the homopolymer at 430 one letter short, three
letters missing at 560); ctg2 is a second, clean sequence of 320 letters with a lower-case stretch; error-free reads of 80 letters every
3 positions of either, on alternating strands.  A second read set holds every other read."""
import os
import subprocess

import numpy as np
import pytest

import bases_model as bm
import breaks_model as brm
import depth_model as dm
import gapped_tables_model as gt
import indelcases as ic
import pileupcases as pc
from carpedeam_amd import capi
from test_gpu_contig_breaks_cli import createdb_order, write_fasta, write_fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
NAMES = ["ctg1", "ctg2"]
SMALL = dict(CDM_DEPTH_CELLS="256", CDM_BASES_POSITIONS="256", CDM_PILEUP_CHUNK="50", CDM_LAUNCH_SLICE="7")
GAPPED = ("--gapped", "1")


@pytest.fixture(scope="module", autouse=True)
def built():
    from carpedeam_amd import build
    build.build()


def run(args, **env):
    e = {k: v for k, v in os.environ.items() if k != "CARPEDEAM_REF_BIN"}
    e.update(env)
    return subprocess.run([EXE] + args, capture_output=True, text=True, env=e, timeout=300)


def placements(genome, kind, p, n):
    """Where one planted error sits is not one boundary: a letter missing from a run of equal letters is missing at either end of the
    run just as well.  -> the boundaries b, on the genome with this plant alone, at which putting n letters back in (a missing
    stretch) or taking n letters out (extra letters: the boundaries b .. b + n around them) gives the genome"""
    if kind == "extra":
        alone = genome[:p] + "GT"[:n] + genome[p:]
        return sorted({b + j for b in range(len(alone) - n + 1) if alone[:b] + alone[b + n:] == genome for j in range(n + 1)})
    alone = genome[:p] + genome[p + n:]
    return [b for b in range(len(alone) + 1) if alone[:b] + genome[b:b + n] + alone[b:] == genome]


def planted_corpus():
    genome, contig, _ = ic.planted_genome(7)
    rng = np.random.default_rng(77)
    clean = pc.rand_seq(rng, 320)
    reads = [r for _, r, _ in ic.planted_reads(genome, strands="alternate")] + [r for _, r, _ in ic.planted_reads(clean, strands="alternate")]
    at, shift = [], 0              # per plant the contig boundaries it can be placed at
    for kind, p, n in ic.PLANTS:
        at.append([b + shift for b in placements(genome, kind, p, n)])
        shift += n if kind == "extra" else -n
    return dict(genome=genome, contigs=[contig, clean[:100] + clean[100:140].lower() + clean[140:]], reads=reads, second=reads[::2], plants=at)


class Sample:
    """one read set against the contigs through the binding, as the commands lay it out: the alignment set, and per gap flags the
    rescued records"""

    def __init__(self, ctx, contigs, reads):
        self.ctx, self.nc = ctx, len(contigs)
        reads = [reads[i] for i in createdb_order(len(reads))]
        self.seqs, self.ext, self.queries = contigs + reads, [1] * self.nc + [0] * len(reads), list(range(self.nc))
        self.both = ctx.concat(ctx.upload_seqs(contigs), ctx.upload_seqs(reads), 1, 0)
        self.hits = ctx.kmermatch(self.both, capi.KmerParams.reads_default())
        self.alns = ctx.rescore(self.both, self.hits, capi.RescoreParams.default())
        self.off, self.rec = self.alns.download()
        self.memo = {}

    def rescued(self, gapped, band=8, min_columns=32):
        """(recs, ops) of --gapped 1 with the command's scores and gap costs; without the flag no record"""
        if not gapped:
            return np.empty(0, capi.GAP_DTYPE), np.empty(0, np.uint32)
        if (band, min_columns) not in self.memo:
            _, grecs, gops, _ = self.ctx.pileup_gapped(self.both, self.hits, self.alns, self.queries, capi.GapParams.default(0.0, True, band, min_columns, 900), records=True)
            self.memo[band, min_columns] = grecs, gops
        return self.memo[band, min_columns]

    def model_args(self, g):
        return self.seqs, self.ext, self.off, self.rec, self.queries, g[0], g[1]

    def depth(self, gapped, edge=0, **gap):
        g = self.rescued(gapped, **gap)
        got = self.ctx.pileup_depth(self.both, self.alns, self.queries, edge, 0.0, True, track=True, gapped=g if gapped else None)
        want = gt.depth_stats(*self.model_args(g), edge, 0.0, True)
        assert np.array_equal(got[0], want[0]) and all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))
        return got

    def bases(self, gapped, mask_ends=0, min_depth=3, min_alt_count=2, min_alt_percent=20, **gap):
        g = self.rescued(gapped, **gap)
        got = self.ctx.pileup_bases(self.both, self.alns, self.queries, mask_ends, min_depth, min_alt_count, min_alt_percent, 0.0, True, sites=True, gapped=g if gapped else None)
        want = gt.bases(*self.model_args(g), mask_ends, min_depth, min_alt_count, min_alt_percent, 0.0, True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[2])
        return got

    def breaks(self, gapped, anchor=16, edge=50, min_span=1, min_span_percent=0, **gap):
        g = self.rescued(gapped, **gap)
        got = self.ctx.pileup_breaks(self.both, self.alns, self.queries, anchor, edge, min_span, min_span_percent, 0.0, True, track=True, breaks=True, gapped=g if gapped else None)
        want = gt.breaks_stats(*self.model_args(g), anchor, edge, min_span, min_span_percent, 0.0, True)
        assert np.array_equal(got[0], want[0]) and all(np.array_equal(a, b) for a, b in zip(got[1], want[1])) and np.array_equal(got[2], want[2])
        return got


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    c = planted_corpus()
    c["dir"] = d = tmp_path_factory.mktemp("contig_tables_gapped")
    write_fasta(d / "contigs.fa", NAMES, c["contigs"])
    write_fastq(d / "reads.fq", c["reads"])
    write_fastq(d / "second.fq", c["second"])
    ctx = capi.Ctx(0)
    c["all"], c["half"] = Sample(ctx, c["contigs"], c["reads"]), Sample(ctx, c["contigs"], c["second"])
    c["keys"], c["lengths"] = list(range(len(NAMES))), [len(s) for s in c["contigs"]]
    return c


def depth_texts(c, gapped, samples=("all",), **kw):
    got = [c[s].depth(gapped, **kw) for s in samples]
    return dm.tsv(NAMES, c["keys"], c["lengths"], [g[0] for g in got]), dm.bedgraph(NAMES, got[0][1])


def variant_texts(c, gapped, **kw):
    stats, sites = c["all"].bases(gapped, **kw)
    return bm.summary_tsv(NAMES, c["keys"], c["lengths"], stats), bm.sites_tsv(NAMES, sites), bm.consensus_fasta(NAMES, c["contigs"], sites)


def break_texts(c, gapped, min_piece=1, **kw):
    stats, tracks, breaks = c["all"].breaks(gapped, **kw)
    return brm.tsv(NAMES, c["keys"], c["lengths"], stats, breaks), brm.split(NAMES, c["contigs"], breaks, min_piece), brm.bedgraph(NAMES, tracks)


def depth_command(d, out, *flags, reads=("reads.fq",), track=True):
    return ["contig_depth", str(d / "contigs.fa")] + [str(d / r) for r in reads] + [str(d / (out + ".tsv"))] + (["--depth-track", str(d / (out + ".bg"))] if track else []) + list(flags)


def variant_command(d, out, *flags):
    return ["contig_variants", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / (out + ".tsv")), "--sites", str(d / (out + ".sites")), "--consensus", str(d / (out + ".fa"))] + list(flags)


def break_command(d, out, *flags):
    return ["contig_breaks", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / (out + ".tsv")), "--split", str(d / (out + ".fa")), "--span-track", str(d / (out + ".bg"))] + list(flags)


def files(d, out, *exts):
    return tuple(open(d / (out + ext)).read() for ext in exts)


def ok(r):
    assert r.returncode == 0, r.stderr[-1500:]
    return r


def test_the_corpus_meets_its_conditions(corpus):
    """without the flag contig_breaks reports a break whose run covers each of the four plants, with the flag none; with the flag
    contig_depth's sum is larger and the variance it gives (sumsq - sum^2 / window) / (window - 1) is smaller"""
    d = corpus["dir"]
    ok(run(["contig_breaks", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "cond_plain.tsv")]))
    ok(run(["contig_breaks", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "cond_gapped.tsv"), *GAPPED]))
    plain = [l.split("\t") for l in open(d / "cond_plain.tsv").read().split("\n") if l.startswith("#break\t")]
    runs = [(int(l[2]) - 1, int(l[3]) - 1) for l in plain if l[1] == "ctg1"]
    assert [p[0] for p in corpus["plants"]] == [150, 289, 431, 560] and corpus["plants"][2] == [431, 432, 433, 434, 435]
    for at in corpus["plants"]:         # the run holds a boundary the plant can be placed at
        assert any(first <= x <= last for first, last in runs for x in at), (at, runs)
    assert not [l for l in open(d / "cond_gapped.tsv").read().split("\n") if l.startswith("#break\t")]
    ok(run(depth_command(d, "cond_plain_depth", "--depth-edge", "50", track=False)))
    ok(run(depth_command(d, "cond_gapped_depth", "--depth-edge", "50", *GAPPED, track=False)))
    rows = [[l.split("\t") for l in open(d / (name + ".tsv")).read().split("\n")[1:-1]] for name in ("cond_plain_depth", "cond_gapped_depth")]
    head = dm.tsv_header(1).rstrip("\n").split("\t")
    window, s, sq = head.index("window"), head.index("sum_1"), head.index("sumsq_1")
    (w0, s0, q0), (w1, s1, q1) = [(int(r[0][window]), int(r[0][s]), int(r[0][sq])) for r in rows]          # ctg1
    assert w0 == w1 and s1 > s0
    assert q1 * w1 - s1 * s1 < q0 * w0 - s0 * s0                # (window - 1) x window x the variance, in integers


def test_contig_depth_with_rescued_reads(corpus):
    d = corpus["dir"]
    ok(run(depth_command(d, "depth", "--depth-edge", "50", *GAPPED)))
    assert files(d, "depth", ".tsv", ".bg") == depth_texts(corpus, True, edge=50)
    assert files(d, "depth", ".tsv", ".bg") != depth_texts(corpus, False, edge=50)
    # two read sets, each with its own rescued reads; other gap flags
    ok(run(depth_command(d, "depth2", *GAPPED, "--gap-band", "2", "--gap-min-columns", "70", reads=("reads.fq", "second.fq"), track=False)))
    assert files(d, "depth2", ".tsv")[0] == depth_texts(corpus, True, samples=("all", "half"), band=2, min_columns=70)[0]


def test_contig_variants_with_rescued_reads(corpus):
    d = corpus["dir"]
    ok(run(variant_command(d, "var", *GAPPED)))
    assert files(d, "var", ".tsv", ".sites", ".fa") == variant_texts(corpus, True)
    ok(run(variant_command(d, "var2", *GAPPED, "--mask-ends", "3", "--min-depth", "1", "--min-alt-count", "1", "--min-alt-percent", "5", "--gap-band", "4")))
    assert files(d, "var2", ".tsv", ".sites", ".fa") == variant_texts(corpus, True, mask_ends=3, min_depth=1, min_alt_count=1, min_alt_percent=5, band=4)
    assert files(d, "var", ".tsv") != variant_texts(corpus, False)[:1]


def test_contig_breaks_with_rescued_reads(corpus):
    d = corpus["dir"]
    ok(run(break_command(d, "brk", *GAPPED)))
    assert files(d, "brk", ".tsv", ".fa", ".bg") == break_texts(corpus, True)
    assert files(d, "brk", ".fa")[0] == ">ctg1\n%s\n>ctg2\n%s\n" % tuple(corpus["contigs"])          # nothing is cut
    ok(run(break_command(d, "brk2", *GAPPED, "--break-anchor", "30", "--min-span", "8", "--min-span-percent", "60", "--min-piece", "40", "--gap-min-columns", "75")))
    assert files(d, "brk2", ".tsv", ".fa", ".bg") == break_texts(corpus, True, min_piece=40, anchor=30, min_span=8, min_span_percent=60, min_columns=75)


def test_gapped_0_and_no_flag_give_equal_bytes(corpus):
    d = corpus["dir"]
    for command, exts, texts in ((depth_command, (".tsv", ".bg"), depth_texts), (variant_command, (".tsv", ".sites", ".fa"), variant_texts), (break_command, (".tsv", ".fa", ".bg"), break_texts)):
        ok(run(command(d, "none")))
        ok(run(command(d, "zero", "--gapped", "0")))
        assert files(d, "none", *exts) == files(d, "zero", *exts) == texts(corpus, False)


def test_small_batches_give_the_same_bytes(corpus):
    d = corpus["dir"]
    for command, exts, texts in ((depth_command, (".tsv", ".bg"), depth_texts), (variant_command, (".tsv", ".sites", ".fa"), variant_texts), (break_command, (".tsv", ".fa", ".bg"), break_texts)):
        ok(run(command(d, "small", *GAPPED), CDM_GAP_TRACE_BUDGET="100000", **SMALL))
        assert files(d, "small", *exts) == texts(corpus, True)


def test_the_timing_line_reports_the_rescue(corpus):
    d = corpus["dir"]
    r = ok(run(break_command(d, "timed", *GAPPED), CDM_TIMING="1"))
    line = [l for l in r.stderr.split("\n") if "break report:" in l and "rescued" in l]
    assert len(line) == 1 and "candidates" in line[0] and "gapped kernels" in line[0] and "break point kernels" in line[0]
    assert " %d rescued" % len(corpus["all"].rescued(True)[0]) in line[0]
