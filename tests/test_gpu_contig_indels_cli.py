"""`carpedeam contig_indels` on the device: the summary, the sites file and the polished FASTA against the texts tests/indels_model.py
writes for the records the command's own library calls give through the Python binding - compared as bytes - on a corpus with planted
contig errors that the defaults have to find and repair.

The corpus (planted_corpus): one genome of 700 letters (seed 7) with a five-letter homopolymer; ctg1 is the genome with the four plants
of tests/indelcases.py (a letter missing at 150, two letters too many in front of 290, the homopolymer at 430 one letter short, three
letters missing at 560); ctg2 is a second, clean sequence of 320 letters with a lower-case stretch; error-free reads of 80 letters every
3 positions of either, on alternating strands; 10 reads of the genome that lack its letter 70 and 8 reads of ctg2 with two letters too
many in front of its letter 200, the minority alleles."""
import os
import subprocess

import numpy as np
import pytest

import gapped_model as gm
import indelcases as ic
import indels_model as im
import pileupcases as pc
from carpedeam_amd import capi
from test_gpu_contig_breaks_cli import createdb_order, write_fasta, write_fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
NAMES = ["ctg1", "ctg2"]
SMALL = dict(CDM_INDEL_POSITIONS="256", CDM_PILEUP_CHUNK="50", CDM_LAUNCH_SLICE="7")


@pytest.fixture(scope="module", autouse=True)
def built():
    from carpedeam_amd import build
    build.build()


def run(args, **env):
    e = {k: v for k, v in os.environ.items() if k != "CARPEDEAM_REF_BIN"}
    e.update(env)
    return subprocess.run([EXE] + args, capture_output=True, text=True, env=e, timeout=300)


def planted_corpus():
    genome, contig, _ = ic.planted_genome(7)
    rng = np.random.default_rng(77)
    clean = pc.rand_seq(rng, 320)
    reads = [r for _, r, _ in ic.planted_reads(genome, strands="alternate")] + [r for _, r, _ in ic.planted_reads(clean, strands="alternate")]
    for k, s in enumerate(range(20, 60, 4)):           # the genome's letter 70 missing, 22..50 letters into the read
        r = genome[s:70] + genome[71:s + 81]
        reads.append(ic.revcomp(r) if k % 2 else r)
    for k, s in enumerate(range(140, 172, 4)):         # "CA" too many in front of the clean contig's letter 200
        r = clean[s:200] + "CA" + clean[200:s + 78]
        reads.append(ic.revcomp(r) if k % 2 else r)
    assert all(len(r) == 80 for r in reads)
    return dict(genome=genome, contigs=[contig, clean[:100] + clean[100:140].lower() + clean[140:]], reads=reads)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """the corpus as files; per (thresholds, gap flags) the results of the command's library calls through the binding, held against the
    model once, and the three texts the model writes for them"""
    c = planted_corpus()
    c["dir"] = d = tmp_path_factory.mktemp("contig_indels")
    write_fasta(d / "contigs.fa", NAMES, c["contigs"])
    write_fastq(d / "reads.fq", c["reads"])
    reads = [c["reads"][i] for i in createdb_order(len(c["reads"]))]
    nc = len(c["contigs"])
    seqs, ext, queries = c["contigs"] + reads, [1] * nc + [0] * len(reads), list(range(nc))
    ctx = capi.Ctx(0)
    both = ctx.concat(ctx.upload_seqs(c["contigs"]), ctx.upload_seqs(reads), 1, 0)
    hits = ctx.kmermatch(both, capi.KmerParams.reads_default())
    alns = ctx.rescore(both, hits, capi.RescoreParams.default())
    off, rec = alns.download()
    memo = {}

    def results(min_depth=3, min_count=2, min_percent=20, band=8, min_columns=32):
        key = (min_depth, min_count, min_percent, band, min_columns)
        if key not in memo:
            _, grecs, gops, _ = ctx.pileup_gapped(both, hits, alns, queries, capi.GapParams.default(0.0, True, band, min_columns, 900), records=True)
            want = im.indels_sorted(seqs, ext, off, rec, queries, grecs, gops, im.Params(min_depth, min_count, min_percent, 0.0, True))
            got = ctx.pileup_indels(both, alns, queries, grecs, gops, capi.IndelParams.default(min_depth, min_count, min_percent, 0.0, True), track=True, sites=True)
            assert np.array_equal(got[0], want[0]) and all(np.array_equal(g, w) for g, w in zip(got[1], want[1])) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
            memo[key] = want + (grecs,)
        return memo[key]

    def texts(**kw):
        stats, _, sites, letters, _ = results(**kw)
        return (im.summary_tsv(NAMES, queries, c["contigs"], stats, sites, letters), im.sites_tsv(NAMES, c["contigs"], sites, letters),
                im.consensus_fasta(NAMES, c["contigs"], sites, letters))

    c["results"], c["texts"] = results, texts
    return c


def command(d, out, *flags):
    return ["contig_indels", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / (out + ".tsv")), "--sites", str(d / (out + ".sites")), "--consensus", str(d / (out + ".fa"))] + list(flags)


def files(d, out):
    return tuple(open(d / (out + ext)).read() for ext in (".tsv", ".sites", ".fa"))


def test_the_corpus_meets_its_conditions(corpus):
    """by the model alone, on the device's records"""
    stats, _, sites, letters, grecs = corpus["results"]()
    flags, kind = sites["info"] >> 16, sites["info"] & 15
    major = (flags & im.MAJOR) != 0
    assert (major & (kind == im.INS)).any() and (major & (kind == im.DEL)).any() and (~major).any()
    assert {int(f) & gm.REVERSE for f in grecs["flags"]} == {0, gm.REVERSE}
    polished = [im.apply_consensus(c, sites[sites["query"] == i], letters)[0] for i, c in enumerate(corpus["contigs"])]
    assert polished[1] == corpus["contigs"][1] and polished[0] == corpus["genome"] and polished[0] != corpus["contigs"][0]
    assert not (major & (sites["query"] == 1)).any() and int(stats[0][9]) >= 4 and int(stats[:, 2].sum()) == len(grecs) >= 40


def test_summary_sites_and_consensus(corpus):
    d = corpus["dir"]
    r = run(command(d, "all"))
    assert r.returncode == 0, r.stderr[-1500:]
    summary, sites, fasta = files(d, "all")
    want = corpus["texts"]()
    assert summary == want[0] and sites == want[1] and fasta == want[2]
    assert fasta == ">ctg1\n%s\n>ctg2\n%s\n" % (corpus["genome"], corpus["contigs"][1])
    lines = [l.split("\t") for l in summary.split("\n")[1:-1]]
    assert [l[0] for l in lines] == NAMES and int(lines[0][-2]) >= 4 and lines[0][-1] == "700" and lines[1][-2:] == ["0", "320"]
    assert {l.split("\t")[-1] for l in sites.split("\n")[:-1]} == {"S", "SM"}
    # the summary alone: the same bytes, and neither of the other files
    r = run(["contig_indels", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "alone.tsv")])
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(d / "alone.tsv").read() == summary and not os.path.exists(d / "alone.sites") and not os.path.exists(d / "alone.fa")


def test_thresholds_and_gap_flags(corpus):
    d = corpus["dir"]
    r = run(command(d, "strict", "--min-depth", "5", "--min-indel-count", "4", "--min-indel-percent", "60", "--gap-band", "2", "--gap-min-columns", "70"))
    assert r.returncode == 0, r.stderr[-1500:]
    got, want = files(d, "strict"), corpus["texts"](min_depth=5, min_count=4, min_percent=60, band=2, min_columns=70)
    assert got == want and want != corpus["texts"]()
    assert all(l.endswith("\tSM") for l in got[1].split("\n")[:-1])             # (60 percent: every supported site is major)


def test_small_batches_give_the_same_bytes(corpus):
    d = corpus["dir"]
    r = run(command(d, "small"), CDM_GAP_TRACE_BUDGET="100000", **SMALL)
    assert r.returncode == 0, r.stderr[-1500:]
    assert files(d, "small") == corpus["texts"]()


def test_no_contigs_gives_an_empty_table(corpus, tmp_path):
    (tmp_path / "none.fa").write_text("")
    r = run(["contig_indels", str(tmp_path / "none.fa"), str(corpus["dir"] / "reads.fq"), str(tmp_path / "none.tsv"), "--sites", str(tmp_path / "none.sites"), "--consensus", str(tmp_path / "none.out")])
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(tmp_path / "none.tsv").read() == im.HEADER and open(tmp_path / "none.sites").read() == "" and open(tmp_path / "none.out").read() == ""
