"""`carpedeam contig_map --gapped 1` on the device: the SAM file against the text tests/gapped_model.py writes for the records of the
command's own library calls - compared as bytes - against gapped_model.sam_check_gapped, which looks at the file and the contigs
alone, and against the file without the flag: every line of that file is still there, unchanged."""
import os
import re
import subprocess

import numpy as np
import pytest

import gapped_model as gm
import map_model as mm
from carpedeam_amd import capi
from test_gpu_contig_breaks_cli import createdb_order, write_fasta, write_fastq
from test_gpu_contig_map_cli import NAMES, map_corpus

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")


@pytest.fixture(scope="module", autouse=True)
def built():
    from carpedeam_amd import build
    build.build()


def gapped_corpus():
    """the corpus of tests/test_gpu_contig_map_cli.py and 90 reads more of 60..80 letters on both strands, each with an inserted or a
    deleted stretch of 1..3 letters: on ctg1's stretch that ctg4 repeats (two rescued lines a read, one of them secondary), elsewhere on
    ctg1, and on ctg3 across its lower-case stretch and IUPAC letters"""
    c = map_corpus()
    rng = np.random.default_rng(4242)
    reads = list(c["reads"])
    for i in range(90):
        contig = mm.mapped(c["contigs"][(0, 0, 2)[i % 3]]).replace("N", "A")
        n = int(rng.integers(60, 81))
        at = int(rng.integers(110, 200)) if i % 3 == 0 else int(rng.integers(0, 400 - n - 4))
        g, p = int(rng.integers(1, 4)), int(rng.integers(25, n - 25))
        r = contig[at:at + n + 4]
        r = (r[:p] + "".join(rng.choice(list("ACGT"), size=g)) + r[p:] if i % 2 else r[:p] + r[p + g:])[:n]
        reads.append(r.translate(mm.COMPLEMENT)[::-1] if (i // 2) % 2 else r)
    return dict(contigs=c["contigs"], reads=reads)


def run(args, **env):
    e = {k: v for k, v in os.environ.items() if k != "CARPEDEAM_REF_BIN"}
    e.update(env)
    return subprocess.run([EXE] + args, capture_output=True, text=True, env=e, timeout=300)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """gapped_corpus() as files; the records of the command's library calls through the Python binding, held against both models once"""
    c = gapped_corpus()
    c["dir"] = d = tmp_path_factory.mktemp("contig_gapped")
    write_fasta(d / "contigs.fa", NAMES, c["contigs"])
    write_fastq(d / "reads.fq", c["reads"])
    order = createdb_order(len(c["reads"]))
    reads = [c["reads"][i] for i in order]
    nc = len(c["contigs"])
    seqs, ext = c["contigs"] + reads, [1] * nc + [0] * len(reads)
    ctx = capi.Ctx(0)
    both = ctx.concat(ctx.upload_seqs(c["contigs"]), ctx.upload_seqs(reads), 1, 0)
    hits = ctx.kmermatch(both, capi.KmerParams.reads_default())
    alns = ctx.rescore(both, hits, capi.RescoreParams.default())
    hoff, hrec = hits.download()
    aoff, arec = alns.download()
    queries = list(range(nc))
    _, recs, mism = mm.map_records(seqs, ext, aoff, arec, queries, 0.0, True)

    memo = {}

    def records(band=8, min_columns=32):
        if (band, min_columns) in memo:
            return memo[(band, min_columns)]
        p = gm.Params(0.0, True, band, min_columns, 900)
        want = gm.gapped_records(seqs, ext, hoff, hrec, aoff, arec, queries, p)
        got = ctx.pileup_gapped(both, hits, alns, queries, capi.GapParams.default(0.0, True, band, min_columns, 900), records=True)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        memo[(band, min_columns)] = want
        return want

    def text(band=8, min_columns=32, **kw):
        _, grecs, gops, gwords = records(band, min_columns)
        return gm.sam_text_gapped(NAMES, [len(s) for s in c["contigs"]], lambda t: "r%d" % order[t - nc], lambda t: reads[t - nc], recs, mism, grecs, gops, gwords, **kw)

    c["records"], c["text"], c["recs"] = records, text, recs
    c["by_name"] = dict(zip(NAMES, c["contigs"]))
    return c


def record_lines(text):
    return [l for l in text.split("\n") if l and not l.startswith("@")]


def test_the_gapped_file_and_the_file_without_the_flag(corpus):
    d = corpus["dir"]
    files = [str(d / "contigs.fa"), str(d / "reads.fq")]
    r = run(["contig_map"] + files + [str(d / "gapped.sam"), "--gapped", "1", "--threads", "4"])
    assert r.returncode == 0, r.stderr[-1500:]
    text = open(d / "gapped.sam").read()
    assert text == corpus["text"]()
    reads_with_lines, rescued = gm.sam_check_gapped(text, corpus["by_name"])
    stats, grecs, gops, _ = corpus["records"]()
    assert rescued == len(grecs) >= 60 and reads_with_lines == len(set(corpus["recs"]["target"].tolist()) | set(grecs["target"].tolist()))
    # the corpus does reach the cases: insertions and deletions on both strands, rescued secondaries (ctg1 and ctg4), a gap-free rescue
    lines = [l.split("\t") for l in record_lines(text) if "\tXG:i:" in l]
    assert {l[1] for l in lines} >= {"0", "16"} and any(int(l[1]) & 256 for l in lines)
    assert any("I" in l[5] for l in lines if l[1] == "0") and any("D" in l[5] for l in lines if l[1] == "0")
    assert any("I" in l[5] for l in lines if l[1] == "16") and any("D" in l[5] for l in lines if l[1] == "16") and any("^" in l[12] for l in lines)
    assert all(l[-1] == "XG:i:%d" % sum(int(x) for x in re.findall(r"(\d+)[ID]", l[5])) for l in lines)
    # without its XG lines the file is the file of --gapped 0, which is the file without the flag
    r = run(["contig_map"] + files + [str(d / "zero.sam"), "--gapped", "0"])
    assert r.returncode == 0, r.stderr[-1500:]
    r = run(["contig_map"] + files + [str(d / "plain.sam")])
    assert r.returncode == 0, r.stderr[-1500:]
    zero = open(d / "zero.sam").read()
    assert zero == open(d / "plain.sam").read()
    assert "".join(l + "\n" for l in text.split("\n")[:-1] if "\tXG:i:" not in l) == zero and "XG:i:" not in zero and len(record_lines(zero)) == len(corpus["recs"])


def test_primary_only_read_group_and_the_two_gap_flags(corpus):
    d = corpus["dir"]
    files = [str(d / "contigs.fa"), str(d / "reads.fq")]
    r = run(["contig_map"] + files + [str(d / "primary.sam"), "--gapped", "1", "--primary-only", "1", "--read-group", "lib 1", "--threads", "3"])
    assert r.returncode == 0, r.stderr[-1500:]
    text = open(d / "primary.sam").read()
    assert text == corpus["text"](read_group="lib 1", primary_only=True)
    every = record_lines(corpus["text"](read_group="lib 1"))
    dropped = [l for l in every if int(l.split("\t")[1]) & 256 and "\tXG:i:" in l]
    assert len(dropped) >= 1 and record_lines(text) == [l for l in every if not int(l.split("\t")[1]) & 256]
    assert all(l.endswith("\tRG:Z:lib 1") or "\tRG:Z:lib 1\tXG:i:" in l for l in record_lines(text))
    gm.sam_check_gapped(text, corpus["by_name"])
    r = run(["contig_map"] + files + [str(d / "narrow.sam"), "--gapped", "1", "--gap-band", "2", "--gap-min-columns", "70"])
    assert r.returncode == 0, r.stderr[-1500:]
    narrow = open(d / "narrow.sam").read()
    assert narrow == corpus["text"](band=2, min_columns=70)
    n = sum(1 for l in record_lines(narrow) if "\tXG:i:" in l)
    assert 0 < n < len(corpus["records"]()[1])


def test_small_batches_give_the_same_bytes(corpus):
    d = corpus["dir"]
    r = run(["contig_map", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "small.sam"), "--gapped", "1"], CDM_MAP_BATCH="64", CDM_PILEUP_CHUNK="50", CDM_LAUNCH_SLICE="7",
            CDM_GAP_TRACE_BUDGET="100000")
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(d / "small.sam").read() == corpus["text"]()
