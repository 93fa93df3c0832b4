"""`carpedeam contig_map` on the device: the SAM file against the text tests/map_model.py writes for the records the same four library
calls give - compared as bytes - and against map_model.sam_check, which looks at the file and the contigs alone."""
import os
import subprocess

import numpy as np
import pytest

import map_model as mm
from carpedeam_amd import capi
from stageflags import K_FLAGS, R_FLAGS
from test_gpu_contig_breaks_cli import NAMES, build_corpus, createdb_order, write_fasta, write_fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT = os.path.join(ROOT, "carpedeam_amd", "carpedeam")
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")


@pytest.fixture(scope="module", autouse=True)
def built():
    from carpedeam_amd import build
    build.build()


NAMES = NAMES + ["ctg4"]
SHARED, ODD = (100, 300), range(0, 48, 2)          # ctg1's letters that ctg4 repeats; the reads written with letters beyond ACGT


def map_corpus():
    """the corpus of tests/test_gpu_contig_breaks_cli.py (three contigs of 400 letters, ctg3 with a lower-case stretch and IUPAC letters,
    330 reads of 40..80 letters on both strands) and, for what a SAM writer adds to the tables: a fourth contig that repeats ctg1[100:300]
    between letters of its own, so that reads of that stretch seed on two contigs and have a secondary line (established on the CPU oracle
    before the first run on a device: 12 reads with two records), and 24 reads rewritten with a lower-case stretch, IUPAC letters and N"""
    c = build_corpus()
    rng = np.random.default_rng(2026)
    own = ["".join(rng.choice(list("ACGT"), size=n)) for n in (120, 80)]
    contigs = c["contigs"] + [own[0] + c["contigs"][0][SHARED[0]:SHARED[1]] + own[1]]
    reads = list(c["reads"])
    for k, i in enumerate(ODD):
        r = list(reads[i])
        if k % 4 == 0:
            r[5:25] = "".join(r[5:25]).lower()
        elif k % 4 == 1:
            r[7], r[20] = "R", "y"
        elif k % 4 == 2:
            r[11] = "N"
        else:
            r[3], r[15] = "n", "K"
            r[16:30] = "".join(r[16:30]).lower()
        reads[i] = "".join(r)
    return dict(contigs=contigs, reads=reads)


def run(exe, args, **env):
    e = {k: v for k, v in os.environ.items() if k != "CARPEDEAM_REF_BIN"}
    e.update(env)
    return subprocess.run([exe] + args, capture_output=True, text=True, env=e, timeout=300)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """map_corpus() as files; the records of the command's four steps through the Python binding, held against the model once for every
    test below"""
    c = map_corpus()
    c["dir"] = d = tmp_path_factory.mktemp("contig_map")
    write_fasta(d / "contigs.fa", NAMES, c["contigs"])
    write_fastq(d / "reads.fq", c["reads"])
    assert K_FLAGS[-2:] == ["-k", "20"] and "--min-seq-id 0.9" in " ".join(R_FLAGS)
    order = createdb_order(len(c["reads"]))
    reads = [c["reads"][i] for i in order]
    nc = len(c["contigs"])
    ctx = capi.Ctx(0)
    both = ctx.concat(ctx.upload_seqs(c["contigs"]), ctx.upload_seqs(reads), 1, 0)
    alns = ctx.rescore(both, ctx.kmermatch(both, capi.KmerParams.reads_default()), capi.RescoreParams.default())
    off, rec = alns.download()
    queries = list(range(nc))
    stats, recs, mism = mm.map_records(c["contigs"] + reads, [1] * nc + [0] * len(reads), off, rec, queries, 0.0, True)
    got = ctx.pileup_map(both, alns, queries, 0.0, True, records=True)
    assert np.array_equal(got[0], stats) and np.array_equal(got[1], recs) and np.array_equal(got[2], mism)
    c["stats"], c["recs"], c["mism"] = stats, recs, mism
    c["text"] = lambda **kw: mm.sam_text(NAMES, [len(s) for s in c["contigs"]], lambda t: "r%d" % order[t - nc], lambda t: reads[t - nc], recs, mism, **kw)
    c["by_name"] = dict(zip(NAMES, c["contigs"]))
    c["name_of"] = lambda t: "r%d" % order[t - nc]
    return c


def record_lines(text):
    return [l for l in text.split("\n") if l and not l.startswith("@")]


def test_contig_map_from_fastq(corpus):
    d = corpus["dir"]
    log, out = str(d / "dispatch.log"), str(d / "out.sam")
    r = run(FRONT, ["contig_map", str(d / "contigs.fa"), str(d / "reads.fq"), out, "--threads", "4"], CARPEDEAM_DISPATCH_LOG=log)
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(log).read() == "gpu contig_map\n"
    text = open(out).read()
    assert text == corpus["text"]()
    reads_with_lines = mm.sam_check(text, corpus["by_name"])
    recs, stats = corpus["recs"], corpus["stats"]
    # the corpus does reach the cases: most reads map, on both strands, some with mismatches (ctg3's N and IUPAC letters)
    assert reads_with_lines >= 150 and reads_with_lines == int(stats[:, 3].sum()) == len(set(recs["target"].tolist()))
    assert (recs["flags"] & mm.REVERSE).any() and (recs["flags"] & mm.REVERSE == 0).any() and stats[:, 2].sum() > 0
    assert text.count("\n") == 6 + len(recs)
    lines = [l.split("\t") for l in record_lines(text)]
    assert "N" in "".join(l[12] for l in lines)
    # reads with two lines, on ctg1 and on ctg4: one of them carries 256, forward (256) and reverse (272)
    n_secondary = int((recs["flags"] & mm.SECONDARY != 0).sum())
    assert n_secondary >= 5 and sum(1 for l in lines if int(l[1]) & 256) == n_secondary and len(recs) == reads_with_lines + n_secondary
    assert {l[1] for l in lines} == {"0", "16", "256", "272"}
    twice = {l[0] for l in lines if int(l[1]) & 256}
    assert all(sorted(l[2] for l in lines if l[0] == name) == ["ctg1", "ctg4"] for name in twice)
    # the reads written with letters beyond ACGT: SEQ shows the mapped letters on either strand (R as G, y as C, lower case as upper)
    odd = {"r%d" % i: corpus["reads"][i] for i in ODD}
    shown = [(l[0], int(l[1]) & 16, l[9]) for l in lines if l[0] in odd]
    assert len(shown) >= 20 and {rev for _, rev, _ in shown} == {0, 16}
    for name, rev, seq in shown:
        want = mm.mapped(odd[name])
        assert seq == (want.translate(mm.COMPLEMENT)[::-1] if rev else want) and seq == seq.upper() and set(seq) <= set("ACGTN"), name
    assert any("N" in seq for _, rev, seq in shown if rev) and any("N" in seq for _, rev, seq in shown if not rev)
    assert mm.mapped("aRyKn") == "AGCGN"


def test_contig_map_from_dbs_with_header_dbs(corpus):
    d = corpus["dir"]
    for src, db, shuffle in (("contigs.fa", "contigsdb", "0"), ("reads.fq", "readsdb", "1")):
        r = run(FRONT, ["createdb", str(d / src), str(d / db), "--shuffle", shuffle])
        assert r.returncode == 0 and os.path.exists(d / (db + "_h.index")), r.stderr[-1500:]
    r = run(EXE, ["contig_map", str(d / "contigsdb"), str(d / "readsdb"), str(d / "db.sam")])
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(d / "db.sam").read() == corpus["text"]()


def test_read_group_and_primary_only(corpus):
    d = corpus["dir"]
    r = run(EXE, ["contig_map", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "rg.sam"), "--read-group", "lib 1", "--primary-only", "1", "--threads", "3"])
    assert r.returncode == 0, r.stderr[-1500:]
    text = open(d / "rg.sam").read()
    assert text == corpus["text"](read_group="lib 1", primary_only=True)
    assert "@RG\tID:lib 1\n" in text and mm.sam_check(text, corpus["by_name"]) == int(corpus["stats"][:, 3].sum())
    lines = record_lines(text)
    assert len(lines) == int(corpus["stats"][:, 3].sum()) and all(l.endswith("\tRG:Z:lib 1") for l in lines)
    r = run(EXE, ["contig_map", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "all.sam"), "--primary-only", "0", "--read-group", "lib 1"])
    assert r.returncode == 0 and open(d / "all.sam").read() == corpus["text"](read_group="lib 1")
    # the filter leaves out exactly the lines with 256, and there are some
    every = record_lines(open(d / "all.sam").read())
    dropped = [l for l in every if int(l.split("\t")[1]) & 256]
    assert len(dropped) >= 5 and [l for l in every if not int(l.split("\t")[1]) & 256] == lines and len(every) == len(lines) + len(dropped)


def test_small_batches_give_the_same_bytes(corpus):
    """CDM_MAP_BATCH=64: batches of at most 64 records, every contig alone and its records in several work items and launches; the
    primary of a read on ctg1 and ctg4 - two batches - is still chosen over the whole call"""
    d = corpus["dir"]
    r = run(EXE, ["contig_map", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "small.sam")], CDM_MAP_BATCH="64", CDM_PILEUP_CHUNK="50", CDM_LAUNCH_SLICE="3")
    assert r.returncode == 0, r.stderr[-1500:]
    text = open(d / "small.sam").read()
    assert text == corpus["text"]() and "\t256\t" in text and "\t272\t" in text
    r = run(EXE, ["contig_map", str(d / "contigs.fa"), str(d / "reads.fq"), str(d / "small1.sam"), "--primary-only", "1"], CDM_MAP_BATCH="64", CDM_PILEUP_CHUNK="50")
    assert r.returncode == 0 and open(d / "small1.sam").read() == corpus["text"](primary_only=True)


def test_an_empty_contig_file_gives_the_header_lines_without_sq(corpus):
    d = corpus["dir"]
    open(d / "empty.fa", "w").close()
    r = run(EXE, ["contig_map", str(d / "empty.fa"), str(d / "reads.fq"), str(d / "empty.sam"), "--read-group", "g"])
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(d / "empty.sam").read() == "@HD\tVN:1.6\tSO:coordinate\n@RG\tID:g\n@PG\tID:carpedeam\tPN:carpedeam\n"


def test_reads_without_sequences_are_an_error(corpus):
    d = corpus["dir"]
    open(d / "none.fq", "w").close()
    r = run(EXE, ["contig_map", str(d / "contigs.fa"), str(d / "none.fq"), str(d / "none.sam")])
    assert r.returncode == 1 and "holds no reads" in r.stderr
    assert not os.path.exists(d / "none.sam")


def test_two_contigs_of_one_name_are_an_error(corpus):
    d = corpus["dir"]
    write_fasta(d / "twice.fa", ["ctg1", "ctg2", "ctg1", "ctg4"], corpus["contigs"])
    r = run(EXE, ["contig_map", str(d / "twice.fa"), str(d / "reads.fq"), str(d / "twice.sam")])
    assert r.returncode == 1 and "two contigs are named ctg1" in r.stderr
    assert not os.path.exists(d / "twice.sam")
