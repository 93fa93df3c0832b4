"""`carpedeam contig_links` on the device: its three files, with and without --dedup 1, against the text the writers of
tests/links_model.py give for the alignment set that the same library calls give through the binding - compared as text.  The corpus is
built here: a genome of 1600 letters cut into three contigs - 12 letters missing between the first two, the last two overlapping by 9,
the third reverse-complemented - and a fourth contig of other letters; reads of 100 letters from both strands every 2 letters, and a
few copies of one read across the first junction."""
import os
import subprocess

import numpy as np
import pytest

import dedup_model
import links_model as lm
from carpedeam_amd import capi
from stageflags import K_FLAGS, R_FLAGS
from test_gpu_contig_breaks_cli import COMP, createdb_order, write_fasta, write_fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT = os.path.join(ROOT, "carpedeam_amd", "carpedeam")
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
NAMES = ["left", "middle", "right_rc", "other"]
CUTS = ((0, 500), (512, 1000), (991, 1600))         # 12 letters between the first two, 9 shared by the last two
COPIES, COPIED_AT = 3, 450                          # the read at 450: 50 letters on `left`, 12 between, 38 on `middle`


@pytest.fixture(scope="module", autouse=True)
def built():
    from carpedeam_amd import build
    build.build()


def run(exe, args, **env):
    e = {k: v for k, v in os.environ.items() if k != "CARPEDEAM_REF_BIN"}
    e.update(env)
    return subprocess.run([exe] + args, capture_output=True, text=True, env=e, timeout=300)


def build_corpus():
    rng = np.random.default_rng(1600)
    genome = "".join(rng.choice(list("ACGT"), size=1600))
    contigs = [genome[a:b] for a, b in CUTS]
    contigs[2] = contigs[2].translate(COMP)[::-1]
    contigs.append("".join(rng.choice(list("ACGT"), size=300)))
    reads = []
    for i, at in enumerate(range(0, 1501, 2)):
        r = genome[at:at + 100]
        reads.append(r.translate(COMP)[::-1] if i % 2 else r)
    source = reads[COPIED_AT // 2]
    assert source == genome[COPIED_AT:COPIED_AT + 100] or source.translate(COMP)[::-1] == genome[COPIED_AT:COPIED_AT + 100]
    return dict(contigs=contigs, reads=reads + [source] * COPIES)


def pipeline(ctx, contigs, reads, k=20, min_seq_id=0.9):
    """the steps of the command through the Python binding: the joint DB in createdb's read order, kmermatcher, rescorediagonal, with
    --dedup 1 cdm_alns_dedup over the contigs, then cdm_pileup_links - each held against its model here, once -> per dedup (stats,
    totals, links) of the model"""
    assert K_FLAGS[-2:] == ["-k", "20"] and "--min-seq-id 0.9" in " ".join(R_FLAGS)
    laid = [reads[i] for i in createdb_order(len(reads))]
    nc = len(contigs)
    both = ctx.concat(ctx.upload_seqs(contigs), ctx.upload_seqs(laid), 1, 0)
    kp = capi.KmerParams.reads_default()
    kp.kmer_size = k
    rp = capi.RescoreParams.default()
    rp.seq_id_thr = min_seq_id
    alns = ctx.rescore(both, ctx.kmermatch(both, kp), rp)
    off, rec = alns.download()
    queries, seqs, ext = list(range(nc)), contigs + laid, [1] * nc + [0] * len(laid)
    d_off, d_rec, _, d_stats = dedup_model.dedup(seqs, ext, off, rec, queries, 0.0, True)
    unique, got_stats = ctx.alns_dedup(both, alns, queries, 0.0, True)
    got_off, got_rec = unique.download()
    assert np.array_equal(got_stats, d_stats) and np.array_equal(got_off, d_off) and got_rec.tobytes() == d_rec.tobytes()
    out = {}
    par = capi.LinksParams.default(skip_extended_targets=True)
    for dedup, (o, r, h) in ((False, (off, rec, alns)), (True, (d_off, d_rec, unique))):
        want = lm.links(seqs, ext, o, r, queries, min_seq_id=0.0, skip=True, **lm.DEFAULTS)
        got = ctx.pileup_links(both, h, queries, par, links=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2].tobytes() == want[2].tobytes()
        out[dedup] = want
    out["removed"] = int(d_stats[:, 2].sum())
    return out


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    c = build_corpus()
    c["dir"] = d = tmp_path_factory.mktemp("contig_links")
    write_fasta(d / "contigs.fa", NAMES, c["contigs"])
    write_fastq(d / "reads.fq", c["reads"])
    c["p"] = pipeline(capi.Ctx(0), c["contigs"], c["reads"])
    c["lengths"] = [len(s) for s in c["contigs"]]
    c["io"] = [str(d / "contigs.fa"), str(d / "reads.fq")]
    return c


def junction(found, a, b, info):
    hit = found[(found["a"] == a) & (found["b"] == b) & (found["info"] == info)]
    assert len(hit) == 1, (a, b, info, found.tolist())
    return hit[0]


def test_the_plants_do_what_they_are_planted_for(corpus):
    """each of the two junctions shows as one link with the planted orientations and gap and at least two reads; without the duplicates
    the first junction has exactly the planted copies fewer, the second as many as before"""
    p = corpus["p"]
    for dedup in (False, True):
        found = p[dedup][2]
        first, second = junction(found, 0, 1, 0), junction(found, 1, 2, 2)         # left + -> middle +, middle + -> right_rc -
        print("dedup", dedup, "links", found.tolist(), "totals", p[dedup][1].tolist())
        assert int(first["gap_mode"]) == 12 and int(second["gap_mode"]) == -9
        assert int(first["reads"]) >= 2 and int(second["reads"]) >= 2
        assert not ((found["a"] == 3) | (found["b"] == 3)).any() and int(p[dedup][0][3, 2:5].sum()) == 0       # the fourth contig has no read
    assert int(junction(p[False][2], 0, 1, 0)["reads"]) - int(junction(p[True][2], 0, 1, 0)["reads"]) == COPIES
    assert int(junction(p[False][2], 1, 2, 2)["reads"]) == int(junction(p[True][2], 1, 2, 2)["reads"])
    assert p["removed"] == 2 * COPIES           # a record on either contig per copy


def test_the_three_files(corpus):
    d, p = corpus["dir"], corpus["p"]
    texts = {}
    for flags, dedup, tag in ((["--dedup", "1"], True, "l1"), (["--dedup", "0"], False, "l0"), ([], False, "l")):
        files = [str(d / (tag + x)) for x in (".tsv", "_ends.tsv", ".gfa")]
        log = str(d / (tag + "_dispatch.log"))
        r = run(FRONT, ["contig_links"] + corpus["io"] + [files[0], "--ends", files[1], "--gfa", files[2], "--threads", "4"] + flags, CARPEDEAM_DISPATCH_LOG=log, CDM_TIMING="1")
        assert r.returncode == 0, r.stderr[-1500:]
        assert open(log).read() == "gpu contig_links\n"
        stats, totals, found = p[dedup]
        texts[tag] = [open(f).read() for f in files]
        assert texts[tag][0] == lm.links_tsv(NAMES, found), tag
        assert texts[tag][1] == lm.ends_tsv(NAMES, [0, 1, 2, 3], corpus["lengths"], stats), tag
        assert texts[tag][2] == lm.gfa(NAMES, corpus["contigs"], found), tag
        assert "link report: " in r.stderr and " %d end records, " % int(totals[0]) in r.stderr and " %d returned, " % len(found) in r.stderr
    assert texts["l0"] == texts["l"] and texts["l0"][0] != texts["l1"][0]
    # the overlap is an L line, the junction with letters between its contigs is in the table only
    assert "L\tmiddle\t+\tright_rc\t-\t9M\tRC:i:" in texts["l"][2] and "L\tleft" not in texts["l"][2] and texts["l"][0].startswith("left\t+\tmiddle\t+\t")
    # the table alone, and other thresholds
    r = run(EXE, ["contig_links"] + corpus["io"] + [str(d / "alone.tsv")])
    assert r.returncode == 0 and open(d / "alone.tsv").read() == texts["l"][0] and not os.path.exists(d / "alone_ends.tsv")
    r = run(EXE, ["contig_links"] + corpus["io"] + [str(d / "many.tsv"), "--min-link-reads", "1000"])
    assert r.returncode == 0 and open(d / "many.tsv").read() == ""


def test_an_empty_contig_file(corpus):
    d = corpus["dir"]
    open(d / "empty.fa", "w").close()
    r = run(EXE, ["contig_links", str(d / "empty.fa"), corpus["io"][1], str(d / "e.tsv"), "--ends", str(d / "e_ends.tsv"), "--gfa", str(d / "e.gfa")])
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(d / "e.tsv").read() == "" and open(d / "e_ends.tsv").read() == "" and open(d / "e.gfa").read() == "H\tVN:Z:1.0\n"


def test_two_contigs_of_one_name_end_the_command(corpus):
    d = corpus["dir"]
    write_fasta(d / "twice.fa", ["left", "middle", "left", "other"], corpus["contigs"])
    r = run(EXE, ["contig_links", str(d / "twice.fa"), corpus["io"][1], str(d / "t.tsv"), "--gfa", str(d / "t.gfa")])
    assert r.returncode == 1 and r.stderr.endswith("contig_links: two contigs are named left; a link can not tell them apart\n")
    assert not os.path.exists(d / "t.tsv") and not os.path.exists(d / "t.gfa")
