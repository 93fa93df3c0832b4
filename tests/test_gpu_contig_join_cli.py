"""`carpedeam contig_join` on the device: its three files, with and without --dedup 1, against the writers of tests/join_model.py for the
alignment set that the same library calls give through the binding - compared as text.  The corpus is that of
tests/test_gpu_contig_links_cli.py: a genome of 1600 letters in three contigs, 12 letters missing at the first junction, an overlap of 9
and a strand flip at the second, and a fourth contig of other letters.  The command must give the genome back, letter for letter."""
import os

import numpy as np
import pytest

import join_model as jm
import links_model as lm
from carpedeam_amd import capi
from test_gpu_contig_breaks_cli import COMP, createdb_order, write_fasta, write_fastq
from test_gpu_contig_links_cli import CUTS, EXE, FRONT, NAMES, build_corpus, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    from carpedeam_amd import build
    build.build()


@pytest.fixture(scope="module")
def ctx():
    return capi.Ctx(0)


def genome_of(c):
    return c["contigs"][0] + c["genome_gap"] + c["contigs"][1] + c["contigs"][2].translate(COMP)[::-1][9:]


def pipeline(ctx, names, contigs, reads, dedup, percent=90):
    """the steps of the command through the Python binding -> the model's dict (tests/join_model.py join()), with the links"""
    laid = [reads[i] for i in createdb_order(len(reads))]
    nc = len(contigs)
    both = ctx.concat(ctx.upload_seqs(contigs), ctx.upload_seqs(laid), 1, 0)
    kp = capi.KmerParams.reads_default()
    rp = capi.RescoreParams.default()
    rp.seq_id_thr = 0.9
    alns = ctx.rescore(both, ctx.kmermatch(both, kp), rp)
    queries, seqs, ext = list(range(nc)), contigs + laid, [1] * nc + [0] * len(laid)
    if dedup:
        alns = ctx.alns_dedup(both, alns, queries, 0.0, True)[0]
    off, rec = alns.download()
    links = lm.links(seqs, ext, off, rec, queries, min_seq_id=0.0, skip=True, **lm.DEFAULTS)[2]
    par = capi.LinksParams.default(skip_extended_targets=True)
    assert ctx.pileup_links(both, alns, queries, par, links=True)[2].tobytes() == links.tobytes()

    def junctions(juncs):
        want = jm.junctions(seqs, ext, off, rec, queries, juncs, min_seq_id=0.0, skip=True, anchor=16, overhang=1, max_ends=16)
        got = ctx.pileup_junctions(both, alns, queries, juncs, par, counts=True)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
        return want
    out = jm.join(names, contigs, links, junctions, min_link_reads=2, overlap_percent=percent)
    out["links"] = links
    return out


def command(d, tag, io, flags, exe=EXE, **env):
    files = [str(d / (tag + x)) for x in (".tsv", "_joined.fa", "_paths.tsv")]
    r = run(exe, ["contig_join"] + io + [files[0], "--joined", files[1], "--paths", files[2], "--threads", "4"] + flags, **env)
    assert r.returncode == 0, r.stderr[-1500:]
    return [open(f).read() for f in files], r


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    c = build_corpus()
    rng = np.random.default_rng(1600)
    genome = "".join(rng.choice(list("ACGT"), size=1600))          # (build_corpus draws the genome first from the same seed)
    assert [genome[a:b] for a, b in CUTS[:2]] == c["contigs"][:2]
    c["genome"], c["genome_gap"] = genome, genome[500:512]
    c["dir"] = d = tmp_path_factory.mktemp("contig_join")
    write_fasta(d / "contigs.fa", NAMES, c["contigs"])
    write_fastq(d / "reads.fq", c["reads"])
    c["io"] = [str(d / "contigs.fa"), str(d / "reads.fq")]
    return c


def test_the_genome_comes_back(ctx, corpus):
    d, texts = corpus["dir"], {}
    assert genome_of(corpus) == corpus["genome"]
    for flags, dedup, tag in ((["--dedup", "1"], True, "j1"), (["--dedup", "0"], False, "j0"), ([], False, "j")):
        log = str(d / (tag + "_dispatch.log"))
        texts[tag], r = command(d, tag, corpus["io"], flags, exe=FRONT, CARPEDEAM_DISPATCH_LOG=log, CDM_TIMING="1")
        assert open(log).read() == "gpu contig_join\n"
        want = pipeline(ctx, NAMES, corpus["contigs"], corpus["reads"], dedup)
        print(tag, texts[tag][0], texts[tag][2])
        assert "".join(want["dec"]) == "JJ" and len(want["paths"]) == 1
        assert texts[tag] == [want["joins"], want["joined"], want["paths_tsv"]], tag
        assert texts[tag][1] == ">left_join3\n%s\n>other\n%s\n" % (corpus["genome"], corpus["contigs"][3]), tag
        assert texts[tag][2] == "left_join3\t1\tleft\t+\t1\t500\t0\t0\nleft_join3\t2\tmiddle\t+\t513\t488\t0\t12\nleft_join3\t3\tright_rc\t-\t1001\t609\t9\t0\n"
        voters = sum(int(x) for x in want["res"]["voters"])
        assert "join report: 2 links, 2 junctions, %d voters, 12 fill letters, " % voters in r.stderr
        corpus[tag] = want
    assert texts["j0"] == texts["j"] and texts["j0"][0] != texts["j1"][0] and texts["j0"][1:] == texts["j1"][1:]
    reads = lambda tag: [int(k["reads"]) for k in corpus[tag]["links"]]
    assert reads("j1")[0] < reads("j0")[0] and reads("j1")[1] == reads("j0")[1]            # the planted copies bridge the first junction
    # the table alone
    r = run(EXE, ["contig_join"] + corpus["io"] + [str(d / "alone.tsv")])
    assert r.returncode == 0 and open(d / "alone.tsv").read() == texts["j"][0] and sorted(f for f in os.listdir(d) if f.startswith("alone")) == ["alone.tsv"]


def test_an_overlap_whose_letters_disagree_is_not_joined(ctx, corpus):
    """three of the nine letters that right_rc shares with middle are changed: 6 of 9 columns agree, X at 90 percent, J at 60"""
    d = corpus["dir"]
    contigs = list(corpus["contigs"])
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    s = list(contigs[2])
    for p in (len(s) - 2, len(s) - 5, len(s) - 8):          # its last 9 letters are the reverse complement of the genome's 991 .. 999
        s[p] = other[s[p]]
    contigs[2] = "".join(s)
    assert sum(x != y for x, y in zip(contigs[2], corpus["contigs"][2])) == 3 and contigs[2][:-9] == corpus["contigs"][2][:-9]
    write_fasta(d / "changed.fa", NAMES, contigs)
    io = [str(d / "changed.fa"), corpus["io"][1]]
    texts, _ = command(d, "x90", io, [])
    want = pipeline(ctx, NAMES, contigs, corpus["reads"], False)
    assert texts == [want["joins"], want["joined"], want["paths_tsv"]]
    assert "".join(want["dec"]) == "JX" and texts[0].splitlines()[1].split("\t")[5:] == ["-9", str(int(want["links"][1]["mode_reads"])), "9", "6", "0", "0", "X", "-"]
    assert texts[1] == ">left_join2\n%s\n>right_rc\n%s\n>other\n%s\n" % (corpus["genome"][:1000], contigs[2], contigs[3])
    texts, _ = command(d, "x60", io, ["--join-overlap-percent", "60"])
    want = pipeline(ctx, NAMES, contigs, corpus["reads"], False, percent=60)
    assert texts == [want["joins"], want["joined"], want["paths_tsv"]] and "".join(want["dec"]) == "JJ"
    assert texts[1] == ">left_join3\n%s\n>other\n%s\n" % (corpus["genome"], contigs[3])           # the overlap is taken from the contig in front


def test_an_ambiguous_end_is_not_joined(ctx, corpus):
    """a fifth contig repeats middle's first 60 letters: the reads that leave `left` enter both, the two links at left's right end are A"""
    d = corpus["dir"]
    rng = np.random.default_rng(77)
    names = NAMES + ["repeat"]
    contigs = list(corpus["contigs"]) + [corpus["contigs"][1][:60] + "".join(rng.choice(list("ACGT"), size=240))]
    write_fasta(d / "repeat.fa", names, contigs)
    texts, _ = command(d, "amb", [str(d / "repeat.fa"), corpus["io"][1]], [])
    want = pipeline(ctx, names, contigs, corpus["reads"], False)
    print(texts[0])
    assert texts == [want["joins"], want["joined"], want["paths_tsv"]]
    at_left = [i for i, k in enumerate(want["links"]) if int(k["a"]) == 0 and not int(k["info"]) & 1]
    assert len(at_left) == 2 and [int(want["links"][i]["b"]) for i in at_left] == [1, 4] and all(want["dec"][i] == "A" for i in at_left)
    assert ">left\n" in texts[1] and ">repeat\n" in texts[1] and ">middle_join2\n" in texts[1] and "left" not in texts[2]


def test_an_empty_contig_file(corpus):
    d = corpus["dir"]
    open(d / "empty.fa", "w").close()
    r = run(EXE, ["contig_join", str(d / "empty.fa"), corpus["io"][1], str(d / "e.tsv"), "--joined", str(d / "e.fa"), "--paths", str(d / "e_paths.tsv")])
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(d / "e.tsv").read() == "" and open(d / "e.fa").read() == "" and open(d / "e_paths.tsv").read() == ""


def test_two_contigs_of_one_name_end_the_command(corpus):
    d = corpus["dir"]
    write_fasta(d / "twice.fa", ["left", "middle", "left", "other"], corpus["contigs"])
    r = run(EXE, ["contig_join", str(d / "twice.fa"), corpus["io"][1], str(d / "t.tsv"), "--joined", str(d / "t.fa")])
    assert r.returncode == 1 and r.stderr.endswith("contig_join: two contigs are named left; a join can not tell them apart\n")
    assert not os.path.exists(d / "t.tsv") and not os.path.exists(d / "t.fa")
