"""`--dedup 1` on the five contig_* commands that take it, and `carpedeam contig_dedup`, on the device: every file against the text the
existing model writers give for the set tests/dedup_model.py leaves of the records the same library calls give - compared as text.  The
corpus is the one of tests/test_gpu_contig_breaks_cli.py with planted copies; what the plants must do is asserted on the downloaded set."""
import os
import re
import subprocess

import numpy as np
import pytest

import bases_model
import breaks_model
import dedup_model as dm
import depth_model
import map_model
import pileup_model
from carpedeam_amd import capi
from pileup_model import orient
from stageflags import K_FLAGS, R_FLAGS
from test_gpu_contig_breaks_cli import COMP, NAMES, build_corpus, createdb_order, write_fasta, write_fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT = os.path.join(ROOT, "carpedeam_amd", "carpedeam")
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
BREAKS = dict(anchor=16, edge=50, min_span=1, min_span_percent=0)


@pytest.fixture(scope="module", autouse=True)
def built():
    from carpedeam_amd import build
    build.build()


def run(exe, args, **env):
    e = {k: v for k, v in os.environ.items() if k != "CARPEDEAM_REF_BIN"}
    e.update(env)
    return subprocess.run([exe] + args, capture_output=True, text=True, env=e, timeout=300)


def planted_corpus():
    """build_corpus() and 20 reads that overhang a contig end by 5..15 letters; 60 of these reads - the 20 among them - get 1 to 3 extra
    copies each: exact, with one substitution outside the first 20 letters, or (at most one per read) the reverse complement.
    plants: (index of the copy, index of its source, kind)"""
    c = build_corpus()
    rng = np.random.default_rng(4711)
    reads = list(c["reads"])
    first_overhang = len(reads)
    for i in range(20):
        contig = c["contigs"][i % 2]            # (ctg3 is written with letters the reads do not carry)
        n, over = int(rng.integers(40, 81)), int(rng.integers(5, 16))
        beyond = "".join(rng.choice(list("ACGT"), size=over))
        r = beyond + contig[:n - over] if i % 4 < 2 else contig[400 - (n - over):] + beyond
        reads.append(r.translate(COMP)[::-1] if i % 3 == 0 else r)
    sources = [int(x) for x in rng.choice(first_overhang, size=40, replace=False)] + list(range(first_overhang, first_overhang + 20))
    plants = []
    for k, s in enumerate(sources):
        kinds = [("exact", "subst", "rc")[(k + j) % 3] for j in range(1 + k % 3)]
        for kind in kinds:
            r = reads[s]
            if kind == "subst":
                at = int(rng.integers(20, len(r)))
                r = r[:at] + "ACGT"[("ACGT".index(r[at]) + 1 + int(rng.integers(0, 3))) % 4] + r[at + 1:]
            elif kind == "rc":
                r = r.translate(COMP)[::-1]
            plants.append((len(reads), s, kind))
            reads.append(r)
    c["reads"], c["plants"], c["overhang"] = reads, plants, range(first_overhang, first_overhang + 20)
    return c


def pipeline(ctx, contigs, reads, k=20, min_seq_id=0.9):
    """the steps of a --dedup 1 command through the Python binding: the joint DB in createdb's read order, kmermatcher, rescorediagonal,
    cdm_alns_dedup over the contigs - held against the model here, once -> what the model writers need, before and after"""
    assert K_FLAGS[-2:] == ["-k", "20"] and "--min-seq-id 0.9" in " ".join(R_FLAGS)
    order = createdb_order(len(reads))
    laid = [reads[i] for i in order]
    nc = len(contigs)
    both = ctx.concat(ctx.upload_seqs(contigs), ctx.upload_seqs(laid), 1, 0)
    kp = capi.KmerParams.reads_default()
    kp.kmer_size = k
    rp = capi.RescoreParams.default()
    rp.seq_id_thr = min_seq_id
    alns = ctx.rescore(both, ctx.kmermatch(both, kp), rp)
    off, rec = alns.download()
    queries, seqs, ext = list(range(nc)), contigs + laid, [1] * nc + [0] * len(laid)
    d_off, d_rec, keep, stats = dm.dedup(seqs, ext, off, rec, queries, 0.0, True)
    out, got_stats, got_keep = ctx.alns_dedup(both, alns, queries, 0.0, True, keep=True)
    got_off, got_rec = out.download()
    assert np.array_equal(got_stats, stats) and np.array_equal(got_keep, keep) and np.array_equal(got_off, d_off) and got_rec.tobytes() == d_rec.tobytes()
    return dict(seqs=seqs, ext=ext, order=order, queries=queries, off=off, rec=rec, d_off=d_off, d_rec=d_rec, keep=keep, stats=stats, nc=nc, laid=laid)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    c = planted_corpus()
    c["dir"] = d = tmp_path_factory.mktemp("contig_dedup")
    write_fasta(d / "contigs.fa", NAMES, c["contigs"])
    write_fastq(d / "reads.fq", c["reads"])
    c["second"] = c["reads"][100:300] + c["reads"][120:180]         # a second library with copies of its own
    write_fastq(d / "second.fq", c["second"])
    ctx = capi.Ctx(0)
    c["p"] = pipeline(ctx, c["contigs"], c["reads"])
    c["p2"] = pipeline(ctx, c["contigs"], c["second"])
    c["lengths"] = [len(s) for s in c["contigs"]]
    c["io"] = [str(d / "contigs.fa"), str(d / "reads.fq")]
    return c


def args_of(p, dedup):
    return (p["seqs"], p["ext"], p["d_off"] if dedup else p["off"], p["d_rec"] if dedup else p["rec"], p["queries"])


def removed_columns(p):
    """per contig, the columns of the records the model removed"""
    out = [0] * p["nc"]
    for q in range(p["nc"]):
        for r in range(int(p["off"][q]), int(p["off"][q + 1])):
            if not p["keep"][r]:
                out[q] += abs(int(p["rec"][r]["q_end"]) - int(p["rec"][r]["q_start"])) + 1
    return out


def test_the_plants_do_what_they_are_planted_for(corpus):
    """on the downloaded set: every family of a source and its same-strand copies loses all but one of its records, the reverse-complement
    copies lose none, and the overhanging reads are among both"""
    p, plants = corpus["p"], corpus["plants"]
    assert len({s for _, s, _ in plants}) == 60 and len(plants) == 120 and {k for _, _, k in plants} == {"exact", "subst", "rc"}
    assert sum(1 for s in {s for _, s, _ in plants} if s in corpus["overhang"]) == 20
    where = {}            # original read index -> [(record, contig)]
    for q in range(p["nc"]):
        for r in range(int(p["off"][q]), int(p["off"][q + 1])):
            t = int(p["rec"][r]["target"])
            if t >= p["nc"]:
                where.setdefault(p["order"][t - p["nc"]], []).append((r, q))
    family = {}
    for i, s, kind in plants:
        if kind != "rc":
            family.setdefault(s, [s]).append(i)
    seeded = removed = overhanging = clipped = 0
    for s, members in family.items():
        records = [r for i in members for r, _ in where.get(i, [])]
        plants_seeded = sum(1 for i in members[1:] if i in where)
        gone = sum(1 for r in records if not p["keep"][r])
        assert gone >= len(records) - 1 and (s not in where or gone >= plants_seeded), (s, members, records)
        seeded += plants_seeded; removed += gone
        if s in corpus["overhang"] and gone:
            overhanging += 1
            r = p["rec"][records[0]]
            qs, qe, ds, de, _ = orient(r, len(p["seqs"][int(r["target"])]))
            clipped += ds > 0 or de < len(p["seqs"][int(r["target"])]) - 1
    assert seeded >= 60 and removed >= 60 and overhanging >= 8 and clipped >= 8, (seeded, removed, overhanging, clipped)
    rc = [r for i, _, kind in plants if kind == "rc" for r, _ in where.get(i, [])]
    assert len(rc) >= 20 and all(p["keep"][r] for r in rc)
    assert int(p["stats"][:, 2].sum()) >= removed and corpus["p2"]["stats"][:, 2].sum() >= 40


def test_contig_dedup_table(corpus):
    d, p = corpus["dir"], corpus["p"]
    log, out = str(d / "dispatch.log"), str(d / "dedup.tsv")
    r = run(FRONT, ["contig_dedup"] + corpus["io"] + [out, "--threads", "4"], CARPEDEAM_DISPATCH_LOG=log, CDM_TIMING="1")
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(log).read() == "gpu contig_dedup\n"
    assert open(out).read() == dm.table(NAMES, [0, 1, 2], corpus["lengths"], p["off"], p["stats"])
    m = re.search(r"duplicate reads: (\d+) records, (\d+) removed, dedup kernels [0-9.]+ ms", r.stderr)
    assert m and int(m.group(1)) == len(p["rec"]) and int(m.group(2)) == int(p["stats"][:, 2].sum())
    open(d / "empty.fa", "w").close()
    r = run(EXE, ["contig_dedup", str(d / "empty.fa"), corpus["io"][1], str(d / "empty.tsv")])
    assert r.returncode == 0 and open(d / "empty.tsv").read() == dm.HEADER


def test_contig_damage(corpus):
    d, p = corpus["dir"], corpus["p"]
    for flags, dedup, name in ((["--dedup", "1"], True, "damage1.tsv"), (["--dedup", "0"], False, "damage0.tsv"), ([], False, "damage.tsv")):
        r = run(EXE, ["contig_damage"] + corpus["io"] + [str(d / name)] + flags)
        assert r.returncode == 0, r.stderr[-1500:]
        counts, reads, columns = pileup_model.profile(*args_of(p, dedup), 16, 0.0, True)
        assert open(d / name).read() == pileup_model.tsv(NAMES, [0, 1, 2], corpus["lengths"], counts, reads, columns), name
    assert open(d / "damage0.tsv").read() == open(d / "damage.tsv").read() != open(d / "damage1.tsv").read()


def test_contig_depth_of_two_read_sets_and_the_track(corpus):
    d, p, p2 = corpus["dir"], corpus["p"], corpus["p2"]
    two = [corpus["io"][0], corpus["io"][1], str(d / "second.fq")]
    texts = {}
    for flags, dedup, name in ((["--dedup", "1"], True, "depth1.tsv"), (["--dedup", "0"], False, "depth0.tsv"), ([], False, "depth.tsv")):
        r = run(EXE, ["contig_depth"] + two + [str(d / name)] + flags)
        assert r.returncode == 0, r.stderr[-1500:]
        samples = [depth_model.depth_stats(*args_of(x, dedup), 0, 0.0, True)[0] for x in (p, p2)]
        texts[name] = open(d / name).read()
        assert texts[name] == depth_model.tsv(NAMES, [0, 1, 2], corpus["lengths"], samples), name
    assert texts["depth0.tsv"] == texts["depth.tsv"] != texts["depth1.tsv"]
    # the depth sum of either read set falls by exactly the columns of the removed records
    rows0, rows1 = ([l.split("\t") for l in texts[n].split("\n")[1:] if l] for n in ("depth0.tsv", "depth1.tsv"))
    header = texts["depth.tsv"].split("\n")[0].split("\t")
    for s, x in ((1, p), (2, p2)):
        col = header.index("sum_%d" % s)
        fall = [int(a[col]) - int(b[col]) for a, b in zip(rows0, rows1)]
        assert fall == removed_columns(x) and sum(fall) > 0
    r = run(EXE, ["contig_depth"] + corpus["io"] + [str(d / "depth_t.tsv"), "--depth-track", str(d / "depth.bedgraph"), "--dedup", "1", "--depth-edge", "30"])
    assert r.returncode == 0, r.stderr[-1500:]
    stats, tracks = depth_model.depth_stats(*args_of(p, True), 30, 0.0, True)
    assert open(d / "depth_t.tsv").read() == depth_model.tsv(NAMES, [0, 1, 2], corpus["lengths"], [stats])
    assert open(d / "depth.bedgraph").read() == depth_model.bedgraph(NAMES, tracks)


def test_contig_variants(corpus):
    d, p = corpus["dir"], corpus["p"]
    for flags, dedup, tag in ((["--dedup", "1"], True, "v1"), (["--dedup", "0"], False, "v0"), ([], False, "v")):
        files = [str(d / (tag + x)) for x in (".tsv", "_sites.tsv", "_cons.fa")]
        r = run(EXE, ["contig_variants"] + corpus["io"] + [files[0], "--sites", files[1], "--consensus", files[2]] + flags)
        assert r.returncode == 0, r.stderr[-1500:]
        stats, _, sites = bases_model.bases(*args_of(p, dedup), min_seq_id=0.0, skip=True, **bases_model.DEFAULTS)
        assert open(files[0]).read() == bases_model.summary_tsv(NAMES, [0, 1, 2], corpus["lengths"], stats), tag
        assert open(files[1]).read() == bases_model.sites_tsv(NAMES, sites), tag
        assert open(files[2]).read() == bases_model.consensus_fasta(NAMES, corpus["contigs"], sites), tag
    for x in (".tsv", "_sites.tsv", "_cons.fa"):
        assert open(d / ("v0" + x)).read() == open(d / ("v" + x)).read()
    assert open(d / "v0.tsv").read() != open(d / "v1.tsv").read()


def test_contig_breaks(corpus):
    d, p = corpus["dir"], corpus["p"]
    for flags, dedup, tag in ((["--dedup", "1"], True, "b1"), (["--dedup", "0"], False, "b0"), ([], False, "b")):
        files = [str(d / (tag + x)) for x in (".tsv", "_split.fa", ".bedgraph")]
        r = run(EXE, ["contig_breaks"] + corpus["io"] + [files[0], "--split", files[1], "--span-track", files[2]] + flags)
        assert r.returncode == 0, r.stderr[-1500:]
        stats, tracks, breaks = breaks_model.breaks_stats(*args_of(p, dedup), BREAKS["anchor"], BREAKS["edge"], BREAKS["min_span"], BREAKS["min_span_percent"], 0.0, True)
        assert open(files[0]).read() == breaks_model.tsv(NAMES, [0, 1, 2], corpus["lengths"], stats, breaks), tag
        assert open(files[1]).read() == breaks_model.split(NAMES, corpus["contigs"], breaks), tag
        assert open(files[2]).read() == breaks_model.bedgraph(NAMES, tracks), tag
    for x in (".tsv", "_split.fa", ".bedgraph"):
        assert open(d / ("b0" + x)).read() == open(d / ("b" + x)).read()
    assert open(d / "b0.bedgraph").read() != open(d / "b1.bedgraph").read()


def sam_keys(text):
    """(RNAME, strand, unclipped start, read length) of every record line"""
    out = []
    for l in text.split("\n"):
        if l and not l.startswith("@"):
            f = l.split("\t")
            clip = re.match(r"^(\d+)S", f[5])
            out.append((f[2], int(f[1]) & 16, int(f[3]) - (int(clip.group(1)) if clip else 0), len(f[9])))
    return out


def test_contig_map(corpus):
    d, p = corpus["dir"], corpus["p"]
    nc, order, laid = p["nc"], p["order"], p["laid"]
    texts = {}
    for flags, dedup, name in ((["--dedup", "1"], True, "map1.sam"), (["--dedup", "0"], False, "map0.sam"), ([], False, "map.sam"), (["--dedup", "1", "--primary-only", "1"], True, "map1p.sam")):
        r = run(EXE, ["contig_map"] + corpus["io"] + [str(d / name), "--threads", "4"] + flags)
        assert r.returncode == 0, r.stderr[-1500:]
        _, recs, mism = map_model.map_records(*args_of(p, dedup), 0.0, True)
        texts[name] = open(d / name).read()
        assert texts[name] == map_model.sam_text(NAMES, corpus["lengths"], lambda t: "r%d" % order[t - nc], lambda t: laid[t - nc], recs, mism, primary_only="--primary-only" in flags), name
    assert texts["map0.sam"] == texts["map.sam"]
    with_copies, without = sam_keys(texts["map.sam"]), sam_keys(texts["map1.sam"])
    assert len(set(without)) == len(without) == len(with_copies) - int(p["stats"][:, 2].sum()) and len(set(with_copies)) < len(with_copies)
    assert map_model.sam_check(texts["map1.sam"], dict(zip(NAMES, corpus["contigs"]))) > 0        # (one primary line per read that is left)
