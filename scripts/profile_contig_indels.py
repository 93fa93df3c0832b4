"""Device time of cdm_pileup_indels (its kernel_ms: the marks of both record kinds, the count pass and the scan of the cells; the emit
pass, the radix sort of the event keys, the head flags and their scans; the place pass; and, where the caller takes sites, the two
placing scans, the compaction and the letter vote) on three shapes, written to profiles/contig_indels.txt:

    python scripts/profile_contig_indels.py [out.txt]

1. the planted corpus of tests/test_gpu_contig_indels_cli.py through the command's library calls;
2. one deep query: a contig of 100 000 letters under 100 000 ungapped records of 100 letters and 20 000 hand-built gapped records that
   put 40 events each on 500 places, half of them insertions of 1..3 letters, half deletions;
3. 200 000 synth reads of 100 letters (cdm_seqdb_synth), every fiftieth rewritten as a copy of its neighbour with an indel, through
   cdm_kmermatch, cdm_rescore and cdm_pileup_gapped; every read with two hits or more as a query.
Each figure is the median and the range of 20 calls after 3 warm-up calls.  No speed is claimed: the call is new."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from carpedeam_amd import capi  # noqa: E402
from pileup_model import csr, unorient  # noqa: E402
from profile_contig_gapped import with_indel  # noqa: E402

LINES = []


def say(text):
    print(text)
    LINES.append(text)


def timed(ctx, db, alns, queries, grecs, gops, what, **kw):
    ms = []
    par = capi.IndelParams.default(3, 2, 20, 0.0, True)
    for i in range(23):
        out = ctx.pileup_indels(db, alns, queries, grecs, gops, par, **kw)
        if i >= 3:
            ms.append(ctx.indels_kernel_ms)
    stats = out[0] if isinstance(out, tuple) else out
    say("  %-40s median %.3f ms (min %.3f, max %.3f)  rescued %d events %d places %d supported %d major %d" % (
        what, float(np.median(ms)), min(ms), max(ms), int(stats[:, 2].sum()), int(stats[:, 3:5].sum()), int(stats[:, 7].sum()), int(stats[:, 8].sum()), int(stats[:, 9].sum())))


def three_forms(ctx, db, alns, queries, grecs, gops):
    timed(ctx, db, alns, queries, grecs, gops, "statistics alone")
    timed(ctx, db, alns, queries, grecs, gops, "statistics and the cross track", track=True)
    timed(ctx, db, alns, queries, grecs, gops, "statistics, sites and letters", sites=True)


def cli_corpus(ctx):
    import test_gpu_contig_breaks_cli as t
    from test_gpu_contig_indels_cli import planted_corpus
    c = planted_corpus()
    reads = [c["reads"][i] for i in t.createdb_order(len(c["reads"]))]
    both = ctx.concat(ctx.upload_seqs(c["contigs"]), ctx.upload_seqs(reads), 1, 0)
    hits = ctx.kmermatch(both, capi.KmerParams.reads_default())
    alns = ctx.rescore(both, hits, capi.RescoreParams.default())
    _, grecs, gops, _ = ctx.pileup_gapped(both, hits, alns, [0, 1], capi.GapParams.default(0.0, True), records=True)
    say("1. the CLI test corpus: contigs of 697 and 320 letters, %d reads of 80 letters, %d records in the set, %d gapped records" % (len(reads), alns.count, len(grecs)))
    three_forms(ctx, both, alns, [0, 1], grecs, gops)


def deep(ctx):
    rng = np.random.default_rng(7)
    n, length, rl, places, per = 100_000, 100_000, 100, 500, 40
    contig = "".join(rng.choice(list("ACGT"), size=length))
    seqs, recs = [contig], [(0, 0, 0, 0, length - 1, 0, length - 1, 1.0)]
    starts = rng.integers(0, length - rl, size=n)
    for i in range(n):
        at = int(starts[i])
        seqs.append(contig[at:at + rl])
        recs.append(unorient(1 + i, at, at + rl - 1, 0, rl - 1, False, rl))
    grecs, gops = np.zeros(places * per, capi.GAP_DTYPE), []
    for j in range(places):
        p, g, op = 150 + j * 190, 1 + j % 3, 1 + j % 2
        for k in range(per):
            read = contig[p - 30:p] + ("ACG"[:g] if op == 1 else "") + contig[p + (g if op == 2 else 0):p + (g if op == 2 else 0) + 30]
            seqs.append(read)
            r = grecs[j * per + k]
            r["target"], r["pos"], r["span"], r["tlen"], r["columns"], r["n_ops"], r["ops"] = len(seqs) - 1, p - 30, 60 + (g if op == 2 else 0), len(read), len(read), 3, len(gops)
            gops += [30 << 2, g << 2 | op, 30 << 2]
    off, rec = csr(len(seqs), {0: recs})
    db = ctx.upload_seqs(seqs, ext=[1] + [0] * (len(seqs) - 1))
    alns = ctx.upload_alns(db, off, rec)
    say("2. one contig of %d letters under %d ungapped records of %d letters and %d gapped records on %d places" % (length, n, rl, len(grecs), places))
    three_forms(ctx, db, alns, [0], grecs, np.array(gops, np.uint32))


def synth_reads(ctx):
    n = 200_000
    seqs = [s.decode() for s in ctx.synth(n, 100, 100, 11).download()[0]]
    rng = np.random.default_rng(13)
    for i in range(0, n - 1, 50):       # a copy of the next read, shifted, with an indel: it seeds there and fails the ungapped test
        src = seqs[i + 1] + "".join(rng.choice(list("ACGT"), size=8))
        seqs[i] = with_indel(rng, src[2:], 100)
    db = ctx.upload_seqs(seqs)
    hits = ctx.kmermatch(db)
    alns = ctx.rescore(db, hits)
    hoff, _ = hits.download()
    queries = np.flatnonzero(np.diff(hoff.astype(np.int64)) >= 2).astype(np.uint32)
    _, grecs, gops, _ = ctx.pileup_gapped(db, hits, alns, queries, capi.GapParams.default(0.0, False), records=True)
    say("3. %d synth reads of 100 letters, %d records in the set, %d queries with two hits or more, %d gapped records" % (n, alns.count, len(queries), len(grecs)))
    three_forms(ctx, db, alns, queries, grecs, gops)


if __name__ == "__main__":
    ctx = capi.Ctx(0)
    say("contig_indels (csrc/pileup_indels.hip, cdm_pileup_indels): the kernels' device time on one MI355X")
    say("=" * 98)
    say("")
    say("One execution of scripts/profile_contig_indels.py.  The figures are the call's own kernel_ms (HIP events around the stretches of")
    say("kernels of every batch; the radix sort synchronises the stream inside its stretch, so its host gaps are in the figure; the upload")
    say("of the records, the memsets and the copies back are outside).  Per line 20 calls after 3 warm-up calls: median (min, max).  No")
    say("speed is claimed and no threshold is set: the call is new, there is no figure of the parent commit and none of the reference.")
    say("min_depth 3, min_count 2, min_percent 20.")
    say("")
    cli_corpus(ctx)
    deep(ctx)
    synth_reads(ctx)
    say("")
    say("Not measured: the host's check of the records, their upload, the share of each kernel inside kernel_ms (no profiler run was made)")
    say("and the host side of `carpedeam contig_indels` (the tables and the FASTA).")
    say("")
    say("Compile-time resources (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage):")
    say("    k_indel_marks 27 VGPRs    k_indel_count 25    k_indel_emit 20    k_indel_track 7    k_indel_heads 6    k_indel_starts 6")
    say("    k_indel_places 32    k_indel_sites 18    k_indel_letters 26 (and 3968 bytes of LDS a block)    8 waves/SIMD")
    say("    all: scratch 0 bytes/lane, no SGPR / VGPR spills")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "contig_indels.txt")
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
