"""Device time of cdm_pileup_links and cdm_pileup_junctions (their kernel_ms) on two sets, written to profiles/contig_join.txt:

    python scripts/profile_contig_join.py [out.txt] [junctions:reads ...]        (default: 10000:50)

The first set is the corpus of tests/test_gpu_contig_join_cli.py (a genome of 1600 letters in three contigs and a fourth contig, 754 reads)
through kmermatcher and rescorediagonal, as the command runs it.  The sets of scripts/profile_contig_dedup.py hold one contig and so no
link; the larger set here has their size and read length with the contigs in a chain: `junctions` + 1 contigs of 500 letters, every
junction bridged by `reads` reads of 100 letters (a read of its own each, drawn from 64 letter sequences), gaps of 0 to 6 letters and,
for every fourth junction, an overlap of 9.  Each figure is the median and the range of 20 calls after 3 warm-up calls.  No speed is
claimed: the calls are new."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from carpedeam_amd import capi  # noqa: E402
from profile_contig_dedup import timed  # noqa: E402

LINES = []


def say(text):
    print(text)
    LINES.append(text)


def chain(junctions, reads, seed=23):
    """-> (seqs, off, rec): contig i's right end and contig i + 1's left end under `reads` reads with 40 columns on the first"""
    rng = np.random.default_rng(seed)
    nc, cl, rl, left = junctions + 1, 500, 100, 40
    letters = ["".join(rng.choice(list("ACGT"), size=rl)) for _ in range(64)]
    seqs = ["".join(rng.choice(list("ACGT"), size=cl)) for _ in range(nc)] + [letters[i % 64] for i in range(junctions * reads)]
    gap = np.where(np.arange(junctions) % 4 == 3, -9, np.arange(junctions) % 7)
    rec = np.zeros(nc + 2 * junctions * reads, capi.ALN_DTYPE)
    off = np.zeros(len(seqs) + 1, np.uint64)
    at = 0
    for q in range(nc):
        off[q] = at
        rec[at] = (q, 0, 0, 0, cl - 1, 0, cl - 1, 1.0)
        at += 1
        if q:               # head records of junction q - 1: the read's last rl - left - gap letters on the contig's first
            t = nc + (q - 1) * reads + np.arange(reads)
            cols = rl - left - int(gap[q - 1])
            r = rec[at:at + reads]
            r["target"], r["q_start"], r["q_end"], r["db_start"], r["db_end"], r["seq_id"] = t, 0, cols - 1, rl - cols, rl - 1, 1.0
            at += reads
        if q < junctions:   # tail records of junction q: the read's first `left` letters on the contig's last
            t = nc + q * reads + np.arange(reads)
            r = rec[at:at + reads]
            r["target"], r["q_start"], r["q_end"], r["db_start"], r["db_end"], r["seq_id"] = t, cl - left, cl - 1, 0, left - 1, 1.0
            at += reads
    off[nc:] = at
    assert at == len(rec)
    return seqs, off, rec, nc


def measure(ctx, what, db, alns, queries, par):
    (stats, totals, links), med, lo, hi = timed(lambda: ctx.pileup_links(db, alns, queries, par, links=True), lambda: ctx.links_kernel_ms)
    say("  %-24s median %.3f ms (min %.3f, max %.3f)  end records %d pairs %d links %d" % ("cdm_pileup_links", med, lo, hi, int(totals[0]), int(totals[3]), len(links)))
    j = np.empty(len(links), capi.JUNCTION_DTYPE)
    for f in ("a", "b", "info"):
        j[f] = links[f]
    j["gap"] = links["gap_mode"]
    (res, letters), med, lo, hi = timed(lambda: ctx.pileup_junctions(db, alns, queries, j, par), lambda: ctx.junctions_kernel_ms)
    say("  %-24s median %.3f ms (min %.3f, max %.3f)  junctions %d voters %d fill letters %d overlap columns %d" % (
        "cdm_pileup_junctions", med, lo, hi, len(j), int(res["voters"].sum()), len(letters), int(res["columns"].sum())))


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "contig_join.txt")
    pairs = [tuple(int(x) for x in a.split(":")) for a in (sys.argv[2:] or ["10000:50"])]
    ctx = capi.Ctx(0)
    say("contig_join (csrc/pileup_links.hip, csrc/pileup_junctions.hip): the kernels' device time on one MI355X")
    say("=" * 98)
    say("")
    say("One execution of scripts/profile_contig_join.py with %s.  The figures are the calls' own kernel_ms (HIP events around the" % " ".join("%d:%d" % p for p in pairs))
    say("stretches of kernels; the radix sorts synchronise the stream inside their stretch, so their host gaps are in the figure; uploads,")
    say("memsets and the copies back are outside).  Per line 20 calls after 3 warm-up calls: median (min, max).  No speed is claimed and no")
    say("threshold is set: cdm_pileup_junctions is new, and cdm_pileup_links was never measured before.  Both calls run the end-record stage")
    say("(count, emit, sort by read), so the second figure holds that stage again.")
    from test_gpu_contig_breaks_cli import createdb_order
    from test_gpu_contig_links_cli import build_corpus
    c = build_corpus()
    laid = [c["reads"][i] for i in createdb_order(len(c["reads"]))]
    both = ctx.concat(ctx.upload_seqs(c["contigs"]), ctx.upload_seqs(laid), 1, 0)
    rp = capi.RescoreParams.default()
    rp.seq_id_thr = 0.9
    alns = ctx.rescore(both, ctx.kmermatch(both, capi.KmerParams.reads_default()), rp)
    say("")
    say("the command's test corpus: 4 contigs, %d reads of 100 letters, %d records" % (len(laid), alns.count))
    measure(ctx, "corpus", both, alns, [0, 1, 2, 3], capi.LinksParams.default(skip_extended_targets=True))
    for junctions, reads in pairs:
        seqs, off, rec, nc = chain(junctions, reads)
        db = ctx.upload_seqs(seqs, ext=[1] * nc + [0] * (len(seqs) - nc))
        alns = ctx.upload_alns(db, off, rec)
        say("")
        say("a chain of %d contigs of 500 letters, %d reads of 100 letters across every junction, %d records" % (nc, reads, len(rec)))
        measure(ctx, "chain", db, alns, list(range(nc)), capi.LinksParams.default(skip_extended_targets=True))
    say("")
    say("Not measured: the share of each kernel inside kernel_ms (no profiler run was made), batches other than the default, the bound of")
    say("2^26 fill letters a call (reasoned from the 20 bytes of counters a letter takes) and the host side of `carpedeam contig_join`;")
    say("its --join-overlap-percent 90 is reasoned as well.")
    with open(path, "w") as f:
        f.write("\n".join(LINES) + "\n")
