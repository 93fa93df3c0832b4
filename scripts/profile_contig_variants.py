"""Device time of cdm_pileup_bases (its kernel_ms: counting, classification, the scan of the marks, emission) on two shapes, for
profiles/contig_variants.txt:

    python scripts/profile_contig_variants.py

1. the corpus of tests/test_gpu_contig_variants_cli.py (three contigs of 400 letters, 300 reads) through the command's four library calls;
2. one contig of 100 000 letters under 100 000 records of 100 letters (reads cut from it on both strands, 1 % of their letters changed),
   the alignment set written directly, and the same records piled on the first 1 000 letters (hot words).
Each figure is the median and the range of 20 calls after 3 warm-up calls.  The second shape is also run with CDM_PILEUP_CHUNK=64 and
256: its 100 000 records are one query's, which the default of 1024 records a work item cuts into 98 waves."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from carpedeam_amd import capi  # noqa: E402
from pileup_model import csr, unorient  # noqa: E402

COMP = str.maketrans("ACGT", "TGCA")


def timed(ctx, db, alns, queries, what, **kw):
    ms = []
    for i in range(23):
        out = ctx.pileup_bases(db, alns, queries, skip_extended_targets=True, **kw)
        if i >= 3:
            ms.append(ctx.bases_kernel_ms)
    stats = out[0] if isinstance(out, tuple) else out
    print("  %-46s median %.3f ms (min %.3f, max %.3f)  reads %d columns %d bases %d flagged %d" % (
        what, float(np.median(ms)), min(ms), max(ms), int(stats[:, 0].sum()), int(stats[:, 1].sum()), int(stats[:, 2].sum()), int(stats[:, 7].sum())))


def cli_corpus(ctx):
    import test_gpu_contig_variants_cli as t
    c = t.build_corpus()
    reads = [c["reads"][i] for i in t.createdb_order(len(c["reads"]))]
    both = ctx.concat(ctx.upload_seqs(c["contigs"]), ctx.upload_seqs(reads), 1, 0)
    rp = capi.RescoreParams.default()
    rp.seq_id_thr = 0.9
    alns = ctx.rescore(both, ctx.kmermatch(both, capi.KmerParams.reads_default()), rp)
    print("1. the CLI test corpus: 3 contigs of 400 letters, 300 reads of 40..80 letters, %d records in the set" % alns.count)
    timed(ctx, both, alns, [0, 1, 2], "summary alone")
    timed(ctx, both, alns, [0, 1, 2], "summary and sites", sites=True)
    timed(ctx, both, alns, [0, 1, 2], "summary, sites and the counts table", sites=True, counts=True)


def deep(ctx, spread):
    rng = np.random.default_rng(7)
    n, length, rl = 100_000, 100_000, 100
    contig = "".join(rng.choice(list("ACGT"), size=length))
    seqs, recs = [contig], [(0, 0, 0, 0, length - 1, 0, length - 1, 1.0)]
    starts = rng.integers(0, spread - rl + 1, size=n)
    for i in range(n):
        at = int(starts[i])
        r = np.array(list(contig[at:at + rl]))
        hit = rng.random(rl) < 0.01
        r[hit] = rng.choice(list("ACGT"), size=int(hit.sum()))
        r = "".join(r)
        rev = bool(i & 1)
        seqs.append(r.translate(COMP)[::-1] if rev else r)
        recs.append(unorient(1 + i, at, at + rl - 1, 0, rl - 1, rev, rl))
    off, rec = csr(len(seqs), {0: recs})
    db = ctx.upload_seqs(seqs, ext=[1] + [0] * n)
    alns = ctx.upload_alns(db, off, rec)
    print("2. one contig of %d letters under %d records of %d letters, starts drawn from the first %d letters" % (length, n, rl, spread))
    timed(ctx, db, alns, [0], "summary alone")
    timed(ctx, db, alns, [0], "summary and sites", sites=True)
    timed(ctx, db, alns, [0], "summary, sites and the counts table", sites=True, counts=True)
    timed(ctx, db, alns, [0], "summary and sites, mask_ends 5", sites=True, mask_ends=5)
    for chunk in ("64", "256"):         # the one contig's records in more, smaller work items (the default is 1024 records a wave)
        os.environ["CDM_PILEUP_CHUNK"] = chunk
        timed(ctx, db, alns, [0], "summary and sites, CDM_PILEUP_CHUNK=" + chunk, sites=True)
    del os.environ["CDM_PILEUP_CHUNK"]


if __name__ == "__main__":
    ctx = capi.Ctx(0)
    cli_corpus(ctx)
    deep(ctx, 100_000)
    deep(ctx, 1_000)
