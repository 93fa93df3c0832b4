"""Device time of cdm_pileup_breaks (its kernel_ms: the marks in two planes, the prefix sum over them, the classification, the prefix sum
of the run starts and, where a batch has a break, the emission) on three shapes, for profiles/contig_breaks.txt:

    python scripts/profile_contig_breaks.py

1. the corpus of tests/test_gpu_contig_breaks_cli.py (three contigs of 400 letters, 330 reads) through the command's four library calls;
2. the planted join of the same file (two contigs of 1200 letters, 1143 reads of 60 letters);
3. one contig of 100 000 letters under 100 000 records of 100 letters, the alignment set written directly: starts drawn from the whole
   contig, and the same with no read on the letters 40 000..59 999 (one gap of 20 000 boundaries: the emission's shared-run path).
Each figure is the median and the range of 20 calls after 3 warm-up calls.  Beside each shape stands cdm_pileup_depth's time on the same
handles (cdm_ctx_last_kernel_ms(ctx, 17)): the reading aid, not a comparison - the depth call marks one plane and classifies nothing."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from carpedeam_amd import capi  # noqa: E402
from pileup_model import csr, unorient  # noqa: E402


def timed(ctx, db, alns, queries, what, **kw):
    ms = []
    for i in range(23):
        out = ctx.pileup_breaks(db, alns, queries, skip_extended_targets=True, **kw)
        if i >= 3:
            ms.append(ctx.breaks_kernel_ms)
    stats = out[0] if isinstance(out, tuple) else out
    print("  %-46s median %.3f ms (min %.3f, max %.3f)  reads %d columns %d window %d weak %d breaks %d joins %d" % (
        what, float(np.median(ms)), min(ms), max(ms), int(stats[:, 0].sum()), int(stats[:, 1].sum()), int(stats[:, 2].sum()), int(stats[:, 3].sum()), int(stats[:, 4].sum()),
        int(stats[:, 5].sum())))


def depth_timed(ctx, db, alns, queries):
    ms = []
    for i in range(23):
        ctx.pileup_depth(db, alns, queries, edge=50, skip_extended_targets=True)
        if i >= 3:
            ms.append(ctx.last_kernel_ms(17))
    print("  %-46s median %.3f ms (min %.3f, max %.3f)" % ("cdm_pileup_depth on the same handles", float(np.median(ms)), min(ms), max(ms)))


def all_forms(ctx, db, alns, queries, **kw):
    timed(ctx, db, alns, queries, "summary alone", **kw)
    timed(ctx, db, alns, queries, "summary and records", breaks=True, **kw)
    timed(ctx, db, alns, queries, "summary, records and the span track", breaks=True, track=True, **kw)
    depth_timed(ctx, db, alns, queries)


def piled(ctx, contigs, reads, order):
    reads = [reads[i] for i in order(len(reads))]
    both = ctx.concat(ctx.upload_seqs(contigs), ctx.upload_seqs(reads), 1, 0)
    rp = capi.RescoreParams.default()
    rp.seq_id_thr = 0.9
    return both, ctx.rescore(both, ctx.kmermatch(both, capi.KmerParams.reads_default()), rp)


def cli_corpora(ctx):
    import test_gpu_contig_breaks_cli as t
    c = t.build_corpus()
    both, alns = piled(ctx, c["contigs"], c["reads"], t.createdb_order)
    print("1. the CLI test corpus: 3 contigs of 400 letters, %d reads of 40..80 letters, %d records in the set" % (len(c["reads"]), alns.count))
    all_forms(ctx, both, alns, [0, 1, 2])
    timed(ctx, both, alns, [0, 1, 2], "records, anchor 8 edge 10 min_span 4 percent 60", breaks=True, anchor=8, edge=10, min_span=4, min_span_percent=60)
    names, contigs, reads = t.planted_join()
    both, alns = piled(ctx, contigs, reads, t.createdb_order)
    print("2. the planted join: 2 contigs of 1200 letters, %d reads of 60 letters, %d records in the set" % (len(reads), alns.count))
    all_forms(ctx, both, alns, [0, 1])


def deep(ctx, hole):
    rng = np.random.default_rng(7)
    n, length, rl = 100_000, 100_000, 100
    contig = "".join(rng.choice(list("ACGT"), size=length))
    seqs, recs = [contig], [(0, 0, 0, 0, length - 1, 0, length - 1, 1.0)]
    starts = rng.integers(0, length - rl + 1, size=n)
    read = "".join(rng.choice(list("ACGT"), size=rl))        # (the letters play no part in this reduction)
    for i in range(n):
        at = int(starts[i])
        if hole and at + rl > 40_000 and at < 60_000:
            at = at % (40_000 - rl)
        seqs.append(read)
        recs.append(unorient(1 + i, at, at + rl - 1, 0, rl - 1, bool(i & 1), rl))
    off, rec = csr(len(seqs), {0: recs})
    db = ctx.upload_seqs(seqs, ext=[1] + [0] * n)
    alns = ctx.upload_alns(db, off, rec)
    print("3. one contig of %d letters under %d records of %d letters%s" % (length, n, rl, ", none on the letters 40000..59999" if hole else ""))
    all_forms(ctx, db, alns, [0])
    timed(ctx, db, alns, [0], "summary and records, min_span 60 percent 50", breaks=True, min_span=60, min_span_percent=50)
    for chunk in ("64", "256"):         # the one contig's records in more, smaller work items (the default is 1024 records a wave)
        os.environ["CDM_PILEUP_CHUNK"] = chunk
        timed(ctx, db, alns, [0], "summary and records, CDM_PILEUP_CHUNK=" + chunk, breaks=True)
    del os.environ["CDM_PILEUP_CHUNK"]


if __name__ == "__main__":
    ctx = capi.Ctx(0)
    cli_corpora(ctx)
    deep(ctx, False)
    deep(ctx, True)
