"""Device time of cdm_pileup_map (its kernel_ms: the primary pass, the count with its two scans and, where a batch has records, the
emission, the sort, the scan of the sorted counts and the gather) on three shapes, for profiles/contig_map.txt:

    python scripts/profile_contig_map.py

1. the corpus of tests/test_gpu_contig_map_cli.py (three contigs of 400 letters, 330 reads) through the command's four library calls;
2. one deep query: a contig of 100 000 letters under 100 000 records of 100 letters, the alignment set written directly, the reads cut
   from the contig on both strands with 2 % of their letters changed;
3. 200 000 synth reads of 100 letters (cdm_seqdb_synth) through cdm_kmermatch and cdm_rescore, every read with two records or more as a
   query: many short queries, reads on several of them.
Each figure is the median and the range of 20 calls after 3 warm-up calls.  Beside each shape stands cdm_pileup_depth's time on the same
handles (cdm_ctx_last_kernel_ms(ctx, 17)): for scale, not a comparison - the depth call reads no letters and sorts nothing."""
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
        out = ctx.pileup_map(db, alns, queries, skip_extended_targets=True, **kw)
        if i >= 3:
            ms.append(ctx.map_kernel_ms)
    stats = out[0] if isinstance(out, tuple) else out
    print("  %-46s median %.3f ms (min %.3f, max %.3f)  reads %d columns %d mismatches %d primary %d" % (
        what, float(np.median(ms)), min(ms), max(ms), int(stats[:, 0].sum()), int(stats[:, 1].sum()), int(stats[:, 2].sum()), int(stats[:, 3].sum())))


def depth_timed(ctx, db, alns, queries):
    ms = []
    for i in range(23):
        ctx.pileup_depth(db, alns, queries, edge=0, skip_extended_targets=True)
        if i >= 3:
            ms.append(ctx.last_kernel_ms(17))
    print("  %-46s median %.3f ms (min %.3f, max %.3f)" % ("cdm_pileup_depth on the same handles", float(np.median(ms)), min(ms), max(ms)))


def both_forms(ctx, db, alns, queries):
    timed(ctx, db, alns, queries, "statistics alone")
    timed(ctx, db, alns, queries, "statistics, records and mismatch words", records=True)
    depth_timed(ctx, db, alns, queries)


def cli_corpus(ctx):
    import test_gpu_contig_breaks_cli as t
    c = t.build_corpus()
    reads = [c["reads"][i] for i in t.createdb_order(len(c["reads"]))]
    both = ctx.concat(ctx.upload_seqs(c["contigs"]), ctx.upload_seqs(reads), 1, 0)
    alns = ctx.rescore(both, ctx.kmermatch(both, capi.KmerParams.reads_default()), capi.RescoreParams.default())
    print("1. the CLI test corpus: 3 contigs of 400 letters, %d reads of 40..80 letters, %d records in the set" % (len(reads), alns.count))
    both_forms(ctx, both, alns, [0, 1, 2])


def deep(ctx):
    rng = np.random.default_rng(7)
    n, length, rl = 100_000, 100_000, 100
    contig = "".join(rng.choice(list("ACGT"), size=length))
    seqs, recs = [contig], [(0, 0, 0, 0, length - 1, 0, length - 1, 1.0)]
    starts = rng.integers(0, length - rl + 1, size=n)
    for i in range(n):
        at = int(starts[i])
        r = list(contig[at:at + rl])
        for j in rng.integers(0, rl, size=2):
            r[j] = "ACGT"[("ACGT".index(r[j]) + 1) % 4]
        r = "".join(r)
        seqs.append(r.translate(COMP)[::-1] if i & 1 else r)
        recs.append(unorient(1 + i, at, at + rl - 1, 0, rl - 1, bool(i & 1), rl))
    off, rec = csr(len(seqs), {0: recs})
    db = ctx.upload_seqs(seqs, ext=[1] + [0] * n)
    alns = ctx.upload_alns(db, off, rec)
    print("2. one contig of %d letters under %d records of %d letters" % (length, n, rl))
    both_forms(ctx, db, alns, [0])
    for chunk in ("64", "256"):         # the one contig's records in more, smaller work items (the default is 1024 records a wave)
        os.environ["CDM_PILEUP_CHUNK"] = chunk
        timed(ctx, db, alns, [0], "records and words, CDM_PILEUP_CHUNK=" + chunk, records=True)
    del os.environ["CDM_PILEUP_CHUNK"]


def synth_reads(ctx):
    n = 200_000
    db = ctx.synth(n, 100, 100, 11)
    alns = ctx.rescore(db, ctx.kmermatch(db))
    off, _ = alns.download()
    queries = np.flatnonzero(np.diff(off.astype(np.int64)) >= 2).astype(np.uint32)
    print("3. %d synth reads of 100 letters, %d records in the set, %d queries with two records or more" % (n, alns.count, len(queries)))
    both_forms(ctx, db, alns, queries)


if __name__ == "__main__":
    ctx = capi.Ctx(0)
    cli_corpus(ctx)
    deep(ctx)
    synth_reads(ctx)
