"""Device time of cdm_pileup_gapped (its kernel_ms: the marking of the counted records and the sort of their keys, the two candidate
passes, the count pass of the alignment with its three scans and, where the caller takes records, the emission pass, the sort and the
gather) on the three shapes of scripts/profile_contig_map.py, each with about 2 % of the reads carrying one inserted or deleted
stretch of 1..3 letters, for profiles/contig_gapped.txt:

    python scripts/profile_contig_gapped.py

1. the corpus of tests/test_gpu_contig_map_cli.py (330 reads, 7 of them rewritten with an indel) through the command's library calls;
2. one deep query: a contig of 100 000 letters under 100 000 reads of 100 letters, hits and alignment set written directly: the reads
   with an indel have a hit and no record;
3. 200 000 synth reads of 100 letters (cdm_seqdb_synth), every fiftieth rewritten as a copy of its neighbour with an indel, through
   cdm_kmermatch and cdm_rescore; every read with two hits or more as a query.
Each figure is the median and the range of 20 calls after 3 warm-up calls.  Beside each shape stands cdm_pileup_map's time on the same
handles, with records: for scale, not a comparison - the map call aligns nothing."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from carpedeam_amd import capi  # noqa: E402
from pileup_model import csr, unorient  # noqa: E402

COMP = str.maketrans("ACGT", "TGCA")


def with_indel(rng, letters, n):
    """n letters from `letters` (n + 3 at the least) with one inserted or deleted stretch of 1..3 letters away from the ends"""
    g, p = int(rng.integers(1, 4)), int(rng.integers(25, n - 25))
    if rng.integers(0, 2):
        return (letters[:p] + "".join(rng.choice(list("ACGT"), size=g)) + letters[p:])[:n]
    return (letters[:p] + letters[p + g:])[:n]


def timed(ctx, db, hits, alns, queries, what, **kw):
    ms = []
    par = capi.GapParams.default(0.0, True)
    for i in range(23):
        out = ctx.pileup_gapped(db, hits, alns, queries, par, **kw)
        if i >= 3:
            ms.append(ctx.gapped_kernel_ms)
    stats = out[0] if isinstance(out, tuple) else out
    print("  %-46s median %.3f ms (min %.3f, max %.3f)  candidates %d rescued %d gap letters %d too long %d" % (
        what, float(np.median(ms)), min(ms), max(ms), int(stats[:, 0].sum()), int(stats[:, 1].sum()), int(stats[:, 2].sum()), int(stats[:, 3].sum())))


def map_timed(ctx, db, alns, queries):
    ms = []
    for i in range(23):
        ctx.pileup_map(db, alns, queries, skip_extended_targets=True, records=True)
        if i >= 3:
            ms.append(ctx.map_kernel_ms)
    print("  %-46s median %.3f ms (min %.3f, max %.3f)" % ("cdm_pileup_map with records, same handles", float(np.median(ms)), min(ms), max(ms)))


def both_forms(ctx, db, hits, alns, queries):
    timed(ctx, db, hits, alns, queries, "statistics alone")
    timed(ctx, db, hits, alns, queries, "statistics, records, operations and words", records=True)
    map_timed(ctx, db, alns, queries)


def cli_corpus(ctx):
    import test_gpu_contig_breaks_cli as t
    c = t.build_corpus()
    rng = np.random.default_rng(3)
    reads = list(c["reads"])
    for i in range(0, len(reads), 50):
        contig = c["contigs"][0].upper()
        at = int(rng.integers(0, 300))
        reads[i] = with_indel(rng, contig[at:at + 84], 80)
    reads = [reads[i] for i in t.createdb_order(len(reads))]
    both = ctx.concat(ctx.upload_seqs(c["contigs"]), ctx.upload_seqs(reads), 1, 0)
    hits = ctx.kmermatch(both, capi.KmerParams.reads_default())
    alns = ctx.rescore(both, hits, capi.RescoreParams.default())
    print("1. the CLI test corpus: 3 contigs of 400 letters, %d reads of 40..80 letters, %d hits and %d records in the sets" % (len(reads), hits.count, alns.count))
    both_forms(ctx, both, hits, alns, [0, 1, 2])


def deep(ctx):
    rng = np.random.default_rng(7)
    n, length, rl = 100_000, 100_000, 100
    contig = "".join(rng.choice(list("ACGT"), size=length))
    seqs, recs, hits = [contig], [(0, 0, 0, 0, length - 1, 0, length - 1, 1.0)], [(0, 2 * length, 0)]
    starts = rng.integers(0, length - rl - 3, size=n)
    for i in range(n):
        at = int(starts[i])
        if i % 50 == 0:
            r = with_indel(rng, contig[at:at + rl + 4], rl)
        else:
            r = list(contig[at:at + rl])
            for j in rng.integers(0, rl, size=2):
                r[j] = "ACGT"[("ACGT".index(r[j]) + 1) % 4]
            r = "".join(r)
            recs.append(unorient(1 + i, at, at + rl - 1, 0, rl - 1, bool(i & 1), rl))
        seqs.append(r.translate(COMP)[::-1] if i & 1 else r)
        d = (length - rl - at) if i & 1 else at
        hits.append((1 + i, -50 if i & 1 else 50, ((d & 0xFFFF) ^ 0x8000) - 0x8000))
    off, rec = csr(len(seqs), {0: recs})
    hoff = np.full(len(seqs) + 1, len(hits), np.uint64)
    hoff[0] = 0
    db = ctx.upload_seqs(seqs, ext=[1] + [0] * n)
    alns = ctx.upload_alns(db, off, rec)
    h = ctx.upload_hits(db, hoff, np.array(hits, capi.HIT_DTYPE))
    print("2. one contig of %d letters under %d reads of %d letters, %d of them with an indel and without record" % (length, n, rl, n - len(recs) + 1))
    both_forms(ctx, db, h, alns, [0])
    for chunk in ("64", "256"):         # the one contig's hits in more, smaller work items (the default is 1024 a wave)
        os.environ["CDM_PILEUP_CHUNK"] = chunk
        timed(ctx, db, h, alns, [0], "records, CDM_PILEUP_CHUNK=" + chunk, records=True)
    del os.environ["CDM_PILEUP_CHUNK"]


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
    print("3. %d synth reads of 100 letters, %d hits and %d records in the sets, %d queries with two hits or more" % (n, hits.count, alns.count, len(queries)))
    both_forms(ctx, db, hits, alns, queries)


if __name__ == "__main__":
    ctx = capi.Ctx(0)
    cli_corpus(ctx)
    deep(ctx)
    synth_reads(ctx)
