// Per-query coverage and damage tables of the read pile-up (cdm_pileup_profile; not a module of the reference).  The other reductions
// over the same pile-up are in pileup_depth.hip and pileup_bases.hip, what they all share in pileup.h.
//
// ancient_correction orients every record of a query and piles the targets up column by column (correct.hip: orient(), targetBase());
// this unit walks the same columns and COUNTS: for the first and the last `ends` positions of every read, which query base stands
// under which read base - the tables a damage profiler builds from a mapping (C->T falling off from the 5' end, G->A from the 3' end).
//
// A record touches at most 2 x ends columns, whatever its length: the work per record is small and bounded; the number of records
// of a query (a contig under 10 M reads) is not.  So the work items are (query, chunk of its records), cut by a scan over the listed
// queries' record counts.  One wave takes one item, its lanes take records, and the 2 x ends x 16 table of the item lives in the wave's
// slice of the LDS as 32-bit counters (LDS atomics: the lanes of a wave meet on the few hot cells - C under C, T under C at position 0 -
// where the LDS serialises them, not a memory channel).  The table is flushed ONCE per item with 64-bit global atomics into the
// query's own row: different queries never share a word, and a query with k chunks sees k adds per cell at the most.
#include "pileup.h"

namespace {

constexpr int PU_MAX_ENDS = 64;

struct PileupArgs : ItemArgs {
    const uint32_t *codes, *nmask;
    uint32_t ends;
    unsigned long long *counts, *reads, *columns;       // [nq][2][ends][4][4], [nq], [nq]
};

// one wave per work item of this launch's slice [first, first + nThis)
__global__ __launch_bounds__(64 * PU_WAVES) void k_pileup(PileupArgs a, uint64_t first, uint64_t nThis) {
    extern __shared__ uint32_t sTab[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;                       // (no block-wide barrier below: a wave may leave on its own)
    const uint64_t item = first + local;
    const uint32_t P = a.ends, cells = 2u * P * 16u;
    uint32_t *tab = sTab + (uint32_t) wave * cells;
    const ItemRecords it = itemRecords(a, item);
    const uint32_t qi = it.qi, q = it.q;
    for (uint32_t i = lane; i < cells; i += 64) tab[i] = 0;
    waveLdsSync();
    const SeqMeta qm = a.meta[q];
    const uint32_t qLen = qm.len, qw = qm.woff;
    unsigned int nReads = 0; unsigned long long nCols = 0;
    for (uint64_t r = it.r0 + lane; r < it.r1; r += 64) {
        const AlnRec rec = a.rec[r];
        Oriented o; uint32_t tLen, tw;
        if (!countedRecord(a.meta, a.n, a.skipExt, a.minSeqId, q, qLen, rec, o, tLen, tw)) continue;
        const uint32_t L = (uint32_t) (o.qe - o.qs) + 1u;
        nReads++; nCols += L;
        // the overlap on the read as stored: positions [pLo, pHi]
        const uint32_t pLo = o.rev ? tLen - 1u - (uint32_t) o.de : (uint32_t) o.ds, pHi = pLo + L - 1u;
        // column of read position p: query position, both letters; false where either is N
        auto column = [&](uint32_t p, uint32_t &x, uint32_t &y) {
            const uint32_t op = o.rev ? tLen - 1u - p : p;
            const uint32_t qpos = (uint32_t) o.qs + (op - (uint32_t) o.ds);
            if (cdm_isN(a.nmask, qw, qpos) || cdm_isN(a.nmask, tw, p)) return false;
            y = cdm_base(a.codes, tw, p);
            x = cdm_base(a.codes, qw, qpos);
            if (o.rev) x = 3u - x;                    // the query base as the read's strand sees it
            return true;
        };
        uint32_t x, y;
        // 5' table: read positions p < ends
        for (uint32_t p = pLo; p <= pHi && p < P; p++)
            if (column(p, x, y)) atomicAdd(&tab[(p * 4u + x) * 4u + y], 1u);
        // 3' table: distances tLen - 1 - p < ends
        for (uint32_t p = max(pLo, tLen > P ? tLen - P : 0u); p <= pHi; p++)
            if (column(p, x, y)) atomicAdd(&tab[P * 16u + ((tLen - 1u - p) * 4u + x) * 4u + y], 1u);
    }
    waveLdsSync();
    unsigned long long *row = a.counts + (uint64_t) qi * cells;
    for (uint32_t i = lane; i < cells; i += 64) { const uint32_t v = tab[i]; if (v) atomicAdd(&row[i], (unsigned long long) v); }
    addReadsColumns(&a.reads[qi], &a.columns[qi], nReads, nCols, lane);
}
}  // namespace

// test aid, not part of the public header: records per work item as the next call will cut them (tests pile up one record more)
extern "C" uint32_t cdm_pileup_chunk_records(void) { return pileupChunk(); }

static int cdm_pileup_impl(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t nq, const cdm_pileup_params *par, uint64_t *counts,
                           uint64_t *reads, uint64_t *columns) {
    hipStream_t s = ctx->stream;
    const uint32_t P = (uint32_t) par->ends, cells = 2u * P * 16u, chunk = pileupChunk();
    DevBuf<SeqMeta> meta;
    if (int rc = cdm_build_meta(ctx, db, &meta.p)) return rc;
    // the listed queries in batches whose tables take at most 1 GB of device memory
    const uint64_t batch = std::max<uint64_t>(1, (1ull << 30) / ((uint64_t) cells * 8));
    float msTotal = 0.f;
    for (uint64_t b0 = 0; b0 < nq; b0 += batch) {
        const uint32_t m = (uint32_t) std::min<uint64_t>(batch, nq - b0);
        DevBuf<uint32_t> dq; WorkItems work; DevBuf<unsigned long long> dCounts, dReads, dCols;
        if (!dq.alloc(m) || !work.alloc(m) || !dCounts.alloc((size_t) m * cells) || !dReads.alloc(m) || !dCols.alloc(m)) {
            cdm_set_error("cdm_pileup_profile: out of device memory for the tables of %u queries", m); return CDM_ERR_HIP;
        }
        CDM_HIP(hipMemcpyAsync(dq.p, queries + b0, (size_t) m * 4, hipMemcpyHostToDevice, s));
        CDM_HIP(hipMemsetAsync(dCounts.p, 0, (size_t) m * cells * 8, s));
        CDM_HIP(hipMemsetAsync(dReads.p, 0, (size_t) m * 8, s));
        CDM_HIP(hipMemsetAsync(dCols.p, 0, (size_t) m * 8, s));
        if (int rc = workItems(s, alns, dq.p, m, chunk, work)) return rc;
        PileupArgs a;
        fillArgs(a, meta.p, db, alns, par->min_seq_id, par->skip_extended_targets, work);
        a.codes = db->codes; a.nmask = db->nmask; a.ends = P;
        a.counts = dCounts.p; a.reads = dReads.p; a.columns = dCols.p;
        hipEventRecord(ctx->ev0, s);
        launchWaveItems(s, k_pileup, a, work.n, (size_t) PU_WAVES * cells * 4);
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        CDM_HIP(hipMemcpyAsync(counts + b0 * cells, dCounts.p, (size_t) m * cells * 8, hipMemcpyDeviceToHost, s));
        CDM_HIP(hipMemcpyAsync(reads + b0, dReads.p, (size_t) m * 8, hipMemcpyDeviceToHost, s));
        CDM_HIP(hipMemcpyAsync(columns + b0, dCols.p, (size_t) m * 8, hipMemcpyDeviceToHost, s));
        if (int rc = finishTimed(ctx, "cdm_pileup_profile", "kernel", msTotal)) return rc;
    }
    ctx->lastMs[16] = msTotal;
    return CDM_OK;
}

extern "C" int cdm_pileup_profile(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_pileup_params *par,
                                  uint64_t *counts, uint64_t *reads, uint64_t *columns) {
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, "cdm_pileup_profile");
    if (!ctx || !db || !alns || !par || (n_queries && (!queries || !counts || !reads || !columns))) { cdm_set_error("cdm_pileup_profile: NULL argument"); return CDM_ERR_INVALID; }
    if (par->ends < 1 || par->ends > PU_MAX_ENDS) { cdm_set_error("cdm_pileup_profile: ends = %d; the tables hold 1 to %d positions from either end of a read", par->ends, PU_MAX_ENDS); return CDM_ERR_INVALID; }
    if (int rc = pileupCheckArgs("cdm_pileup_profile", db, alns, queries, n_queries)) return rc;
    if (n_queries == 0) return CDM_OK;
    CDM_HIP(hipSetDevice(ctx->device));
    return cdm_pileup_impl(ctx, db, alns, queries, n_queries, par, counts, reads, columns);
}
