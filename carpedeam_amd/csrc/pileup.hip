// Per-query coverage and damage tables of the read pile-up (cdm_pileup_profile; not a module of the reference).
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
#include <algorithm>

#include "common.h"
#include "devutil.h"
#include "scan.h"

namespace {

constexpr int PU_WAVES = 4;                    // waves per block; ends = 64 takes 4 x 8 KB of LDS
// Records per work item.  A cell of an item's table gets at most ONE increment per record and table (a read has one column at each of
// its positions), so a 32-bit cell cannot overflow while an item holds fewer than 2^32 records; the bound asked of this unit is the
// stricter 2^32 / (2 x ends) = 2^25 records at ends = 64 (every increment of a record counted as if it fell on one cell).  The chunk
// is capped at 2^20, far below either.  CDM_PILEUP_CHUNK=<records> (tests): small pile-ups in several items.
constexpr uint32_t PU_CHUNK_DEFAULT = 1024, PU_CHUNK_MAX = 1u << 20;
constexpr int PU_MAX_ENDS = 64;

uint32_t pileupChunk() {
    if (const char *e = cdmGetenv("CDM_PILEUP_CHUNK")) { const long long v = atoll(e); if (v > 0) return (uint32_t) std::min<long long>(v, PU_CHUNK_MAX); }
    return PU_CHUNK_DEFAULT;
}

struct PileupArgs {
    const SeqMeta *meta; const uint32_t *codes, *nmask;
    const uint64_t *aoff; const AlnRec *rec;
    const uint32_t *queries;        // [nq] the listed queries of this call's batch
    const uint64_t *itemOff;        // [nq + 1] first work item of each listed query
    uint32_t n, nq, chunk, ends, skipExt; float minSeqId;
    unsigned long long *counts, *reads, *columns;       // [nq][2][ends][4][4], [nq], [nq]
};

// work items per listed query: its records in chunks
__global__ void k_pileup_chunks(const uint64_t *__restrict__ aoff, const uint32_t *__restrict__ queries, uint32_t nq, uint32_t chunk, uint64_t *__restrict__ items) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nq) return;
    uint64_t c = 0;
    if (i < nq) { const uint32_t q = queries[i]; c = (aoff[q + 1] - aoff[q] + chunk - 1) / chunk; }
    items[i] = c;
}

// oriented copy of a record (correction.cpp:229-242; correct.hip orient())
struct Oriented { int qs, qe, ds, de; bool rev; };
__device__ __forceinline__ Oriented orient(const AlnRec &r, uint32_t dbLen) {
    Oriented o;
    if (r.qStart > r.qEnd) { o.qs = r.qEnd; o.qe = r.qStart; o.ds = (int) dbLen - r.dbEnd - 1; o.de = (int) dbLen - r.dbStart - 1; o.rev = true; }
    else { o.qs = r.qStart; o.qe = r.qEnd; o.ds = r.dbStart; o.de = r.dbEnd; o.rev = false; }
    return o;
}

__device__ __forceinline__ void waveLdsSync() {     // LDS traffic of this wave's lanes in front of the call is visible to all of them behind it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one wave per work item of this launch's slice [first, first + nThis)
__global__ __launch_bounds__(64 * PU_WAVES) void k_pileup(PileupArgs a, uint64_t first, uint64_t nThis) {
    extern __shared__ uint32_t sTab[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;                       // (no block-wide barrier below: a wave may leave on its own)
    const uint64_t item = first + local;
    const uint32_t P = a.ends, cells = 2u * P * 16u;
    uint32_t *tab = sTab + (uint32_t) wave * cells;
    // the listed query that owns the item: the last i with itemOff[i] <= item (a query without records owns no item)
    uint32_t lo = 0, hi = a.nq;
    while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (a.itemOff[mid] <= item) lo = mid; else hi = mid; }
    const uint32_t qi = lo, q = a.queries[qi];
    const uint64_t r0 = a.aoff[q] + (item - a.itemOff[qi]) * a.chunk, r1 = min((uint64_t) a.aoff[q + 1], r0 + a.chunk);
    for (uint32_t i = lane; i < cells; i += 64) tab[i] = 0;
    waveLdsSync();
    const SeqMeta qm = a.meta[q];
    const uint32_t qLen = qm.len, qw = qm.woff;
    unsigned int nReads = 0; unsigned long long nCols = 0;
    for (uint64_t r = r0 + lane; r < r1; r += 64) {
        const AlnRec rec = a.rec[r];
        const uint32_t t = rec.target;
        if (t == q || t >= a.n) continue;             // the identity record is not a read on the query
        if (!(rec.seqId >= a.minSeqId)) continue;
        const SeqMeta tm = a.meta[t];
        if (a.skipExt && (tm.flags & 2u)) continue;
        const uint32_t tLen = tm.len, tw = tm.woff;
        const Oriented o = orient(rec, tLen);
        // (every record of a set went through cdm_alns_upload's checks or came from cdm_rescore; a record that does not fit its two
        // sequences all the same is left out here, not followed out of bounds)
        if (o.qs < 0 || o.ds < 0 || o.qe < o.qs || (uint32_t) o.qe >= qLen || (uint32_t) o.de >= tLen || o.qe - o.qs != o.de - o.ds) continue;
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
    const unsigned int rd = (unsigned int) cdm_wave_sum((int) nReads);      // (at most 2^20 records per item)
    const unsigned long long cl = cdm_wave_incl_sum<unsigned long long>(nCols);
    if (lane == 63 && rd) { atomicAdd(&a.reads[qi], (unsigned long long) rd); atomicAdd(&a.columns[qi], cl); }
}

}  // namespace

// test aid, not part of the public header: records per work item as the next call will cut them (tests pile up one record more)
extern "C" uint32_t cdm_pileup_chunk_records(void) { return pileupChunk(); }

int cdm_pileup_impl(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t nq, const cdm_pileup_params *par, uint64_t *counts,
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
        DevBuf<uint32_t> dq; DevBuf<uint64_t> items, itemOff; DevBuf<unsigned long long> dCounts, dReads, dCols;
        if (!dq.alloc(m) || !items.alloc((size_t) m + 1) || !itemOff.alloc((size_t) m + 1) || !dCounts.alloc((size_t) m * cells) || !dReads.alloc(m) || !dCols.alloc(m)) {
            cdm_set_error("cdm_pileup_profile: out of device memory for the tables of %u queries", m); return CDM_ERR_HIP;
        }
        CDM_HIP(hipMemcpyAsync(dq.p, queries + b0, (size_t) m * 4, hipMemcpyHostToDevice, s));
        CDM_HIP(hipMemsetAsync(dCounts.p, 0, (size_t) m * cells * 8, s));
        CDM_HIP(hipMemsetAsync(dReads.p, 0, (size_t) m * 8, s));
        CDM_HIP(hipMemsetAsync(dCols.p, 0, (size_t) m * 8, s));
        hipLaunchKernelGGL(k_pileup_chunks, dim3((m + 256) / 256), dim3(256), 0, s, (const uint64_t *) alns->off, (const uint32_t *) dq.p, m, chunk, items.p);
        cdmscan::ScanTemp st;
        if (int rc = cdmscan::exclusiveScan<uint64_t>(s, st, items.p, itemOff.p, (size_t) m + 1)) return rc;
        uint64_t nItems = 0;
        CDM_HIP(hipMemcpyAsync(&nItems, itemOff.p + m, 8, hipMemcpyDeviceToHost, s));
        CDM_HIP(hipStreamSynchronize(s));
        PileupArgs a;
        a.meta = meta.p; a.codes = db->codes; a.nmask = db->nmask; a.aoff = alns->off; a.rec = alns->rec; a.queries = dq.p; a.itemOff = itemOff.p;
        a.n = (uint32_t) db->n; a.nq = m; a.chunk = chunk; a.ends = P; a.skipExt = par->skip_extended_targets ? 1u : 0u; a.minSeqId = par->min_seq_id;
        a.counts = dCounts.p; a.reads = dReads.p; a.columns = dCols.p;
        hipEventRecord(ctx->ev0, s);
        for (uint64_t first = 0, slice = cdmSliceItems(64); first < nItems; first += slice) {
            const uint64_t nThis = std::min<uint64_t>(slice, nItems - first);
            hipLaunchKernelGGL(k_pileup, CDM_GRID((nThis + PU_WAVES - 1) / PU_WAVES, 64 * PU_WAVES), dim3(64 * PU_WAVES), (size_t) PU_WAVES * cells * 4, s, a, first, nThis);
        }
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        CDM_HIP(hipMemcpyAsync(counts + b0 * cells, dCounts.p, (size_t) m * cells * 8, hipMemcpyDeviceToHost, s));
        CDM_HIP(hipMemcpyAsync(reads + b0, dReads.p, (size_t) m * 8, hipMemcpyDeviceToHost, s));
        CDM_HIP(hipMemcpyAsync(columns + b0, dCols.p, (size_t) m * 8, hipMemcpyDeviceToHost, s));
        { hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) { cdm_set_error("cdm_pileup_profile: the kernel failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; } }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) msTotal += ms;
    }
    ctx->lastMs[16] = msTotal;
    return CDM_OK;
}

extern "C" int cdm_pileup_profile(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_pileup_params *par,
                                  uint64_t *counts, uint64_t *reads, uint64_t *columns) {
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, "cdm_pileup_profile");
    if (!ctx || !db || !alns || !par || (n_queries && (!queries || !counts || !reads || !columns))) { cdm_set_error("cdm_pileup_profile: NULL argument"); return CDM_ERR_INVALID; }
    if (par->ends < 1 || par->ends > PU_MAX_ENDS) { cdm_set_error("cdm_pileup_profile: ends = %d; the tables hold 1 to %d positions from either end of a read", par->ends, PU_MAX_ENDS); return CDM_ERR_INVALID; }
    if (alns->n != db->n) { cdm_set_error("cdm_pileup_profile: alignment CSR has %llu queries, DB has %llu", (unsigned long long) alns->n, (unsigned long long) db->n); return CDM_ERR_INVALID; }
    if (db->residues && !db->codes) { cdm_set_error("cdm_pileup_profile: the DB holds no letters (an index copy)"); return CDM_ERR_INVALID; }
    {
        std::vector<uint32_t> sorted(queries, queries + n_queries);
        std::sort(sorted.begin(), sorted.end());
        if (n_queries && sorted.back() >= db->n) { cdm_set_error("cdm_pileup_profile: query index %u of a DB of %llu sequences", sorted.back(), (unsigned long long) db->n); return CDM_ERR_INVALID; }
        for (uint64_t i = 1; i < n_queries; i++)
            if (sorted[i] == sorted[i - 1]) { cdm_set_error("cdm_pileup_profile: query index %u is listed twice", sorted[i]); return CDM_ERR_INVALID; }
    }
    if (n_queries == 0) return CDM_OK;
    CDM_HIP(hipSetDevice(ctx->device));
    return cdm_pileup_impl(ctx, db, alns, queries, n_queries, par, counts, reads, columns);
}
