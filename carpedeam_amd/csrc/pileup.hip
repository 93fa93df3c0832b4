// Per-query coverage and damage tables of the read pile-up (cdm_pileup_profile), the depth at every position of a query with its
// statistics (cdm_pileup_depth, the second part of this file), the per-position base counts with the variant sites
// (cdm_pileup_bases, the third) and the contig break points from spanning reads (cdm_pileup_breaks, the fourth); none is a module of
// the reference.
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

// The records that count on query q of qLen letters (the rule of cdm_pileup_profile and cdm_pileup_depth, include/carpedeam_hip.h):
// true with the oriented record, its target's length and word offset.
__device__ __forceinline__ bool countedRecord(const SeqMeta *__restrict__ meta, uint32_t n, uint32_t skipExt, float minSeqId, uint32_t q, uint32_t qLen, const AlnRec &rec,
                                              Oriented &o, uint32_t &tLen, uint32_t &tw) {
    const uint32_t t = rec.target;
    if (t == q || t >= n) return false;               // the identity record is not a read on the query
    if (!(rec.seqId >= minSeqId)) return false;
    const SeqMeta tm = meta[t];
    if (skipExt && (tm.flags & 2u)) return false;
    tLen = tm.len; tw = tm.woff;
    o = orient(rec, tLen);
    // (every record of a set went through cdm_alns_upload's checks or came from cdm_rescore; a record that does not fit its two
    // sequences all the same is left out here, not followed out of bounds)
    return !(o.qs < 0 || o.ds < 0 || o.qe < o.qs || (uint32_t) o.qe >= qLen || (uint32_t) o.de >= tLen || o.qe - o.qs != o.de - o.ds);
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
    const unsigned int rd = (unsigned int) cdm_wave_sum((int) nReads);      // (at most 2^20 records per item)
    const unsigned long long cl = cdm_wave_incl_sum<unsigned long long>(nCols);
    if (lane == 63 && rd) { atomicAdd(&a.reads[qi], (unsigned long long) rd); atomicAdd(&a.columns[qi], cl); }
}

// ---------------------------------------------------------------------------------------------- cdm_pileup_depth
// Depth at every position of the listed queries, and its statistics (include/carpedeam_hip.h).  k_pileup touches at most 2 x ends
// columns of a record; depth touches all of them, so the records are not walked column by column: a counted record MARKS its two ends
// in a 32-bit cell array (+1 at qs, -1 behind qe; len + 1 cells per listed query, the last one its closing cell), every query's cells
// sum to zero, and ONE device-wide prefix sum over the batch's cells turns the marks into depths - no segmented scan.  A third kernel
// walks the positions in tiles and reduces the statistics.  The cells live modulo 2^32: a depth is below the query's record count,
// and a query with 2^32 records or more is refused.
constexpr int DP_NT = 256, DP_PER = 8, DP_TILE = DP_NT * DP_PER;       // positions per statistics item
constexpr uint64_t DP_CELLS_DEFAULT = 1ull << 28, DP_CELLS_MAX = 1ull << 32;

uint64_t depthCells() {     // CDM_DEPTH_CELLS=<cells> (tests): small inputs in several batches
    if (const char *e = cdmGetenv("CDM_DEPTH_CELLS")) { const long long v = atoll(e); if (v > 0) return std::min<uint64_t>((uint64_t) v, DP_CELLS_MAX); }
    return DP_CELLS_DEFAULT;
}

struct DepthArgs {
    const SeqMeta *meta; const uint64_t *aoff; const AlnRec *rec;
    const uint32_t *queries;        // [nq] the listed queries of this call's batch
    const uint64_t *itemOff;        // [nq + 1] first marking item (chunk of records) of each listed query
    const uint64_t *tileOff;        // [nq + 1] first statistics item (tile of positions) of each
    const uint64_t *base;           // [nq + 1] first cell of each
    uint32_t n, nq, chunk, skipExt, edge; float minSeqId;
    uint32_t *cells;                // [base[nq]]
    unsigned long long *stats;      // [nq][8]
    uint32_t *track;                // NULL, or [base[nq] - nq]: the depths without the closing cells
};

// length and record count of every listed query
__global__ void k_depth_sizes(const SeqMeta *__restrict__ meta, const uint64_t *__restrict__ aoff, const uint32_t *__restrict__ queries, uint64_t nq, uint32_t *__restrict__ len,
                              uint64_t *__restrict__ recs) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const uint32_t q = queries[i];
    len[i] = meta[q].len; recs[i] = aoff[q + 1] - aoff[q];
}

__device__ __forceinline__ unsigned long long waveSum64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v += ((unsigned long long) (unsigned int) __shfl_xor((int) (v >> 32), o, 64) << 32) | (unsigned int) __shfl_xor((int) (unsigned int) v, o, 64);
    return v;
}

// The marks of one item (listed query, chunk of its records) by one wave, lanes take records: +1 at qs and -1 behind qe in the depth
// cells; with SPAN (cdm_pileup_breaks, the fourth part of this file) also +1 at qs + w and -1 at qe + 2 - w in a second plane of the same
// layout `plane` cells behind the first, for the records of at least 2 w columns.  reads and columns go to the query's stats row, once
// per item.
template <bool SPAN>
__device__ __forceinline__ void depthMarkItem(const DepthArgs &a, uint64_t item, int lane, uint32_t w, uint64_t plane) {
    uint32_t lo = 0, hi = a.nq;
    while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (a.itemOff[mid] <= item) lo = mid; else hi = mid; }
    const uint32_t qi = lo, q = a.queries[qi];
    const uint64_t r0 = a.aoff[q] + (item - a.itemOff[qi]) * a.chunk, r1 = min((uint64_t) a.aoff[q + 1], r0 + a.chunk);
    const uint32_t qLen = a.meta[q].len;
    uint32_t *cell = a.cells + a.base[qi];
    unsigned int nReads = 0; unsigned long long nCols = 0;
    for (uint64_t r = r0 + lane; r < r1; r += 64) {
        const AlnRec rec = a.rec[r];
        Oriented o; uint32_t tLen, tw;
        if (!countedRecord(a.meta, a.n, a.skipExt, a.minSeqId, q, qLen, rec, o, tLen, tw)) continue;
        const uint32_t L = (uint32_t) (o.qe - o.qs) + 1u;
        nReads++; nCols += L;
        atomicAdd(&cell[(uint32_t) o.qs], 1u);                        // (results unused: atomics without return)
        atomicAdd(&cell[(uint32_t) o.qe + 1u], 0xFFFFFFFFu);          // qe < qLen: at the most the query's closing cell
        if (SPAN && L >= 2u * w) {                                    // qs + w <= qe + 1 - w < qe + 2 - w <= qLen (w >= 1): inside the query's cells
            atomicAdd(&cell[plane + (uint32_t) o.qs + w], 1u);
            atomicAdd(&cell[plane + (uint32_t) o.qe + 2u - w], 0xFFFFFFFFu);
        }
    }
    const unsigned int rd = (unsigned int) cdm_wave_sum((int) nReads);
    const unsigned long long cl = waveSum64(nCols);
    if (lane == 0 && rd) { atomicAdd(&a.stats[(uint64_t) qi * 8], (unsigned long long) rd); atomicAdd(&a.stats[(uint64_t) qi * 8 + 1], cl); }
}

// marks: one wave per item of this launch's slice
__global__ __launch_bounds__(64 * PU_WAVES) void k_depth_marks(DepthArgs a, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    depthMarkItem<false>(a, first + local, lane, 0u, 0ull);
}

// statistics: one block per item (listed query, tile of DP_TILE positions) of this launch's slice, on the scanned cells:
// depth[p] = the exclusive prefix at cell p + 1
__global__ __launch_bounds__(DP_NT) void k_depth_stats(DepthArgs a, uint64_t first) {
    __shared__ unsigned long long sRed[DP_NT / 64][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t item = first + blockIdx.x;
    uint32_t lo = 0, hi = a.nq;
    while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (a.tileOff[mid] <= item) lo = mid; else hi = mid; }
    const uint32_t qi = lo, len = a.meta[a.queries[qi]].len;
    const uint64_t cb = a.base[qi], p0 = (item - a.tileOff[qi]) * DP_TILE;
    // the statistics window: the whole query when len <= 2 x edge, else [edge, len - 1 - edge]
    uint32_t w0 = 0, w1 = len - 1u;
    if ((uint64_t) len > 2ull * a.edge) { w0 = a.edge; w1 = len - 1u - a.edge; }
    const uint32_t *__restrict__ cell = a.cells + cb + 1;
    uint32_t *__restrict__ out = a.track ? a.track + (cb - qi) : nullptr;
    unsigned long long sum = 0, sumsq = 0; uint32_t breadth = 0, covered = 0, mx = 0;
#pragma unroll
    for (int j = 0; j < DP_PER; j++) {
        const uint64_t p = p0 + threadIdx.x + (uint64_t) DP_NT * j;
        if (p >= len) continue;
        const uint32_t d = cell[p];
        if (out) out[p] = d;
        breadth += d != 0;
        if (p >= w0 && p <= w1) { covered += d != 0; sum += d; sumsq += (unsigned long long) d * d; mx = max(mx, d); }
    }
    sum = waveSum64(sum); sumsq = waveSum64(sumsq);
    const unsigned long long bc = waveSum64(((unsigned long long) breadth << 32) | covered);       // (at most DP_TILE each)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t) __shfl_xor((int) mx, o, 64));
    if (lane == 0) { sRed[wave][0] = sum; sRed[wave][1] = sumsq; sRed[wave][2] = bc; sRed[wave][3] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t[3] = {0, 0, 0}, m = 0;
        for (int w = 0; w < DP_NT / 64; w++) { t[0] += sRed[w][0]; t[1] += sRed[w][1]; t[2] += sRed[w][2]; m = max(m, sRed[w][3]); }
        unsigned long long *row = a.stats + (uint64_t) qi * 8;
        if (t[2] >> 32) atomicAdd(&row[2], t[2] >> 32);
        if (t[2] & 0xFFFFFFFFull) atomicAdd(&row[4], t[2] & 0xFFFFFFFFull);
        if (t[0]) { atomicAdd(&row[5], t[0]); atomicAdd(&row[6], t[1]); atomicMax(&row[7], m); }
    }
}

// ---------------------------------------------------------------------------------------------- cdm_pileup_bases
// Which bases the reads put on every position of the listed queries, and the positions where they disagree with the query or among
// themselves (include/carpedeam_hip.h).  Unlike the two reductions above this one walks EVERY column of every counted record, so the
// lanes of a wave take the columns of ONE record, not records: a wave instruction then reads one or two read code words per 16 lanes and
// adds to consecutive words.  The batch's counters are eight planes [forward A,C,G,T, reverse A,C,G,T][position]: the lanes of one
// instruction that carry the same base add to a contiguous run of one plane (an interleaved [position][8] table would touch one word
// in each of 64 separate 32-byte cells).  A second kernel reads the planes by tiles of positions, classifies, reduces the query's
// figures and marks the flagged positions; one prefix sum over the marks places the site records, which a third kernel writes.
constexpr uint64_t BS_POS_DEFAULT = 1ull << 25;         // positions per batch: 2^25 x 8 planes x 4 bytes = 1 GB
constexpr int BS_MAX_MASK = 64;

uint64_t basesPositions() {     // CDM_BASES_POSITIONS=<positions> (tests): small inputs in several batches
    if (const char *e = cdmGetenv("CDM_BASES_POSITIONS")) { const long long v = atoll(e); if (v > 0) return std::min<uint64_t>((uint64_t) v, BS_POS_DEFAULT); }
    return BS_POS_DEFAULT;
}

struct BasesArgs {
    const SeqMeta *meta; const uint32_t *codes, *nmask; const uint64_t *aoff; const AlnRec *rec;
    const uint32_t *queries;        // [nq] the listed queries of this call's batch
    const uint64_t *itemOff;        // [nq + 1] first counting item (chunk of records) of each listed query
    const uint64_t *tileOff;        // [nq + 1] first classification item (tile of positions) of each
    const uint64_t *base;           // [nq + 1] first position of each in a plane
    uint32_t n, nq, chunk, skipExt, maskEnds, minDepth, minAlt, minPct, firstQuery; float minSeqId;
    uint64_t nPos;                  // positions of the batch: the length of a plane
    uint32_t *planes;               // [8][nPos]
    unsigned long long *stats;      // [nq][8]
    uint32_t *place;                // [nPos + 1]: 0/1 per flagged position, after the scan the position's first site record
    uint32_t *counts;               // NULL, or [nPos][8]
    cdm_site *sites;                // k_base_emit: [place[nPos]]
};

// counting: one wave per item (listed query, chunk of its records) of this launch's slice.  Each lane loads one record and evaluates
// the filter; the wave then walks the counted records one at a time, its lanes on the columns lane, lane + 64, ...
__global__ __launch_bounds__(64 * PU_WAVES) void k_base_counts(BasesArgs a, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    const uint64_t item = first + local;
    uint32_t lo = 0, hi = a.nq;
    while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (a.itemOff[mid] <= item) lo = mid; else hi = mid; }
    const uint32_t qi = lo, q = a.queries[qi];
    const uint64_t r0 = a.aoff[q] + (item - a.itemOff[qi]) * a.chunk, r1 = min((uint64_t) a.aoff[q + 1], r0 + a.chunk);
    const uint32_t qLen = a.meta[q].len, m = a.maskEnds;
    uint32_t *__restrict__ plane0 = a.planes + a.base[qi];
    unsigned int nReads = 0; unsigned long long nCols = 0;
    for (uint64_t rb = r0; rb < r1; rb += 64) {       // (wave-uniform: the shuffles below see all 64 lanes)
        Oriented o = {0, 0, 0, 0, false}; uint32_t tLen = 0, tw = 0;
        bool counted = false;
        if (rb + lane < r1) { const AlnRec rec = a.rec[rb + lane]; counted = countedRecord(a.meta, a.n, a.skipExt, a.minSeqId, q, qLen, rec, o, tLen, tw); }
        const uint32_t myL = counted ? (uint32_t) (o.qe - o.qs) + 1u : 0u;
        nReads += counted; nCols += myL;
        for (unsigned long long live = __ballot(counted); live; live &= live - 1) {
            const int src = __ffsll((long long) live) - 1;
            const uint32_t qs = (uint32_t) __shfl(o.qs, src, 64), ds = (uint32_t) __shfl(o.ds, src, 64), L = __shfl(myL, src, 64);
            const uint32_t len = __shfl(tLen, src, 64), w = __shfl(tw, src, 64), rev = (uint32_t) __shfl((int) o.rev, src, 64);
            // (countedRecord: qs + L <= qLen and ds + L <= len, so every index below stays inside the query's planes and the read's words)
            for (uint32_t c = lane; c < L; c += 64) {
                const uint32_t op = ds + c, p = rev ? len - 1u - op : op;
                if (cdm_isN(a.nmask, w, p)) continue;
                if (m && (p < m || len - 1u - p < m)) continue;
                uint32_t b = cdm_base(a.codes, w, p);
                if (rev) b = 3u - b;                  // the read base as the query's strand sees it
                atomicAdd(&plane0[(uint64_t) (rev * 4u + b) * a.nPos + qs + c], 1u);        // (result unused: an atomic without return)
            }
        }
    }
    const unsigned int rd = (unsigned int) cdm_wave_sum((int) nReads);
    const unsigned long long cl = waveSum64(nCols);
    if (lane == 0 && rd) { atomicAdd(&a.stats[(uint64_t) qi * 8], (unsigned long long) rd); atomicAdd(&a.stats[(uint64_t) qi * 8 + 1], cl); }
}

// one position's verdict from its eight counters and the query's letter (ref: its code, 4 for N)
struct SiteCall { uint32_t ref, major, flags; unsigned long long depth, atRef; };
__device__ __forceinline__ SiteCall callSite(const uint32_t c[8], uint32_t ref, uint32_t minDepth, uint32_t minAlt, uint32_t minPct) {
    const uint32_t t[4] = {c[0] + c[4], c[1] + c[5], c[2] + c[6], c[3] + c[7]};       // (a record adds one column to a position: each below 2^32)
    SiteCall s;
    s.ref = ref; s.depth = (unsigned long long) t[0] + t[1] + t[2] + t[3];
    uint32_t mj = 0;
#pragma unroll
    for (uint32_t b = 1; b < 4; b++) if (t[b] > t[mj]) mj = b;        // the lowest code among equal largest
    if (ref < 4u && t[ref] == t[mj]) mj = ref;
    uint32_t second = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; b++) if (b != mj) second = max(second, t[b]);
    s.major = mj; s.atRef = ref < 4u ? t[ref] : 0ull;
    uint32_t f = 0;
    if (s.depth >= minDepth) {
        f = CDM_SITE_CALLED;
        if (mj != ref && t[mj] > second) f |= CDM_SITE_DIFFERS;
        if (second >= minAlt && (unsigned long long) second * 100ull >= (unsigned long long) minPct * s.depth) f |= CDM_SITE_VARIABLE;
    }
    s.flags = f;
    return s;
}

// the item (listed query, tile of DP_TILE positions) of a block and what its threads need of it
struct BaseTile { uint32_t qi, len, qw; uint64_t pb, p0; };
__device__ __forceinline__ BaseTile baseTile(const BasesArgs &a, uint64_t item) {
    uint32_t lo = 0, hi = a.nq;
    while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (a.tileOff[mid] <= item) lo = mid; else hi = mid; }
    const SeqMeta qm = a.meta[a.queries[lo]];
    BaseTile t;
    t.qi = lo; t.len = qm.len; t.qw = qm.woff; t.pb = a.base[lo]; t.p0 = (item - a.tileOff[lo]) * DP_TILE;
    return t;
}
__device__ __forceinline__ SiteCall callAt(const BasesArgs &a, const BaseTile &t, uint32_t p, uint32_t c[8]) {
#pragma unroll
    for (int k = 0; k < 8; k++) c[k] = a.planes[(uint64_t) k * a.nPos + t.pb + p];
    const uint32_t ref = cdm_isN(a.nmask, t.qw, p) ? 4u : cdm_base(a.codes, t.qw, p);
    return callSite(c, ref, a.minDepth, a.minAlt, a.minPct);
}

// classification: one block per item (listed query, tile of DP_TILE positions) of this launch's slice
__global__ __launch_bounds__(DP_NT) void k_base_sites(BasesArgs a, uint64_t first) {
    __shared__ unsigned long long sRed[DP_NT / 64][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const BaseTile t = baseTile(a, first + blockIdx.x);
    unsigned long long bases = 0, mism = 0, four = 0;       // four: called, differs, variable, flagged in 16 bits each (at most DP_TILE)
#pragma unroll
    for (int j = 0; j < DP_PER; j++) {
        const uint64_t p = t.p0 + threadIdx.x + (uint64_t) DP_NT * j;
        if (p >= t.len) continue;
        uint32_t c[8];
        const SiteCall s = callAt(a, t, (uint32_t) p, c);
        if (a.counts) {
            uint4 *row = reinterpret_cast<uint4 *>(a.counts + (t.pb + p) * 8);
            row[0] = make_uint4(c[0], c[1], c[2], c[3]); row[1] = make_uint4(c[4], c[5], c[6], c[7]);
        }
        const uint32_t fl = (s.flags & (CDM_SITE_DIFFERS | CDM_SITE_VARIABLE)) != 0;
        a.place[t.pb + p] = fl;
        bases += s.depth;
        if (s.ref < 4u) mism += s.depth - s.atRef;
        four += (unsigned long long) (s.flags & 1u) | (unsigned long long) ((s.flags >> 1) & 1u) << 16 | (unsigned long long) ((s.flags >> 2) & 1u) << 32 | (unsigned long long) fl << 48;
    }
    bases = waveSum64(bases); mism = waveSum64(mism); four = waveSum64(four);
    if (lane == 0) { sRed[wave][0] = bases; sRed[wave][1] = mism; sRed[wave][2] = four; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long r[3] = {0, 0, 0};
        for (int w = 0; w < DP_NT / 64; w++) { r[0] += sRed[w][0]; r[1] += sRed[w][1]; r[2] += sRed[w][2]; }
        unsigned long long *row = a.stats + (uint64_t) t.qi * 8;
        if (r[0]) { atomicAdd(&row[2], r[0]); if (r[1]) atomicAdd(&row[3], r[1]); }
        for (int k = 0; k < 4; k++) { const unsigned long long v = (r[2] >> (16 * k)) & 0xFFFFull; if (v) atomicAdd(&row[4 + k], v); }
    }
}

// emission: the same items; a position is flagged where the scanned marks step, and its record goes to the place the scan gave it
__global__ __launch_bounds__(DP_NT) void k_base_emit(BasesArgs a, uint64_t first) {
    const BaseTile t = baseTile(a, first + blockIdx.x);
#pragma unroll
    for (int j = 0; j < DP_PER; j++) {
        const uint64_t p = t.p0 + threadIdx.x + (uint64_t) DP_NT * j;
        if (p >= t.len) continue;
        const uint32_t at = a.place[t.pb + p];
        if (a.place[t.pb + p + 1] == at) continue;
        uint32_t c[8];
        const SiteCall s = callAt(a, t, (uint32_t) p, c);
        cdm_site *out = a.sites + at;
        out->query = a.firstQuery + t.qi; out->pos = (uint32_t) p; out->info = s.ref | s.major << 4 | s.flags << 8;
#pragma unroll
        for (int k = 0; k < 8; k++) out->counts[k] = c[k];
    }
}

// ---------------------------------------------------------------------------------------------- cdm_pileup_breaks
// Contig break points (include/carpedeam_hip.h): how many counted records SPAN every boundary b of the listed queries with at least
// `anchor` columns on either side, and the runs of boundaries where too few do.  The marks are depth's, in two planes of len + 1 cells
// per listed query laid end to end (depthMarkItem<true>): both planes sum to zero per query, so ONE prefix sum over the 2 x N cells
// turns them into depth[i] and span[i], each at cell i + 1 of its plane.  A tile kernel classifies the boundaries, reduces the query's
// figures and writes a 0/1 word where a run of weak boundaries starts; a prefix sum over those words numbers the runs, and an emission
// kernel fills one record per run.  A run never leaves its query, and a batch holds whole queries.
constexpr int BK_MAX_ANCHOR = 1024, BK_MAX_EDGE = 1048576, BK_MAX_SPAN = 1000000;

struct BreakArgs {
    DepthArgs d;                    // edge: the window's; stats: [nq][8]; track: NULL, or the spans without the closing cells
    uint64_t plane;                 // N = base[nq]: the span plane lies N cells behind the depth plane
    uint32_t anchor, minSpan, minPct, firstQuery;
    uint32_t *place;                // [N + 1], laid out as a plane: 0/1 per run start, after the scan the number of run starts in front
    cdm_break *out;                 // k_break_init, k_break_emit, k_break_flags: [nRuns]
    uint32_t nRuns;
};

// marks: one wave per item (listed query, chunk of its records) of this launch's slice, into both planes
__global__ __launch_bounds__(64 * PU_WAVES) void k_break_marks(BreakArgs a, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    depthMarkItem<true>(a.d, first + local, lane, a.anchor, a.plane);
}

// the item (listed query, tile of DP_TILE boundaries) of a block: the query's scanned cells, depth[i] = dep[i] and span[i] = spn[i]
struct BreakTile { uint32_t qi, len; uint64_t cb, p0; const uint32_t *dep, *spn; };
__device__ __forceinline__ BreakTile breakTile(const BreakArgs &a, uint64_t item) {
    uint32_t lo = 0, hi = a.d.nq;
    while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (a.d.tileOff[mid] <= item) lo = mid; else hi = mid; }
    BreakTile t;
    t.qi = lo; t.len = a.d.meta[a.d.queries[lo]].len; t.cb = a.d.base[lo]; t.p0 = (item - a.d.tileOff[lo]) * DP_TILE;
    t.dep = a.d.cells + t.cb + 1; t.spn = t.dep + a.plane;
    return t;
}
// boundary b lies in the window: edge <= b <= len - edge (edge >= 1: never b = 0; nothing when len < 2 x edge)
__device__ __forceinline__ bool breakWindow(const BreakArgs &a, const BreakTile &t, uint64_t b) { return b >= a.d.edge && b + a.d.edge <= t.len; }
// a window boundary with span s is weak
__device__ __forceinline__ bool breakWeakSpan(const BreakArgs &a, const BreakTile &t, uint32_t b, uint32_t s) {
    if (s < a.minSpan) return true;
    return a.minPct && (unsigned long long) s * 100ull < (unsigned long long) a.minPct * min(t.dep[b - 1], t.dep[b]);
}
__device__ __forceinline__ bool breakWeak(const BreakArgs &a, const BreakTile &t, uint64_t b) { return breakWindow(a, t, b) && breakWeakSpan(a, t, (uint32_t) b, t.spn[b]); }

// classification: one block per item of this launch's slice
__global__ __launch_bounds__(DP_NT) void k_break_classify(BreakArgs a, uint64_t first) {
    __shared__ unsigned long long sRed[DP_NT / 64][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const BreakTile t = breakTile(a, first + blockIdx.x);
    uint32_t *__restrict__ track = a.d.track ? a.d.track + (t.cb - t.qi) : nullptr;
    unsigned long long sum = 0, three = 0;       // three: window, weak, run starts in 16 bits each (at most DP_TILE)
    uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < DP_PER; j++) {
        const uint64_t b = t.p0 + threadIdx.x + (uint64_t) DP_NT * j;
        if (b >= t.len) continue;
        const uint32_t s = t.spn[b];
        if (track) track[b] = s;
        bool start = false;
        if (breakWindow(a, t, b)) {
            const bool weak = breakWeakSpan(a, t, (uint32_t) b, s);
            start = weak && !breakWeak(a, t, b - 1);
            sum += s; mn = min(mn, s);
            three += 1ull | (unsigned long long) weak << 16 | (unsigned long long) start << 32;
        }
        if (a.place) a.place[t.cb + b] = start;
    }
    sum = waveSum64(sum); three = waveSum64(three);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = min(mn, (uint32_t) __shfl_xor((int) mn, o, 64));
    if (lane == 0) { sRed[wave][0] = sum; sRed[wave][1] = three; sRed[wave][2] = mn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long r[2] = {0, 0}, m = 0xFFFFFFFFull;
        for (int w = 0; w < DP_NT / 64; w++) { r[0] += sRed[w][0]; r[1] += sRed[w][1]; m = min(m, sRed[w][2]); }
        unsigned long long *row = a.d.stats + (uint64_t) t.qi * 8;
        if (r[1] & 0xFFFFull) {
            atomicAdd(&row[2], r[1] & 0xFFFFull); atomicMin(&row[6], m);
            if (r[0]) atomicAdd(&row[7], r[0]);
            if ((r[1] >> 16) & 0xFFFFull) atomicAdd(&row[3], (r[1] >> 16) & 0xFFFFull);
            if ((r[1] >> 32) & 0xFFFFull) atomicAdd(&row[4], (r[1] >> 32) & 0xFFFFull);
        }
    }
}

// the records before emission: nothing uncovered, the largest span
__global__ void k_break_init(BreakArgs a) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.nRuns) return;
    cdm_break b = {0u, 0u, 0u, 0xFFFFFFFFu, 0u, 0u, 0u, 0u};
    a.out[r] = b;
}

// emission: the same items on the scanned run starts.  The run of a weak boundary b is the number of run starts up to b, minus 1.
__global__ __launch_bounds__(DP_NT) void k_break_emit(BreakArgs a, uint64_t first) {
    const int lane = threadIdx.x & 63;
    const BreakTile t = breakTile(a, first + blockIdx.x);
#pragma unroll
    for (int j = 0; j < DP_PER; j++) {              // (wave-uniform: the ballots and shuffles below see all 64 lanes)
        const uint64_t b = t.p0 + threadIdx.x + (uint64_t) DP_NT * j;
        uint32_t s = 0, run = 0;
        bool weak = false, more = false;
        if (b < t.len && breakWindow(a, t, b)) { s = t.spn[b]; weak = breakWeakSpan(a, t, (uint32_t) b, s); }
        if (weak) {
            const uint32_t upTo = a.place[t.cb + b + 1];              // (b + 1 <= len: at the most the query's closing word)
            run = upTo - 1u;
            more = breakWeak(a, t, b + 1);
            cdm_break *out = a.out + run;
            if (a.place[t.cb + b] != upTo) { out->query = a.firstQuery + t.qi; out->first = (uint32_t) b; out->depth_left = t.dep[b - 1]; }
            if (!more) { out->last = (uint32_t) b; out->depth_right = t.dep[b]; }
        }
        const uint32_t hole = weak && more && t.dep[b] == 0u;         // position b of first .. last - 1 without a read
        const unsigned long long live = __ballot(weak);
        if (!live) continue;
        const uint32_t run0 = (uint32_t) __shfl((int) run, __ffsll((long long) live) - 1, 64);
        if (!__ballot(weak && run != run0)) {       // the wave's weak lanes share a run (a long gap): one atomic of each kind
            uint32_t mn = weak ? s : 0xFFFFFFFFu;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mn = min(mn, (uint32_t) __shfl_xor((int) mn, o, 64));
            const uint32_t holes = (uint32_t) cdm_wave_sum((int) hole);
            if (lane == 0) { atomicMin(&a.out[run0].min_span, mn); if (holes) atomicAdd(&a.out[run0].uncovered, holes); }
        } else if (weak) {
            atomicMin(&a.out[run].min_span, s);
            if (hole) atomicAdd(&a.out[run].uncovered, 1u);
        }
    }
}

// the last pass: gap or join, and the query's number of joins
__global__ void k_break_flags(BreakArgs a) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.nRuns) return;
    const bool gap = a.out[r].uncovered != 0u;
    a.out[r].flags = gap ? CDM_BREAK_GAP : CDM_BREAK_JOIN;
    if (!gap) atomicAdd(&a.d.stats[(uint64_t) (a.out[r].query - a.firstQuery) * 8 + 5], 1ull);
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

static int cdm_depth_impl(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t nq, const cdm_depth_params *par, uint64_t *stats, uint32_t *depth) {
    hipStream_t s = ctx->stream;
    const uint32_t chunk = pileupChunk(), edge = (uint32_t) par->edge;
    const uint64_t bound = depthCells();
    DevBuf<SeqMeta> meta;
    if (int rc = cdm_build_meta(ctx, db, &meta.p)) return rc;
    DevBuf<uint32_t> dq, dLen; DevBuf<uint64_t> dRecs;
    if (!dq.alloc(nq) || !dLen.alloc(nq) || !dRecs.alloc(nq)) { cdm_set_error("cdm_pileup_depth: out of device memory for %llu queries", (unsigned long long) nq); return CDM_ERR_HIP; }
    std::vector<uint32_t> len(nq); std::vector<uint64_t> recs(nq);
    CDM_HIP(hipMemcpyAsync(dq.p, queries, (size_t) nq * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_depth_sizes, CDM_GRID((nq + 255) / 256, 256), dim3(256), 0, s, (const SeqMeta *) meta.p, (const uint64_t *) alns->off, (const uint32_t *) dq.p, nq, dLen.p, dRecs.p);
    CDM_LAUNCH_CHECK();
    CDM_HIP(hipMemcpyAsync(len.data(), dLen.p, (size_t) nq * 4, hipMemcpyDeviceToHost, s));
    CDM_HIP(hipMemcpyAsync(recs.data(), dRecs.p, (size_t) nq * 8, hipMemcpyDeviceToHost, s));
    CDM_HIP(hipStreamSynchronize(s));
    for (uint64_t i = 0; i < nq; i++)
        if (recs[i] >> 32) { cdm_set_error("cdm_pileup_depth: query %u has %llu records; the 32-bit depth cells hold fewer than 2^32", queries[i], (unsigned long long) recs[i]); return CDM_ERR_UNSUPPORTED; }
    float msTotal = 0.f;
    uint64_t trackAt = 0;
    for (uint64_t b0 = 0; b0 < nq;) {
        // the batch: listed queries while their cells stay within the bound; a single query longer than the bound goes alone
        uint32_t m = 0; uint64_t nCells = 0;
        while (b0 + m < nq && m < (1u << 30) && (m == 0 || nCells + len[b0 + m] + 1ull <= bound)) { nCells += len[b0 + m] + 1ull; m++; }
        std::vector<uint64_t> base((size_t) m + 1), tileOff((size_t) m + 1);
        base[0] = tileOff[0] = 0;
        for (uint32_t i = 0; i < m; i++) { base[i + 1] = base[i] + len[b0 + i] + 1ull; tileOff[i + 1] = tileOff[i] + ((uint64_t) len[b0 + i] + DP_TILE - 1) / DP_TILE; }
        const uint64_t nTiles = tileOff[m], nTrack = nCells - m;
        DevBuf<uint64_t> items, itemOff, dBase, dTile; DevBuf<uint32_t> cells, track; DevBuf<unsigned long long> dStats;
        if (!items.alloc((size_t) m + 1) || !itemOff.alloc((size_t) m + 1) || !dBase.alloc((size_t) m + 1) || !dTile.alloc((size_t) m + 1) || !cells.alloc(nCells) || !dStats.alloc((size_t) m * 8) ||
            (depth && !track.alloc(nTrack))) {
            cdm_set_error("cdm_pileup_depth: out of device memory for the %llu cells of %u queries", (unsigned long long) nCells, m); return CDM_ERR_HIP;
        }
        CDM_HIP(hipMemcpyAsync(dBase.p, base.data(), ((size_t) m + 1) * 8, hipMemcpyHostToDevice, s));
        CDM_HIP(hipMemcpyAsync(dTile.p, tileOff.data(), ((size_t) m + 1) * 8, hipMemcpyHostToDevice, s));
        CDM_HIP(hipMemsetAsync(cells.p, 0, (size_t) nCells * 4, s));
        CDM_HIP(hipMemsetAsync(dStats.p, 0, (size_t) m * 64, s));
        hipLaunchKernelGGL(k_pileup_chunks, dim3((m + 256) / 256), dim3(256), 0, s, (const uint64_t *) alns->off, (const uint32_t *) (dq.p + b0), m, chunk, items.p);
        cdmscan::ScanTemp st, stCells;
        if (int rc = cdmscan::exclusiveScan<uint64_t>(s, st, items.p, itemOff.p, (size_t) m + 1)) return rc;
        uint64_t nItems = 0;
        CDM_HIP(hipMemcpyAsync(&nItems, itemOff.p + m, 8, hipMemcpyDeviceToHost, s));
        CDM_HIP(hipStreamSynchronize(s));
        DepthArgs a;
        a.meta = meta.p; a.aoff = alns->off; a.rec = alns->rec; a.queries = dq.p + b0; a.itemOff = itemOff.p; a.tileOff = dTile.p; a.base = dBase.p;
        a.n = (uint32_t) db->n; a.nq = m; a.chunk = chunk; a.skipExt = par->skip_extended_targets ? 1u : 0u; a.edge = edge; a.minSeqId = par->min_seq_id;
        a.cells = cells.p; a.stats = dStats.p; a.track = depth ? track.p : nullptr;
        hipEventRecord(ctx->ev0, s);
        for (uint64_t first = 0, slice = cdmSliceItems(64); first < nItems; first += slice) {
            const uint64_t nThis = std::min<uint64_t>(slice, nItems - first);
            hipLaunchKernelGGL(k_depth_marks, CDM_GRID((nThis + PU_WAVES - 1) / PU_WAVES, 64 * PU_WAVES), dim3(64 * PU_WAVES), 0, s, a, first, nThis);
        }
        if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stCells, cells.p, cells.p, (size_t) nCells)) return rc;     // (in place: scan.h)
        for (uint64_t first = 0, slice = cdmSliceItems(DP_NT); first < nTiles; first += slice) {
            const uint64_t nThis = std::min<uint64_t>(slice, nTiles - first);
            hipLaunchKernelGGL(k_depth_stats, CDM_GRID(nThis, DP_NT), dim3(DP_NT), 0, s, a, first);
        }
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        CDM_HIP(hipMemcpyAsync(stats + b0 * 8, dStats.p, (size_t) m * 64, hipMemcpyDeviceToHost, s));
        if (depth && nTrack) CDM_HIP(hipMemcpyAsync(depth + trackAt, track.p, (size_t) nTrack * 4, hipMemcpyDeviceToHost, s));
        { hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) { cdm_set_error("cdm_pileup_depth: the kernels failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; } }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) msTotal += ms;
        for (uint32_t i = 0; i < m; i++) {
            uint64_t *row = stats + (b0 + i) * 8;
            const uint64_t L = len[b0 + i];
            row[3] = L > 2ull * edge ? L - 2ull * edge : L;
            // max x sum bounds sumsq from above: where it does not fit 64 bits, sumsq may have wrapped
            if (((unsigned __int128) row[7] * row[5]) >> 64) { cdm_set_error("cdm_pileup_depth: query %u: max depth %llu x depth sum %llu does not fit 64 bits (the bound of sumsq)", queries[b0 + i], (unsigned long long) row[7], (unsigned long long) row[5]); return CDM_ERR_UNSUPPORTED; }
        }
        trackAt += nTrack; b0 += m;
    }
    ctx->lastMs[17] = msTotal;
    return CDM_OK;
}

static int cdm_bases_impl(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t nq, const cdm_bases_params *par, uint64_t *stats, uint32_t *counts,
                          cdm_site **sites, uint64_t *nSitesOut, float *kernelMs) {
    hipStream_t s = ctx->stream;
    const uint32_t chunk = pileupChunk();
    const uint64_t bound = basesPositions();
    DevBuf<SeqMeta> meta;
    if (int rc = cdm_build_meta(ctx, db, &meta.p)) return rc;
    DevBuf<uint32_t> dq, dLen; DevBuf<uint64_t> dRecs;
    if (!dq.alloc(nq) || !dLen.alloc(nq) || !dRecs.alloc(nq)) { cdm_set_error("cdm_pileup_bases: out of device memory for %llu queries", (unsigned long long) nq); return CDM_ERR_HIP; }
    std::vector<uint32_t> len(nq); std::vector<uint64_t> recs(nq);
    CDM_HIP(hipMemcpyAsync(dq.p, queries, (size_t) nq * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_depth_sizes, CDM_GRID((nq + 255) / 256, 256), dim3(256), 0, s, (const SeqMeta *) meta.p, (const uint64_t *) alns->off, (const uint32_t *) dq.p, nq, dLen.p, dRecs.p);
    CDM_LAUNCH_CHECK();
    CDM_HIP(hipMemcpyAsync(len.data(), dLen.p, (size_t) nq * 4, hipMemcpyDeviceToHost, s));
    CDM_HIP(hipMemcpyAsync(recs.data(), dRecs.p, (size_t) nq * 8, hipMemcpyDeviceToHost, s));
    CDM_HIP(hipStreamSynchronize(s));
    for (uint64_t i = 0; i < nq; i++)
        if (recs[i] >> 32) { cdm_set_error("cdm_pileup_bases: query %u has %llu records; the 32-bit counters hold fewer than 2^32", queries[i], (unsigned long long) recs[i]); return CDM_ERR_UNSUPPORTED; }
    float msTotal = 0.f;
    uint64_t countsAt = 0;
    for (uint64_t b0 = 0; b0 < nq;) {
        // the batch: listed queries while their positions stay within the bound; a single query longer than the bound goes alone
        uint32_t m = 0; uint64_t nPos = 0;
        while (b0 + m < nq && m < (1u << 30) && (m == 0 || nPos + len[b0 + m] <= bound)) { nPos += len[b0 + m]; m++; }
        std::vector<uint64_t> base((size_t) m + 1), tileOff((size_t) m + 1);
        base[0] = tileOff[0] = 0;
        for (uint32_t i = 0; i < m; i++) { base[i + 1] = base[i] + len[b0 + i]; tileOff[i + 1] = tileOff[i] + ((uint64_t) len[b0 + i] + DP_TILE - 1) / DP_TILE; }
        const uint64_t nTiles = tileOff[m];
        DevBuf<uint64_t> items, itemOff, dBase, dTile; DevBuf<uint32_t> planes, place, dCounts; DevBuf<unsigned long long> dStats; DevBuf<cdm_site> dSites;
        if (!items.alloc((size_t) m + 1) || !itemOff.alloc((size_t) m + 1) || !dBase.alloc((size_t) m + 1) || !dTile.alloc((size_t) m + 1) || !planes.alloc((size_t) nPos * 8) || !place.alloc((size_t) nPos + 1) ||
            !dStats.alloc((size_t) m * 8) || (counts && !dCounts.alloc((size_t) nPos * 8))) {
            cdm_set_error("cdm_pileup_bases: out of device memory for the counters of %llu positions of %u queries", (unsigned long long) nPos, m); return CDM_ERR_HIP;
        }
        CDM_HIP(hipMemcpyAsync(dBase.p, base.data(), ((size_t) m + 1) * 8, hipMemcpyHostToDevice, s));
        CDM_HIP(hipMemcpyAsync(dTile.p, tileOff.data(), ((size_t) m + 1) * 8, hipMemcpyHostToDevice, s));
        CDM_HIP(hipMemsetAsync(planes.p, 0, (size_t) nPos * 32, s));
        CDM_HIP(hipMemsetAsync(place.p + nPos, 0, 4, s));             // (the closing word: the scan leaves the batch's number of sites there)
        CDM_HIP(hipMemsetAsync(dStats.p, 0, (size_t) m * 64, s));
        hipLaunchKernelGGL(k_pileup_chunks, dim3((m + 256) / 256), dim3(256), 0, s, (const uint64_t *) alns->off, (const uint32_t *) (dq.p + b0), m, chunk, items.p);
        cdmscan::ScanTemp st, stPlace;
        if (int rc = cdmscan::exclusiveScan<uint64_t>(s, st, items.p, itemOff.p, (size_t) m + 1)) return rc;
        uint64_t nItems = 0;
        CDM_HIP(hipMemcpyAsync(&nItems, itemOff.p + m, 8, hipMemcpyDeviceToHost, s));
        CDM_HIP(hipStreamSynchronize(s));
        BasesArgs a;
        a.meta = meta.p; a.codes = db->codes; a.nmask = db->nmask; a.aoff = alns->off; a.rec = alns->rec; a.queries = dq.p + b0; a.itemOff = itemOff.p; a.tileOff = dTile.p; a.base = dBase.p;
        a.n = (uint32_t) db->n; a.nq = m; a.chunk = chunk; a.skipExt = par->skip_extended_targets ? 1u : 0u; a.maskEnds = (uint32_t) par->mask_ends; a.minDepth = (uint32_t) par->min_depth;
        a.minAlt = (uint32_t) par->min_alt_count; a.minPct = (uint32_t) par->min_alt_percent; a.firstQuery = (uint32_t) b0; a.minSeqId = par->min_seq_id;
        a.nPos = nPos; a.planes = planes.p; a.stats = dStats.p; a.place = place.p; a.counts = counts ? dCounts.p : nullptr; a.sites = nullptr;
        hipEventRecord(ctx->ev0, s);
        for (uint64_t first = 0, slice = cdmSliceItems(64); first < nItems; first += slice) {
            const uint64_t nThis = std::min<uint64_t>(slice, nItems - first);
            hipLaunchKernelGGL(k_base_counts, CDM_GRID((nThis + PU_WAVES - 1) / PU_WAVES, 64 * PU_WAVES), dim3(64 * PU_WAVES), 0, s, a, first, nThis);
        }
        for (uint64_t first = 0, slice = cdmSliceItems(DP_NT); first < nTiles; first += slice) {
            const uint64_t nThis = std::min<uint64_t>(slice, nTiles - first);
            hipLaunchKernelGGL(k_base_sites, CDM_GRID(nThis, DP_NT), dim3(DP_NT), 0, s, a, first);
        }
        uint32_t nSites = 0;
        if (sites) {
            if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stPlace, place.p, place.p, (size_t) nPos + 1)) return rc;      // (in place: scan.h)
            CDM_HIP(hipMemcpyAsync(&nSites, place.p + nPos, 4, hipMemcpyDeviceToHost, s));
        }
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        CDM_HIP(hipMemcpyAsync(stats + b0 * 8, dStats.p, (size_t) m * 64, hipMemcpyDeviceToHost, s));
        if (counts && nPos) CDM_HIP(hipMemcpyAsync(counts + countsAt * 8, dCounts.p, (size_t) nPos * 32, hipMemcpyDeviceToHost, s));
        { hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) { cdm_set_error("cdm_pileup_bases: the kernels failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; } }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) msTotal += ms;
        if (nSites) {       // the records of this batch behind those of the batches before it
            if (!dSites.alloc(nSites)) { cdm_set_error("cdm_pileup_bases: out of device memory for %u site records", nSites); return CDM_ERR_HIP; }
            a.sites = dSites.p;
            hipEventRecord(ctx->ev0, s);
            for (uint64_t first = 0, slice = cdmSliceItems(DP_NT); first < nTiles; first += slice) {
                const uint64_t nThis = std::min<uint64_t>(slice, nTiles - first);
                hipLaunchKernelGGL(k_base_emit, CDM_GRID(nThis, DP_NT), dim3(DP_NT), 0, s, a, first);
            }
            hipEventRecord(ctx->ev1, s);
            CDM_LAUNCH_CHECK();
            cdm_site *grown = (cdm_site *) realloc(*sites, (size_t) (*nSitesOut + nSites) * sizeof(cdm_site));
            if (!grown) { cdm_set_error("cdm_pileup_bases: out of host memory for %llu site records", (unsigned long long) (*nSitesOut + nSites)); return CDM_ERR_INVALID; }
            *sites = grown;
            CDM_HIP(hipMemcpyAsync(grown + *nSitesOut, dSites.p, (size_t) nSites * sizeof(cdm_site), hipMemcpyDeviceToHost, s));
            *nSitesOut += nSites;
            { hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) { cdm_set_error("cdm_pileup_bases: the emission failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; } }
            if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) msTotal += ms;
        }
        countsAt += nPos; b0 += m;
    }
    if (kernelMs) *kernelMs = msTotal;
    return CDM_OK;
}

static int cdm_breaks_impl(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t nq, const cdm_breaks_params *par, uint64_t *stats, uint32_t *track,
                           cdm_break **breaks, uint64_t *nBreaksOut, float *kernelMs) {
    hipStream_t s = ctx->stream;
    const uint32_t chunk = pileupChunk();
    const uint64_t bound = depthCells();
    DevBuf<SeqMeta> meta;
    if (int rc = cdm_build_meta(ctx, db, &meta.p)) return rc;
    DevBuf<uint32_t> dq, dLen; DevBuf<uint64_t> dRecs;
    if (!dq.alloc(nq) || !dLen.alloc(nq) || !dRecs.alloc(nq)) { cdm_set_error("cdm_pileup_breaks: out of device memory for %llu queries", (unsigned long long) nq); return CDM_ERR_HIP; }
    std::vector<uint32_t> len(nq); std::vector<uint64_t> recs(nq);
    CDM_HIP(hipMemcpyAsync(dq.p, queries, (size_t) nq * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_depth_sizes, CDM_GRID((nq + 255) / 256, 256), dim3(256), 0, s, (const SeqMeta *) meta.p, (const uint64_t *) alns->off, (const uint32_t *) dq.p, nq, dLen.p, dRecs.p);
    CDM_LAUNCH_CHECK();
    CDM_HIP(hipMemcpyAsync(len.data(), dLen.p, (size_t) nq * 4, hipMemcpyDeviceToHost, s));
    CDM_HIP(hipMemcpyAsync(recs.data(), dRecs.p, (size_t) nq * 8, hipMemcpyDeviceToHost, s));
    CDM_HIP(hipStreamSynchronize(s));
    for (uint64_t i = 0; i < nq; i++)
        if (recs[i] >> 32) { cdm_set_error("cdm_pileup_breaks: query %u has %llu records; the 32-bit cells hold fewer than 2^32", queries[i], (unsigned long long) recs[i]); return CDM_ERR_UNSUPPORTED; }
    float msTotal = 0.f;
    uint64_t trackAt = 0;
    for (uint64_t b0 = 0; b0 < nq;) {
        // the batch: listed queries while the cells of their two planes stay within the bound; a single longer query goes alone
        uint32_t m = 0; uint64_t N = 0;
        while (b0 + m < nq && m < (1u << 30) && (m == 0 || 2ull * (N + len[b0 + m] + 1ull) <= bound)) { N += len[b0 + m] + 1ull; m++; }
        std::vector<uint64_t> base((size_t) m + 1), tileOff((size_t) m + 1), init((size_t) m * 8, 0);
        base[0] = tileOff[0] = 0;
        for (uint32_t i = 0; i < m; i++) { base[i + 1] = base[i] + len[b0 + i] + 1ull; tileOff[i + 1] = tileOff[i] + ((uint64_t) len[b0 + i] + DP_TILE - 1) / DP_TILE; init[(size_t) i * 8 + 6] = ~0ull; }
        const uint64_t nTiles = tileOff[m], nTrack = N - m;
        DevBuf<uint64_t> items, itemOff, dBase, dTile; DevBuf<uint32_t> cells, dTrack, place; DevBuf<unsigned long long> dStats; DevBuf<cdm_break> dBreaks;
        if (!items.alloc((size_t) m + 1) || !itemOff.alloc((size_t) m + 1) || !dBase.alloc((size_t) m + 1) || !dTile.alloc((size_t) m + 1) || !cells.alloc((size_t) N * 2) || !place.alloc((size_t) N + 1) ||
            !dStats.alloc((size_t) m * 8) || (track && !dTrack.alloc(nTrack))) {
            cdm_set_error("cdm_pileup_breaks: out of device memory for the %llu cells of %u queries", (unsigned long long) N * 2, m); return CDM_ERR_HIP;
        }
        CDM_HIP(hipMemcpyAsync(dBase.p, base.data(), ((size_t) m + 1) * 8, hipMemcpyHostToDevice, s));
        CDM_HIP(hipMemcpyAsync(dTile.p, tileOff.data(), ((size_t) m + 1) * 8, hipMemcpyHostToDevice, s));
        CDM_HIP(hipMemcpyAsync(dStats.p, init.data(), (size_t) m * 64, hipMemcpyHostToDevice, s));        // (zeros; min_span all ones)
        CDM_HIP(hipMemsetAsync(cells.p, 0, (size_t) N * 8, s));
        CDM_HIP(hipMemsetAsync(place.p, 0, ((size_t) N + 1) * 4, s));       // (the closing words stay 0; the scan leaves the batch's number of runs in the last)
        hipLaunchKernelGGL(k_pileup_chunks, dim3((m + 256) / 256), dim3(256), 0, s, (const uint64_t *) alns->off, (const uint32_t *) (dq.p + b0), m, chunk, items.p);
        cdmscan::ScanTemp st, stCells, stPlace;
        if (int rc = cdmscan::exclusiveScan<uint64_t>(s, st, items.p, itemOff.p, (size_t) m + 1)) return rc;
        uint64_t nItems = 0;
        CDM_HIP(hipMemcpyAsync(&nItems, itemOff.p + m, 8, hipMemcpyDeviceToHost, s));
        CDM_HIP(hipStreamSynchronize(s));
        BreakArgs a;
        a.d.meta = meta.p; a.d.aoff = alns->off; a.d.rec = alns->rec; a.d.queries = dq.p + b0; a.d.itemOff = itemOff.p; a.d.tileOff = dTile.p; a.d.base = dBase.p;
        a.d.n = (uint32_t) db->n; a.d.nq = m; a.d.chunk = chunk; a.d.skipExt = par->skip_extended_targets ? 1u : 0u; a.d.edge = (uint32_t) par->edge; a.d.minSeqId = par->min_seq_id;
        a.d.cells = cells.p; a.d.stats = dStats.p; a.d.track = track ? dTrack.p : nullptr;
        a.plane = N; a.anchor = (uint32_t) par->anchor; a.minSpan = (uint32_t) par->min_span; a.minPct = (uint32_t) par->min_span_percent; a.firstQuery = (uint32_t) b0;
        a.place = place.p; a.out = nullptr; a.nRuns = 0;
        hipEventRecord(ctx->ev0, s);
        for (uint64_t first = 0, slice = cdmSliceItems(64); first < nItems; first += slice) {
            const uint64_t nThis = std::min<uint64_t>(slice, nItems - first);
            hipLaunchKernelGGL(k_break_marks, CDM_GRID((nThis + PU_WAVES - 1) / PU_WAVES, 64 * PU_WAVES), dim3(64 * PU_WAVES), 0, s, a, first, nThis);
        }
        if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stCells, cells.p, cells.p, (size_t) N * 2)) return rc;      // (in place: scan.h; both planes, each summing to zero)
        for (uint64_t first = 0, slice = cdmSliceItems(DP_NT); first < nTiles; first += slice) {
            const uint64_t nThis = std::min<uint64_t>(slice, nTiles - first);
            hipLaunchKernelGGL(k_break_classify, CDM_GRID(nThis, DP_NT), dim3(DP_NT), 0, s, a, first);
        }
        // The runs are numbered whether or not the caller takes the records: `joins` needs every run's `uncovered`.
        uint32_t nRuns = 0;
        if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stPlace, place.p, place.p, (size_t) N + 1)) return rc;
        CDM_HIP(hipMemcpyAsync(&nRuns, place.p + N, 4, hipMemcpyDeviceToHost, s));
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        { hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) { cdm_set_error("cdm_pileup_breaks: the kernels failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; } }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) msTotal += ms;
        if (nRuns) {
            if (!dBreaks.alloc(nRuns)) { cdm_set_error("cdm_pileup_breaks: out of device memory for %u break records", nRuns); return CDM_ERR_HIP; }
            a.out = dBreaks.p; a.nRuns = nRuns;
            hipEventRecord(ctx->ev0, s);
            hipLaunchKernelGGL(k_break_init, CDM_GRID(((uint64_t) nRuns + 255) / 256, 256), dim3(256), 0, s, a);
            for (uint64_t first = 0, slice = cdmSliceItems(DP_NT); first < nTiles; first += slice) {
                const uint64_t nThis = std::min<uint64_t>(slice, nTiles - first);
                hipLaunchKernelGGL(k_break_emit, CDM_GRID(nThis, DP_NT), dim3(DP_NT), 0, s, a, first);
            }
            hipLaunchKernelGGL(k_break_flags, CDM_GRID(((uint64_t) nRuns + 255) / 256, 256), dim3(256), 0, s, a);
            hipEventRecord(ctx->ev1, s);
            CDM_LAUNCH_CHECK();
            if (breaks) {       // the records of this batch behind those of the batches before it
                cdm_break *grown = (cdm_break *) realloc(*breaks, (size_t) (*nBreaksOut + nRuns) * sizeof(cdm_break));
                if (!grown) { cdm_set_error("cdm_pileup_breaks: out of host memory for %llu break records", (unsigned long long) (*nBreaksOut + nRuns)); return CDM_ERR_INVALID; }
                *breaks = grown;
                CDM_HIP(hipMemcpyAsync(grown + *nBreaksOut, dBreaks.p, (size_t) nRuns * sizeof(cdm_break), hipMemcpyDeviceToHost, s));
                *nBreaksOut += nRuns;
            }
        }
        CDM_HIP(hipMemcpyAsync(stats + b0 * 8, dStats.p, (size_t) m * 64, hipMemcpyDeviceToHost, s));
        if (track && nTrack) CDM_HIP(hipMemcpyAsync(track + trackAt, dTrack.p, (size_t) nTrack * 4, hipMemcpyDeviceToHost, s));
        { hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) { cdm_set_error("cdm_pileup_breaks: the emission failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; } }
        if (nRuns && hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) msTotal += ms;
        for (uint32_t i = 0; i < m; i++) { uint64_t *row = stats + (b0 + i) * 8; if (row[2] == 0) row[6] = 0; }       // (an empty window has no smallest span)
        trackAt += nTrack; b0 += m;
    }
    if (kernelMs) *kernelMs = msTotal;
    return CDM_OK;
}

// the argument checks the entry points share
static int pileupCheckArgs(const char *who, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries) {
    if (alns->n != db->n) { cdm_set_error("%s: alignment CSR has %llu queries, DB has %llu", who, (unsigned long long) alns->n, (unsigned long long) db->n); return CDM_ERR_INVALID; }
    if (db->residues && !db->codes) { cdm_set_error("%s: the DB holds no letters (an index copy)", who); return CDM_ERR_INVALID; }
    std::vector<uint32_t> sorted(queries, queries + n_queries);
    std::sort(sorted.begin(), sorted.end());
    if (n_queries && sorted.back() >= db->n) { cdm_set_error("%s: query index %u of a DB of %llu sequences", who, sorted.back(), (unsigned long long) db->n); return CDM_ERR_INVALID; }
    for (uint64_t i = 1; i < n_queries; i++)
        if (sorted[i] == sorted[i - 1]) { cdm_set_error("%s: query index %u is listed twice", who, sorted[i]); return CDM_ERR_INVALID; }
    return CDM_OK;
}

extern "C" int cdm_pileup_depth(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_depth_params *par,
                                uint64_t *stats, uint32_t *depth) {
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, "cdm_pileup_depth");
    if (!ctx || !db || !alns || !par || (n_queries && (!queries || !stats))) { cdm_set_error("cdm_pileup_depth: NULL argument"); return CDM_ERR_INVALID; }
    if (par->edge < 0) { cdm_set_error("cdm_pileup_depth: edge = %d; the positions left out at either end of a contig are 0 or more", par->edge); return CDM_ERR_INVALID; }
    if (int rc = pileupCheckArgs("cdm_pileup_depth", db, alns, queries, n_queries)) return rc;
    if (n_queries == 0) return CDM_OK;
    CDM_HIP(hipSetDevice(ctx->device));
    return cdm_depth_impl(ctx, db, alns, queries, n_queries, par, stats, depth);
}

extern "C" int cdm_pileup_bases(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_bases_params *par,
                                uint64_t *stats, uint32_t *counts, cdm_site **sites, uint64_t *n_sites, float *kernel_ms) {
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, "cdm_pileup_bases");
    if (!ctx || !db || !alns || !par || (sites && !n_sites) || (n_queries && (!queries || !stats))) { cdm_set_error("cdm_pileup_bases: NULL argument"); return CDM_ERR_INVALID; }
    if (par->mask_ends < 0 || par->mask_ends > BS_MAX_MASK) { cdm_set_error("cdm_pileup_bases: mask_ends = %d; 0 to %d positions are left out at either end of a read", par->mask_ends, BS_MAX_MASK); return CDM_ERR_INVALID; }
    if (par->min_depth < 1) { cdm_set_error("cdm_pileup_bases: min_depth = %d; a called position has at least one base", par->min_depth); return CDM_ERR_INVALID; }
    if (par->min_alt_count < 1) { cdm_set_error("cdm_pileup_bases: min_alt_count = %d; a second allele has at least one base", par->min_alt_count); return CDM_ERR_INVALID; }
    if (par->min_alt_percent < 0 || par->min_alt_percent > 100) { cdm_set_error("cdm_pileup_bases: min_alt_percent = %d; a percentage of the depth is 0 to 100", par->min_alt_percent); return CDM_ERR_INVALID; }
    if (int rc = pileupCheckArgs("cdm_pileup_bases", db, alns, queries, n_queries)) return rc;
    if (sites) { *sites = NULL; *n_sites = 0; }
    if (kernel_ms) *kernel_ms = 0.f;
    if (n_queries == 0) return CDM_OK;
    CDM_HIP(hipSetDevice(ctx->device));
    cdm_site *got = NULL; uint64_t nGot = 0;
    const int rc = cdm_bases_impl(ctx, db, alns, queries, n_queries, par, stats, counts, sites ? &got : NULL, &nGot, kernel_ms);
    if (rc != CDM_OK) { free(got); return rc; }
    if (sites) { *sites = got; *n_sites = nGot; }
    return CDM_OK;
}

extern "C" void cdm_sites_free(cdm_site *sites) { free(sites); }

extern "C" int cdm_pileup_breaks(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_breaks_params *par,
                                 uint64_t *stats, uint32_t *track, cdm_break **breaks, uint64_t *n_breaks, float *kernel_ms) {
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, "cdm_pileup_breaks");
    if (!ctx || !db || !alns || !par || (breaks && !n_breaks) || (n_queries && (!queries || !stats))) { cdm_set_error("cdm_pileup_breaks: NULL argument"); return CDM_ERR_INVALID; }
    if (par->anchor < 1 || par->anchor > BK_MAX_ANCHOR) { cdm_set_error("cdm_pileup_breaks: anchor = %d; a spanning read has 1 to %d columns on either side of a boundary", par->anchor, BK_MAX_ANCHOR); return CDM_ERR_INVALID; }
    if (par->edge < par->anchor || par->edge > BK_MAX_EDGE) { cdm_set_error("cdm_pileup_breaks: edge = %d; anchor (%d) to %d boundaries are left out at either end of a query", par->edge, par->anchor, BK_MAX_EDGE); return CDM_ERR_INVALID; }
    if (par->min_span < 1 || par->min_span > BK_MAX_SPAN) { cdm_set_error("cdm_pileup_breaks: min_span = %d; a boundary is held by 1 to %d spanning reads", par->min_span, BK_MAX_SPAN); return CDM_ERR_INVALID; }
    if (par->min_span_percent < 0 || par->min_span_percent > 100) { cdm_set_error("cdm_pileup_breaks: min_span_percent = %d; a percentage of the depth is 0 to 100", par->min_span_percent); return CDM_ERR_INVALID; }
    if (int rc = pileupCheckArgs("cdm_pileup_breaks", db, alns, queries, n_queries)) return rc;
    if (breaks) { *breaks = NULL; *n_breaks = 0; }
    if (kernel_ms) *kernel_ms = 0.f;
    if (n_queries == 0) return CDM_OK;
    CDM_HIP(hipSetDevice(ctx->device));
    cdm_break *got = NULL; uint64_t nGot = 0;
    const int rc = cdm_breaks_impl(ctx, db, alns, queries, n_queries, par, stats, track, breaks ? &got : NULL, &nGot, kernel_ms);
    if (rc != CDM_OK) { free(got); return rc; }
    if (breaks) { *breaks = got; *n_breaks = nGot; }
    return CDM_OK;
}

extern "C" void cdm_breaks_free(cdm_break *breaks) { free(breaks); }

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
