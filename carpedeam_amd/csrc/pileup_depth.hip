// Depth at every position of the listed queries with its statistics (cdm_pileup_depth) and, behind it, the contig break points from
// spanning reads (cdm_pileup_breaks), which marks the same cells; neither is a module of the reference.  What they share with the
// other reductions over the read pile-up is in pileup.h.
//
// Depth (include/carpedeam_hip.h).  k_pileup (pileup.hip) touches at most 2 x ends columns of a record; depth touches all of them,
// so the records are not walked column by column: a counted record MARKS its two ends in a 32-bit cell array (+1 at qs, -1 behind
// qe; len + 1 cells per listed query, the last one its closing cell), every query's cells sum to zero, and ONE device-wide prefix
// sum over the batch's cells turns the marks into depths - no segmented scan.  A third kernel walks the positions in tiles and
// reduces the statistics.  The cells live modulo 2^32: a depth is below the query's record count, and a query with 2^32 records or
// more is refused.  cdm_pileup_depth_gapped and cdm_pileup_breaks_gapped are the same two host sequences with the caller's gapped
// records (cdm_pileup_gapped's) marked into the same cells by a kernel of their own, depthMarkGapped.
#include "pileup.h"

namespace {

constexpr uint64_t DP_CELLS_DEFAULT = 1ull << 28, DP_CELLS_MAX = 1ull << 32;

// CDM_DEPTH_CELLS=<cells> (tests): small inputs in several batches
uint64_t depthCells() { return envCount("CDM_DEPTH_CELLS", DP_CELLS_DEFAULT, DP_CELLS_MAX); }

struct DepthArgs : TiledArgs {      // (items: marking; tiles: statistics)
    uint32_t edge;
    uint32_t *cells;                // [base[nq]]
    unsigned long long *stats;      // [nq][8]
    uint32_t *track;                // NULL, or [base[nq] - nq]: the depths without the closing cells
    const cdm_gap_rec *grec;        // the *_gapped calls: the batch's gapped records [nG] (query: the index into the call's list)
    const uint32_t *gops;           // the caller's whole operation pool
    uint32_t nG, firstQuery;        // firstQuery: the batch's first listed query
};
// The marks of one item (listed query, chunk of its records) by one wave, lanes take records: +1 at qs and -1 behind qe in the depth
// cells; with SPAN (cdm_pileup_breaks, below) also +1 at qs + w and -1 at qe + 2 - w in a second plane of the same
// layout `plane` cells behind the first, for the records of at least 2 w columns.  reads and columns go to the query's stats row, once
// per item.
template <bool SPAN>
__device__ __forceinline__ void depthMarkItem(const DepthArgs &a, uint64_t item, int lane, uint32_t w, uint64_t plane) {
    const ItemRecords it = itemRecords(a, item);
    const uint32_t qi = it.qi, q = it.q, qLen = a.meta[q].len;
    uint32_t *cell = a.cells + a.base[qi];
    unsigned int nReads = 0; unsigned long long nCols = 0;
    for (uint64_t r = it.r0 + lane; r < it.r1; r += 64) {
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
    addReadsColumns(&a.stats[(uint64_t) qi * 8], &a.stats[(uint64_t) qi * 8 + 1], nReads, nCols, lane);
}

// marks: one wave per item of this launch's slice
__global__ __launch_bounds__(64 * PU_WAVES) void k_depth_marks(DepthArgs a, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    depthMarkItem<false>(a, first + local, lane, 0u, 0ull);
}

// The marks of the gapped records (cdm_pileup_depth_gapped, cdm_pileup_breaks_gapped; include/carpedeam_hip.h), a thread per record
// into the cells the ungapped marks use, in front of the one prefix sum: +1 at p and -1 at p + g for every M operation of g letters at
// query position p - a deleted letter gets no depth.  With SPAN one mark pair in the span plane: with C M columns on the query
// positions m_1 < .. < m_C, a record of C >= 2 w spans the boundaries m_w + 1 .. m_(C - w + 1), found in a second walk (the words are
// few and stay in cache).  reads and columns (C) go to the query's stats row, one atomic of each per wave where its lanes share a
// query - the records are sorted by query.  indelCheckRecords (pileup.h): pos + span <= the query's length, so every cell lies inside
// the query's, the closing cell included.
template <bool SPAN>
__device__ __forceinline__ void depthMarkGapped(const DepthArgs &a, uint64_t i, int lane, uint32_t w, uint64_t plane) {
    const bool live = i < a.nG;
    uint32_t qi = 0, C = 0;
    if (live) {
        const cdm_gap_rec r = a.grec[i];
        qi = r.query - a.firstQuery;
        uint32_t *cell = a.cells + a.base[qi];
        gappedWalk(r, a.gops, [&](uint32_t p, uint32_t, uint32_t g) {
            C += g;
            atomicAdd(&cell[p], 1u);                            // (results unused: atomics without return)
            atomicAdd(&cell[p + g], 0xFFFFFFFFu);
        }, [](uint32_t, uint32_t, uint32_t, uint32_t) {});
        if (SPAN && C >= 2u * w) {
            // the w-th and the (C - w + 1)-th M column, counted from 1: column k lies in the M operation that holds the columns
            // seen + 1 .. seen + g
            const uint32_t kLo = w, kHi = C - w + 1u;
            uint32_t seen = 0, mLo = 0, mHi = 0;
            gappedWalk(r, a.gops, [&](uint32_t p, uint32_t, uint32_t g) {
                if (kLo > seen && kLo <= seen + g) mLo = p + (kLo - seen - 1u);
                if (kHi > seen && kHi <= seen + g) mHi = p + (kHi - seen - 1u);
                seen += g;
            }, [](uint32_t, uint32_t, uint32_t, uint32_t) {});
            atomicAdd(&cell[plane + mLo + 1u], 1u);             // mLo < mHi + 1 <= pos + span <= the query's length
            atomicAdd(&cell[plane + mHi + 1u], 0xFFFFFFFFu);
        }
    }
    const unsigned long long all = __ballot(live);
    if (!all) return;
    const int head = __ffsll((long long) all) - 1;
    const uint32_t qi0 = (uint32_t) __shfl((int) qi, head, 64);
    if (!__ballot(live && qi != qi0)) addReadsColumns(&a.stats[(uint64_t) qi0 * 8], &a.stats[(uint64_t) qi0 * 8 + 1], live ? 1u : 0u, live ? C : 0ull, lane);
    else if (live) { atomicAdd(&a.stats[(uint64_t) qi * 8], 1ull); atomicAdd(&a.stats[(uint64_t) qi * 8 + 1], (unsigned long long) C); }
}
__global__ __launch_bounds__(DP_NT) void k_depth_gapped(DepthArgs a, uint64_t first) {
    depthMarkGapped<false>(a, (first + blockIdx.x) * DP_NT + threadIdx.x, threadIdx.x & 63, 0u, 0ull);
}

// statistics: one block per item (listed query, tile of DP_TILE positions) of this launch's slice, on the scanned cells:
// depth[p] = the exclusive prefix at cell p + 1
__global__ __launch_bounds__(DP_NT) void k_depth_stats(DepthArgs a, uint64_t first) {
    __shared__ unsigned long long sRed[DP_NT / 64][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Tile t = tileOf(a, first + blockIdx.x);
    const uint32_t qi = t.qi, len = t.len;
    const uint64_t cb = t.base, p0 = t.p0;
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
// and the marks of the gapped records, a thread per record, into both planes
__global__ __launch_bounds__(DP_NT) void k_break_gapped(BreakArgs a, uint64_t first) {
    depthMarkGapped<true>(a.d, (first + blockIdx.x) * DP_NT + threadIdx.x, threadIdx.x & 63, a.anchor, a.plane);
}

// the item (listed query, tile of DP_TILE boundaries) of a block with the query's scanned cells: depth[i] = dep[i] and span[i] = spn[i]
struct BreakTile : Tile { const uint32_t *dep, *spn; };
__device__ __forceinline__ BreakTile breakTile(const BreakArgs &a, uint64_t item) {
    BreakTile t;
    static_cast<Tile &>(t) = tileOf(a.d, item);
    t.dep = a.d.cells + t.base + 1; t.spn = t.dep + a.plane;
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
    uint32_t *__restrict__ track = a.d.track ? a.d.track + (t.base - t.qi) : nullptr;
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
        if (a.place) a.place[t.base + b] = start;
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
            const uint32_t upTo = a.place[t.base + b + 1];              // (b + 1 <= len: at the most the query's closing word)
            run = upTo - 1u;
            more = breakWeak(a, t, b + 1);
            cdm_break *out = a.out + run;
            if (a.place[t.base + b] != upTo) { out->query = a.firstQuery + t.qi; out->first = (uint32_t) b; out->depth_left = t.dep[b - 1]; }
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

// the gapped records of the batch [b0, b0 + m) into the kernel arguments: the range [g0, g1) of the sorted records; -> g1
static uint64_t depthGappedRange(DepthArgs &a, const GappedRecords &gr, uint64_t g0, uint64_t b0, uint32_t m) {
    const uint64_t g1 = gr.end(g0, b0 + m);
    a.grec = gr.dRecs.p ? gr.dRecs.p + g0 : nullptr; a.gops = gr.dOps.p; a.nG = (uint32_t) (g1 - g0); a.firstQuery = (uint32_t) b0;        // (fewer than 2^31 operation words: fewer records)
    return g1;
}

// The host sequence of cdm_pileup_depth (who; gr without records) and of cdm_pileup_depth_gapped (gr: the caller's gapped records,
// checked before anything goes to the device).
static int cdm_depth_impl(cdm_ctx *ctx, const char *who, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t nq, GappedRecords &gr, const cdm_depth_params *par,
                          uint64_t *stats, uint32_t *depth, float *kernelMs) {
    hipStream_t s = ctx->stream;
    const uint32_t chunk = pileupChunk(), edge = (uint32_t) par->edge;
    const uint64_t bound = depthCells();
    if (int rc = gr.check(who, db, queries, nq)) return rc;
    QuerySizes qs;
    if (int rc = querySizes(ctx, db, alns, queries, nq, who, "depth cells", qs)) return rc;
    if (int rc = gr.checkCounts(who, "depth cells", queries, qs.recs)) return rc;
    if (int rc = gr.upload(s, who)) return rc;
    float msTotal = 0.f; uint64_t trackAt = 0, g0 = 0;
    for (uint64_t b0 = 0; b0 < nq;) {
        // the batch: listed queries while their cells stay within the bound; a single query longer than the bound goes alone
        BatchPlan plan; WorkItems work; cdmscan::ScanTemp stCells;
        plan.cut(qs.len, b0, 1u, [](uint64_t len) { return len + 1ull; }, bound);
        const uint32_t m = plan.m; const uint64_t nCells = plan.cells, nTrack = nCells - m;
        DevBuf<uint32_t> cells, track; DevBuf<unsigned long long> dStats;
        if (!work.alloc(m) || !plan.alloc() || !cells.alloc(nCells) || !dStats.alloc((size_t) m * 8) || (depth && !track.alloc(nTrack))) {
            cdm_set_error("%s: out of device memory for the %llu cells of %u queries", who, (unsigned long long) nCells, m); return CDM_ERR_HIP;
        }
        if (int rc = plan.upload(s)) return rc;
        CDM_HIP(hipMemsetAsync(cells.p, 0, (size_t) nCells * 4, s));
        CDM_HIP(hipMemsetAsync(dStats.p, 0, (size_t) m * 64, s));
        if (int rc = workItems(s, alns, qs.dq.p + b0, m, chunk, work)) return rc;
        DepthArgs a;
        fillArgs(a, qs.meta.p, db, alns, par->min_seq_id, par->skip_extended_targets, work, plan);
        a.edge = edge; a.cells = cells.p; a.stats = dStats.p; a.track = depth ? track.p : nullptr;
        g0 = depthGappedRange(a, gr, g0, b0, m);
        hipEventRecord(ctx->ev0, s);
        launchWaveItems(s, k_depth_marks, a, work.n);
        launchTiles(s, k_depth_gapped, a, ((uint64_t) a.nG + DP_NT - 1) / DP_NT);
        if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stCells, cells.p, cells.p, (size_t) nCells)) return rc;     // (in place: scan.h)
        launchTiles(s, k_depth_stats, a, plan.nTiles);
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        CDM_HIP(hipMemcpyAsync(stats + b0 * 8, dStats.p, (size_t) m * 64, hipMemcpyDeviceToHost, s));
        if (depth && nTrack) CDM_HIP(hipMemcpyAsync(depth + trackAt, track.p, (size_t) nTrack * 4, hipMemcpyDeviceToHost, s));
        if (int rc = finishTimed(ctx, who, "kernels", msTotal)) return rc;
        for (uint32_t i = 0; i < m; i++) {
            uint64_t *row = stats + (b0 + i) * 8;
            const uint64_t L = qs.len[b0 + i];
            row[3] = L > 2ull * edge ? L - 2ull * edge : L;
            // max x sum bounds sumsq from above: where it does not fit 64 bits, sumsq may have wrapped
            if (((unsigned __int128) row[7] * row[5]) >> 64) { cdm_set_error("%s: query %u: max depth %llu x depth sum %llu does not fit 64 bits (the bound of sumsq)", who, queries[b0 + i], (unsigned long long) row[7], (unsigned long long) row[5]); return CDM_ERR_UNSUPPORTED; }
        }
        trackAt += nTrack; b0 += m;
    }
    ctx->lastMs[17] = msTotal;
    if (kernelMs) *kernelMs = msTotal;
    return CDM_OK;
}

// The host sequence of cdm_pileup_breaks (who; gr without records) and of cdm_pileup_breaks_gapped (gr: the caller's gapped records,
// checked before anything goes to the device).
static int cdm_breaks_impl(cdm_ctx *ctx, const char *who, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t nq, GappedRecords &gr, const cdm_breaks_params *par,
                           uint64_t *stats, uint32_t *track, cdm_break **breaks, uint64_t *nBreaksOut, float *kernelMs) {
    hipStream_t s = ctx->stream;
    const uint32_t chunk = pileupChunk();
    const uint64_t bound = depthCells();
    if (int rc = gr.check(who, db, queries, nq)) return rc;
    QuerySizes qs;
    if (int rc = querySizes(ctx, db, alns, queries, nq, who, "cells", qs)) return rc;
    if (int rc = gr.checkCounts(who, "cells", queries, qs.recs)) return rc;
    if (int rc = gr.upload(s, who)) return rc;
    float msTotal = 0.f; uint64_t trackAt = 0, g0 = 0;
    for (uint64_t b0 = 0; b0 < nq;) {
        // the batch: listed queries while the cells of their two planes stay within the bound; a single longer query goes alone
        BatchPlan plan; WorkItems work; cdmscan::ScanTemp stCells, stPlace;
        plan.cut(qs.len, b0, 1u, [](uint64_t len) { return 2ull * (len + 1ull); }, bound);
        const uint32_t m = plan.m; const uint64_t N = plan.cells, nTiles = plan.nTiles, nTrack = N - m;
        std::vector<uint64_t> init((size_t) m * 8, 0);
        for (uint32_t i = 0; i < m; i++) init[(size_t) i * 8 + 6] = ~0ull;
        DevBuf<uint32_t> cells, dTrack, place; DevBuf<unsigned long long> dStats; DevBuf<cdm_break> dBreaks;
        if (!work.alloc(m) || !plan.alloc() || !cells.alloc((size_t) N * 2) || !place.alloc((size_t) N + 1) || !dStats.alloc((size_t) m * 8) || (track && !dTrack.alloc(nTrack))) {
            cdm_set_error("%s: out of device memory for the %llu cells of %u queries", who, (unsigned long long) N * 2, m); return CDM_ERR_HIP;
        }
        if (int rc = plan.upload(s)) return rc;
        CDM_HIP(hipMemcpyAsync(dStats.p, init.data(), (size_t) m * 64, hipMemcpyHostToDevice, s));        // (zeros; min_span all ones)
        CDM_HIP(hipMemsetAsync(cells.p, 0, (size_t) N * 8, s));
        CDM_HIP(hipMemsetAsync(place.p, 0, ((size_t) N + 1) * 4, s));       // (the closing words stay 0; the scan leaves the batch's number of runs in the last)
        if (int rc = workItems(s, alns, qs.dq.p + b0, m, chunk, work)) return rc;
        BreakArgs a;
        fillArgs(a.d, qs.meta.p, db, alns, par->min_seq_id, par->skip_extended_targets, work, plan);
        a.d.edge = (uint32_t) par->edge; a.d.cells = cells.p; a.d.stats = dStats.p; a.d.track = track ? dTrack.p : nullptr;
        a.plane = N; a.anchor = (uint32_t) par->anchor; a.minSpan = (uint32_t) par->min_span; a.minPct = (uint32_t) par->min_span_percent; a.firstQuery = (uint32_t) b0;
        a.place = place.p; a.out = nullptr; a.nRuns = 0;
        g0 = depthGappedRange(a.d, gr, g0, b0, m);
        hipEventRecord(ctx->ev0, s);
        launchWaveItems(s, k_break_marks, a, work.n);
        launchTiles(s, k_break_gapped, a, ((uint64_t) a.d.nG + DP_NT - 1) / DP_NT);
        if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stCells, cells.p, cells.p, (size_t) N * 2)) return rc;      // (in place: scan.h; both planes, each summing to zero)
        launchTiles(s, k_break_classify, a, nTiles);
        // The runs are numbered whether or not the caller takes the records: `joins` needs every run's `uncovered`.
        uint32_t nRuns = 0;
        if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stPlace, place.p, place.p, (size_t) N + 1)) return rc;
        CDM_HIP(hipMemcpyAsync(&nRuns, place.p + N, 4, hipMemcpyDeviceToHost, s));
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        if (int rc = finishTimed(ctx, who, "kernels", msTotal)) return rc;
        if (nRuns) {
            if (!dBreaks.alloc(nRuns)) { cdm_set_error("%s: out of device memory for %u break records", who, nRuns); return CDM_ERR_HIP; }
            a.out = dBreaks.p; a.nRuns = nRuns;
            hipEventRecord(ctx->ev0, s);
            hipLaunchKernelGGL(k_break_init, CDM_GRID(((uint64_t) nRuns + 255) / 256, 256), dim3(256), 0, s, a);
            launchTiles(s, k_break_emit, a, nTiles);
            hipLaunchKernelGGL(k_break_flags, CDM_GRID(((uint64_t) nRuns + 255) / 256, 256), dim3(256), 0, s, a);
            hipEventRecord(ctx->ev1, s);
            CDM_LAUNCH_CHECK();
            // the records of this batch behind those of the batches before it
            if (breaks) { if (int rc = appendRecords(s, who, "break", breaks, nBreaksOut, (const cdm_break *) dBreaks.p, nRuns)) return rc; }
        }
        CDM_HIP(hipMemcpyAsync(stats + b0 * 8, dStats.p, (size_t) m * 64, hipMemcpyDeviceToHost, s));
        if (track && nTrack) CDM_HIP(hipMemcpyAsync(track + trackAt, dTrack.p, (size_t) nTrack * 4, hipMemcpyDeviceToHost, s));
        if (int rc = finishTimed(ctx, who, "emission", msTotal, nRuns != 0)) return rc;
        for (uint32_t i = 0; i < m; i++) { uint64_t *row = stats + (b0 + i) * 8; if (row[2] == 0) row[6] = 0; }       // (an empty window has no smallest span)
        trackAt += nTrack; b0 += m;
    }
    if (kernelMs) *kernelMs = msTotal;
    return CDM_OK;
}

// the checks of the two depth entry points, and of the two break point entry points
static int depthCheck(const char *who, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_depth_params *par) {
    if (par->edge < 0) { cdm_set_error("%s: edge = %d; the positions left out at either end of a contig are 0 or more", who, par->edge); return CDM_ERR_INVALID; }
    return pileupCheckArgs(who, db, alns, queries, n_queries);
}
static int breaksCheck(const char *who, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_breaks_params *par) {
    if (par->anchor < 1 || par->anchor > BK_MAX_ANCHOR) { cdm_set_error("%s: anchor = %d; a spanning read has 1 to %d columns on either side of a boundary", who, par->anchor, BK_MAX_ANCHOR); return CDM_ERR_INVALID; }
    if (par->edge < par->anchor || par->edge > BK_MAX_EDGE) { cdm_set_error("%s: edge = %d; anchor (%d) to %d boundaries are left out at either end of a query", who, par->edge, par->anchor, BK_MAX_EDGE); return CDM_ERR_INVALID; }
    if (par->min_span < 1 || par->min_span > BK_MAX_SPAN) { cdm_set_error("%s: min_span = %d; a boundary is held by 1 to %d spanning reads", who, par->min_span, BK_MAX_SPAN); return CDM_ERR_INVALID; }
    if (par->min_span_percent < 0 || par->min_span_percent > 100) { cdm_set_error("%s: min_span_percent = %d; a percentage of the depth is 0 to 100", who, par->min_span_percent); return CDM_ERR_INVALID; }
    return pileupCheckArgs(who, db, alns, queries, n_queries);
}

extern "C" int cdm_pileup_depth(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_depth_params *par,
                                uint64_t *stats, uint32_t *depth) {
    static const char *const WHO = "cdm_pileup_depth";
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, WHO);
    if (!ctx || !db || !alns || !par || (n_queries && (!queries || !stats))) { cdm_set_error("%s: NULL argument", WHO); return CDM_ERR_INVALID; }
    if (int rc = depthCheck(WHO, db, alns, queries, n_queries, par)) return rc;
    if (n_queries == 0) return CDM_OK;
    CDM_HIP(hipSetDevice(ctx->device));
    GappedRecords none;
    return cdm_depth_impl(ctx, WHO, db, alns, queries, n_queries, none, par, stats, depth, NULL);
}

extern "C" int cdm_pileup_depth_gapped(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_gap_rec *recs, uint64_t n_recs,
                                       const uint32_t *ops, uint64_t n_ops, const cdm_depth_params *par, uint64_t *stats, uint32_t *depth, float *kernel_ms) {
    static const char *const WHO = "cdm_pileup_depth_gapped";
    if (kernel_ms) *kernel_ms = 0.f;
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, WHO);
    if (!ctx || !db || !alns || !par || (n_recs && (!recs || !ops)) || (n_queries && (!queries || !stats))) { cdm_set_error("%s: NULL argument", WHO); return CDM_ERR_INVALID; }
    if (int rc = depthCheck(WHO, db, alns, queries, n_queries, par)) return rc;
    if (n_ops >> 31) { cdm_set_error("%s: %llu operation words; the 32-bit record slots hold fewer than 2^31", WHO, (unsigned long long) n_ops); return CDM_ERR_UNSUPPORTED; }
    if (n_queries == 0) return CDM_OK;
    CDM_HIP(hipSetDevice(ctx->device));
    GappedRecords gr; gr.recs = recs; gr.nRecs = n_recs; gr.ops = ops; gr.nOps = n_ops;
    return cdm_depth_impl(ctx, WHO, db, alns, queries, n_queries, gr, par, stats, depth, kernel_ms);
}

extern "C" int cdm_pileup_breaks(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_breaks_params *par,
                                 uint64_t *stats, uint32_t *track, cdm_break **breaks, uint64_t *n_breaks, float *kernel_ms) {
    static const char *const WHO = "cdm_pileup_breaks";
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, WHO);
    if (!ctx || !db || !alns || !par || (breaks && !n_breaks) || (n_queries && (!queries || !stats))) { cdm_set_error("%s: NULL argument", WHO); return CDM_ERR_INVALID; }
    if (int rc = breaksCheck(WHO, db, alns, queries, n_queries, par)) return rc;
    GappedRecords none;
    return runWithRecords(ctx, n_queries, breaks, n_breaks, kernel_ms, [&](cdm_break **got, uint64_t *nGot, float *ms) {
        return cdm_breaks_impl(ctx, WHO, db, alns, queries, n_queries, none, par, stats, track, got, nGot, ms);
    });
}

extern "C" int cdm_pileup_breaks_gapped(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_gap_rec *recs, uint64_t n_recs,
                                        const uint32_t *ops, uint64_t n_ops, const cdm_breaks_params *par, uint64_t *stats, uint32_t *track, cdm_break **breaks, uint64_t *n_breaks,
                                        float *kernel_ms) {
    static const char *const WHO = "cdm_pileup_breaks_gapped";
    if (kernel_ms) *kernel_ms = 0.f;
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, WHO);
    if (!ctx || !db || !alns || !par || (n_recs && (!recs || !ops)) || (breaks && !n_breaks) || (n_queries && (!queries || !stats))) { cdm_set_error("%s: NULL argument", WHO); return CDM_ERR_INVALID; }
    if (int rc = breaksCheck(WHO, db, alns, queries, n_queries, par)) return rc;
    if (n_ops >> 31) { cdm_set_error("%s: %llu operation words; the 32-bit record slots hold fewer than 2^31", WHO, (unsigned long long) n_ops); return CDM_ERR_UNSUPPORTED; }
    GappedRecords gr; gr.recs = recs; gr.nRecs = n_recs; gr.ops = ops; gr.nOps = n_ops;
    return runWithRecords(ctx, n_queries, breaks, n_breaks, kernel_ms, [&](cdm_break **got, uint64_t *nGot, float *ms) {
        return cdm_breaks_impl(ctx, WHO, db, alns, queries, n_queries, gr, par, stats, track, got, nGot, ms);
    });
}

extern "C" void cdm_breaks_free(cdm_break *breaks) { free(breaks); }
