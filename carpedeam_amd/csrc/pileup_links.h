// The end-record stage that cdm_pileup_links (pileup_links.hip) and cdm_pileup_junctions (pileup_junctions.hip) share: which counted
// records are END RECORDS (the rule: include/carpedeam_hip.h), the end records of all batches in one array sorted by read, and every
// read's run of places in it.  Like cdm_alns_dedup the batch cut is by RECORDS, and the end records of ALL batches go into one array,
// because a read's records lie in the rows of several queries.
//
//   per batch (consecutive listed queries whose record counts sum to at most the bound):
//   k_ln_count     one wave per work item, lanes over records: reads, columns, left, right and both ends per query, end records per item
//   scan           every item's first slot in the batch; the batches' totals add up to every batch's first slot
//   over all batches, once the number of end records is known:
//   k_ln_emit      the same walk again per batch: slots by wave ballot and prefix rank; per slot the key = the read and the value
//                  list index << 24 | tail << 23 | reverse << 22 | h
//   sort           by read, on the bits in use (radix.h): a run of equal keys is a read
//   k_ln_read_heads, scan, k_ln_read_starts      the run of every place and every run's first place
// What walks the runs (the pairs of a read: every tail record x every head record on another list index) is the callers' own.
#pragma once
#include <memory>

#include "pileup.h"
#include "radix.h"

namespace {

constexpr uint64_t LN_BATCH_DEFAULT = 1ull << 26;       // records per batch, cdm_alns_dedup's bound
constexpr int LN_LEN_BITS = 22, LN_QUERY_BITS = 24, LN_GAP_BITS = LN_LEN_BITS + 1;
// The entry points refuse a DB whose longest sequence has 2^22 letters or more and more than 2^24 listed queries, so h < tLen < 2^22,
// -2^22 < gap = hX + hY - tLen < 2^22 and a list index fits its 24 bits: no field runs into its neighbour.
constexpr uint32_t LN_MAX_LETTERS = 1u << LN_LEN_BITS, LN_GAP_BIAS = 1u << LN_LEN_BITS, LN_GAP_MASK = (1u << LN_GAP_BITS) - 1u, LN_H_MASK = LN_MAX_LETTERS - 1u;
constexpr uint64_t LN_QUERIES_MOST = 1ull << LN_QUERY_BITS;
constexpr int LN_X_SHIFT = 24, LN_TAIL_BIT = 23, LN_REV_BIT = 22;
constexpr int LN_MAX_ANCHOR = 1024, LN_MAX_OVERHANG = 1024, LN_MAX_ENDS = 64, LN_MAX_READS = 1000000;

// CDM_LINKS_BATCH=<records>, CDM_LINKS_QUERIES=<queries> (tests): small inputs in several batches
uint64_t linksBatch() { return envCount("CDM_LINKS_BATCH", LN_BATCH_DEFAULT, LN_BATCH_DEFAULT); }
uint64_t linksQueries() { return envCount("CDM_LINKS_QUERIES", LN_QUERIES_MOST, LN_QUERIES_MOST); }

struct LinkArgs : ItemArgs {
    unsigned long long *stats;      // [nq][5] of the batch: reads, columns, left, right, both
    uint32_t *itemEnds;             // [items + 1]: end records per item, after the scan the item's first slot in the batch
    uint32_t *keys; uint64_t *vals; // k_ln_emit: [end records of the call] the read and the end word
    uint64_t slotBase;              // the batch's first slot
    uint32_t firstQuery, anchor, overhang;      // the batch's first list index
};

// The ends a counted record hangs over: bit 0 left, bit 1 right (0: no end record); h: the letters beyond the end it hangs over.
__device__ __forceinline__ uint32_t linkEnds(const Oriented &o, uint32_t qLen, uint32_t tLen, uint32_t anchor, uint32_t overhang, uint32_t &h) {
    const int u = o.qs - o.ds;          // (countedRecord: 0 <= qs < qLen, 0 <= ds < tLen, both below 2^22)
    const uint32_t L = (uint32_t) max(0, -u), R = (uint32_t) max(0, u + (int) tLen - (int) qLen);
    h = 0;
    if ((uint32_t) (o.qe - o.qs + 1) < anchor) return 0u;
    const bool left = L >= overhang, right = R >= overhang;
    h = left ? L : R;
    return (left ? 1u : 0u) | (right ? 2u : 0u);
}

__global__ __launch_bounds__(64 * PU_WAVES) void k_ln_count(LinkArgs a, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    const uint64_t item = first + local;
    const ItemRecords it = itemRecords(a, item);
    const uint32_t qLen = a.meta[it.q].len;
    unsigned int nReads = 0, nLeft = 0, nRight = 0, nBoth = 0; unsigned long long nCols = 0;
    for (uint64_t r = it.r0 + lane; r < it.r1; r += 64) {
        const AlnRec rec = a.rec[r];
        Oriented o; uint32_t tLen, tw, h;
        if (!countedRecord(a.meta, a.n, a.skipExt, a.minSeqId, it.q, qLen, rec, o, tLen, tw)) continue;
        nReads++; nCols += (uint32_t) (o.qe - o.qs) + 1u;
        const uint32_t ends = linkEnds(o, qLen, tLen, a.anchor, a.overhang, h);
        nLeft += ends == 1u; nRight += ends == 2u; nBoth += ends == 3u;
    }
    unsigned long long *row = a.stats + (uint64_t) it.qi * 5;
    addReadsColumns(&row[0], &row[1], nReads, nCols, lane);
    const unsigned int left = (unsigned int) cdm_wave_sum((int) nLeft), right = (unsigned int) cdm_wave_sum((int) nRight), both = (unsigned int) cdm_wave_sum((int) nBoth);
    if (lane == 0) {        // (at most 2^20 records per item)
        a.itemEnds[item] = left + right;
        if (left) atomicAdd(&row[2], (unsigned long long) left);
        if (right) atomicAdd(&row[3], (unsigned long long) right);
        if (both) atomicAdd(&row[4], (unsigned long long) both);
    }
}

// Slot of an end record: the batch's first, the item's first, the end records of the item's earlier rounds of 64, the end lanes below this one.
__global__ __launch_bounds__(64 * PU_WAVES) void k_ln_emit(LinkArgs a, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    const uint64_t item = first + local;
    const ItemRecords it = itemRecords(a, item);
    const uint32_t qLen = a.meta[it.q].len;
    uint64_t slot0 = a.slotBase + a.itemEnds[item];
    for (uint64_t rb = it.r0; rb < it.r1; rb += 64) {       // (wave-uniform: the ballot sees all 64 lanes)
        const uint64_t r = rb + lane;
        Oriented o = {0, 0, 0, 0, false}; uint32_t tLen = 0, tw = 0, h = 0, ends = 0, read = 0;
        if (r < it.r1) {
            const AlnRec rec = a.rec[r];
            if (countedRecord(a.meta, a.n, a.skipExt, a.minSeqId, it.q, qLen, rec, o, tLen, tw)) { ends = linkEnds(o, qLen, tLen, a.anchor, a.overhang, h); read = rec.target; }
        }
        const bool isEnd = ends == 1u || ends == 2u;
        const unsigned long long live = __ballot(isEnd);
        if (isEnd) {
            const uint64_t slot = slot0 + (uint64_t) __popcll(live & ((1ull << lane) - 1ull));
            const uint32_t tail = ((ends == 2u) != o.rev) ? 1u : 0u;
            a.keys[slot] = read;
            a.vals[slot] = (uint64_t) (a.firstQuery + it.qi) << LN_X_SHIFT | (uint64_t) tail << LN_TAIL_BIT | (uint64_t) (o.rev ? 1u : 0u) << LN_REV_BIT | h;
        }
        slot0 += (uint64_t) __popcll(live);
    }
}

// the end records sorted by read: a tile is DP_NT places
struct ReadRuns {
    const uint32_t *keys; const uint64_t *vals; const SeqMeta *meta;
    uint32_t *runOf;                // [n + 1]: 1 at a read's first place, after the scan the reads in front of a place
    uint32_t *runStart;             // [reads + 1]: per read, its first place; the closing entry is n
    uint32_t n, maxEnds; int qBits;
};
__global__ __launch_bounds__(DP_NT) void k_ln_read_heads(ReadRuns g, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i < g.n) g.runOf[i] = i == 0 || g.keys[i] != g.keys[i - 1];
}
__global__ __launch_bounds__(DP_NT) void k_ln_read_starts(ReadRuns g, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i >= g.n) return;
    if (g.runOf[i + 1] != g.runOf[i]) g.runStart[g.runOf[i]] = (uint32_t) i;
    if (i + 1 == g.n) g.runStart[g.runOf[g.n]] = g.n;
}
__device__ __forceinline__ bool lnTail(uint64_t v) { return (v >> LN_TAIL_BIT) & 1u; }
// the places [rs, re) of the read at place i; false: the read is crowded
__device__ __forceinline__ bool lnRun(const ReadRuns &g, uint64_t i, uint32_t &rs, uint32_t &re) {
    const uint32_t run = g.runOf[i + 1] - 1u;
    rs = g.runStart[run]; re = g.runStart[run + 1];
    return re - rs <= g.maxEnds;
}
// A pair: tail record v on list index x, head record w on list index y != x, of a read of tLen letters.  The canonical form has a < b:
// with x < y the edge as it stands (forward), otherwise (y, flip oY) -> (x, flip oX).  key: (a << 1 | oA) << (qBits + 1) | b << 1 | oB
struct LnPair { uint64_t key; int gap; bool fwd; uint32_t hX; };
__device__ __forceinline__ LnPair lnPair(uint64_t v, uint64_t w, int tLen, int qBits) {
    const uint32_t x = (uint32_t) (v >> LN_X_SHIFT), oX = (uint32_t) (v >> LN_REV_BIT) & 1u, hX = (uint32_t) v & LN_H_MASK;
    const uint32_t y = (uint32_t) (w >> LN_X_SHIFT), oY = (uint32_t) (w >> LN_REV_BIT) & 1u, hY = (uint32_t) w & LN_H_MASK;
    LnPair p;
    p.gap = (int) hX + (int) hY - tLen; p.fwd = x < y; p.hX = hX;
    const uint32_t from = p.fwd ? (x << 1 | oX) : (y << 1 | (oY ^ 1u)), to = p.fwd ? (y << 1 | oY) : (x << 1 | (oX ^ 1u));
    p.key = (uint64_t) from << (qBits + 1) | to;
    return p;
}

int linkBitsFor(uint64_t n) { int b = 0; while (b < 64 && (n - 1) >> b) b++; return n > 1 ? b : 0; }

// what a batch keeps from its count pass for its emit pass
struct LinkBatch {
    WorkItems work; cdmscan::ScanTemp st; DevBuf<uint32_t> itemEnds;
    uint64_t b0 = 0, slotBase = 0; uint32_t m = 0;
};

// What the stage leaves: nEnds end records, and where there are any the sorted arrays with the runs, as g names them.
struct EndRecords {
    QuerySizes qs;
    std::vector<std::unique_ptr<LinkBatch>> batches;
    DevBuf<uint32_t> k0, k1, runOf, runStart; DevBuf<uint64_t> v0, v1; cdmscan::ScanTemp stRuns;
    uint64_t nEnds = 0; ReadRuns g;
};

// The stage.  stats: NULL, or [nq][6] - columns 0..4 are written, 5 is set to 0.  CDM_ERR_UNSUPPORTED with e.nEnds set where the end
// records reach 2^32.  ms: the kernels' time is added.
int linkEndRecords(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t nq, const cdm_links_params *par, const char *WHO, uint64_t *stats,
                   EndRecords &e, float &msTotal) {
    hipStream_t s = ctx->stream;
    const uint32_t chunk = pileupChunk();
    const uint64_t bound = linksBatch(), mostQueries = linksQueries();
    QuerySizes &qs = e.qs;
    if (int rc = querySizes(ctx, db, alns, queries, nq, WHO, "record slots", qs)) return rc;
    LinkArgs a;
    a.stats = nullptr; a.itemEnds = nullptr; a.keys = nullptr; a.vals = nullptr; a.slotBase = 0; a.firstQuery = 0;
    a.anchor = (uint32_t) par->anchor; a.overhang = (uint32_t) par->overhang;
    // the count pass: the statistics of every query, the end records of every item
    std::vector<uint64_t> row;
    uint64_t nEnds = 0;
    for (uint64_t b0 = 0; b0 < nq;) {
        // the batch: listed queries while their records stay within the bound; a single query with more goes alone
        uint32_t m = 0; uint64_t sum = 0;
        for (; b0 + m < nq && m < mostQueries && (m == 0 || sum + qs.recs[b0 + m] <= bound); m++) sum += qs.recs[b0 + m];
        e.batches.emplace_back(new LinkBatch());
        LinkBatch &b = *e.batches.back();
        b.b0 = b0; b.m = m; b.slotBase = nEnds;
        DevBuf<unsigned long long> dStats;
        if (!b.work.alloc(m) || !dStats.alloc((size_t) m * 5)) { cdm_set_error("%s: out of device memory for %u queries", WHO, m); return CDM_ERR_HIP; }
        CDM_HIP(hipMemsetAsync(dStats.p, 0, (size_t) m * 40, s));
        if (int rc = workItems(s, alns, qs.dq.p + b0, m, chunk, b.work)) return rc;
        const uint64_t nItems = b.work.n;
        fillArgs(a, qs.meta.p, db, alns, par->min_seq_id, par->skip_extended_targets, b.work);
        if (!b.itemEnds.alloc((size_t) nItems + 1)) { cdm_set_error("%s: out of device memory for %llu work items", WHO, (unsigned long long) nItems); return CDM_ERR_HIP; }
        CDM_HIP(hipMemsetAsync(b.itemEnds.p + nItems, 0, 4, s));          // (the closing word: the scan leaves the batch's total there)
        a.stats = dStats.p; a.itemEnds = b.itemEnds.p; a.firstQuery = (uint32_t) b0;
        uint32_t nThis = 0;
        row.assign((size_t) m * 5, 0);
        hipEventRecord(ctx->ev0, s);
        launchWaveItems(s, k_ln_count, a, nItems);
        if (int rc = cdmscan::exclusiveScan<uint32_t>(s, b.st, b.itemEnds.p, b.itemEnds.p, (size_t) nItems + 1)) return rc;        // (in place: scan.h)
        CDM_HIP(hipMemcpyAsync(&nThis, b.itemEnds.p + nItems, 4, hipMemcpyDeviceToHost, s));
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        CDM_HIP(hipMemcpyAsync(row.data(), dStats.p, (size_t) m * 40, hipMemcpyDeviceToHost, s));
        if (int rc = finishTimed(ctx, WHO, "counting", msTotal)) return rc;
        if (stats)
            for (uint32_t i = 0; i < m; i++) { for (int c = 0; c < 5; c++) stats[(b0 + i) * 6 + c] = row[(size_t) i * 5 + c]; stats[(b0 + i) * 6 + 5] = 0; }
        nEnds += nThis;
        b0 += m;
    }
    e.nEnds = nEnds;
    e.g.keys = nullptr; e.g.vals = nullptr; e.g.meta = qs.meta.p; e.g.runOf = nullptr; e.g.runStart = nullptr; e.g.n = 0; e.g.maxEnds = (uint32_t) par->max_ends; e.g.qBits = std::max(1, linkBitsFor(nq));
    if (nEnds >> 32) { cdm_set_error("%s: the listed queries hold %llu end records; the 32-bit places of the read sort hold fewer than 2^32", WHO, (unsigned long long) nEnds); return CDM_ERR_UNSUPPORTED; }
    if (!nEnds) return CDM_OK;
    const uint32_t n = (uint32_t) nEnds;
    if (!e.k0.alloc(n) || !e.k1.alloc(n) || !e.v0.alloc(n) || !e.v1.alloc(n) || !e.runOf.alloc((size_t) n + 1) || !e.runStart.alloc((size_t) n + 1)) {
        cdm_set_error("%s: out of device memory for %u end records", WHO, n); return CDM_ERR_HIP;
    }
    a.keys = e.k0.p; a.vals = e.v0.p; a.stats = nullptr;
    CDM_HIP(hipMemsetAsync(e.runOf.p + n, 0, 4, s));
    hipEventRecord(ctx->ev0, s);
    for (const auto &bp : e.batches) {
        const LinkBatch &b = *bp;
        fillArgs(a, qs.meta.p, db, alns, par->min_seq_id, par->skip_extended_targets, b.work);
        a.itemEnds = b.itemEnds.p; a.slotBase = b.slotBase; a.firstQuery = (uint32_t) b.b0;
        launchWaveItems(s, k_ln_emit, a, b.work.n);
    }
    bool inFirst = true;        // on the bits of a sequence index in use; nothing below leans on the order inside a read's run
    if (int rc = rx::sortPairs<uint32_t, uint64_t>(s, ctx->cuCount, e.k0.p, e.k1.p, e.v0.p, e.v1.p, (uint64_t) n, 0, std::max(1, linkBitsFor(db->n)), inFirst)) return rc;
    e.g.keys = inFirst ? e.k0.p : e.k1.p; e.g.vals = inFirst ? e.v0.p : e.v1.p; e.g.runOf = e.runOf.p; e.g.runStart = e.runStart.p; e.g.n = n;
    const uint64_t nTiles = ((uint64_t) n + DP_NT - 1) / DP_NT;
    launchTiles(s, k_ln_read_heads, e.g, nTiles);
    if (int rc = cdmscan::exclusiveScan<uint32_t>(s, e.stRuns, e.runOf.p, e.runOf.p, (size_t) n + 1)) return rc;       // (in place)
    launchTiles(s, k_ln_read_starts, e.g, nTiles);
    hipEventRecord(ctx->ev1, s);
    CDM_LAUNCH_CHECK();
    return finishTimed(ctx, WHO, "read sort", msTotal);
}

}  // namespace
