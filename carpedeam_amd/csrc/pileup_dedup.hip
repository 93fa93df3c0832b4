// Duplicate reads out of an alignment set (cdm_alns_dedup; not a module of the reference): a second set over the same DB without the
// PCR copies on the listed queries, so that every reduction over the read pile-up sees a molecule once.  The rule is DeDup's for merged
// reads on the records a set holds (include/carpedeam_hip.h): the counted records of a listed query with equal strand, unclipped start
// u = qs - ds and read length form a group; the record with the largest ident, among equals the earliest in the set, stays.  What it
// shares with the reductions over the pile-up is in pileup.h.  Its own: like cdm_pileup_map the batch cut is by RECORDS.
//
//   per batch (consecutive listed queries whose record counts sum to at most the bound, at most 2^18 of them):
//   k_dd_count     one wave per work item, lanes over records: the counted records per item and per query
//   scan           every item's first slot
//   k_dd_emit      the same walk again: slots by wave ballot and prefix rank (alignment-set order); per slot the key
//                  batch query << 46 | rev << 45 | tLen << 23 | (u + 2^22), the slot as the value, the record's index
//   sort           on the key bits in use (radix.h): a run of equal keys is a group.  Nothing here leans on the sort being stable: the
//                  survivor is the maximum below, which carries the slot, and the slots of a query follow the set's order
//   k_dd_heads     1 where a key differs from its predecessor; the scan makes the run ids
//   k_dd_best      ident << 32 | (2^32 - 1 - slot) into best[run] with a 64-bit atomicMax, the lanes of a wave that share a run reduced
//                  first (the records of a run are neighbours); the run's first place
//   k_dd_keep      a record that is not its run's best clears its keep flag; a run's last record adds the run to the query's statistics
//   over the whole set:
//   k_dd_flag      the keep flags as 64-bit counts; the scan gives every record's place in the output
//   k_dd_offsets   the output's offsets: the place of every row's first record (rows that are not listed keep their counts)
//   k_dd_compact   records and purine/pyrimidine counts to their places: the order inside every row is kept
#include "pileup.h"
#include "radix.h"

namespace {

constexpr uint64_t DD_BATCH_DEFAULT = 1ull << 26;       // records per batch, cdm_pileup_map's bound: 2^26 x (2 x 8 + 2 x 4 + 8 + 4 + 8 + 4) bytes = 3.2 GB
constexpr uint64_t DD_QUERIES_MOST = 1ull << 18;        // queries per batch: the key's top 18 bits
constexpr int DD_U_BITS = 23, DD_LEN_BITS = 22, DD_QUERY_SHIFT = DD_U_BITS + DD_LEN_BITS + 1;        // 46
// The entry point refuses a DB whose longest sequence has 2^22 letters or more (db->maxLen; kmermatcher's own bound, kmer_plan.h
// MAX_SEQ_LETTERS, but no upload checks it), so tLen < 2^22 and -(2^22 - 1) <= u < 2^22: the fields cannot run into each other.
constexpr uint32_t DD_MAX_LETTERS = 1u << DD_LEN_BITS, DD_U_BIAS = 1u << 22;

// CDM_DEDUP_BATCH=<records>, CDM_DEDUP_QUERIES=<queries> (tests): small inputs in several batches
uint64_t dedupBatch() { return envCount("CDM_DEDUP_BATCH", DD_BATCH_DEFAULT, DD_BATCH_DEFAULT); }
uint64_t dedupQueries() { return envCount("CDM_DEDUP_QUERIES", DD_QUERIES_MOST, DD_QUERIES_MOST); }

struct DedupArgs : ItemArgs {
    unsigned long long *stats;      // [nq][4] of the batch
    uint32_t *itemRecs;             // [items + 1]: counted records per item, after the scan the item's first slot
    uint64_t *keys; uint32_t *vals; // k_dd_emit: [itemRecs[items]] the group key and the slot
    uint64_t *recOf;                // [itemRecs[items]] the slot's record in the set
};

__global__ __launch_bounds__(64 * PU_WAVES) void k_dd_count(DedupArgs a, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    const uint64_t item = first + local;
    const ItemRecords it = itemRecords(a, item);
    const uint32_t qLen = a.meta[it.q].len;
    unsigned int nCounted = 0;
    for (uint64_t r = it.r0 + lane; r < it.r1; r += 64) {
        const AlnRec rec = a.rec[r];
        Oriented o; uint32_t tLen, tw;
        nCounted += countedRecord(a.meta, a.n, a.skipExt, a.minSeqId, it.q, qLen, rec, o, tLen, tw);
    }
    const unsigned int all = (unsigned int) cdm_wave_sum((int) nCounted);       // (at most 2^20 records per item)
    if (lane == 0) {
        a.itemRecs[item] = all;
        if (all) atomicAdd(&a.stats[(uint64_t) it.qi * 4], (unsigned long long) all);
    }
}

// Slot of a counted record: the item's first, the counted records of the item's earlier rounds of 64, the counted lanes below this one.
__global__ __launch_bounds__(64 * PU_WAVES) void k_dd_emit(DedupArgs a, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    const uint64_t item = first + local;
    const ItemRecords it = itemRecords(a, item);
    const uint32_t qLen = a.meta[it.q].len;
    uint32_t slot0 = a.itemRecs[item];
    for (uint64_t rb = it.r0; rb < it.r1; rb += 64) {       // (wave-uniform: the ballot sees all 64 lanes)
        const uint64_t r = rb + lane;
        Oriented o = {0, 0, 0, 0, false}; uint32_t tLen = 0, tw = 0;
        bool counted = false;
        if (r < it.r1) { const AlnRec rec = a.rec[r]; counted = countedRecord(a.meta, a.n, a.skipExt, a.minSeqId, it.q, qLen, rec, o, tLen, tw); }
        const unsigned long long live = __ballot(counted);
        if (counted) {
            const uint32_t slot = slot0 + (uint32_t) __popcll(live & ((1ull << lane) - 1ull));
            const uint32_t u = (uint32_t) (o.qs - o.ds + (int) DD_U_BIAS);          // (countedRecord: 0 <= qs < qLen, 0 <= ds < tLen)
            a.keys[slot] = (uint64_t) it.qi << DD_QUERY_SHIFT | (uint64_t) (o.rev ? 1u : 0u) << (DD_QUERY_SHIFT - 1) | (uint64_t) tLen << DD_U_BITS | u;
            a.vals[slot] = slot; a.recOf[slot] = r;
        }
        slot0 += (uint32_t) __popcll(live);
    }
}

// the sorted order: a tile is DP_NT places
struct RunArgs {
    const uint64_t *keys; const uint32_t *vals; const uint64_t *recOf; const AlnRec *rec;
    uint32_t *runOf;                // [n + 1]: 1 at a run's first place, after the scan the runs in front of a place
    unsigned long long *best;       // [n]: per run, the key of its survivor
    uint32_t *runStart;             // [n]: per run, its first place
    unsigned long long *stats;      // [nq][4] of the batch
    uint8_t *keep;                  // [records of the set]
    uint32_t n;
};
__global__ __launch_bounds__(DP_NT) void k_dd_heads(RunArgs g, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i < g.n) g.runOf[i] = i == 0 || g.keys[i] != g.keys[i - 1];
}
__device__ __forceinline__ unsigned long long ddShflDown64(unsigned long long v, int d) {
    return ((unsigned long long) (unsigned int) __shfl_down((int) (v >> 32), d, 64) << 32) | (unsigned int) __shfl_down((int) (unsigned int) v, d, 64);
}
// What decides a group's survivor: the larger ident (signed: the sign bit flipped), then the smaller slot - the slots of a query follow
// the set's order.  (every lane of a wave reaches the shuffles: no early return)
__global__ __launch_bounds__(DP_NT) void k_dd_best(RunArgs g, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = i < g.n;
    uint32_t run = 0xFFFFFFFFu; unsigned long long v = 0; bool head = false;
    if (valid) {
        const uint32_t before = g.runOf[i], upTo = g.runOf[i + 1], slot = g.vals[i];
        run = upTo - 1u; head = upTo != before;
        v = (unsigned long long) ((uint32_t) g.rec[g.recOf[slot]].ident ^ 0x80000000u) << 32 | (0xFFFFFFFFu - slot);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {      // the lanes of a run are neighbours: its first lane in the wave ends with the maximum
        const unsigned long long ov = ddShflDown64(v, d);
        const uint32_t orun = (uint32_t) __shfl_down((int) run, d, 64);
        if (lane + d < 64 && orun == run && ov > v) v = ov;
    }
    const uint32_t prev = (uint32_t) __shfl_up((int) run, 1, 64);
    if (!valid) return;
    if (lane == 0 || prev != run) atomicMax(&g.best[run], v);
    if (head) g.runStart[run] = (uint32_t) i;
}
// (the places of a query are neighbours too: the runs that end in a wave and their longest are reduced per query before the atomics -
// one word takes some 88 atomics a microsecond)
__global__ __launch_bounds__(DP_NT) void k_dd_keep(RunArgs g, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = i < g.n;
    uint32_t q = 0xFFFFFFFFu, ended = 0, longest = 0;
    if (valid) {
        const uint32_t slot = g.vals[i], run = g.runOf[i + 1] - 1u;
        if (slot != 0xFFFFFFFFu - (uint32_t) g.best[run]) g.keep[g.recOf[slot]] = 0;
        q = (uint32_t) (g.keys[i] >> DD_QUERY_SHIFT);
        if (i + 1 == g.n || g.runOf[i + 2] != g.runOf[i + 1]) { ended = 1; longest = (uint32_t) i - g.runStart[run] + 1u; }      // the run's last place
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t oq = (uint32_t) __shfl_down((int) q, d, 64), oe = (uint32_t) __shfl_down((int) ended, d, 64), ol = (uint32_t) __shfl_down((int) longest, d, 64);
        if (lane + d < 64 && oq == q) { ended += oe; longest = max(longest, ol); }
    }
    const uint32_t prev = (uint32_t) __shfl_up((int) q, 1, 64);
    if (!valid || !ended || !(lane == 0 || prev != q)) return;
    unsigned long long *row = g.stats + (uint64_t) q * 4;
    atomicAdd(&row[1], (unsigned long long) ended);
    atomicMax(&row[3], (unsigned long long) longest);
}

// the whole set: a tile is DP_NT records or rows
struct PackArgs {
    const uint64_t *off; const AlnRec *rec; const uint16_t *ry; const uint8_t *keep;
    uint64_t *place;                // [count + 1]: the keep flag, after the scan the record's place in the output
    uint64_t *offOut; AlnRec *recOut; uint16_t *ryOut;
    uint64_t count, n;
};
__global__ __launch_bounds__(DP_NT) void k_dd_flag(PackArgs p, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i <= p.count) p.place[i] = i < p.count ? p.keep[i] : 0;
}
__global__ __launch_bounds__(DP_NT) void k_dd_offsets(PackArgs p, uint64_t first) {
    const uint64_t q = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (q <= p.n) p.offOut[q] = p.place[p.off[q]];       // (off[q] <= count)
}
__global__ __launch_bounds__(DP_NT) void k_dd_compact(PackArgs p, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i >= p.count || !p.keep[i]) return;
    const uint64_t to = p.place[i];
    p.recOut[to] = p.rec[i];
    if (p.ry) p.ryOut[to] = p.ry[i];
}

int dedupBitsFor(uint64_t n) { int b = 0; while (b < 64 && (n - 1) >> b) b++; return n > 1 ? b : 0; }

// the new set while it is built: the caller's only on success
struct NewSet {
    cdm_alns *a = nullptr;
    ~NewSet() { if (a) cdm_alns_free(a); }
    cdm_alns *release() { cdm_alns *r = a; a = nullptr; return r; }
};
bool allocSet(NewSet &to, const cdm_alns *like, uint64_t count) {
    to.a = new cdm_alns();
    to.a->n = like->n; to.a->count = count; to.a->rySerial = like->rySerial;
    return cdmMalloc(&to.a->off, (like->n + 1) * 8) == hipSuccess && cdmMalloc(&to.a->rec, (count + 1) * sizeof(AlnRec)) == hipSuccess &&
           (!like->ryMism || cdmMalloc(&to.a->ryMism, (count + 1) * sizeof(uint16_t)) == hipSuccess);
}

}  // namespace

static int cdm_dedup_impl(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t nq, const cdm_dedup_params *par, cdm_alns **out, uint64_t *stats,
                          uint8_t *keepOut, float *kernelMs) {
    static const char *const WHO = "cdm_alns_dedup";
    hipStream_t s = ctx->stream;
    const uint32_t chunk = pileupChunk();
    const uint64_t bound = dedupBatch(), mostQueries = dedupQueries();
    const uint64_t count = alns->count;
    QuerySizes qs;
    if (int rc = querySizes(ctx, db, alns, queries, nq, WHO, "record slots", qs)) return rc;
    DevBuf<uint8_t> keep;
    if (!keep.alloc((size_t) count)) { cdm_set_error("%s: out of device memory for the keep flags of %llu records", WHO, (unsigned long long) count); return CDM_ERR_HIP; }
    CDM_HIP(hipMemsetAsync(keep.p, 1, (size_t) count + 1, s));
    float msTotal = 0.f;
    DedupArgs a;
    a.stats = nullptr; a.itemRecs = nullptr; a.keys = nullptr; a.vals = nullptr; a.recOf = nullptr;
    for (uint64_t b0 = 0; b0 < nq;) {
        // the batch: listed queries while their records stay within the bound; a single query with more goes alone
        uint32_t m = 0; uint64_t sum = 0;
        for (; b0 + m < nq && m < mostQueries && (m == 0 || sum + qs.recs[b0 + m] <= bound); m++) sum += qs.recs[b0 + m];
        WorkItems work; cdmscan::ScanTemp stRecs, stRuns;
        DevBuf<unsigned long long> dStats; DevBuf<uint32_t> itemRecs;
        if (!work.alloc(m) || !dStats.alloc((size_t) m * 4)) { cdm_set_error("%s: out of device memory for %u queries", WHO, m); return CDM_ERR_HIP; }
        CDM_HIP(hipMemsetAsync(dStats.p, 0, (size_t) m * 32, s));
        if (int rc = workItems(s, alns, qs.dq.p + b0, m, chunk, work)) return rc;
        const uint64_t nItems = work.n;
        fillArgs(a, qs.meta.p, db, alns, par->min_seq_id, par->skip_extended_targets, work);
        if (!itemRecs.alloc((size_t) nItems + 1)) { cdm_set_error("%s: out of device memory for %llu work items", WHO, (unsigned long long) nItems); return CDM_ERR_HIP; }
        CDM_HIP(hipMemsetAsync(itemRecs.p + nItems, 0, 4, s));          // (the closing word: the scan leaves the batch's total there)
        a.stats = dStats.p; a.itemRecs = itemRecs.p;
        uint32_t nRec = 0;
        hipEventRecord(ctx->ev0, s);
        launchWaveItems(s, k_dd_count, a, nItems);
        if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stRecs, itemRecs.p, itemRecs.p, (size_t) nItems + 1)) return rc;        // (in place: scan.h)
        CDM_HIP(hipMemcpyAsync(&nRec, itemRecs.p + nItems, 4, hipMemcpyDeviceToHost, s));
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        if (int rc = finishTimed(ctx, WHO, "counting", msTotal)) return rc;
        if (nRec) {
            DevBuf<uint64_t> k0, k1, recOf; DevBuf<uint32_t> v0, v1, runOf, runStart; DevBuf<unsigned long long> best;
            if (!k0.alloc(nRec) || !k1.alloc(nRec) || !recOf.alloc(nRec) || !v0.alloc(nRec) || !v1.alloc(nRec) || !runOf.alloc((size_t) nRec + 1) || !runStart.alloc(nRec) || !best.alloc(nRec)) {
                cdm_set_error("%s: out of device memory for %u counted records", WHO, nRec); return CDM_ERR_HIP;
            }
            a.keys = k0.p; a.vals = v0.p; a.recOf = recOf.p;
            CDM_HIP(hipMemsetAsync(runOf.p + nRec, 0, 4, s));
            CDM_HIP(hipMemsetAsync(best.p, 0, (size_t) nRec * 8, s));
            hipEventRecord(ctx->ev0, s);
            launchWaveItems(s, k_dd_emit, a, nItems);
            bool inFirst = true;        // on the bits in use; the value is the slot: 32 bits that order a query's records as the set does, for k_dd_best's key
            if (int rc = rx::sortPairs<uint64_t, uint32_t>(s, ctx->cuCount, k0.p, k1.p, v0.p, v1.p, (uint64_t) nRec, 0, DD_QUERY_SHIFT + dedupBitsFor(m), inFirst)) return rc;
            RunArgs g;
            g.keys = inFirst ? k0.p : k1.p; g.vals = inFirst ? v0.p : v1.p; g.recOf = recOf.p; g.rec = alns->rec; g.runOf = runOf.p; g.best = best.p; g.runStart = runStart.p;
            g.stats = dStats.p; g.keep = keep.p; g.n = nRec;
            const uint64_t nTiles = ((uint64_t) nRec + DP_NT - 1) / DP_NT;
            launchTiles(s, k_dd_heads, g, nTiles);
            if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stRuns, runOf.p, runOf.p, (size_t) nRec + 1)) return rc;       // (in place)
            launchTiles(s, k_dd_best, g, nTiles);
            launchTiles(s, k_dd_keep, g, nTiles);
            hipEventRecord(ctx->ev1, s);
            CDM_LAUNCH_CHECK();
            CDM_HIP(hipMemcpyAsync(stats + b0 * 4, dStats.p, (size_t) m * 32, hipMemcpyDeviceToHost, s));
            if (int rc = finishTimed(ctx, WHO, "grouping", msTotal)) return rc;
        } else {
            for (uint64_t i = 0; i < (uint64_t) m * 4; i++) stats[b0 * 4 + i] = 0;
        }
        b0 += m;
    }
    for (uint64_t i = 0; i < nq; i++) stats[i * 4 + 2] = stats[i * 4] - stats[i * 4 + 1];
    // the output: every kept record's place, the rows' new offsets, the records at their places
    DevBuf<uint64_t> place; cdmscan::ScanTemp stPlace;
    if (!place.alloc((size_t) count + 1)) { cdm_set_error("%s: out of device memory for the places of %llu records", WHO, (unsigned long long) count); return CDM_ERR_HIP; }
    PackArgs p;
    p.off = alns->off; p.rec = alns->rec; p.ry = alns->ryMism; p.keep = keep.p; p.place = place.p; p.offOut = nullptr; p.recOut = nullptr; p.ryOut = nullptr; p.count = count; p.n = alns->n;
    uint64_t total = 0;
    hipEventRecord(ctx->ev0, s);
    launchTiles(s, k_dd_flag, p, (count + 1 + DP_NT - 1) / DP_NT);
    if (int rc = cdmscan::exclusiveScan<uint64_t>(s, stPlace, place.p, place.p, (size_t) count + 1)) return rc;       // (in place)
    CDM_HIP(hipMemcpyAsync(&total, place.p + count, 8, hipMemcpyDeviceToHost, s));
    hipEventRecord(ctx->ev1, s);
    CDM_LAUNCH_CHECK();
    if (int rc = finishTimed(ctx, WHO, "placing", msTotal)) return rc;
    NewSet made;
    if (!allocSet(made, alns, total)) { cdm_set_error("%s: out of device memory for a set of %llu records", WHO, (unsigned long long) total); return CDM_ERR_HIP; }
    p.offOut = made.a->off; p.recOut = made.a->rec; p.ryOut = made.a->ryMism;
    hipEventRecord(ctx->ev0, s);
    launchTiles(s, k_dd_offsets, p, (alns->n + 1 + DP_NT - 1) / DP_NT);
    launchTiles(s, k_dd_compact, p, (count + DP_NT - 1) / DP_NT);
    hipEventRecord(ctx->ev1, s);
    CDM_LAUNCH_CHECK();
    if (keepOut && count) CDM_HIP(hipMemcpyAsync(keepOut, keep.p, (size_t) count, hipMemcpyDeviceToHost, s));
    if (int rc = finishTimed(ctx, WHO, "compaction", msTotal)) return rc;
    *out = made.release();
    if (kernelMs) *kernelMs = msTotal;
    return CDM_OK;
}

// n_queries == 0: a copy of the set, no kernel
static int cdm_dedup_copy(cdm_ctx *ctx, const cdm_alns *alns, cdm_alns **out, uint8_t *keepOut) {
    hipStream_t s = ctx->stream;
    NewSet made;
    if (!allocSet(made, alns, alns->count)) { cdm_set_error("cdm_alns_dedup: out of device memory for a set of %llu records", (unsigned long long) alns->count); return CDM_ERR_HIP; }
    CDM_HIP(hipMemcpyAsync(made.a->off, alns->off, (alns->n + 1) * 8, hipMemcpyDeviceToDevice, s));
    if (alns->count) CDM_HIP(hipMemcpyAsync(made.a->rec, alns->rec, alns->count * sizeof(AlnRec), hipMemcpyDeviceToDevice, s));
    if (alns->count && alns->ryMism) CDM_HIP(hipMemcpyAsync(made.a->ryMism, alns->ryMism, alns->count * sizeof(uint16_t), hipMemcpyDeviceToDevice, s));
    CDM_HIP(hipStreamSynchronize(s));
    if (keepOut) memset(keepOut, 1, (size_t) alns->count);
    *out = made.release();
    return CDM_OK;
}

extern "C" int cdm_alns_dedup(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_dedup_params *par, cdm_alns **out, uint64_t *stats,
                              uint8_t *keep, float *kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.f;
    if (out) *out = NULL;
    if (!ctx || !db || !alns || !par || !out || (n_queries && (!queries || !stats))) { cdm_set_error("cdm_alns_dedup: NULL argument"); return CDM_ERR_INVALID; }
    CDM_REFUSE_UNDEFINED_ALNS(alns, "cdm_alns_dedup");
    if (int rc = pileupCheckArgs("cdm_alns_dedup", db, alns, queries, n_queries)) return rc;
    CDM_HIP(hipSetDevice(ctx->device));
    if (n_queries == 0) return cdm_dedup_copy(ctx, alns, out, keep);
    if (db->maxLen >= DD_MAX_LETTERS) {     // (no upload refuses such a DB: cdm_kmermatch does, which a set from cdm_alns_upload never met)
        cdm_set_error("cdm_alns_dedup: the DB holds a sequence of %u letters; the group key holds a read's length in %d bits and its unclipped start in %d (sequences of fewer than %u letters)",
                      db->maxLen, DD_LEN_BITS, DD_U_BITS, DD_MAX_LETTERS);
        return CDM_ERR_UNSUPPORTED;
    }
    return cdm_dedup_impl(ctx, db, alns, queries, n_queries, par, out, stats, keep, kernel_ms);
}
