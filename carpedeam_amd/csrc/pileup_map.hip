// The reads on the listed queries as alignment records (cdm_pileup_map; not a module of the reference): one record per counted record
// of the pile-up with what a SAM line needs and the alignment set does not carry - the number of mismatch columns, the mismatch
// columns themselves, coordinate order, and one primary record per read (include/carpedeam_hip.h).  What it shares with the other
// reductions over the read pile-up is in pileup.h.  Its own: the batch cut is by RECORDS, not by query length (a batch's buffers hold
// records), and the primary of a read is chosen over the whole call before any batch is emitted.
//
//   k_map_primary  one wave per work item, lanes over records: a counted record puts columns << 40 | (2^40 - 1 - record index) into
//                  best[target] with a 64-bit atomicMax - the most columns, among equals the earliest record.  No letters are read.
//   per batch (consecutive listed queries whose record counts sum to at most the bound):
//   k_map_count    the same walk; a lane compares the columns of its record 16 at a time (2-bit codes XORed, the N bits of both
//                  sequences ORed in, the tail masked, popcount) and keeps the count in a register; per item the counted records and
//                  the mismatches, per query the four statistics
//   scans          every item's first record slot and first mismatch word
//   k_map_emit     the same walk again: record slots by wave ballot and prefix rank (alignment-set order), mismatch words behind
//                  the item's first by a wave prefix sum of the lanes' counts; the secondary flag from best[target]
//   sort           the slots by query << 24 | pos, stable (radix.h): the third ordering key, the order in the set, comes free
//   k_map_gather   records and words in sorted order, mm as the running sum of nm
// A batch holds consecutive listed queries, so the batches' records concatenate into the order the header defines.
#include "pileup.h"
#include "radix.h"

namespace {

constexpr uint64_t MP_BATCH_DEFAULT = 1ull << 26;       // records per batch: 2^26 x (2 x 40 + 2 x 12 + 8) bytes = 7.5 GB and the words
constexpr int MP_POS_BITS = 24, MP_INDEX_BITS = 40;
constexpr unsigned long long MP_INDEX_MASK = (1ull << MP_INDEX_BITS) - 1ull;

// CDM_MAP_BATCH=<records> (tests): small inputs in several batches
uint64_t mapBatch() { return envCount("CDM_MAP_BATCH", MP_BATCH_DEFAULT, MP_BATCH_DEFAULT); }

struct MapArgs : ItemArgs {
    const uint32_t *codes, *nmask;
    unsigned long long *best;       // [n]: the key of every target's primary record, 0 for a target without counted record
    unsigned long long *stats;      // [nq][4]
    uint32_t *itemRecs;             // NULL, or [items + 1]: counted records per item, after the scan the item's first record slot
    uint64_t *itemWords;            // [items + 1]: mismatches per item, after the scan the item's first mismatch word
    cdm_map_rec *recs;              // k_map_emit: [itemRecs[items]], query = the index in the batch, mm = the index in `words`
    uint32_t *words;                // [itemWords[items]]
    uint64_t *keys; uint32_t *vals; // [itemRecs[items]]: query << 24 | pos and the slot
};

// what decides the primary of a target: more columns, then the smaller index r in the set
__device__ __forceinline__ unsigned long long mapKey(uint32_t columns, uint64_t r) { return (unsigned long long) columns << MP_INDEX_BITS | (MP_INDEX_MASK - r); }

// 16 N bits of the (optionally reversed) sequence at word w0 from oriented position i (i < L); the bits of positions beyond the
// sequence are garbage.  The mask plane has a spare word behind its last (seqdbMaskBytes), so the second load stays inside.
__device__ __forceinline__ uint32_t mapNWindow16(const uint32_t *__restrict__ nmask, uint32_t w0, uint32_t L, bool rc, uint32_t i) {
    const int s = rc ? (int) L - 16 - (int) i : (int) i;
    const uint64_t bit = (uint64_t) w0 * 16u + (uint32_t) max(s, 0);
    const uint64_t two = (uint64_t) nmask[bit >> 5] | (uint64_t) nmask[(bit >> 5) + 1] << 32;
    uint32_t w = (uint32_t) (two >> (bit & 31u)) & 0xFFFFu;
    if (!rc) return w;
    if (s < 0) w = (w << (-s)) & 0xFFFFu;
    return __brev(w) >> 16;
}

// a counted record's columns: column c sits on query position qs + c and on oriented read position ds + c
struct MapCols { uint32_t qw, qLen, qLast, tw, tLen, tLast, qs, ds, L; bool rev; };
__device__ __forceinline__ MapCols mapCols(const SeqMeta &qm, const Oriented &o, uint32_t tLen, uint32_t tw) {
    MapCols m;
    m.qw = qm.woff; m.qLen = qm.len; m.qLast = (qm.len + 15u) / 16u - 1u; m.tw = tw; m.tLen = tLen; m.tLast = (tLen + 15u) / 16u - 1u;
    m.qs = (uint32_t) o.qs; m.ds = (uint32_t) o.ds; m.L = (uint32_t) (o.qe - o.qs) + 1u; m.rev = o.rev;
    return m;
}
// The columns c .. c + 15 (c < L): bit j of the result is set where column c + j is a mismatch - the codes differ or either letter is
// an N.  qWin / tWin: the 2-bit codes of the query and of the read as the query's strand sees it; qN / tN: their N bits.
// (countedRecord: qs + L <= qLen and ds + L <= tLen, so every column below L lies inside both sequences)
__device__ __forceinline__ uint32_t mapMismatch16(const MapArgs &a, const MapCols &m, uint32_t c, uint32_t &qWin, uint32_t &tWin, uint32_t &qN, uint32_t &tN) {
    qWin = cdm_window16(a.codes, m.qw, m.qs + c, m.qLast);
    tWin = cdm_oriented_window16(a.codes, m.tw, m.tLen, m.tLast, m.rev, m.ds + c);
    qN = mapNWindow16(a.nmask, m.qw, m.qLen, false, m.qs + c);
    tN = mapNWindow16(a.nmask, m.tw, m.tLen, m.rev, m.ds + c);
    const uint32_t x = qWin ^ tWin, left = m.L - c;
    const uint32_t bits = cdm_squash16(x | (x >> 1)) | qN | tN;
    return left >= 16u ? bits : bits & ((1u << left) - 1u);
}
__device__ __forceinline__ uint32_t mapMismatches(const MapArgs &a, const MapCols &m) {
    uint32_t nm = 0, qWin, tWin, qN, tN;
    for (uint32_t c = 0; c < m.L; c += 16u) nm += (uint32_t) __popc(mapMismatch16(a, m, c, qWin, tWin, qN, tN));
    return nm;
}

// the primary pass: one wave per item of this launch's slice
__global__ __launch_bounds__(64 * PU_WAVES) void k_map_primary(MapArgs a, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    const ItemRecords it = itemRecords(a, first + local);
    const uint32_t qLen = a.meta[it.q].len;
    for (uint64_t r = it.r0 + lane; r < it.r1; r += 64) {
        const AlnRec rec = a.rec[r];
        Oriented o; uint32_t tLen, tw;
        if (!countedRecord(a.meta, a.n, a.skipExt, a.minSeqId, it.q, qLen, rec, o, tLen, tw)) continue;
        atomicMax(&a.best[rec.target], mapKey((uint32_t) (o.qe - o.qs) + 1u, r));       // (countedRecord: target < n; result unused)
    }
}

// counting: one wave per item of this launch's slice, lanes take records
__global__ __launch_bounds__(64 * PU_WAVES) void k_map_count(MapArgs a, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    const uint64_t item = first + local;
    const ItemRecords it = itemRecords(a, item);
    const SeqMeta qm = a.meta[it.q];
    unsigned int nReads = 0, nPrimary = 0; unsigned long long nCols = 0, nMism = 0;
    for (uint64_t r = it.r0 + lane; r < it.r1; r += 64) {
        const AlnRec rec = a.rec[r];
        Oriented o; uint32_t tLen, tw;
        if (!countedRecord(a.meta, a.n, a.skipExt, a.minSeqId, it.q, qm.len, rec, o, tLen, tw)) continue;
        const MapCols m = mapCols(qm, o, tLen, tw);
        nReads++; nCols += m.L; nMism += mapMismatches(a, m);
        nPrimary += a.best[rec.target] == mapKey(m.L, r);
    }
    unsigned long long *row = a.stats + (uint64_t) it.qi * 4;
    addReadsColumns(&row[0], &row[1], nReads, nCols, lane);
    const unsigned int rd = (unsigned int) cdm_wave_sum((int) nReads), pr = (unsigned int) cdm_wave_sum((int) nPrimary);       // (at most 2^20 records per item)
    const unsigned long long mm = waveSum64(nMism);
    if (lane == 0) {
        if (mm) atomicAdd(&row[2], mm);
        if (pr) atomicAdd(&row[3], (unsigned long long) pr);
        if (a.itemRecs) { a.itemRecs[item] = rd; a.itemWords[item] = mm; }
    }
}

// emission: the same items on the scanned counts.  Slot of a counted record: the item's first, the counted records of the item's
// earlier rounds of 64, the counted lanes below this one; its words likewise, by the lanes' mismatch counts.
__global__ __launch_bounds__(64 * PU_WAVES) void k_map_emit(MapArgs a, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    const uint64_t item = first + local;
    const ItemRecords it = itemRecords(a, item);
    const SeqMeta qm = a.meta[it.q];
    uint32_t slot0 = a.itemRecs[item]; uint64_t word0 = a.itemWords[item];
    for (uint64_t rb = it.r0; rb < it.r1; rb += 64) {       // (wave-uniform: the ballot and the shuffles below see all 64 lanes)
        const uint64_t r = rb + lane;
        AlnRec rec = {}; Oriented o = {0, 0, 0, 0, false}; uint32_t tLen = 0, tw = 0;
        bool counted = false;
        if (r < it.r1) { rec = a.rec[r]; counted = countedRecord(a.meta, a.n, a.skipExt, a.minSeqId, it.q, qm.len, rec, o, tLen, tw); }
        const unsigned long long live = __ballot(counted);
        if (!live) continue;
        MapCols m = mapCols(qm, o, tLen, tw);
        const uint32_t nm = counted ? mapMismatches(a, m) : 0u;
        const uint32_t upTo = cdm_wave_incl_sum<uint32_t>(nm);        // (64 records of fewer than 2^22 columns each)
        const uint32_t all = (uint32_t) __shfl((int) upTo, 63, 64);
        if (counted) {
            const uint32_t slot = slot0 + (uint32_t) __popcll(live & ((1ull << lane) - 1ull));
            uint64_t w = word0 + (upTo - nm);
            cdm_map_rec out;
            out.query = it.qi; out.target = rec.target; out.pos = m.qs; out.columns = m.L; out.tstart = m.ds; out.tlen = tLen; out.nm = nm;
            out.flags = (m.rev ? CDM_MAP_REVERSE : 0u) | (a.best[rec.target] == mapKey(m.L, r) ? 0u : CDM_MAP_SECONDARY);
            out.mm = w;
            a.recs[slot] = out;
            a.keys[slot] = (uint64_t) it.qi << MP_POS_BITS | m.qs; a.vals[slot] = slot;
            for (uint32_t c = 0; c < m.L && nm; c += 16u) {
                uint32_t qWin, tWin, qN, tN;
                for (uint32_t bits = mapMismatch16(a, m, c, qWin, tWin, qN, tN); bits; bits &= bits - 1u) {
                    const uint32_t j = (uint32_t) __ffs((int) bits) - 1u;
                    const uint32_t ref = (qN >> j) & 1u ? 4u : (qWin >> (2u * j)) & 3u, read = (tN >> j) & 1u ? 4u : (tWin >> (2u * j)) & 3u;
                    a.words[w++] = (c + j) | ref << 24 | read << 28;
                }
            }
        }
        slot0 += (uint32_t) __popcll(live); word0 += all;
    }
}

// the sorted order: a tile is DP_NT slots
struct MapGatherArgs {
    const cdm_map_rec *in; const uint32_t *order, *wordsIn;
    uint64_t *place;                // [n + 1]: nm of the record at every sorted place, after the scan its first word
    cdm_map_rec *out; uint32_t *wordsOut;
    uint32_t n, firstQuery; uint64_t firstWord;     // the batch's first listed query, the words of the batches before it
};
__global__ __launch_bounds__(DP_NT) void k_map_place(MapGatherArgs g, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i < g.n) g.place[i] = g.in[g.order[i]].nm;
}
__global__ __launch_bounds__(DP_NT) void k_map_gather(MapGatherArgs g, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i >= g.n) return;
    cdm_map_rec r = g.in[g.order[i]];
    const uint64_t to = g.place[i];
    for (uint32_t k = 0; k < r.nm; k++) g.wordsOut[to + k] = g.wordsIn[r.mm + k];
    r.query += g.firstQuery; r.mm = g.firstWord + to;
    g.out[i] = r;
}

// bits that hold the values below n
int mapBitsFor(uint64_t n) { int b = 0; while (b < 64 && (n - 1) >> b) b++; return n > 1 ? b : 0; }

}  // namespace

static int cdm_map_impl(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t nq, const cdm_map_params *par, uint64_t *stats,
                        cdm_map_rec **recs, uint64_t *nRecsOut, uint32_t **mism, uint64_t *nMismOut, float *kernelMs) {
    static const char *const WHO = "cdm_pileup_map";
    hipStream_t s = ctx->stream;
    const uint32_t chunk = pileupChunk();
    const uint64_t bound = mapBatch();
    QuerySizes qs;
    if (int rc = querySizes(ctx, db, alns, queries, nq, WHO, "record slots", qs)) return rc;
    DevBuf<unsigned long long> best;
    if (!best.alloc((size_t) db->n)) { cdm_set_error("%s: out of device memory for the primary keys of %llu sequences", WHO, (unsigned long long) db->n); return CDM_ERR_HIP; }
    CDM_HIP(hipMemsetAsync(best.p, 0, (size_t) db->n * 8, s));
    float msTotal = 0.f;
    MapArgs a;
    a.codes = db->codes; a.nmask = db->nmask; a.best = best.p; a.stats = nullptr; a.itemRecs = nullptr; a.itemWords = nullptr;
    a.recs = nullptr; a.words = nullptr; a.keys = nullptr; a.vals = nullptr;
    // the primary of every read over ALL listed queries, before any record is written (workItems takes at most 2^30 queries at a time)
    for (uint64_t b0 = 0; b0 < nq;) {
        const uint32_t m = (uint32_t) std::min<uint64_t>(nq - b0, 1ull << 30);
        WorkItems work;
        if (!work.alloc(m)) { cdm_set_error("%s: out of device memory for the work items of %u queries", WHO, m); return CDM_ERR_HIP; }
        if (int rc = workItems(s, alns, qs.dq.p + b0, m, chunk, work)) return rc;
        fillArgs(a, qs.meta.p, db, alns, par->min_seq_id, par->skip_extended_targets, work);
        hipEventRecord(ctx->ev0, s);
        launchWaveItems(s, k_map_primary, a, work.n);
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        if (int rc = finishTimed(ctx, WHO, "primary pass", msTotal)) return rc;
        b0 += m;
    }
    for (uint64_t b0 = 0; b0 < nq;) {
        // the batch: listed queries while their records stay within the bound; a single query with more goes alone
        uint32_t m = 0; uint64_t sum = 0;
        for (; b0 + m < nq && m < (1u << 30) && (m == 0 || sum + qs.recs[b0 + m] <= bound); m++) sum += qs.recs[b0 + m];
        WorkItems work; cdmscan::ScanTemp stRecs, stWords, stPlace;
        DevBuf<unsigned long long> dStats; DevBuf<uint32_t> itemRecs; DevBuf<uint64_t> itemWords;
        if (!work.alloc(m) || !dStats.alloc((size_t) m * 4)) { cdm_set_error("%s: out of device memory for %u queries", WHO, m); return CDM_ERR_HIP; }
        CDM_HIP(hipMemsetAsync(dStats.p, 0, (size_t) m * 32, s));
        if (int rc = workItems(s, alns, qs.dq.p + b0, m, chunk, work)) return rc;
        const uint64_t nItems = work.n;
        fillArgs(a, qs.meta.p, db, alns, par->min_seq_id, par->skip_extended_targets, work);
        a.stats = dStats.p; a.itemRecs = nullptr; a.itemWords = nullptr;
        if (recs) {
            if (!itemRecs.alloc((size_t) nItems + 1) || !itemWords.alloc((size_t) nItems + 1)) { cdm_set_error("%s: out of device memory for %llu work items", WHO, (unsigned long long) nItems); return CDM_ERR_HIP; }
            CDM_HIP(hipMemsetAsync(itemRecs.p + nItems, 0, 4, s));          // (the closing words: the scans leave the batch's totals there)
            CDM_HIP(hipMemsetAsync(itemWords.p + nItems, 0, 8, s));
            a.itemRecs = itemRecs.p; a.itemWords = itemWords.p;
        }
        uint32_t nRec = 0; uint64_t nWords = 0;
        hipEventRecord(ctx->ev0, s);
        launchWaveItems(s, k_map_count, a, nItems);
        if (recs) {
            if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stRecs, itemRecs.p, itemRecs.p, (size_t) nItems + 1)) return rc;        // (in place: scan.h)
            if (int rc = cdmscan::exclusiveScan<uint64_t>(s, stWords, itemWords.p, itemWords.p, (size_t) nItems + 1)) return rc;
            CDM_HIP(hipMemcpyAsync(&nRec, itemRecs.p + nItems, 4, hipMemcpyDeviceToHost, s));
            CDM_HIP(hipMemcpyAsync(&nWords, itemWords.p + nItems, 8, hipMemcpyDeviceToHost, s));
        }
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        CDM_HIP(hipMemcpyAsync(stats + b0 * 4, dStats.p, (size_t) m * 32, hipMemcpyDeviceToHost, s));
        if (int rc = finishTimed(ctx, WHO, "counting", msTotal)) return rc;
        if (nRec) {     // the records of this batch behind those of the batches before it
            DevBuf<cdm_map_rec> placed, sorted; DevBuf<uint32_t> words, wordsSorted, v0, v1; DevBuf<uint64_t> k0, k1, place;
            if (!placed.alloc(nRec) || !sorted.alloc(nRec) || !words.alloc((size_t) nWords) || !wordsSorted.alloc((size_t) nWords) || !v0.alloc(nRec) || !v1.alloc(nRec) || !k0.alloc(nRec) ||
                !k1.alloc(nRec) || !place.alloc((size_t) nRec + 1)) {
                cdm_set_error("%s: out of device memory for %u records and %llu mismatch words", WHO, nRec, (unsigned long long) nWords); return CDM_ERR_HIP;
            }
            a.recs = placed.p; a.words = words.p; a.keys = k0.p; a.vals = v0.p;
            CDM_HIP(hipMemsetAsync(place.p + nRec, 0, 8, s));
            hipEventRecord(ctx->ev0, s);
            launchWaveItems(s, k_map_emit, a, nItems);
            bool inFirst = true;        // stable on the query and position bits in use; the slots come in alignment-set order
            if (int rc = rx::sortPairs<uint64_t, uint32_t>(s, ctx->cuCount, k0.p, k1.p, v0.p, v1.p, (uint64_t) nRec, 0, MP_POS_BITS + mapBitsFor(m), inFirst)) return rc;
            MapGatherArgs g;
            g.in = placed.p; g.order = inFirst ? v0.p : v1.p; g.wordsIn = words.p; g.place = place.p; g.out = sorted.p; g.wordsOut = wordsSorted.p;
            g.n = nRec; g.firstQuery = (uint32_t) b0; g.firstWord = *nMismOut;
            const uint64_t nTiles = ((uint64_t) nRec + DP_NT - 1) / DP_NT;
            launchTiles(s, k_map_place, g, nTiles);
            if (int rc = cdmscan::exclusiveScan<uint64_t>(s, stPlace, place.p, place.p, (size_t) nRec + 1)) return rc;       // (in place)
            launchTiles(s, k_map_gather, g, nTiles);
            hipEventRecord(ctx->ev1, s);
            CDM_LAUNCH_CHECK();
            if (int rc = appendRecords(s, WHO, "map", recs, nRecsOut, (const cdm_map_rec *) sorted.p, nRec)) return rc;
            for (uint64_t at = 0; at < nWords;) {       // (appendRecords takes fewer than 2^32 at a time)
                const uint32_t nThis = (uint32_t) std::min<uint64_t>(nWords - at, 1ull << 31);
                if (int rc = appendRecords(s, WHO, "mismatch", mism, nMismOut, (const uint32_t *) wordsSorted.p + at, nThis)) return rc;
                at += nThis;
            }
            if (int rc = finishTimed(ctx, WHO, "emission", msTotal)) return rc;
        }
        b0 += m;
    }
    if (kernelMs) *kernelMs = msTotal;
    return CDM_OK;
}

extern "C" int cdm_pileup_map(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_map_params *par, uint64_t *stats,
                              cdm_map_rec **recs, uint64_t *n_recs, uint32_t **mism, uint64_t *n_mism, float *kernel_ms) {
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, "cdm_pileup_map");
    if (!ctx || !db || !alns || !par || (recs && (!n_recs || !mism || !n_mism)) || (!recs && mism) || (n_queries && (!queries || !stats))) { cdm_set_error("cdm_pileup_map: NULL argument"); return CDM_ERR_INVALID; }
    if (int rc = pileupCheckArgs("cdm_pileup_map", db, alns, queries, n_queries)) return rc;
    if (alns->count >> MP_INDEX_BITS) {
        cdm_set_error("cdm_pileup_map: the set has %llu records; the primary key holds a record's index in %d bits", (unsigned long long) alns->count, MP_INDEX_BITS); return CDM_ERR_UNSUPPORTED;
    }
    if (mism) { *mism = NULL; *n_mism = 0; }
    uint32_t *words = NULL; uint64_t nWords = 0;
    const int rc = runWithRecords(ctx, n_queries, recs, n_recs, kernel_ms, [&](cdm_map_rec **got, uint64_t *nGot, float *ms) {
        return cdm_map_impl(ctx, db, alns, queries, n_queries, par, stats, got, nGot, got ? &words : (uint32_t **) NULL, &nWords, ms);
    });
    if (rc == CDM_OK && mism) { *mism = words; *n_mism = nWords; } else free(words);
    return rc;
}

extern "C" void cdm_map_free(cdm_map_rec *recs, uint32_t *mism) { free(recs); free(mism); }
