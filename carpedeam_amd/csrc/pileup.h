// What the reductions over the read pile-up (pileup.hip: cdm_pileup_profile; pileup_depth.hip: cdm_pileup_depth and
// cdm_pileup_breaks; pileup_bases.hip: cdm_pileup_bases; pileup_map.hip: cdm_pileup_map; pileup_links.hip: cdm_pileup_links; pileup_junctions.hip: cdm_pileup_junctions) and
// cdm_alns_dedup (pileup_dedup.hip), which takes the duplicate reads out of the set they reduce, share: the rule by which a record counts, the
// work items (listed query, chunk of its records) and the tiles (listed query, DP_TILE positions) with their lookups, and the host
// steps of a call - query sizes, batch cut, work items, sliced launches, the timed synchronisation, the caller's record array - and
// what the users of cdm_pileup_gapped's records share: the walk over a record's operations and the host's check of them.  Every step
// is defined here once.
#pragma once
#include <algorithm>
#include <vector>

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
constexpr int DP_NT = 256, DP_PER = 8, DP_TILE = DP_NT * DP_PER;       // positions per tile

// a count from the library's snapshot of the environment: the positive value of `name`, at most `most`, or dflt
uint64_t envCount(const char *name, uint64_t dflt, uint64_t most) {
    if (const char *e = cdmGetenv(name)) { const long long v = atoll(e); if (v > 0) return std::min<uint64_t>((uint64_t) v, most); }
    return dflt;
}
uint32_t pileupChunk() { return (uint32_t) envCount("CDM_PILEUP_CHUNK", PU_CHUNK_DEFAULT, PU_CHUNK_MAX); }

// what every kernel over work items reads; the per-call argument structs derive from it
struct ItemArgs {
    const SeqMeta *meta; const uint64_t *aoff; const AlnRec *rec;
    const uint32_t *queries;        // [nq] the listed queries of this call's batch
    const uint64_t *itemOff;        // [nq + 1] first work item (chunk of records) of each listed query
    uint32_t n, nq, chunk, skipExt; float minSeqId;
};
struct TiledArgs : ItemArgs {       // and what the calls with tiles add
    const uint64_t *tileOff;        // [nq + 1] first tile of each listed query
    const uint64_t *base;           // [nq + 1] first cell (position) of each in a plane
};

// work items per listed query: its records in chunks
__global__ void k_pileup_chunks(const uint64_t *__restrict__ aoff, const uint32_t *__restrict__ queries, uint32_t nq, uint32_t chunk, uint64_t *__restrict__ items) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nq) return;
    uint64_t c = 0;
    if (i < nq) { const uint32_t q = queries[i]; c = (aoff[q + 1] - aoff[q] + chunk - 1) / chunk; }
    items[i] = c;
}

// length and record count of every listed query
__global__ void k_depth_sizes(const SeqMeta *__restrict__ meta, const uint64_t *__restrict__ aoff, const uint32_t *__restrict__ queries, uint64_t nq, uint32_t *__restrict__ len,
                              uint64_t *__restrict__ recs) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const uint32_t q = queries[i];
    len[i] = meta[q].len; recs[i] = aoff[q + 1] - aoff[q];
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

// the listed query that owns an item: the last i < nq with off[i] <= item (a query without items owns none)
__device__ __forceinline__ uint32_t ownerOf(const uint64_t *__restrict__ off, uint32_t nq, uint64_t item) {
    uint32_t lo = 0, hi = nq;
    while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (off[mid] <= item) lo = mid; else hi = mid; }
    return lo;
}
// a work item: the listed query qi = query q of the DB, and its records [r0, r1)
struct ItemRecords { uint32_t qi, q; uint64_t r0, r1; };
__device__ __forceinline__ ItemRecords itemRecords(const ItemArgs &a, uint64_t item) {
    ItemRecords it;
    it.qi = ownerOf(a.itemOff, a.nq, item); it.q = a.queries[it.qi];
    it.r0 = a.aoff[it.q] + (item - a.itemOff[it.qi]) * a.chunk; it.r1 = min((uint64_t) a.aoff[it.q + 1], it.r0 + a.chunk);
    return it;
}
// a tile: DP_TILE positions from p0 of the listed query qi of `len` letters at word `woff`, whose cells start at `base` in a plane
struct Tile { uint32_t qi, len, woff; uint64_t base, p0; };
__device__ __forceinline__ Tile tileOf(const TiledArgs &a, uint64_t item) {
    Tile t;
    t.qi = ownerOf(a.tileOff, a.nq, item);
    const SeqMeta qm = a.meta[a.queries[t.qi]];
    t.len = qm.len; t.woff = qm.woff; t.base = a.base[t.qi]; t.p0 = (item - a.tileOff[t.qi]) * DP_TILE;
    return t;
}

// the counted records of a wave's item and their columns, added to the query's two totals once per item
__device__ __forceinline__ void addReadsColumns(unsigned long long *reads, unsigned long long *columns, unsigned int nReads, unsigned long long nCols, int lane) {
    const unsigned int rd = (unsigned int) cdm_wave_sum((int) nReads);      // (at most 2^20 records per item)
    const unsigned long long cl = waveSum64(nCols);
    if (lane == 0 && rd) { atomicAdd(reads, (unsigned long long) rd); atomicAdd(columns, cl); }
}

// ---------------------------------------------------------------------------------------------- gapped records
// What the users of cdm_pileup_gapped's records share (pileup_indels.hip: cdm_pileup_indels; pileup_depth.hip and pileup_bases.hip:
// the three *_gapped reductions): the operation codes, the walk over a record's operations, and further down the host's check.
constexpr uint32_t ID_MAX_GAP = 62;         // letters of an I or D: 2 x the largest band
constexpr uint32_t ID_OP_M = 0, ID_OP_I = 1, ID_OP_D = 2;

// The walk over a gapped record's operations from p = pos and off = tstart: match(p, off, g) for every M of g letters - column j < g
// sits on query position p + j with the read's oriented offset off + j -, event(p, kind, g, off) for every I and D.
// indelCheckRecords: n_ops words inside the pool, M + D = span, M + I = columns
template <class Match, class Event> __device__ __forceinline__ void gappedWalk(const cdm_gap_rec &r, const uint32_t *__restrict__ ops, Match match, Event event) {
    uint32_t p = r.pos, off = r.tstart;
    for (uint32_t j = 0; j < r.n_ops; j++) {
        const uint32_t w = ops[r.ops + j], g = w >> 2, op = w & 3u;
        if (op == ID_OP_M) { match(p, off, g); p += g; off += g; }
        else if (op == ID_OP_I) { event(p, ID_OP_I, g, off); off += g; }
        else { event(p, ID_OP_D, g, off); p += g; }
    }
}
// the I and D operations alone
template <class Event> __device__ __forceinline__ void indelWalk(const cdm_gap_rec &r, const uint32_t *__restrict__ ops, Event event) {
    gappedWalk(r, ops, [](uint32_t, uint32_t, uint32_t) {}, event);
}

// ---------------------------------------------------------------------------------------------- host
// One pass over the caller's gapped records and their operation words (include/carpedeam_hip.h): CDM_OK, or CDM_ERR_INVALID with the
// first record that fails.  qLen: the listed queries' lengths; tLen: the length of every sequence of the DB.
int indelCheckRecords(const char *who, const cdm_gap_rec *recs, uint64_t nRecs, const uint32_t *ops, uint64_t nOps, const std::vector<uint32_t> &qLen, const std::vector<uint32_t> &tLen) {
    for (uint64_t i = 0; i < nRecs; i++) {
        const cdm_gap_rec &r = recs[i];
        auto bad = [&](const char *what) { cdm_set_error("%s: gapped record %llu: %s", who, (unsigned long long) i, what); return CDM_ERR_INVALID; };
        if (r.query >= qLen.size()) return bad("its query is not an index into the listed queries");
        if (r.target >= tLen.size()) return bad("its target is not a sequence of the DB");
        if (r.tlen != tLen[r.target]) return bad("tlen is not the length of its target");
        if (i && (r.query < recs[i - 1].query || (r.query == recs[i - 1].query && r.pos < recs[i - 1].pos))) return bad("the records do not ascend by (query, pos)");
        if (r.n_ops < 1 || r.ops > nOps || r.n_ops > nOps - r.ops) return bad("its operations are not words of the pool");
        uint64_t span = 0, columns = 0;
        for (uint32_t j = 0; j < r.n_ops; j++) {
            const uint32_t w = ops[r.ops + j], g = w >> 2, op = w & 3u;
            if (op > ID_OP_D || g < 1) return bad("an operation that is not M, I or D of at least one letter");
            if ((j == 0 || j + 1 == r.n_ops) && op != ID_OP_M) return bad("its first or last operation is not M");
            if (j && (ops[r.ops + j - 1] & 3u) == op) return bad("two neighbouring operations of one code");
            if (op != ID_OP_M && g > ID_MAX_GAP) return bad("an insertion or deletion of more than 62 letters");
            if (op != ID_OP_I) span += g;
            if (op != ID_OP_D) columns += g;
        }
        if (span != r.span || columns != r.columns) return bad("its operations do not sum to span and columns");
        if ((uint64_t) r.pos + r.span > qLen[r.query]) return bad("pos + span lies beyond its query");
        if ((uint64_t) r.tstart + r.columns > r.tlen) return bad("tstart + columns lies beyond its target");
    }
    return CDM_OK;
}

// The caller's gapped records of a call, as the host sequences take them.  check(): the records against the DB's lengths, before
// anything else goes to the device or is launched - the lengths come down in one plain copy.  upload(): both arrays in the stream.
// end(): the records are sorted by listed query, so those of the batch of listed queries in front of q1 are the range [g0, end(g0, q1)).
struct GappedRecords {
    const cdm_gap_rec *recs = nullptr; uint64_t nRecs = 0; const uint32_t *ops = nullptr; uint64_t nOps = 0;
    DevBuf<cdm_gap_rec> dRecs; DevBuf<uint32_t> dOps;
    int check(const char *who, const cdm_seqdb *db, const uint32_t *queries, uint64_t nq) const {
        if (!nRecs) return CDM_OK;
        std::vector<uint32_t> tLen(db->n), qLen(nq);
        CDM_HIP(hipMemcpy(tLen.data(), db->len, (size_t) db->n * 4, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < nq; i++) qLen[i] = tLen[queries[i]];
        return indelCheckRecords(who, recs, nRecs, ops, nOps, qLen, tLen);
    }
    int upload(hipStream_t s, const char *who) {
        if (!nRecs) return CDM_OK;
        if (!dRecs.alloc(nRecs) || !dOps.alloc(nOps)) { cdm_set_error("%s: out of device memory for %llu gapped records and %llu operations", who, (unsigned long long) nRecs, (unsigned long long) nOps); return CDM_ERR_HIP; }
        CDM_HIP(hipMemcpyAsync(dRecs.p, recs, (size_t) nRecs * sizeof(cdm_gap_rec), hipMemcpyHostToDevice, s));
        CDM_HIP(hipMemcpyAsync(dOps.p, ops, (size_t) nOps * 4, hipMemcpyHostToDevice, s));
        return CDM_OK;
    }
    uint64_t end(uint64_t g0, uint64_t q1) const { while (g0 < nRecs && recs[g0].query < q1) g0++; return g0; }
    // a listed query whose ungapped plus gapped records reach 2^32 is refused (the 32-bit `what` hold fewer)
    int checkCounts(const char *who, const char *what, const uint32_t *queries, const std::vector<uint64_t> &ungapped) const {
        for (uint64_t g = 0; g < nRecs;) {
            const uint64_t q = recs[g].query, g1 = end(g, q + 1);
            if ((ungapped[q] + (g1 - g)) >> 32) { cdm_set_error("%s: query %u has %llu records; the 32-bit %s hold fewer than 2^32", who, queries[q], (unsigned long long) (ungapped[q] + (g1 - g)), what); return CDM_ERR_UNSUPPORTED; }
            g = g1;
        }
        return CDM_OK;
    }
};

// the argument checks the entry points share
int pileupCheckArgs(const char *who, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries) {
    if (alns->n != db->n) { cdm_set_error("%s: alignment CSR has %llu queries, DB has %llu", who, (unsigned long long) alns->n, (unsigned long long) db->n); return CDM_ERR_INVALID; }
    if (db->residues && !db->codes) { cdm_set_error("%s: the DB holds no letters (an index copy)", who); return CDM_ERR_INVALID; }
    std::vector<uint32_t> sorted(queries, queries + n_queries);
    std::sort(sorted.begin(), sorted.end());
    if (n_queries && sorted.back() >= db->n) { cdm_set_error("%s: query index %u of a DB of %llu sequences", who, sorted.back(), (unsigned long long) db->n); return CDM_ERR_INVALID; }
    for (uint64_t i = 1; i < n_queries; i++)
        if (sorted[i] == sorted[i - 1]) { cdm_set_error("%s: query index %u is listed twice", who, sorted[i]); return CDM_ERR_INVALID; }
    return CDM_OK;
}

// (a) The DB's metadata and the listed queries on the device, the queries' lengths and record counts on the host; a query with 2^32
// records or more is refused (the 32-bit `what` of `who` hold fewer).  One stream synchronisation behind cdm_build_meta's own.
struct QuerySizes { DevBuf<SeqMeta> meta; DevBuf<uint32_t> dq; std::vector<uint32_t> len; std::vector<uint64_t> recs; };
int querySizes(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t nq, const char *who, const char *what, QuerySizes &qs) {
    hipStream_t s = ctx->stream;
    if (int rc = cdm_build_meta(ctx, db, &qs.meta.p)) return rc;
    DevBuf<uint32_t> dLen; DevBuf<uint64_t> dRecs;
    if (!qs.dq.alloc(nq) || !dLen.alloc(nq) || !dRecs.alloc(nq)) { cdm_set_error("%s: out of device memory for %llu queries", who, (unsigned long long) nq); return CDM_ERR_HIP; }
    qs.len.resize(nq); qs.recs.resize(nq);
    std::vector<uint64_t> &recs = qs.recs;
    CDM_HIP(hipMemcpyAsync(qs.dq.p, queries, (size_t) nq * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_depth_sizes, CDM_GRID((nq + 255) / 256, 256), dim3(256), 0, s, (const SeqMeta *) qs.meta.p, (const uint64_t *) alns->off, (const uint32_t *) qs.dq.p, nq, dLen.p, dRecs.p);
    CDM_LAUNCH_CHECK();
    CDM_HIP(hipMemcpyAsync(qs.len.data(), dLen.p, (size_t) nq * 4, hipMemcpyDeviceToHost, s));
    CDM_HIP(hipMemcpyAsync(recs.data(), dRecs.p, (size_t) nq * 8, hipMemcpyDeviceToHost, s));
    CDM_HIP(hipStreamSynchronize(s));
    for (uint64_t i = 0; i < nq; i++)
        if (recs[i] >> 32) { cdm_set_error("%s: query %u has %llu records; the 32-bit %s hold fewer than 2^32", who, queries[i], (unsigned long long) recs[i], what); return CDM_ERR_UNSUPPORTED; }
    return CDM_OK;
}

// (b) The batch that starts at listed query b0: the queries that follow while the sum of cost(len) stays within the bound (a single
// query beyond the bound goes alone), each with len + closing cells in a plane.  No synchronisation: upload() is ordered in the
// stream in front of the kernels that read the two arrays.
struct BatchPlan {
    uint32_t m = 0; uint64_t cells = 0, nTiles = 0;     // listed queries of the batch, cells of a plane, tiles
    std::vector<uint64_t> base, tileOff;                // [m + 1] (kept until the copies of upload() have run)
    DevBuf<uint64_t> dBase, dTile;
    template <class Cost> void cut(const std::vector<uint32_t> &len, uint64_t b0, uint32_t closing, Cost cost, uint64_t bound) {
        const uint64_t nq = len.size();
        uint64_t sum = 0;
        for (m = 0; b0 + m < nq && m < (1u << 30) && (m == 0 || sum + cost((uint64_t) len[b0 + m]) <= bound); m++) sum += cost((uint64_t) len[b0 + m]);
        base.assign((size_t) m + 1, 0); tileOff.assign((size_t) m + 1, 0);
        for (uint32_t i = 0; i < m; i++) { base[i + 1] = base[i] + len[b0 + i] + closing; tileOff[i + 1] = tileOff[i] + ((uint64_t) len[b0 + i] + DP_TILE - 1) / DP_TILE; }
        cells = base[m]; nTiles = tileOff[m];
    }
    bool alloc() { return dBase.alloc((size_t) m + 1) && dTile.alloc((size_t) m + 1); }
    int upload(hipStream_t s) {
        CDM_HIP(hipMemcpyAsync(dBase.p, base.data(), ((size_t) m + 1) * 8, hipMemcpyHostToDevice, s));
        CDM_HIP(hipMemcpyAsync(dTile.p, tileOff.data(), ((size_t) m + 1) * 8, hipMemcpyHostToDevice, s));
        return CDM_OK;
    }
};

// (c) The work items of the m listed queries at dq: k_pileup_chunks, the scan, the number of items.  One stream synchronisation.
// off: the CSR whose rows are cut into items - the alignment set's, or (cdm_pileup_gapped) the hit set's.
struct WorkItems {
    DevBuf<uint64_t> items, itemOff; cdmscan::ScanTemp st;
    const uint32_t *queries = nullptr; uint32_t m = 0, chunk = 0; uint64_t n = 0;       // n: work items
    bool alloc(uint32_t nq) { return items.alloc((size_t) nq + 1) && itemOff.alloc((size_t) nq + 1); }
};
int workItems(hipStream_t s, const uint64_t *off, const uint32_t *dq, uint32_t m, uint32_t chunk, WorkItems &w) {
    w.queries = dq; w.m = m; w.chunk = chunk;
    hipLaunchKernelGGL(k_pileup_chunks, dim3((m + 256) / 256), dim3(256), 0, s, off, dq, m, chunk, w.items.p);
    if (int rc = cdmscan::exclusiveScan<uint64_t>(s, w.st, w.items.p, w.itemOff.p, (size_t) m + 1)) return rc;
    CDM_HIP(hipMemcpyAsync(&w.n, w.itemOff.p + m, 8, hipMemcpyDeviceToHost, s));
    CDM_HIP(hipStreamSynchronize(s));
    return CDM_OK;
}
int workItems(hipStream_t s, const cdm_alns *alns, const uint32_t *dq, uint32_t m, uint32_t chunk, WorkItems &w) { return workItems(s, (const uint64_t *) alns->off, dq, m, chunk, w); }

// the shared part of a call's kernel arguments
void fillArgs(ItemArgs &a, const SeqMeta *meta, const cdm_seqdb *db, const cdm_alns *alns, float minSeqId, int skipExtended, const WorkItems &w) {
    a.meta = meta; a.aoff = alns->off; a.rec = alns->rec; a.queries = w.queries; a.itemOff = w.itemOff.p;
    a.n = (uint32_t) db->n; a.nq = w.m; a.chunk = w.chunk; a.skipExt = skipExtended ? 1u : 0u; a.minSeqId = minSeqId;
}
void fillArgs(TiledArgs &a, const SeqMeta *meta, const cdm_seqdb *db, const cdm_alns *alns, float minSeqId, int skipExtended, const WorkItems &w, const BatchPlan &p) {
    fillArgs(static_cast<ItemArgs &>(a), meta, db, alns, minSeqId, skipExtended, w);
    a.tileOff = p.dTile.p; a.base = p.dBase.p;
}

// (d) The launches of a batch in slices of at most 2^31 threads: kernel(args, first, nThis) with one wave per work item of the slice
// [first, first + nThis), kernel(args, first) with one block of DP_NT threads per tile
template <class Args> void launchWaveItems(hipStream_t s, void (*kernel)(Args, uint64_t, uint64_t), const Args &a, uint64_t nItems, size_t ldsBytes = 0) {
    for (uint64_t first = 0, slice = cdmSliceItems(64); first < nItems; first += slice) {
        const uint64_t nThis = std::min<uint64_t>(slice, nItems - first);
        hipLaunchKernelGGL(kernel, CDM_GRID((nThis + PU_WAVES - 1) / PU_WAVES, 64 * PU_WAVES), dim3(64 * PU_WAVES), ldsBytes, s, a, first, nThis);
    }
}
template <class Args> void launchTiles(hipStream_t s, void (*kernel)(Args, uint64_t), const Args &a, uint64_t nTiles) {
    for (uint64_t first = 0, slice = cdmSliceItems(DP_NT); first < nTiles; first += slice) {
        const uint64_t nThis = std::min<uint64_t>(slice, nTiles - first);
        hipLaunchKernelGGL(kernel, CDM_GRID(nThis, DP_NT), dim3(DP_NT), 0, s, a, first);
    }
}

// (e) Synchronise the stream ("<who>: the <what> failed"); timed: the time between the context's two events is added to ms
int finishTimed(cdm_ctx *ctx, const char *who, const char *what, float &ms, bool timed = true) {
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { cdm_set_error("%s: the %s failed: %s", who, what, hipGetErrorString(e)); return CDM_ERR_HIP; }
    float t = 0.f;
    if (timed && hipEventElapsedTime(&t, ctx->ev0, ctx->ev1) == hipSuccess) ms += t;
    return CDM_OK;
}

// (f) nNew records of a batch from the device behind the *n the caller's array holds already (a copy in the stream: synchronise
// before the device array goes)
template <class T> int appendRecords(hipStream_t s, const char *who, const char *what, T **recs, uint64_t *n, const T *dNew, uint32_t nNew) {
    T *grown = (T *) realloc(*recs, (size_t) (*n + nNew) * sizeof(T));
    if (!grown) { cdm_set_error("%s: out of host memory for %llu %s records", who, (unsigned long long) (*n + nNew), what); return CDM_ERR_INVALID; }
    *recs = grown;
    CDM_HIP(hipMemcpyAsync(grown + *n, dNew, (size_t) nNew * sizeof(T), hipMemcpyDeviceToHost, s));
    *n += nNew;
    return CDM_OK;
}
// the tail of an entry point that hands out a record array: run(got, nGot, kernel_ms) fills it, and it is the caller's only on success
template <class T, class Run> int runWithRecords(cdm_ctx *ctx, uint64_t n_queries, T **recs, uint64_t *n_recs, float *kernel_ms, Run run) {
    if (recs) { *recs = NULL; *n_recs = 0; }
    if (kernel_ms) *kernel_ms = 0.f;
    if (n_queries == 0) return CDM_OK;
    CDM_HIP(hipSetDevice(ctx->device));
    T *got = NULL; uint64_t nGot = 0;
    const int rc = run(recs ? &got : (T **) NULL, &nGot, kernel_ms);
    if (rc == CDM_OK && recs) { *recs = got; *n_recs = nGot; } else free(got);
    return rc;
}

}  // namespace
