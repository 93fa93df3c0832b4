// Per-position base counts and variant sites of the read pile-up (cdm_pileup_bases; not a module of the reference): which bases the
// reads put on every position of the listed queries, and the positions where they disagree with the query or among themselves
// (include/carpedeam_hip.h).  What it shares with the other reductions over the read pile-up is in pileup.h.  Unlike the profile
// (pileup.hip) and the depth (pileup_depth.hip) this one walks EVERY column of every counted record, so the
// lanes of a wave take the columns of ONE record, not records: a wave instruction then reads one or two read code words per 16 lanes and
// adds to consecutive words.  The batch's counters are eight planes [forward A,C,G,T, reverse A,C,G,T][position]: the lanes of one
// instruction that carry the same base add to a contiguous run of one plane (an interleaved [position][8] table would touch one word
// in each of 64 separate 32-byte cells).  A second kernel reads the planes by tiles of positions, classifies, reduces the query's
// figures and marks the flagged positions; one prefix sum over the marks places the site records, which a third kernel writes.
// cdm_pileup_bases_gapped is the same host sequence with the caller's gapped records (cdm_pileup_gapped's) counted into the same planes
// by k_base_counts_gapped.
#include "pileup.h"

namespace {

constexpr uint64_t BS_POS_DEFAULT = 1ull << 25;         // positions per batch: 2^25 x 8 planes x 4 bytes = 1 GB
constexpr int BS_MAX_MASK = 64;

// CDM_BASES_POSITIONS=<positions> (tests): small inputs in several batches
uint64_t basesPositions() { return envCount("CDM_BASES_POSITIONS", BS_POS_DEFAULT, BS_POS_DEFAULT); }

struct BasesArgs : TiledArgs {      // (items: counting; tiles: classification and emission)
    const uint32_t *codes, *nmask;
    uint32_t maskEnds, minDepth, minAlt, minPct, firstQuery;
    uint64_t nPos;                  // positions of the batch: the length of a plane
    uint32_t *planes;               // [8][nPos]
    unsigned long long *stats;      // [nq][8]
    uint32_t *place;                // [nPos + 1]: 0/1 per flagged position, after the scan the position's first site record
    uint32_t *counts;               // NULL, or [nPos][8]
    cdm_site *sites;                // k_base_emit: [place[nPos]]
    const cdm_gap_rec *grec;        // cdm_pileup_bases_gapped: the batch's gapped records [nG] (query: the index into the call's list)
    const uint32_t *gops;           // the caller's whole operation pool
    uint32_t nG;
};
// counting: one wave per item (listed query, chunk of its records) of this launch's slice.  Each lane loads one record and evaluates
// the filter; the wave then walks the counted records one at a time, its lanes on the columns lane, lane + 64, ...
__global__ __launch_bounds__(64 * PU_WAVES) void k_base_counts(BasesArgs a, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    const ItemRecords it = itemRecords(a, first + local);
    const uint32_t qi = it.qi, q = it.q, qLen = a.meta[q].len, m = a.maskEnds;
    uint32_t *__restrict__ plane0 = a.planes + a.base[qi];
    unsigned int nReads = 0; unsigned long long nCols = 0;
    for (uint64_t rb = it.r0; rb < it.r1; rb += 64) {       // (wave-uniform: the shuffles below see all 64 lanes)
        Oriented o = {0, 0, 0, 0, false}; uint32_t tLen = 0, tw = 0;
        bool counted = false;
        if (rb + lane < it.r1) { const AlnRec rec = a.rec[rb + lane]; counted = countedRecord(a.meta, a.n, a.skipExt, a.minSeqId, q, qLen, rec, o, tLen, tw); }
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
    addReadsColumns(&a.stats[(uint64_t) qi * 8], &a.stats[(uint64_t) qi * 8 + 1], nReads, nCols, lane);
}

// The gapped records (cdm_pileup_bases_gapped; include/carpedeam_hip.h) into the same planes: one wave per item of 64 records of this
// launch's slice.  Each lane loads one record; the wave then walks the records one at a time, their fields broadcast, the operation
// words loaded wave-uniformly, and for every M operation the lanes take its columns lane, lane + 64, ... - what k_base_counts does
// with the columns of an ungapped record.  An inserted letter has no query position and a deleted one no read letter: neither counts.
// reads and columns (the M columns) go to the query's stats row once per wave where its records share a query - they are sorted by
// query -, else once per record.  indelCheckRecords (pileup.h): pos + span <= the query's length, tstart + columns <= tlen = the
// target's length and the operation words lie in the pool, below 2^31 of them, so every index below stays inside the query's planes,
// the read's words and the pool.
__global__ __launch_bounds__(64 * PU_WAVES) void k_base_counts_gapped(BasesArgs a, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    const uint64_t rb = (first + local) * 64;
    const bool have = rb + lane < a.nG;
    const uint32_t m = a.maskEnds;
    uint32_t myQi = 0, myPos = 0, myOff = 0, myLen = 0, myW = 0, myRev = 0, myOps = 0, myN = 0, myCols = 0;
    if (have) {
        const cdm_gap_rec r = a.grec[rb + lane];
        myQi = r.query - a.firstQuery; myPos = r.pos; myOff = r.tstart; myLen = r.tlen; myW = a.meta[r.target].woff; myRev = r.flags & CDM_MAP_REVERSE ? 1u : 0u;
        myOps = (uint32_t) r.ops; myN = r.n_ops;
    }
    const unsigned long long all = __ballot(have);
    for (unsigned long long live = all; live; live &= live - 1) {       // (wave-uniform: the shuffles below see all 64 lanes)
        const int src = __ffsll((long long) live) - 1;
        const uint32_t qi = __shfl(myQi, src, 64), len = __shfl(myLen, src, 64), w = __shfl(myW, src, 64), rev = __shfl(myRev, src, 64);
        const uint32_t o0 = __shfl(myOps, src, 64), n = __shfl(myN, src, 64);
        uint32_t p = __shfl(myPos, src, 64), off = __shfl(myOff, src, 64), cols = 0;
        uint32_t *__restrict__ plane0 = a.planes + a.base[qi];
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t word = a.gops[__builtin_amdgcn_readfirstlane(o0 + j)], g = word >> 2, op = word & 3u;
            if (op == ID_OP_M) {
                for (uint32_t c = lane; c < g; c += 64) {
                    const uint32_t oc = off + c, rp = rev ? len - 1u - oc : oc;       // the position in the read's own orientation
                    if (cdm_isN(a.nmask, w, rp)) continue;
                    if (m && (rp < m || len - 1u - rp < m)) continue;
                    uint32_t b = cdm_base(a.codes, w, rp);
                    if (rev) b = 3u - b;                  // the read base as the query's strand sees it
                    atomicAdd(&plane0[(uint64_t) (rev * 4u + b) * a.nPos + p + c], 1u);     // (result unused: an atomic without return)
                }
                p += g; off += g; cols += g;
            } else if (op == ID_OP_I) off += g;
            else p += g;
        }
        if (lane == src) myCols = cols;
    }
    const uint32_t qi0 = __shfl(myQi, __ffsll((long long) all) - 1, 64);        // (local < nThis: the item holds a record)
    if (!__ballot(have && myQi != qi0)) addReadsColumns(&a.stats[(uint64_t) qi0 * 8], &a.stats[(uint64_t) qi0 * 8 + 1], have ? 1u : 0u, (unsigned long long) myCols, lane);
    else if (have) { atomicAdd(&a.stats[(uint64_t) myQi * 8], 1ull); atomicAdd(&a.stats[(uint64_t) myQi * 8 + 1], (unsigned long long) myCols); }
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

__device__ __forceinline__ SiteCall callAt(const BasesArgs &a, const Tile &t, uint32_t p, uint32_t c[8]) {
#pragma unroll
    for (int k = 0; k < 8; k++) c[k] = a.planes[(uint64_t) k * a.nPos + t.base + p];
    const uint32_t ref = cdm_isN(a.nmask, t.woff, p) ? 4u : cdm_base(a.codes, t.woff, p);
    return callSite(c, ref, a.minDepth, a.minAlt, a.minPct);
}

// classification: one block per item (listed query, tile of DP_TILE positions) of this launch's slice
__global__ __launch_bounds__(DP_NT) void k_base_sites(BasesArgs a, uint64_t first) {
    __shared__ unsigned long long sRed[DP_NT / 64][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Tile t = tileOf(a, first + blockIdx.x);
    unsigned long long bases = 0, mism = 0, four = 0;       // four: called, differs, variable, flagged in 16 bits each (at most DP_TILE)
#pragma unroll
    for (int j = 0; j < DP_PER; j++) {
        const uint64_t p = t.p0 + threadIdx.x + (uint64_t) DP_NT * j;
        if (p >= t.len) continue;
        uint32_t c[8];
        const SiteCall s = callAt(a, t, (uint32_t) p, c);
        if (a.counts) {
            uint4 *row = reinterpret_cast<uint4 *>(a.counts + (t.base + p) * 8);
            row[0] = make_uint4(c[0], c[1], c[2], c[3]); row[1] = make_uint4(c[4], c[5], c[6], c[7]);
        }
        const uint32_t fl = (s.flags & (CDM_SITE_DIFFERS | CDM_SITE_VARIABLE)) != 0;
        a.place[t.base + p] = fl;
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
    const Tile t = tileOf(a, first + blockIdx.x);
#pragma unroll
    for (int j = 0; j < DP_PER; j++) {
        const uint64_t p = t.p0 + threadIdx.x + (uint64_t) DP_NT * j;
        if (p >= t.len) continue;
        const uint32_t at = a.place[t.base + p];
        if (a.place[t.base + p + 1] == at) continue;
        uint32_t c[8];
        const SiteCall s = callAt(a, t, (uint32_t) p, c);
        cdm_site *out = a.sites + at;
        out->query = a.firstQuery + t.qi; out->pos = (uint32_t) p; out->info = s.ref | s.major << 4 | s.flags << 8;
#pragma unroll
        for (int k = 0; k < 8; k++) out->counts[k] = c[k];
    }
}
}  // namespace

// The host sequence of cdm_pileup_bases (who; gr without records) and of cdm_pileup_bases_gapped (gr: the caller's gapped records,
// checked before anything goes to the device).
static int cdm_bases_impl(cdm_ctx *ctx, const char *who, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t nq, GappedRecords &gr, const cdm_bases_params *par,
                          uint64_t *stats, uint32_t *counts, cdm_site **sites, uint64_t *nSitesOut, float *kernelMs) {
    hipStream_t s = ctx->stream;
    const uint32_t chunk = pileupChunk();
    const uint64_t bound = basesPositions();
    if (int rc = gr.check(who, db, queries, nq)) return rc;
    QuerySizes qs;
    if (int rc = querySizes(ctx, db, alns, queries, nq, who, "counters", qs)) return rc;
    if (int rc = gr.checkCounts(who, "counters", queries, qs.recs)) return rc;
    if (int rc = gr.upload(s, who)) return rc;
    float msTotal = 0.f; uint64_t countsAt = 0, g0 = 0;
    for (uint64_t b0 = 0; b0 < nq;) {
        // the batch: listed queries while their positions stay within the bound; a single query longer than the bound goes alone
        BatchPlan plan; WorkItems work; cdmscan::ScanTemp stPlace;
        plan.cut(qs.len, b0, 0u, [](uint64_t len) { return len; }, bound);
        const uint32_t m = plan.m; const uint64_t nPos = plan.cells, nTiles = plan.nTiles;
        DevBuf<uint32_t> planes, place, dCounts; DevBuf<unsigned long long> dStats; DevBuf<cdm_site> dSites;
        if (!work.alloc(m) || !plan.alloc() || !planes.alloc((size_t) nPos * 8) || !place.alloc((size_t) nPos + 1) || !dStats.alloc((size_t) m * 8) || (counts && !dCounts.alloc((size_t) nPos * 8))) {
            cdm_set_error("%s: out of device memory for the counters of %llu positions of %u queries", who, (unsigned long long) nPos, m); return CDM_ERR_HIP;
        }
        if (int rc = plan.upload(s)) return rc;
        CDM_HIP(hipMemsetAsync(planes.p, 0, (size_t) nPos * 32, s));
        CDM_HIP(hipMemsetAsync(place.p + nPos, 0, 4, s));             // (the closing word: the scan leaves the batch's number of sites there)
        CDM_HIP(hipMemsetAsync(dStats.p, 0, (size_t) m * 64, s));
        if (int rc = workItems(s, alns, qs.dq.p + b0, m, chunk, work)) return rc;
        BasesArgs a;
        fillArgs(a, qs.meta.p, db, alns, par->min_seq_id, par->skip_extended_targets, work, plan);
        a.codes = db->codes; a.nmask = db->nmask; a.maskEnds = (uint32_t) par->mask_ends; a.minDepth = (uint32_t) par->min_depth;
        a.minAlt = (uint32_t) par->min_alt_count; a.minPct = (uint32_t) par->min_alt_percent; a.firstQuery = (uint32_t) b0;
        a.nPos = nPos; a.planes = planes.p; a.stats = dStats.p; a.place = place.p; a.counts = counts ? dCounts.p : nullptr; a.sites = nullptr;
        // the gapped records are sorted by query: the batch's are one contiguous range
        const uint64_t g1 = gr.end(g0, b0 + m);
        a.grec = gr.dRecs.p ? gr.dRecs.p + g0 : nullptr; a.gops = gr.dOps.p; a.nG = (uint32_t) (g1 - g0);      // (fewer than 2^31 operation words: fewer records)
        hipEventRecord(ctx->ev0, s);
        launchWaveItems(s, k_base_counts, a, work.n);
        launchWaveItems(s, k_base_counts_gapped, a, ((uint64_t) a.nG + 63) / 64);
        launchTiles(s, k_base_sites, a, nTiles);
        uint32_t nSites = 0;
        if (sites) {
            if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stPlace, place.p, place.p, (size_t) nPos + 1)) return rc;      // (in place: scan.h)
            CDM_HIP(hipMemcpyAsync(&nSites, place.p + nPos, 4, hipMemcpyDeviceToHost, s));
        }
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        CDM_HIP(hipMemcpyAsync(stats + b0 * 8, dStats.p, (size_t) m * 64, hipMemcpyDeviceToHost, s));
        if (counts && nPos) CDM_HIP(hipMemcpyAsync(counts + countsAt * 8, dCounts.p, (size_t) nPos * 32, hipMemcpyDeviceToHost, s));
        if (int rc = finishTimed(ctx, who, "kernels", msTotal)) return rc;
        if (nSites) {       // the records of this batch behind those of the batches before it
            if (!dSites.alloc(nSites)) { cdm_set_error("%s: out of device memory for %u site records", who, nSites); return CDM_ERR_HIP; }
            a.sites = dSites.p;
            hipEventRecord(ctx->ev0, s);
            launchTiles(s, k_base_emit, a, nTiles);
            hipEventRecord(ctx->ev1, s);
            CDM_LAUNCH_CHECK();
            if (int rc = appendRecords(s, who, "site", sites, nSitesOut, (const cdm_site *) dSites.p, nSites)) return rc;
            if (int rc = finishTimed(ctx, who, "emission", msTotal)) return rc;
        }
        countsAt += nPos; b0 += m; g0 = g1;
    }
    if (kernelMs) *kernelMs = msTotal;
    return CDM_OK;
}

// the checks of the two entry points
static int basesCheck(const char *who, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_bases_params *par) {
    if (par->mask_ends < 0 || par->mask_ends > BS_MAX_MASK) { cdm_set_error("%s: mask_ends = %d; 0 to %d positions are left out at either end of a read", who, par->mask_ends, BS_MAX_MASK); return CDM_ERR_INVALID; }
    if (par->min_depth < 1) { cdm_set_error("%s: min_depth = %d; a called position has at least one base", who, par->min_depth); return CDM_ERR_INVALID; }
    if (par->min_alt_count < 1) { cdm_set_error("%s: min_alt_count = %d; a second allele has at least one base", who, par->min_alt_count); return CDM_ERR_INVALID; }
    if (par->min_alt_percent < 0 || par->min_alt_percent > 100) { cdm_set_error("%s: min_alt_percent = %d; a percentage of the depth is 0 to 100", who, par->min_alt_percent); return CDM_ERR_INVALID; }
    return pileupCheckArgs(who, db, alns, queries, n_queries);
}

extern "C" int cdm_pileup_bases(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_bases_params *par,
                                uint64_t *stats, uint32_t *counts, cdm_site **sites, uint64_t *n_sites, float *kernel_ms) {
    static const char *const WHO = "cdm_pileup_bases";
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, WHO);
    if (!ctx || !db || !alns || !par || (sites && !n_sites) || (n_queries && (!queries || !stats))) { cdm_set_error("%s: NULL argument", WHO); return CDM_ERR_INVALID; }
    if (int rc = basesCheck(WHO, db, alns, queries, n_queries, par)) return rc;
    GappedRecords none;
    return runWithRecords(ctx, n_queries, sites, n_sites, kernel_ms, [&](cdm_site **got, uint64_t *nGot, float *ms) {
        return cdm_bases_impl(ctx, WHO, db, alns, queries, n_queries, none, par, stats, counts, got, nGot, ms);
    });
}

extern "C" int cdm_pileup_bases_gapped(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_gap_rec *recs, uint64_t n_recs,
                                       const uint32_t *ops, uint64_t n_ops, const cdm_bases_params *par, uint64_t *stats, uint32_t *counts, cdm_site **sites, uint64_t *n_sites,
                                       float *kernel_ms) {
    static const char *const WHO = "cdm_pileup_bases_gapped";
    if (kernel_ms) *kernel_ms = 0.f;
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, WHO);
    if (!ctx || !db || !alns || !par || (n_recs && (!recs || !ops)) || (sites && !n_sites) || (n_queries && (!queries || !stats))) { cdm_set_error("%s: NULL argument", WHO); return CDM_ERR_INVALID; }
    if (int rc = basesCheck(WHO, db, alns, queries, n_queries, par)) return rc;
    if (n_ops >> 31) { cdm_set_error("%s: %llu operation words; the 32-bit record slots hold fewer than 2^31", WHO, (unsigned long long) n_ops); return CDM_ERR_UNSUPPORTED; }
    GappedRecords gr; gr.recs = recs; gr.nRecs = n_recs; gr.ops = ops; gr.nOps = n_ops;
    return runWithRecords(ctx, n_queries, sites, n_sites, kernel_ms, [&](cdm_site **got, uint64_t *nGot, float *ms) {
        return cdm_bases_impl(ctx, WHO, db, alns, queries, n_queries, gr, par, stats, counts, got, nGot, ms);
    });
}

extern "C" void cdm_sites_free(cdm_site *sites) { free(sites); }
