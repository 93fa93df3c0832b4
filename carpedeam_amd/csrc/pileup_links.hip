// Contig links from the reads that bridge two contig ends (cdm_pileup_links; not a module of the reference): the edges of the assembly
// graph that the read pile-up holds already.  A counted record of a listed query whose read hangs over exactly one end of the query by
// `overhang` letters, with `anchor` columns on it, is an END RECORD; a read's tail record on one listed query and its head record on
// another are a PAIR, the pairs with equal canonical (a, oA, b, oB) are a LINK (the rule: include/carpedeam_hip.h).  What the unit
// shares with the reductions over the pile-up is in pileup.h; the end-record stage, which cdm_pileup_junctions runs as well, is in
// pileup_links.h (k_ln_count, k_ln_emit, the sort by read, k_ln_read_heads, k_ln_read_starts).  Behind it:
//
//   k_ln_pair_count   per place: a tail record of a read with at most max_ends end records counts the read's head records on other
//                  list indices (at most max_ends places looked at); self pairs and crowded reads summed per wave, one atomic each
//   scan           every tail's first pair
//   k_ln_expand    the same walk: per pair the link key (a << 1 | oA) << (qBits + 1) | b << 1 | oB and the gap word
//                  (gap + 2^22) | forward << 23
//   sort           by link, then gap: the radix order is stable and least significant digit first, so its passes over the 23 gap
//                  bits run in front of those over the link bits in use
//   k_ln_link_heads, scans, k_ln_link_starts     link id and gap-run id of every place, first place of every link and gap run
//   k_ln_reduce    per place: forward and gap into the link's sums, a gap run's length << 32 | (2^32 - 1 - gap word) into the link's mode
//                  with a 64-bit atomicMax; the lanes of a wave that share a link are reduced first (its places are neighbours)
//   k_ln_finish    per link: a, b, info from its key, reads from its two ends, gap_min and gap_max from its first and last place
//                  (the places of a link ascend by gap), the keep flag; the scan gives the places of the links at min_reads
//   k_ln_compact   those links in order
// Integer atomics only (sums and a maximum): no result depends on the order in which they arrive.
#include "pileup_links.h"

namespace {

// the walk over the runs of the sorted end records
struct ReadArgs : ReadRuns {
    uint64_t *pairAt;               // [n + 1]: the pairs of a tail record, after the scan its first pair
    unsigned long long *totals;     // [5]: 1 crowded reads, 2 self pairs
    uint32_t *gapKeys; uint64_t *linkKeys;      // k_ln_expand: [pairs]
};
// (every lane of a wave reaches the sums: no early return)
__global__ __launch_bounds__(DP_NT) void k_ln_pair_count(ReadArgs g, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    unsigned int nPairs = 0, nSelf = 0, nCrowded = 0;
    if (i < g.n) {
        uint32_t rs, re;
        if (!lnRun(g, i, rs, re)) nCrowded = i == rs;
        else {
            const uint64_t v = g.vals[i];
            if (lnTail(v))
                for (uint32_t j = rs; j < re; j++) {        // (at most max_ends places)
                    const uint64_t w = g.vals[j];
                    if (lnTail(w)) continue;
                    if ((w >> LN_X_SHIFT) == (v >> LN_X_SHIFT)) nSelf++; else nPairs++;
                }
        }
        g.pairAt[i] = nPairs;
    }
    const unsigned int self = (unsigned int) cdm_wave_sum((int) nSelf), crowded = (unsigned int) cdm_wave_sum((int) nCrowded);
    if (lane == 0) {
        if (crowded) atomicAdd(&g.totals[1], (unsigned long long) crowded);
        if (self) atomicAdd(&g.totals[2], (unsigned long long) self);
    }
}
__global__ __launch_bounds__(DP_NT) void k_ln_expand(ReadArgs g, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i >= g.n) return;
    uint32_t rs, re;
    if (!lnRun(g, i, rs, re)) return;
    const uint64_t v = g.vals[i];
    if (!lnTail(v)) return;
    const int tLen = (int) g.meta[g.keys[i]].len;       // (the read: a sequence of the DB, countedRecord)
    uint64_t p = g.pairAt[i];                           // (the same walk as k_ln_pair_count's: pairAt[i + 1] - pairAt[i] pairs)
    for (uint32_t j = rs; j < re; j++) {
        const uint64_t w = g.vals[j];
        if (lnTail(w) || (w >> LN_X_SHIFT) == (v >> LN_X_SHIFT)) continue;
        const LnPair pr = lnPair(v, w, tLen, g.qBits);
        g.linkKeys[p] = pr.key;
        g.gapKeys[p] = ((uint32_t) (pr.gap + (int) LN_GAP_BIAS) & LN_GAP_MASK) | (pr.fwd ? 1u : 0u) << LN_GAP_BITS;
        p++;
    }
}

// the pairs sorted by link and gap: a tile is DP_NT places
struct PairArgs {
    const uint64_t *linkKeys; const uint32_t *gapKeys;
    uint32_t *linkOf, *gapOf;       // [n + 1]: 1 at a link's / a gap run's first place, after the scans the links / gap runs in front of a place
    uint32_t *linkStart, *gapStart; // [links + 1], [gap runs + 1]: their first places; the closing entry is n
    unsigned int *forward; unsigned long long *sum, *mode;      // [links]
    cdm_link *links;                // [links]
    uint32_t *keepAt;               // [links + 1]: 1 for a link at min_reads, after the scan its place in the output
    cdm_link *out;
    uint32_t n, nLinks, minReads; int qBits;
};
__global__ __launch_bounds__(DP_NT) void k_ln_link_heads(PairArgs g, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i >= g.n) return;
    const bool link = i == 0 || g.linkKeys[i] != g.linkKeys[i - 1];
    g.linkOf[i] = link;
    g.gapOf[i] = link || ((g.gapKeys[i] ^ g.gapKeys[i - 1]) & LN_GAP_MASK) != 0;
}
__global__ __launch_bounds__(DP_NT) void k_ln_link_starts(PairArgs g, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i >= g.n) return;
    if (g.linkOf[i + 1] != g.linkOf[i]) g.linkStart[g.linkOf[i]] = (uint32_t) i;
    if (g.gapOf[i + 1] != g.gapOf[i]) g.gapStart[g.gapOf[i]] = (uint32_t) i;
    if (i + 1 == g.n) { g.linkStart[g.linkOf[g.n]] = g.n; g.gapStart[g.gapOf[g.n]] = g.n; }
}
__device__ __forceinline__ unsigned long long lnShflDown64(unsigned long long v, int d) {
    return ((unsigned long long) (unsigned int) __shfl_down((int) (v >> 32), d, 64) << 32) | (unsigned int) __shfl_down((int) (unsigned int) v, d, 64);
}
// What decides a link's mode: the longer gap run, then the smaller gap.  (every lane of a wave reaches the shuffles: no early return)
__global__ __launch_bounds__(DP_NT) void k_ln_reduce(PairArgs g, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = i < g.n;
    uint32_t link = 0xFFFFFFFFu, fwd = 0; unsigned long long sum = 0, mode = 0;
    if (valid) {
        const uint32_t word = g.gapKeys[i], gapB = word & LN_GAP_MASK, run = g.gapOf[i];
        link = g.linkOf[i + 1] - 1u; fwd = word >> LN_GAP_BITS & 1u;
        sum = (unsigned long long) (long long) ((int) gapB - (int) LN_GAP_BIAS);        // (two's complement: the sum of the words is the signed sum)
        if (g.gapOf[i + 1] != run) mode = (unsigned long long) (g.gapStart[run + 1] - g.gapStart[run]) << 32 | (0xFFFFFFFFu - gapB);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {      // the lanes of a link are neighbours: its first lane in the wave ends with the sums and the maximum
        const unsigned long long os = lnShflDown64(sum, d), om = lnShflDown64(mode, d);
        const uint32_t of = (uint32_t) __shfl_down((int) fwd, d, 64), olink = (uint32_t) __shfl_down((int) link, d, 64);
        if (lane + d < 64 && olink == link) { sum += os; fwd += of; if (om > mode) mode = om; }
    }
    const uint32_t prev = (uint32_t) __shfl_up((int) link, 1, 64);
    if (!valid || !(lane == 0 || prev != link)) return;
    if (fwd) atomicAdd(&g.forward[link], fwd);
    if (sum) atomicAdd(&g.sum[link], sum);
    if (mode) atomicMax(&g.mode[link], mode);
}
__global__ __launch_bounds__(DP_NT) void k_ln_finish(PairArgs g, uint64_t first) {
    const uint64_t l = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (l >= g.nLinks) return;
    const uint32_t s = g.linkStart[l], e = g.linkStart[l + 1];      // (s < e <= n)
    const uint64_t key = g.linkKeys[s];
    const uint32_t to = (uint32_t) (key & ((1ull << (g.qBits + 1)) - 1ull)), from = (uint32_t) (key >> (g.qBits + 1));
    const unsigned long long mode = g.mode[l];
    cdm_link k;
    k.a = from >> 1; k.b = to >> 1; k.info = (from & 1u) | (to & 1u) << 1; k.reads = e - s; k.forward = g.forward[l]; k.mode_reads = (uint32_t) (mode >> 32);
    k.gap_mode = (int) (0xFFFFFFFFu - (uint32_t) mode) - (int) LN_GAP_BIAS;
    k.gap_min = (int) (g.gapKeys[s] & LN_GAP_MASK) - (int) LN_GAP_BIAS; k.gap_max = (int) (g.gapKeys[e - 1] & LN_GAP_MASK) - (int) LN_GAP_BIAS;
    k.reserved = 0; k.gap_sum = (long long) g.sum[l];
    g.links[l] = k;
    g.keepAt[l] = k.reads >= g.minReads;
}
__global__ __launch_bounds__(DP_NT) void k_ln_compact(PairArgs g, uint64_t first) {
    const uint64_t l = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (l >= g.nLinks) return;
    const cdm_link k = g.links[l];
    if (k.reads >= g.minReads) g.out[g.keepAt[l]] = k;
}

}  // namespace

static int cdm_links_impl(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t nq, const cdm_links_params *par, uint64_t *stats, uint64_t *totals,
                          cdm_link **links, uint64_t *nLinksOut, float *kernelMs) {
    static const char *const WHO = "cdm_pileup_links";
    hipStream_t s = ctx->stream;
    DevBuf<unsigned long long> dTotals;
    if (!dTotals.alloc(5)) { cdm_set_error("%s: out of device memory for the totals", WHO); return CDM_ERR_HIP; }
    CDM_HIP(hipMemsetAsync(dTotals.p, 0, 5 * 8, s));
    float msTotal = 0.f;
    EndRecords ends;
    {
        const int rc = linkEndRecords(ctx, db, alns, queries, nq, par, WHO, stats, ends, msTotal);
        totals[0] = ends.nEnds;
        if (rc) return rc;
    }
    DevBuf<cdm_link> kept; uint32_t nKept = 0;
    if (ends.nEnds) {
        const uint32_t n = (uint32_t) ends.nEnds;
        DevBuf<uint64_t> pairAt; cdmscan::ScanTemp stPairs;
        if (!pairAt.alloc((size_t) n + 1)) { cdm_set_error("%s: out of device memory for %u end records", WHO, n); return CDM_ERR_HIP; }
        CDM_HIP(hipMemsetAsync(pairAt.p + n, 0, 8, s));
        ReadArgs g;
        static_cast<ReadRuns &>(g) = ends.g;
        g.pairAt = pairAt.p; g.totals = dTotals.p; g.gapKeys = nullptr; g.linkKeys = nullptr;
        const uint64_t nTiles = ((uint64_t) n + DP_NT - 1) / DP_NT;
        uint64_t nPairs = 0;
        hipEventRecord(ctx->ev0, s);
        launchTiles(s, k_ln_pair_count, g, nTiles);
        if (int rc = cdmscan::exclusiveScan<uint64_t>(s, stPairs, pairAt.p, pairAt.p, (size_t) n + 1)) return rc;     // (in place)
        CDM_HIP(hipMemcpyAsync(&nPairs, pairAt.p + n, 8, hipMemcpyDeviceToHost, s));
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        CDM_HIP(hipMemcpyAsync(totals + 1, dTotals.p + 1, 2 * 8, hipMemcpyDeviceToHost, s));
        if (int rc = finishTimed(ctx, WHO, "pairing", msTotal)) return rc;
        totals[3] = nPairs;
        if (nPairs >> 32) { cdm_set_error("%s: the reads make %llu pairs; the 32-bit places of the link sort hold fewer than 2^32", WHO, (unsigned long long) nPairs); return CDM_ERR_UNSUPPORTED; }
        if (nPairs) {
            const uint32_t np = (uint32_t) nPairs;
            DevBuf<uint32_t> g0, g1, linkOf, gapOf, linkStart, gapStart; DevBuf<uint64_t> l0, l1; cdmscan::ScanTemp stLinks, stGaps, stKeep;
            if (!g0.alloc(np) || !g1.alloc(np) || !l0.alloc(np) || !l1.alloc(np) || !linkOf.alloc((size_t) np + 1) || !gapOf.alloc((size_t) np + 1) || !linkStart.alloc((size_t) np + 1) ||
                !gapStart.alloc((size_t) np + 1)) {
                cdm_set_error("%s: out of device memory for %u pairs", WHO, np); return CDM_ERR_HIP;
            }
            g.gapKeys = g0.p; g.linkKeys = l0.p;
            CDM_HIP(hipMemsetAsync(linkOf.p + np, 0, 4, s));
            CDM_HIP(hipMemsetAsync(gapOf.p + np, 0, 4, s));
            hipEventRecord(ctx->ev0, s);
            launchTiles(s, k_ln_expand, g, nTiles);
            bool gapFirst = true, linkFirst = true;     // least significant digits first: the gap, then (stable) the link
            if (int rc = rx::sortPairs<uint32_t, uint64_t>(s, ctx->cuCount, g0.p, g1.p, l0.p, l1.p, (uint64_t) np, 0, LN_GAP_BITS, gapFirst)) return rc;
            uint64_t *const lIn = gapFirst ? l0.p : l1.p, *const lAlt = gapFirst ? l1.p : l0.p; uint32_t *const gIn = gapFirst ? g0.p : g1.p, *const gAlt = gapFirst ? g1.p : g0.p;
            if (int rc = rx::sortPairs<uint64_t, uint32_t>(s, ctx->cuCount, lIn, lAlt, gIn, gAlt, (uint64_t) np, 0, 2 * (g.qBits + 1), linkFirst)) return rc;
            PairArgs p;
            p.linkKeys = linkFirst ? lIn : lAlt; p.gapKeys = linkFirst ? gIn : gAlt; p.linkOf = linkOf.p; p.gapOf = gapOf.p; p.linkStart = linkStart.p; p.gapStart = gapStart.p;
            p.forward = nullptr; p.sum = nullptr; p.mode = nullptr; p.links = nullptr; p.keepAt = nullptr; p.out = nullptr; p.n = np; p.nLinks = 0; p.minReads = (uint32_t) par->min_reads; p.qBits = g.qBits;
            const uint64_t pTiles = ((uint64_t) np + DP_NT - 1) / DP_NT;
            uint32_t nAll = 0;
            launchTiles(s, k_ln_link_heads, p, pTiles);
            if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stLinks, linkOf.p, linkOf.p, (size_t) np + 1)) return rc;       // (in place)
            if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stGaps, gapOf.p, gapOf.p, (size_t) np + 1)) return rc;
            launchTiles(s, k_ln_link_starts, p, pTiles);
            CDM_HIP(hipMemcpyAsync(&nAll, linkOf.p + np, 4, hipMemcpyDeviceToHost, s));
            hipEventRecord(ctx->ev1, s);
            CDM_LAUNCH_CHECK();
            if (int rc = finishTimed(ctx, WHO, "link sort", msTotal)) return rc;
            totals[4] = nAll;
            DevBuf<unsigned int> forward; DevBuf<unsigned long long> sum, mode; DevBuf<cdm_link> all; DevBuf<uint32_t> keepAt;
            if (!forward.alloc(nAll) || !sum.alloc(nAll) || !mode.alloc(nAll) || !all.alloc(nAll) || !keepAt.alloc((size_t) nAll + 1) || !kept.alloc(nAll)) {
                cdm_set_error("%s: out of device memory for %u links", WHO, nAll); return CDM_ERR_HIP;
            }
            CDM_HIP(hipMemsetAsync(forward.p, 0, (size_t) nAll * 4, s));
            CDM_HIP(hipMemsetAsync(sum.p, 0, (size_t) nAll * 8, s));
            CDM_HIP(hipMemsetAsync(mode.p, 0, (size_t) nAll * 8, s));
            CDM_HIP(hipMemsetAsync(keepAt.p + nAll, 0, 4, s));
            p.forward = forward.p; p.sum = sum.p; p.mode = mode.p; p.links = all.p; p.keepAt = keepAt.p; p.out = kept.p; p.nLinks = nAll;
            const uint64_t lTiles = ((uint64_t) nAll + DP_NT - 1) / DP_NT;
            hipEventRecord(ctx->ev0, s);
            launchTiles(s, k_ln_reduce, p, pTiles);
            launchTiles(s, k_ln_finish, p, lTiles);
            if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stKeep, keepAt.p, keepAt.p, (size_t) nAll + 1)) return rc;       // (in place)
            launchTiles(s, k_ln_compact, p, lTiles);
            CDM_HIP(hipMemcpyAsync(&nKept, keepAt.p + nAll, 4, hipMemcpyDeviceToHost, s));
            hipEventRecord(ctx->ev1, s);
            CDM_LAUNCH_CHECK();
            if (int rc = finishTimed(ctx, WHO, "link reduction", msTotal)) return rc;
        }
    }
    // the returned links: the caller's array, and the queries' link counts from it
    cdm_link *host = NULL;
    if (nKept) {
        host = (cdm_link *) malloc((size_t) nKept * sizeof(cdm_link));
        if (!host) { cdm_set_error("%s: out of host memory for %u links", WHO, nKept); return CDM_ERR_INVALID; }
        const hipError_t e = hipMemcpy(host, kept.p, (size_t) nKept * sizeof(cdm_link), hipMemcpyDeviceToHost);
        if (e != hipSuccess) { free(host); cdm_set_error("%s: the download of %u links failed: %s", WHO, nKept, hipGetErrorString(e)); return CDM_ERR_HIP; }
        for (uint32_t i = 0; i < nKept; i++) { stats[(uint64_t) host[i].a * 6 + 5]++; stats[(uint64_t) host[i].b * 6 + 5]++; }
    }
    if (links) { *links = host; *nLinksOut = nKept; } else free(host);
    if (kernelMs) *kernelMs = msTotal;
    return CDM_OK;
}

extern "C" int cdm_pileup_links(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_links_params *par, uint64_t *stats,
                                uint64_t *totals, cdm_link **links, uint64_t *n_links, float *kernel_ms) {
    static const char *const WHO = "cdm_pileup_links";
    if (kernel_ms) *kernel_ms = 0.f;
    if (links) *links = NULL;
    if (n_links) *n_links = 0;
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, WHO);
    if (!ctx || !db || !alns || !par || !totals || (links && !n_links) || (n_queries && (!queries || !stats))) { cdm_set_error("%s: NULL argument", WHO); return CDM_ERR_INVALID; }
    if (par->anchor < 1 || par->anchor > LN_MAX_ANCHOR) { cdm_set_error("%s: anchor = %d; an end record has 1 to %d columns on its query", WHO, par->anchor, LN_MAX_ANCHOR); return CDM_ERR_INVALID; }
    if (par->overhang < 1 || par->overhang > LN_MAX_OVERHANG) { cdm_set_error("%s: overhang = %d; an end record's read has 1 to %d letters beyond the query's end", WHO, par->overhang, LN_MAX_OVERHANG); return CDM_ERR_INVALID; }
    if (par->max_ends < 2 || par->max_ends > LN_MAX_ENDS) { cdm_set_error("%s: max_ends = %d; a read that makes pairs has 2 to %d end records at the most", WHO, par->max_ends, LN_MAX_ENDS); return CDM_ERR_INVALID; }
    if (par->min_reads < 1 || par->min_reads > LN_MAX_READS) { cdm_set_error("%s: min_reads = %d; a returned link has 1 to %d pairs at the least", WHO, par->min_reads, LN_MAX_READS); return CDM_ERR_INVALID; }
    if (int rc = pileupCheckArgs(WHO, db, alns, queries, n_queries)) return rc;
    for (int i = 0; i < 5; i++) totals[i] = 0;
    if (n_queries == 0) return CDM_OK;
    if (db->maxLen >= LN_MAX_LETTERS) {     // (no upload refuses such a DB: cdm_kmermatch does, which a set from cdm_alns_upload never met)
        cdm_set_error("%s: the DB holds a sequence of %u letters; an end word holds a read's overhang in %d bits and a gap word the gap in %d (sequences of fewer than %u letters)",
                      WHO, db->maxLen, LN_LEN_BITS, LN_GAP_BITS, LN_MAX_LETTERS);
        return CDM_ERR_UNSUPPORTED;
    }
    if (n_queries > LN_QUERIES_MOST) {
        cdm_set_error("%s: %llu listed queries; an end word and a link key hold a list index in %d bits (%llu queries at the most)", WHO, (unsigned long long) n_queries, LN_QUERY_BITS,
                      (unsigned long long) LN_QUERIES_MOST);
        return CDM_ERR_UNSUPPORTED;
    }
    CDM_HIP(hipSetDevice(ctx->device));
    const int rc = cdm_links_impl(ctx, db, alns, queries, n_queries, par, stats, totals, links, n_links, kernel_ms);
    if (rc != CDM_OK && kernel_ms) *kernel_ms = 0.f;
    return rc;
}

extern "C" void cdm_link_free(cdm_link *links) { free(links); }
