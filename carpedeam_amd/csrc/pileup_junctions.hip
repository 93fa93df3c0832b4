// What the letters say at a contig junction (cdm_pileup_junctions; not a module of the reference): for a list of junctions - a canonical
// link (a, oA) -> (b, oB) of cdm_pileup_links with ONE gap value - the letters of two overlapping ends compared, or the letters between
// two ends voted from the reads that bridge them (the rule: include/carpedeam_hip.h).  The end-record stage is cdm_pileup_links' own
// (pileup_links.h); behind it:
//
//   k_jn_pair_count   per place of the sorted end records, the walk of k_ln_expand: every pair's canonical key is looked up in the sorted
//                  junction keys (binary search); a pair whose gap is the junction's is a VOTER (one 32-bit atomicAdd), and where that
//                  gap is positive a matched pair
//   scan           every tail's first matched pair
//   k_jn_pair_emit the same walk: per matched pair the read and junction | first letter << 32 | flipped << 54
//   k_jn_letters   a wave per matched pair, lanes over the gap's offsets: the read's letter (cdm_base, cdm_isN; the reverse complement for a
//                  pair that needed the flip) into the junction's five counters of that offset, 32-bit atomicAdd
//   k_jn_vote      a thread per fill letter: the base with the largest count, the lowest code among equals, N where no voter has a base;
//                  the junction's smallest winning count (atomicMin) and its N letters (atomicAdd)
//   k_jn_overlap   a wave per junction with an overlap, lanes over its columns, a wave sum
// Integer sums, minima and maxima only: no result depends on the order in which the atomics arrive.  Every index a kernel follows comes
// from countedRecord() (the read, its length, h < tLen), from a scan of counts made by the same walk, or from a junction the host checked
// (a, b < n_queries; k <= min(lenA, lenB); fill_off + gap within the pool).
#include "pileup_links.h"

namespace {

// The fill letters of a call.  Reasoned, not measured: a letter costs 5 x 4 bytes of counters and one byte, so 2^26 letters are 1.4 GB of
// the device's 288 GB beside the end records; no assembly graph comes near (a gap is shorter than a read).
constexpr uint64_t JN_FILL_MOST = 1ull << 26;
constexpr int JN_START_SHIFT = 32, JN_FLIP_BIT = 54;

struct JunctionArgs : ReadRuns {
    const uint64_t *jKeys; const int32_t *jGap;     // [nj] the junctions' keys, ascending, and gaps
    const uint64_t *fillOff;                        // [nj + 1] first fill letter of every junction (a junction without a fill has none)
    uint32_t nj;
    uint64_t *pairAt;                               // [n + 1]: the matched pairs of a tail record, after the scan its first
    unsigned int *voters;                           // [nj]
    uint32_t *mRead; uint64_t *mWord;               // [matched pairs]
    const uint32_t *codes, *nmask;
    unsigned int *counts;                           // [fill letters][5]
    uint8_t *letters;                               // [fill letters]
    unsigned int *fillMin, *fillN, *matches;        // [nj]
    const uint32_t *jA, *jB, *jInfo;                // [nj] k_jn_overlap: the two DB sequences and the junction's info
    uint64_t nFill;
};

// the junction with this key, or nj
__device__ __forceinline__ uint32_t jnFind(const JunctionArgs &g, uint64_t key) {
    uint32_t lo = 0, hi = g.nj;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (g.jKeys[mid] < key) lo = mid + 1; else hi = mid; }
    return lo < g.nj && g.jKeys[lo] == key ? lo : g.nj;
}
// The walk both kernels make over the pairs of the tail record at place i: found(junction, pair) for every pair whose gap is its junction's.
template <class Found> __device__ __forceinline__ void jnWalk(const JunctionArgs &g, uint64_t i, Found found) {
    uint32_t rs, re;
    if (!lnRun(g, i, rs, re)) return;
    const uint64_t v = g.vals[i];
    if (!lnTail(v)) return;
    const int tLen = (int) g.meta[g.keys[i]].len;       // (the read: a sequence of the DB, countedRecord)
    for (uint32_t j = rs; j < re; j++) {                // (at most max_ends places)
        const uint64_t w = g.vals[j];
        if (lnTail(w) || (w >> LN_X_SHIFT) == (v >> LN_X_SHIFT)) continue;
        const LnPair pr = lnPair(v, w, tLen, g.qBits);
        const uint32_t jn = jnFind(g, pr.key);
        if (jn < g.nj && g.jGap[jn] == pr.gap) found(jn, pr, (uint32_t) tLen);
    }
}
__global__ __launch_bounds__(DP_NT) void k_jn_pair_count(JunctionArgs g, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i >= g.n) return;
    uint64_t nMatched = 0;
    jnWalk(g, i, [&](uint32_t jn, const LnPair &pr, uint32_t) { atomicAdd(&g.voters[jn], 1u); if (pr.gap > 0) nMatched++; });
    g.pairAt[i] = nMatched;
}
__global__ __launch_bounds__(DP_NT) void k_jn_pair_emit(JunctionArgs g, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i >= g.n) return;
    uint64_t p = g.pairAt[i];           // (the same walk as k_jn_pair_count's: pairAt[i + 1] - pairAt[i] matched pairs)
    const uint32_t read = g.keys[i];
    jnWalk(g, i, [&](uint32_t jn, const LnPair &pr, uint32_t tLen) {
        if (pr.gap <= 0) return;
        g.mRead[p] = read;              // the letters between the queries: read[tLen - hX .. hY), hY = tLen - hX + gap
        g.mWord[p] = (uint64_t) jn | (uint64_t) (tLen - pr.hX) << JN_START_SHIFT | (uint64_t) (pr.fwd ? 0u : 1u) << JN_FLIP_BIT;
        p++;
    });
}
// 0 < start = tLen - hX and start + gap = hY < tLen (an end record's h is below its read's length): every letter is the read's own.
__global__ __launch_bounds__(64 * PU_WAVES) void k_jn_letters(JunctionArgs g, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    const uint64_t word = g.mWord[first + local];
    const uint32_t jn = (uint32_t) word, start = (uint32_t) (word >> JN_START_SHIFT) & LN_H_MASK, woff = g.meta[g.mRead[first + local]].woff;
    const bool flip = (word >> JN_FLIP_BIT) & 1u;
    const uint32_t gap = (uint32_t) g.jGap[jn];
    unsigned int *row = g.counts + g.fillOff[jn] * 5;
    for (uint32_t o = lane; o < gap; o += 64) {
        const uint32_t pos = start + (flip ? gap - 1u - o : o);
        const uint32_t code = cdm_base(g.codes, woff, pos);
        const uint32_t c = cdm_isN(g.nmask, woff, pos) ? 4u : (flip ? 3u - code : code);
        atomicAdd(&row[(uint64_t) o * 5 + c], 1u);
    }
}
__global__ __launch_bounds__(DP_NT) void k_jn_vote(JunctionArgs g, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i >= g.nFill) return;
    const unsigned int *c = g.counts + i * 5;
    uint32_t best = 0;
    for (uint32_t k = 1; k < 4; k++) if (c[k] > c[best]) best = k;      // (the lowest code among equals)
    const unsigned int win = c[best];
    const uint32_t jn = ownerOf(g.fillOff, g.nj, i);
    g.letters[i] = (uint8_t) "ACGTN"[win ? best : 4u];
    atomicMin(&g.fillMin[jn], win);
    if (!win) atomicAdd(&g.fillN[jn], 1u);
}
// oriented A[lenA - k + j] against oriented B[j], j < k: the - form of a sequence is its reverse complement, which keeps the N bit
__global__ __launch_bounds__(64 * PU_WAVES) void k_jn_overlap(JunctionArgs g, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    const uint32_t jn = (uint32_t) (first + local);
    const int gap = g.jGap[jn];
    if (gap >= 0) return;                   // (wave-uniform)
    const uint32_t k = (uint32_t) -gap;
    const SeqMeta A = g.meta[g.jA[jn]], B = g.meta[g.jB[jn]];
    if (k > min(A.len, B.len)) return;      // contained
    const bool minusA = g.jInfo[jn] & 1u, minusB = g.jInfo[jn] & 2u;
    int same = 0;
    for (uint32_t j = lane; j < k; j += 64) {
        const uint32_t pa = minusA ? k - 1u - j : A.len - k + j, pb = minusB ? B.len - 1u - j : j;
        const uint32_t ca = cdm_base(g.codes, A.woff, pa), cb = cdm_base(g.codes, B.woff, pb);
        const bool n = cdm_isN(g.nmask, A.woff, pa) || cdm_isN(g.nmask, B.woff, pb);
        same += !n && (minusA ? 3u - ca : ca) == (minusB ? 3u - cb : cb);
    }
    same = cdm_wave_sum(same);
    if (lane == 0) g.matches[jn] = (unsigned int) same;
}

}  // namespace

static int cdm_junctions_impl(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t nq, const cdm_links_params *par, const cdm_junction *junctions,
                              uint64_t nj, cdm_junction_res *res, uint8_t **lettersOut, uint32_t **countsOut, float *kernelMs) {
    static const char *const WHO = "cdm_pileup_junctions";
    hipStream_t s = ctx->stream;
    float msTotal = 0.f;
    EndRecords ends;
    if (int rc = linkEndRecords(ctx, db, alns, queries, nq, par, WHO, NULL, ends, msTotal)) return rc;
    const int qBits = ends.g.qBits;
    // the junctions as the kernels take them, and what the host knows of every result from the lengths alone
    std::vector<uint64_t> keys(nj), fillOff(nj + 1, 0); std::vector<int32_t> gaps(nj); std::vector<uint32_t> jA(nj), jB(nj), jInfo(nj);
    for (uint64_t i = 0; i < nj; i++) {
        const cdm_junction &j = junctions[i];
        keys[i] = (uint64_t) (j.a << 1 | (j.info & 1u)) << (qBits + 1) | (j.b << 1 | (j.info >> 1 & 1u));
        gaps[i] = j.gap; jA[i] = queries[j.a]; jB[i] = queries[j.b]; jInfo[i] = j.info;
        cdm_junction_res &r = res[i];
        r.columns = 0; r.matches = 0; r.voters = 0; r.flags = 0; r.fill_off = fillOff[i]; r.fill_len = 0; r.fill_min = 0; r.fill_n = 0; r.reserved = 0;
        if (j.gap < 0) {
            const uint32_t k = (uint32_t) -(int64_t) j.gap;
            if (k > std::min(ends.qs.len[j.a], ends.qs.len[j.b])) r.flags |= CDM_JUNCTION_CONTAINED; else r.columns = k;
        } else r.fill_len = (uint32_t) j.gap;
        fillOff[i + 1] = fillOff[i] + r.fill_len;
    }
    const uint64_t nFill = fillOff[nj];         // (the entry point: at most JN_FILL_MOST)
    const uint32_t n = (uint32_t) ends.nEnds;
    DevBuf<uint64_t> dKeys, dFillOff, pairAt, mWord; DevBuf<int32_t> dGaps; DevBuf<uint32_t> dA, dB, dInfo, mRead; DevBuf<unsigned int> voters, fillMin, fillN, matches, counts; DevBuf<uint8_t> letters;
    cdmscan::ScanTemp stPairs;
    if (!dKeys.alloc(nj) || !dFillOff.alloc(nj + 1) || !dGaps.alloc(nj) || !dA.alloc(nj) || !dB.alloc(nj) || !dInfo.alloc(nj) || !voters.alloc(nj) || !fillMin.alloc(nj) || !fillN.alloc(nj) ||
        !matches.alloc(nj) || !counts.alloc((size_t) nFill * 5) || !letters.alloc(nFill) || !pairAt.alloc((size_t) n + 1)) {
        cdm_set_error("%s: out of device memory for %llu junctions and %llu fill letters", WHO, (unsigned long long) nj, (unsigned long long) nFill); return CDM_ERR_HIP;
    }
    CDM_HIP(hipMemcpyAsync(dKeys.p, keys.data(), nj * 8, hipMemcpyHostToDevice, s));
    CDM_HIP(hipMemcpyAsync(dFillOff.p, fillOff.data(), (nj + 1) * 8, hipMemcpyHostToDevice, s));
    CDM_HIP(hipMemcpyAsync(dGaps.p, gaps.data(), nj * 4, hipMemcpyHostToDevice, s));
    CDM_HIP(hipMemcpyAsync(dA.p, jA.data(), nj * 4, hipMemcpyHostToDevice, s));
    CDM_HIP(hipMemcpyAsync(dB.p, jB.data(), nj * 4, hipMemcpyHostToDevice, s));
    CDM_HIP(hipMemcpyAsync(dInfo.p, jInfo.data(), nj * 4, hipMemcpyHostToDevice, s));
    CDM_HIP(hipMemsetAsync(voters.p, 0, nj * 4, s));
    CDM_HIP(hipMemsetAsync(fillMin.p, 0xFF, nj * 4, s));
    CDM_HIP(hipMemsetAsync(fillN.p, 0, nj * 4, s));
    CDM_HIP(hipMemsetAsync(matches.p, 0, nj * 4, s));
    if (nFill) CDM_HIP(hipMemsetAsync(counts.p, 0, (size_t) nFill * 20, s));
    CDM_HIP(hipMemsetAsync(pairAt.p + n, 0, 8, s));
    JunctionArgs g;
    static_cast<ReadRuns &>(g) = ends.g;
    g.jKeys = dKeys.p; g.jGap = dGaps.p; g.fillOff = dFillOff.p; g.nj = (uint32_t) nj; g.pairAt = pairAt.p; g.voters = voters.p; g.mRead = nullptr; g.mWord = nullptr;
    g.codes = db->codes; g.nmask = db->nmask; g.counts = counts.p; g.letters = letters.p; g.fillMin = fillMin.p; g.fillN = fillN.p; g.matches = matches.p;
    g.jA = dA.p; g.jB = dB.p; g.jInfo = dInfo.p; g.nFill = nFill;
    const uint64_t nTiles = ((uint64_t) n + DP_NT - 1) / DP_NT;
    uint64_t nMatched = 0;
    if (n) {
        hipEventRecord(ctx->ev0, s);
        launchTiles(s, k_jn_pair_count, g, nTiles);
        if (int rc = cdmscan::exclusiveScan<uint64_t>(s, stPairs, pairAt.p, pairAt.p, (size_t) n + 1)) return rc;     // (in place)
        CDM_HIP(hipMemcpyAsync(&nMatched, pairAt.p + n, 8, hipMemcpyDeviceToHost, s));
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        if (int rc = finishTimed(ctx, WHO, "pairing", msTotal)) return rc;
    }
    if (nMatched && (!mRead.alloc(nMatched) || !mWord.alloc(nMatched))) { cdm_set_error("%s: out of device memory for %llu pairs with letters", WHO, (unsigned long long) nMatched); return CDM_ERR_HIP; }
    g.mRead = mRead.p; g.mWord = mWord.p;
    std::vector<unsigned int> hVoters(nj), hMin(nj), hN(nj), hMatches(nj);
    uint8_t *hostLetters = NULL; uint32_t *hostCounts = NULL;
    if (nFill) {
        hostLetters = (uint8_t *) malloc(nFill);
        if (countsOut) hostCounts = (uint32_t *) malloc(nFill * 20);
        if (!hostLetters || (countsOut && !hostCounts)) { free(hostLetters); free(hostCounts); cdm_set_error("%s: out of host memory for %llu fill letters", WHO, (unsigned long long) nFill); return CDM_ERR_INVALID; }
    }
    hipEventRecord(ctx->ev0, s);
    if (nMatched) { launchTiles(s, k_jn_pair_emit, g, nTiles); launchWaveItems(s, k_jn_letters, g, nMatched); }
    if (nFill) launchTiles(s, k_jn_vote, g, (nFill + DP_NT - 1) / DP_NT);
    launchWaveItems(s, k_jn_overlap, g, nj);
    hipEventRecord(ctx->ev1, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(hVoters.data(), voters.p, nj * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(hMin.data(), fillMin.p, nj * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(hN.data(), fillN.p, nj * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(hMatches.data(), matches.p, nj * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && nFill) e = hipMemcpyAsync(hostLetters, letters.p, nFill, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && hostCounts) e = hipMemcpyAsync(hostCounts, counts.p, nFill * 20, hipMemcpyDeviceToHost, s);
    int rc = CDM_OK;
    if (e != hipSuccess) { cdm_set_error("%s: the letter kernels or their downloads failed: %s", WHO, hipGetErrorString(e)); hipStreamSynchronize(s); rc = CDM_ERR_HIP; }
    else rc = finishTimed(ctx, WHO, "letter kernels", msTotal);
    if (rc) { free(hostLetters); free(hostCounts); return rc; }
    for (uint64_t i = 0; i < nj; i++) {
        res[i].voters = hVoters[i]; res[i].matches = hMatches[i];
        if (res[i].fill_len) { res[i].fill_min = hMin[i]; res[i].fill_n = hN[i]; }
    }
    *lettersOut = hostLetters;
    if (countsOut) *countsOut = hostCounts;
    if (kernelMs) *kernelMs = msTotal;
    return CDM_OK;
}

extern "C" int cdm_pileup_junctions(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_links_params *par,
                                    const cdm_junction *junctions, uint64_t n_junctions, cdm_junction_res *res, uint8_t **letters, uint32_t **counts, float *kernel_ms) {
    static const char *const WHO = "cdm_pileup_junctions";
    if (kernel_ms) *kernel_ms = 0.f;
    if (letters) *letters = NULL;
    if (counts) *counts = NULL;
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, WHO);
    if (!ctx || !db || !alns || !par || !letters || (n_queries && !queries) || (n_junctions && (!junctions || !res))) { cdm_set_error("%s: NULL argument", WHO); return CDM_ERR_INVALID; }
    if (par->anchor < 1 || par->anchor > LN_MAX_ANCHOR) { cdm_set_error("%s: anchor = %d; an end record has 1 to %d columns on its query", WHO, par->anchor, LN_MAX_ANCHOR); return CDM_ERR_INVALID; }
    if (par->overhang < 1 || par->overhang > LN_MAX_OVERHANG) { cdm_set_error("%s: overhang = %d; an end record's read has 1 to %d letters beyond the query's end", WHO, par->overhang, LN_MAX_OVERHANG); return CDM_ERR_INVALID; }
    if (par->max_ends < 2 || par->max_ends > LN_MAX_ENDS) { cdm_set_error("%s: max_ends = %d; a read that makes pairs has 2 to %d end records at the most", WHO, par->max_ends, LN_MAX_ENDS); return CDM_ERR_INVALID; }
    if (int rc = pileupCheckArgs(WHO, db, alns, queries, n_queries)) return rc;
    uint64_t nFill = 0; int32_t widest = 0; uint64_t widestAt = 0;
    for (uint64_t i = 0; i < n_junctions; i++) {
        const cdm_junction &j = junctions[i];
        if (j.a >= j.b || j.b >= n_queries) { cdm_set_error("%s: junction %llu joins list indices %u and %u; a < b < %llu listed queries", WHO, (unsigned long long) i, j.a, j.b, (unsigned long long) n_queries); return CDM_ERR_INVALID; }
        if (j.info > 3u) { cdm_set_error("%s: junction %llu has info = %u; bit 0 and bit 1 are the two orientations", WHO, (unsigned long long) i, j.info); return CDM_ERR_INVALID; }
        if (i) {
            const cdm_junction &p = junctions[i - 1];
            const uint64_t now[4] = {j.a, j.info & 1u, j.b, j.info >> 1}, was[4] = {p.a, p.info & 1u, p.b, p.info >> 1};
            if (!std::lexicographical_compare(was, was + 4, now, now + 4)) { cdm_set_error("%s: junction %llu does not follow junction %llu; the junctions ascend strictly by (a, oA, b, oB)", WHO, (unsigned long long) i, (unsigned long long) (i - 1)); return CDM_ERR_INVALID; }
        }
        if (j.gap > 0) nFill += (uint64_t) j.gap;
        const int32_t w = j.gap < 0 ? (j.gap == INT32_MIN ? INT32_MAX : -j.gap) : j.gap;
        if (w > widest) { widest = w; widestAt = i; }
    }
    if (n_queries == 0 || n_junctions == 0) return CDM_OK;
    if (db->maxLen >= LN_MAX_LETTERS) {
        cdm_set_error("%s: the DB holds a sequence of %u letters; an end word holds a read's overhang in %d bits and a gap word the gap in %d (sequences of fewer than %u letters)",
                      WHO, db->maxLen, LN_LEN_BITS, LN_GAP_BITS, LN_MAX_LETTERS);
        return CDM_ERR_UNSUPPORTED;
    }
    if (n_queries > LN_QUERIES_MOST) {
        cdm_set_error("%s: %llu listed queries; an end word and a link key hold a list index in %d bits (%llu queries at the most)", WHO, (unsigned long long) n_queries, LN_QUERY_BITS,
                      (unsigned long long) LN_QUERIES_MOST);
        return CDM_ERR_UNSUPPORTED;
    }
    if (n_junctions >> 32) { cdm_set_error("%s: %llu junctions; a pair holds its junction's index in 32 bits", WHO, (unsigned long long) n_junctions); return CDM_ERR_UNSUPPORTED; }
    if ((uint32_t) widest >= LN_MAX_LETTERS) {
        cdm_set_error("%s: junction %llu has gap = %d; no pair has a gap or an overlap of %u letters or more", WHO, (unsigned long long) widestAt, junctions[widestAt].gap, LN_MAX_LETTERS);
        return CDM_ERR_UNSUPPORTED;
    }
    if (nFill > JN_FILL_MOST) {
        cdm_set_error("%s: the junctions ask for %llu fill letters; a call votes %llu at the most (20 bytes of counters per letter)", WHO, (unsigned long long) nFill, (unsigned long long) JN_FILL_MOST);
        return CDM_ERR_UNSUPPORTED;
    }
    CDM_HIP(hipSetDevice(ctx->device));
    const int rc = cdm_junctions_impl(ctx, db, alns, queries, n_queries, par, junctions, n_junctions, res, letters, counts, kernel_ms);
    if (rc != CDM_OK && kernel_ms) *kernel_ms = 0.f;
    return rc;
}

extern "C" void cdm_junction_free(uint8_t *letters, uint32_t *counts) { free(letters); free(counts); }
