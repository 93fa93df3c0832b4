// mergereads on the device: FLASH's pair merging (src/assembler/mergereads.cpp, lib/flash/combine_reads.cpp, lib/flash/read.cpp)
// for a batch of read pairs.
//
// One wave per pair.  The wave stages R1 and the reverse complement of R2 (FLASH's complement_tab, read.cpp:4-13, and the reversed
// qualities, read.cpp reverse_complement) in LDS, the lanes take the overlap shifts i = max(0, L1-L2) .. L1-min_overlap (lane l: the
// shifts l, l + 64, ... from the first), each lane keeps the best of its shifts in the reference's order, and a wave reduction
// picks the lexicographic minimum of (density, quality score, shift) - pair_align's "smallest density, then smallest quality
// score, then the first shift" (combine_reads.cpp:266-334).
//
// The compare is byte by byte: a shift can only win with density <= max_mismatch_density, and since the score length is capped
// at max_overlap, a shift is out as soon as mismatches / min(L1 - i, max_overlap) exceeds that bound (7 mismatches at the
// defaults), so a wrong shift of a real pair leaves after ~10 bytes.  The lane that holds the right shift still walks its whole
// overlap while the rest of the wave waits: at 10 M 2 x 150 pairs this kernel takes 68 ms, far above the ~1 ms its bytes cost
// at HBM speed (profiles/mergereads_10M.txt).  Comparing 2-bit codes with an N mask, 16 bases per word and a popcount, would
// cut that walk about 8x, with this byte path kept for pairs with letters beyond ACGTN; it is not built yet.  Pairs longer than
// the LDS stage (either read > PM_STAGE bytes) read their bytes from global memory with the complement applied on the fly: the
// same code, no length cap.
//
// A second kernel writes the text of mergereads' entries ("SEQ\n\0": the consensus, or R1 and the reverse-complemented R2) at
// offsets from a scan of the per-pair byte counts.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "seqdb.h"
#include "devutil.h"
#include "scan.h"

struct cdm_pairs {
    uint64_t n = 0, entries = 0, bytes = 0;
    int device = 0;
    float kernelMs = -1.f;         // device time of the two kernels and the scans between them
    uint8_t *status = nullptr;     // [n] 1 = combined
    uint32_t *mlen = nullptr;      // [n] combined length (0: not combined)
    uint64_t *entOff = nullptr;    // [entries] offset of entry j in text
    uint32_t *entLen = nullptr;    // [entries] sequence length of entry j (without "\n\0")
    char *text = nullptr;          // [bytes]
};

namespace {
constexpr int PM_WAVES = 4, PM_STAGE = 512;

// FLASH's complement_tab (read.cpp:4-13): IUPAC codes and lower case to their complements, U -> A, everything else '.'
__device__ __forceinline__ char pmComp(char c) {
    switch (c) {
        case 'A': return 'T'; case 'B': return 'V'; case 'C': return 'G'; case 'D': return 'H'; case 'G': return 'C'; case 'H': return 'D';
        case 'K': return 'M'; case 'M': return 'K'; case 'N': return 'N'; case 'R': return 'Y'; case 'S': return 'S'; case 'T': return 'A';
        case 'U': return 'A'; case 'V': return 'B'; case 'W': return 'W'; case 'Y': return 'R';
        case 'a': return 't'; case 'b': return 'v'; case 'c': return 'g'; case 'd': return 'h'; case 'g': return 'c'; case 'h': return 'd';
        case 'k': return 'm'; case 'm': return 'k'; case 'n': return 'n'; case 'r': return 'y'; case 's': return 's'; case 't': return 'a';
        case 'u': return 'a'; case 'v': return 'b'; case 'w': return 'w'; case 'y': return 'r';
        default: return '.';
    }
}
// the pair as the search sees it: R1 forward, R2 reverse-complemented (position j of R2' = complement of R2[L2 - 1 - j])
struct StagedPair {          // in LDS, complemented while staging
    const char *s1, *q1, *s2, *q2;
    __device__ char a(int i) const { return s1[i]; }
    __device__ int qa(int i) const { return q1[i]; }
    __device__ char b(int j) const { return s2[j]; }
    __device__ int qb(int j) const { return q2[j]; }
};
struct GlobalPair {          // straight from the batch
    const char *s1, *q1, *s2, *q2; int L2;
    __device__ char a(int i) const { return s1[i]; }
    __device__ int qa(int i) const { return q1[i]; }
    __device__ char b(int j) const { return pmComp(s2[L2 - 1 - j]); }
    __device__ int qb(int j) const { return q2[L2 - 1 - j]; }
};

// the best shift of this pair (-1: not combined); every lane of the wave calls it and gets the same answer
template <typename P>
__device__ int bestShift(const P &p, int L1, int L2, int minOv, int maxOv, float maxDens) {
    const int lane = threadIdx.x & 63;
    const int start = max(0, L1 - L2), end = L1 - minOv + 1;
    float bd = maxDens + 1.0f, bq = 0.0f; int bi = INT_MAX;
    for (int i = start + lane; i < end; i += 64) {
        const int len = L1 - i;
        // the score length is at most min(len, maxOv) (positions with an 'N' only shorten it): from mmStop mismatches on, the density is
        // above maxDens whatever the rest of the overlap holds - the shift can not be selected (the smallest mmStop, in float as below).
        // An overlap has at most len mismatches: len + 1 never stops the walk, and it bounds both searches whatever maxDens is.
        const float capf = (float) min(len, maxOv), guess = maxDens * capf;
        const int lim = len + 1;
        int mmStop = guess >= (float) lim ? lim : max(1, (int) guess);
        while (mmStop > 1 && (float) (mmStop - 1) / capf > maxDens) mmStop--;
        while (mmStop < lim && (float) mmStop / capf <= maxDens) mmStop++;
        unsigned mm = 0, qs = 0; int nN = 0; bool out = false;
        for (int k = 0; k < len; k++) {
            const char x = p.a(i + k), y = p.b(k);
            if (x == 'N' || y == 'N') nN++;
            else if (x != y) {
                mm++; qs += (unsigned) min(p.qa(i + k), p.qb(k));
                if ((int) mm >= mmStop) { out = true; break; }
            }
        }
        if (out) continue;
        const int ov = len - nN;
        if (ov < minOv) continue;
        const float sl = (float) min(ov, maxOv);
        const float q = (float) qs / sl, d = (float) mm / sl;
        if (d <= bd && (d < bd || q < bq)) { bd = d; bq = q; bi = i; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float od = __shfl_xor(bd, o, 64), oq = __shfl_xor(bq, o, 64); const int oi = __shfl_xor(bi, o, 64);
        if (od < bd || (od == bd && (oq < bq || (oq == bq && oi < bi)))) { bd = od; bq = oq; bi = oi; }
    }
    return (bi == INT_MAX || bd > maxDens) ? -1 : bi;
}

__global__ __launch_bounds__(64 * PM_WAVES) void k_pair_align(const char *__restrict__ seq1, const char *__restrict__ qual1, const uint64_t *__restrict__ off1,
                                                              const uint32_t *__restrict__ len1, const char *__restrict__ seq2, const char *__restrict__ qual2,
                                                              const uint64_t *__restrict__ off2, const uint32_t *__restrict__ len2, uint64_t n, uint64_t first,
                                                              int minOv, int maxOv, float maxDens, int32_t *__restrict__ pos, uint64_t *__restrict__ bytes,
                                                              uint32_t *__restrict__ ents, unsigned int *__restrict__ badQual) {
    __shared__ char sS1[PM_WAVES][PM_STAGE], sQ1[PM_WAVES][PM_STAGE], sS2[PM_WAVES][PM_STAGE], sQ2[PM_WAVES][PM_STAGE];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t pr = first + (uint64_t) blockIdx.x * PM_WAVES + w;
    if (pr >= n) return;                 // (a whole wave: nothing below synchronises beyond the wave)
    const int L1 = (int) len1[pr], L2 = (int) len2[pr];
    const char *s1 = seq1 + off1[pr], *q1 = qual1 + off1[pr], *s2 = seq2 + off2[pr], *q2 = qual2 + off2[pr];
    // qualities are compared as signed char in the reference's scalar code and as unsigned bytes in its SSE code: they agree below 0x80 only
    bool bad = false;
    for (int j = lane; j < L1; j += 64) bad |= (q1[j] & 0x80) != 0;
    for (int j = lane; j < L2; j += 64) bad |= (q2[j] & 0x80) != 0;
    if (__ballot(bad)) { if (lane == 0) atomicOr(badQual, 1u); }
    int b;
    if (L1 <= PM_STAGE && L2 <= PM_STAGE) {
        for (int j = lane; j < L1; j += 64) { sS1[w][j] = s1[j]; sQ1[w][j] = q1[j]; }
        for (int j = lane; j < L2; j += 64) { sS2[w][j] = pmComp(s2[L2 - 1 - j]); sQ2[w][j] = q2[L2 - 1 - j]; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        b = bestShift(StagedPair{sS1[w], sQ1[w], sS2[w], sQ2[w]}, L1, L2, minOv, maxOv, maxDens);
    } else {
        b = bestShift(GlobalPair{s1, q1, s2, q2, L2}, L1, L2, minOv, maxOv, maxDens);
    }
    if (lane == 0) {
        pos[pr] = b;
        bytes[pr] = b >= 0 ? (uint64_t) (b + L2) + 2 : (uint64_t) L1 + 2 + (uint64_t) L2 + 2;
        ents[pr] = b >= 0 ? 1u : 2u;
    }
}
// the entries' text: combined - R1's prefix, the overlap (equal bases kept, else the base with the higher quality, on equal qualities
// R2's unless it is 'N'; generate_combined_read, combine_reads.cpp:338-446), R2's tail; not combined - R1, then R2 reverse-complemented
__global__ __launch_bounds__(256) void k_pair_emit(const char *__restrict__ seq1, const char *__restrict__ qual1, const uint64_t *__restrict__ off1,
                                                   const uint32_t *__restrict__ len1, const char *__restrict__ seq2, const char *__restrict__ qual2,
                                                   const uint64_t *__restrict__ off2, const uint32_t *__restrict__ len2, uint64_t n, uint64_t first,
                                                   const int32_t *__restrict__ pos, const uint64_t *__restrict__ textOff, const uint32_t *__restrict__ entIdx,
                                                   char *__restrict__ text, uint64_t *__restrict__ entOff, uint32_t *__restrict__ entLen,
                                                   uint8_t *__restrict__ status, uint32_t *__restrict__ mlen) {
    const int lane = threadIdx.x & 63;
    const uint64_t pr = first + (((uint64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (pr >= n) return;
    const int L1 = (int) len1[pr], L2 = (int) len2[pr], b = pos[pr];
    const char *s1 = seq1 + off1[pr], *q1 = qual1 + off1[pr], *s2 = seq2 + off2[pr], *q2 = qual2 + off2[pr];
    char *o = text + textOff[pr];
    const uint32_t e = entIdx[pr];
    if (b >= 0) {
        const int Lc = b + L2;
        for (int k = lane; k < Lc; k += 64) {
            char c;
            if (k < b) c = s1[k];
            else {
                const char y = pmComp(s2[L2 - 1 - (k - b)]);
                if (k >= L1) c = y;
                else {
                    const char x = s1[k]; const int qx = q1[k], qy = q2[L2 - 1 - (k - b)];
                    c = (x == y || qx > qy) ? x : qx < qy ? y : (y == 'N' ? x : y);
                }
            }
            o[k] = c;
        }
        if (lane == 0) { o[Lc] = '\n'; o[Lc + 1] = '\0'; entOff[e] = textOff[pr]; entLen[e] = (uint32_t) Lc; status[pr] = 1; mlen[pr] = (uint32_t) Lc; }
    } else {
        for (int k = lane; k < L1; k += 64) o[k] = s1[k];
        char *o2 = o + L1 + 2;
        for (int k = lane; k < L2; k += 64) o2[k] = pmComp(s2[L2 - 1 - k]);
        if (lane == 0) {
            o[L1] = '\n'; o[L1 + 1] = '\0'; o2[L2] = '\n'; o2[L2 + 1] = '\0';
            entOff[e] = textOff[pr]; entLen[e] = (uint32_t) L1; entOff[e + 1] = textOff[pr] + L1 + 2; entLen[e + 1] = (uint32_t) L2;
            status[pr] = 0; mlen[pr] = 0;
        }
    }
}
template <typename T> struct LoadOrZero { const T *p; uint64_t n; __device__ __forceinline__ T operator()(size_t i) const { return i < n ? p[i] : (T) 0; } };
}  // namespace

extern "C" int cdm_pairs_merge(cdm_ctx *ctx, const char *seq1, const char *qual1, const uint64_t *off1, const uint32_t *len1,
                               const char *seq2, const char *qual2, const uint64_t *off2, const uint32_t *len2, uint64_t n,
                               const cdm_merge_params *par, cdm_pairs **out) {
    if (!ctx || !out || (n && (!seq1 || !qual1 || !off1 || !len1 || !seq2 || !qual2 || !off2 || !len2))) { cdm_set_error("cdm_pairs_merge: NULL argument"); return CDM_ERR_INVALID; }
    cdm_merge_params P = par ? *par : cdm_merge_params{15, 65, 0.10f};
    // (a density above 1e6 is no bound at all: no overlap of reads the parser accepts reaches it - and NaN / inf are no numbers to compare)
    if (P.min_overlap < 1 || P.max_overlap < 1 || !(P.max_mismatch_density >= 0.0f && P.max_mismatch_density <= 1e6f)) {
        cdm_set_error("cdm_pairs_merge: invalid parameters (min_overlap, max_overlap >= 1; 0 <= max_mismatch_density <= 1e6)"); return CDM_ERR_INVALID;
    }
    if (n >= 0x7FFFFFFFull) { cdm_set_error("cdm_pairs_merge: more than 2^31-1 pairs in one batch"); return CDM_ERR_UNSUPPORTED; }
    CDM_HIP(hipSetDevice(ctx->device));
    // the byte ranges of the batch in the caller's blobs (one copy each; the kernels index relative to their start)
    uint64_t lo1 = UINT64_MAX, hi1 = 0, lo2 = UINT64_MAX, hi2 = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (len1[i] == 0 || len2[i] == 0) { cdm_set_error("cdm_pairs_merge: pair %llu has an empty read (mergereads: \"Invalid sequence record found\")", (unsigned long long) i); return CDM_ERR_INVALID; }
        if (len1[i] > (1u << 30) || len2[i] > (1u << 30)) { cdm_set_error("cdm_pairs_merge: pair %llu has a read of more than 2^30 bases", (unsigned long long) i); return CDM_ERR_UNSUPPORTED; }
        lo1 = std::min(lo1, off1[i]); hi1 = std::max(hi1, off1[i] + len1[i]);
        lo2 = std::min(lo2, off2[i]); hi2 = std::max(hi2, off2[i] + len2[i]);
    }
    if (n == 0) lo1 = lo2 = 0;
    std::vector<uint64_t> r1(n), r2(n);
    for (uint64_t i = 0; i < n; i++) { r1[i] = off1[i] - lo1; r2[i] = off2[i] - lo2; }
    hipStream_t s = ctx->stream;
    DevBuf<char> dS1, dQ1, dS2, dQ2; DevBuf<uint64_t> dO1, dO2, dBytes, dTextOff; DevBuf<uint32_t> dL1, dL2, dEnts, dEntIdx; DevBuf<int32_t> dPos; DevBuf<unsigned int> dBad;
    if (!dS1.alloc(hi1 - lo1) || !dQ1.alloc(hi1 - lo1) || !dS2.alloc(hi2 - lo2) || !dQ2.alloc(hi2 - lo2) || !dO1.alloc(n) || !dO2.alloc(n) || !dL1.alloc(n) || !dL2.alloc(n) ||
        !dBytes.alloc(n) || !dTextOff.alloc(n + 1) || !dEnts.alloc(n) || !dEntIdx.alloc(n + 1) || !dPos.alloc(n) || !dBad.alloc(1)) {
        cdm_set_error("out of device memory staging a batch of %llu pairs", (unsigned long long) n); return CDM_ERR_HIP;
    }
    cdm_pairs *h = new cdm_pairs();
    h->n = n; h->device = ctx->device;
    auto fail = [&](const char *what) { cdm_set_error("cdm_pairs_merge: %s: %s", what, hipGetErrorString(hipGetLastError())); cdm_pairs_free(h); return CDM_ERR_HIP; };
    hipMemsetAsync(dBad.p, 0, 4, s);
    if (n) {
        hipMemcpyAsync(dS1.p, seq1 + lo1, hi1 - lo1, hipMemcpyHostToDevice, s); hipMemcpyAsync(dQ1.p, qual1 + lo1, hi1 - lo1, hipMemcpyHostToDevice, s);
        hipMemcpyAsync(dS2.p, seq2 + lo2, hi2 - lo2, hipMemcpyHostToDevice, s); hipMemcpyAsync(dQ2.p, qual2 + lo2, hi2 - lo2, hipMemcpyHostToDevice, s);
        hipMemcpyAsync(dO1.p, r1.data(), n * 8, hipMemcpyHostToDevice, s); hipMemcpyAsync(dO2.p, r2.data(), n * 8, hipMemcpyHostToDevice, s);
        hipMemcpyAsync(dL1.p, len1, n * 4, hipMemcpyHostToDevice, s); hipMemcpyAsync(dL2.p, len2, n * 4, hipMemcpyHostToDevice, s);
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const bool timed = hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    if (timed) hipEventRecord(e0, s);
    const uint64_t slice = cdmSliceItems(64);
    for (uint64_t f = 0; f < n; f += slice) {
        const uint64_t m = std::min(slice, n - f);
        hipLaunchKernelGGL(k_pair_align, CDM_GRID((m + PM_WAVES - 1) / PM_WAVES, 64 * PM_WAVES), dim3(64 * PM_WAVES), 0, s, dS1.p, dQ1.p, dO1.p, dL1.p, dS2.p, dQ2.p, dO2.p, dL2.p,
                           n, f, P.min_overlap, P.max_overlap, P.max_mismatch_density, dPos.p, dBytes.p, dEnts.p, dBad.p);
    }
    cdmscan::ScanTemp t1, t2;
    int rc = cdmscan::exclusiveScanFn<uint64_t>(s, t1, LoadOrZero<uint64_t>{dBytes.p, n}, dTextOff.p, n + 1);
    if (!rc) rc = cdmscan::exclusiveScanFn<uint32_t>(s, t2, LoadOrZero<uint32_t>{dEnts.p, n}, dEntIdx.p, n + 1);
    if (rc) {       // (the search may still be running on the buffers the DevBufs give back on return)
        (void) hipStreamSynchronize(s);
        if (timed) { hipEventDestroy(e0); hipEventDestroy(e1); }
        cdm_pairs_free(h); return rc;
    }
    uint64_t tot = 0; uint32_t ents = 0; unsigned int bad = 0;
    hipMemcpyAsync(&tot, dTextOff.p + n, 8, hipMemcpyDeviceToHost, s); hipMemcpyAsync(&ents, dEntIdx.p + n, 4, hipMemcpyDeviceToHost, s);
    hipMemcpyAsync(&bad, dBad.p, 4, hipMemcpyDeviceToHost, s);
    if (hipStreamSynchronize(s) != hipSuccess) { if (timed) { hipEventDestroy(e0); hipEventDestroy(e1); } return fail("overlap search"); }
    if (bad) {
        if (timed) { hipEventDestroy(e0); hipEventDestroy(e1); }
        cdm_pairs_free(h);
        cdm_set_error("cdm_pairs_merge: a quality byte >= 0x80 (not FASTQ; the reference's SSE and scalar paths disagree on it)");
        return CDM_ERR_UNSUPPORTED;
    }
    h->bytes = tot; h->entries = ents;
    if (cdmMalloc(&h->status, n + 1) != hipSuccess || cdmMalloc(&h->mlen, (n + 1) * 4) != hipSuccess || cdmMalloc(&h->entOff, (ents + 1) * 8) != hipSuccess ||
        cdmMalloc(&h->entLen, (ents + 1) * 4) != hipSuccess || cdmMalloc(&h->text, tot + 16) != hipSuccess) {
        if (timed) { hipEventDestroy(e0); hipEventDestroy(e1); }
        cdm_pairs_free(h); cdm_set_error("out of device memory for the merged text of %llu pairs (%llu bytes)", (unsigned long long) n, (unsigned long long) tot); return CDM_ERR_HIP;
    }
    const uint64_t eslice = cdmSliceItems(64);
    for (uint64_t f = 0; f < n; f += eslice) {
        const uint64_t m = std::min(eslice, n - f);
        hipLaunchKernelGGL(k_pair_emit, CDM_GRID((m + 3) / 4, 256), dim3(256), 0, s, dS1.p, dQ1.p, dO1.p, dL1.p, dS2.p, dQ2.p, dO2.p, dL2.p, n, f, dPos.p, dTextOff.p, dEntIdx.p,
                           h->text, h->entOff, h->entLen, h->status, h->mlen);
    }
    if (timed) hipEventRecord(e1, s);
    if (hipStreamSynchronize(s) != hipSuccess) { if (timed) { hipEventDestroy(e0); hipEventDestroy(e1); } return fail("merged text"); }
    if (timed) { float ms = 0.f; if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) h->kernelMs = ms; hipEventDestroy(e0); hipEventDestroy(e1); }
    *out = h;
    return CDM_OK;
}
extern "C" uint64_t cdm_pairs_count(const cdm_pairs *h) { return h->n; }
extern "C" uint64_t cdm_pairs_entries(const cdm_pairs *h) { return h->entries; }
extern "C" uint64_t cdm_pairs_bytes(const cdm_pairs *h) { return h->bytes; }
extern "C" float cdm_pairs_kernel_ms(const cdm_pairs *h) { return h->kernelMs; }
extern "C" int cdm_pairs_download(cdm_ctx *ctx, const cdm_pairs *h, uint8_t *status, uint32_t *merged_len, char *text, uint32_t *entry_len) {
    if (!ctx || !h) { cdm_set_error("cdm_pairs_download: NULL argument"); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    if (status && h->n) CDM_HIP(hipMemcpyAsync(status, h->status, h->n, hipMemcpyDeviceToHost, ctx->stream));
    if (merged_len && h->n) CDM_HIP(hipMemcpyAsync(merged_len, h->mlen, h->n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (entry_len && h->entries) CDM_HIP(hipMemcpyAsync(entry_len, h->entLen, h->entries * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (text && h->bytes) CDM_HIP(hipMemcpyAsync(text, h->text, h->bytes, hipMemcpyDeviceToHost, ctx->stream));
    CDM_HIP(hipStreamSynchronize(ctx->stream));
    return CDM_OK;
}
extern "C" int cdm_pairs_download_stream(cdm_ctx *ctx, const cdm_pairs *h, uint64_t pieceBytes, int (*sink)(void *user, const char *data, uint64_t offset, uint64_t bytes), void *user) {
    if (!ctx || !h || !sink) { cdm_set_error("cdm_pairs_download_stream: invalid argument"); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    const uint64_t total = h->bytes;
    if (total == 0) return CDM_OK;
    if (pieceBytes < (1u << 20)) pieceBytes = 64u << 20;
    pieceBytes = std::min(pieceBytes, total);
    hipStream_t s = ctx->stream;
    char *pin[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr};
    auto cleanup = [&] { for (int b = 0; b < 2; b++) { if (pin[b]) (void) hipHostFree(pin[b]); if (ev[b]) (void) hipEventDestroy(ev[b]); } };
    for (int b = 0; b < 2; b++) if (hipHostMalloc((void **) &pin[b], pieceBytes, hipHostMallocDefault) != hipSuccess || hipEventCreateWithFlags(&ev[b], hipEventDisableTiming) != hipSuccess) {
        (void) hipGetLastError(); cleanup(); cdm_set_error("cdm_pairs_download_stream: no pinned staging buffer of %llu bytes", (unsigned long long) pieceBytes); return CDM_ERR_HIP;
    }
    const uint64_t pieces = (total + pieceBytes - 1) / pieceBytes;
    auto issue = [&](uint64_t i) { const uint64_t at = i * pieceBytes, nb = std::min(pieceBytes, total - at); hipMemcpyAsync(pin[i & 1], h->text + at, nb, hipMemcpyDeviceToHost, s); hipEventRecord(ev[i & 1], s); };
    issue(0);
    int rc = CDM_OK;
    for (uint64_t i = 0; i < pieces && rc == CDM_OK; i++) {
        // (piece i + 1 goes into the other buffer once the sink is done with piece i - 1, which it is: the sink runs on this thread)
        if (i + 1 < pieces) issue(i + 1);
        if (hipEventSynchronize(ev[i & 1]) != hipSuccess) { cdm_set_error("cdm_pairs_download_stream failed: %s", hipGetErrorString(hipGetLastError())); rc = CDM_ERR_HIP; break; }
        const uint64_t at = i * pieceBytes, nb = std::min(pieceBytes, total - at);
        if (sink(user, pin[i & 1], at, nb) != 0) { cdm_set_error("cdm_pairs_download_stream: the sink refused a piece at offset %llu", (unsigned long long) at); rc = CDM_ERR_INVALID; }
    }
    (void) hipStreamSynchronize(s);
    cleanup();
    return rc;
}
extern "C" int cdm_pairs_to_seqdb(cdm_ctx *ctx, const cdm_pairs *h, uint32_t first_key, cdm_seqdb **out) {
    if (!ctx || !h || !out) { cdm_set_error("cdm_pairs_to_seqdb: NULL argument"); return CDM_ERR_INVALID; }
    if (h->entries == 0) { cdm_set_error("cdm_pairs_to_seqdb: no entries"); return CDM_ERR_INVALID; }
    if ((uint64_t) first_key + h->entries > 0xFFFFFFFFull) { cdm_set_error("cdm_pairs_to_seqdb: keys beyond 2^32-1"); return CDM_ERR_UNSUPPORTED; }
    CDM_HIP(hipSetDevice(ctx->device));
    return cdm_seqdb_from_device_text(ctx, h->text, h->entOff, h->entLen, h->entries, first_key, 1 /* as mergereads writes them */, out);
}
extern "C" void cdm_pairs_free(cdm_pairs *h) {
    if (!h) return;
    hipSetDevice(h->device);
    cdmFree(h->status); cdmFree(h->mlen); cdmFree(h->entOff); cdmFree(h->entLen); cdmFree(h->text);
    delete h;
}
