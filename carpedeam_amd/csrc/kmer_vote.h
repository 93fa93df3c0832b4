// kmermatcher on the device (kmermatch.hip), stage K4:
//   K4 k_seg_count/place   writeKmerMatcherResult :815-930  per (rep, target): shared k-mer count, most frequent diagonal
//                     (last maximum wins), strand of that diagonal's last tuple; every sequence gets a record that starts
//                     with its self hit (fill-in :717-729)
// Quirk kept on purpose (observable in the prefilter DB): the per-target scan in the writer running on into the next
// representative's tuples when they have the same target id (:875-887).
#pragma once
#include "common.h"
#include "devutil.h"

namespace {

// tiles of the vote kernels: 4096 keys (256 threads x 16 consecutive items)
// (2048 keys: the place kernel runs on blocks in flight - 35 KB of LDS per block gave 4 per CU and 19 ms)
#ifndef CDM_CP_ITEMS
#define CDM_CP_ITEMS 8
#endif
constexpr int CP_ITEMS = CDM_CP_ITEMS, CP_TILE = 256 * CP_ITEMS;
static_assert(CP_ITEMS == 8 || CP_ITEMS == 16, "vote tile: the start bits of a thread are one byte or one 16-bit word");
template <int N> struct BitsOf { typedef uint16_t T; };
template <> struct BitsOf<8> { typedef uint8_t T; };
typedef BitsOf<CP_ITEMS>::T CpBits;
// LDS index with one pad slot per 16 items: thread t walks items 16t..16t+15 without bank conflicts
__device__ __forceinline__ int padIdx(int i) { return i + (i >> 4); }
constexpr int CP_LDS = CP_TILE + CP_TILE / 16 + 1;

// ------------------------------------------------------------------------------------------------ K4: vote
struct VoteArgs {
    const uint64_t *keys;   // sorted (rep, id, diag), strand in bit 0
    uint64_t n;
    uint32_t idBits, diagBits; int diagBias;
    unsigned long long *perRep;  // [nSeq] number of hits per representative
    // The reference's per-target scan does not stop at the end of the sorted group tuples: it runs on into the tuples that
    // assignGroup's in-place compaction left behind (kmermatcher.cpp:875-887 reads hashSeqPair[kmerPos + kmerOffset].id up to
    // the end of the array), i.e. the k-mer-ordered tuples from index nGroup on, while their sequence id equals the target.
    // stale[0] = number of such tuples, stale[1] = their sequence id, stale[2..] their positions (k_stale_tail); their k-mer
    // field is UINT64_MAX by then, so they count as forward.
    const uint32_t *stale;
    // Multi-GPU runs (every rank votes on the representatives it owns): what the scan of this rank's LAST segment runs into is
    // the head of the next rank's sorted array - cont[0] entries (cont[3 + j] = biased diagonal | "reverse" << 31) that apply if
    // the target is cont[1]; only if cont[2] is set does the scan go on into the left-over tuples (`stale`) after them.  NULL on
    // a single device.
    const uint32_t *cont;
};
constexpr int CONT_CAP = 2048;
// a (rep, target != rep) segment starts at i
__device__ __forceinline__ bool validStart(const VoteArgs &a, uint64_t i, uint32_t &rep, uint32_t &target) {
    const uint64_t seg = a.keys[i] >> (a.diagBits + 1);
    if (i > 0 && (a.keys[i - 1] >> (a.diagBits + 1)) == seg) return false;
    target = (uint32_t) (seg & ((1ull << a.idBits) - 1)); rep = (uint32_t) (seg >> a.idBits);
    return target != rep;   // self tuples give no hit (:898-903)
}
// tiles of 4096 tuples: number of hit-producing segment starts per tile and per representative (coalesced, order free)
__global__ __launch_bounds__(256) void k_seg_count(VoteArgs a, unsigned long long *__restrict__ tileCnt) {
    const uint64_t base = (uint64_t) blockIdx.x * CP_TILE;
    unsigned int c = 0;
#pragma unroll
    for (int j = 0; j < CP_ITEMS; j++) {
        const uint64_t i = base + threadIdx.x + 256 * j;
        uint32_t rep, target;
        if (i < a.n && validStart(a, i, rep, target)) { c++; atomicAdd(&a.perRep[rep], 1ull); }
    }
    const unsigned int tot = cdm_block_sum<unsigned int>(c);
    if (threadIdx.x == 0) tileCnt[blockIdx.x] = tot;
}
// vote of the segment starting at tile-local index li, reading the tile from LDS and whatever lies beyond it from memory
__device__ __forceinline__ HitRec voteSegmentTile(const VoteArgs &a, const uint64_t *sKeys, uint64_t base, int li, uint32_t target) {
    const uint64_t idMask = (1ull << a.idBits) - 1, diagMask = (1ull << a.diagBits) - 1;
    const uint64_t key = sKeys[padIdx(li)];
    uint32_t prevDiag = (uint32_t) ((key >> 1) & diagMask), diagonal = prevDiag;
    uint32_t maxDiag = 0, diagCnt = 0, top = 0; int bestRev = (key & 1ull) ? 0 : 1;
    // two separate loops so that the common in-tile walk issues LDS reads only
    const int tileEnd = (int) min((uint64_t) CP_TILE, a.n - base);
    int i = li; bool done = false;
    for (; i < tileEnd; i++) {
        const uint64_t k2 = sKeys[padIdx(i)];
        if ((uint32_t) ((k2 >> (a.diagBits + 1)) & idMask) != target) { done = true; break; }
        const uint32_t d = (uint32_t) ((k2 >> 1) & diagMask);
        if (prevDiag == d) diagCnt++; else diagCnt = 1;
        if (diagCnt >= maxDiag) { diagonal = d; maxDiag = diagCnt; bestRev = (k2 & 1ull) ? 0 : 1; }
        prevDiag = d; top++;
    }
    if (!done) {
        for (uint64_t kk = base + CP_TILE; kk < a.n; kk++) {
            const uint64_t k2 = a.keys[kk];
            if ((uint32_t) ((k2 >> (a.diagBits + 1)) & idMask) != target) { done = true; break; }
            const uint32_t d = (uint32_t) ((k2 >> 1) & diagMask);
            if (prevDiag == d) diagCnt++; else diagCnt = 1;
            if (diagCnt >= maxDiag) { diagonal = d; maxDiag = diagCnt; bestRev = (k2 & 1ull) ? 0 : 1; }
            prevDiag = d; top++;
        }
    }
    bool intoStale = !done;
    if (!done && a.cont) {                      // the scan reached the end of this rank's group tuples: on into the next ranks'
        if (target == a.cont[1]) {
            const uint32_t m = a.cont[0];
            for (uint32_t j = 0; j < m; j++) {
                const uint32_t e = a.cont[3 + j], d = e & 0x7FFFFFFFu;
                if (prevDiag == d) diagCnt++; else diagCnt = 1;
                if (diagCnt >= maxDiag) { diagonal = d; maxDiag = diagCnt; bestRev = (int) (e >> 31); }
                prevDiag = d; top++;
            }
        }
        intoStale = a.cont[2] != 0u;
    }
    if (intoStale && target == a.stale[1]) {    // the scan reached the end of all group tuples: on into the left-over ones
        const uint32_t m = a.stale[0];
        for (uint32_t j = 0; j < m; j++) {
            const uint32_t d = a.stale[2 + j] + (uint32_t) a.diagBias;
            if (prevDiag == d) diagCnt++; else diagCnt = 1;
            if (diagCnt >= maxDiag) { diagonal = d; maxDiag = diagCnt; bestRev = 0; }
            prevDiag = d; top++;
        }
    }
    HitRec h;
    h.target = target;
    h.score = bestRev ? -(int) top : (int) top;
    h.diagonal = (int) (short) ((int) diagonal - a.diagBias);
    return h;
}
__global__ __launch_bounds__(256) void k_seg_place(VoteArgs a, const unsigned long long *__restrict__ tileOff, const unsigned long long *__restrict__ perRepScan,
                                                   const uint64_t *__restrict__ off, HitRec *__restrict__ out) {
    __shared__ uint64_t sKeys[CP_LDS];
    __shared__ uint64_t sPrev;
    __shared__ __align__(8) CpBits sFirst[256 + 32 / sizeof(CpBits)];       // "starts a (rep, target) segment" bits, CP_ITEMS per thread = one bit array
    const uint64_t base = (uint64_t) blockIdx.x * CP_TILE;
#pragma unroll
    for (int j = 0; j < CP_ITEMS; j++) { const int li = threadIdx.x + 256 * j; const uint64_t i = base + li; sKeys[padIdx(li)] = (i < a.n) ? a.keys[i] : ~0ull; }
    if (threadIdx.x == 0) sPrev = base ? a.keys[base - 1] : ~0ull;
    if (threadIdx.x < 32 / sizeof(CpBits)) sFirst[256 + threadIdx.x] = 0;
    __syncthreads();
    const int shift = a.diagBits + 1;
    const uint64_t idMask = (1ull << a.idBits) - 1, diagMask = (1ull << a.diagBits) - 1;
    const int tileEnd = (int) min((uint64_t) CP_TILE, a.n - base);
    unsigned int c = 0, mask = 0, firstBits = 0;
#pragma unroll
    for (int j = 0; j < CP_ITEMS; j++) {
        const int li = threadIdx.x * CP_ITEMS + j;
        if (li >= tileEnd) break;
        const uint64_t seg = sKeys[padIdx(li)] >> shift;
        const uint64_t prevSeg = ((li == 0) ? sPrev : sKeys[padIdx(li - 1)]) >> shift;
        const bool first = (base + li == 0) || prevSeg != seg;
        if (first) firstBits |= 1u << j;
        if (first && (uint32_t) (seg & idMask) != (uint32_t) (seg >> a.idBits)) { c++; mask |= 1u << j; }
    }
    sFirst[threadIdx.x] = (CpBits) firstBits;
    unsigned int pre, totC;
    pre = cdm_block_excl_sum<unsigned int>(c, totC);       // (its barriers also publish sFirst)
    unsigned long long rank = tileOff[blockIdx.x] + pre;   // number of hit-producing segments before this one, whole array
    const unsigned long long *firstWords = reinterpret_cast<const unsigned long long *>(sFirst);
#pragma unroll 1
    while (mask) {   // one copy of the walk in the instruction stream (an unrolled x16 body thrashes the instruction cache)
        const int j = __ffs(mask) - 1;
        mask &= mask - 1;
        const int li = threadIdx.x * CP_ITEMS + j;
        const uint64_t k0 = sKeys[padIdx(li)], seg = k0 >> shift;
        const uint32_t target = (uint32_t) (seg & idMask), rep = (uint32_t) (seg >> a.idBits);
        // Most segments are one run of one diagonal that ends where the next segment starts: the next start is the next set bit
        // of the bit array; if the tuple there has another target id (no run-on into the next representative) and the first
        // and last tuples of the segment agree on the diagonal (they are sorted by it), the vote is known without a walk.
        HitRec h; bool quick = false;
        {
            int e = -1;
            for (int w = (li + 1) >> 6; w < CP_TILE / 64 && e < 0; w++) {
                unsigned long long m = firstWords[w];
                if (w == ((li + 1) >> 6)) m &= ~0ull << ((li + 1) & 63);
                if (m) e = w * 64 + __ffsll(m) - 1;
            }
            if (e > 0 && e < tileEnd) {
                const uint64_t kn = sKeys[padIdx(e)], kl = sKeys[padIdx(e - 1)];
                if ((uint32_t) ((kn >> shift) & idMask) != target && ((k0 >> 1) & diagMask) == ((kl >> 1) & diagMask)) {
                    h.target = target;
                    h.score = (kl & 1ull) ? (e - li) : -(e - li);
                    h.diagonal = (int) (short) ((int) ((k0 >> 1) & diagMask) - a.diagBias);
                    quick = true;
                }
            }
        }
        if (!quick) h = voteSegmentTile(a, sKeys, base, li, target);
        out[off[rep] + 1 + (rank - perRepScan[rep])] = h;
        rank++;
    }
}
// The head of a sorted group-key array: the tuples from its start on while they have the target id of the first one, whatever
// their representative (what a scan coming in from the rank in front runs through, kmermatcher.cpp:875-887).
// out[0] = count (CONT_CAP + 1: longer than the list), out[1] = that id, out[2] = 1 if the head is the whole array, out[3..] entries
__global__ void k_head_segment(const uint64_t *__restrict__ keys, uint64_t n, uint32_t idBits, uint32_t diagBits, uint32_t *__restrict__ out) {
    const uint64_t idMask = (1ull << idBits) - 1ull, diagMask = (1ull << diagBits) - 1ull;
    if (n == 0) { out[0] = 0; out[1] = 0; out[2] = 1; return; }
    const uint32_t id = (uint32_t) ((keys[0] >> (diagBits + 1)) & idMask);
    uint64_t c = 0;
    for (; c < n && c <= (uint64_t) CONT_CAP; c++) {
        const uint64_t k2 = keys[c];
        if ((uint32_t) ((k2 >> (diagBits + 1)) & idMask) != id) break;
        if (c < (uint64_t) CONT_CAP) out[3 + c] = (uint32_t) ((k2 >> 1) & diagMask) | ((k2 & 1ull) ? 0u : 1u << 31);
    }
    out[0] = (uint32_t) c; out[1] = id; out[2] = (c == n) ? 1u : 0u;
}
__global__ void k_offsets(const unsigned long long *__restrict__ perRepScan, uint32_t n, uint64_t *__restrict__ off) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q <= n) off[q] = (uint64_t) q + perRepScan[q];        // one self hit per sequence in front of its own hits
}
__global__ void k_self(const uint64_t *__restrict__ off, uint32_t n, HitRec *__restrict__ out) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    HitRec h; h.target = q; h.score = 0; h.diagonal = 0;
    out[off[q]] = h;
}
// first index of `keys` (sorted by representative) whose representative is >= bound[t]
__global__ void k_rep_bounds(const uint64_t *__restrict__ keys, uint64_t n, int repShift, const uint64_t *__restrict__ bound, int nb, unsigned long long *__restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nb) return;
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if ((keys[mid] >> repShift) < bound[t]) lo = mid + 1; else hi = mid; }
    out[t] = lo;
}

}  // namespace
