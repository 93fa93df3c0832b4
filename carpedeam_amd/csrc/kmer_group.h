// kmermatcher on the device (kmermatch.hip), stage K3 and what sort 1 and sort 2 need around it:
//   K3 k_bucket_groups (k_groups)   assignGroup :453-562  first sequence of every k-mer run by (length desc, id, pos) is the
//                     representative; members become (rep, id, diagonal, strand); singletons dropped.  Fused with the
//                     on-chip part of sort 1 (bucket.h)
// the run records of sort 2 that the grouping kernel stages (runsort.h), the left-over tuples of the reference's last per-target scan
// (k_stale_tail), and the small counting kernels.
// Quirk kept on purpose (observable in the prefilter DB): repIsReverse starting as false for the very first k-mer group (:453-467).
#pragma once
#include "kmer_tuple.h"
#include "runsort.h"

namespace {

// ------------------------------------------------------------------------------------------------ K3: groups
struct GroupParams {
    uint64_t n;
    int onlyExtendable, covMode; float covThr;
    uint32_t idBits, diagBits; int diagBias;
    int wide;                   // group keys without the representative (runsort.h: GK_START / GK_DROPPED mark the run starts)
    uint64_t first;             // the kernel covers the tuples [first, n)
    uint64_t firstRunIdx;       // index of the array's very first tuple in this view (0; ~0 if the view does not hold it)
    unsigned long long *stat;   // STAT_STRIPES counters: members kept
};
// Count of kept members, one atomic per wave, striped over many addresses: millions of waves hitting one counter serialise
// (370 ms instead of 53 for k_bucket_groups at 50 M reads).  cnt is wave-uniform.
constexpr int STAT_STRIPES = 4096;
__device__ __forceinline__ void waveGroupStats(unsigned long long *stat, uint32_t cnt) {
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(stat + ((blockIdx.x * 4 + (threadIdx.x >> 6)) & (STAT_STRIPES - 1)), (unsigned long long) cnt);
}
template <typename LY> struct GroupArgs : GroupParams {
    const uint64_t *keys; const typename LY::V *vals;   // sorted by k-mer
    TupleGeom geom;
};
__device__ __forceinline__ bool canBeCoveredK(float covThr, int covMode, float ql, float tl) {
    switch (covMode) {
        case 0: return ((ql / tl >= covThr) && (tl / ql >= covThr));
        case 2: return ((tl / ql) >= covThr);
        case 1: return ((ql / tl) >= covThr);
        case 3: return ((tl / ql) >= covThr) && (tl / ql) <= 1.0;
        case 4: return ((ql / tl) >= covThr) && (ql / tl) <= 1.0;
        case 5: return (fminf(tl, ql) / fmaxf(tl, ql)) >= covThr;
        default: return true;
    }
}
// key layout of the second sort: [ rep | id | diagonal + bias | strand ] , strand (1 = query needs no reversal) in bit 0; the wide form
// (DBs whose ids and diagonals do not leave room for the representative in 63 bits) is [ id | diagonal + bias | strand ]
__device__ __forceinline__ uint64_t packGroupKey(const GroupParams &a, uint32_t rep, uint32_t id, int diag, bool noRev) {
    const uint64_t hi = a.wide ? (uint64_t) id : (((uint64_t) rep << a.idBits) | id);
    return (hi << (a.diagBits + 1)) | ((uint64_t) (uint32_t) (diag + a.diagBias) << 1) | (noRev ? 1ull : 0ull);
}
// wide form: the first slot of a k-mer run with members names the representative (its own tuple: id == rep), kept or not
__device__ __forceinline__ uint64_t markRunStart(const GroupParams &a, uint64_t gk, uint32_t rep) {
    return (runsort::gkKept(gk) ? gk : (runsort::GK_DROPPED | ((uint64_t) rep << (a.diagBits + 1)))) | runsort::GK_START;
}
// run start index of every tuple = inclusive max-scan of (start ? i : 0); fed to the scan through this functor
template <typename LY> struct StartIndex {
    const uint64_t *keys; TupleGeom geom; unsigned long long first;
    __device__ unsigned long long operator()(unsigned long long i) const {
        if (i == first) return i;
        const uint64_t a = keys[i], b = keys[i - 1];
        const bool start = (a == ~0ull) || (b == ~0ull) || (LY::kmerOf(a, i, geom) != LY::kmerOf(b, i - 1, geom));
        return start ? i : 0ull;
    }
};
template <typename LY> struct StartFrom {      // the scan's index starts at 0, the tuples at `first`
    StartIndex<LY> f;
    __device__ __forceinline__ unsigned long long operator()(size_t i) const { return f(f.first + (unsigned long long) i); }
};

// K3, one thread per tuple.  The tuple array was filled in (sequence length descending, id ascending, position) order and
// the radix sort is stable, so the first tuple of a k-mer run is the reference's representative (sort order
// kmermatcher.h:76-96); only a k-mer that the representative's own sequence carries twice needs a look at the next tuples.
// (rep, id, diagonal, strand) key of one member of a k-mer run, ~0 if the member is dropped (assignGroup :453-562)
__device__ __forceinline__ uint64_t groupKeyCore(const GroupParams &a, uint32_t repId, int queryLen, int repPos, bool repIsReverse,
                                                 uint32_t id, int tLen, int tPos0, bool targetIsReverse) {
    // the reference's four strand cases of assignGroup: a target on the reverse strand counts both positions from the other end -
    // qPos = (queryLen - 1) - repPos, tPos = (tLen - 1) - tPos0 -, and the query is reversed when the two strands differ.  As selects:
    // the four branches were an exec save / restore nest per member
    const bool qRev = repIsReverse != targetIsReverse;
    // (the reference holds positions and the diagonal in `short` below 32 765 letters and in `int` above, kmermatcher.cpp:803-808;
    // below that limit the casts never change a value, so one expression serves both paths)
    const int plain = repPos - tPos0;
    const int diagonal = targetIsReverse ? (queryLen - tLen) - plain : plain;
    const bool canBeExtended = diagonal < 0 || (diagonal > (queryLen - tLen));
    // coverage modes 0-2 with a threshold <= 0 hold for any two positive lengths: skip the divisions
    const bool cbc = (a.covThr <= 0.0f && a.covMode <= 2 && queryLen > 0 && tLen > 0) ? true : canBeCoveredK(a.covThr, a.covMode, (float) queryLen, (float) tLen);
    const bool keep = (a.onlyExtendable == 0 && cbc) || (canBeExtended && a.onlyExtendable != 0);
    return keep ? packGroupKey(a, repId, id, diagonal, !qRev) : ~0ull;
}
template <typename LY>
__device__ __forceinline__ uint64_t groupKeyOf(const GroupParams &a, const TupleGeom &geom, uint64_t repKey, typename LY::V repVal, uint64_t repSlot, uint32_t repPos0,
                                               bool firstRun, uint64_t key, typename LY::V v, uint64_t slot) {
    // the reference initialises repIsReverse = false and only updates it when a NEW run starts (:465,:535-538):
    // the very first run of the array keeps false whatever its strand
    return groupKeyCore(a, LY::seqOf(repVal), (int) LY::lenOf(repKey, repVal, repSlot, geom), (int) repPos0, firstRun ? false : ((repKey & BIT63) == 0),
                        LY::seqOf(v), (int) LY::lenOf(key, v, slot, geom), (int) LY::posOf(key, v, slot, geom), (key & BIT63) == 0);
}

template <typename LY>
__global__ __launch_bounds__(256) void k_groups(GroupArgs<LY> a, unsigned long long *__restrict__ startIo /* in: run start, out: packed key */) {
    const uint64_t i = a.first + (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long gk = ~0ull;
    if (i < a.n) {
        const uint64_t key = a.keys[i];
        if (key != ~0ull) {                                        // (an unused slot has no group key)
            const uint64_t st = startIo[i];
            const uint64_t km = LY::kmerOf(key, i, a.geom);
            const bool hasNext = (i + 1 < a.n) && a.keys[i + 1] != ~0ull && LY::kmerOf(a.keys[i + 1], i + 1, a.geom) == km;
            if (st != i || hasNext) {                              // singletons are dropped (:479)
                uint64_t bestKey = a.keys[st]; const typename LY::V best = a.vals[st];
                const uint32_t repId = LY::seqOf(best);
                uint32_t bestPos = LY::posOf(bestKey, best, st, a.geom);
                // same sequence twice in the run: the smaller position wins (rare)
                for (uint64_t e = st + 1; e < a.n && a.keys[e] != ~0ull && LY::kmerOf(a.keys[e], e, a.geom) == km && LY::seqOf(a.vals[e]) == repId; e++) {
                    const uint32_t pe = LY::posOf(a.keys[e], a.vals[e], e, a.geom);
                    if (pe < bestPos) { bestPos = pe; bestKey = a.keys[e]; }
                }
                gk = groupKeyOf<LY>(a, a.geom, bestKey, best, st, bestPos, st == a.firstRunIdx, key, a.vals[i], i);
                if (a.wide && st == i) gk = markRunStart(a, gk, repId);
            }
        }
        startIo[i] = gk;
    }
    waveGroupStats(a.stat, (uint32_t) __popcll(__ballot(runsort::gkKept(gk))));
}

// K2b + K3 fused for region 1 when only the top bits of the k-mer went through the global radix passes (bucket.h): a wave
// sorts a group of buckets on the remaining low bits in registers, finds the k-mer runs in the sorted order and writes the
// group keys of the members straight to their final slots.  W = word of the network: (bucket ordinal, low bits, position).
// LayoutSlot: where the slots of a grouping block lie in their head-digit segment - the head digit of the block's first slot and how far
// the segment reaches to either side of it, in slots relative to that first slot (clipped to 2^30; one 16-byte load per block: looking
// the digit up in the segment table is nine dependent loads, which every wave of this latency-bound kernel paid at its start)
struct BlockHead { int32_t lo, hi; uint32_t td, pad; };
#ifndef CDM_REC_CAP
#define CDM_REC_CAP 32
#endif
constexpr int REC_CAP = CDM_REC_CAP;     // staged run records per wave of the grouping kernel (its owned slots hold ~8 k-mer runs per 128 at 20x coverage)
static_assert(REC_CAP <= 64, "a wave writes its stage out with one lane per record");
__global__ void k_block_heads(TupleGeom geom, uint64_t n, uint64_t perBlock, uint64_t blocks, BlockHead *__restrict__ out) {
    const uint64_t b = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= blocks) return;
    const uint64_t base = b * perBlock;
    const uint32_t td = headDigit(geom, base);
    const uint64_t since = base - geom.seg[td], until = geom.seg[td + 1] - base;
    BlockHead h; h.td = td; h.pad = 0; h.lo = -(int32_t) min(since, (uint64_t) 1 << 30); h.hi = (int32_t) min(until, (uint64_t) 1 << 30);
    out[b] = h;
}
// The staged run records of REC_WAVES consecutive waves of the grouping kernel, packed: off = exclusive sums of the waves' counts.
// The buckets the grouping kernel left to the caller have records of their own (bigVal: sorted by start, nBig of them) - a packed record
// moves back by the number of those that start in front of it, so that the two lists interleave in k-mer order (k_rec_place_big puts
// the others in).
constexpr int REC_WAVES = 256, REC_BIG_LDS = 256;
struct RecCount { const uint8_t *c; __device__ __forceinline__ unsigned long long operator()(size_t i) const { return c[i]; } };
__device__ __forceinline__ uint64_t lowerBoundStart(const uint64_t *__restrict__ val, uint64_t n, uint64_t start) {      // first record whose start is >= start
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if ((val[mid] >> runsort::RUN_CNT_BITS) < start) lo = mid + 1; else hi = mid; }
    return lo;
}
__global__ __launch_bounds__(256) void k_rec_compact(const uint32_t *__restrict__ stRep, const uint64_t *__restrict__ stVal, const unsigned long long *__restrict__ off, uint64_t waves,
                                                     uint64_t own, const uint64_t *__restrict__ bigVal, uint64_t nBig, uint32_t *__restrict__ recRep, uint64_t *__restrict__ recVal) {
    __shared__ unsigned long long sOff[REC_WAVES + 1];
    __shared__ uint64_t sBig[REC_BIG_LDS];
    __shared__ uint64_t sB[2];
    const uint64_t w0 = (uint64_t) blockIdx.x * REC_WAVES;
    const int nw = (int) min((uint64_t) REC_WAVES, waves - w0);
    for (int i = threadIdx.x; i <= nw; i += 256) sOff[i] = off[w0 + i];
    if (threadIdx.x < 2) sB[threadIdx.x] = nBig ? lowerBoundStart(bigVal, nBig, (w0 + (threadIdx.x ? (uint64_t) nw : 0ull)) * own) : 0ull;      // the big records inside this block's slots
    __syncthreads();
    const uint64_t b0 = sB[0], nb = sB[1] - sB[0];
    for (uint64_t i = threadIdx.x; i < nb && i < (uint64_t) REC_BIG_LDS; i += 256) sBig[i] = bigVal[b0 + i] >> runsort::RUN_CNT_BITS;
    __syncthreads();
    const unsigned long long base = sOff[0], total = sOff[nw] - base;
    for (unsigned long long i = threadIdx.x; i < total; i += 256) {
        int w = 0;
#pragma unroll
        for (int st = REC_WAVES / 2; st > 0; st >>= 1) if (w + st < nw && sOff[w + st] - base <= i) w += st;
        const uint64_t src = (w0 + (uint64_t) w) * REC_CAP + (i - (sOff[w] - base));
        const uint64_t v = stVal[src], start = v >> runsort::RUN_CNT_BITS;
        uint64_t before = b0;
        if (nb <= (uint64_t) REC_BIG_LDS) { for (uint64_t q = 0; q < nb; q++) before += sBig[q] < start; }
        else before = lowerBoundStart(bigVal, nBig, start);
        recRep[base + i + before] = stRep[src]; recVal[base + i + before] = v;
    }
}
// big record b goes behind the packed records that start in front of it: those of the waves in front of the wave that owns its first
// slot, and that wave's own ones with a smaller start
__global__ __launch_bounds__(256) void k_rec_place_big(const uint32_t *__restrict__ bigRep, const uint64_t *__restrict__ bigVal, uint64_t nBig, const uint64_t *__restrict__ stVal,
                                                       const uint8_t *__restrict__ stCnt, const unsigned long long *__restrict__ off, uint64_t own, uint32_t *__restrict__ recRep, uint64_t *__restrict__ recVal) {
    const uint64_t b = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nBig) return;
    const uint64_t v = bigVal[b], start = v >> runsort::RUN_CNT_BITS, w = start / own;
    uint64_t before = off[w];
    const int c = stCnt[w];
    for (int j = 0; j < c; j++) before += (stVal[w * REC_CAP + j] >> runsort::RUN_CNT_BITS) < start;
    recRep[b + before] = bigRep[b]; recVal[b + before] = v;
}
// the group keys of the big buckets (dense staging array, ranges = (start, end, offset)) with one dropped key behind every range: run
// records made from that array (k_run_records) never span two buckets
__global__ __launch_bounds__(256) void k_big_gap_copy(const unsigned long long *__restrict__ ranges, unsigned int cnt, const unsigned long long *__restrict__ dense, unsigned long long *__restrict__ gapped) {
    const unsigned int lane = threadIdx.x & 63, wavesPerGrid = gridDim.x * 4;
    for (unsigned int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < cnt; r += wavesPerGrid) {
        const unsigned long long len = ranges[3 * (size_t) r + 1] - ranges[3 * (size_t) r], o = ranges[3 * (size_t) r + 2];
        for (unsigned long long i = lane; i < len; i += 64) gapped[o + r + i] = dense[o + i];
        if (lane == 0) gapped[o + r + len] = ~0ull;
    }
}
// their records' starts from the gapped array's coordinates to slots of the key array
__global__ __launch_bounds__(256) void k_big_rec_starts(const unsigned long long *__restrict__ ranges, unsigned int cnt, uint64_t *__restrict__ recVal, uint64_t nRec) {
    const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nRec) return;
    const uint64_t v = recVal[j], x = v >> runsort::RUN_CNT_BITS;
    unsigned int lo = 0, hi = cnt;                          // last range r with offset + r <= x
    while (hi - lo > 1) { const unsigned int mid = lo + ((hi - lo) >> 1); if (ranges[3 * (size_t) mid + 2] + mid <= x) lo = mid; else hi = mid; }
    const uint64_t slot = ranges[3 * (size_t) lo] + (x - (ranges[3 * (size_t) lo + 2] + lo));
    recVal[j] = (slot << runsort::RUN_CNT_BITS) | (v & ((1ull << runsort::RUN_CNT_BITS) - 1ull));
}
template <typename LY, typename W>
struct BucketGroupArgs : GroupParams {
    const BlockHead *blockHead = nullptr;
    // Run records of sort 2 (runsort.h), emitted while the group keys are written: every wave stages the records of the k-mer runs it
    // finishes - (representative, first slot << 13 | kept keys) per stretch of kept keys - in its own REC_CAP entries (k_rec_compact packs
    // them: the waves in order are the k-mer order).  NULL: not staged.
    uint32_t *recRep = nullptr; uint64_t *recVal = nullptr; uint8_t *recCnt = nullptr;
    uint32_t recLimit = REC_CAP;        // (CDM_REC_LIMIT lowers it: tests reach the overflow list)
    // what a wave's stage does not hold goes to a global list (a cursor, ovCap entries; in arrival order - the caller sorts it by start and
    // merges it like the big buckets' records); only a list that is too small sends the caller back to k_run_records
    uint32_t *ovRep = nullptr; uint64_t *ovVal = nullptr; unsigned long long *ovCursor = nullptr; unsigned long long ovCap = 0;
    const uint64_t *keys; const typename LY::V *vals; TupleGeom geom;
    unsigned long long *out;        // group key (or ~0) per slot, in k-mer order
    int lowBits;                    // k-mer bits the global passes left unsorted
    int own; uint32_t maxBucket; bucket::BigList big;
};
// Geometry of the grouping kernel: a smaller window than bucket.h's default - the kernel runs on the latency of its loads and LDS
// round trips (its time scales with 1 / waves per CU), so the LDS a wave needs decides its speed; k-mer buckets are ~40 tuples.
#ifndef CDM_GK_OWN
#define CDM_GK_OWN 128
#define CDM_GK_WIN 384
#define CDM_GK_FIRST 256
#endif
// With slot tuples (8 bytes per window slot, no value array) twice the owned range costs the LDS the (key, value) window did: 256 owned
// slots in a window of 512 take the kernel from 59 to 53 ms at 50 M reads (384 / 640, 512 / 768 and a 768-slot window for buckets of
// up to 512 all lose: 64-66 ms; profiles/r05_probe_grouping_geometry.txt).  Round 9 (profiles/slot_split_geometry.txt): with 27 k-mer
// bits sorted globally a bucket spans half the k-mers, but a window for buckets of up to 128 (256 / 384 / 320, 8 blocks per CU) sends 88 M
// tuples of the bench's 4.05 G to the caller's list where this one sends 10 thousand - buckets are sums of whole k-mer runs, their tail
// does not halve - and groups of up to 128 cost more than they save (50.7 against 45.4 ms): geometry and group capacity stay.
#ifndef CDM_GKS_OWN
#define CDM_GKS_OWN 256
#define CDM_GKS_WIN 512
#define CDM_GKS_FIRST 384
#endif
#ifndef CDM_GKS_GROUP
#define CDM_GKS_GROUP 256     // largest group of several buckets of the slot instance (a single bucket: up to WIN - OWN)
#endif
template <typename LY> struct GkGeom {
    static constexpr int OWN = LY::bySlot ? CDM_GKS_OWN : CDM_GK_OWN, WIN = LY::bySlot ? CDM_GKS_WIN : CDM_GK_WIN, FIRST = LY::bySlot ? CDM_GKS_FIRST : CDM_GK_FIRST, MAXB = WIN - OWN;
    // GROUP: the capacity of a group of several buckets (bucket::waveBuckets; at most a bucket's); CAP: the most elements one network
    // sorts = the words of sSAll (the network writes all 64 R slots of it, R = CAP / 64 at the most).  The slot instance is built with
    // that largest R; the (key, value) layouts' instances are left as they were, all four networks (their R = 8 is as unreachable).
    static constexpr int GROUP = LY::bySlot ? CDM_GKS_GROUP : bucket::BK_GROUP, CAP = MAXB, MAXR = LY::bySlot ? CAP / 64 : 8;
    static_assert(WIN % 64 == 0 && FIRST % 64 == 0 && FIRST <= WIN && OWN <= FIRST && WIN <= (1 << bucket::WV_IDX) && (MAXB == 64 || MAXB == 128 || MAXB == 256 || MAXB == 512), "grouping kernel geometry");
    static_assert(GROUP >= 64 && GROUP <= MAXB && GROUP <= (1 << bucket::BK_ORD), "grouping kernel group capacity");
};
#ifndef CDM_GK_MINW
#define CDM_GK_MINW 0      // waves per SIMD the register allocation of the grouping kernel leaves room for (scripts/build_variant.py sweeps it; 0: 6 with slot tuples - the 6 blocks of 4 waves per CU its LDS lets run -, no request with (key, value) pairs in the window)
#endif
// LDS the kernel declares per block (a block of BK_NT threads is one wave per SIMD: blocks per CU = waves per SIMD)
template <typename LY> constexpr size_t gkLdsBytes() {
    return (size_t) bucket::BK_WAVES * ((size_t) GkGeom<LY>::WIN * 8 + (LY::bySlot ? 1 : (size_t) GkGeom<LY>::WIN) * sizeof(typename LY::V) + (size_t) GkGeom<LY>::CAP * 4 + sizeof(bucket::WaveLdsT<GkGeom<LY>::WIN>) +
                                      (LY::bySlot ? (size_t) REC_CAP : 1) * 12);
}
// A request the LDS cannot meet is not approximated by the compiler but dropped ("failed to meet occupancy target"): the slot instance
// asked for 7 with 26 KB of LDS per block, got an uncapped allocation of 83 registers and ran at 5.  Hence the assert next to the bound
// (a sweep's CDM_GK_MINW reaches the other layouts' instances as far as their LDS goes).
template <typename LY> constexpr int gkMinWaves() {
    return LY::bySlot ? (CDM_GK_MINW ? CDM_GK_MINW : 6) : (CDM_GK_MINW ? (int) std::min<size_t>(CDM_GK_MINW, CU_LDS_BYTES / gkLdsBytes<LY>()) : 1);
}
template <typename LY, typename W>
__global__ __launch_bounds__(bucket::BK_NT, gkMinWaves<LY>()) void k_bucket_groups(BucketGroupArgs<LY, W> a) {
    static_assert(bucket::BK_NT == 256 && (size_t) gkMinWaves<LY>() * gkLdsBytes<LY>() <= CU_LDS_BYTES, "the launch bound asks for more blocks per CU than the kernel's LDS lets run: the compiler would drop the request");
    using namespace bucket;
    typedef typename LY::V V;
    constexpr int GK_WIN = GkGeom<LY>::WIN, GK_FIRST = GkGeom<LY>::FIRST, GK_CAP = GkGeom<LY>::CAP;
    __shared__ uint64_t sKeyAll[BK_WAVES][GK_WIN];
    __shared__ V sValAll[BK_WAVES][LY::bySlot ? 1 : GK_WIN];       // (slot tuples: no value array)
    __shared__ uint32_t sSAll[BK_WAVES][GK_CAP];
    static_assert(GK_CAP >= 64 * GkGeom<LY>::MAXR || !LY::bySlot, "the largest network of the instance writes 64 R words of sSAll");
    __shared__ WaveLdsT<GK_WIN> wAll[BK_WAVES];
    // (slot instance: the wave's number as a scalar - r0 and every address made of it, a.keys + r0, a.out + r0, stay out of the vector unit)
    const int lane = threadIdx.x & 63, wave = LY::bySlot ? __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6)) : (int) (threadIdx.x >> 6);
    const uint64_t r0 = ((uint64_t) blockIdx.x * BK_WAVES + wave) * (uint64_t) a.own;
    if (r0 >= a.n) return;      // (whole wave)
    uint64_t *sKey = sKeyAll[wave]; V *sVal = sValAll[wave]; uint32_t *ss = sSAll[wave];
    WaveLdsT<GK_WIN> &w = wAll[wave];
    const uint64_t hmask = (2ull << a.geom.kbits) - 1ull, lowMask = (1ull << a.lowBits) - 1ull;   // k-mer bits + the unused-slot bit
    const int lowBits = a.lowBits;
    struct Tup { uint64_t k; V v; };
    constexpr uint32_t IDXM = (1u << WV_IDX) - 1u;
    uint32_t keptCnt = 0;       // wave-uniform
    uint32_t recCount = 0, prevRowKept = 0;      // (lane 0's copies are complete) run records staged so far; was the last key of the row in front kept
    // (staged in LDS, written out in one piece at the wave's end)
    // Only the slot layout's instance stages records: with (key, value) pairs in the window the stage's LDS and registers take the kernel
    // from six blocks per CU to five (63 instead of 49 ms), more than k_run_records' pass over the keys costs.
    constexpr bool REC = LY::bySlot;
    __shared__ uint32_t sRecRep[BK_WAVES][REC ? REC_CAP : 1];
    __shared__ uint64_t sRecVal[BK_WAVES][REC ? REC_CAP : 1];
    const uint32_t recLimit = a.recLimit;
    // the array's first run as a slot of this wave's window (no slot of it: the run starts elsewhere) - one 32-bit compare per member
    const uint32_t firstRel = a.firstRunIdx - r0 < (uint64_t) GK_WIN ? (uint32_t) (a.firstRunIdx - r0) : ~0u;
    unsigned long long *const outW = a.out + r0;
    const uint64_t waveIdx = (uint64_t) blockIdx.x * BK_WAVES + wave;
    // slot tuples (LayoutSlot): a tuple becomes its (key, id) pair as it is loaded; the head digit is the segment the index lies in -
    // the wave's own one for nearly every tuple of its window (segments are millions of tuples long)
    BlockHead bh; bh.lo = 0; bh.hi = 0; bh.td = 0; bh.pad = 0;
    const uint64_t blockBase = (uint64_t) blockIdx.x * BK_WAVES * (uint64_t) a.own;
    if constexpr (LY::bySlot) bh = a.blockHead[blockIdx.x];
    auto digitAt = [&](uint64_t g) -> uint32_t { const long long off = (long long) (g - blockBase); return (off >= (long long) bh.lo && off < (long long) bh.hi) ? bh.td : headDigit(a.geom, g); };
    waveBuckets<Tup, GK_WIN, GK_FIRST, GkGeom<LY>::GROUP>(r0, a.n, a.own, a.maxBucket, hmask & ~lowMask, a.big, w, lane,
        [&](uint64_t g) {
            Tup t;
            if constexpr (LY::bySlot) { t.k = a.keys[g]; t.v = digitAt(g); }       // (raw: the window holds far more tuples than the wave owns)
            else { t.k = a.keys[g]; t.v = a.vals[g]; }
            return t;
        },
        [&](int i, const Tup &t) {
            sKey[i] = t.k;
            if constexpr (LY::bySlot) return ((uint64_t) t.v << a.geom.headShift) | (t.k >> rx::SLOT_KEY_SHIFT);       // what buckets are told apart by: the k-mer
            else { sVal[i] = t.v; return t.k; }
        },
        [&](uint64_t g) {
            if constexpr (LY::bySlot) return ((uint64_t) digitAt(g) << a.geom.headShift) | (a.keys[g] >> rx::SLOT_KEY_SHIFT);
            else return a.keys[g];
        },
        [&](int g0, int gm) {

            // word of the network: (bucket ordinal within the group, low k-mer bits, position within the group)
            const int idxBits = (GK_CAP > 256 && gm > 256) ? 9 : 8, ord0 = w.ord[g0];
            sortGroup<W, GkGeom<LY>::MAXR>(gm, lane,
                [&](int i) {
                    const uint64_t low = LY::bySlot ? (uint64_t) ((uint32_t) (sKey[g0 + i] >> rx::SLOT_KEY_SHIFT)) & lowMask : sKey[g0 + i] & lowMask;      // (a slot tuple's k-mer bits sit above its index)
                    return (W) ((((W) (w.ord[g0 + i] - ord0) << lowBits | (W) low) << idxBits) | (W) i);
                },
                [&](auto &v) {
                    // per sorted position: window slot of the element, start of its run (= equal bucket and low bits; from an
                    // inclusive max-scan of the start positions over the wave) and whether it starts one
                    constexpr int R = sizeof(v) / sizeof(v[0]);
                    const W prevLast = shflUpW<W>(v[R - 1], 1);
                    int st[R], last = -1;
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        const int p = lane * R + r;
                        const W prev = r ? v[r - 1] : prevLast;
                        if (p == 0 || (v[r] >> idxBits) != (prev >> idxBits)) last = p;
                        st[r] = last;
                    }
                    int sc = last;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(sc, d, 64); if (lane >= d) sc = max(sc, o); }
                    const int carry = __shfl_up(sc, 1, 64);
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        const int p = lane * R + r, s0 = st[r] < 0 ? carry : st[r];
                        ss[p] = (uint32_t) (g0 + (int) ((uint32_t) v[r] & ((1u << idxBits) - 1u))) | ((uint32_t) s0 << WV_IDX) | (s0 == p ? 1u << 31 : 0u);
                    }
                });
            waveLdsSync();
            // one copy of the member code in the instruction stream, whatever the size of the network before it
#pragma unroll 1
            for (int p = lane; p < gm; p += 64) {
                const uint32_t cw = ss[p];
                const int s0 = (int) ((cw >> WV_IDX) & 1023u), e = (int) (cw & IDXM), p0row = p - lane;
                unsigned long long gk = ~0ull;
                uint32_t recRepOfLane = 0;      // the run's representative (kept members only read it)
                const bool hasNext = (p + 1 < gm) && !(ss[p + 1] >> 31);
                if constexpr (LY::bySlot) {
                if (s0 != p || hasNext) {
                    // slot tuples: sequence, position and strand come straight out of the slot index (the k-mer itself is of no interest
                    // behind the sort; every sequence has the one length)
                    const int er = (int) (ss[s0] & IDXM);
                    uint32_t repId, bestPos, id, tPos, repR; bool repFwd, fwd;
                    const uint64_t repT = sKey[er];
                    slotFields(a.geom, repT, repId, bestPos, repFwd, repR);
                    // Same sequence twice in the run: inside a k-mer run the sorted order is the slot order (stable passes, the index is
                    // part of the word), and a sequence's slots are consecutive - the representative's sequence has another tuple in the
                    // run exactly when the NEXT tuple's slot (there is one: the run has two tuples or more here) lies in front of that
                    // sequence's last slot.  A subtract and a compare per lane; the scan behind it decodes tuples and is rare
                    const uint32_t nextSlot = (uint32_t) sKey[(int) (ss[s0 + 1] & IDXM)];
                    if (nextSlot - (uint32_t) repT < a.geom.uniS - repR) {
                        for (int t = s0 + 1; t < gm && !(ss[t] >> 31); t++) {
                            uint32_t ie, pe; bool fe;
                            slotFields(a.geom, sKey[(int) (ss[t] & IDXM)], ie, pe, fe);
                            if (ie != repId) break;
                            if (pe < bestPos) { bestPos = pe; repFwd = fe; }
                        }
                    }
                    slotFields(a.geom, sKey[e], id, tPos, fwd);
                    const bool firstRun = (uint32_t) (g0 + s0) == firstRel;
                    gk = groupKeyCore(a, repId, (int) a.geom.uniL, (int) bestPos, firstRun ? false : !repFwd, id, (int) a.geom.uniL, (int) tPos, !fwd);
                    if (a.wide && s0 == p) gk = markRunStart(a, gk, repId);
                    recRepOfLane = repId;
                }
                } else
                if (s0 != p || hasNext) {       // the staged range holds real tuples only (the unused slots sorted behind it)
                    const int er = (int) (ss[s0] & IDXM);
                    uint64_t bestKey = sKey[er]; const V best = sVal[er];
                    const uint32_t repId = LY::seqOf(best);
                    uint32_t repLen, bestPos;
                    LY::unpackR1(bestKey, best, a.geom, repLen, bestPos);
                    for (int t = s0 + 1; t < gm && !(ss[t] >> 31); t++) {     // same sequence twice in the run (rare)
                        const int et = (int) (ss[t] & IDXM);
                        if (LY::seqOf(sVal[et]) != repId) break;
                        uint32_t le, pe;
                        LY::unpackR1(sKey[et], sVal[et], a.geom, le, pe);
                        if (pe < bestPos) { bestPos = pe; bestKey = sKey[et]; }
                    }
                    const uint64_t key = sKey[e]; const V val = sVal[e];
                    uint32_t tLen, tPos;
                    LY::unpackR1(key, val, a.geom, tLen, tPos);
                    const bool firstRun = r0 + (uint64_t) (g0 + s0) == a.firstRunIdx;
                    gk = groupKeyCore(a, repId, (int) repLen, (int) bestPos, firstRun ? false : ((bestKey & BIT63) == 0), LY::seqOf(val), (int) tLen, (int) tPos, (key & BIT63) == 0);
                    if (a.wide && s0 == p) gk = markRunStart(a, gk, repId);
                    recRepOfLane = repId;
                }
                if constexpr (LY::bySlot) outW[(uint32_t) (g0 + p)] = gk;       // (scalar base, 32-bit lane part)
                else a.out[r0 + (uint64_t) (g0 + p)] = gk;
                const unsigned long long keptMask = __ballot(runsort::gkKept(gk));
                keptCnt += (uint32_t) __popcll(keptMask);
                if constexpr (REC) if (a.recRep) {
                    // records of this row of 64 sorted positions: a record begins at a kept key that starts a k-mer run or follows a key that
                    // is not kept, and ends in front of the next run start / not-kept key; a stretch that runs on from the row in front
                    // (the same k-mer run: rows of one group) lengthens that row's last record instead of beginning one
                    const uint32_t recBase = (uint32_t) __builtin_amdgcn_readfirstlane((int) recCount);       // (lane 0 runs every row: its values are complete)
                    const bool lastKept = __builtin_amdgcn_readfirstlane((int) prevRowKept) != 0;
                    const unsigned long long startMask = __ballot((cw >> 31) != 0u);
                    const bool runsOn = p0row != 0 && lastKept && (keptMask & 1ull) && !(startMask & 1ull) && recBase - 1u < recLimit;      // (a record on the overflow list is not lengthened: the stretch goes on as a record of its own)
                    const unsigned long long begins = keptMask & (startMask | ~(keptMask << 1)) & ~(runsOn ? 1ull : 0ull), ends = ~keptMask | startMask;
                    if (((begins >> lane) & 1ull) || (runsOn && lane == 0)) {
                        const unsigned long long behind = lane == 63 ? 0ull : ends >> (lane + 1);
                        const uint32_t len = behind ? (uint32_t) __ffsll(behind) : (uint32_t) (64 - lane);
                        const uint32_t j = recBase + (uint32_t) __popcll(begins & ((1ull << lane) - 1ull));
                        // (a wave's LDS operations take effect in program order: the add meets the record an earlier row wrote)
                        const uint64_t rv = ((r0 + (uint64_t) (g0 + p)) << runsort::RUN_CNT_BITS) | (uint64_t) len;
                        if (runsOn && lane == 0) atomicAdd(reinterpret_cast<unsigned long long *>(&sRecVal[wave][recBase - 1u]), (unsigned long long) len);
                        else if (j < recLimit) { sRecRep[wave][j] = recRepOfLane; sRecVal[wave][j] = rv; }
                        else { const unsigned long long q = atomicAdd(a.ovCursor, 1ull); if (q < a.ovCap) { a.ovRep[q] = recRepOfLane; a.ovVal[q] = rv; } }
                    }
                    recCount = recBase + (uint32_t) __popcll(begins);
                    prevRowKept = (uint32_t) (keptMask >> 63);
                }
            }
            waveLdsSync();      // ss is reused by the next group
        });
    waveGroupStats(a.stat, keptCnt);
    recCount = (uint32_t) __builtin_amdgcn_readfirstlane((int) recCount);
    if constexpr (REC) if (a.recRep && recCount) {
        // the wave's records go out in one piece
        const uint32_t m = min(recCount, recLimit);
        waveLdsSync();
        if ((uint32_t) lane < m) { const uint64_t slot = waveIdx * (uint64_t) REC_CAP + (uint32_t) lane; a.recRep[slot] = sRecRep[wave][lane]; a.recVal[slot] = sRecVal[wave][lane]; }
        if (lane == 0) a.recCnt[waveIdx] = (uint8_t) m;
    }
}

__global__ __launch_bounds__(256) void k_reduce_stats(const unsigned long long *__restrict__ stripes, unsigned long long *__restrict__ out) {
    unsigned long long c = 0;
    for (int i = threadIdx.x; i < STAT_STRIPES; i += 256) c += stripes[i];
    c = cdm_block_sum<unsigned long long>(c);
    if (threadIdx.x == 0) out[0] = c;
}
// number of keys in front of the unused / dropped ones (key ~0) once the array is sorted on bits up to `bit`, which is set
// only in them: the first key with that bit set
__global__ void k_live_count(const uint64_t *__restrict__ keys, uint64_t n, int kbits, unsigned long long *__restrict__ out) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if ((keys[mid] >> kbits) & 1ull) hi = mid; else lo = mid + 1; }
    *out = lo;
}
// number of real tuples in region 2 (sorted on the low 63 bits; the empty slots, key ~0, are last)
__global__ void k_count_hash_tuples(const uint64_t *__restrict__ keys, uint64_t n, unsigned long long *__restrict__ out) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (keys[mid] == ~0ull) hi = mid; else lo = mid + 1; }
    *out = lo;
}
constexpr int STALE_MAX = CDM_STALE_MAX;
// The tuples the reference's last per-target scan runs into (see VoteArgs): k-mer-ordered real tuples from index J = nGroup on
// while their sequence id is `target`.  Region 1 is only sorted on its high bits in memory (unless `sorted`): the bucket that
// holds index J is ranked here (all pairs, one block); buckets larger than STALE_BUCKET were finished through the big-bucket
// path, which leaves them sorted in memory.  Region 2 is sorted.
constexpr int STALE_BUCKET = 2048;
template <typename LY>
struct StaleArgs {
    const uint64_t *keys; const typename LY::V *vals; TupleGeom geom;
    uint64_t live, kmerSlots, nTuples, J; int lowBits; bool sorted;
    uint32_t *out;      // [0] count, [1] their sequence id, [2..] positions
};
template <typename LY>
__global__ __launch_bounds__(256) void k_stale_tail(StaleArgs<LY> a) {
    __shared__ uint64_t sC[STALE_BUCKET];
    __shared__ uint64_t sB[2];
    __shared__ int sSel;
    const uint64_t hmask = (2ull << a.geom.kbits) - 1ull, lowMask = (1ull << a.lowBits) - 1ull;
    uint32_t cnt = 0, target = ~0u;
    for (uint64_t j = a.J; cnt < (uint32_t) STALE_MAX; j++) {
        uint64_t idx;
        if (j < a.live) {
            idx = j;
            if (!a.sorted) {
                if (threadIdx.x == 0) {     // bucket of j: equal high bits
                    const uint64_t h = (memSortBits<LY>(a.keys, j, a.geom) & hmask) >> a.lowBits;
                    uint64_t lo = 0, hi = j;
                    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (((memSortBits<LY>(a.keys, mid, a.geom) & hmask) >> a.lowBits) < h) lo = mid + 1; else hi = mid; }
                    sB[0] = lo;
                    lo = j; hi = a.live;
                    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (((memSortBits<LY>(a.keys, mid, a.geom) & hmask) >> a.lowBits) == h) lo = mid + 1; else hi = mid; }
                    sB[1] = lo;
                }
                __syncthreads();
                const uint64_t b0 = sB[0], b1 = sB[1];
                const int m = (int) min((uint64_t) STALE_BUCKET + 1, b1 - b0);
                if (m <= STALE_BUCKET) {
                    for (int i = threadIdx.x; i < m; i += blockDim.x) sC[i] = ((memSortBits<LY>(a.keys, b0 + i, a.geom) & lowMask) << 12) | (uint64_t) i;
                    if (threadIdx.x == 0) sSel = 0;
                    __syncthreads();
                    const int want = (int) (j - b0);
                    for (int e = threadIdx.x; e < m; e += blockDim.x) {
                        const uint64_t mine = sC[e]; int r = 0;
                        for (int f = 0; f < m; f++) r += sC[f] < mine;
                        if (r == want) sSel = e;
                    }
                    __syncthreads();
                    idx = b0 + (uint64_t) sSel;
                }
                __syncthreads();
            }
        } else {
            idx = a.kmerSlots + (j - a.live);
            if (idx >= a.nTuples) break;
        }
        if (a.keys[idx] == ~0ull) break;                           // end of the real tuples (the empty slots of region 2; region 1 is read below `live` only)
        uint64_t key; typename LY::V v;
        memPair<LY>(a.keys, a.vals, idx, a.geom, key, v);
        if (cnt == 0) target = LY::seqOf(v);                       // the scan can only run on for this sequence id
        else if (LY::seqOf(v) != target) break;
        if (threadIdx.x == 0) a.out[2 + cnt] = LY::posOf(key, v, idx, a.geom);
        cnt++;
    }
    if (threadIdx.x == 0) { a.out[0] = cnt; a.out[1] = target; }
}
// smallest index at which the two arrays differ (atomicMin; *out starts as ~0)
__global__ void k_first_diff(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b, uint64_t n, unsigned long long *__restrict__ out) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x)
        if (a[i] != b[i]) { atomicMin(out, (unsigned long long) i); return; }
}
// LayoutSlot, buckets the grouping kernel left alone: their slot tuples as (key, id) pairs in the dense staging arrays, and the sorted
// pairs back as slot tuples (a wave per listed range (start, end, offset), as bucket::k_big_copy)
template <bool GATHER>
__global__ __launch_bounds__(256) void k_big_slot_pairs(const unsigned long long *__restrict__ ranges, unsigned int cnt, uint64_t *arr, TupleGeom geom, uint64_t *denseK, uint32_t *denseV) {
    const unsigned int lane = threadIdx.x & 63, wavesPerGrid = gridDim.x * 4;
    for (unsigned int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < cnt; r += wavesPerGrid) {
        const unsigned long long s = ranges[3 * (size_t) r], e = ranges[3 * (size_t) r + 1], o = ranges[3 * (size_t) r + 2];
        const uint32_t td = headDigit(geom, s);         // (a bucket lies inside one segment)
        for (unsigned long long i = lane; i < e - s; i += 64) {
            if (GATHER) { uint64_t key; uint32_t id; slotTupleToPair(geom, arr[s + i], td, key, id); denseK[o + i] = key; denseV[o + i] = id; }
            else arr[s + i] = pairToSlotTuple(geom, denseK[o + i], denseV[o + i]);
        }
    }
}

}  // namespace
