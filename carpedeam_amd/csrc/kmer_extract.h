// kmermatcher on the device (kmermatch.hip), stage K1:
//   K1 k_seq_hash, k_extract_pair, k_extract_uniform, k_extract_fast, k_extract   fillKmerPositionArray :77-388  per sequence: canonical k-mers, XXH64 16-bit
//                     min-hash, per-sequence ordering by (hash, k-mer, pos) for the repeated-k-mer skipping and the bottom-m
//                     selection, + the whole-sequence hash tuple
// and the helper kernels that lay the sequences' slots out in front of it (KmerJob::phaseA, splitPartition).
// Quirk kept on purpose (observable in the prefilter DB): the repeated-k-mer skip that processes the element after a run
// unconditionally (:277-350).
#pragma once
#include "kmer_tuple.h"

namespace {

struct SeqPos;
template <typename LY> struct ExtractArgs {
    const uint32_t *woff, *len, *codes, *nmask;
    const uint8_t *hasN;
    const uint32_t *list;       // sequence indices this launch handles
    uint32_t nList;
    int k, kmersPerSeq; float scale; uint64_t seed; int ignoreMultiKmer;
    uint64_t *keys; typename LY::V *vals;   // tuple array
    const uint64_t *slotOff;    // [n+1] first slot of every sequence: 1 whole-sequence tuple + one slot per k-mer position;
                                // unused slots hold the key ~0 (sorts last, dropped by k_groups)
    uint32_t *slowShort, *slowLong; unsigned int *slowCnt;   // sequences the fast kernel hands to the general one
    uint32_t *single;           // sequences k_extract_pair hands to k_extract_fast (count in slowCnt[2])
    uint32_t *slowHuge;         // sequences with 4096 k-mer positions or more (count in slowCnt[3]): k_extract with global scratch
    SeqPos *hugeSp; uint8_t *hugeSel; uint32_t hugeCap;   // that scratch: hugeCap records per block
    const unsigned int *listCount;   // device-side length of `list` for k_extract_fast (NULL: all sequences)
    uint32_t n;
    // The whole-sequence hash tuple (63 random bits) lives in a second region behind the k-mer slots, [hashBase, hashBase+n),
    // at the sequence's rank in (length desc, id asc) order, unless its key happens to fit the 2k bits of a k-mer (then it
    // stays in slot 0 of the sequence).  Region 1 is sorted on 2k bits, region 2 on 63: every key of region 1 is smaller
    // than every key of region 2, so the concatenation is the array the reference sorts on the full key.
    uint64_t hashBase; const uint32_t *rankOf;
    TupleGeom geom;
    // Multi-GPU runs split the k-mer space into ranges (the reference's MPI split, kmermatcher.cpp:634-663, by value instead of
    // by hash so that the ranges are in k-mer order): only tuples with kLo <= key < kHi are stored, the others leave their slot
    // empty; the whole-sequence hash tuples of region 2 belong to the last range.  belowFlag is set when a real tuple lies
    // below the range (the array's very first run is then not in it).  Single-GPU: kLo = 0, kHi = ~0, lastPart = 1.
    uint64_t kLo, kHi; int lastPart; unsigned int *belowFlag;
    // The other split of a multi-GPU run (round 4, cdm_kmermatch_split_*): a rank extracts the k-mers of ITS sequences only - the
    // sequences with order ranks [ordLo, ordHi) in the (length desc, id asc) slot order, all k-mer values - and the tuples then travel
    // to the owner of their k-mer range.  ordHi = 0: every sequence (one device, and the k-mer-range split above).
    uint32_t ordLo = 0, ordHi = 0;
    uint32_t uniS = 0;          // LayoutSlot: every sequence has uniS slots, sequence i the slots from i x uniS on, rank i (slotOff / rankOf are not built)
    // LayoutSlot: the extraction kernels count the head digits (k-mer bits from headShift on) of the tuples they leave in the slots -
    // the histogram of sort 1's head pass, which then needs no read of the keys of its own (NULL: not counted)
    unsigned long long *headHist = nullptr; int headShift = 0;
};
constexpr int HEAD_BINS = rx::BINS;
// a block's head digit counters: cleared at the start of an extraction kernel, added to the global ones at its end
__device__ __forceinline__ void headHistClear(unsigned int *sHead) { for (int i = threadIdx.x; i < HEAD_BINS; i += blockDim.x) sHead[i] = 0u; __syncthreads(); }
__device__ __forceinline__ void headHistFlush(const unsigned int *sHead, unsigned long long *hist) {
    __syncthreads();
    for (int i = threadIdx.x; i < HEAD_BINS; i += blockDim.x) { const unsigned int c = sHead[i]; if (c) atomicAdd(&hist[i], (unsigned long long) c); }
}
template <typename LY> __device__ __forceinline__ uint64_t slotBase(const ExtractArgs<LY> &a, uint32_t seq) { if constexpr (LY::bySlot) return (uint64_t) seq * a.uniS; else return a.slotOff[seq]; }
template <typename LY> __device__ __forceinline__ uint32_t seqRank(const ExtractArgs<LY> &a, uint32_t seq) { if constexpr (LY::bySlot) return seq; else return a.rankOf[seq]; }
template <typename LY> __device__ __forceinline__ bool ownedSeq(const ExtractArgs<LY> &a, uint32_t seq) {
    if (a.ordHi == 0) return true;
    const uint32_t r = a.rankOf[seq];
    return r >= a.ordLo && r < a.ordHi;
}
template <typename LY> __device__ __forceinline__ bool inRange(const ExtractArgs<LY> &a, uint64_t km) { return km >= a.kLo && km < a.kHi; }
template <typename LY> __device__ __forceinline__ void noteBelow(const ExtractArgs<LY> &a, bool below) {       // whole wave
    if (__ballot(below) != 0ull && (threadIdx.x & 63) == 0 && a.belowFlag[0] == 0u) a.belowFlag[0] = 1u;
}
template <typename LY>
__device__ __forceinline__ void putSeqHashTuple(const ExtractArgs<LY> &a, uint32_t seq, uint32_t L, uint64_t base, uint64_t h) {
    const uint64_t key = xxh64_u64(h, a.seed);
    const uint64_t hslot = a.hashBase + (seqRank(a, seq) - a.ordLo);
    const bool small = (key & ~BIT63) < (1ull << (2 * a.k));
    if (small) {
        if (inRange(a, key & ~BIT63)) LY::storeHash(a.keys, a.vals, base, key, seq, L, a.geom); else LY::storeEmpty(a.keys, a.vals, base);
        if constexpr (LY::bySlot) { if (a.headHist && inRange(a, key & ~BIT63)) atomicAdd(&a.headHist[(key & ~BIT63) >> a.headShift], 1ull); }      // (one sequence in 2^(63 - 2k))
        if ((key & ~BIT63) < a.kLo && a.belowFlag[0] == 0u) a.belowFlag[0] = 1u;
        LY::storeEmpty(a.keys, a.vals, hslot);
    } else {
        LY::storeEmpty(a.keys, a.vals, base);
        if (a.lastPart) LY::storeHash(a.keys, a.vals, hslot, key, seq, L, a.geom); else LY::storeEmpty(a.keys, a.vals, hslot);
    }
}

// 2k-bit window of the sequence starting at base pos, MMseqs2 coding (A,C,T,G), first base in the LOW bits
__device__ __forceinline__ uint64_t kmerWindow(const uint32_t *__restrict__ codes, uint32_t w0, uint32_t pos, uint32_t lastWord, int k) {
    const uint32_t w = pos >> 4, sh = (pos & 15u) * 2u;
    const uint64_t a = codes[w0 + w];
    const uint64_t b = (w + 1 <= lastWord) ? codes[w0 + w + 1] : 0u;
    const uint64_t c = (w + 2 <= lastWord) ? codes[w0 + w + 2] : 0u;
    uint64_t x = (a | (b << 32)) >> sh;
    if (sh) x |= c << (64 - sh);
    x ^= (x >> 1) & 0x5555555555555555ull;                     // A,C,G,T -> A,C,T,G
    return x;                                                   // 32 bases from pos on; callers mask what they need
}
// Indexer::computeKmerIdx order (first base most significant) from the window: reverse the 2-bit groups
__device__ __forceinline__ uint64_t groupsReversed(uint64_t x, int k) {
    x = ((x >> 2) & 0x3333333333333333ULL) | ((x & 0x3333333333333333ULL) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0FULL) | ((x & 0x0F0F0F0F0F0F0F0FULL) << 4);
    x = __builtin_bswap64(x);
    return x >> (64 - 2 * k);
}
// The whole-sequence tuple of every sequence (kmermatcher.cpp:244-267): Util::hash over the numeric sequence
// (M/commons/Util.h:338-346, h = h * 31 + c) then XXH64 (:135-138).  One thread per sequence: a serial Horner walk over packed
// words costs a wave a few instructions per sequence, where the wave-per-sequence extraction kernels spent hundreds on it.
template <typename LY>
__global__ __launch_bounds__(256) void k_seq_hash(ExtractArgs<LY> a) {
    const uint32_t seq = blockIdx.x * blockDim.x + threadIdx.x;
    if (seq >= a.n || !ownedSeq(a, seq)) return;
    const uint32_t L = a.len[seq], w0 = a.woff[seq];
    uint64_t h = 0;
    if (a.hasN[seq]) {
        for (uint32_t i = 0; i < L; i++) {
            uint32_t c = cdm_base(a.codes, w0, i); c ^= c >> 1;
            if (cdm_isN(a.nmask, w0, i)) c = 4;
            h = h * 31 + c;
        }
    } else {
        for (uint32_t i = 0; i < L; i += 16) {
            uint32_t word = a.codes[w0 + (i >> 4)];
            const uint32_t nb = min(16u, L - i);
            for (uint32_t j = 0; j < nb; j++) { uint32_t c = word & 3u; c ^= c >> 1; h = h * 31 + c; word >>= 2; }
        }
    }
    putSeqHashTuple(a, seq, L, slotBase(a, seq), h);
}

constexpr int FAST_WAVES = 4, FAST_TABLE = 1024, FAST_CAP = 448;
// Fast path of K1: one wavefront per sequence, no per-sequence sort.  Valid when every k-mer is taken
// (positions <= kmersPerSeq - 1 + scale * L) and no canonical k-mer occurs twice in the sequence (checked with an LDS
// hash set); then the selection is "all k-mers" whatever the (hash, k-mer, pos) order.  Anything else goes to k_extract.
template <typename LY>
__global__ __launch_bounds__(64 * FAST_WAVES) void k_extract_fast(ExtractArgs<LY> a) {
    __shared__ unsigned long long sTable[FAST_WAVES][FAST_TABLE];
    __shared__ unsigned int sHead[LY::bySlot ? HEAD_BINS : 1];
    const bool countHead = LY::bySlot && a.headHist != nullptr;
    if (countHead) headHistClear(sHead);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long *table = sTable[wave];
    const int k = a.k;
    const uint32_t nItems = a.listCount ? *a.listCount : a.n;
    for (uint32_t item = blockIdx.x * FAST_WAVES + wave; item < nItems; item += gridDim.x * FAST_WAVES) {
        const uint32_t seq = a.listCount ? a.list[item] : item;
        if (!a.listCount && !ownedSeq(a, seq)) continue;          // (wave-uniform)
        const uint32_t L = a.len[seq], w0 = a.woff[seq];
        const bool hasN = a.hasN[seq] != 0;
        const uint32_t nPos = (L >= (uint32_t) k) ? (L - k + 1) : 0;
        const uint64_t base = slotBase(a, seq);
        const size_t cap = (size_t) (float) ((float) (a.kmersPerSeq - 1) + (a.scale * (float) L));
        if (nPos > cap || nPos > FAST_CAP) {   // wave uniform
            if (lane == 0) {
                if (nPos < 256) a.slowShort[atomicAdd(&a.slowCnt[0], 1u)] = seq;
                else if (nPos < 4096) a.slowLong[atomicAdd(&a.slowCnt[1], 1u)] = seq;
                else a.slowHuge[atomicAdd(&a.slowCnt[3], 1u)] = seq;
            }
            continue;
        }
        // hash set sized to the sequence (load factor <= 1/2): clearing it is a large share of this kernel's LDS traffic
        uint32_t tsize = 64; while (tsize < 2 * nPos) tsize <<= 1;
        const uint32_t tmask = tsize - 1;
        for (uint32_t i = lane; i < tsize; i += 64) table[i] = ~0ull;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier();
        const uint32_t lastWord = (L + 15) / 16 - 1;
        bool dup = false, below = false;
        const uint64_t kmask = (1ull << (2 * k)) - 1ull;
        // canonical k-mer of the window w (idx = the same k-mer in Indexer order) at position pos: insert, store
        auto emit = [&](uint64_t w, uint64_t idx, uint32_t pos, bool x) {
            const uint64_t rc = (w ^ 0xAAAAAAAAAAAAAAAAull) & kmask;     // Util::revComplement(idx): window order, complemented
            if (!x && rc != idx) {
                const bool pickRev = rc < idx;
                const uint64_t km = pickRev ? rc : idx;
                const uint32_t p = pickRev ? (L - pos - k) : pos;
                if (a.ignoreMultiKmer) {
                    uint32_t h = (uint32_t) ((km * 0x9E3779B97F4A7C15ull) >> 40) & tmask;
                    while (true) {
                        const unsigned long long old = atomicCAS(&table[h], ~0ull, (unsigned long long) km);
                        if (old == ~0ull) break;
                        if (old == km) { dup = true; break; }
                        h = (h + 1) & tmask;
                    }
                }
                below |= km < a.kLo;
                if (inRange(a, km)) LY::store(a.keys, a.vals, base + 1 + pos, km, !pickRev, seq, L, p, a.geom); else LY::storeEmpty(a.keys, a.vals, base + 1 + pos);
                if (countHead && !a.ignoreMultiKmer && inRange(a, km)) atomicAdd(&sHead[km >> a.headShift], 1u);      // (no repeated-k-mer rule: what is stored stays)
            } else LY::storeEmpty(a.keys, a.vals, base + 1 + pos);
        };
        if (hasN) {
            for (uint32_t pos = lane; pos < nPos; pos += 64) {
                const uint64_t w = kmerWindow(a.codes, w0, pos, lastWord, k) & kmask;
                bool x = false;
                for (int j = 0; j < k; j++) x |= cdm_isN(a.nmask, w0, pos + j) != 0;
                emit(w, groupsReversed(w, k), pos, x);
            }
        } else {
            // two consecutive positions per lane: the second window is the first one shifted by a base, and its Indexer-order
            // k-mer follows from the first one's without a second bit reversal
            for (uint32_t pos = 2 * lane; pos < nPos; pos += 128) {
                const uint64_t xr = kmerWindow(a.codes, w0, pos, lastWord, k);      // k + 1 bases
                const uint64_t wA = xr & kmask, idxA = groupsReversed(wA, k);
                emit(wA, idxA, pos, false);
                if (pos + 1 < nPos) {
                    const uint64_t wB = (xr >> 2) & kmask, idxB = ((idxA << 2) & kmask) | ((xr >> (2 * k)) & 3ull);
                    emit(wB, idxB, pos + 1, false);
                }
            }
        }
        const bool anyDup = __ballot(dup) != 0ull;
        if (anyDup && lane == 0) a.slowShort[atomicAdd(&a.slowCnt[0], 1u)] = seq;   // rewritten by k_extract
        // head digits: a sequence that stays as written counts the k-mers its hash set holds (every one it stored); one that k_extract
        // rewrites is counted there
        if (countHead && a.ignoreMultiKmer && !anyDup) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            for (uint32_t i = lane; i < tsize; i += 64) { const unsigned long long km = table[i]; if (km != ~0ull && inRange(a, km)) atomicAdd(&sHead[km >> a.headShift], 1u); }
        }
        noteBelow(a, below);
        __builtin_amdgcn_wave_barrier();
    }
    if (countHead) headHistFlush(sHead, a.headHist);
}


// Short reads, two per wavefront: a half-wave per sequence, three consecutive positions per lane (one 64-bit window and one
// bit reversal serve all three), each half with its own LDS hash set.  A 100 bp read has 81 positions: 27 busy lanes per half
// instead of 41 of 64 with a wave per read, and the per-sequence bookkeeping is shared by two sequences.  Sequences that do not
// fit (N letters, more than 96 positions, not every k-mer taken) go to k_extract_fast through the `single` list.
constexpr int PAIR_POS = 96, PAIR_TABLE = 256;
template <typename LY>
__global__ __launch_bounds__(64 * FAST_WAVES) void k_extract_pair(ExtractArgs<LY> a) {
    __shared__ unsigned long long sTable[FAST_WAVES][2 * PAIR_TABLE];
    __shared__ unsigned int sHead[LY::bySlot ? HEAD_BINS : 1];
    const bool countHead = LY::bySlot && a.headHist != nullptr;
    if (countHead) headHistClear(sHead);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, hl = lane & 31;
    unsigned long long *table = sTable[wave] + half * PAIR_TABLE;
    const int k = a.k;
    const uint64_t kmask = (1ull << (2 * k)) - 1ull;
    const uint32_t nPairs = (a.n + 1) / 2;
    for (uint32_t pr = blockIdx.x * FAST_WAVES + wave; pr < nPairs; pr += gridDim.x * FAST_WAVES) {
        const uint32_t seq = 2 * pr + (uint32_t) half;
        const bool have = seq < a.n && ownedSeq(a, seq);
        uint32_t L = 0, w0 = 0; bool hasN = false; uint64_t base = 0;
        if (have) { L = a.len[seq]; w0 = a.woff[seq]; hasN = a.hasN[seq] != 0; base = slotBase(a, seq); }
        const uint32_t nPos = (L >= (uint32_t) k) ? (L - k + 1) : 0;
        const size_t cap = (size_t) (float) ((float) (a.kmersPerSeq - 1) + (a.scale * (float) L));
        const bool elig = have && nPos <= cap && nPos <= (uint32_t) PAIR_POS && !hasN;
        if (have && !elig && hl == 0) a.single[atomicAdd(&a.slowCnt[2], 1u)] = seq;
        for (int i = hl; i < PAIR_TABLE; i += 32) table[i] = ~0ull;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier();
        bool dup = false, below = false;
        constexpr uint32_t NO_DIGIT = 0xFFFFFFFFu;
        // (returns the head digit of the tuple it stored, NO_DIGIT if the slot stays empty)
        auto emit = [&](uint64_t w, uint64_t idx, uint32_t pos) -> uint32_t {
            const uint64_t rc = (w ^ 0xAAAAAAAAAAAAAAAAull) & kmask;     // Util::revComplement(idx): window order, complemented
            if (rc != idx) {
                const bool pickRev = rc < idx;
                const uint64_t km = pickRev ? rc : idx;
                const uint32_t p = pickRev ? (L - pos - k) : pos;
                if (a.ignoreMultiKmer) {
                    uint32_t h = (uint32_t) ((km * 0x9E3779B97F4A7C15ull) >> 40) & (PAIR_TABLE - 1);
                    while (true) {
                        const unsigned long long old = atomicCAS(&table[h], ~0ull, (unsigned long long) km);
                        if (old == ~0ull) break;
                        if (old == km) { dup = true; break; }
                        h = (h + 1) & (PAIR_TABLE - 1);
                    }
                }
                below |= km < a.kLo;
                if (inRange(a, km)) { LY::store(a.keys, a.vals, base + 1 + pos, km, !pickRev, seq, L, p, a.geom); return (uint32_t) (km >> a.headShift); }
                LY::storeEmpty(a.keys, a.vals, base + 1 + pos);
            } else LY::storeEmpty(a.keys, a.vals, base + 1 + pos);
            return NO_DIGIT;
        };
        const uint32_t pos = 3u * (uint32_t) hl;
        uint32_t dA = NO_DIGIT, dB = NO_DIGIT, dC = NO_DIGIT;
        if (elig && pos < nPos) {
            const uint64_t xr = kmerWindow(a.codes, w0, pos, (L + 15) / 16 - 1, k);     // k + 2 bases
            const uint64_t wA = xr & kmask, idxA = groupsReversed(wA, k);
            dA = emit(wA, idxA, pos);
            if (pos + 1 < nPos) {
                const uint64_t idxB = ((idxA << 2) & kmask) | ((xr >> (2 * k)) & 3ull);
                dB = emit((xr >> 2) & kmask, idxB, pos + 1);
                if (pos + 2 < nPos) dC = emit((xr >> 4) & kmask, ((idxB << 2) & kmask) | ((xr >> (2 * k + 2)) & 3ull), pos + 2);
            }
        }
        const unsigned long long dm = __ballot(dup);
        const bool halfDup = (half ? (dm >> 32) : (dm & 0xFFFFFFFFull)) != 0ull;
        if (halfDup && hl == 0) a.slowShort[atomicAdd(&a.slowCnt[0], 1u)] = seq;   // rewritten by k_extract
        if (countHead && !halfDup) {        // (a sequence k_extract rewrites is counted there)
            if (dA != NO_DIGIT) atomicAdd(&sHead[dA], 1u);
            if (dB != NO_DIGIT) atomicAdd(&sHead[dB], 1u);
            if (dC != NO_DIGIT) atomicAdd(&sHead[dC], 1u);
        }
        noteBelow(a, below);
        __builtin_amdgcn_wave_barrier();
    }
    if (countHead) headHistFlush(sHead, a.headHist);
}

// A PLAIN UNIFORM DB (common.h MetaUniform) in the slot layout, the whole k-mer space on one device: ONE kernel writes what k_seq_hash and
// k_extract_pair write together.  A half-wave per read as there, but
//   - length and word offset follow from the index (no per-read metadata loads).  A wave works on BATCHES of 32 consecutive pairs:
//     the 64 reads' words are one contiguous stretch, loaded with at most 8 coalesced instructions ONE BATCH AHEAD and kept in LDS
//     while the batch is worked on; a lane reads the words of its windows from there.  Nothing inside a batch waits for memory:
//     the stores stream out behind the wave (a wait for a load would be s_waitcnt vmcnt(0) here, i.e. for every store before it);
//   - lane hl has the positions hl, hl + 32, hl + 64: a store instruction of a half writes 256 contiguous bytes.  All three windows of
//     a lane start at the same bit of a word, two words apart: two v_alignbit each;
//   - the repeated-k-mer test is a set of 32-bit tags (256 x 4 bytes per half; the tag is the k-mer's low word with its bits from 32 on
//     folded in - the k-mer itself up to k = 15).  Equal k-mers have equal tags and walk the same probe sequence, so no repeat is
//     missed; two different k-mers of a read share a tag once in ~10^7 reads, and all that costs is that read's trip through
//     k_extract, which is exact.  No multiplication anywhere in an iteration: the kernel is bound by its vector instructions
//     (a wave's takes a SIMD four cycles, v_mul_lo_u32 sixteen);
//   - the whole-sequence hashes (Util::hash's Horner walk, then XXH64) are made once per batch by all 64 lanes, a lane per read, from
//     the words in LDS - a few instructions per letter for 64 reads at once, as in k_seq_hash, without its second pass over the DB -
//     and the region-2 stores of a batch are 64 consecutive keys.
// k_uniform_check is the test k_build_meta makes (seqdb.hip), without the table.
__global__ void k_uniform_check(const uint32_t *__restrict__ len, const uint32_t *__restrict__ woff, const uint8_t *__restrict__ hasN, uint32_t n, uint32_t uniLen, uint32_t uniWords,
                                unsigned int *__restrict__ notUniform) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (len[i] != uniLen || woff[i] != i * uniWords || hasN[i] != 0)) atomicOr(notUniform, 1u);
}
constexpr int UNI_TABLE = 256, UNI_BATCH = 32, UNI_MINW = 8, UNI_WORDS = 8;      // (96 positions of k <= 30 letters: at most 8 words per read)
static_assert(PAIR_POS == 96 && UNI_BATCH * 2 == 64, "three rounds of 32 positions per half; a lane per read of the batch for the hashes");
template <typename LY>
__global__ __launch_bounds__(64 * FAST_WAVES, UNI_MINW) void k_extract_uniform(ExtractArgs<LY> a, uint32_t L, uint32_t W) {
    static_assert(LY::bySlot, "slot layout only");
    __shared__ __attribute__((aligned(16))) uint32_t sTag[FAST_WAVES][2][UNI_TABLE];
    __shared__ uint32_t sWords[FAST_WAVES][64 * UNI_WORDS + 8];       // the batch's words (+ 8: the last read's windows look two words on)
    __shared__ unsigned int sHead[HEAD_BINS];
    const bool countHead = a.headHist != nullptr;
    if (countHead) headHistClear(sHead);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, hl = lane & 31;
    uint32_t *table = sTag[wave][half];
    const int k = a.k;
    const uint64_t kmask = (1ull << (2 * k)) - 1ull;
    const uint32_t nPos = L - (uint32_t) k + 1u, uniS = a.uniS, n = a.n;
    const uint32_t nPairs = (n + 1) / 2, nBatch = (nPairs + UNI_BATCH - 1) / UNI_BATCH;
    const uint32_t waveId = blockIdx.x * FAST_WAVES + wave, nWaves = gridDim.x * FAST_WAVES;
    const uint32_t sh = (uint32_t) (hl & 15) * 2u, rsh = 64u - 2u * (uint32_t) k;
    uint32_t *words = sWords[wave];
    const uint64_t nWords = (uint64_t) n * W;
    // words j x 64 + lane (j < W) of the 64 reads of batch b, A,C,G,T -> A,C,T,G (0: behind the DB's last word)
    uint32_t pre[UNI_WORDS];
    auto loadBatch = [&](uint64_t b) {
#pragma unroll
        for (int j = 0; j < UNI_WORDS; j++) {
            const uint64_t g = b * (2u * UNI_BATCH) * W + (uint32_t) (j * 64 + lane);
            pre[j] = ((uint32_t) j < W && b < nBatch && g < nWords) ? a.codes[g] : 0u;
        }
    };
    loadBatch(waveId);
    for (uint32_t b = waveId; b < nBatch; b += nWaves) {
        const uint32_t pr0 = b * UNI_BATCH, cnt = min((uint32_t) UNI_BATCH, nPairs - pr0);
#pragma unroll
        for (int j = 0; j < UNI_WORDS; j++) if ((uint32_t) j < W) words[j * 64 + lane] = pre[j] ^ ((pre[j] >> 1) & 0x55555555u);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
        loadBatch((uint64_t) b + nWaves);      // the wave's next batch: on its way while this one is worked on
        for (uint32_t it = 0; it < cnt; it++) {
            const uint32_t pr = pr0 + it, seq = 2 * pr + (uint32_t) half;
            const bool have = seq < n;
            const uint64_t base = (uint64_t) seq * uniS;
            const uint32_t *rw = words + (2 * it + (uint32_t) half) * W;
            { uint4 z; z.x = z.y = z.z = z.w = 0u; ((uint4 *) table)[hl] = z; ((uint4 *) table)[hl + 32] = z; }
            // The set is this wave's own, and a wave's LDS instructions execute in order: a fence of WAVEFRONT scope keeps the compiler from
            // moving the compare-and-swaps in front of the clear and costs no wait.  (A workgroup-scope release, as in k_extract_pair, orders
            // every address space: s_waitcnt vmcnt(0) - the iteration then waits for the read-ahead and for all stores of the one before.)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
            uint32_t x[7];
#pragma unroll
            for (int i = 0; i < 7; i++) x[i] = rw[(hl >> 4) + i];
            // ---- the k-mers at hl, hl + 32, hl + 64
            uint64_t key[3]; uint32_t tag[3], digit[3]; bool real[3];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const uint32_t pos = 32u * j + (uint32_t) hl;
                const bool act = have && pos < nPos;
                const uint32_t lo = __builtin_amdgcn_alignbit(x[2 * j + 1], x[2 * j], sh), hi = __builtin_amdgcn_alignbit(x[2 * j + 2], x[2 * j + 1], sh);
                const uint64_t w = (((uint64_t) hi << 32) | lo) & kmask;
                const uint64_t rc = (w ^ 0xAAAAAAAAAAAAAAAAull) & kmask;     // Util::revComplement(idx): window order, complemented
                // Indexer order (groupsReversed): all bits reversed, the two bits of every letter swapped back
                uint64_t idx;
                {
                    const uint32_t rh = __builtin_bitreverse32((uint32_t) w), rl = __builtin_bitreverse32((uint32_t) (w >> 32));      // (the reversed value's high and low word)
                    const uint32_t th = ((rh >> 1) & 0x55555555u) | ((rh & 0x55555555u) << 1), tl = ((rl >> 1) & 0x55555555u) | ((rl & 0x55555555u) << 1);
                    // >> (64 - 2k), word by word (64-bit shifts are slow vector instructions)
                    idx = rsh >= 32u ? (uint64_t) (th >> (rsh - 32u)) : (((uint64_t) (th >> rsh) << 32) | __builtin_amdgcn_alignbit(th, tl, rsh));
                }
                const bool pickRev = rc < idx;
                const uint64_t km = pickRev ? rc : idx;
                real[j] = act && rc != idx;
                key[j] = rc != idx ? (km | (pickRev ? 0ull : BIT63)) : ~0ull;
                tag[j] = ((uint32_t) km ^ ((uint32_t) (km >> 32) << 4)) | 0x80000000u;      // (never 0 = empty; k <= 30: 28 bits from 32 on)
                digit[j] = (uint32_t) (km >> a.headShift);
                if (act) a.keys[base + 1 + pos] = key[j];
            }
            if (have && hl == 0) a.keys[base] = ~0ull;      // (slot 0: a hash that fits 2k bits is written at the batch's end, behind this)
            bool dup = false;
            if (a.ignoreMultiKmer) {
                uint32_t h[3], old[3];
#pragma unroll
                for (int j = 0; j < 3; j++) { h[j] = tag[j] & (UNI_TABLE - 1); old[j] = real[j] ? atomicCAS(&table[h[j]], 0u, tag[j]) : 0u; }
#pragma unroll
                for (int j = 0; j < 3; j++)
                    while (old[j] != 0u) {
                        if (old[j] == tag[j]) { dup = true; break; }
                        h[j] = (h[j] + 1) & (UNI_TABLE - 1);
                        old[j] = atomicCAS(&table[h[j]], 0u, tag[j]);
                    }
            }
            const unsigned long long dm = __ballot(dup);
            const bool halfDup = (half ? (dm >> 32) : (dm & 0xFFFFFFFFull)) != 0ull;
            if (halfDup && hl == 0) a.slowShort[atomicAdd(&a.slowCnt[0], 1u)] = seq;   // rewritten by k_extract
            if (countHead && !halfDup) {        // (a sequence k_extract rewrites is counted there)
#pragma unroll
                for (int j = 0; j < 3; j++) if (real[j]) atomicAdd(&sHead[digit[j]], 1u);
            }
            __builtin_amdgcn_wave_barrier();
        }
        // ---- the whole-sequence hash tuples of the batch's sequences (putSeqHashTuple for the whole k-mer space): lane l has sequence
        // 2 pr0 + l and walks its words in LDS
        const uint32_t seq = 2 * pr0 + (uint32_t) lane;
        if ((uint32_t) (lane >> 1) < cnt && seq < n) {
            uint64_t acc = 0;
            for (uint32_t j = 0; j < W; j++) {
                uint32_t word = words[(uint32_t) lane * W + j];
                const uint32_t nb = min(16u, L - 16u * j);
                for (uint32_t i = 0; i < nb; i++) { acc = (acc << 5) - acc + (word & 3u); word >>= 2; }      // h = h x 31 + c
            }
            const uint64_t hk = xxh64_u64(acc, a.seed);
            const uint64_t hslot = a.hashBase + seq;
            if ((hk & ~BIT63) < (1ull << (2 * k))) {            // (one sequence in 2^(63 - 2k): the tuple stays in slot 0)
                __threadfence();                                 // behind the ~0 another lane of this wave put there
                LY::storeHash(a.keys, a.vals, (uint64_t) seq * uniS, hk, seq, L, a.geom);
                if (a.headHist) atomicAdd(&a.headHist[(hk & ~BIT63) >> a.headShift], 1ull);
                LY::storeEmpty(a.keys, a.vals, hslot);
            } else LY::storeHash(a.keys, a.vals, hslot, hk, seq, L, a.geom);
        }
    }
    if (countHead) headHistFlush(sHead, a.headHist);
}

// sort element of the per-sequence ordering compareByScoreReverse (kmermatcher.h:30-46): (score, kmer|bit63, pos)
struct SeqPos { uint64_t a, b; };   // a = score << 48 | kmer63 >> 15 ; b = (kmer63 & 0x7FFF) << 49 | pos << 1 | forward
__device__ __forceinline__ bool spLess(const SeqPos &x, const SeqPos &y) { return x.a < y.a || (x.a == y.a && x.b < y.b); }
__device__ __forceinline__ uint64_t spKmer63(const SeqPos &x) { return ((x.a & 0xFFFFFFFFFFFFull) << 15) | (x.b >> 49); }
__device__ __forceinline__ uint32_t spScore(const SeqPos &x) { return (uint32_t) (x.a >> 48); }
__device__ __forceinline__ uint32_t spPos(const SeqPos &x) { return (uint32_t) ((x.b >> 1) & 0xFFFFFFFFFFFFull); }

// the (score, k-mer, position, strand) record of the k-mer at pos, false if it has an N or is its own reverse complement
// (Sequence::nextKmer + Indexer::computeKmerIdx, canonical pick kmermatcher.cpp:155-190)
template <typename LY>
__device__ __forceinline__ bool makeSeqPos(const ExtractArgs<LY> &a, uint32_t w0, uint32_t L, uint32_t lastWord, bool hasN, int k, uint32_t pos, SeqPos &e) {
    // k bases starting at pos in MMseqs coding (gray code of ours), first base most significant
    uint64_t idx = 0; bool x = false;
    for (int j = 0; j < k; j += 16) {
        uint32_t w = cdm_window16(a.codes, w0, pos + j, lastWord);
        w ^= (w >> 1) & 0x55555555u;                       // A,C,G,T -> A,C,T,G
        const int take = min(16, k - j);
        for (int b = 0; b < take; b++) idx = (idx << 2) | ((w >> (2 * b)) & 3u);
    }
    if (hasN) for (int j = 0; j < k; j++) x |= cdm_isN(a.nmask, w0, pos + j) != 0;
    if (x) return false;
    const uint64_t rc = revComplement(idx, k);
    if (rc == idx) return false;
    const bool pickRev = rc < idx;
    const uint64_t km = pickRev ? rc : idx;
    const uint32_t score = (uint32_t) (xxh64_u64(km, a.seed) & 0xFFFFu);
    const uint32_t p = pickRev ? (L - pos - k) : pos;
    e.a = ((uint64_t) score << 48) | (km >> 15);
    e.b = ((km & 0x7FFFull) << 49) | ((uint64_t) p << 1) | (pickRev ? 0ull : 1ull);
    return true;
}

// SequencePosition::compareByScoreReverse (kmermatcher.h:29-46): score, k-mer without the strand bit, position - NOT the strand
__device__ __forceinline__ bool spCmp(const SeqPos &x, const SeqPos &y) { return x.a < y.a || (x.a == y.a && (x.b >> 1) < (y.b >> 1)); }

// libstdc++'s std::sort (bits/stl_algo.h: introsort with median-of-three, threshold 16, heap sort below the depth limit, final
// insertion sort), statement for statement.  The reference sorts a sequence's k-mers with it (SORT_SERIAL, kmermatcher.cpp:271)
// and its comparator ignores the strand: when a sequence carries the same canonical k-mer at the same stored position on both
// strands, which of the two comes first - and with it the strand of a tuple - is whatever this algorithm leaves.  Serial, one
// thread; only such sequences come here.
__device__ void stdAdjustHeap(SeqPos *first, long holeIndex, long len, SeqPos value) {
    const long topIndex = holeIndex;
    long secondChild = holeIndex;
    while (secondChild < (len - 1) / 2) {
        secondChild = 2 * (secondChild + 1);
        if (spCmp(first[secondChild], first[secondChild - 1])) secondChild--;
        first[holeIndex] = first[secondChild];
        holeIndex = secondChild;
    }
    if ((len & 1) == 0 && secondChild == (len - 2) / 2) {
        secondChild = 2 * (secondChild + 1);
        first[holeIndex] = first[secondChild - 1];
        holeIndex = secondChild - 1;
    }
    long parent = (holeIndex - 1) / 2;                          // __push_heap
    while (holeIndex > topIndex && spCmp(first[parent], value)) { first[holeIndex] = first[parent]; holeIndex = parent; parent = (holeIndex - 1) / 2; }
    first[holeIndex] = value;
}
__device__ void stdHeapSort(SeqPos *first, long n) {           // __partial_sort(first, last, last): make_heap + sort_heap
    if (n >= 2) {
        long parent = (n - 2) / 2;
        while (true) { const SeqPos v = first[parent]; stdAdjustHeap(first, parent, n, v); if (parent == 0) break; parent--; }
    }
    for (long last = n; last > 1;) { --last; const SeqPos v = first[last]; first[last] = first[0]; stdAdjustHeap(first, 0, last, v); }
}
__device__ void stdUnguardedLinearInsert(SeqPos *base, long last) {
    const SeqPos val = base[last];
    long next = last - 1;
    while (spCmp(val, base[next])) { base[last] = base[next]; last = next; --next; }
    base[last] = val;
}
__device__ void stdInsertionSort(SeqPos *base, long first, long last) {
    if (first == last) return;
    for (long i = first + 1; i != last; ++i) {
        if (spCmp(base[i], base[first])) { const SeqPos val = base[i]; for (long j = i; j > first; j--) base[j] = base[j - 1]; base[first] = val; }
        else stdUnguardedLinearInsert(base, i);
    }
}
__device__ void stdSort(SeqPos *base, long n) {
    if (n <= 0) return;
    // __introsort_loop with an explicit stack for its one recursive call
    long stFirst[64], stLast[64]; int stDepth[64]; int top = 0;
    int lg = 0; for (long v = n; v > 1; v >>= 1) lg++;
    stFirst[0] = 0; stLast[0] = n; stDepth[0] = 2 * lg; top = 1;
    while (top > 0) {
        top--;
        long first = stFirst[top], last = stLast[top]; int depth = stDepth[top];
        while (last - first > 16) {
            if (depth == 0) { stdHeapSort(base + first, last - first); break; }
            --depth;
            // __unguarded_partition_pivot
            const long mid = first + (last - first) / 2, ia = first + 1, ib = mid, ic = last - 1;
            long m;                                             // __move_median_to_first(first, a, b, c)
            if (spCmp(base[ia], base[ib])) { if (spCmp(base[ib], base[ic])) m = ib; else if (spCmp(base[ia], base[ic])) m = ic; else m = ia; }
            else if (spCmp(base[ia], base[ic])) m = ia; else if (spCmp(base[ib], base[ic])) m = ic; else m = ib;
            { const SeqPos t = base[first]; base[first] = base[m]; base[m] = t; }
            long lo = first + 1, hi = last;                     // __unguarded_partition(first + 1, last, first)
            while (true) {
                while (spCmp(base[lo], base[first])) ++lo;
                --hi;
                while (spCmp(base[first], base[hi])) --hi;
                if (!(lo < hi)) break;
                { const SeqPos t = base[lo]; base[lo] = base[hi]; base[hi] = t; }
                ++lo;
            }
            const long cut = lo;
            stFirst[top] = cut; stLast[top] = last; stDepth[top] = depth; top++;     // __introsort_loop(cut, last, depth)
            last = cut;
        }
    }
    // __final_insertion_sort
    if (n > 16) { stdInsertionSort(base, 0, 16); for (long i = 16; i != n; ++i) stdUnguardedLinearInsert(base, i); }
    else stdInsertionSort(base, 0, n);
}

// One workgroup of NT threads per sequence; CAP = power of two >= number of k-mers of the sequence, records in LDS; CAP = 0:
// records in a per-block slice of global scratch (sequences with 4096 positions or more: rare, speed is not the point).
template <typename LY, int CAP, int NT>
__global__ __launch_bounds__(NT) void k_extract(ExtractArgs<LY> a) {
    __shared__ SeqPos sSp[CAP ? CAP : 1];
    __shared__ uint8_t sSel[CAP ? CAP : 1];
    SeqPos *sp = CAP ? sSp : a.hugeSp + (size_t) blockIdx.x * a.hugeCap;
    uint8_t *sel = CAP ? sSel : a.hugeSel + (size_t) blockIdx.x * a.hugeCap;
    __shared__ uint32_t sN, sCursor;
    // CAP = 0: the head of the sorted records is copied to LDS for the serial selection walk (one thread chasing through global
    // scratch took milliseconds per contig; the walk ends after ~0.2 n + 200 records)
    constexpr uint32_t HEADN = CAP ? 1 : 3072;
    __shared__ SeqPos sHead[HEADN];
    __shared__ unsigned int sDigits[LY::bySlot ? HEAD_BINS : 1];
    const bool countHead = LY::bySlot && a.headHist != nullptr;
    if (countHead) headHistClear(sDigits);
    const int tid = threadIdx.x;
    for (uint32_t item = blockIdx.x; item < a.nList; item += gridDim.x) {
        const uint32_t seq = a.list[item];
        const uint32_t L = a.len[seq], w0 = a.woff[seq];
        const bool hasN = a.hasN[seq] != 0;
        const int k = a.k;
        const uint32_t nPos = (L >= (uint32_t) k) ? (L - k + 1) : 0;
        if (tid == 0) sN = 0;
        __syncthreads();
        // ---- k-mers (Sequence::nextKmer + Indexer::computeKmerIdx, canonical pick kmermatcher.cpp:155-190)
        const uint32_t lastWord = (L + 15) / 16 - 1;
        for (uint32_t pos = tid; pos < nPos; pos += NT) {
            SeqPos e;
            if (!makeSeqPos(a, w0, L, lastWord, hasN, k, pos, e)) continue;
            const uint32_t slot = atomicAdd(&sN, 1u);
            sp[slot] = e;
        }
        __syncthreads();
        const uint32_t n = sN;
        // ---- sort by (score, kmer, pos): bitonic over the next power of two, padding = max
        uint32_t np2 = 1; while (np2 < n) np2 <<= 1;
        for (uint32_t i = n + tid; i < np2; i += NT) { sp[i].a = ~0ull; sp[i].b = ~0ull; }
        __syncthreads();
        if constexpr (CAP == 0) {
            // The records are in global scratch.  The same bitonic network, but every exchange over a distance below CH happens in
            // LDS: the array is taken CH records at a time (sHead's memory - it holds the head of the sorted records only later), all
            // the network's stages that stay inside such a stretch run there, and only the exchanges over CH records or more go
            // through memory - 28 passes over the array instead of 153 for a 100 k-letter contig (this kernel was half of the
            // device time of the workflow loop's contig iterations).
            constexpr uint32_t CH = 2048;
            static_assert(CH <= HEADN, "the chunk lives in sHead");
            const uint32_t cs = min(np2, CH);
            auto ldsStages = [&](uint32_t c0, uint32_t size, uint32_t strideFrom) {      // stages of `size` with stride <= strideFrom on [c0, c0 + cs)
                for (uint32_t i = tid; i < cs; i += NT) sHead[i] = sp[c0 + i];
                __syncthreads();
                for (uint32_t stride = strideFrom; stride > 0; stride >>= 1) {
                    for (uint32_t t = tid; t < cs / 2; t += NT) {
                        const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                        const bool up = ((c0 + lo) & size) == 0;
                        SeqPos x = sHead[lo], y = sHead[hi];
                        if (spLess(y, x) == up) { sHead[lo] = y; sHead[hi] = x; }
                    }
                    __syncthreads();
                }
            };
            for (uint32_t c0 = 0; c0 < np2; c0 += cs) {          // sizes up to the chunk: wholly in LDS
                for (uint32_t i = tid; i < cs; i += NT) sHead[i] = sp[c0 + i];
                __syncthreads();
                for (uint32_t size = 2; size <= cs; size <<= 1)
                    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                        for (uint32_t t = tid; t < cs / 2; t += NT) {
                            const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                            const bool up = ((c0 + lo) & size) == 0;
                            SeqPos x = sHead[lo], y = sHead[hi];
                            if (spLess(y, x) == up) { sHead[lo] = y; sHead[hi] = x; }
                        }
                        __syncthreads();
                    }
                for (uint32_t i = tid; i < cs; i += NT) sp[c0 + i] = sHead[i];
                __syncthreads();
            }
            for (uint32_t size = 2 * cs; size <= np2 && size != 0; size <<= 1) {
                for (uint32_t stride = size >> 1; stride >= cs; stride >>= 1) {
                    for (uint32_t t = tid; t < np2 / 2; t += NT) {
                        const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                        const bool up = (lo & size) == 0;
                        SeqPos x = sp[lo], y = sp[hi];
                        if (spLess(y, x) == up) { sp[lo] = y; sp[hi] = x; }
                    }
                    __syncthreads();
                }
                for (uint32_t c0 = 0; c0 < np2; c0 += cs) {
                    ldsStages(c0, size, cs >> 1);
                    for (uint32_t i = tid; i < cs; i += NT) sp[c0 + i] = sHead[i];
                    __syncthreads();
                }
            }
        } else
        for (uint32_t size = 2; size <= np2; size <<= 1)
            for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                for (uint32_t t = tid; t < np2 / 2; t += NT) {
                    const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                    const bool up = (lo & size) == 0;
                    SeqPos x = sp[lo], y = sp[hi];
                    if (spLess(y, x) == up) { sp[lo] = y; sp[hi] = x; }
                }
                __syncthreads();
            }
        // The bitonic order breaks comparator ties by the strand bit.  The reference's comparator has no such rule: if two records
        // tie (same score, k-mer, stored position, opposite strands) redo the sort the way the reference does, from the order
        // in which fillKmerPositionArray generated the records (ascending position).
        {
            int tie = 0;
            for (uint32_t i = tid; i + 1 < n; i += NT) tie |= (sp[i].a == sp[i + 1].a && (sp[i].b >> 1) == (sp[i + 1].b >> 1));
            if (__syncthreads_or(tie && a.ignoreMultiKmer)) {
                if (tid == 0) {
                    uint32_t m = 0;
                    for (uint32_t pos = 0; pos < nPos; pos++) { SeqPos e; if (makeSeqPos(a, w0, L, lastWord, hasN, k, pos, e)) sp[m++] = e; }
                    stdSort(sp, (long) m);
                }
                __syncthreads();
            }
        }
        // ---- selection (kmermatcher.cpp:224-240, 277-350)
        const size_t considered = min((size_t) (float) ((float) (a.kmersPerSeq - 1) + (a.scale * (float) L)), (size_t) n);
        uint32_t headN = 0;
        if (CAP == 0) { headN = min(n, HEADN); for (uint32_t i = tid; i < headN; i += NT) sHead[i] = sp[i]; }
        // fast path test: no two equal k-mers next to each other, and every k-mer is taken
        int dup = 0;
        for (uint32_t i = tid; i + 1 < n; i += NT) dup |= (spKmer63(sp[i]) == spKmer63(sp[i + 1]));
        const int anyDup = __syncthreads_or(dup && a.ignoreMultiKmer);
        if (!anyDup && considered == n) {
            for (uint32_t i = tid; i < n; i += NT) sel[i] = 1;
        } else {
            for (uint32_t i = tid; i < n; i += NT) sel[i] = 0;
            __syncthreads();
            // The selection walk is serial (one thread), its reads are not: with the records in global scratch (CAP = 0) the block
            // stages the next HEADN records in LDS, thread 0 walks them, and so on until the walk is done (it ends after about
            // 0.2 n + 200 records; chasing them one by one through global memory took ~1 us each).
            __shared__ uint32_t wThreshold, wDone; __shared__ int wTooMuch; __shared__ unsigned long long wKi, wSelected;
            uint32_t winLo = 0, winN = headN;                 // [winLo, winLo + winN) of the sorted records is in sHead
            auto at = [&](size_t i) -> SeqPos { return (CAP == 0 && i >= winLo && i < (size_t) winLo + winN) ? sHead[i - winLo] : sp[i]; };
            if (tid == 0) {
                wDone = (n == 0) ? 1u : 0u; wKi = 0; wSelected = 0; wThreshold = 0; wTooMuch = 0;
                if (n > 0) {
                    // threshold = (score of the considered-th smallest) + 1, inBins = #(score < threshold)  [:224-240]
                    uint32_t threshold = 0; size_t inBins = 0;
                    if (considered > 0) {
                        threshold = spScore(at(considered - 1)) + 1;
                        inBins = considered;
                        while (inBins < n && spScore(at(inBins)) < threshold) inBins++;
                    } else {
                        // the reference's loops leave threshold at the start of the first non-empty 512-bin and subtract that bin
                        threshold = (spScore(at(0)) >> 9) * 512; inBins = 0;
                    }
                    wThreshold = threshold; wTooMuch = (int) (inBins - considered);
                    if (!a.ignoreMultiKmer) {
                        // without --ignore-multi-kmer the reference does not sort (:269-275): the selection walks the k-mers in the
                        // order they were generated; the threshold above only needed the score distribution
                        uint32_t m = 0;
                        for (uint32_t pos = 0; pos < nPos; pos++) { SeqPos e; if (makeSeqPos(a, w0, L, lastWord, hasN, k, pos, e)) sp[m++] = e; }
                    }
                }
            }
            __syncthreads();
            if (CAP == 0 && !a.ignoreMultiKmer) { winN = min(n, HEADN); for (uint32_t i = tid; i < winN; i += NT) sHead[i] = sp[i]; __syncthreads(); }   // (the LDS copy held the sorted order)
            while (!wDone) {
                if (tid == 0) {
                    uint32_t threshold = wThreshold; int tooMuch = wTooMuch; size_t ki = (size_t) wKi, selected = (size_t) wSelected;
                    // walk while the record and its successor are staged (CAP != 0: everything is)
                    const size_t stop = (CAP == 0) ? ((size_t) winLo + winN >= n ? n : (size_t) winLo + winN - 1) : n;
                    for (; ki < n && selected < considered; ki++) {
                        if (ki >= stop) break;
                        if (a.ignoreMultiKmer) {
                            const uint64_t km = spKmer63(at(ki));
                            if (ki + 1 < n) {
                                uint64_t nx = spKmer63(at(ki + 1));
                                if (km == nx) {
                                    while (km == nx && ki < n) { ki++; if (ki >= n) break; nx = spKmer63(at(ki)); }
                                }
                            }
                            if (ki >= n) break;
                        }
                        const uint32_t sc = spScore(at(ki));
                        if (sc < threshold) {
                            if (sc == (threshold - 1) && tooMuch) { tooMuch--; threshold -= (tooMuch == 0) ? 1 : 0; }
                            selected++;
                            sel[ki] = 1;
                        }
                    }
                    wThreshold = threshold; wTooMuch = tooMuch; wKi = ki; wSelected = selected;
                    wDone = (ki >= n || selected >= considered) ? 1u : 0u;
                }
                __syncthreads();
                if (CAP == 0 && !wDone) {      // next window starts at the record the walk stopped at
                    winLo = (uint32_t) wKi; winN = min(n - winLo, HEADN);
                    for (uint32_t i = tid; i < winN; i += NT) sHead[i] = sp[winLo + i];
                }
                __syncthreads();
            }
        }
        __syncthreads();
        // ---- emit: 1 whole-sequence tuple (:244-267) + the selected k-mers
        {
            const uint64_t base = slotBase(a, seq);
            if (tid == 0) sCursor = 0;       // (the whole-sequence tuple :244-267 is written by k_seq_hash)
            if constexpr (LY::bySlot) { for (uint32_t i = tid; i < nPos; i += NT) LY::storeEmpty(a.keys, a.vals, base + 1 + i); }      // (a slot IS a position: every one is written, the selected ones again)
            __syncthreads();
            // selected tuples first (their order within the sequence does not matter: a global sort follows), then sentinels
            for (uint32_t i = tid; i < n; i += NT) {
                if (!sel[i]) continue;
                const SeqPos e = sp[i];
                const uint64_t km = spKmer63(e);
                if (km < a.kLo && a.belowFlag[0] == 0u) a.belowFlag[0] = 1u;
                if (!inRange(a, km)) continue;              // another rank's k-mer range
                if constexpr (LY::bySlot) {
                    const bool fwd = (e.b & 1ull) != 0;
                    LY::store(a.keys, a.vals, base + 1 + (fwd ? spPos(e) : L - spPos(e) - (uint32_t) k), km, fwd, seq, L, spPos(e), a.geom);
                    if (countHead) atomicAdd(&sDigits[km >> a.headShift], 1u);
                } else {
                const uint32_t o = atomicAdd(&sCursor, 1u);
                LY::store(a.keys, a.vals, base + 1 + o, km, (e.b & 1ull) != 0, seq, L, spPos(e), a.geom);
                }
            }
            __syncthreads();
            if constexpr (!LY::bySlot) { for (uint32_t i = sCursor + tid; i < nPos; i += NT) LY::storeEmpty(a.keys, a.vals, base + 1 + i); }
        }
        __syncthreads();
    }
    if (countHead) headHistFlush(sDigits, a.headHist);
}

__global__ void k_len_keys(const uint32_t *__restrict__ len, uint32_t n, uint32_t maxLen, uint32_t *__restrict__ key, uint32_t *__restrict__ val) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { key[i] = maxLen - len[i]; val[i] = i; }   // ascending key = descending length; stable sort keeps ids ascending
}
// slots of the r-th sequence in (length desc, id asc) order
__global__ void k_slot_counts(const uint32_t *__restrict__ len, const uint32_t *__restrict__ order, uint32_t n, int k, unsigned long long *__restrict__ slots) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    if (r == n) { slots[r] = 0; return; }
    const uint32_t L = len[order[r]];
    slots[r] = 1ull + ((L >= (uint32_t) k) ? (L - k + 1) : 0);
}
__global__ void k_slot_scatter(const uint32_t *__restrict__ order, const unsigned long long *__restrict__ ordOff, uint32_t n, uint64_t *__restrict__ slotOff,
                               uint32_t *__restrict__ rankOf) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) { slotOff[order[r]] = ordOff[r]; rankOf[order[r]] = r; }
    if (r == n) slotOff[n] = ordOff[n];
}
// split by reads: only the sequences with order ranks [lo, hi) get slots
__global__ void k_slot_mask(unsigned long long *__restrict__ slots, uint32_t n, uint32_t lo, uint32_t hi) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n && (r < lo || r >= hi)) slots[r] = 0;
}
// Split by reads: the blocks of the slot order hold about the same number of SLOTS each (not of sequences: the order starts with the
// longest ones, and in a contig phase a tenth of the sequences holds nine tenths of the letters).  prefix = exclusive sums of the slot
// counts in that order, prefix[n] = all slots; block `blk` of `of` = the order ranks [out[0], out[1]): first rank whose prefix reaches
// total * blk / of - the same arithmetic on every rank, so the blocks tile the order.
__global__ void k_block_cuts(const unsigned long long *__restrict__ prefix, uint32_t n, uint32_t blk, uint32_t of, uint32_t *__restrict__ out) {
    const unsigned long long total = prefix[n];
    for (int side = 0; side < 2; side++) {
        const uint32_t b = blk + (uint32_t) side;
        uint32_t res = n;
        if (b < of) {
            const unsigned long long want = (unsigned long long) (((unsigned __int128) total * b) / of);
            uint32_t lo = 0, hi = n;
            while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (prefix[mid] < want) lo = mid + 1; else hi = mid; }
            res = lo;
        }
        out[side] = res;
    }
}
// first index of the keys (ordered by the `slices`-valued field at bit `shift`) whose field is >= p, for p = 0 .. slices
__global__ void k_slice_bounds(const uint64_t *__restrict__ keys, uint64_t m, int shift, uint32_t slices, unsigned long long *__restrict__ out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > slices) return;
    if (p == slices) { out[p] = m; return; }
    uint64_t lo = 0, hi = m;
    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (((keys[mid] >> shift) & (uint64_t) (slices - 1)) < p) lo = mid + 1; else hi = mid; }
    out[p] = lo;
}

}  // namespace
