// kmermatcher on the device (kmermatch.hip), the tuples: the physical layouts of the (k-mer, strand, sequence id, sequence length,
// position) tuple the reference keeps in KmerPosition<T> (lib/mmseqs/src/linclust/kmermatcher.h:49-54), the slot tuples of sort 1 on
// DBs of one sequence length (radix.h sortSlotKeys) and their conversion to (key, id) pairs, and the two hashes of K1.
#pragma once
#include "radix.h"

namespace {

constexpr uint64_t BIT63 = 1ull << 63;
// xxHash64 of one 8-byte word (lib/mmseqs/lib/xxhash/xxhash.h XXH64, len = 8; kmermatcher.cpp:33-38)
__host__ __device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__host__ __device__ __forceinline__ uint64_t xxh64_u64(uint64_t in, uint64_t seed) {
    const uint64_t P1 = 11400714785074694791ULL, P2 = 14029467366897019727ULL, P3 = 1609587929392839161ULL, P4 = 9650029242287828579ULL,
                   P5 = 2870177450012600261ULL;
    uint64_t h = seed + P5 + 8;
    uint64_t k1 = in * P2; k1 = rotl64(k1, 31); k1 *= P1;
    h ^= k1; h = rotl64(h, 27) * P1 + P4;
    h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
    return h;
}
// Util::revComplement (M/commons/Util.cpp:601-638) in MMseqs2's A,C,T,G = 0..3 coding: complement = xor 2
__device__ __forceinline__ uint64_t revComplement(uint64_t kmer, int k) {
    uint64_t x = kmer ^ 0xAAAAAAAAAAAAAAAAULL;
    x = ((x >> 2) & 0x3333333333333333ULL) | ((x & 0x3333333333333333ULL) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0FULL) | ((x & 0x0F0F0F0F0F0F0F0FULL) << 4);
    x = __builtin_bswap64(x);
    return x >> (64 - 2 * k);
}

// ------------------------------------------------------------------------------------------------ tuple layouts
// Two physical layouts of the (k-mer, strand, sequence id, sequence length, position) tuple the reference keeps in
// KmerPosition<T> (kmermatcher.h:49-54).  Region 1 of the array (one slot per k-mer position + slot 0 per sequence) is sorted
// on the low 2k key bits, region 2 (one whole-sequence hash tuple per sequence, 63 random bits) on 63 bits.
struct TupleGeom {
    int kbits, lb;              // 2k, bits of a length/position field
    uint64_t kmerSlots;         // size of region 1
    const uint32_t *lenArr;     // sequence lengths (region-2 tuples of the packed layout look their length up)
    // LayoutSlot (every sequence uniL letters): uniS slots per sequence; after sort 1 the region-1 tuples are SLOT TUPLES (radix.h) in
    // seg[0 .. BINS] segments by head digit (the k-mer bits from headShift on)
    uint32_t uniS = 0, uniL = 0; int uniK = 0; uint32_t uniMul = 0; int uniSh = 0;       // (uniMul, uniSh: division by uniS, slotSplit)
    const unsigned long long *seg = nullptr; int headShift = 0;
};
// division of a 32-bit number by an invariant d >= 1 (Granlund & Montgomery): q = (t + ((n - t) >> 1)) >> sh with t = mulhi(n, mul)
inline void divMagic(uint32_t d, uint32_t &mul, int &sh) {
    int l = 0; while ((1ull << l) < d) l++;
    mul = (uint32_t) ((((1ull << l) - d) << 32) / d + 1ull); sh = l > 0 ? l - 1 : 0;
    if (d == 1) { mul = 0; sh = 0; }       // t = 0: q = n >> 1 >> 0 would be wrong - d = 1 is special-cased in slotSplit
}
// head digit of the slot tuple at k-mer-order index idx: the last segment that starts at or in front of it
__device__ __forceinline__ uint32_t headDigit(const TupleGeom &g, uint64_t idx) {
    uint32_t d = 0;
#pragma unroll
    for (uint32_t st = rx::BINS / 2; st > 0; st >>= 1) if (g.seg[d + st] <= idx) d += st;
    return d;
}
// the same for a wave-uniform index: the nine look-ups go through the scalar cache (as vector loads they are nine L2 round trips in a
// row at the start of every wave of the grouping kernel: 67 instead of 49 ms at 50 M reads)
__device__ __forceinline__ uint32_t headDigitUniform(const TupleGeom &g, uint64_t idx) {
    const uint64_t u = ((uint64_t) (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) (idx >> 32)) << 32) | (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) idx);
    uint32_t d = 0;
#pragma unroll
    for (uint32_t st = rx::BINS / 2; st > 0; st >>= 1) { const unsigned long long b = g.seg[d + st]; if (b <= u) d += st; }
    return (uint32_t) __builtin_amdgcn_readfirstlane((int) d);
}
// slot index -> (sequence, slot of the sequence): slots are laid out sequence by sequence, uniS each (0: the whole-sequence hash tuple's
// slot, 1 + p: k-mer position p).  The quotient by a double product, corrected (exact for any 32-bit slot).
__device__ __forceinline__ void slotSplit(const TupleGeom &g, uint32_t slot, uint32_t &seq, uint32_t &r) {
    const uint32_t t = __umulhi(slot, g.uniMul);
    const uint32_t q = g.uniS == 1u ? slot : (t + ((slot - t) >> 1)) >> g.uniSh;
    seq = q; r = slot - q * g.uniS;
}
// 16 bytes: u64 key = k-mer | strand << 63, u64 value = id << 2 FB | len << FB | pos.  FB = 16: any DB with sequences below
// 65 536 letters (ids up to 2^32); FB = 20: sequences up to 2^20 letters (the reference's `int` position path,
// kmermatcher.cpp:803-808: contigs), ids up to 2^24.
template <int FB>
struct LayoutWideT {
    typedef uint64_t V;
    static constexpr bool bySlot = false;
    static constexpr uint64_t FM = (1ull << FB) - 1ull;
    __device__ static void store(uint64_t *keys, V *vals, uint64_t slot, uint64_t kmer63, bool fwd, uint32_t seq, uint32_t L, uint32_t pos, const TupleGeom &) {
        keys[slot] = kmer63 | (fwd ? BIT63 : 0ull); vals[slot] = ((uint64_t) seq << (2 * FB)) | ((uint64_t) L << FB) | pos;
    }
    __device__ static void storeHash(uint64_t *keys, V *vals, uint64_t slot, uint64_t hash64, uint32_t seq, uint32_t L, const TupleGeom &) {
        keys[slot] = hash64; vals[slot] = ((uint64_t) seq << (2 * FB)) | ((uint64_t) L << FB);
    }
    __device__ static void storeEmpty(uint64_t *keys, V *vals, uint64_t slot) { keys[slot] = ~0ull; vals[slot] = 0; }
    __device__ static uint64_t kmerOf(uint64_t key, uint64_t, const TupleGeom &) { return key & ~BIT63; }
    __device__ static uint32_t seqOf(V v) { return (uint32_t) (v >> (2 * FB)); }
    __device__ static uint32_t lenOf(uint64_t, V v, uint64_t, const TupleGeom &) { return (uint32_t) ((v >> FB) & FM); }
    __device__ static uint32_t posOf(uint64_t, V v, uint64_t, const TupleGeom &) { return (uint32_t) (v & FM); }
    // length and position of a region-1 tuple
    __device__ static void unpackR1(uint64_t, V v, const TupleGeom &, uint32_t &len, uint32_t &pos) { pos = (uint32_t) (v & FM); len = (uint32_t) ((v >> FB) & FM); }
};
typedef LayoutWideT<16> LayoutWide;
typedef LayoutWideT<20> LayoutLong;
// 16 bytes for any DB: u64 key = k-mer | strand << 63, u64 value = id << 32 | pos; the sequence's length is looked up (a DB of 2^24
// sequences or more with one of them beyond 65 534 letters: the contig iterations of a 25 M-read run, BASELINE config 5)
struct LayoutHuge {
    typedef uint64_t V;
    static constexpr bool bySlot = false;
    __device__ static void store(uint64_t *keys, V *vals, uint64_t slot, uint64_t kmer63, bool fwd, uint32_t seq, uint32_t, uint32_t pos, const TupleGeom &) {
        keys[slot] = kmer63 | (fwd ? BIT63 : 0ull); vals[slot] = ((uint64_t) seq << 32) | pos;
    }
    __device__ static void storeHash(uint64_t *keys, V *vals, uint64_t slot, uint64_t hash64, uint32_t seq, uint32_t, const TupleGeom &) { keys[slot] = hash64; vals[slot] = (uint64_t) seq << 32; }
    __device__ static void storeEmpty(uint64_t *keys, V *vals, uint64_t slot) { keys[slot] = ~0ull; vals[slot] = 0; }
    __device__ static uint64_t kmerOf(uint64_t key, uint64_t, const TupleGeom &) { return key & ~BIT63; }
    __device__ static uint32_t seqOf(V v) { return (uint32_t) (v >> 32); }
    __device__ static uint32_t lenOf(uint64_t, V v, uint64_t, const TupleGeom &g) { return g.lenArr[(uint32_t) (v >> 32)]; }
    __device__ static uint32_t posOf(uint64_t, V v, uint64_t, const TupleGeom &) { return (uint32_t) v; }
    __device__ static void unpackR1(uint64_t, V v, const TupleGeom &g, uint32_t &len, uint32_t &pos) { pos = (uint32_t) v; len = g.lenArr[(uint32_t) (v >> 32)]; }
};
// 12 bytes: u64 key = k-mer | pos << (2k + 1) | len << (2k + 1 + lb) | strand << 63, u32 value = id.  Needs 2k + 1 + 2 lb <= 63
// (k = 20: sequences up to 2047 letters); a quarter less traffic in every radix pass.  Bit 2k stays clear in every real tuple
// of region 1 (in both layouts): it is set only in the unused-slot key ~0, so sorting region 1 on bits up to and including
// 2k moves the unused slots behind all real tuples.
struct LayoutPacked {
    typedef uint32_t V;
    static constexpr bool bySlot = false;
    __device__ static void store(uint64_t *keys, V *vals, uint64_t slot, uint64_t kmer63, bool fwd, uint32_t seq, uint32_t L, uint32_t pos, const TupleGeom &g) {
        keys[slot] = kmer63 | ((uint64_t) pos << (g.kbits + 1)) | ((uint64_t) L << (g.kbits + 1 + g.lb)) | (fwd ? BIT63 : 0ull); vals[slot] = seq;
    }
    __device__ static void storeHash(uint64_t *keys, V *vals, uint64_t slot, uint64_t hash64, uint32_t seq, uint32_t L, const TupleGeom &g) {
        // region 1 (a hash that fits 2k bits): position 0, length packed above it; region 2: the full hash, length looked up
        keys[slot] = (slot < g.kmerSlots) ? (hash64 | ((uint64_t) L << (g.kbits + 1 + g.lb))) : hash64; vals[slot] = seq;
    }
    __device__ static void storeEmpty(uint64_t *keys, V *vals, uint64_t slot) { keys[slot] = ~0ull; vals[slot] = 0; }
    __device__ static uint64_t kmerOf(uint64_t key, uint64_t slot, const TupleGeom &g) { return slot < g.kmerSlots ? (key & ((1ull << g.kbits) - 1ull)) : (key & ~BIT63); }
    __device__ static uint32_t seqOf(V v) { return v; }
    __device__ static uint32_t lenOf(uint64_t key, V v, uint64_t slot, const TupleGeom &g) { return slot < g.kmerSlots ? (uint32_t) ((key >> (g.kbits + 1 + g.lb)) & ((1ull << g.lb) - 1ull)) : g.lenArr[v]; }
    __device__ static uint32_t posOf(uint64_t key, V, uint64_t slot, const TupleGeom &g) { return slot < g.kmerSlots ? (uint32_t) ((key >> (g.kbits + 1)) & ((1ull << g.lb) - 1ull)) : 0u; }
    __device__ static void unpackR1(uint64_t key, V, const TupleGeom &g, uint32_t &len, uint32_t &pos) {
        const uint32_t t = (uint32_t) (key >> (g.kbits + 1)), m = (1u << g.lb) - 1u;      // 2 lb + 1 <= 63 - 2k - 1 bits are left
        pos = t & m; len = (t >> g.lb) & m;
    }
};
// 8 bytes per tuple through all of sort 1, for DBs whose sequences all have ONE length (uniL letters, uniS = uniL - k + 2 slots each,
// n x uniS < 2^32; k <= 20): the extractor writes only u64 key = k-mer | strand << 63 at the tuple's slot (~0 = empty), and WHICH
// sequence and position a tuple belongs to is the slot's index - slot = seq x uniS + 1 + position in the forward sequence (slot 0 of a
// sequence: its whole-sequence hash tuple, if that fits 2k bits).  The head pass of the sort (radix.h sortSlotKeys) drops the empty
// slots, makes the index explicit and the head digit implicit: the sorted region 1 holds SLOT TUPLES [k-mer bits below headShift | strand
// | slot index].  Wherever a tuple is looked at - the grouping kernel's window, big buckets, the left-over scan - it is first turned into
// the (key, id) pair of LayoutPacked (slotTupleToPair), so everything behind sort 1 is that layout's code.  Region 2 (whole-sequence
// hashes) keeps (key, id) pairs; its values live in an array of their own that `vals` points kmerSlots entries in front of.
struct LayoutSlot {
    typedef uint32_t V;
    static constexpr bool bySlot = true;
    __device__ static void store(uint64_t *keys, V *, uint64_t slot, uint64_t kmer63, bool fwd, uint32_t, uint32_t, uint32_t, const TupleGeom &) { keys[slot] = kmer63 | (fwd ? BIT63 : 0ull); }
    __device__ static void storeHash(uint64_t *keys, V *vals, uint64_t slot, uint64_t hash64, uint32_t seq, uint32_t, const TupleGeom &g) { keys[slot] = hash64; if (slot >= g.kmerSlots) vals[slot] = seq; }
    __device__ static void storeEmpty(uint64_t *keys, V *, uint64_t slot) { keys[slot] = ~0ull; }
    __device__ static uint64_t kmerOf(uint64_t key, uint64_t slot, const TupleGeom &g) { return LayoutPacked::kmerOf(key, slot, g); }
    __device__ static uint32_t seqOf(V v) { return v; }
    __device__ static uint32_t lenOf(uint64_t key, V v, uint64_t slot, const TupleGeom &g) { return LayoutPacked::lenOf(key, v, slot, g); }
    __device__ static uint32_t posOf(uint64_t key, V v, uint64_t slot, const TupleGeom &g) { return LayoutPacked::posOf(key, v, slot, g); }
    __device__ static void unpackR1(uint64_t key, V v, const TupleGeom &g, uint32_t &len, uint32_t &pos) { LayoutPacked::unpackR1(key, v, g, len, pos); }
};
// sequence, stored position (kmermatcher.cpp:186: counted from the other end on the reverse strand) and strand of a slot tuple
// (r: the slot of the sequence, 0 = its whole-sequence hash tuple.  Both positions are computed and one is selected: as branches the
// two cases cost the grouping kernel's member loop an exec save / restore nest per decoded tuple)
__device__ __forceinline__ void slotFields(const TupleGeom &g, uint64_t t8, uint32_t &id, uint32_t &pos, bool &fwd, uint32_t &r) {
    fwd = ((uint32_t) (t8 >> rx::SLOT_STRAND_SHIFT) & 1u) != 0u;
    slotSplit(g, (uint32_t) t8, id, r);
    const uint32_t pf = r - 1u, pr = (g.uniL + 1u - (uint32_t) g.uniK) - r;
    const uint32_t p = fwd ? pf : pr;
    pos = r == 0u ? 0u : p;
}
__device__ __forceinline__ void slotFields(const TupleGeom &g, uint64_t t8, uint32_t &id, uint32_t &pos, bool &fwd) {
    uint32_t r;
    slotFields(g, t8, id, pos, fwd, r);
}
// the slot tuple at k-mer-order index idx (head digit td) as the (key, id) pair LayoutPacked holds
__device__ __forceinline__ void slotTupleToPair(const TupleGeom &g, uint64_t t8, uint32_t td, uint64_t &key, uint32_t &id) {
    static_assert(rx::SLOT_STRAND_SHIFT == 32 && rx::SLOT_KEY_SHIFT == 33, "the tuple's high word is k-mer bits << 1 | strand");
    const uint32_t hiw = (uint32_t) (t8 >> 32);
    const bool fwd = (hiw & 1u) != 0u;
    uint32_t r;
    slotSplit(g, (uint32_t) t8, id, r);
    const uint32_t pos = r == 0u ? 0u : (fwd ? r - 1u : g.uniL - (r - 1u) - (uint32_t) g.uniK);     // (the reverse strand's position, kmermatcher.cpp:186)
    if (g.kbits + 1 >= 32) {
        // the key word by word (64-bit shifts are slow vector instructions, and this runs once per tuple): k-mer = td << headShift | low bits
        const uint32_t lo = (hiw >> 1) | (td << g.headShift);
        const uint32_t hi = (g.headShift ? td >> (32 - g.headShift) : 0u) | (pos << (g.kbits + 1 - 32)) | (g.uniL << (g.kbits + 1 + g.lb - 32)) | (fwd ? 0x80000000u : 0u);
        key = ((uint64_t) hi << 32) | lo;
    } else {
        const uint64_t kmer = ((uint64_t) td << g.headShift) | (uint64_t) (hiw >> 1);
        key = kmer | ((uint64_t) pos << (g.kbits + 1)) | ((uint64_t) g.uniL << (g.kbits + 1 + g.lb)) | (fwd ? BIT63 : 0ull);
    }
}
// ... and back (a tuple that came out of slot 0 - a whole-sequence hash that fits 2k bits, position 0 - gets the slot of position 0 on its
// strand: the index is only ever read through slotTupleToPair, which gives the same pair again)
__device__ __forceinline__ uint64_t pairToSlotTuple(const TupleGeom &g, uint64_t key, uint32_t id) {
    uint32_t len, pos;
    LayoutPacked::unpackR1(key, id, g, len, pos);
    const bool fwd = (key & BIT63) != 0ull;
    const uint32_t slot = id * g.uniS + 1u + (fwd ? pos : g.uniL - pos - (uint32_t) g.uniK);
    return ((key & ((1ull << g.headShift) - 1ull)) << rx::SLOT_KEY_SHIFT) | ((fwd ? 1ull : 0ull) << rx::SLOT_STRAND_SHIFT) | (uint64_t) slot;
}
// what the kernels that look at region 1 IN MEMORY (behind sort 1) go through: the sort bits of the tuple at idx (k-mer + unused-slot bit),
// and the tuple as a (key, value) pair
template <typename LY> __device__ __forceinline__ uint64_t memSortBits(const uint64_t *keys, uint64_t idx, const TupleGeom &g) {
    if constexpr (LY::bySlot) { if (idx < g.kmerSlots) return ((uint64_t) headDigit(g, idx) << g.headShift) | (keys[idx] >> rx::SLOT_KEY_SHIFT); }
    return keys[idx] & ((2ull << g.kbits) - 1ull);
}
template <typename LY> __device__ __forceinline__ void memPair(const uint64_t *keys, const typename LY::V *vals, uint64_t idx, const TupleGeom &g, uint64_t &key, typename LY::V &v) {
    if constexpr (LY::bySlot) { if (idx < g.kmerSlots) { uint32_t id; slotTupleToPair(g, keys[idx], headDigit(g, idx), key, id); v = id; return; } }
    key = keys[idx]; v = vals[idx];
}

}  // namespace
