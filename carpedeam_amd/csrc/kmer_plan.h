// kmermatcher on the device (kmermatch.hip), the plan: which tuple layout a DB takes at each of the three entries, whether its tuples fit
// the device in one pass and, if not, in how many passes over how many blocks, and the cuts of a histogram into ranges of equal shares.
// Plain arithmetic on plain numbers - no HIP, no environment, no device query: the callers read the switches and the device's memory,
// and tests/test_kmer_plan.py compiles this header alone.
#pragma once
#include <cstdint>
#include <cmath>
#include <algorithm>
#include <vector>

namespace kplan {

constexpr int RADIX_BITS = 9, SLOT_REM_BITS = 31;     // radix.h rx::BITS, rx::SLOT_REM (kmermatch.hip asserts that they are)
constexpr uint32_t MAX_SEQ_LETTERS = 1u << 22;        // (diagonals of 24 bits: a tuple position is 32 bits wide, the group key's diagonal field is what bounds it)

// what the plan looks at: sequences, the longest one, Σ lengths, k, and the device's memory in bytes (0: unknown - everything fits)
struct Db { uint64_t n = 0; uint32_t maxLen = 0; uint64_t residues = 0; int k = 0; uint64_t deviceBytes = 0; };
// the values of the switches the layout choice reads
enum class LayoutSwitch { Unset, Wide, Packed, Slot, Other };      // CDM_KMER_LAYOUT
// (... and whether CDM_FORCE_HUGE_LAYOUT, CDM_FORCE_WIDE_KEY, CDM_KMER_SORT, CDM_KMER_PASSES are set)
struct Switches { LayoutSwitch layout = LayoutSwitch::Unset; bool forceHuge = false, forceWideKey = false, kmerSort = false, kmerPasses = false; };
enum class Entry { Single, Part, SplitBegin };         // cdm_kmermatch(_ranks), cdm_kmermatch_part, cdm_kmermatch_split_begin
// (the last four refuse: a sequence of MAX_SEQ_LETTERS or more; the single-device entry's checks of CDM_KMER_LAYOUT)
enum class Layout { Slot, Packed, Wide, Long, Huge, TooLong, BadSwitch, PackedUnfit, SlotUnfit };

inline uint32_t bitsFor(uint64_t v) { uint32_t b = 1; while ((1ull << b) < v) b++; return b; }
inline uint32_t slotsPerSeq(uint32_t L, int k) { return L >= (uint32_t) k ? L - (uint32_t) k + 2u : 1u; }
// LayoutPacked: k-mer, position and length share 63 key bits
inline bool packedLayoutFits(const Db &d) { return 2 * d.k + 1 + 2 * (int) bitsFor((uint64_t) d.maxLen + 1) <= 63; }
// LayoutSlot serves a DB whose sequences all have one length (Σ lengths = n x longest), of at least k letters, with fewer than 2^32 k-mer
// slots, a k-mer of 14 .. 20 letters (the tuple keeps 31 k-mer bits behind the 9-bit head digit) and lengths LayoutPacked's key holds
inline bool slotLayoutFits(const Db &d) {
    if (d.n == 0 || d.residues != d.n * (uint64_t) d.maxLen || d.maxLen < (uint32_t) d.k) return false;
    if (2 * d.k + 1 <= 27 || 2 * d.k - RADIX_BITS > SLOT_REM_BITS) return false;       // (k of 14 .. 20 letters: low bits left to the grouping kernel, at most 31 behind the head digit)
    if (!packedLayoutFits(d)) return false;
    return d.n * (uint64_t) slotsPerSeq(d.maxLen, d.k) < (1ull << 32);
}
// LayoutSlot's split of sort 1: how many of the 2k k-mer bits the global passes leave to the grouping kernel.  The head pass drops the
// empty slots, so every globally sorted bit is a k-mer bit: the head digit and two full passes inside its segments sort 27 of them
// (the 12-byte layouts spend one of their 27 on the unused-slot bit 2k), and a bucket of equal high bits spans half the k-mers.
inline int slotLowBits(int k) { return std::max(0, 2 * k - 3 * RADIX_BITS); }
// ... and what CDM_SLOT_LOWBITS=<n> may ask for instead (A/B runs, tests): at most two passes behind the head digit.  The grouping
// kernel's sort word - 8 bits of bucket ordinal, the n low bits, 9 of position - fits the word chosen for n whatever n that admits:
// 32 bits up to 15 low bits, and n <= 2k - 9 <= 31 keeps 17 + n below 64.  So no n is refused for the word.
constexpr int GROUP_WORD32_LOWBITS = 15;     // (kmermatch.hip groupBuckets: every layout's choice of the word)
static_assert(8 + GROUP_WORD32_LOWBITS + 9 <= 32 && 8 + SLOT_REM_BITS + 9 <= 64, "the grouping kernel's sort word");
inline bool slotLowBitsServed(int k, int n) {
    const int rem = 2 * k - RADIX_BITS - n;
    return n >= 0 && rem >= 0 && rem <= 2 * RADIX_BITS;
}
// bits of a group key below the representative: id, diagonal, strand
inline uint32_t repShiftOf(const Db &d) { return bitsFor(d.n) + bitsFor(2ull * d.maxLen + 2) + 1; }
// does this DB take the wide group key (the representative not in the members' keys)?
inline bool needsWideKey(const Db &d, bool forceWideKey) { return bitsFor(d.n) + repShiftOf(d) > 63 || forceWideKey; }
// do the tuples of one pass (bytesPerSlot for every k-mer slot, both buffers) fit 80 % of the device?
inline bool onePassFits(const Db &d, double bytesPerSlot) {
    const unsigned long long slots = d.residues + 2 * d.n;          // (an upper bound: a slot per k-mer position and two per sequence)
    if (!d.deviceBytes) return true;
    return (double) slots * bytesPerSlot * 1.1 <= 0.80 * (double) d.deviceBytes;
}

// The layout ladder.  Packed 12-byte tuples when they fit, else the 16-byte ones by sequence length and count; in front of them the 8-byte
// slot layout for a DB of one length - on the single-device entry on the default single-pass pipeline only (no A/B sort variant, not over
// ranks, tuples that fit the device at once), on a rank's k-mer range (Part) unless the DB needs the wide key, never for the split by reads.
// CDM_KMER_LAYOUT=wide|packed|slot and CDM_FORCE_HUGE_LAYOUT pin a layout on the single-device entry alone (tests); the other two only
// tell "unset or slot" from anything else.
inline Layout chooseLayout(Entry e, const Db &d, const Switches &sw, bool overRanks = false) {
    const bool single = e == Entry::Single, slotWanted = sw.layout == LayoutSwitch::Unset || sw.layout == LayoutSwitch::Slot;
    if (single && sw.layout == LayoutSwitch::Other) return Layout::BadSwitch;
    if (single && sw.layout == LayoutSwitch::Packed && !packedLayoutFits(d)) return Layout::PackedUnfit;
    if (single && sw.layout == LayoutSwitch::Slot && !slotLayoutFits(d)) return Layout::SlotUnfit;
    const bool slotServes = single ? !overRanks && !sw.kmerSort && !sw.kmerPasses : e == Entry::Part && !needsWideKey(d, sw.forceWideKey);
    if (slotWanted && slotServes && slotLayoutFits(d) && onePassFits(d, 16.0 + 8.0)) return Layout::Slot;
    if (packedLayoutFits(d) && !(single && sw.layout == LayoutSwitch::Wide)) return Layout::Packed;
    const bool huge = single && sw.forceHuge;
    if (d.maxLen < 65535u && !huge) return Layout::Wide;
    if (d.maxLen < (1u << 20) - 1u && d.n < (1ull << 24) && !huge) return Layout::Long;
    if (d.maxLen < MAX_SEQ_LETTERS) return Layout::Huge;       // (CDM_FORCE_HUGE_LAYOUT=1 with CDM_KMER_LAYOUT=wide: this layout for any DB, tests)
    return Layout::TooLong;
}

// One pass while the tuples fit the device: 16 bytes of keys + two values (valBytes each) per k-mer slot, two buffers of each; else P
// passes over the k-mer space, the sequences extracted in B blocks (kmermatchPassesT)
struct PassPlan { int P = 1, B = 1; };
inline PassPlan passPlan(const Db &d, size_t valBytes) {
    PassPlan pl;
    if (onePassFits(d, 16.0 + 2.0 * valBytes)) return pl;
    const double slots = (double) (d.residues + 2 * d.n), room = 0.30 * (double) d.deviceBytes;
    pl.P = (int) std::min(255.0, std::ceil(slots * (16.0 + 2.0 * valBytes + 8.0) / room));
    pl.B = (int) std::ceil(slots * (32.0 + 4.0 * valBytes + 16.0) / room);
    return pl;
}

// Cuts a histogram into at most `parts` ranges of about equal counts, greedily: range r = bins [cut[r], cut[r + 1]), and the last entry
// is `bins`.  A range ends in front of the bin that would take it beyond its share; fewer ranges come out where few bins hold the counts.
inline std::vector<uint32_t> equalShareCuts(const unsigned long long *hist, int bins, int parts) {
    unsigned long long grand = 0, acc = 0;
    for (int b = 0; b < bins; b++) grand += hist[b];
    const unsigned long long target = (grand + (unsigned) parts - 1) / (unsigned) parts;
    std::vector<uint32_t> cut(1, 0u);
    for (int b = 0; b < bins; b++) { if (acc && acc + hist[b] > target && (int) cut.size() < parts) { cut.push_back((uint32_t) b); acc = 0; } acc += hist[b]; }
    cut.push_back((uint32_t) bins);
    return cut;
}

}  // namespace kplan
