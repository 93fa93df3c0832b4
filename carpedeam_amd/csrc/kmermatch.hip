// kmermatcher (linclust-style k-mer matching) on the device, single-split semantics.
//
// Replaces lib/mmseqs/src/linclust/kmermatcher.cpp doComputation (:391-451) and the result writer (:815-930, :717-729):
//   K1 k_seq_hash, k_extract_pair, k_extract_fast, k_extract   fillKmerPositionArray :77-388  per sequence: canonical k-mers, XXH64 16-bit
//                     min-hash, per-sequence ordering by (hash, k-mer, pos) for the repeated-k-mer skipping and the bottom-m
//                     selection, + the whole-sequence hash tuple
//   K2 sort 1         :412   stable sort on the k-mer: the top 27 sort bits by three onesweep radix passes (radix.h), the low bits per
//                     bucket on chip
//   K3 k_bucket_groups (k_groups)   assignGroup :453-562  first sequence of every k-mer run by (length desc, id, pos) is the
//                     representative; members become (rep, id, diagonal, strand); singletons dropped.  Fused with the
//                     on-chip part of sort 1 (bucket.h)
//   K2 sort 2         :431   stable sort on (rep, id, diagonal) packed into one 64-bit key: the k-mer RUNS are sorted by
//                     representative (run records, runsort.h), every representative's tuples then on chip (k_unit_sort)
//   K4 k_seg_count/place   writeKmerMatcherResult :815-930  per (rep, target): shared k-mer count, most frequent diagonal
//                     (last maximum wins), strand of that diagonal's last tuple; every sequence gets a record that starts
//                     with its self hit (fill-in :717-729)
// Quirks kept on purpose (they are observable in the prefilter DB): the repeated-k-mer skip that processes the element
// after a run unconditionally (:277-350); repIsReverse starting as false for the very first k-mer group (:453-467); the
// per-target scan in the writer running on into the next representative's tuples when they have the same target id
// (:875-887).
// The device code lives in the stage headers beside this file: kmer_tuple.h (layouts), kmer_extract.h (K1), kmer_group.h (K3, run records,
// left-over tuples), kmer_vote.h (K4); the layout choice and the pass plan are plain arithmetic in kmer_plan.h.
#include <memory>
#include <cstring>

#include "aggvote.h"
#include "kmer_plan.h"
#include "kmer_tuple.h"
#include "kmer_extract.h"
#include "kmer_group.h"
#include "kmer_vote.h"

namespace {

using rx::DoubleBuf;
using namespace kplan;
static_assert(RADIX_BITS == rx::BITS && SLOT_REM_BITS == rx::SLOT_REM, "kmer_plan.h restates the radix sort's geometry");
// the numbers kmer_plan.h looks at (device: with the device's memory, for the plans that ask whether the tuples fit)
inline uint64_t deviceBytes() { size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) == hipSuccess) return tot; (void) hipGetLastError(); return 0; }
inline Db planDb(const cdm_seqdb *db, int k, bool device = false) { Db d; d.n = db->n; d.maxLen = db->maxLen; d.residues = db->residues; d.k = k; if (device) d.deviceBytes = deviceBytes(); return d; }
// the slot layout's split of sort 1 at this k: kmer_plan.h's, or what CDM_SLOT_LOWBITS=<n> asks for (A/B: 2k + 1 - 27 is the split of
// the rounds before 9) - refused where the passes or the grouping kernel's sort word do not serve it
inline int slotSplit(int k, int &lowBits) {
    lowBits = slotLowBits(k);
    if (const char *e = cdmGetenv("CDM_SLOT_LOWBITS")) {
        char *end = nullptr; const long v = strtol(e, &end, 10);
        if (end == e || *end || v < 0 || v > 64 || !slotLowBitsServed(k, (int) v)) {
            cdm_set_error("cdm_kmermatch: CDM_SLOT_LOWBITS=%s: k = %d takes 0 <= 2k - %d - n <= %d global bits behind the head digit", e, k, RADIX_BITS, 2 * RADIX_BITS); return CDM_ERR_INVALID;
        }
        lowBits = (int) v;
    }
    return CDM_OK;
}

// One kmermatcher run, in phases so that a multi-GPU run can exchange between them (shard.py / cdm_kmermatch_part):
//   phaseA     extraction (of this rank's k-mer range), sort 1, grouping -> group keys in k-mer order (startIo), live, nKept
//   staleTail  the left-over tuples behind global k-mer-order index J (the reference's run-past-the-end scan)
//   phaseB     sort 2 + vote -> prefilter hits
struct KmerJobBase {
    virtual ~KmerJobBase() {}
    virtual int phaseA() = 0;
    virtual int staleTail(unsigned long long J) = 0;
    virtual int phaseB(cdm_hits **out) = 0;
    virtual int gatherByRep() = 0;
    virtual int sortFrom(const uint64_t *devKeys, uint64_t nKeys, uint32_t *head, uint64_t info[2]) = 0;
    virtual int voteWith(const uint32_t *cont, const uint32_t *staleIn, cdm_hits **out) = 0;
    // the split by reads (cdm_kmermatch_split_*): splitBegin = extraction of the owned sequences + the tuples ordered by destination
    // range; splitFinish = sort 1 + grouping on what arrived (region 1: m tuples, region 2: h whole-sequence hash tuples)
    virtual int splitBegin() = 0;
    virtual int splitFinish(const void *keys, const void *vals, uint64_t m, const void *hkeys, const void *hvals, uint64_t h, bool below) = 0;
    bool split = false;
    std::vector<unsigned long long> sendOff;        // [nparts + 1] tuples per destination range, prefix sums
    const void *sendKeys = nullptr, *sendVals = nullptr, *sendHashKeys = nullptr, *sendHashVals = nullptr; unsigned long long sendHash = 0; int valBytes = 0;
    cdm_ctx *ctx = nullptr; const cdm_seqdb *db = nullptr; cdm_kmer_params parCopy; const cdm_kmer_params *par = nullptr;
    int part = 0, nparts = 1;           // this rank's k-mer range (nparts == 1: everything)
    int block = 0, nBlocks = 0;         // splitBegin: block `block` of `nBlocks` of the sequences (0: block `part` of `nparts`), the tuples ordered by nparts ranges
    unsigned long long live = 0, nKept = 0, regionTwo = 0;      // real tuples of region 1 in this range; kept group tuples; real tuples of region 2
    bool anyBelow = false;              // a real tuple with a k-mer below this range exists (then the array's very first run is not here)
    uint64_t *gathered = nullptr;       // gatherByRep: the kept group keys grouped by representative, k-mer order inside (device)
    uint32_t staleHost[64 + 3] = {0};   // staleTail's result: [0] count, [1] sequence id, [2..] positions, [66] = 1 if the scan reached the end of this range's tuples
};
template <typename LY>
struct KmerJob : KmerJobBase {
    typedef typename LY::V V;
    hipStream_t s = nullptr; uint32_t n = 0; int k = 0;
    uint32_t idBits = 0, diagBits = 0; int diagBias = 0; const char *sortEnv = nullptr; bool lsdOnly = false;
    bool wide = false;                        // group keys without the representative (runsort.h RunArgs; packGroupKey)
    bool passes = false;                      // a range of the k-mer-range passes on one device (kmermatchPassesT): no exchange of group keys follows
    uint64_t r2Slots = 0;                     // size of region 2: n (one whole-sequence hash slot per sequence), or what arrived (split by reads)
    uint32_t ordLo = 0, ordHi = 0;            // split by reads: the order ranks of the sequences this rank extracts
    DevBuf<uint64_t> splitK; DevBuf<V> splitV;           // keepOnlyOutgoing: the ordered tuples in buffers of their own size
    DevBuf<unsigned long long> counters;      // scratch counters ([2] = number of kept group tuples)
    DevBuf<unsigned int> cls;                 // slow-path list sizes
    DevBuf<uint32_t> listShort, listLong, listSingle, listHuge;
    DevBuf<unsigned long long> slots; DevBuf<uint64_t> slotOff; DevBuf<uint32_t> rankOf;
    uint64_t kmerSlots = 0; unsigned long long nTuples = 0;
    DoubleBuf<uint64_t> keys; DoubleBuf<V> vals;
    DevBuf<uint64_t> k0, k1; DevBuf<V> v0, v1;
    V *vA = nullptr, *vB = nullptr;           // v0 / v1 as the kernels index them (LayoutSlot: values exist for region 2 only, the pointers stand kmerSlots entries in front of them)
    DevBuf<unsigned long long> segBuf;        // LayoutSlot: where every head digit's slot tuples start (rx::sortSlotKeys)
    TupleGeom geom; int lowBits = 0;
    DevBuf<unsigned long long> headHist; bool headCounted = false;        // LayoutSlot: head digit counts taken by the extraction kernels
    // run records staged by the grouping kernel (BucketGroupArgs::recRep): valid for region 1 when stagedWaves != 0
    DevBuf<uint32_t> stRep, ovRep; DevBuf<uint64_t> stVal, ovVal; DevBuf<uint8_t> stCnt; DevBuf<unsigned long long> recFlag; uint64_t stagedWaves = 0, stagedOwn = 0; unsigned long long ovCap = 0, nOvRec = 0;
    DevBuf<uint32_t> bigRecRep, bigRecRep1; DevBuf<uint64_t> bigRecVal, bigRecVal1; unsigned long long nBigRec = 0;        // ... and the records of the buckets that kernel left to the caller
    bool ownPipeline = false;                 // sortAndGroup runs for the single-device call that also runs sort 2 on its own buffers (phaseA + phaseB)
    // slot layout on a rank (cdm_kmermatch_part for a DB of one read length): the rank extracts every read, the head histogram the
    // extraction counts cuts the 512 head digits into nparts ranges of equal tuple counts (the same cuts on every rank), and the head
    // pass keeps this rank's digits only - what it drops costs a read, not a write
    bool headRange = false; uint32_t headLo = 0, headHi = 0xFFFFFFFFu;
    GroupArgs<LY> ga; DevBuf<unsigned long long> statStripes; unsigned long long *startIo = nullptr; DevBuf<uint32_t> staleBuf;
    DevBuf<uint64_t> runsOut, runsTmp;       // sort 2 "check" mode: the run-based result next to the radix one
    DevBuf<uint64_t> recvA, recvB; DevBuf<uint32_t> contBuf;      // multi-GPU second half: received keys / their sorted form, the continuation list
    const uint64_t *sorted2M = nullptr; unsigned long long nGroupM = 0;
    // the aggregated form of sort 2's result (aggvote.h): entries per representative segment; set when sort2 took that way
    bool haveEntries = false; uint64_t nSegM = 0;
    DevBuf<uint32_t> agSegOfRec, agSegRep, agEntCnt, agPending; DevBuf<unsigned long long> agSegFirstRec, agEntOff, agPerRep, agCursor; DevBuf<aggv::Ent> agEnt; DevBuf<unsigned int> agFlags;
    float msSort1 = 0;
    KmerJob(cdm_ctx *c, const cdm_seqdb *d, const cdm_kmer_params *p) { ctx = c; db = d; parCopy = *p; par = &parCopy; }
// the members every phase reads: stream, sizes, the form of the group key, the scratch counters
int init() {
    s = ctx->stream;
    n = (uint32_t) db->n;
    k = par->kmer_size;
    if (k < 4 || k > 31) { cdm_set_error("cdm_kmermatch: k must be in 4..31 (got %d)", k); return CDM_ERR_INVALID; }
    idBits = bitsFor(n); diagBits = bitsFor(2ull * db->maxLen + 2);
    // (rep, id, diagonal, strand) in one word while it fits 63 bits - 2 M sequences with contigs of 500 k letters, 50 M reads of 2 k
    // letters; beyond that (25 M sequences with contigs: BASELINE config 5) the representative leaves the key (the wide form:
    // runsort.h RunArgs) and sort 2 + vote run on aggregated entries only.  CDM_FORCE_WIDE_KEY=1: the wide form for any DB (tests).
    wide = 2 * idBits + diagBits + 1 > 63 || cdmGetenv("CDM_FORCE_WIDE_KEY") != nullptr;
    if (wide && (int) (aggv::AG_ORD + idBits + diagBits) > 64) {
        cdm_set_error("cdm_kmermatch: %u sequences x max length %u: ids and diagonals beyond %d bits are not implemented", n, db->maxLen, 64 - aggv::AG_ORD); return CDM_ERR_UNSUPPORTED;
    }
    if (wide && nparts > 1 && !passes) { cdm_set_error("cdm_kmermatch_part: %u sequences x max length %u need the wide group key, which the exchange of the k-mer-range split does not carry yet", n, db->maxLen); return CDM_ERR_UNSUPPORTED; }
    diagBias = (int) db->maxLen + 1;
    sortEnv = cdmGetenv("CDM_KMER_SORT");
    lsdOnly = sortEnv && !strcmp(sortEnv, "lsd");
    if (!counters.alloc(8)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
    hipMemsetAsync(counters.p, 0, 8 * 8, s);
    geom.kbits = 2 * k; geom.lb = (int) bitsFor((uint64_t) db->maxLen + 1); geom.lenArr = db->len;
    if constexpr (LY::bySlot) {
        if (!slotLayoutFits(planDb(db, k)) || split || (nparts != 1 && !headRange) || passes || lsdOnly) { cdm_set_error("cdm_kmermatch: internal error: the slot layout was chosen for a run it does not serve"); return CDM_ERR_INVALID; }
        geom.uniL = db->maxLen; geom.uniK = k; geom.uniS = slotsPerSeq(db->maxLen, k); divMagic(geom.uniS, geom.uniMul, geom.uniSh); geom.headShift = 2 * k - std::min(rx::BITS, 2 * k);
    }
    return CDM_OK;
}
int phaseA() override {
    if (int rc = init()) return rc;
    constexpr uint32_t SHORT_CAP = 256, LONG_CAP = 4096;

    if (!cls.alloc(8) || !listShort.alloc(n) || !listLong.alloc(n) || !listSingle.alloc(n) || !listHuge.alloc(n)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
    if (!LY::bySlot && (!slots.alloc((size_t) n + 1) || !slotOff.alloc((size_t) n + 1) || !rankOf.alloc(n))) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
    hipMemsetAsync(cls.p, 0, 8 * 4, s);
    // One slot per k-mer position + one for the whole-sequence tuple, at a fixed offset per sequence (no global counter).
    // Slots are laid out in (sequence length descending, id ascending) order: after the stable k-mer sort the first tuple
    // of every run is then the representative.
    uint64_t capacity = 0;
    if constexpr (LY::bySlot) capacity = (uint64_t) n * geom.uniS;       // one length: that order is the id order, sequence i has the slots from i x uniS on
    else {
        DevBuf<uint32_t> lk0, lk1, lv0, lv1; DevBuf<unsigned long long> ordOff;
        if (!lk0.alloc(n) || !lk1.alloc(n) || !lv0.alloc(n) || !lv1.alloc(n) || !ordOff.alloc((size_t) n + 1)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
        hipLaunchKernelGGL(k_len_keys, dim3((n + 255) / 256), dim3(256), 0, s, db->len, n, db->maxLen, lk0.p, lv0.p);
        const unsigned lenBits = bitsFor((uint64_t) db->maxLen + 2);
        cdmscan::ScanTemp st;
        DoubleBuf<uint32_t> lk(lk0.p, lk1.p), lv(lv0.p, lv1.p);
        if (int rc = rx::sortPairs<uint32_t, uint32_t>(s, ctx->cuCount, lk, lv, (uint64_t) n, 0, (int) lenBits)) return rc;
        hipLaunchKernelGGL(k_slot_counts, dim3((n + 256) / 256), dim3(256), 0, s, db->len, lv.current(), n, k, slots.p);
        if (split) {
            const unsigned blk = nBlocks ? (unsigned) block : (unsigned) part, of = nBlocks ? (unsigned) nBlocks : (unsigned) nparts;      // (the passes on one device cut the sequences into more blocks than the k-mers into ranges)
            DevBuf<uint32_t> cuts; uint32_t hc[2] = {0, 0};
            if (!cuts.alloc(2)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
            cdmscan::ScanTemp stCut;
            if (int rc = cdmscan::exclusiveScan<unsigned long long>(s, stCut, slots.p, ordOff.p, (size_t) n + 1)) return rc;
            hipLaunchKernelGGL(k_block_cuts, dim3(1), dim3(1), 0, s, (const unsigned long long *) ordOff.p, n, blk, of, cuts.p);
            hipMemcpyAsync(hc, cuts.p, 8, hipMemcpyDeviceToHost, s);
            if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: slot layout failed"); return CDM_ERR_HIP; }
            ordLo = hc[0]; ordHi = hc[1];
            hipLaunchKernelGGL(k_slot_mask, dim3((n + 255) / 256), dim3(256), 0, s, slots.p, n, ordLo, ordHi);
        }
        if (int rc = cdmscan::exclusiveScan<unsigned long long>(s, st, slots.p, ordOff.p, (size_t) n + 1)) return rc;
        hipLaunchKernelGGL(k_slot_scatter, dim3((n + 256) / 256), dim3(256), 0, s, lv.current(), ordOff.p, n, slotOff.p, rankOf.p);
        hipMemcpyAsync(&capacity, ordOff.p + n, 8, hipMemcpyDeviceToHost, s);
        if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: slot layout failed"); return CDM_ERR_HIP; }
    }
    kmerSlots = geom.kmerSlots = capacity;           // region 1: k-mer slots (+ slot 0 per sequence)
    r2Slots = split ? (uint64_t) (ordHi - ordLo) : (uint64_t) n;
    capacity += r2Slots;                             // region 2: whole-sequence hash tuples
    nTuples = capacity;

    const uint64_t valSlots = LY::bySlot ? r2Slots : capacity;      // (LayoutSlot: only the whole-sequence hash tuples carry a value)
    if (!k0.alloc(capacity) || !k1.alloc(capacity) || !v0.alloc(valSlots) || !v1.alloc(valSlots)) {
        cdm_set_error("cdm_kmermatch: out of device memory for %llu k-mer tuples (%.1f GB)", (unsigned long long) capacity, (capacity * 16.0 + valSlots * 2.0 * sizeof(V)) / 1e9); return CDM_ERR_HIP;
    }
    vA = LY::bySlot ? v0.p - kmerSlots : v0.p; vB = LY::bySlot ? v1.p - kmerSlots : v1.p;
    ExtractArgs<LY> ea; ea.geom = geom; ea.uniS = geom.uniS;
    ea.woff = db->woff; ea.len = db->len; ea.codes = db->codes; ea.nmask = db->nmask; ea.hasN = db->hasN;
    ea.k = k; ea.kmersPerSeq = par->kmers_per_seq; ea.scale = par->kmers_per_seq_scale; ea.seed = par->hash_shift; ea.ignoreMultiKmer = par->ignore_multi_kmer;
    ea.keys = k0.p; ea.vals = vA; ea.slotOff = slotOff.p; ea.slowShort = listShort.p; ea.slowLong = listLong.p; ea.slowHuge = listHuge.p; ea.slowCnt = cls.p; ea.n = n;
    ea.hugeSp = nullptr; ea.hugeSel = nullptr; ea.hugeCap = 0;
    ea.list = nullptr; ea.nList = 0; ea.hashBase = kmerSlots; ea.rankOf = rankOf.p;
    if constexpr (LY::bySlot) {
        const char *e = cdmGetenv("CDM_SLOT_HIST");        // "kernel": sort 1 counts the head digits itself, with a read of the keys (A/B, tests)
        if (headRange || !(e && !strcmp(e, "kernel"))) {
            if (!headHist.alloc(HEAD_BINS)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
            hipMemsetAsync(headHist.p, 0, HEAD_BINS * 8, s);
            ea.headHist = headHist.p; ea.headShift = geom.headShift; headCounted = true;
        }
    }
    {   // this rank's k-mer range: equal slices of the 2k-bit k-mer space, in k-mer order
        const unsigned __int128 space = (unsigned __int128) 1 << (2 * k);
        ea.kLo = (uint64_t) (space * (unsigned) part / (unsigned) nparts);
        ea.kHi = (part == nparts - 1) ? ~0ull : (uint64_t) (space * (unsigned) (part + 1) / (unsigned) nparts);
        ea.lastPart = (part == nparts - 1) ? 1 : 0; ea.belowFlag = cls.p + 5;
        if (split) { ea.kLo = 0; ea.kHi = ~0ull; ea.lastPart = 1; ea.ordLo = ordLo; ea.ordHi = ordHi; }     // every k-mer of the owned sequences
        if (headRange) { ea.kLo = 0; ea.kHi = ~0ull; }      // (every k-mer: the head pass keeps the rank's range; the whole-sequence hash tuples stay the last rank's)
    }
    hipEventRecord(ctx->ev0, s);
    // A plain uniform DB (common.h MetaUniform: one length, stored back to back, no N) in the slot layout, every k-mer of every read on
    // this device, reads short enough for a half-wave that takes all their k-mers: k_extract_uniform does the work of k_seq_hash and
    // k_extract_pair.  CDM_EXTRACT=pair: those two for every DB (A/B, tests).
    bool uniformKernel = false;
    if constexpr (LY::bySlot) {
        const char *e = cdmGetenv("CDM_EXTRACT");
        const uint32_t L = db->maxLen, W = (L + 15) / 16, nPos = L - (uint32_t) k + 1u;
        const size_t cap = (size_t) (float) ((float) (par->kmers_per_seq - 1) + (par->kmers_per_seq_scale * (float) L));
        if (!(e && !strcmp(e, "pair")) && k <= 30 && ea.kLo == 0 && ea.kHi == ~0ull && ea.ordHi == 0 && ea.lastPart && nPos <= cap && nPos <= (uint32_t) PAIR_POS &&
            db->nCount == 0 && !db->raw && (uint64_t) n * W < (1ull << 32)) {
            unsigned int bad = 1;                  // (cls[6] is zero: the memset above)
            hipLaunchKernelGGL(k_uniform_check, dim3((n + 255) / 256), dim3(256), 0, s, (const uint32_t *) db->len, (const uint32_t *) db->woff, (const uint8_t *) db->hasN, n, L, W, cls.p + 6);
            hipMemcpyAsync(&bad, cls.p + 6, 4, hipMemcpyDeviceToHost, s);
            if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: looking at the sequence lengths failed"); return CDM_ERR_HIP; }
            uniformKernel = bad == 0;
        }
        if (uniformKernel) {
            const uint32_t batches = ((n + 1) / 2 + UNI_BATCH - 1) / UNI_BATCH;
            uint32_t blocks = std::min<uint32_t>((batches + FAST_WAVES - 1) / FAST_WAVES, ctx->cuCount * UNI_MINW);     // (every wave resident at once)
            if (const char *eb = cdmGetenv("CDM_EXTRACT_BLOCKS")) blocks = std::max(1u, std::min<uint32_t>(blocks, (uint32_t) atoi(eb)));      // (tests: several batches per wave on a small DB)
            hipLaunchKernelGGL(k_extract_uniform<LY>, dim3(blocks), dim3(64 * FAST_WAVES), 0, s, ea, L, W);
        }
    }
    ea.single = listSingle.p; ea.listCount = nullptr;
    if (!uniformKernel) {
        hipLaunchKernelGGL(k_seq_hash<LY>, dim3((n + 255) / 256), dim3(256), 0, s, ea);
        if (k <= 30) {      // two short reads per wave; what does not fit comes back through the `single` list
            hipLaunchKernelGGL(k_extract_pair<LY>, dim3(std::min<uint32_t>(((n + 1) / 2 + FAST_WAVES - 1) / FAST_WAVES, ctx->cuCount * 16)), dim3(64 * FAST_WAVES), 0, s, ea);
            ea.list = listSingle.p; ea.listCount = cls.p + 2;
        }
        hipLaunchKernelGGL(k_extract_fast<LY>, dim3(std::min<uint32_t>((n + FAST_WAVES - 1) / FAST_WAVES, ctx->cuCount * 16)), dim3(64 * FAST_WAVES), 0, s, ea);
        ea.listCount = nullptr;
    }
    unsigned int hcls[4] = {0, 0, 0, 0};
    hipMemcpyAsync(hcls, cls.p, 16, hipMemcpyDeviceToHost, s);
    { hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) { cdm_set_error("cdm_kmermatch: extraction failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; } }
    // sequences that need the exact per-sequence ordering (repeated k-mers, more positions than the bottom-m budget)
    auto general = [&](void (*kern)(ExtractArgs<LY>), const uint32_t *list, uint32_t cnt, uint32_t blocks, uint32_t nt) { ea.list = list; ea.nList = cnt; hipLaunchKernelGGL(kern, dim3(blocks), dim3(nt), 0, s, ea); };
    if (hcls[0]) general(k_extract<LY, SHORT_CAP, 64>, listShort.p, hcls[0], std::min<uint32_t>(hcls[0], ctx->cuCount * 32), 64);
    if (hcls[1]) general(k_extract<LY, LONG_CAP, 256>, listLong.p, hcls[1], std::min<uint32_t>(hcls[1], ctx->cuCount * 2), 256);
    DevBuf<SeqPos> hugeSp; DevBuf<uint8_t> hugeSel;
    if (hcls[3]) {
        uint32_t cap = LONG_CAP; while (cap < db->maxLen) cap <<= 1;
        const uint32_t blocks = std::min<uint32_t>(hcls[3], (uint32_t) ctx->cuCount * 4);       // (17 bytes of scratch per record: 2.2 MB per block for 100 k-letter contigs)
        if (!hugeSp.alloc((size_t) blocks * cap) || !hugeSel.alloc((size_t) blocks * cap)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
        ea.hugeSp = hugeSp.p; ea.hugeSel = hugeSel.p; ea.hugeCap = cap;
        general(k_extract<LY, 0, 256>, listHuge.p, hcls[3], blocks, 256);
    }
    hipEventRecord(ctx->ev1, s);
    unsigned int belowHost = 0;
    hipMemcpyAsync(&belowHost, cls.p + 5, 4, hipMemcpyDeviceToHost, s);
    { hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) { cdm_set_error("cdm_kmermatch: extraction (general path) failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; } }
    anyBelow = belowHost != 0;
    hipEventElapsedTime(&ctx->lastMs[3], ctx->ev0, ctx->ev1);
    if (cdmGetenv("CDM_BUCKET_STATS")) fprintf(stderr, "kmermatch extraction (%s): %u sequences through k_extract for a repeated k-mer or a bottom-m selection, %u + %u longer ones\n", uniformKernel ? "uniform kernel" : "pair + fast kernels", hcls[0], hcls[1], hcls[3]);
    if (split) return splitPartition();
    if constexpr (LY::bySlot) if (headRange) {
        unsigned long long hh[HEAD_BINS];
        if (hipMemcpy(hh, headHist.p, sizeof(hh), hipMemcpyDeviceToHost) != hipSuccess) { cdm_set_error("cdm_kmermatch: reading the head histogram failed"); return CDM_ERR_HIP; }
        std::vector<uint32_t> cut = equalShareCuts(hh, HEAD_BINS, nparts);
        cut.resize((size_t) nparts + 1, (uint32_t) HEAD_BINS);      // (fewer ranges than ranks: the last ranks' are empty)
        headLo = cut[part]; headHi = cut[part + 1];
        anyBelow = false; for (uint32_t d = 0; d < headLo; d++) anyBelow = anyBelow || hh[d] != 0;
    }
    return sortAndGroup();
}
// Split by reads, second step: the real tuples of the owned sequences (compacted, still in slot order) ordered by the k-mer range
// they belong to - a stable one-digit radix sort of (range, index) and a gather -, and the real whole-sequence hash tuples, which all go
// to the last range.  What a rank receives, concatenated in rank order, is then in the global slot order: ranks own consecutive blocks
// of that order.
int splitPartition() {
    // ONE radix pass on the top 8 bits of the k-mer and the bit above it (set in unused slots only, which so end up last): the real tuples
    // ordered by CDM_KPART_SLICES = 256 slices of the k-mer space, slot order inside a slice
    DevBuf<unsigned long long> cnt, bounds;
    if (!cnt.alloc(2) || !bounds.alloc((size_t) CDM_KPART_SLICES + 2)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
    unsigned long long m = 0, h = 0;
    const int shift = 2 * k - 8;
    DoubleBuf<uint64_t> ordK(k0.p, k1.p); DoubleBuf<V> ordV(v0.p, v1.p);
    if (kmerSlots) {
        if (int rc = rx::sortPairs<uint64_t, V>(s, ctx->cuCount, ordK, ordV, (uint64_t) kmerSlots, shift, 2 * k + 1)) return rc;
        hipLaunchKernelGGL(k_live_count, dim3(1), dim3(1), 0, s, (const uint64_t *) ordK.current(), (uint64_t) kmerSlots, 2 * k, cnt.p);
        hipMemcpyAsync(&m, cnt.p, 8, hipMemcpyDeviceToHost, s);
    }
    uint64_t *rK = ordK.current(); V *rV = ordV.current();
    // the hash tuples of region 2, compacted (from the extraction buffers into the other pair, behind region 1)
    if (r2Slots) {
        if (int rc = rx::compactPairs<uint64_t, V>(s, k0.p + kmerSlots, v0.p + kmerSlots, (uint64_t) r2Slots, k1.p + kmerSlots, v1.p + kmerSlots, cnt.p + 1)) return rc;
        hipMemcpyAsync(&h, cnt.p + 1, 8, hipMemcpyDeviceToHost, s);
    }
    if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: ordering the tuples by k-mer slice failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP; }
    sendOff.assign((size_t) CDM_KPART_SLICES + 1, 0);
    if (m) {
        hipLaunchKernelGGL(k_slice_bounds, dim3(2), dim3(256), 0, s, (const uint64_t *) rK, (uint64_t) m, shift, (uint32_t) CDM_KPART_SLICES, bounds.p);
        hipMemcpyAsync(sendOff.data(), bounds.p, ((size_t) CDM_KPART_SLICES + 1) * 8, hipMemcpyDeviceToHost, s);
        if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: ordering the tuples by k-mer slice failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP; }
    }
    sendKeys = rK; sendVals = rV; valBytes = (int) sizeof(V);
    sendHashKeys = k1.p + kmerSlots; sendHashVals = v1.p + kmerSlots; sendHash = h;
    return CDM_OK;
}
int splitBegin() override {
    split = true;
    // (which sequences: phaseA's slot layout, blocks of about equal slot counts)
    if (nparts != CDM_KPART_SLICES) { cdm_set_error("cdm_kmermatch: internal error: the split by reads orders its tuples by %d slices", CDM_KPART_SLICES); return CDM_ERR_INVALID; }
    return phaseA();       // (a rank without sequences of its own - fewer sequences than ranks - goes through with empty buffers)
}
// k0 / v0 hold tuples that were not extracted here (m in region 1, h in region 2): sort 1 + grouping on them
int takeOver(uint64_t m, uint64_t h, bool below) { vA = v0.p; vB = v1.p; kmerSlots = m; r2Slots = h; nTuples = m + h; geom.kmerSlots = m; anyBelow = below; return sortAndGroup(); }
void freeExtraction() { slots.free(); slotOff.free(); rankOf.free(); listShort.free(); listLong.free(); listSingle.free(); listHuge.free(); }
int splitFinish(const void *keysIn, const void *valsIn, uint64_t m, const void *hkeys, const void *hvals, uint64_t h, bool below) override {
    // the extraction's buffers go, the received tuples become the two regions of the tuple array
    freeExtraction();
    splitK.free(); splitV.free(); k0.free(); k1.free(); v0.free(); v1.free();        // (sent: the exchange is over)
    DevBuf<uint64_t> nk0, nk1; DevBuf<V> nv0, nv1;
    const uint64_t tot = m + h;
    if (!nk0.alloc(tot) || !nk1.alloc(tot) || !nv0.alloc(tot) || !nv1.alloc(tot)) { cdm_set_error("cdm_kmermatch: out of device memory for %llu received k-mer tuples", (unsigned long long) tot); return CDM_ERR_HIP; }
    if (m) { hipMemcpyAsync(nk0.p, keysIn, m * 8, hipMemcpyDeviceToDevice, s); hipMemcpyAsync(nv0.p, valsIn, m * sizeof(V), hipMemcpyDeviceToDevice, s); }
    if (h) { hipMemcpyAsync(nk0.p + m, hkeys, h * 8, hipMemcpyDeviceToDevice, s); hipMemcpyAsync(nv0.p + m, hvals, h * sizeof(V), hipMemcpyDeviceToDevice, s); }
    if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: taking over the received tuples failed"); return CDM_ERR_HIP; }
    k0.p = nk0.release(); k1.p = nk1.release(); v0.p = nv0.release(); v1.p = nv1.release();
    return takeOver(m, h, below);
}
// after splitBegin: everything goes but what would be sent - the tuples ordered by range (splitK / splitV) and the hash tuples, which
// move out of the extraction buffers into two small ones
int keepOnlyOutgoing() {
    DevBuf<uint64_t> hk; DevBuf<V> hv;
    const unsigned long long m = sendOff.empty() ? 0 : sendOff.back();
    if (!hk.alloc(sendHash) || !hv.alloc(sendHash) || !splitK.alloc(m) || !splitV.alloc(m)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
    if (m) { hipMemcpyAsync(splitK.p, sendKeys, m * 8, hipMemcpyDeviceToDevice, s); hipMemcpyAsync(splitV.p, sendVals, m * sizeof(V), hipMemcpyDeviceToDevice, s); }
    if (sendHash) { hipMemcpyAsync(hk.p, sendHashKeys, sendHash * 8, hipMemcpyDeviceToDevice, s); hipMemcpyAsync(hv.p, sendHashVals, sendHash * sizeof(V), hipMemcpyDeviceToDevice, s); }
    if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: keeping a block's tuples failed"); return CDM_ERR_HIP; }
    k0.free(); k1.free(); v0.free(); v1.free();
    sendKeys = splitK.p; sendVals = splitV.p;
    freeExtraction(); cls.free(); counters.free();
    sendHashKeys = keptHashK.p = hk.release(); sendHashVals = keptHashV.p = hv.release();
    return CDM_OK;
}
DevBuf<uint64_t> keptHashK; DevBuf<V> keptHashV;
// a range of the passes on one device: its tuples, gathered by the caller (m k-mer tuples, then h whole-sequence hash tuples), are
// taken over as they are
int rangeFinishOwned(DevBuf<uint64_t> &keysBuf, DevBuf<V> &valsBuf, uint64_t m, uint64_t h, bool below) {
    passes = true; split = true;
    if (int rc = init()) return rc;
    const uint64_t tot = m + h;
    if (!k1.alloc(tot) || !v1.alloc(tot)) { cdm_set_error("cdm_kmermatch: out of device memory for a pass over %llu k-mer tuples", (unsigned long long) tot); return CDM_ERR_HIP; }
    k0.p = keysBuf.release(); v0.p = valsBuf.release();
    return takeOver(m, h, below);
}
// sort 1 + grouping of the tuple array (k0 / vA: region 1 = kmerSlots k-mer slots, region 2 = r2Slots whole-sequence hash tuples) ->
// group keys in k-mer order (startIo), live, nKept, regionTwo
int sortAndGroup() {
    // ---- sort 1: stable LSD radix sort by k-mer.  Region 1 (k-mer slots) on the 2k key bits, region 2 (whole-sequence hashes)
    // on 63 bits into the same physical buffers; the strand bit 63 rides along outside the sorted bit range.
    keys = DoubleBuf<uint64_t>(k0.p, k1.p); vals = DoubleBuf<V>(vA, vB);
    // Region 1: only the top 27 sort bits go through global passes, the low bits are finished per bucket by k_bucket_groups
    // (bucket.h); CDM_KMER_SORT=lsd sorts all 2k bits globally and keeps the separate scan + k_groups kernels (A/B).
    // With low bits left over the passes cover bits [lowBits, 2k]: bit 2k is set only in unused slots, which end up last.
    // 27 high bits = 3 onesweep passes of 9 bits (library radix sorts default to 8 bits per pass; 9 still fits the LDS and three
    // 9-bit passes take 29 ms per 2^30 tuples where four 8-bit ones take 35).
    // The slot layout's head pass drops the unused slots: its 27 bits are all k-mer bits (slotLowBits, kmer_plan.h; CDM_SLOT_LOWBITS).
    lowBits = lsdOnly ? 0 : std::max(0, 2 * k + 1 - 27);
    if constexpr (LY::bySlot) if (int rc = slotSplit(k, lowBits)) return rc;
    hipEventRecord(ctx->ev0, s);
    if (int rc = sortRegionOne()) return rc;
    hipEventRecord(ctx->ev1, s);
    hipEventRecord(ctx->ev2, s);
    if (int rc = sortRegionTwo()) return rc;
    hipEventRecord(ctx->ev3, s);
    // ---- K3: group keys per slot (fused bucket kernel for region 1, run-start max-scan + k_groups elsewhere), then the
    // order-preserving compaction
    ga.geom = geom;
    ga.keys = keys.current(); ga.vals = vals.current(); ga.n = nTuples; ga.onlyExtendable = par->include_only_extendable; ga.covMode = par->cov_mode;
    ga.covThr = par->cov_thr; ga.idBits = idBits; ga.diagBits = diagBits; ga.diagBias = diagBias; ga.first = 0; ga.wide = wide ? 1 : 0;
    ga.firstRunIdx = (anyBelow || (split && kmerSlots == 0)) ? ~0ull : 0ull;      // (split with nothing in region 1: index 0 is a hash tuple, which is never the first run)
    // the very first run of the (global) array is in the lowest k-mer range that has tuples
    if (!statStripes.alloc(STAT_STRIPES)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
    hipMemsetAsync(statStripes.p, 0, STAT_STRIPES * 8, s);
    ga.stat = statStripes.p;
    startIo = (unsigned long long *) keys.alternate();   // free after the sort
    if (!LY::bySlot) live = 0;
    nKept = 0;
    if (!staleBuf.alloc(STALE_MAX + 3)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
    hipMemsetAsync(staleBuf.p, 0, (STALE_MAX + 3) * 4, s);
    if (kmerSlots && !LY::bySlot) {        // real tuples of region 1 (the unused slots sort behind them in both variants)
        hipLaunchKernelGGL(k_live_count, dim3(1), dim3(1), 0, s, ga.keys, (uint64_t) kmerSlots, 2 * k, counters.p + 3);
        hipMemcpyAsync(&live, counters.p + 3, 8, hipMemcpyDeviceToHost, s);
        if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: grouping failed"); return CDM_ERR_HIP; }
    }
    if (lowBits == 0) { if (scanGroups(ga, startIo) != CDM_OK) return groupingFailed(); }
    else if (int rc = groupBuckets()) return rc;
    return countKept();
}
int groupingFailed() { cdm_set_error("cdm_kmermatch: grouping failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP; }
// sort 1, region 1: keys / vals point at the result (LayoutSlot: and `live` is known)
int sortRegionOne() {
    const int sortTop = lowBits ? 2 * k + 1 : 2 * k;
    if constexpr (LY::bySlot) {
        // one length, 8-byte tuples: the head pass drops the empty slots and writes slot tuples, the other global passes run inside the
        // head digit's segments (rx::sortSlotKeys); `live` comes out of the head histogram
        if (!segBuf.alloc(rx::BINS + 1)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
        uint64_t *res = nullptr; unsigned long long liveSlots = 0;
        if (int rc = rx::sortSlotKeys(s, ctx->cuCount, k0.p, k1.p, (uint64_t) kmerSlots, 2 * k, lowBits, headCounted ? headHist.p : nullptr, segBuf.p, liveSlots, res, &ctx->lastMs[13], &ctx->lastMs[14],
                                      headRange ? headLo : 0u, headRange ? std::min<uint32_t>(headHi, (uint32_t) rx::BINS) : (uint32_t) rx::BINS)) return rc;
        keys = DoubleBuf<uint64_t>(res, res == k0.p ? k1.p : k0.p); vals = res == k0.p ? DoubleBuf<V>(vA, vB) : DoubleBuf<V>(vB, vA);     // (region 2's values follow its keys' buffer)
        // what those launches move at the least, in GB: the head pass reads every slot's key and writes the real ones' tuples, the passes
        // inside the segments read and write every tuple (bench.py's roofline figure)
        ctx->lastMs[15] = (float) (((double) kmerSlots * 8.0 + (double) liveSlots * 8.0 + (double) (ctx->lastMs[14] - 1.f) * (double) liveSlots * 16.0) / 1e9);
        live = liveSlots; geom.seg = segBuf.p;
        return CDM_OK;
    }
    uint64_t sorted = kmerSlots;        // the tuples the passes run over
    const bool range = nparts > 1 && kmerSlots && !lsdOnly && !split;      // (split by reads: what arrived has no empty slots)
    DevBuf<unsigned long long> cnt;     // (lives until the passes are through, as the allocations' order has it)
    if (range) {
        // a k-mer RANGE: most slots are empty.  The real tuples are compacted (stable) into the other buffers first, so that the
        // passes run over this rank's share only; behind them the result holds empty slots again, as if all had been sorted.
        if (!cnt.alloc(1)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
        if (int rc = rx::compactPairs<uint64_t, V>(s, k0.p, vA, (uint64_t) kmerSlots, k1.p, vB, cnt.p)) return rc;
        unsigned long long m = 0;
        hipMemcpyAsync(&m, cnt.p, 8, hipMemcpyDeviceToHost, s);
        if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: compaction failed"); return CDM_ERR_HIP; }
        keys = DoubleBuf<uint64_t>(k1.p, k0.p); vals = DoubleBuf<V>(vB, vA); sorted = m;
    }
    if (int rc = rx::sortPairs<uint64_t, V>(s, ctx->cuCount, keys, vals, sorted, lowBits, sortTop, &ctx->lastMs[13])) return rc;
    ctx->lastMs[14] = (float) ((sortTop - lowBits + rx::BITS - 1) / rx::BITS);     // its launches
    ctx->lastMs[15] = (float) ((double) ctx->lastMs[14] * (double) sorted * 2.0 * (8.0 + sizeof(V)) / 1e9);
    if (range) hipMemsetAsync(keys.current() + sorted, 0xFF, (size_t) (kmerSlots - sorted) * 8, s);        // (the values of empty slots are never read)
    return CDM_OK;
}
// sort 1, region 2: it goes to wherever region 1 ended up (the input is always the extraction buffers k0/v0)
int sortRegionTwo() {
    DoubleBuf<uint64_t> rk(k0.p + kmerSlots, k1.p + kmerSlots); DoubleBuf<V> rv(vA + kmerSlots, vB + kmerSlots);
    if (int rc = rx::sortPairs<uint64_t, V>(s, ctx->cuCount, rk, rv, (uint64_t) r2Slots, 0, 63)) return rc;
    uint64_t *kOut = keys.current() + kmerSlots; V *vOut = vals.current() + kmerSlots;
    if (rk.current() != kOut && r2Slots) { hipMemcpyAsync(kOut, rk.current(), (size_t) r2Slots * 8, hipMemcpyDeviceToDevice, s); hipMemcpyAsync(vOut, rv.current(), (size_t) r2Slots * sizeof(V), hipMemcpyDeviceToDevice, s); }
    return CDM_OK;
}
// scan + k_groups over the tuples [first, last) of (kk, vv), group keys to io[first..last)
int scanGroups(GroupArgs<LY> g, unsigned long long *io) {
    const size_t cnt = (size_t) (g.n - g.first);
    if (cnt == 0) return CDM_OK;
    cdmscan::ScanTemp t;                                                  // alive until the synchronise below
    if (int rc = cdmscan::inclusiveMaxScanFn(s, t, StartFrom<LY>{StartIndex<LY>{g.keys, g.geom, (unsigned long long) g.first}}, io + g.first, cnt)) return rc;
    if (cnt > CDM_MAX_LAUNCH_THREADS - 256) { cdm_set_error("cdm_kmermatch: %zu tuples in one grouping launch (CDM_KMER_SORT=lsd takes fewer than 2^32)", cnt); return CDM_ERR_UNSUPPORTED; }
    hipLaunchKernelGGL(k_groups<LY>, CDM_GRID((cnt + 255) / 256, 256), dim3(256), 0, s, g, io);
    return hipStreamSynchronize(s) == hipSuccess ? CDM_OK : CDM_ERR_HIP;
}
// the fused grouping launch over region 1 (W: the word of its sorting network), with the stages for sort 2's run records where they
// are taken; false: out of device memory (error set)
template <typename W>
bool launchFused(int own, uint32_t maxBucket, DevBuf<unsigned long long> &bigList, DevBuf<unsigned int> &bigCnt, DevBuf<BlockHead> &heads) {
    BucketGroupArgs<LY, W> ba;
    static_cast<GroupParams &>(ba) = ga; ba.n = live;
    ba.keys = ga.keys; ba.vals = ga.vals; ba.geom = geom; ba.out = startIo; ba.lowBits = lowBits; ba.own = own; ba.maxBucket = maxBucket;
    ba.big.list = bigList.p; ba.big.cnt = bigCnt.p;
    const uint64_t perBlock = (uint64_t) own * bucket::BK_WAVES;
    // the run records of sort 2 come out of this kernel (on the default single-device pipeline; CDM_RUN_RECORDS=kernel|twopass: from
    // the key array, as before round 5)
    stagedWaves = 0;
    if (LY::bySlot && (ownPipeline || headRange) && live && !cdmGetenv("CDM_RUN_RECORDS") && !cdmGetenv("CDM_RUN_CAP")) {
        const uint64_t waves = (live + (uint64_t) own - 1) / (uint64_t) own;
        ovCap = live / 256 + 4096;
        if (stRep.alloc(waves * REC_CAP) && stVal.alloc(waves * REC_CAP) && stCnt.alloc(waves + 1) && recFlag.alloc(2) && ovRep.alloc(ovCap) && ovVal.alloc(ovCap)) {
            hipMemsetAsync(stCnt.p, 0, waves + 1, s); hipMemsetAsync(recFlag.p, 0, 8, s);
            ba.recRep = stRep.p; ba.recVal = stVal.p; ba.recCnt = stCnt.p; stagedWaves = waves; stagedOwn = (uint64_t) own; nBigRec = 0;
            ba.ovRep = ovRep.p; ba.ovVal = ovVal.p; ba.ovCursor = recFlag.p; ba.ovCap = ovCap;
            if (const char *e = cdmGetenv("CDM_REC_LIMIT")) { const long v = atol(e); if (v >= 0 && v <= REC_CAP) ba.recLimit = (uint32_t) v; }
        } else { dropStages(); (void) hipGetLastError(); }      // (no room: the records come from the key array)
    }
    if constexpr (LY::bySlot) {
        const uint64_t blocks = (live + perBlock - 1) / perBlock;
        if (!heads.alloc(blocks)) { cdm_set_error("cdm_kmermatch: out of device memory"); return false; }
        if (blocks) hipLaunchKernelGGL(k_block_heads, CDM_GRID((blocks + 255) / 256, 256), dim3(256), 0, s, geom, (uint64_t) live, perBlock, blocks, heads.p);
        ba.blockHead = heads.p;
    }
    if (live) hipLaunchKernelGGL((k_bucket_groups<LY, W>), dim3((unsigned) ((live + perBlock - 1) / perBlock)), dim3(bucket::BK_NT), cdm_lds_pad("CDM_LDS_PAD_GROUPS"), s, ba);
    return true;
}
void dropStages() { stagedWaves = 0; stRep.free(); stVal.free(); stCnt.free(); ovRep.free(); ovVal.free(); }
// K3 where low bits are left over: the fused kernel over region 1, scan + k_groups over region 2, then the buckets that kernel left alone
int groupBuckets() {
    int own; uint32_t maxBucket; bucket::capacities(own, maxBucket);
    own = std::min(own, GkGeom<LY>::OWN); maxBucket = std::min<uint32_t>(maxBucket, (uint32_t) GkGeom<LY>::MAXB);
    DevBuf<unsigned long long> bigList; DevBuf<unsigned int> bigCnt;
    if (!bigList.alloc(bucket::bigListSlots(kmerSlots, maxBucket)) || !bigCnt.alloc(1)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
    hipMemsetAsync(bigCnt.p, 0, 4, s);
    if (kmerSlots) hipMemsetAsync(startIo + live, 0xFF, (size_t) (kmerSlots - live) * 8, s);     // unused slots: no group key
    DevBuf<BlockHead> heads;        // (freed behind the synchronise below)
    // 8 bits of bucket ordinal + low bits + 9 of position in one word
    if (!(lowBits <= GROUP_WORD32_LOWBITS ? launchFused<uint32_t>(own, maxBucket, bigList, bigCnt, heads) : launchFused<uint64_t>(own, maxBucket, bigList, bigCnt, heads))) return CDM_ERR_HIP;
    unsigned int nBig = 0; unsigned long long recOver = 0;
    hipMemcpyAsync(&nBig, bigCnt.p, 4, hipMemcpyDeviceToHost, s);
    if (stagedWaves) hipMemcpyAsync(&recOver, recFlag.p, 8, hipMemcpyDeviceToHost, s);
    GroupArgs<LY> g2 = ga; g2.first = kmerSlots;                      // region 2 is sorted on all its bits
    int rc = scanGroups(g2, startIo);
    nOvRec = recOver;
    if (stagedWaves && recOver > ovCap) dropStages();     // (more records beyond the waves' stages than their list holds: from the key array after all)
    if (rc == CDM_OK && nBig) rc = groupBigBuckets(bigList, nBig);
    return rc == CDM_OK ? CDM_OK : groupingFailed();
}
// the tuples of the listed buckets as (key, value) pairs into the dense arrays (GATHER), or back from them
template <bool GATHER> void bigBucketPairs(unsigned int grid, const unsigned long long *ranges, unsigned int nBig, uint64_t *dk, V *dv) {
    if constexpr (LY::bySlot) hipLaunchKernelGGL(k_big_slot_pairs<GATHER>, dim3(grid), dim3(256), 0, s, ranges, nBig, const_cast<uint64_t *>(ga.keys), geom, dk, dv);
    else {
        hipLaunchKernelGGL((bucket::k_big_copy<uint64_t, GATHER>), dim3(grid), dim3(256), 0, s, ranges, nBig, const_cast<uint64_t *>(ga.keys), dk);
        hipLaunchKernelGGL((bucket::k_big_copy<V, GATHER>), dim3(grid), dim3(256), 0, s, ranges, nBig, const_cast<V *>(ga.vals), dv);
    }
}
// buckets the kernel left alone: gather them, sort on the whole k-mer, group, scatter the group keys back
int groupBigBuckets(DevBuf<unsigned long long> &bigList, unsigned int nBig) {
    DevBuf<unsigned long long> ranges; uint64_t total = 0; unsigned long long firstStart = ~0ull;
    int rc = bucket::loadBigList(s, bigList.p, nBig, ranges, total, &firstStart);
    if (cdmGetenv("CDM_BUCKET_STATS")) fprintf(stderr, "kmermatch sort 1: %llu slots, low bits %d: %u big buckets, %llu tuples\n", (unsigned long long) kmerSlots, lowBits, nBig, (unsigned long long) total);
    DevBuf<uint64_t> dk0, dk1; DevBuf<V> dv0, dv1; DevBuf<unsigned long long> ds;
    if (rc == CDM_OK && (!dk0.alloc(total) || !dk1.alloc(total) || !dv0.alloc(total) || !dv1.alloc(total) || !ds.alloc(total))) rc = CDM_ERR_HIP;
    if (rc != CDM_OK) return rc;
    const unsigned int grid = bucket::bigCopyGrid(nBig);
    bigBucketPairs<true>(grid, ranges.p, nBig, dk0.p, dv0.p);
    DoubleBuf<uint64_t> dk(dk0.p, dk1.p); DoubleBuf<V> dv(dv0.p, dv1.p);
    if (int rc2 = rx::sortPairs<uint64_t, V>(s, ctx->cuCount, dk, dv, (uint64_t) total, 0, 2 * k)) return rc2;
    // the sorted tuples go back in place too: k_stale_tail indexes big buckets directly
    bigBucketPairs<false>(grid, ranges.p, nBig, dk.current(), dv.current());
    GroupArgs<LY> gd = ga; gd.keys = dk.current(); gd.vals = dv.current(); gd.n = total; gd.first = 0;
    gd.geom.kmerSlots = ~0ull;                                   // every tuple of the dense view is a region-1 tuple
    gd.firstRunIdx = (firstStart == 0 && !anyBelow) ? 0ull : ~0ull;           // dense index 0 is the array's first tuple only then
    if (int rc2 = scanGroups(gd, ds.p)) return rc2;
    hipLaunchKernelGGL((bucket::k_big_copy<unsigned long long, false>), dim3(grid), dim3(256), 0, s, (const unsigned long long *) ranges.p, nBig, startIo, ds.p);
    if (hipStreamSynchronize(s) != hipSuccess) return CDM_ERR_HIP;
    if (stagedWaves) {
        // the run records of these buckets (the kernel staged none for them): from their group keys, a dropped key between
        // two buckets, the starts put back into the key array's coordinates
        DevBuf<unsigned long long> gapped;
        if (!gapped.alloc(total + nBig)) return CDM_ERR_HIP;
        hipLaunchKernelGGL(k_big_gap_copy, dim3(grid), dim3(256), 0, s, (const unsigned long long *) ranges.p, nBig, (const unsigned long long *) ds.p, gapped.p);
        runsort::RunArgs ra = runArgs((const uint64_t *) gapped.p, total + nBig, 0, 0);
        rc = runsort::makeRunRecords(s, ra, bigRecRep, bigRecRep1, bigRecVal, bigRecVal1, nBigRec);
        if (rc == CDM_OK && nBigRec) hipLaunchKernelGGL(k_big_rec_starts, CDM_GRID((nBigRec + 255) / 256, 256), dim3(256), 0, s, (const unsigned long long *) ranges.p, nBig, bigRecVal.p, (uint64_t) nBigRec);
        if (rc == CDM_OK && hipStreamSynchronize(s) != hipSuccess) rc = CDM_ERR_HIP;
        bigRecRep1.free(); bigRecVal1.free();
    }
    return rc;
}
// the counts behind the grouping: kept group tuples, and a multi-range run's real whole-sequence hash tuples
int countKept() {
    hipLaunchKernelGGL(k_reduce_stats, dim3(1), dim3(256), 0, s, (const unsigned long long *) statStripes.p, counters.p + 4);
    hipMemcpyAsync(&nKept, counters.p + 4, 8, hipMemcpyDeviceToHost, s);
    { hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) { cdm_set_error("cdm_kmermatch: grouping failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; } }
    hipEventElapsedTime(&msSort1, ctx->ev0, ctx->ev1);
    regionTwo = 0;
    if (nparts > 1 && part == nparts - 1 && r2Slots) {        // real whole-sequence hash tuples (they sort in front of the empty slots of region 2)
        hipLaunchKernelGGL(k_count_hash_tuples, dim3(1), dim3(1), 0, s, (const uint64_t *) ga.keys + kmerSlots, (uint64_t) r2Slots, counters.p + 6);
        hipMemcpyAsync(&regionTwo, counters.p + 6, 8, hipMemcpyDeviceToHost, s);
        if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: grouping failed"); return CDM_ERR_HIP; }
    }
    return CDM_OK;
}
// the run records' view of a group-key array (runsort.h)
runsort::RunArgs runArgs(const uint64_t *gk, unsigned long long nIn, unsigned long long skipLo, unsigned long long skipHi) const {
    runsort::RunArgs ra; ra.keys = gk; ra.n = nIn; ra.skipLo = skipLo; ra.skipHi = skipHi; ra.repShift = (int) (idBits + diagBits + 1);
    ra.wide = wide ? 1 : 0; ra.idShift = (int) diagBits + 1; ra.idMask = (1ull << idBits) - 1ull;
    return ra;
}
// The tuples behind the kept ones that the reference's last per-target scan may run into (VoteArgs, k_stale_tail): the real
// tuples of this range from k-mer-order index J on (0: from the range's first tuple, for a scan that comes in from the range in
// front), while they belong to one sequence.  Result in staleBuf (device) and staleHost.
int staleTail(unsigned long long J) override {
    memset(staleHost, 0, sizeof(staleHost));
    hipMemsetAsync(staleBuf.p, 0, (STALE_MAX + 3) * 4, s);
    const unsigned long long realTuples = live + regionTwo;       // (regionTwo is only counted for multi-range runs)
    if (nparts > 1 && J >= realTuples) { staleHost[STALE_MAX + 4] = 1; return hipStreamSynchronize(s) == hipSuccess ? CDM_OK : CDM_ERR_HIP; }
    StaleArgs<LY> sa;
    sa.keys = ga.keys; sa.vals = ga.vals; sa.geom = geom; sa.live = live; sa.kmerSlots = kmerSlots; sa.nTuples = nTuples; sa.J = J;
    sa.lowBits = lowBits; sa.sorted = (lowBits == 0); sa.out = staleBuf.p;
    hipLaunchKernelGGL(k_stale_tail<LY>, dim3(1), dim3(256), 0, s, sa);
    hipMemcpyAsync(staleHost, staleBuf.p, (STALE_MAX + 3) * 4, hipMemcpyDeviceToHost, s);
    if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: grouping failed"); return CDM_ERR_HIP; }
    if (staleHost[0] >= (uint32_t) STALE_MAX) {
        cdm_set_error("cdm_kmermatch: the reference's last per-target scan could run over %d or more left-over tuples of one sequence; not reproduced on the device", STALE_MAX);
        return CDM_ERR_UNSUPPORTED;
    }
    staleHost[STALE_MAX + 4] = (J + staleHost[0] >= realTuples) ? 1u : 0u;     // the scan consumed every tuple up to the end of this range
    return CDM_OK;
}
int phaseB(cdm_hits **out) override {
    if (int rc = sort2((const uint64_t *) startIo, nTuples, live, kmerSlots, keys.current(), (uint64_t *) startIo, true)) return rc;
    return vote(nullptr, true, out);
}
// kept group keys of [keysIn, keysIn + nIn) (~0 = dropped; [skipLo, skipHi) holds only ~0) -> sort 2 -> vote -> hits.
// bufA / bufB: two buffers of nIn keys (bufB may be keysIn itself).
int sort2(const uint64_t *keysIn, unsigned long long nIn, unsigned long long skipLo, unsigned long long skipHi, uint64_t *bufA, uint64_t *bufB, bool ownBuffers) {

    // ---- sort 2: by (rep, id, diagonal) = key bits 1.., stable; strand bit 0 rides along.
    // Default ("runs", runsort.h): the k-mer runs are sorted by representative, not the tuples - records of (rep, start, length),
    // a stable radix sort of those, an expanding gather that also drops the ~0 keys, then a segmented sort of every
    // representative's tuples on (id, diagonal) on chip.
    // CDM_KMER_SORT2=radix (A/B; also what CDM_KMER_SORT=lsd uses): no compaction, dropped members carry the key ~0, and bit top2
    // (the first bit above the key fields) is set only there, so sorting on bits up to and including top2 moves them behind all
    // kept members; the top 32 of those bits go through global radix passes, the rest is finished bucket by bucket on chip
    // (bucket.h).  CDM_KMER_SORT2=check runs both and compares the two arrays on the device.
    if (ownBuffers) { v0.free(); v1.free(); }                                // the tuple values are dead after k_groups
    const int top2 = (int) ((wide ? idBits : 2 * idBits) + diagBits + 1);
    const char *sort2Env = cdmGetenv("CDM_KMER_SORT2");
    const bool sort2Check = sort2Env && !strcmp(sort2Env, "check");
    const bool sort2Runs = !lsdOnly && (!sort2Env || !strcmp(sort2Env, "runs") || sort2Check);
    if (wide && (!sort2Runs || sort2Check || !ownBuffers)) { cdm_set_error("cdm_kmermatch: the wide group key runs on the default pipeline only (run records + aggregated entries)"); return CDM_ERR_UNSUPPORTED; }
    if (sort2Env && strcmp(sort2Env, "runs") && strcmp(sort2Env, "radix") && !sort2Check) { cdm_set_error("cdm_kmermatch: CDM_KMER_SORT2 must be runs, radix or check"); return CDM_ERR_INVALID; }
    unsigned long long nGroup = 0;
    const uint64_t *sorted2 = nullptr;
    hipEventRecord(ctx->ev0, s);
    if (sort2Runs) {
        using namespace runsort;
        const uint64_t *gk = keysIn;
        // the sorters read the records' tuples from keysIn while they write: the sorted array goes to the OTHER buffer (bufB may be
        // keysIn); the few segments no unit holds are expanded into their final place first and sorted there
        uint64_t *sortedOut = bufA;
        if (sort2Check) {
            if (!runsOut.alloc(nIn)) { cdm_set_error("cdm_kmermatch: out of device memory (sort 2 check)"); return CDM_ERR_HIP; }
            sortedOut = runsOut.p;
        }
        const RunArgs ra = runArgs(gk, nIn, skipLo, skipHi);
        const bool fromStage = stagedWaves && ownBuffers && keysIn == (const uint64_t *) startIo;
        RepRecords R;
        if (int rc = recordsByRep(ra, fromStage, true, R, nGroup)) return rc;
        const unsigned long long nRec = R.nRec; const DoubleBuf<uint32_t> &rk = R.rep; const DoubleBuf<uint64_t> &rv = R.val; DevBuf<unsigned long long> &dst = R.dst;
        if (nRec) {
            // (the expansion of the records - k_run_gather - is not run as a pass of its own: the unit sorter expands its records
            // into LDS, the few longer segments are expanded on demand)
            if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: sort 2 (records) failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP; }
            // Default on one device: the representatives' tuples are aggregated, not sorted (aggvote.h).  The tuple path below stays for
            // the multi-GPU split (its ranks exchange heads of the sorted array), for keys too wide for the aggregation's sort word,
            // under CDM_KMER_VOTE=tuples, and as the fallback when the entry buffer overflows.
            const char *voteEnv = cdmGetenv("CDM_KMER_VOTE");
            const bool wordFits = aggv::AG_ORD + idBits + diagBits + aggv::AG_IDX <= 64 && !(wide && cdmGetenv("CDM_FORCE_WIDE_WORD"));    // (tests: the 128-bit entry sort word for any DB)
            // (a rank's second half - sortFrom, !ownBuffers - aggregates as well since round 5: the heads the ranks exchange and the continuation
            //  of a rank's last scan are expressed on entries, aggvote.h k_head_entries / VoteEntArgs::cont; CDM_DIST_VOTE=tuples keeps the tuple path)
            const char *distVote = cdmGetenv("CDM_DIST_VOTE");
            bool aggregated = wide || ((ownBuffers || !(distVote && !strcmp(distVote, "tuples"))) && !sort2Check && !(voteEnv && !strcmp(voteEnv, "tuples")) && wordFits);
            if ((wide || fromStage) && ownBuffers && nGroup != nKept) { cdm_set_error("cdm_kmermatch: internal error: %llu group tuples counted, %llu in the run records", nKept, nGroup); return CDM_ERR_HIP; }
            if (aggregated) {
                // (the wide form has no tuple path to fall back to: an entry buffer that proves too small is tried again, larger)
                const unsigned long long slack = aggv::aggChunkSlack(nGroup / runsort::U_T, nRec, ctx->cuCount, aggWaveGeom() >= 0);     // (the units' and segments' chunks of the entry array: aggvote.h AG_CHUNK)
                unsigned long long capEnt = nGroup / 6 + (4ull << 20) + slack;
                if (const char *e = cdmGetenv("CDM_AGG_CAP")) capEnt = strtoull(e, nullptr, 10);      // tests: force the overflow fallback
                int rc = aggregate(sortedOut, nGroup, rk.current(), (const uint64_t *) rv.current(), dst.p, nRec, gk, top2, capEnt, !wordFits);
                while (rc == CDM_ERR_UNSUPPORTED && wide && capEnt < nGroup + 1 + slack) {
                    capEnt = std::min<unsigned long long>(nGroup + 1 + slack, std::max<unsigned long long>(capEnt * 3, 1024));
                    rc = aggregate(sortedOut, nGroup, rk.current(), (const uint64_t *) rv.current(), dst.p, nRec, gk, top2, capEnt, !wordFits);
                }
                if (rc == CDM_ERR_UNSUPPORTED && !wide) aggregated = false;      // (entry buffer too small for this input: the tuple path)
                else if (rc) return rc;
            }
            haveEntries = aggregated;
            if (!aggregated && segmentedSortKeys(s, ctx->cuCount, sortedOut, sortedOut, nGroup, (int) (idBits + diagBits + 1), (int) (diagBits + 1), top2, rk.current(), dst.p, nRec, gk,
                                  (const uint64_t *) rv.current()) != CDM_OK) {
                cdm_set_error("cdm_kmermatch: segmented sort 2 failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP;
            }
        }
        sorted2 = sortedOut;
    }
    if (!sort2Runs || sort2Check) {
        // (radix variant: the keys are sorted between keysIn and bufA by the passes of radix.h; bufB == keysIn)
        const int shiftHi2 = lsdOnly ? 1 : std::max(1, top2 + 1 - 32);
        bool g2First = true;
        if (int rc = rx::sortKeys<uint64_t>(s, ctx->cuCount, const_cast<uint64_t *>(keysIn), bufA, (uint64_t) nIn, shiftHi2, top2 + 1, g2First)) return rc;
        DoubleBuf<uint64_t> g(g2First ? const_cast<uint64_t *>(keysIn) : bufA, g2First ? bufA : const_cast<uint64_t *>(keysIn));
        unsigned long long nGroupR = 0;
        if (nIn) {
            hipLaunchKernelGGL(k_live_count, dim3(1), dim3(1), 0, s, (const uint64_t *) g.current(), (uint64_t) nIn, top2, counters.p + 2);
            hipMemcpyAsync(&nGroupR, counters.p + 2, 8, hipMemcpyDeviceToHost, s);
            if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: radix sort 2 failed"); return CDM_ERR_HIP; }
        }
        const uint64_t *sortedR = g.current();
        if (shiftHi2 > 1) {
            if (bucket::bucketSortKeys(s, g.current(), g.alternate(), nGroupR, shiftHi2, 1, top2) != CDM_OK) { cdm_set_error("cdm_kmermatch: bucket sort 2 failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP; }
            sortedR = g.alternate();
        }
        if (sort2Check) {
            if (nGroupR != nGroup) { cdm_set_error("cdm_kmermatch: sort 2 check: %llu kept tuples by runs, %llu by radix", nGroup, nGroupR); return CDM_ERR_HIP; }
            hipMemsetAsync(counters.p + 5, 0xFF, 8, s);
            if (nGroup) hipLaunchKernelGGL(k_first_diff, dim3((unsigned) std::min<uint64_t>((nGroup + 255) / 256, 65535)), dim3(256), 0, s, sorted2, sortedR, (uint64_t) nGroup, counters.p + 5);
            unsigned long long firstDiff = ~0ull, pair[2] = {0, 0};
            hipMemcpyAsync(&firstDiff, counters.p + 5, 8, hipMemcpyDeviceToHost, s);
            if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: sort 2 check failed"); return CDM_ERR_HIP; }
            if (firstDiff != ~0ull) {
                hipMemcpy(&pair[0], sorted2 + firstDiff, 8, hipMemcpyDeviceToHost); hipMemcpy(&pair[1], sortedR + firstDiff, 8, hipMemcpyDeviceToHost);
                cdm_set_error("cdm_kmermatch: sort 2 check: first difference at %llu of %llu: runs %016llx radix %016llx (idBits %u diagBits %u)", firstDiff, nGroup, pair[0], pair[1], idBits, diagBits);
                return CDM_ERR_HIP;
            }
        }
        nGroup = nGroupR; sorted2 = sortedR;
    }
    hipEventRecord(ctx->ev1, s);
    sorted2M = sorted2; nGroupM = nGroup;
    return CDM_OK;
}
// Sort 2's first step, which the hand-off to other ranks shares: the run records of a group-key array - the ones the grouping kernel
// staged (`staged`) or made from the array -, sorted by representative (stable: k-mer order inside one), and in dst the exclusive sums
// of the run lengths, the last of which - the kept tuples - is on its way to `total` when this returns (asynchronous on s).
// dstIfNone: dst is allocated for an array without records too.
struct RepRecords {
    cdmscan::ScanTemp st; DevBuf<uint32_t> r0, r1; DevBuf<uint64_t> v0, v1; DevBuf<unsigned long long> dst; unsigned long long nRec = 0;
    DoubleBuf<uint32_t> rep; DoubleBuf<uint64_t> val;        // the sorted records
};
int recordsByRep(const runsort::RunArgs &ra, bool staged, bool dstIfNone, RepRecords &R, unsigned long long &total) {
    if (staged) { if (int rc = stagedRunRecords(ra, R.r0, R.r1, R.v0, R.v1, R.nRec)) return rc; }       // (the slot layout's grouping kernel wrote them already)
    else if (int rc = runsort::makeRunRecords(s, ra, R.r0, R.r1, R.v0, R.v1, R.nRec)) return rc;
    if (R.nRec == 0 && !dstIfNone) return CDM_OK;
    if (!R.dst.alloc(R.nRec + 1)) { cdm_set_error("cdm_kmermatch: out of device memory (%llu run records)", R.nRec); return CDM_ERR_HIP; }
    if (R.nRec == 0) return CDM_OK;
    R.rep = DoubleBuf<uint32_t>(R.r0.p, R.r1.p); R.val = DoubleBuf<uint64_t>(R.v0.p, R.v1.p);
    if (int rc = rx::sortPairs<uint32_t, uint64_t>(s, ctx->cuCount, R.rep, R.val, (uint64_t) R.nRec, 0, (int) idBits)) return rc;
    // (the scan reads one element past the records: the value buffers have R.nRec + 1 entries, the last one's length is not used)
    hipMemsetAsync(R.val.current() + R.nRec, 0, 8, s);
    if (int rc = cdmscan::exclusiveScanFn<unsigned long long, runsort::RunLen>(s, R.st, runsort::RunLen{R.val.current()}, R.dst.p, (size_t) R.nRec + 1)) return rc;
    hipMemcpyAsync(&total, R.dst.p + R.nRec, 8, hipMemcpyDeviceToHost, s);
    return CDM_OK;
}
// The run records of the whole key array from what the grouping kernel staged for region 1 (k_rec_compact: the waves' records packed,
// in wave order = k-mer order) + the records of region 2 (the whole-sequence hash tuples' group keys: k_run_records on that part).
int stagedRunRecords(const runsort::RunArgs &whole, DevBuf<uint32_t> &rr0, DevBuf<uint32_t> &rr1, DevBuf<uint64_t> &rv0, DevBuf<uint64_t> &rv1, unsigned long long &nRec) {
    DevBuf<unsigned long long> off; cdmscan::ScanTemp st;
    if (!off.alloc(stagedWaves + 1)) { cdm_set_error("cdm_kmermatch: out of device memory (run records)"); return CDM_ERR_HIP; }
    if (int rc = cdmscan::exclusiveScanFn<unsigned long long, RecCount>(s, st, RecCount{stCnt.p}, off.p, (size_t) stagedWaves + 1)) return rc;      // (stCnt[stagedWaves] = 0)
    unsigned long long n1 = 0, n2 = 0;
    hipMemcpyAsync(&n1, off.p + stagedWaves, 8, hipMemcpyDeviceToHost, s);
    // region 2
    DevBuf<uint32_t> q0, q1; DevBuf<uint64_t> w0, w1;
    runsort::RunArgs r2 = whole; r2.keys = whole.keys + kmerSlots; r2.n = whole.n - kmerSlots; r2.skipLo = r2.skipHi = 0; r2.base = kmerSlots;
    if (r2.n) { if (int rc = runsort::makeRunRecords(s, r2, q0, q1, w0, w1, n2)) return rc; }
    if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: run records failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP; }
    // the records that are not in the waves' stages - the big buckets' and the stages' overflow - as ONE list sorted by start
    unsigned long long nb = nBigRec;
    if (nOvRec) {
        DevBuf<uint64_t> x0, x1; DevBuf<uint32_t> y0, y1;
        const unsigned long long tot = nBigRec + nOvRec;
        if (!x0.alloc(tot) || !x1.alloc(tot) || !y0.alloc(tot) || !y1.alloc(tot)) { cdm_set_error("cdm_kmermatch: out of device memory (run records)"); return CDM_ERR_HIP; }
        if (nBigRec) { hipMemcpyAsync(x0.p, bigRecVal.p, nBigRec * 8, hipMemcpyDeviceToDevice, s); hipMemcpyAsync(y0.p, bigRecRep.p, nBigRec * 4, hipMemcpyDeviceToDevice, s); }
        hipMemcpyAsync(x0.p + nBigRec, ovVal.p, nOvRec * 8, hipMemcpyDeviceToDevice, s); hipMemcpyAsync(y0.p + nBigRec, ovRep.p, nOvRec * 4, hipMemcpyDeviceToDevice, s);
        DoubleBuf<uint64_t> x(x0.p, x1.p); DoubleBuf<uint32_t> y(y0.p, y1.p);
        if (int rc = rx::sortPairs<uint64_t, uint32_t>(s, ctx->cuCount, x, y, (uint64_t) tot, runsort::RUN_CNT_BITS, 64)) return rc;
        bigRecVal.free(); bigRecRep.free();
        bigRecVal.p = x.current() == x0.p ? x0.release() : x1.release(); bigRecRep.p = y.current() == y0.p ? y0.release() : y1.release();
        nb = tot;
    }
    nRec = n1 + nb + n2;
    if (!rr0.alloc(nRec) || !rr1.alloc(nRec) || !rv0.alloc(nRec + 1) || !rv1.alloc(nRec + 1)) { cdm_set_error("cdm_kmermatch: out of device memory (%llu run records)", nRec); return CDM_ERR_HIP; }
    if (n1) hipLaunchKernelGGL(k_rec_compact, CDM_GRID((stagedWaves + REC_WAVES - 1) / REC_WAVES, 256), dim3(256), 0, s, (const uint32_t *) stRep.p, (const uint64_t *) stVal.p, (const unsigned long long *) off.p, (uint64_t) stagedWaves,
                               (uint64_t) stagedOwn, (const uint64_t *) bigRecVal.p, (uint64_t) nb, rr0.p, rv0.p);
    if (nb) hipLaunchKernelGGL(k_rec_place_big, CDM_GRID((nb + 255) / 256, 256), dim3(256), 0, s, (const uint32_t *) bigRecRep.p, (const uint64_t *) bigRecVal.p, (uint64_t) nb, (const uint64_t *) stVal.p, (const uint8_t *) stCnt.p,
                               (const unsigned long long *) off.p, (uint64_t) stagedOwn, rr0.p, rv0.p);
    if (n2) { hipMemcpyAsync(rr0.p + n1 + nb, q0.p, n2 * 4, hipMemcpyDeviceToDevice, s); hipMemcpyAsync(rv0.p + n1 + nb, w0.p, n2 * 8, hipMemcpyDeviceToDevice, s); }
    if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: run records (packing) failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP; }
    if (cdmGetenv("CDM_BUCKET_STATS")) fprintf(stderr, "run records: %llu staged by the grouping kernel, %llu beyond its waves' stages, %llu of its big buckets, %llu of the whole-sequence hash region\n", n1, nOvRec, nBigRec, n2);
    stRep.free(); stVal.free(); stCnt.free(); bigRecRep.free(); bigRecVal.free(); ovRep.free(); ovVal.free(); stagedWaves = 0; nBigRec = 0; nOvRec = 0;
    return CDM_OK;
}
// K4 on entries: the per-representative hit counts are known already (aggregate); offsets, self hits, then one thread per segment
int voteEntries(cdm_hits **out, const uint32_t *contDev = nullptr) {
    DevBuf<unsigned long long> perRepScan;
    if (!perRepScan.alloc((size_t) n + 1)) { cdm_set_error("cdm_kmermatch: out of device memory (vote)"); return CDM_ERR_HIP; }
    cdmscan::ScanTemp st4a;
    if (int rc = cdmscan::exclusiveScan<unsigned long long>(s, st4a, agPerRep.p, perRepScan.p, (size_t) n + 1)) return rc;
    if (int rc = placeHits(perRepScan.p, true, out, [&](cdm_hits *res) {
        aggv::VoteEntArgs va; va.ent = agEnt.p; va.entOff = agEntOff.p; va.entCnt = agEntCnt.p; va.segRep = agSegRep.p; va.nSeg = nSegM; va.hitOff = res->off; va.stale = staleBuf.p; va.diagBias = diagBias; va.cont = contDev;
        if (nSegM) hipLaunchKernelGGL(aggv::k_vote_entries<HitRec>, dim3((unsigned) ((nSegM + 255) / 256)), dim3(256), 0, s, va, res->rec);
    })) return rc;
    agEnt.free(); agEntOff.free(); agEntCnt.free(); agSegRep.free(); agSegOfRec.free(); agSegFirstRec.free(); agPerRep.free(); agPending.free();
    return CDM_OK;
}
// The tail of both votes.  perRepScan: exclusive sums of the hits per representative -> the offsets of the hit lists (one self hit per
// sequence in front of its own hits), the records with the self hits in, `place` for the others, and the step's timings (sort1R2:
// with the one of sort 1's region 2).
template <typename Place>
int placeHits(const unsigned long long *perRepScan, bool sort1R2, cdm_hits **out, Place place) {
    cdm_hits *res = new cdm_hits(); res->n = n;
    if (cdmMalloc(&res->off, ((size_t) n + 1) * 8) != hipSuccess) { delete res; cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
    hipLaunchKernelGGL(k_offsets, dim3((n + 256) / 256), dim3(256), 0, s, perRepScan, n, res->off);
    uint64_t total = 0;
    hipMemcpyAsync(&total, res->off + n, 8, hipMemcpyDeviceToHost, s);
    { hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) { cdm_hits_free(res); cdm_set_error("cdm_kmermatch: vote failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; } }
    res->count = total;
    if (cdmMalloc(&res->rec, (total + 1) * sizeof(HitRec)) != hipSuccess) { cdm_hits_free(res); cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
    hipLaunchKernelGGL(k_self, dim3((n + 255) / 256), dim3(256), 0, s, res->off, n, res->rec);
    place(res);
    { hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) { cdm_hits_free(res); cdm_set_error("cdm_kmermatch: placing hits failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; } }
    float msSort2 = 0; hipEventElapsedTime(&msSort2, ctx->ev0, ctx->ev1);
    ctx->lastMs[2] = msSort1 + msSort2;
    ctx->lastMs[5] = msSort1;   // sort 1 call alone (1 histogram + ceil(63/8) onesweep launches)
    ctx->lastMs[6] = msSort2;
    if (sort1R2) hipEventElapsedTime(&ctx->lastMs[7], ctx->ev2, ctx->ev3);   // sort 1, region 2 (whole-sequence hash tuples)
    *out = res;
    return CDM_OK;
}
// The wave-sized instances of k_unit_agg (aggvote.h): unit range, threads, table slots, distinct limit, segments, waves per SIMD the
// registers leave room for, tuples a thread fetches per batch, and the most tuples of a unit of the class.  CDM_AGG_GEOM picks one (the sweep of
// profiles/wave_agg_geometry.txt), CDM_AGG_WAVE_CAP lowers the tuple capacity, CDM_AGG=block runs the block instances alone.
struct AggWaveGeom { int range, nt, h, dl, no, minw, items; uint32_t cap; };
static constexpr AggWaveGeom AGG_WAVE[] = {{256, 64, 256, 128, 32, 6, 2, 2304}, {256, 64, 256, 128, 32, 5, 4, 2304}, {256, 64, 512, 256, 32, 3, 4, 2304},
                                           {512, 128, 512, 256, 64, 6, 2, 2560}, {512, 64, 512, 256, 64, 3, 4, 2560}, {256, 128, 256, 128, 32, 6, 2, 2304}};
static constexpr int AGG_WAVE_GEOMS = (int) (sizeof(AGG_WAVE) / sizeof(AGG_WAVE[0])), AGG_WAVE_DEFAULT = 1;
template <int G, typename W> static void launchWaveAgg(hipStream_t st, unsigned int grid, unsigned int pad, const aggv::AggArgs &a) {
    constexpr AggWaveGeom g = AGG_WAVE[G];
    hipLaunchKernelGGL((aggv::k_unit_agg<g.nt, g.items, g.h, g.dl, 2, g.no, g.minw, W>), dim3(grid), dim3(g.nt), pad, st, a);
}
template <typename W> static void launchWaveAggGeom(int geom, hipStream_t st, unsigned int grid, unsigned int pad, const aggv::AggArgs &a) {
    switch (geom) {
        case 0: launchWaveAgg<0, W>(st, grid, pad, a); break;
        case 1: launchWaveAgg<1, W>(st, grid, pad, a); break;
        case 2: launchWaveAgg<2, W>(st, grid, pad, a); break;
        case 3: launchWaveAgg<3, W>(st, grid, pad, a); break;
        case 4: launchWaveAgg<4, W>(st, grid, pad, a); break;
        default: launchWaveAgg<5, W>(st, grid, pad, a); break;
    }
}
template <int CLS, typename W> static void launchBlockAgg(hipStream_t st, unsigned int grid, unsigned int pad, const aggv::AggArgs &a) {
    // (tuples a thread fetches per batch: the class's capacity in one batch, the largest class's in two - twelve keys in registers next to
    // the look-ahead of the next unit spill)
    constexpr int ITEMS = runsort::U_CLASS_CAP[CLS] / 256 > 8 ? runsort::U_CLASS_CAP[CLS] / 512 : runsort::U_CLASS_CAP[CLS] / 256;
    hipLaunchKernelGGL((aggv::k_unit_agg<256, ITEMS, aggv::AG_H, aggv::AG_D, 2, runsort::U_T, CDM_AGG_MINW, W>), dim3(grid), dim3(256), pad, st, a);
}
// sort 2 on aggregated tuples (aggvote.h): segments, k_unit_agg in k_unit_sort's place, the tuple sorters for what no table holds,
// k_rle_segment for those.  CDM_ERR_UNSUPPORTED: the entry buffer was too small (the caller takes the tuple path).
static void aggUnitHook(hipStream_t st, unsigned int grid, int cls, const unsigned long long *list, const unsigned int *count, const runsort::UnitClassLists &next, bucket::BigList hard, void *user) {
    const aggv::AggArgs *u = reinterpret_cast<const aggv::AggArgs *>(user);
    aggv::AggArgs a = *u;
    a.list = list; a.count = count; a.hard = hard;
    const unsigned int pad = cdm_lds_pad("CDM_LDS_PAD_AGG");
    grid = std::min(grid, (unsigned int) u->cuCount * aggv::aggGridPerCu(u->waveGeom >= 0));
    if (cls < 0) {      // the wave-sized instance, in front of the size classes
        a.next = next;
        if (u->wideWord) launchWaveAggGeom<bucket::u128>(u->waveGeom, st, grid, pad, a); else launchWaveAggGeom<uint64_t>(u->waveGeom, st, grid, pad, a);
        return;
    }
    if (u->wideWord) {
        if (cls == 0) launchBlockAgg<0, bucket::u128>(st, grid, pad, a); else if (cls == 1) launchBlockAgg<1, bucket::u128>(st, grid, pad, a); else launchBlockAgg<2, bucket::u128>(st, grid, pad, a);
        return;
    }
    if (cls == 0) launchBlockAgg<0, uint64_t>(st, grid, pad, a); else if (cls == 1) launchBlockAgg<1, uint64_t>(st, grid, pad, a); else launchBlockAgg<2, uint64_t>(st, grid, pad, a);
}
// the wave-sized instance in use: -1 under CDM_AGG=block
static int aggWaveGeom() {
    const char *m = cdmGetenv("CDM_AGG");
    if (m && !strcmp(m, "block")) return -1;
    int g = AGG_WAVE_DEFAULT;
    if (const char *e = cdmGetenv("CDM_AGG_GEOM")) { const int v = atoi(e); if (v >= 0 && v < AGG_WAVE_GEOMS) g = v; }
    return g;
}
int aggregate(uint64_t *sortedOut, unsigned long long nGroup, const uint32_t *recRep, const uint64_t *recVal, const unsigned long long *dst, unsigned long long nRec,
              const uint64_t *gk, int top2, unsigned long long capEnt, bool wideWord) {
    using namespace aggv;
    cdmscan::ScanTemp st;
    agEnt.free(); agSegOfRec.free(); agPerRep.free(); agCursor.free(); agFlags.free(); agSegRep.free(); agSegFirstRec.free(); agEntOff.free(); agEntCnt.free(); agPending.free();     // (a second try)
    if (!agSegOfRec.alloc(nRec + 2) || !agPerRep.alloc((size_t) n + 1) || !agCursor.alloc(2) || !agFlags.alloc(4)) { cdm_set_error("cdm_kmermatch: out of device memory (aggregation)"); return CDM_ERR_HIP; }
    hipLaunchKernelGGL(k_seg_flags, CDM_GRID((nRec + 1024) / 1024, 1024), dim3(1024), 0, s, recRep, (uint64_t) nRec, agSegOfRec.p);
    if (int rc = cdmscan::exclusiveScan<uint32_t>(s, st, agSegOfRec.p, agSegOfRec.p, (size_t) nRec + 1)) return rc;
    uint32_t nSeg = 0;
    hipMemcpyAsync(&nSeg, agSegOfRec.p + nRec, 4, hipMemcpyDeviceToHost, s);
    if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: aggregation (segments) failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP; }
    if (!agSegRep.alloc(nSeg + 1) || !agSegFirstRec.alloc((size_t) nSeg + 2) || !agEntOff.alloc((size_t) nSeg + 1) || !agEntCnt.alloc((size_t) nSeg + 1) || !agPending.alloc((size_t) nSeg + 1) ||
        !agEnt.alloc(capEnt + 1)) {
        agEnt.free(); cdm_set_error("cdm_kmermatch: out of device memory (aggregation)"); return CDM_ERR_HIP;
    }
    hipLaunchKernelGGL(k_seg_fill, CDM_GRID((nRec + 1024) / 1024, 1024), dim3(1024), 0, s, recRep, (uint64_t) nRec, agSegOfRec.p, agSegRep.p, agSegFirstRec.p, agEntCnt.p);
    hipMemsetAsync(agPerRep.p, 0, ((size_t) n + 1) * 8, s);
    hipMemsetAsync(agCursor.p, 0, 16, s); hipMemsetAsync(agFlags.p, 0, 16, s);
    AggArgs a;
    a.keys = gk; a.recVal = recVal; a.dst = dst; a.nRec = nRec; a.segOfRec = agSegOfRec.p; a.segRep = agSegRep.p; a.segFirstRec = agSegFirstRec.p; a.nSeg = nSeg;
    a.entOff = agEntOff.p; a.entCnt = agEntCnt.p; a.perRep = agPerRep.p; a.ent = agEnt.p; a.cursor = agCursor.p; a.cap = capEnt; a.overflow = agFlags.p;
    a.maxD = AG_D; a.recRep = recRep; a.cuCount = ctx->cuCount; a.waveGeom = aggWaveGeom();
    int unitRange = runsort::U_T; uint32_t frontCap = 0;
    if (a.waveGeom >= 0) {
        unitRange = AGG_WAVE[a.waveGeom].range; frontCap = AGG_WAVE[a.waveGeom].cap;
        if (const char *e = cdmGetenv("CDM_AGG_WAVE_CAP")) { const long v = atol(e); if (v >= 1 && v < (long) frontCap) frontCap = (uint32_t) v; }
    }
    if (const char *e = cdmGetenv("CDM_AGG_D")) { const long v = atol(e); if (v >= 1 && v <= AG_D) a.maxD = (uint32_t) v; }
    a.repShift = (int) (idBits + diagBits + 1); a.diagBits = (int) diagBits; a.idBits = idBits; a.sorted = sortedOut; a.list = nullptr; a.count = nullptr; a.hard.list = nullptr; a.hard.cnt = nullptr;
    a.wideWord = wideWord ? 1 : 0;
    if (runsort::segmentedSortKeys(s, ctx->cuCount, sortedOut, sortedOut, nGroup, (int) (idBits + diagBits + 1), (int) (diagBits + 1), top2, recRep, dst, nRec, gk, recVal, aggUnitHook, &a, wide, agSegOfRec.p, (int) bitsFor((uint64_t) nSeg + 1), agSegFirstRec.p, (uint64_t) nSeg, unitRange, frontCap) != CDM_OK) {
        cdm_set_error("cdm_kmermatch: segmented sort 2 failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP;
    }
    // the segments the tuple sorters finished (deep pile-ups, units with too many distinct triples)
    hipLaunchKernelGGL(k_pending_list, dim3((unsigned) (((uint64_t) nSeg + 1023) / 1024)), dim3(1024), 0, s, (const uint32_t *) agEntCnt.p, (uint64_t) nSeg, agPending.p, agFlags.p + 1);
    unsigned int fl[4] = {0, 0, 0, 0};
    hipMemcpyAsync(fl, agFlags.p, 16, hipMemcpyDeviceToHost, s);
    if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: aggregation failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP; }
    if (fl[1] && cdmGetenv("CDM_RLE_STATS")) {      // diagnosis: how many segments the tuple sorters finished, and how long they are
        std::vector<uint32_t> pl(fl[1]); std::vector<unsigned long long> fr((size_t) nSeg + 1), dd((size_t) nRec + 1);
        hipMemcpy(pl.data(), agPending.p, (size_t) fl[1] * 4, hipMemcpyDeviceToHost); hipMemcpy(fr.data(), agSegFirstRec.p, ((size_t) nSeg + 1) * 8, hipMemcpyDeviceToHost);
        hipMemcpy(dd.data(), dst, ((size_t) nRec + 1) * 8, hipMemcpyDeviceToHost);
        unsigned long long tot = 0, mx = 0, over4k = 0, over64k = 0, inBig = 0;
        for (uint32_t g : pl) { const unsigned long long m = dd[fr[g + 1]] - dd[fr[g]]; tot += m; mx = std::max(mx, m); if (m > 4096) { over4k++; inBig += m; } if (m > 65536) over64k++; }
        fprintf(stderr, "rle segments: %u of %llu, %llu tuples (longest %llu; %llu beyond 4096 tuples holding %llu, %llu beyond 65536)\n", fl[1], (unsigned long long) nSeg, tot, mx, over4k, inBig, over64k);
    }
    if (fl[1] && !fl[0]) {
        hipLaunchKernelGGL(k_rle_segment, dim3(std::min<unsigned int>((fl[1] + 3) / 4, (unsigned int) ctx->cuCount * 16)), dim3(256), 0, s, a, (const uint32_t *) agPending.p, (const unsigned int *) (agFlags.p + 1));
        hipMemcpyAsync(fl, agFlags.p, 16, hipMemcpyDeviceToHost, s);
        if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: aggregation (segments of the tuple sorters) failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP; }
    }
    unsigned long long used = 0;
    hipMemcpy(&used, agCursor.p, 8, hipMemcpyDeviceToHost);
    if (cdmGetenv("CDM_BUCKET_STATS") && !fl[0]) {     // every segment's entries, whoever wrote them: a unit finished twice would show here
        std::vector<uint32_t> ec(nSeg);
        hipMemcpy(ec.data(), agEntCnt.p, (size_t) nSeg * 4, hipMemcpyDeviceToHost);
        unsigned long long written = 0;
        for (uint32_t c : ec) written += c;
        fprintf(stderr, "aggregate: %llu entries written (%s)\n", written, a.waveGeom >= 0 ? "wave-sized units in front" : "block form");
        if (a.waveGeom >= 0) {
            const AggWaveGeom &g = AGG_WAVE[a.waveGeom];
            fprintf(stderr, "aggregate: wave-sized instance %d: unit range %d, %d threads, table of %d slots, distinct limit %d, %d records a round, %u tuples\n", a.waveGeom, g.range, g.nt, g.h, g.dl, 2 * g.nt, frontCap);
        }
    }
    if (cdmGetenv("CDM_BUCKET_STATS")) fprintf(stderr, "aggregate: %llu group tuples, %u segments, %llu entries (room for %llu), %u segments through the tuple sorters%s\n", nGroup, nSeg, used, capEnt, fl[1],
                                            fl[0] ? "; entry buffer overflow" : "");
    if (fl[0]) { agEnt.free(); return CDM_ERR_UNSUPPORTED; }
    nSegM = nSeg;
    return CDM_OK;
}
// ---- K4: count hit-producing segments (per tile and per representative), scan, vote + place.  contDev: VoteArgs::cont
int vote(const uint32_t *contDev, bool ownBuffers, cdm_hits **out) {
    if (haveEntries) return voteEntries(out, contDev);
    const uint64_t *sorted2 = sorted2M; const unsigned long long nGroup = nGroupM;
    DevBuf<unsigned long long> perRep, perRepScan, vTileCnt, vTileOff;
    const uint64_t vTiles = (nGroup + CP_TILE - 1) / CP_TILE;
    if (!perRep.alloc((size_t) n + 1) || !perRepScan.alloc((size_t) n + 1) || !vTileCnt.alloc(vTiles + 1) || !vTileOff.alloc(vTiles + 1)) {
        cdm_set_error("cdm_kmermatch: out of device memory (vote)"); return CDM_ERR_HIP;
    }
    hipMemsetAsync(perRep.p, 0, ((size_t) n + 1) * 8, s);
    hipMemsetAsync(vTileCnt.p, 0, (vTiles + 1) * 8, s);
    VoteArgs va;
    if (ownBuffers && nGroup != nKept) { cdm_set_error("cdm_kmermatch: internal error: %llu group tuples counted, %llu sorted", nKept, nGroup); return CDM_ERR_HIP; }
    va.stale = staleBuf.p; va.cont = contDev;
    va.keys = sorted2; va.n = nGroup; va.idBits = idBits; va.diagBits = diagBits; va.diagBias = diagBias; va.perRep = perRep.p;
    if (nGroup) hipLaunchKernelGGL(k_seg_count, dim3((unsigned) vTiles), dim3(256), 0, s, va, vTileCnt.p);
    cdmscan::ScanTemp st4a, st4b;
    if (int rc = cdmscan::exclusiveScan<unsigned long long>(s, st4a, perRep.p, perRepScan.p, (size_t) n + 1)) return rc;
    if (int rc = cdmscan::exclusiveScan<unsigned long long>(s, st4b, vTileCnt.p, vTileOff.p, (size_t) vTiles + 1)) return rc;
    return placeHits(perRepScan.p, ownBuffers, out, [&](cdm_hits *res) {
        if (nGroup) hipLaunchKernelGGL(k_seg_place, dim3((unsigned) vTiles), dim3(256), cdm_lds_pad("CDM_LDS_PAD_VOTE"), s, va, vTileOff.p, perRepScan.p, res->off, res->rec);
    });
}
// Multi-GPU hand-off: the kept group keys of this range grouped by representative (k-mer order inside a representative), in
// `gathered` (the first nKept entries of the buffer the sorted tuple keys were in): run records, their stable sort by rep, the
// expanding gather (runsort.h).  Slices of it by representative range are what the ranks exchange.
int gatherByRep() override {
    using namespace runsort;
    v0.free(); v1.free();
    RunArgs ra; ra.keys = (const uint64_t *) startIo; ra.n = nTuples; ra.skipLo = live; ra.skipHi = kmerSlots; ra.repShift = (int) (idBits + diagBits + 1);
    unsigned long long nOut = 0;
    RepRecords R;
    if (int rc = recordsByRep(ra, stagedWaves != 0, false, R, nOut)) return rc;
    gathered = keys.current();
    if (R.nRec == 0) return CDM_OK;
    hipLaunchKernelGGL(k_run_gather, CDM_GRID((R.nRec + 255) / 256, 256), dim3(256), 0, s, (const uint64_t *) startIo, (const uint64_t *) R.val.current(), (const unsigned long long *) R.dst.p, (uint64_t) R.nRec, gathered);
    if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: gather by representative failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP; }
    if (nOut != nKept) { cdm_set_error("cdm_kmermatch: internal error: %llu group tuples counted, %llu gathered", nKept, nOut); return CDM_ERR_HIP; }
    return CDM_OK;
}
// second half on group keys received from all ranks (device buffer; concatenated in rank = k-mer order, so that the stable
// sort by representative leaves every representative's tuples in global k-mer order): sort 2, then the head of the sorted array
// for the rank in front (head: CONT_CAP + 3 values, k_head_segment; info[0] = tuples, info[1] = target id of the last one)
int sortFrom(const uint64_t *devKeys, uint64_t nKeys, uint32_t *head, uint64_t info[2]) override {
    k0.free(); k1.free(); v0.free(); v1.free();             // phase A's tuple buffers are not needed any more
    if (!recvA.alloc(nKeys) || !recvB.alloc(nKeys) || !contBuf.alloc(CONT_CAP + 4)) { cdm_set_error("cdm_kmermatch: out of device memory for %llu received group tuples", (unsigned long long) nKeys); return CDM_ERR_HIP; }
    if (nKeys) hipMemcpyAsync(recvB.p, devKeys, nKeys * 8, hipMemcpyDeviceToDevice, s);
    if (int rc = sort2(recvB.p, nKeys, 0, 0, recvA.p, recvB.p, false)) return rc;
    if (haveEntries) {      // the head and the last target from the aggregated entries (two words per entry)
        static_assert(aggv::HEAD_WORDS == CONT_CAP, "the words of a head");
        uint32_t lastId = 0;
        hipLaunchKernelGGL(aggv::k_head_entries, dim3(1), dim3(1), 0, s, (const aggv::Ent *) agEnt.p, (const unsigned long long *) agEntOff.p, (const uint32_t *) agEntCnt.p, (uint64_t) nSegM, contBuf.p);
        hipMemcpyAsync(head, contBuf.p, (CONT_CAP + 3) * 4, hipMemcpyDeviceToHost, s);
        hipMemcpyAsync(&lastId, contBuf.p + CONT_CAP + 3, 4, hipMemcpyDeviceToHost, s);
        if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: second half (aggregation) failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP; }
        info[0] = nGroupM; info[1] = lastId;
        return CDM_OK;
    }
    hipLaunchKernelGGL(k_head_segment, dim3(1), dim3(1), 0, s, sorted2M, (uint64_t) nGroupM, idBits, diagBits, contBuf.p);
    uint64_t last = 0;
    hipMemcpyAsync(head, contBuf.p, (CONT_CAP + 3) * 4, hipMemcpyDeviceToHost, s);
    if (nGroupM) hipMemcpyAsync(&last, sorted2M + nGroupM - 1, 8, hipMemcpyDeviceToHost, s);
    if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: second half (sort) failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP; }
    info[0] = nGroupM; info[1] = (last >> (diagBits + 1)) & ((1ull << idBits) - 1ull);
    return CDM_OK;
}
// the vote: cont = what this rank's last scan runs into (VoteArgs::cont: count, target, into-the-left-overs flag, entries; NULL:
// nothing behind this rank's tuples but the left-over list), staleIn = the combined left-over list
int voteWith(const uint32_t *cont, const uint32_t *staleIn, cdm_hits **out) override {
    if (hipMemcpyAsync(staleBuf.p, staleIn, (STALE_MAX + 3) * 4, hipMemcpyHostToDevice, s) != hipSuccess) { cdm_set_error("cdm_kmermatch: stale list upload failed"); return CDM_ERR_HIP; }
    if (cont) {
        if (cont[0] > (uint32_t) CONT_CAP) { cdm_set_error("cdm_kmermatch: the scan of this rank's last target runs over more than %d tuples of the next ranks; not reproduced", CONT_CAP); return CDM_ERR_UNSUPPORTED; }
        if (hipMemcpyAsync(contBuf.p, cont, (3 + (size_t) cont[0]) * 4, hipMemcpyHostToDevice, s) != hipSuccess) { cdm_set_error("cdm_kmermatch: continuation list upload failed"); return CDM_ERR_HIP; }
    }
    return vote(cont ? contBuf.p : nullptr, false, out);
}
};

// kmermatcher in PASSES over the k-mer space on one device, for inputs whose tuples do not fit it at once (the reference splits the
// same way when memory is short: kmermatcher.cpp:634-663, merged :742-784).  Pass r takes the tuples whose k-mer lies in range r of P:
// the sequences are extracted block by block (B blocks of the slot order; every block's tuples ordered by range, the slice of range r
// appended - the machinery of the multi-GPU split by reads), sorted and grouped as a range of a multi-GPU run is, and the group keys it
// keeps are appended to ONE array.  The ranges in order ARE the k-mer order, so that array is what a single pass leaves for sort 2,
// and sort 2 + vote run on it as they are.  What the reference's run-past-the-end scan needs (the tuples behind k-mer-order index J =
// number of kept keys, known only at the end) comes from running the range that holds J once more.  Cost: P + 2 extractions of the
// whole DB instead of one.
// OVER RANKS (ranks != NULL; csrc/dist.hip for DBs that take the wide group key): the same passes, each range run by ONE rank - every rank
// sweeps the blocks (the counts, hence the cuts, are the same everywhere), runs the ranges it owns (range r belongs to rank r W / P:
// consecutive ranges, in rank order), and the kept group keys - run starts included in the wide form, so the array describes itself -
// are all-gathered: every rank then holds the array a single device would have built and runs sort 2 + vote on it whole.  What is
// split is the first half (extraction aside), 70 % of kmermatcher; what travels is 8 bytes per kept key to every rank.
template <typename LY>
int kmermatchPassesT(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_kmer_params *par, int P, int B, cdm_hits **out, const KmerRanks *ranks = nullptr) {
    typedef typename LY::V V;
    hipStream_t s = ctx->stream;
    const int W = ranks ? ranks->world : 1, R = ranks ? ranks->rank : 0;
    if (W > 1) P = std::min(255, (std::max(P, 1) + W - 1) / W * W);
    if (P < 1 || P > 255 || B < 1) { cdm_set_error("cdm_kmermatch: %d passes over %d blocks", P, B); return CDM_ERR_INVALID; }        // (P: at most; fewer where the tuples sit in few slices of the k-mer space)
    const bool stats = cdmGetenv("CDM_BUCKET_STATS") != nullptr;
    // (this path runs because memory is short: its buffers are planned at their exact sizes, without the allocator's head room)
    struct NoHeadroom { float was; NoHeadroom() : was(cdmPoolHeadroomSwap(1.0f)) {} ~NoHeadroom() { cdmPoolHeadroomSwap(was); } } noHeadroom;
    // ---- how many tuples of every block fall into each of F = 256 fine slices of the k-mer space ([F]: the whole-sequence hash tuples,
    // which sort behind every k-mer).  The P ranges are runs of fine slices with about the same number of tuples: equal slices of the
    // k-mer space are anything but equal in tuples (1 M synthetic reads, 3 slices: 55 / 33 / 12 %).
    constexpr int F = CDM_KPART_SLICES;
    std::vector<std::vector<unsigned long long>> cnt((size_t) B, std::vector<unsigned long long>((size_t) F + 1, 0));
    auto extractBlock = [&](KmerJob<LY> &ex, int b) -> int { ex.part = 0; ex.nparts = F; ex.block = b; ex.nBlocks = B; ex.passes = true; return ex.splitBegin(); };
    std::vector<unsigned long long> fine((size_t) F, 0);
    auto poolLine = [&](const char *what, int i) { if (stats) { uint64_t st[8]; cdm_pool_stats(st); fprintf(stderr, "kmermatch passes (%d x %d): %s %d: %.1f GB mapped, %.1f GB in use\n", P, B, what, i, st[6] / 1e9, st[7] / 1e9); } };
    poolLine("start", 0);
    // The same sweep KEEPS every block's ordered tuples while they fit (the real tuples are far fewer than the slots where a per-sequence
    // budget selects the k-mers: 40 % in a late contig iteration) - then a range is gathered from the kept blocks; where they do not fit,
    // a range extracts the blocks again.  CDM_KMER_KEEP=<bytes> (tests: 0 = never keep).
    std::vector<std::unique_ptr<KmerJob<LY>>> kept((size_t) B);
    bool keepAll = true; unsigned long long keptBytes = 0, keepBudget = 0;
    { size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) == hipSuccess) keepBudget = (unsigned long long) (0.40 * (double) tot); else (void) hipGetLastError(); }
    if (const char *e = cdmGetenv("CDM_KMER_KEEP")) keepBudget = strtoull(e, nullptr, 10);
    for (int b = 0; b < B; b++) {
        std::unique_ptr<KmerJob<LY>> ex(new KmerJob<LY>(ctx, db, par));
        if (int rc = extractBlock(*ex, b)) return rc;
        for (int f = 0; f < F; f++) { cnt[b][f] = ex->sendOff[f + 1] - ex->sendOff[f]; fine[f] += cnt[b][f]; }
        cnt[b][F] = ex->sendHash;
        if (keepAll) {
            const unsigned long long bytes = (ex->sendOff[F] + ex->sendHash) * (8ull + sizeof(V));
            if (keptBytes + bytes > keepBudget) { keepAll = false; for (auto &q : kept) q.reset(); }
            else { if (int rc = ex->keepOnlyOutgoing()) return rc; keptBytes += bytes; kept[b] = std::move(ex); }
        }
        poolLine("counted block", b);
    }
    const std::vector<uint32_t> cut = equalShareCuts(fine.data(), F, P);          // range r = fine slices [cut[r], cut[r + 1])
    P = (int) cut.size() - 1;
    // a range's tuples, gathered from the blocks; then sort 1 + grouping on them
    auto runRange = [&](int r, KmerJob<LY> &job) -> int {
        const int f0 = (int) cut[r], f1 = (int) cut[r + 1];
        unsigned long long m = 0, h = 0; bool below = false;
        std::vector<unsigned long long> mine((size_t) B, 0);
        for (int b = 0; b < B; b++) {
            for (int f = f0; f < f1; f++) mine[b] += cnt[b][f];
            m += mine[b]; if (r == P - 1) h += cnt[b][F];
            for (int f = 0; f < f0; f++) below = below || cnt[b][f] != 0;
        }
        DevBuf<uint64_t> rk; DevBuf<V> rv;
        if (!rk.alloc(m + h) || !rv.alloc(m + h)) { cdm_set_error("cdm_kmermatch: out of device memory for a pass over %llu k-mer tuples", m + h); return CDM_ERR_HIP; }
        unsigned long long at = 0, hat = m;
        for (int b = 0; b < B; b++) {
            if (mine[b] == 0 && !(r == P - 1 && cnt[b][F])) continue;
            std::unique_ptr<KmerJob<LY>> again;
            if (!keepAll) { again.reset(new KmerJob<LY>(ctx, db, par)); if (int rc = extractBlock(*again, b)) return rc; }
            KmerJob<LY> &ex = keepAll ? *kept[b] : *again;
            if ((unsigned long long) (ex.sendOff[f1] - ex.sendOff[f0]) != mine[b] || ex.sendHash != cnt[b][F]) { cdm_set_error("cdm_kmermatch: internal error: a block's tuple counts changed between two extractions"); return CDM_ERR_HIP; }
            if (mine[b]) {
                hipMemcpyAsync(rk.p + at, (const uint64_t *) ex.sendKeys + ex.sendOff[f0], mine[b] * 8, hipMemcpyDeviceToDevice, s);
                hipMemcpyAsync(rv.p + at, (const V *) ex.sendVals + ex.sendOff[f0], mine[b] * sizeof(V), hipMemcpyDeviceToDevice, s);
                at += mine[b];
            }
            if (r == P - 1 && cnt[b][F]) {
                hipMemcpyAsync(rk.p + hat, ex.sendHashKeys, cnt[b][F] * 8, hipMemcpyDeviceToDevice, s);
                hipMemcpyAsync(rv.p + hat, ex.sendHashVals, cnt[b][F] * sizeof(V), hipMemcpyDeviceToDevice, s);
                hat += cnt[b][F];
            }
            if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: gathering a pass's tuples failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP; }
        }
        job.part = r; job.nparts = P;
        return job.rangeFinishOwned(rk, rv, m, h, below);
    };
    // ---- the passes: kept group keys (and, in the wide form, the dropped run starts that name a representative) in k-mer order
    DevBuf<uint64_t> G; unsigned long long gCap = 0, gCount = 0, J = 0;
    std::vector<unsigned long long> realOf((size_t) P, 0);
    DevBuf<unsigned long long> cntDev;
    if (!cntDev.alloc(1)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
    auto ownerOf = [&](int r) { return (int) ((long long) r * W / P); };
    std::vector<unsigned long long> keptOf((size_t) P, 0);
    for (int r = 0; r < P; r++) {
        if (ownerOf(r) != R) continue;
        KmerJob<LY> job(ctx, db, par);
        if (int rc = runRange(r, job)) return rc;
        realOf[r] = job.live + job.regionTwo; J += job.nKept; keptOf[r] = job.nKept;
        const unsigned long long nt = job.nTuples;
        if (stats) fprintf(stderr, "kmermatch pass %d of %d: %llu tuples, %llu kept\n", r + 1, P, nt, job.nKept);
        if (nt == 0) continue;
        if (gCount + nt > gCap) {       // (room for everything this range could keep; grown by doubling)
            const unsigned long long want = std::max(gCount + nt, gCap * 2);
            DevBuf<uint64_t> bigger;
            if (!bigger.alloc(want)) { cdm_set_error("cdm_kmermatch: out of device memory for %llu group keys", want); return CDM_ERR_HIP; }
            if (gCount) hipMemcpyAsync(bigger.p, G.p, gCount * 8, hipMemcpyDeviceToDevice, s);
            if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: growing the group key array failed"); return CDM_ERR_HIP; }
            G.free(); G.p = bigger.release(); gCap = want;
        }
        DevBuf<uint8_t> d0, d1;         // (the compaction moves pairs: one byte per key stands in for the value)
        if (!d0.alloc(nt) || !d1.alloc(nt)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
        if (int rc = rx::compactPairs<uint64_t, uint8_t>(s, (const uint64_t *) job.startIo, d0.p, (uint64_t) nt, G.p + gCount, d1.p, cntDev.p)) return rc;
        unsigned long long got = 0;
        hipMemcpyAsync(&got, cntDev.p, 8, hipMemcpyDeviceToHost, s);
        if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: collecting a pass's group keys failed"); return CDM_ERR_HIP; }
        gCount += got;
    }
    if (W > 1) {
        // every range's counts from its owner, then the kept keys of all ranks in rank (= range = k-mer) order
        std::vector<unsigned long long> mine(2 * (size_t) P + 1), all((2 * (size_t) P + 1) * W);
        for (int r = 0; r < P; r++) { mine[2 * r] = realOf[r]; mine[2 * r + 1] = keptOf[r]; }
        mine[2 * (size_t) P] = gCount;
        if (int rc = ranks->gatherHost(ranks->user, mine.data(), all.data(), mine.size() * 8)) return rc;
        J = 0;
        std::vector<uint64_t> recvOff((size_t) W + 1, 0);
        for (int p = 0; p < W; p++) {
            const unsigned long long *a = all.data() + (size_t) p * mine.size();
            for (int r = 0; r < P; r++) if (ownerOf(r) == p) { realOf[r] = a[2 * r]; J += a[2 * r + 1]; }
            recvOff[p + 1] = recvOff[p] + a[2 * (size_t) P] * 8;
        }
        const unsigned long long total = recvOff[W] / 8;
        DevBuf<uint64_t> whole;
        if (!whole.alloc(total)) { cdm_set_error("cdm_kmermatch: out of device memory for %llu group keys of all ranks", total); return CDM_ERR_HIP; }
        if (!G.p && !G.alloc(0)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
        if (int rc = ranks->gatherDev(ranks->user, G.p, gCount * 8, whole.p, recvOff.data(), s)) return rc;
        if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: gathering the ranks' group keys failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP; }
        G.free(); G.p = whole.release(); gCount = total; gCap = total;
    }
    // ---- the left-over list of the reference's last per-target scan (:875-887): from k-mer-order index J on, while the tuples belong
    // to one sequence - the range that holds index J once more, and the ranges behind it while the scan runs on (csrc/dist.hip does
    // the same across ranks; over ranks here, every rank runs that range itself: no exchange, one range's work)
    uint32_t stale[CDM_STALE_MAX + 5]; memset(stale, 0, sizeof(stale));
    if (J) {
        int holder = -1; unsigned long long jLocal = 0, base = 0;
        for (int r = 0; r < P; r++) { if (J < base + realOf[r]) { holder = r; jLocal = J - base; break; } base += realOf[r]; }
        uint32_t got = 0; bool have = false; uint32_t target = 0;
        for (int r = holder; holder >= 0 && r < P; r++) {
            KmerJob<LY> job(ctx, db, par);
            if (int rc = runRange(r, job)) return rc;
            if (int rc = job.staleTail(r == holder ? jLocal : 0)) return rc;
            const uint32_t *l = job.staleHost;
            if (l[0]) {
                if (!have) { target = l[1]; have = true; } else if (l[1] != target) break;
                for (uint32_t j = 0; j < l[0] && got < (uint32_t) CDM_STALE_MAX; j++) stale[2 + got++] = l[2 + j];
            }
            if (!l[CDM_STALE_MAX + 4]) break;
        }
        if (got >= (uint32_t) CDM_STALE_MAX) { cdm_set_error("cdm_kmermatch: the reference's last per-target scan would run over %d or more left-over tuples; not reproduced", CDM_STALE_MAX); return CDM_ERR_UNSUPPORTED; }
        stale[0] = got; stale[1] = have ? target : 0;
    }
    // ---- sort 2 + vote on the collected keys
    for (auto &q : kept) q.reset();
    KmerJob<LY> fin(ctx, db, par);
    fin.passes = true;
    if (int rc = fin.init()) return rc;
    if (!fin.staleBuf.alloc(STALE_MAX + 3) || !fin.k0.alloc(gCount)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
    if (hipMemcpyAsync(fin.staleBuf.p, stale, (STALE_MAX + 3) * 4, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_kmermatch: stale list upload failed"); return CDM_ERR_HIP; }
    if (!G.p && !G.alloc(0)) { cdm_set_error("cdm_kmermatch: out of device memory"); return CDM_ERR_HIP; }
    fin.startIo = (unsigned long long *) G.p; fin.live = gCount; fin.kmerSlots = gCount; fin.nTuples = gCount; fin.nKept = J;
    fin.keys = DoubleBuf<uint64_t>(fin.k0.p, G.p);
    if (int rc = fin.sort2(G.p, gCount, gCount, gCount, fin.k0.p, G.p, true)) return rc;
    return fin.vote(nullptr, true, out);
}
template <typename LY>
int kmermatchT(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_kmer_params *par, cdm_hits **out, const KmerRanks *ranks, const Db &d) {
    // One pass while the tuples fit the device (kmer_plan.h passPlan).  CDM_KMER_PASSES=P[,B] (tests, A/B): P passes over B blocks for any DB.
    PassPlan pl = passPlan(d, sizeof(typename LY::V));
    if (const char *e = cdmGetenv("CDM_KMER_PASSES")) { pl.P = atoi(e); const char *c = strchr(e, ','); pl.B = c ? atoi(c + 1) : pl.P; }
    const int P = pl.P, B = pl.B;
    if (ranks && ranks->world > 1) return kmermatchPassesT<LY>(ctx, db, par, std::max(P, ranks->world), std::max(B, 1), out, ranks);
    if (P > 1 || B > 1) return kmermatchPassesT<LY>(ctx, db, par, std::max(P, 1), std::max(B, 1), out);
    KmerJob<LY> job(ctx, db, par);
    job.ownPipeline = true;
    if (int rc = job.phaseA()) return rc;
    if (job.nKept) if (int rc = job.staleTail(job.nKept)) return rc;
    return job.phaseB(out);
}

// the switches kmer_plan.h's layout choice looks at
Switches layoutSwitches() {
    Switches sw;
    if (const char *e = cdmGetenv("CDM_KMER_LAYOUT")) sw.layout = !strcmp(e, "wide") ? LayoutSwitch::Wide : !strcmp(e, "packed") ? LayoutSwitch::Packed : !strcmp(e, "slot") ? LayoutSwitch::Slot : LayoutSwitch::Other;
    sw.forceHuge = cdmGetenv("CDM_FORCE_HUGE_LAYOUT"); sw.forceWideKey = cdmGetenv("CDM_FORCE_WIDE_KEY"); sw.kmerSort = cdmGetenv("CDM_KMER_SORT"); sw.kmerPasses = cdmGetenv("CDM_KMER_PASSES");
    return sw;
}
// f(LY()) for the layout's type
template <typename F> auto withLayout(Layout l, F f) -> decltype(f(LayoutHuge())) {
    return l == Layout::Slot ? f(LayoutSlot()) : l == Layout::Packed ? f(LayoutPacked()) : l == Layout::Wide ? f(LayoutWide()) : l == Layout::Long ? f(LayoutLong()) : f(LayoutHuge());
}

}  // namespace

// ---- multi-GPU: kmermatcher in two phases with an exchange in between (include/carpedeam_hip.h, carpedeam_amd/shard.py)
struct cdm_kpart { KmerJobBase *job = nullptr; uint64_t nSeq = 0; uint32_t repShift = 0; bool gatheredDone = false; };
// does cdm_kmermatch_part run this DB on the slot layout with balanced head-digit ranges? (csrc/dist.hip then takes it in place of the
// extract-everything-and-order-by-slice first half)
int cdm_kmermatch_part_takes_slots(const cdm_seqdb *db, const cdm_kmer_params *par) {
    return chooseLayout(Entry::Part, planDb(db, par->kmer_size, true), layoutSwitches()) == Layout::Slot ? 1 : 0;
}
// what cdm_kmermatch_part and cdm_kmermatch_split_begin (`entry`: the name in the error texts) share: the handle with the job of the
// DB's layout, and `start` - the entry's first phase - run on it.  A DB of one read length takes the 8-byte slot layout on a rank's k-mer range as on one device (round 5), the rank's range
// a run of head digits with its share of the tuples (CDM_KMER_LAYOUT=packed|wide: the 12-byte layouts and equal slices of the k-mer
// space by value, as before); the split by reads never does.
template <typename Start>
static int openPart(const char *entry, Entry e, cdm_ctx *ctx, const cdm_seqdb *db, const cdm_kmer_params *par, cdm_kpart **out, Start start) {
    if (cdmGetenv("CDM_KMER_SORT") || cdmGetenv("CDM_KMER_SORT2")) { cdm_set_error("%s: the A/B switches CDM_KMER_SORT / CDM_KMER_SORT2 apply to the single-device path only", entry); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    const Db d = planDb(db, par->kmer_size, e == Entry::Part);
    const Layout l = chooseLayout(e, d, layoutSwitches());
    if (l == Layout::TooLong) { cdm_set_error("%s: sequences of %u letters or more are not implemented", entry, MAX_SEQ_LETTERS); return CDM_ERR_UNSUPPORTED; }
    cdm_kpart *h = new cdm_kpart();
    h->job = withLayout(l, [&](auto ly) -> KmerJobBase * { auto *j = new KmerJob<decltype(ly)>(ctx, db, par); j->headRange = decltype(ly)::bySlot; return j; });
    h->nSeq = db->n; h->repShift = repShiftOf(d);
    const int rc = start(*h->job);
    if (rc != CDM_OK) { cdm_kpart_free(h); return rc; }
    *out = h;
    return CDM_OK;
}
extern "C" int cdm_kmermatch_part(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_kmer_params *par, int part, int nparts, cdm_kpart **out) {
    if (!ctx || !db || !par || !out || nparts < 1 || part < 0 || part >= nparts) { cdm_set_error("cdm_kmermatch_part: invalid argument"); return CDM_ERR_INVALID; }
    return openPart("cdm_kmermatch_part", Entry::Part, ctx, db, par, out, [&](KmerJobBase &j) { j.part = part; j.nparts = nparts; return j.phaseA(); });
}
// The split by READS of the first half: every rank extracts the k-mers of its own block of sequences (blocks of the (length desc, id asc)
// slot order, so that the blocks concatenated in rank order are that order), the tuples go to the rank of their k-mer range, and sort 1 +
// grouping run there on exactly the tuples cdm_kmermatch_part would have extracted for that range - each sequence is read once per job, not
// once per rank.
extern "C" int cdm_kmermatch_split_begin(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_kmer_params *par, int rank, int nranks, cdm_kpart **out) {
    if (!ctx || !db || !par || !out || nranks < 1 || rank < 0 || rank >= nranks) { cdm_set_error("cdm_kmermatch_split_begin: invalid argument"); return CDM_ERR_INVALID; }
    // the tuples ordered by FINE slices of the k-mer space: the caller cuts the ranks' ranges from all ranks' counts
    return openPart("cdm_kmermatch_split_begin", Entry::SplitBegin, ctx, db, par, out, [&](KmerJobBase &j) { j.part = 0; j.nparts = CDM_KPART_SLICES; j.block = rank; j.nBlocks = nranks; return j.splitBegin(); });
}
extern "C" int cdm_kpart_outgoing(const cdm_kpart *h, uint64_t *offsets, const void **keys, const void **vals, int *valBytes, const void **hashKeys, const void **hashVals, uint64_t *nHash) {
    if (!h || !h->job->split || !offsets || !keys || !vals || !valBytes || !hashKeys || !hashVals || !nHash) { cdm_set_error("cdm_kpart_outgoing: invalid argument"); return CDM_ERR_INVALID; }
    for (int p = 0; p <= CDM_KPART_SLICES; p++) offsets[p] = h->job->sendOff[p];
    *keys = h->job->sendKeys; *vals = h->job->sendVals; *valBytes = h->job->valBytes;
    *hashKeys = h->job->sendHashKeys; *hashVals = h->job->sendHashVals; *nHash = h->job->sendHash;
    return CDM_OK;
}
// does this DB take the wide group key (the representative not in the members' keys)?  The exchange of group keys between ranks
// carries the narrow form only; cdm_kmermatch_dist lets every rank run kmermatcher whole for such a DB.
int cdm_kmermatch_needs_wide_key(const cdm_seqdb *db) {
    return needsWideKey(planDb(db, 0), cdmGetenv("CDM_FORCE_WIDE_KEY") != nullptr) ? 1 : 0;
}
// the k-mer range the handle is to finish as (cdm_kmermatch_dist, small worlds: every rank extracts ALL sequences - split_begin as
// block 0 of 1 - and keeps range `rank` of `nranks`, cut from its own counts)
extern "C" int cdm_kpart_set_range(cdm_kpart *h, int rank, int nranks) {
    if (!h || !h->job->split || nranks < 1 || rank < 0 || rank >= nranks) { cdm_set_error("cdm_kpart_set_range: invalid argument"); return CDM_ERR_INVALID; }
    h->job->block = rank; h->job->nBlocks = nranks;
    return CDM_OK;
}
extern "C" int cdm_kmermatch_split_finish(cdm_ctx *ctx, cdm_kpart *h, const void *keys, const void *vals, uint64_t m, const void *hashKeys, const void *hashVals, uint64_t nHash, int below) {
    if (!ctx || !h || !h->job->split || (m && (!keys || !vals)) || (nHash && (!hashKeys || !hashVals))) { cdm_set_error("cdm_kmermatch_split_finish: invalid argument"); return CDM_ERR_INVALID; }
    h->job->part = h->job->block; h->job->nparts = h->job->nBlocks;          // from here on the handle is rank `part` of `nparts` k-mer ranges, as cdm_kmermatch_part leaves it
    if (nHash && h->job->part != h->job->nparts - 1) { cdm_set_error("cdm_kmermatch_split_finish: the whole-sequence hash tuples belong to the last rank"); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    return h->job->splitFinish(keys, vals, m, hashKeys, hashVals, nHash, below != 0);
}
extern "C" void cdm_kpart_free(cdm_kpart *h) { if (!h) return; delete h->job; delete h; }
extern "C" int cdm_kpart_info(const cdm_kpart *h, uint64_t info[4]) {
    info[0] = h->job->live + h->job->regionTwo; info[1] = h->job->nKept; info[2] = h->job->anyBelow ? 1 : 0; info[3] = h->nSeq;
    return CDM_OK;
}
extern "C" int cdm_kpart_stale(cdm_ctx *ctx, cdm_kpart *h, uint64_t J, uint32_t out[67]) {
    CDM_HIP(hipSetDevice(ctx->device));
    const int rc = h->job->staleTail(J);
    if (rc != CDM_OK) return rc;
    memcpy(out, h->job->staleHost, 67 * sizeof(uint32_t));
    return CDM_OK;
}
// offsets[t] = first gathered group key whose representative is >= bounds[t] (ascending sequence ids; nb of them).  The first call
// groups the keys by representative (run records, their stable sort, the expanding gather), later calls only look bounds up.
extern "C" int cdm_kpart_gather_at(cdm_ctx *ctx, cdm_kpart *h, int nb, const uint64_t *bounds, uint64_t *offsets, const void **devKeys) {
    if (nb < 1 || !bounds || !offsets || !devKeys) { cdm_set_error("cdm_kpart_gather_at: invalid argument"); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    if (!h->gatheredDone) { const int rc = h->job->gatherByRep(); if (rc != CDM_OK) return rc; h->gatheredDone = true; }
    DevBuf<uint64_t> dBound; DevBuf<unsigned long long> dOut;
    if (!dBound.alloc(nb) || !dOut.alloc(nb)) { cdm_set_error("cdm_kpart_gather_at: out of device memory"); return CDM_ERR_HIP; }
    CDM_HIP(hipMemcpyAsync(dBound.p, bounds, (size_t) nb * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_rep_bounds, dim3((nb + 63) / 64), dim3(64), 0, ctx->stream, (const uint64_t *) h->job->gathered, (uint64_t) h->job->nKept, (int) h->repShift, (const uint64_t *) dBound.p, nb, dOut.p);
    std::vector<unsigned long long> o((size_t) nb);
    CDM_HIP(hipMemcpyAsync(o.data(), dOut.p, (size_t) nb * 8, hipMemcpyDeviceToHost, ctx->stream));
    CDM_HIP(hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < nb; t++) offsets[t] = o[t];
    *devKeys = h->job->gathered;
    return CDM_OK;
}
extern "C" int cdm_kpart_gather(cdm_ctx *ctx, cdm_kpart *h, int nranks, uint64_t *offsets, const void **devKeys) {
    if (nranks < 1 || !offsets || !devKeys) { cdm_set_error("cdm_kpart_gather: invalid argument"); return CDM_ERR_INVALID; }
    std::vector<uint64_t> bound((size_t) nranks + 1);
    for (int r = 0; r <= nranks; r++) bound[r] = (uint64_t) ((unsigned __int128) h->nSeq * (unsigned) r / (unsigned) nranks);
    if (int rc = cdm_kpart_gather_at(ctx, h, nranks + 1, bound.data(), offsets, devKeys)) return rc;
    offsets[nranks] = h->job->nKept;
    return CDM_OK;
}
extern "C" int cdm_kpart_sort(cdm_ctx *ctx, cdm_kpart *h, const void *devKeys, uint64_t nKeys, uint32_t *head, uint64_t info[2]) {
    if (!head || !info || (nKeys && !devKeys)) { cdm_set_error("cdm_kpart_sort: invalid argument"); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    return h->job->sortFrom((const uint64_t *) devKeys, nKeys, head, info);
}
extern "C" int cdm_kpart_vote(cdm_ctx *ctx, cdm_kpart *h, const uint32_t *cont, const uint32_t *stale, cdm_hits **out) {
    if (!out || !stale) { cdm_set_error("cdm_kpart_vote: invalid argument"); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    return h->job->voteWith(cont, stale, out);
}
extern "C" int cdm_kpart_cont_cap(void) { return CONT_CAP; }
extern "C" int cdm_kmer_slot_split(int k, int *low_bits) {
    if (!low_bits) { cdm_set_error("cdm_kmer_slot_split: invalid argument"); return CDM_ERR_INVALID; }
    Db d; d.n = 1; d.maxLen = 64; d.residues = 64; d.k = k;      // (a DB of one length that the layout serves at this k, if any k-mer size does)
    if (!slotLayoutFits(d)) { cdm_set_error("cdm_kmer_slot_split: the slot layout takes 14 <= k <= 20 (got %d)", k); return CDM_ERR_INVALID; }
    return slotSplit(k, *low_bits);
}
extern "C" int cdm_dev_copy(cdm_ctx *ctx, void *dst, const void *src, uint64_t bytes) {
    CDM_HIP(hipSetDevice(ctx->device));
    if (bytes) CDM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    CDM_HIP(hipStreamSynchronize(ctx->stream));
    return CDM_OK;
}

int cdm_kmermatch_impl(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_kmer_params *par, cdm_hits **out) { return cdm_kmermatch_ranks_impl(ctx, db, par, nullptr, out); }
// ranks != NULL: kmermatcher's first half split over the ranks by ranges of the k-mer space, the whole hit set on every rank (the passes
// path above; csrc/dist.hip cuts the owned view out of it)
int cdm_kmermatch_ranks_impl(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_kmer_params *par, const KmerRanks *ranks, cdm_hits **out) {
    // the layout ladder of kmer_plan.h (CDM_KMER_LAYOUT=wide|packed|slot pins one, tests); one length throughout (reads straight from a
    // sequencer, the bench's 50 M x 100 bp): 8-byte tuples through sort 1 (LayoutSlot)
    const Db d = planDb(db, par->kmer_size, true);
    const Layout l = chooseLayout(Entry::Single, d, layoutSwitches(), ranks != nullptr);
    switch (l) {
        case Layout::PackedUnfit: cdm_set_error("cdm_kmermatch: CDM_KMER_LAYOUT=packed needs 2k + 1 + 2 x length bits <= 63 (k %d, max length %u)", d.k, db->maxLen); return CDM_ERR_INVALID;
        case Layout::BadSwitch: cdm_set_error("cdm_kmermatch: CDM_KMER_LAYOUT must be wide, packed or slot"); return CDM_ERR_INVALID;
        case Layout::SlotUnfit: cdm_set_error("cdm_kmermatch: CDM_KMER_LAYOUT=slot needs sequences of one length (at least k letters), fewer than 2^32 k-mer slots and 14 <= k <= 20"); return CDM_ERR_INVALID;
        case Layout::TooLong: cdm_set_error("cdm_kmermatch: sequences of %u letters or more are not implemented", MAX_SEQ_LETTERS); return CDM_ERR_UNSUPPORTED;
        default: break;
    }
    return withLayout(l, [&](auto ly) { return kmermatchT<decltype(ly)>(ctx, db, par, out, ranks, d); });
}
