// ancient_correction on the device.
//
// Replaces the OpenMP loop of doCorrection (src/assembler/correction.cpp:200-476) and mostLikeliBaseRead (:7-123).
// One wavefront (64 lanes) owns one query that has more than one alignment record; queries with only their self
// alignment have coverage <= 1 everywhere and keep their bases (:418-420) -- for them the output DB is a plain copy.
//
// Per query the wave runs three passes over the query's alignment records (CSR slice):
//   pass 0  avCov = sum(alnLength) / qLen                                              (:218-245)
//   pass 1  per record, all 64 lanes over the aligned columns: RY-space identity (nuclassembleUtil.cpp:78-92), the
//           rymer threshold (:297-301), the right/left/inside class gate (:311-322) and the pile-up gate (:359).
//           The accept bit goes to a scratch byte per record.
//   pass 2  per chunk of 64 query positions (lane = position): pile up the accepted targets into 44 (tBase, damage
//           class) counters per position (:361-385), held in LDS as counter[slot][lane] = total | reverse << 16,
//           then call the base: coverage <= 1 keeps the base, otherwise arg-max over four log-likelihoods that are
//           accumulated in software x87 extended precision in the reference's term order (:80-122), so ties and
//           near-ties resolve exactly as `long double` does on the host.
// All logs come from host-built tables (DamageLut) staged in LDS.
#include "common.h"
#include "devutil.h"

namespace {

struct CorrectArgs {
    MetaWoff woff; MetaLen len; MetaHasN hasN; MetaExt ext; MetaRaw hasRaw;      // per-sequence metadata, one record per sequence
    const uint32_t *codes, *nmask; const uint8_t *raw; uint8_t *outRaw;      // raw: original letters (general kernel only), or NULL
    const uint64_t *aoff;
    const AlnRec *rec;
    const uint16_t *ry;       // purine/pyrimidine mismatches per record from cdm_rescore (0xFFFF = count here), or NULL
    const uint32_t *active;
    const unsigned int *nActive;
    uint8_t *accept;          // [alignment count] scratch
    unsigned int *errFlag;    // (unused: the general kernel's counters are 64 bit)
    uint32_t *outCodes, *outNmask;
    const DamageLut *lut;
    float seqIdThr, corrRy;
    uint32_t stagePool;       // fast kernels: usable words of the stage pool (CDM_CORRECT_STAGE_POOL; clamped to the instance's POOL)
    unsigned long long *stats;        // CDM_CORRECT_STATS: [0] accepted records, [1] of them with N in the target, [2] longer than STAGE_WORDS, [3] past the pool; or NULL
};

constexpr int WAVES_PER_BLOCK = 2;      // general kernel: 64-bit counters (any number of records piles up), 22.5 KB of LDS per wave
constexpr int SLOTS = 44;

__device__ __forceinline__ uint32_t alnLength(const AlnRec &r) {   // Matcher::computeAlnLength, M/alignment/Matcher.cpp:204-206
    int a = abs(r.qEnd - r.qStart), b = abs(r.dbEnd - r.dbStart);
    return (uint32_t) max(a, b) + 1u;
}
// oriented copy of a record (correction.cpp:229-242)
struct Oriented { int qs, qe, ds, de; bool rev; };
__device__ __forceinline__ Oriented orient(const AlnRec &r, uint32_t dbLen) {
    Oriented o;
    if (r.qStart > r.qEnd) { o.qs = r.qEnd; o.qe = r.qStart; o.ds = (int) dbLen - r.dbEnd - 1; o.de = (int) dbLen - r.dbStart - 1; o.rev = true; }
    else { o.qs = r.qStart; o.qe = r.qEnd; o.ds = r.dbStart; o.de = r.dbEnd; o.rev = false; }
    return o;
}
// base of the oriented target (reverse complement when rev), with N -> 'A' (0) as nucleotideMap/ryMap do for any
// letter outside ACGT; getNuclRevFragment maps X to 'N', which those maps also send to 0 (nuclassembleUtil.cpp:67-76)
__device__ __forceinline__ uint32_t targetBase(const CorrectArgs &a, uint32_t tw, uint32_t tLen, bool tHasN, bool rev, uint32_t tpos) {
    uint32_t p = rev ? (tLen - 1u - tpos) : tpos;
    uint32_t c = cdm_base(a.codes, tw, p);
    if (tHasN && cdm_isN(a.nmask, tw, p)) return 0u;
    return rev ? (3u - c) : c;
}
// the same for a target that may carry letters beyond ACGTN (general kernel): forward, nucleotideMap[original byte] ('c' is 0);
// reversed, the complement of what NucleotideMatrix maps the letter to ('c' -> G), as getNuclRevFragment spells it
__device__ __forceinline__ uint32_t targetBaseRaw(const CorrectArgs &a, uint32_t t, uint32_t tw, uint32_t tLen, bool tHasN, bool rev, uint32_t tpos) {
    if (tHasN && !rev && a.raw && a.hasRaw[t]) return cdm_raw_base(cdm_raw_at(a.raw, tw, tpos));
    return targetBase(a, tw, tLen, tHasN, rev, tpos);
}

// exact arg-max in software x87, one accumulator at a time (keeps the register footprint of the callers small)
template <typename F>
__device__ __noinline__ uint32_t callBaseExact(const double *lt, const double *lq, const double *sLogD, F counts, uint64_t mask) {
    X87 bestAcc = x87_zero(); int best = 0;
    for (int qq = 0; qq < 4; qq++) {
        X87 acc = x87_zero();
#pragma unroll 1
        for (uint64_t m = mask; m; m &= m - 1) {        // ascending slots, the reference's loop order (:60-110)
            const int slot = __ffsll((unsigned long long) m) - 1;
            const uint64_t v = counts(slot);
            const int c = (int) (uint32_t) v, nr = (int) (v >> 32);
            if (c == 0) continue;
            const int tb = slot / 11, l = slot - tb * 11;
            const double base2 = __dadd_rn(lt[tb], lq[qq]);
            const double f = __dadd_rn(base2, sLogD[((0 * 11 + l) * 4 + qq) * 4 + tb]);
            const double g = __dadd_rn(base2, sLogD[((1 * 11 + l) * 4 + qq) * 4 + tb]);
            acc = x87_add(acc, x87_from_double(__dmul_rn((double) (c - nr), f)));
            acc = x87_add(acc, x87_from_double(__dmul_rn((double) nr, g)));
        }
        if (qq == 0 || x87_lt(bestAcc, acc)) { bestAcc = acc; best = qq; }   // first maximum wins (:119-122)
    }
    return (uint32_t) best;
}

// mostLikeliBaseRead (src/assembler/correction.cpp:7-123) for one query position.  counts(slot) returns
// total | (uint64) reverse << 32 for slot = tBase * 11 + damage class; mask has a bit for every slot that may be non-zero (a pile-up
// touches a handful of the 44).  keep is set when coverage <= 1 (:418-420).
constexpr uint64_t ALL_SLOTS = (1ull << 44) - 1ull;
template <typename F>
__device__ __forceinline__ uint32_t callBase(const double *sLogT, const double *sLogQ, const double *sLogD, uint32_t qb, uint32_t p, uint32_t qLen,
                                             bool qWasExt, F counts, uint64_t mask, bool &keep, uint32_t cov4 = ~0u) {
    // cov4: records per target base, 8 bits each (callers with at most 64 records count them while piling up); ~0 = sum the slots here
    uint32_t cov[4];
    if (cov4 == ~0u) {
        cov[0] = cov[1] = cov[2] = cov[3] = 0;
#pragma unroll 1
        for (uint64_t m = mask; m; m &= m - 1) {
            const int slot = __ffsll((unsigned long long) m) - 1;
            const uint32_t c = (uint32_t) counts(slot);
            const int tb = slot / 11;
            cov[0] += tb == 0 ? c : 0u; cov[1] += tb == 1 ? c : 0u; cov[2] += tb == 2 ? c : 0u; cov[3] += tb == 3 ? c : 0u;
        }
    } else { cov[0] = cov4 & 0xFFu; cov[1] = (cov4 >> 8) & 0xFFu; cov[2] = (cov4 >> 16) & 0xFFu; cov[3] = cov4 >> 24; }
    const uint32_t total = cov[0] + cov[1] + cov[2] + cov[3];
    keep = total <= 1;
    if (keep) return qb;
    if (!qWasExt) {
        // :27-33 compares double(cov) / double(total) with 0.4.  In integers: a / b >= 2 / 5.  The double 0.4 lies 2.2e-17 above 2/5, less
        // than half an ulp, so the rounded quotient of a / b == 2/5 IS that double (>= holds); any other a / b with b < 2^18 is further
        // than 1 / (5 b) > 7e-7 from 2/5, far beyond the rounding - the two tests agree on every input.
        if (5u * cov[3] >= 2u * total || 5u * cov[0] >= 2u * total) return qb;
    }
    int qcls;
    if (qWasExt) qcls = 11;
    else if (p < 5) qcls = (int) p;
    else if (p >= qLen - 5) qcls = 11 - (int) (qLen - p);
    else qcls = 5;
    const double *lq = &sLogQ[(qcls * 4 + qb) * 4];
    const double *lt = &sLogT[qb * 4];
    // ---- decision in plain double first.  All addends are <= 0, so each of the four sums (at most 88 addends) differs from
    // the reference's long double sum by less than 88 * 2^-52 * |sum|; when the largest sum beats every other one by more
    // than that, the long double arg-max is the same and the extended-precision emulation is skipped.  Near ties and exact
    // ties (the first maximum wins) go through callBaseExact.
    double sd[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (uint64_t m = mask; m; m &= m - 1) {
        const int slot = __ffsll((unsigned long long) m) - 1;
        const uint64_t v = counts(slot);
        const int c = (int) (uint32_t) v, nr = (int) (v >> 32);
        if (c == 0) continue;
        const int tb = slot / 11, l = slot - tb * 11;
#pragma unroll
        for (int qq = 0; qq < 4; qq++) {
            const double base2 = __dadd_rn(lt[tb], lq[qq]);
            const double f = __dadd_rn(base2, sLogD[((0 * 11 + l) * 4 + qq) * 4 + tb]);
            const double g = __dadd_rn(base2, sLogD[((1 * 11 + l) * 4 + qq) * 4 + tb]);
            sd[qq] = __dadd_rn(sd[qq], __dmul_rn((double) (c - nr), f));
            sd[qq] = __dadd_rn(sd[qq], __dmul_rn((double) nr, g));
        }
    }
    int bestD = 0;
#pragma unroll
    for (int qq = 1; qq < 4; qq++) if (sd[bestD] < sd[qq]) bestD = qq;
    bool clear = true;
#pragma unroll
    for (int qq = 0; qq < 4; qq++)
        if (qq != bestD) clear = clear && (sd[bestD] - sd[qq] > 1e-12 * (fabs(sd[bestD]) + fabs(sd[qq])) + 1e-300);
    if (clear) return (uint32_t) bestD;
    return callBaseExact(lt, lq, sLogD, counts, mask);
}

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_correct(CorrectArgs a) {
    __shared__ double sLogT[16], sLogQ[12 * 16], sLogD[2 * 11 * 16];
    __shared__ uint64_t sCnt[WAVES_PER_BLOCK][SLOTS][64];       // total | reverse << 32
    for (int i = threadIdx.x; i < 16; i += blockDim.x) sLogT[i] = (&a.lut->logT[0][0])[i];
    for (int i = threadIdx.x; i < 12 * 16; i += blockDim.x) sLogQ[i] = (&a.lut->logQ[0][0][0])[i];
    for (int i = threadIdx.x; i < 2 * 11 * 16; i += blockDim.x) sLogD[i] = (&a.lut->logD[0][0][0][0])[i];
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned int nAct = *a.nActive;
    uint64_t (*cnt)[64] = sCnt[wave];

    for (unsigned int item = blockIdx.x * WAVES_PER_BLOCK + wave; item < nAct; item += gridDim.x * WAVES_PER_BLOCK) {
        const uint32_t q = a.active[item];
        const uint32_t qLen = a.len[q], qw = a.woff[q];
        const bool qHasN = a.hasN[q] != 0;
        const bool qRaw = qHasN && a.raw && a.hasRaw[q] != 0;
        const bool qWasExt = a.ext[q] != 0;
        const uint64_t r0 = a.aoff[q], r1 = a.aoff[q + 1];

        // ---- pass 0: average coverage (float sum of small integers: exact, order independent)
        int sumLen = 0;
        for (uint64_t r = r0 + lane; r < r1; r += 64) sumLen += (int) alnLength(a.rec[r]);
        sumLen = cdm_wave_sum(sumLen);
        const float avCov = static_cast<float>(static_cast<float>(sumLen)) / qLen;

        // ---- pass 1: gates
        for (uint64_t r = r0; r < r1; r++) {
            const AlnRec rec = a.rec[r];
            const uint32_t t = rec.target;
            const uint32_t tLen = a.len[t], tw = a.woff[t];
            const bool tHasN = a.hasN[t] != 0;
            const uint32_t aLen = alnLength(rec);
            const Oriented o = orient(rec, tLen);
            bool ok = a.ext[t] == 0;                              // target must be a read (:280-284)
            int mism = 0;
            const uint32_t preRy = a.ry ? a.ry[r] : 0xFFFFu;
            if (ok && preRy != 0xFFFFu) mism = (int) preRy;         // counted by cdm_rescore on the same columns
            if (ok) {
                if (preRy == 0xFFFFu) {
                for (uint32_t c = lane; c < aLen; c += 64) {
                    uint32_t qb = cdm_base(a.codes, qw, o.qs + c);
                    if (qHasN && cdm_isN(a.nmask, qw, o.qs + c)) qb = 0;
                    if (qRaw) qb = cdm_raw_base(cdm_raw_at(a.raw, qw, o.qs + c));
                    uint32_t tb = targetBaseRaw(a, t, tw, tLen, tHasN, o.rev, o.ds + c);
                    mism += ((qb & 1u) != (tb & 1u));             // RY class = low bit of the A,C,G,T = 0..3 code
                }
                mism = cdm_wave_sum(mism);
                }
                const float ryId = static_cast<float>(aLen - (uint32_t) mism) / static_cast<float>(aLen);
                float thr = a.corrRy;
                if (aLen <= 100) { thr = (static_cast<float>(aLen) - 1) / static_cast<float>(aLen); thr = floorf(thr * 1000) / 1000; }
                const bool ry = ryId >= thr;
                const bool right = o.ds == 0 && (uint32_t) o.qe == (qLen - 1);
                const bool left = o.qs == 0 && (uint32_t) o.de == (tLen - 1);
                const bool cls = right || left || (avCov < 50);
                ok = ry && cls && rec.seqId >= a.seqIdThr && aLen >= 30;
            }
            if (lane == 0) __hip_atomic_store(&a.accept[r], (uint8_t) (ok ? 1 : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // accept[] is read back by this same wave below: drain the stores, and read with agent-scope (L1-bypassing) loads
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __builtin_amdgcn_wave_barrier();

        // ---- pass 2: pile-up + call, 64 positions at a time
        const uint32_t lastWord = (qLen + 15) / 16;
        for (uint32_t base = 0; base < qLen; base += 64) {
            const uint32_t p = base + lane;
#pragma unroll 4
            for (int s = 0; s < SLOTS; s++) cnt[s][lane] = 0;
            for (uint64_t r = r0; r < r1; r++) {
                if (!__hip_atomic_load(&a.accept[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) continue;
                const AlnRec rec = a.rec[r];
                const uint32_t t = rec.target, tLen = a.len[t], tw = a.woff[t];
                const Oriented o = orient(rec, tLen);
                if ((uint32_t) o.qe < base || (uint32_t) o.qs >= base + 64) continue;   // wave uniform
                if (p >= (uint32_t) o.qs && p <= (uint32_t) o.qe && p < qLen) {
                    const uint32_t tpos = (uint32_t) o.ds + (p - (uint32_t) o.qs);
                    const uint32_t tb = targetBaseRaw(a, t, tw, tLen, a.hasN[t] != 0, o.rev, tpos);
                    const uint32_t cls = tpos < 5 ? tpos : (tpos >= tLen - 5 ? 6 + (tpos - (tLen - 5)) : 5);
                    cnt[tb * 11 + cls][lane] += 1ull + (o.rev ? (1ull << 32) : 0ull);
                }
            }
            // ---- call
            uint32_t newCode = 0; bool keep = true;
            if (p < qLen) {
                uint32_t qb = cdm_base(a.codes, qw, p);
                const bool qIsN = qHasN && cdm_isN(a.nmask, qw, p);
                if (qIsN) qb = 0;
                const uint32_t mapped = qb;
                uint8_t orig = 0;
                if (qRaw) { orig = cdm_raw_at(a.raw, qw, p); qb = cdm_raw_base(orig); }
                newCode = callBase(sLogT, sLogQ, sLogD, qb, p, qLen, qWasExt, [&](int slot) { return cnt[slot][lane]; }, ALL_SLOTS, keep);
                if (qRaw) {     // coverage <= 1 keeps the original byte (:418-420) and with it what the letter maps to
                    if (keep) newCode = mapped;
                    a.outRaw[(uint64_t) qw * 16u + p] = keep ? orig : (uint8_t) "ACGT"[newCode];
                }
            }
            // ---- write 64 positions = 4 code words (+ N bits): lanes 0..3 assemble one word each from ballots
            const uint64_t b0 = cdm_ballot((newCode & 1u) != 0), b1 = cdm_ballot((newCode & 2u) != 0);
            uint64_t nb = 0;
            if (qHasN) nb = cdm_ballot(p < qLen && keep && cdm_isN(a.nmask, qw, p));
            if (lane < 4) {
                const uint32_t w = (base >> 4) + lane;
                if (w < lastWord) {
                    const uint32_t lo = (uint32_t) (b0 >> (16 * lane)), hi = (uint32_t) (b1 >> (16 * lane));
                    a.outCodes[qw + w] = cdm_spread16(lo) | (cdm_spread16(hi) << 1);
                    if (qHasN) reinterpret_cast<uint16_t *>(a.outNmask)[qw + w] = (uint16_t) (nb >> (16 * lane));
                }
            }
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// Fast kernel for queries with at most 64 alignment records (all but the heaviest pile-ups): lane = record in the gate
// phase (RY identity on 16-base words, XOR + popcount) and keeps the record, lane = position in the pile-up.
// Same arithmetic as k_correct; 8-bit (4-bit) pile-up counters (a slot cannot exceed the 64 (15) records).
constexpr int FAST_WAVES = 4;
// Target words staged in LDS (lane = record loads the words its aligned span covers, all records at once): the pile-up then takes
// its letters from LDS instead of one dependent global load per record and 64 positions.  A record of up to STAGE_WORDS words (12
// hold a span of 177 columns wherever it starts) is staged; longer spans and targets with N keep the global path.
constexpr int STAGE_WORDS = 12;
// The stage is a pool of POOL words per wave, cut up per query: an exclusive wave scan over the word counts of the accepted records
// gives each its offset, and a record whose words end past the pool keeps the global path like the long ones (which records land in
// the pool never shows in a result).  A 100-column span takes 7 or 8 words and rejected records take none, so a pool far below
// records * STAGE_WORDS holds nearly every accepted record - and the LDS it frees is what lets a fifth block onto the CU.
constexpr size_t FAST_TABLE_BYTES = (16 + 12 * 16 + 2 * 11 * 16) * sizeof(double);
template <typename CT> constexpr size_t fastCntWords() { return (size_t) SLOTS * (64 / (4 / sizeof(CT))); }
template <typename CT> constexpr size_t fastLdsBytes(size_t pool) { return FAST_TABLE_BYTES + (size_t) FAST_WAVES * 4 * (fastCntWords<CT>() + pool); }
// what the CU takes for a block: its LDS is handed out in CU_LDS_GRANULE steps, so that is what MINW blocks have to fit with
constexpr size_t ldsAllocBytes(size_t bytes) { return (bytes + CU_LDS_GRANULE - 1) / CU_LDS_GRANULE * CU_LDS_GRANULE; }
// POOL: the 15-record instance keeps 16 * STAGE_WORDS (its LDS is small either way); the 64-record one gets the most words with which
// MINW blocks still fit the CU, at most 64 * STAGE_WORDS (every record at full length, what MINW = 4 comes to)
template <int MAXREC, typename CT, int MINW> constexpr int fastPoolWords() {
    if (MAXREC != 64) return 16 * STAGE_WORDS;
    const size_t perBlock = CU_LDS_BYTES / MINW / CU_LDS_GRANULE * CU_LDS_GRANULE, fixed = fastLdsBytes<CT>(0);
    if (perBlock <= fixed) return 0;
    const size_t w = (perBlock - fixed) / (FAST_WAVES * 4);
    return (int) (w < (size_t) 64 * STAGE_WORDS ? w : (size_t) 64 * STAGE_WORDS);
}
// Inclusive sum over the lanes 0 .. RECORDS - 1 of a wave (the others hold 0) on the DPP path: four shifts inside the rows of 16 lanes,
// then the last lane of a row handed to the next row, and lane 31 to the upper two rows.  (A lane whose source lies outside its row, or
// whose row is masked out, keeps the 0 it is given.)  Six VALU steps; the same through __shfl_up is six trips through the LDS crossbar.
template <int RECORDS> __device__ __forceinline__ uint32_t waveInclusiveSum(uint32_t v) {
    int x = (int) v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);      // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);      // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);      // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);      // row_shr:8
    if (RECORDS > 16) {
        x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
        x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
    }
    return (uint32_t) x;
}
// SPLIT pile-up: the two mask words of column col (0..63) in the counter rows of the slots 5, 16, 27 and 38 (32 words each, 16 columns to a row)
__device__ __forceinline__ uint32_t endMaskWord(uint32_t col) { const uint32_t t = col & 0x30u; return 5u * 32u + 2u * col + (t << 4) + (t << 2); }
constexpr uint64_t INTERIOR_SLOTS = (1ull << 5) | (1ull << 16) | (1ull << 27) | (1ull << 38);
constexpr uint32_t NOT_STAGED = 0x80000000u;        // no offset - first word comes near it (offsets < POOL, word indices < 2^26)

// MAXREC: most records of a query on this instance (64, or 15 with CT = uint8_t: two 4-bit fields per counter and a quarter of the
// record slots - less LDS per block, more waves per CU; the kernel is bound by the latency of its dependent gathers, so the
// occupancy is what it runs on).  MINW: waves per SIMD (= blocks per CU) the register allocation has to leave room for.
//
// SPLIT: the pile-up by damage class.  All columns of a record but the five at each end of its target are class 5, so their counts
// are kept per lane (= column) in two registers, forward and reverse records, with one 8-bit field per target base (at most 64
// records: no carries).  The loop over the staged records of one strand is then a range test, the letter and one shifted add; the
// strand is a constant of the loop (a reverse record adds to field 3 - stored letter and walks its words downwards).  The at most ten
// end columns of a record go to the LDS counters with one lane per record and end, one step per class.  The four counter rows of the slots
// tb * 11 + 5 hold no counts then: they are the 64 x 2 words of a per-column mask of the end slots that the record lanes mark and the
// column's lane reads at the call (which is why SPLIT needs 16-bit counters: four rows of 32 words).  Records outside the stage keep
// a loop with lane = column and letters from global memory that feeds the same registers and counters.
template <int MAXREC, typename CT, int MINW, bool SPLIT>
__global__ __launch_bounds__(64 * FAST_WAVES, MINW) void k_correct_fast(CorrectArgs a, const uint32_t *__restrict__ list, const unsigned int *__restrict__ nList) {
    constexpr int HB = sizeof(CT) * 4;                  // bits per field: total | reverse << HB
    constexpr int PER = 4 / sizeof(CT);                 // counters per LDS dword
    constexpr int POOL = fastPoolWords<MAXREC, CT, MINW>();
    static_assert(!SPLIT || (PER == 2 && MAXREC <= 64), "the end mask takes 64 x 2 words: the four interior rows of 16-bit counters");
    static_assert(POOL >= STAGE_WORDS && (size_t) MINW * ldsAllocBytes(fastLdsBytes<CT>(POOL)) <= CU_LDS_BYTES,
                  "the launch bound asks for more blocks per CU than the kernel's LDS lets run: the compiler would drop the request");
    __shared__ double sLogT[16], sLogQ[12 * 16], sLogD[2 * 11 * 16];
    __shared__ uint32_t sCnt[FAST_WAVES][SLOTS * (64 / PER)];      // counter [slot][lane], PER lanes to a word
    __shared__ uint32_t sStage[FAST_WAVES][POOL];
    static_assert(sizeof(sLogT) + sizeof(sLogQ) + sizeof(sLogD) + sizeof(sCnt) + sizeof(sStage) == fastLdsBytes<CT>(POOL), "fastLdsBytes() is not what the kernel declares");
    for (int i = threadIdx.x; i < 16; i += blockDim.x) sLogT[i] = (&a.lut->logT[0][0])[i];
    for (int i = threadIdx.x; i < 12 * 16; i += blockDim.x) sLogQ[i] = (&a.lut->logQ[0][0][0])[i];
    for (int i = threadIdx.x; i < 2 * 11 * 16; i += blockDim.x) sLogD[i] = (&a.lut->logD[0][0][0][0])[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned int nItems = *nList;
    // the pile-up adds to a counter with ONE LDS atomic on the word that holds it (the lanes that share the word are serialised by
    // the LDS): word index of this lane's counter inside a slot row, and the lane's increments shifted to its place in the word
    uint32_t *cntWords = sCnt[wave], *stage = sStage[wave];
    const uint32_t laneWord = (uint32_t) lane / PER, laneShift = ((uint32_t) lane % PER) * (8 * sizeof(CT));
    const uint32_t incFwd = 1u << laneShift, incRev = (1u | (1u << HB)) << laneShift;
    const uint32_t laneClear = ~((uint32_t) (CT) ~(CT) 0 << laneShift);
    const uint32_t pool = min(a.stagePool, (uint32_t) POOL);
    for (int s = lane; s < SLOTS * (64 / PER); s += 64) cntWords[s] = 0;       // a lane clears the slots it touched after every call
    // The chain list -> record offsets + query metadata -> records is walked one query AHEAD: the next query's offsets and metadata are
    // requested at the top of an iteration, its records (one per lane) and their RY counts once the gate of the current query is through,
    // so that they arrive while the pile-up runs.  (Wave-uniform values are moved to scalar registers.)
    const unsigned int stride = gridDim.x * FAST_WAVES;
    unsigned int item = blockIdx.x * FAST_WAVES + wave;
    const SeqMeta *meta = a.len.m;
    auto uni = [](uint32_t v) { return (uint32_t) __builtin_amdgcn_readfirstlane((int) v); };
    uint32_t qCur = 0, qNext = 0; SeqMeta qmCur = {0, 0, 0, 0}; uint64_t r0Cur = 0; uint32_t nRecCur = 0; AlnRec recCur = {}; uint32_t ryCur = 0xFFFFu;
    if (item < nItems) {
        qCur = uni(list[item]); qmCur = meta[qCur]; r0Cur = a.aoff[qCur]; nRecCur = (uint32_t) (a.aoff[qCur + 1] - r0Cur);
        if ((uint32_t) lane < nRecCur) { recCur = a.rec[r0Cur + lane]; if (a.ry) ryCur = a.ry[r0Cur + lane]; }
        if (item + stride < nItems) qNext = uni(list[item + stride]);
    }
    for (; item < nItems; item += stride) {
        const uint32_t q = qCur;
        const uint32_t qLen = uni(qmCur.len), qw = uni(qmCur.woff);
        const bool qHasN = (uni(qmCur.flags) & 1u) != 0, qWasExt = (uni(qmCur.flags) & 2u) != 0;
        const uint64_t r0 = ((uint64_t) uni((uint32_t) (r0Cur >> 32)) << 32) | uni((uint32_t) r0Cur);
        const uint32_t nRec = uni(nRecCur);
        const uint32_t qLast = (qLen + 15) / 16 - 1;
        const bool hasNext = item + stride < nItems;
        const uint32_t qN = qNext;
        SeqMeta qmN = {0, 0, 0, 0}; uint64_t r0N = 0, r1N = 0;
        if (hasNext) { qmN = meta[qN]; r0N = a.aoff[qN]; r1N = a.aoff[qN + 1]; }
        if (item + 2 * stride < nItems) qNext = uni(list[item + 2 * stride]);
        // ---- gate phase, lane = record
        const AlnRec rec = recCur; uint32_t aLen = 0;
        const uint32_t ryOfRec = ryCur;
        const bool have = (uint32_t) lane < nRec;
        if (have) aLen = alnLength(rec);
        const float avCov = static_cast<float>(static_cast<float>(cdm_wave_sum((int) aLen))) / qLen;
        bool ok = false;
        uint32_t iTw = 0, iLenFlags = 0, iQs = 0, iSpan = 0, iDs = 0;     // the record as the pile-up needs it, kept in this lane's registers
        uint32_t iDelta = NOT_STAGED;                                     // staged: stage[iDelta + w] holds word w of the target
        uint32_t w0 = 0, nW = 0; bool tN = false;                         // the span's words on the target as stored (nW = 0: asks for no pool space)
        if (have) {
            const uint32_t t = rec.target, tLen = a.len[t], tw = a.woff[t];
            const bool tHasN = a.hasN[t] != 0;
            const Oriented o = orient(rec, tLen);
            ok = a.ext[t] == 0;
            if (ok) {
                uint32_t mism = ryOfRec;
                if (mism != 0xFFFFu) {
                    // counted by cdm_rescore on the same columns
                } else if (!qHasN && !tHasN) {
                    mism = 0;
                    const uint32_t tLast = (tLen + 15) / 16 - 1;
                    for (uint32_t c = 0; c < aLen; c += 16) {
                        const uint32_t x = cdm_window16(a.codes, qw, (uint32_t) o.qs + c, qLast) ^ cdm_oriented_window16(a.codes, tw, tLen, tLast, o.rev, (uint32_t) o.ds + c);
                        uint32_t mm = x & 0x55555555u;                   // RY class = low bit of the code
                        const uint32_t rem = aLen - c;
                        if (rem < 16) mm &= (1u << (2 * rem)) - 1u;
                        mism += __popc(mm);
                    }
                } else {
                    mism = 0;
                    for (uint32_t c = 0; c < aLen; c++) {
                        uint32_t qb = cdm_base(a.codes, qw, o.qs + c);
                        if (qHasN && cdm_isN(a.nmask, qw, o.qs + c)) qb = 0;
                        const uint32_t tb = targetBase(a, tw, tLen, tHasN, o.rev, o.ds + c);
                        mism += ((qb & 1u) != (tb & 1u));
                    }
                }
                const float ryId = static_cast<float>(aLen - mism) / static_cast<float>(aLen);
                float thr = a.corrRy;
                if (aLen <= 100) { thr = (static_cast<float>(aLen) - 1) / static_cast<float>(aLen); thr = floorf(thr * 1000) / 1000; }
                const bool right = o.ds == 0 && (uint32_t) o.qe == (qLen - 1);
                const bool left = o.qs == 0 && (uint32_t) o.de == (tLen - 1);
                ok = (ryId >= thr) && (right || left || (avCov < 50)) && rec.seqId >= a.seqIdThr && aLen >= 30;
            }
            // sequences on this path are shorter than 2^30 letters (the DB's word offsets are 32 bit)
            iTw = tw; iLenFlags = tLen | (o.rev ? 0x80000000u : 0u) | (tHasN ? 0x40000000u : 0u); iQs = (uint32_t) o.qs; iSpan = (uint32_t) (o.qe - o.qs); iDs = (uint32_t) o.ds;
            tN = tHasN;
            if (ok && !tHasN) {
                const uint32_t fLo = o.rev ? tLen - 1u - (iDs + iSpan) : iDs;       // the span on the target as stored
                w0 = fLo >> 4; nW = ((fLo + iSpan) >> 4) - w0 + 1u;
            }
        }
        const bool fits = nW != 0 && nW <= (uint32_t) STAGE_WORDS;
        const uint32_t end = waveInclusiveSum<MAXREC>(fits ? nW : 0u);       // where this record's words end, if they are all taken
        const bool staged = fits && end <= pool;
        if (staged) {
            const uint32_t off = end - nW;
            for (uint32_t j = 0; j < nW; j++) stage[off + j] = a.codes[iTw + w0 + j];
            iDelta = off - w0;
        }
        const uint64_t okMask = __ballot(ok);
        // SPLIT: the staged records by strand (the strand is a constant of their loops), and the others
        const uint64_t stMask = SPLIT ? __ballot(ok && staged) : 0, revMask = SPLIT ? __ballot((iLenFlags & 0x80000000u) != 0) : 0;
        if (a.stats) {      // (a stats run: not what is timed)
            const uint64_t mN = __ballot(ok && tN), mLong = __ballot(nW > (uint32_t) STAGE_WORDS), mOver = __ballot(fits && !staged);
            if (lane == 0) { atomicAdd(&a.stats[0], (unsigned long long) __popcll(okMask)); atomicAdd(&a.stats[1], (unsigned long long) __popcll(mN));
                             atomicAdd(&a.stats[2], (unsigned long long) __popcll(mLong)); atomicAdd(&a.stats[3], (unsigned long long) __popcll(mOver)); }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // the next query's records, on their way during the pile-up
        qCur = qN; qmCur = qmN; r0Cur = r0N; nRecCur = (uint32_t) (r1N - r0N); ryCur = 0xFFFFu;
        if (hasNext && (uint32_t) lane < nRecCur) { recCur = a.rec[r0N + lane]; if (a.ry) ryCur = a.ry[r0N + lane]; }

        // ---- pile-up + call, 64 positions at a time.  The record fields are wave-uniform: they are read out of the owning lane into
        // scalar registers, the per-lane work is the target letter, its damage class and one LDS add (SPLIT: see above).
        const uint32_t lastWord = (qLen + 15) / 16;
        for (uint32_t base = 0; base < qLen; base += 64) {
            const uint32_t p = base + lane;
            uint64_t touched = 0;       // slots of this lane's column that are non-zero
            uint32_t cov4 = 0;          // records per target base (8 bits each: at most 64 records), counted on the way
            uint32_t inFwd = 0, inRev = 0;      // SPLIT: class 5 records of this lane's column per target base, 8 bits each, by strand
            if constexpr (SPLIT) {
                // the record's interior columns iLo .. iLo + iLen on the query (oriented target positions 5 .. tLen - 6 inside the span;
                // a span of 30 columns or more always has some) and the letter index iC of column iLo: on the target as stored, once
                // staged in sStage as a whole, 16 letters to the word.  A forward record's index goes up with the column, a reverse
                // one's down.  (Made again for every chunk, so that the three are not live through the call.)
                const uint32_t lead = (uint32_t) max(0, 5 - (int) iDs), iLo = iQs + lead, iLen = min(iSpan, (iLenFlags & 0x3FFFFFFFu) - 6u - iDs) - lead;
                const uint32_t iC = ((iLenFlags & 0x80000000u) ? (iLenFlags & 0x3FFFFFFFu) - 1u - (iDs + lead) : iDs + lead) + ((uint32_t) (wave * POOL) + iDelta) * 16u;
                const uint64_t inMask = __ballot(iLo < base + 64u && iLo + iLen >= base) & stMask;
                // ---- the end columns of the staged records, one lane per (record, end).  Up to 32 records: lane l takes the 5' end
                // (target positions 0 .. 4, classes 0 .. 4) of record l & 31 when l < 32 and its 3' end (tLen - 5 .. tLen - 1, classes
                // 6 .. 10) otherwise, five steps in all; more records: lane = record and the two ends one after the other.  The
                // column of a position is qs + tpos - ds, where that lies in the span and in this chunk; position, column and letter
                // index go up (the index of a reverse record down) by one per step.
                uint32_t *const stageAll = &sStage[0][0];
                {
                    const bool halves = nRec <= 32u;
                    const int src = halves ? (lane & 31) : lane;
                    const uint32_t eQs = (uint32_t) __shfl((int) iQs, src), eSpan = (uint32_t) __shfl((int) iSpan, src), eDs = (uint32_t) __shfl((int) iDs, src);
                    const uint32_t eLf = (uint32_t) __shfl((int) iLenFlags, src), eDelta = (uint32_t) __shfl((int) iDelta, src);
                    const uint32_t tLen = eLf & 0x3FFFFFFFu; const bool rev = (eLf & 0x80000000u) != 0;
                    for (uint32_t pass = 0; pass < (halves ? 1u : 2u); pass++) {
                        const bool far = halves ? lane >= 32 : pass != 0;
                        const uint32_t tpos = far ? tLen - 5u : 0u;
                        uint32_t d = tpos - eDs, col = eQs + d - base;            // (either wraps to a large number when below its range)
                        uint32_t f = (rev ? tLen - 1u - tpos : tpos) + ((uint32_t) (wave * POOL) + eDelta) * 16u, cls = far ? 6u : 0u;
                        if (eDelta != NOT_STAGED) {
#pragma unroll
                            for (int step = 0; step < 5; step++) {
                                if (d <= eSpan && col < 64u) {
                                    const uint32_t slot = (__builtin_amdgcn_ubfe(stageAll[f >> 4], f << 1, 2u) ^ (rev ? 3u : 0u)) * 11u + cls;
                                    atomicAdd(&cntWords[slot * 32u + (col >> 1)], (rev ? (1u | (1u << HB)) : 1u) << ((col & 1u) * 16u));
                                    atomicOr(&cntWords[endMaskWord(col) + (slot >> 5)], 1u << (slot & 31u));
                                }
                                d++; col++; cls++; f += rev ? ~0u : 1u;
                            }
                        }
                    }
                }
                // ---- the interior columns of the staged records, lane = column
                for (uint64_t m = inMask & ~revMask; m; m &= m - 1) {
                    const int r = __ffsll((unsigned long long) m) - 1;
                    const uint32_t d = p - (uint32_t) __builtin_amdgcn_readlane((int) iLo, r);
                    if (d <= (uint32_t) __builtin_amdgcn_readlane((int) iLen, r)) {
                        const uint32_t f = (uint32_t) __builtin_amdgcn_readlane((int) iC, r) + d;
                        inFwd += 1u << (__builtin_amdgcn_ubfe(stageAll[f >> 4], f << 1, 2u) << 3);
                    }
                }
                for (uint64_t m = inMask & revMask; m; m &= m - 1) {
                    const int r = __ffsll((unsigned long long) m) - 1;
                    const uint32_t d = p - (uint32_t) __builtin_amdgcn_readlane((int) iLo, r);
                    if (d <= (uint32_t) __builtin_amdgcn_readlane((int) iLen, r)) {
                        const uint32_t f = (uint32_t) __builtin_amdgcn_readlane((int) iC, r) - d;
                        inRev += 0x01000000u >> (__builtin_amdgcn_ubfe(stageAll[f >> 4], f << 1, 2u) << 3);      // field 3 - stored letter
                    }
                }
            }
            // SPLIT: the records outside the stage (lane = column, letters from global memory); otherwise every record
            for (uint64_t m = SPLIT ? __ballot(iQs < base + 64u && iQs + iSpan >= base) & okMask & ~stMask : okMask; m; m &= m - 1) {
                const int r = __ffsll((unsigned long long) m) - 1;
                const uint32_t qs = (uint32_t) __builtin_amdgcn_readlane((int) iQs, r), span = (uint32_t) __builtin_amdgcn_readlane((int) iSpan, r);
                if (qs + span < base || qs >= base + 64) continue;   // wave uniform
                const uint32_t lf = (uint32_t) __builtin_amdgcn_readlane((int) iLenFlags, r), tw = (uint32_t) __builtin_amdgcn_readlane((int) iTw, r);
                const uint32_t ds = (uint32_t) __builtin_amdgcn_readlane((int) iDs, r), tLen = lf & 0x3FFFFFFFu;
                const uint32_t dl = (uint32_t) __builtin_amdgcn_readlane((int) iDelta, r);
                const uint32_t d = p - qs;
                if (d <= span) {
                    const uint32_t tpos = ds + d;                            // position on the oriented target
                    uint32_t tb;
                    if (dl != NOT_STAGED) {
                        const bool rev = (lf & 0x80000000u) != 0;
                        const uint32_t f = rev ? tLen - 1u - tpos : tpos;
                        tb = (stage[dl + (f >> 4)] >> ((f & 15u) * 2u)) & 3u;
                        if (rev) tb = 3u - tb;
                    } else if (lf & 0x40000000u) tb = targetBase(a, tw, tLen, true, (lf & 0x80000000u) != 0, tpos);
                    else if (lf & 0x80000000u) tb = 3u - cdm_base(a.codes, tw, tLen - 1u - tpos);
                    else tb = cdm_base(a.codes, tw, tpos);
                    // damage class 0..4 from the 5' end, 6..10 at the 3' end, 5 inside (accepted records are at least 30 columns long)
                    const uint32_t cls = min(tpos, 5u) + (uint32_t) max((int) tpos - (int) (tLen - 6u), 0);
                    const uint32_t slot = tb * 11u + cls;
                    if (SPLIT && cls == 5u) {
                        if (lf & 0x80000000u) inRev += 1u << (8u * tb); else inFwd += 1u << (8u * tb);
                    } else {
                        atomicAdd(&cntWords[slot * (64 / PER) + laneWord], (lf & 0x80000000u) ? incRev : incFwd);
                        touched |= 1ull << slot;
                        if (!SPLIT) cov4 += 1u << (8u * tb);
                    }
                }
            }
            if constexpr (SPLIT) {
                // the end slots the record lanes marked for this column, their records per target base, and the interior ones
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const uint32_t mw = endMaskWord((uint32_t) lane);
                const uint64_t marked = (uint64_t) cntWords[mw] | ((uint64_t) cntWords[mw + 1] << 32);
                if (marked) { cntWords[mw] = 0; cntWords[mw + 1] = 0; }
                touched |= marked;      // (a slot may have records of both kinds: its counter is read once)
                for (uint64_t m = touched; m; m &= m - 1) {
                    const uint32_t slot = (uint32_t) __ffsll((unsigned long long) m) - 1u;
                    cov4 += ((cntWords[slot * 32u + laneWord] >> laneShift) & 0xFFu) << (8u * (slot / 11u));
                }
                const uint32_t in = inFwd + inRev;
                cov4 += in;
                touched |= ((in & 0xFFu) ? 1ull << 5 : 0) | ((in & 0xFF00u) ? 1ull << 16 : 0) | ((in & 0xFF0000u) ? 1ull << 27 : 0) | ((in >> 24) ? 1ull << 38 : 0);
            }
            uint32_t newCode = 0; bool keep = true;
            if (p < qLen) {
                uint32_t qb = cdm_base(a.codes, qw, p);
                const bool qIsN = qHasN && cdm_isN(a.nmask, qw, p);
                if (qIsN) qb = 0;
                newCode = callBase(sLogT, sLogQ, sLogD, qb, p, qLen, qWasExt,
                                   [=](int slot) {
                                       if constexpr (SPLIT) {
                                           const int tb = slot / 11;
                                           if (slot - tb * 11 == 5) return (uint64_t) (((inFwd + inRev) >> (8 * tb)) & 0xFFu) | ((uint64_t) ((inRev >> (8 * tb)) & 0xFFu) << 32);
                                       }
                                       const uint32_t v = cntWords[slot * (64 / PER) + laneWord] >> laneShift; return (uint64_t) (v & ((1u << HB) - 1u)) | ((uint64_t) ((v >> HB) & ((1u << HB) - 1u)) << 32); },
                                   touched, keep, cov4);
            }
            // (SPLIT: the interior slots have no counter - their rows hold the mask words, cleared above)
            for (uint64_t m = SPLIT ? touched & ~INTERIOR_SLOTS : touched; m; m &= m - 1) atomicAnd(&cntWords[(__ffsll((unsigned long long) m) - 1) * (64 / PER) + laneWord], laneClear);
            if constexpr (SPLIT) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }
            const uint64_t b0 = cdm_ballot((newCode & 1u) != 0), b1 = cdm_ballot((newCode & 2u) != 0);
            uint64_t nb = 0;
            if (qHasN) nb = cdm_ballot(p < qLen && keep && cdm_isN(a.nmask, qw, p));
            if (lane < 4) {
                const uint32_t w = (base >> 4) + lane;
                if (w < lastWord) {
                    const uint32_t lo = (uint32_t) (b0 >> (16 * lane)), hi = (uint32_t) (b1 >> (16 * lane));
                    a.outCodes[qw + w] = cdm_spread16(lo) | (cdm_spread16(hi) << 1);
                    if (qHasN) reinterpret_cast<uint16_t *>(a.outNmask)[qw + w] = (uint16_t) (nb >> (16 * lane));
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// queries with more than one alignment record: up to smallMax records -> small list, up to 64 -> fast list, more -> general list
__global__ void k_mark_active(const uint64_t *__restrict__ aoff, uint32_t n, uint32_t smallMax, uint32_t *__restrict__ active, uint32_t *__restrict__ activeFast,
                              uint32_t *__restrict__ activeSmall, unsigned int *__restrict__ counters) {
    uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t c = (q < n) ? aoff[q + 1] - aoff[q] : 0;
    const uint32_t s0 = cdm_wave_append(&counters[0], c > 64), s2 = cdm_block_append(&counters[2], c > smallMax && c <= 64), s3 = cdm_block_append(&counters[3], c > 1 && c <= smallMax);
    if (c > 64) active[s0] = q; else if (c > smallMax) activeFast[s2] = q; else if (c > 1) activeSmall[s3] = q;
}


// the same for a DB with letters beyond ACGTN: a query that carries such letters, or one of whose targets does, goes to the general kernel
__global__ void k_mark_active_raw(const uint64_t *__restrict__ aoff, const AlnRec *__restrict__ rec, const uint8_t *__restrict__ hasN, uint32_t n, uint32_t smallMax,
                                  uint32_t *__restrict__ active, uint32_t *__restrict__ activeFast, uint32_t *__restrict__ activeSmall, unsigned int *__restrict__ counters) {
    uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t c = (q < n) ? aoff[q + 1] - aoff[q] : 0;
    if (c > 1 && c <= 64) {
        bool odd = (hasN[q] & 2u) != 0;
        for (uint64_t r = aoff[q]; r < aoff[q + 1] && !odd; r++) odd = (hasN[rec[r].target] & 2u) != 0;
        if (odd) c = 65;
    }
    const uint32_t s0 = cdm_wave_append(&counters[0], c > 64), s2 = cdm_block_append(&counters[2], c > smallMax && c <= 64), s3 = cdm_block_append(&counters[3], c > 1 && c <= smallMax);
    if (c > 64) active[s0] = q; else if (c > smallMax) activeFast[s2] = q; else if (c > 1) activeSmall[s3] = q;
}


// test hook: one thread per count vector {qBase, qIter, qLen, wasCorr, 44 x (total | reverse << 16)}
__global__ void k_debug_call(const DamageLut *lut, const uint32_t *vec, uint32_t n, uint8_t *out) {
    __shared__ double sLogT[16], sLogQ[12 * 16], sLogD[2 * 11 * 16];
    for (int i = threadIdx.x; i < 16; i += blockDim.x) sLogT[i] = (&lut->logT[0][0])[i];
    for (int i = threadIdx.x; i < 12 * 16; i += blockDim.x) sLogQ[i] = (&lut->logQ[0][0][0])[i];
    for (int i = threadIdx.x; i < 2 * 11 * 16; i += blockDim.x) sLogD[i] = (&lut->logD[0][0][0][0])[i];
    __syncthreads();
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *v = vec + (size_t) i * 48;
    bool keep;
    out[i] = (uint8_t) callBase(sLogT, sLogQ, sLogD, v[0], v[1], v[2], v[3] != 0, [&](int slot) { const uint32_t x = v[4 + slot]; return (uint64_t) (x & 0xFFFFu) | ((uint64_t) (x >> 16) << 32); }, ALL_SLOTS, keep);
}

// blocks of a persistent kernel: GRID_ROUNDS times what the device holds at once; `guess` when the runtime cannot tell
constexpr int GRID_ROUNDS = 8;
template <typename K> int residentGrid(K kernel, int threads, unsigned dynLds, int cuCount, int guess) {
    int perCu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, kernel, threads, dynLds) != hipSuccess || perCu <= 0) { (void) hipGetLastError(); return guess; }
    return cuCount * perCu * GRID_ROUNDS;
}

}  // namespace

// not part of the public header: used by tests/test_gpu_correct.py through ctypes to run the reference's
// mostLikeliBaseRead known answers (tests/golden/functions/mostlikeli.tsv.gz) through the device call path
extern "C" int cdm_debug_call_bases(cdm_ctx *ctx, const uint32_t *vectors, uint32_t n, uint8_t *out) {
    if (!ctx->haveDamage) { cdm_set_error("cdm_debug_call_bases: no damage model"); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    uint32_t *dv = nullptr; uint8_t *dout = nullptr;
    CDM_HIP(cdmMalloc(&dv, (size_t) n * 48 * 4));
    CDM_HIP(cdmMalloc(&dout, n));
    hipMemcpyAsync(dv, vectors, (size_t) n * 48 * 4, hipMemcpyHostToDevice, ctx->stream);
    hipLaunchKernelGGL(k_debug_call, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, ctx->lutDev, dv, n, dout);
    hipMemcpyAsync(out, dout, n, hipMemcpyDeviceToHost, ctx->stream);
    hipError_t e = hipStreamSynchronize(ctx->stream);
    cdmFree(dv); cdmFree(dout);
    if (e != hipSuccess) { cdm_set_error("debug kernel failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; }
    return CDM_OK;
}

int cdm_correct_impl(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const cdm_ancient_params *par, cdm_seqdb *out) {
    hipStream_t s = ctx->stream;
    const uint32_t n = (uint32_t) db->n;
    DevBuf<uint32_t> active, activeFast, activeSmall; DevBuf<unsigned int> counters; DevBuf<uint8_t> accept;
    if (!active.alloc(n) || !activeFast.alloc(n) || !activeSmall.alloc(n) || !counters.alloc(4) || !accept.alloc(alns->count)) { cdm_set_error("out of device memory in cdm_correct"); return CDM_ERR_HIP; }
    // coverage <= 1 everywhere unless the kernels overwrite: start from a copy of the input bases
    CDM_HIP(hipMemcpyAsync(out->codes, db->codes, db->words * 4, hipMemcpyDeviceToDevice, s));
    CDM_HIP(hipMemcpyAsync(out->nmask, db->nmask, ((db->words * 16 + 31) / 32) * 4, hipMemcpyDeviceToDevice, s));
    CDM_HIP(hipMemsetAsync(counters.p, 0, 16, s));   // [0] queries for the general kernel, [1] error flag, [2] queries for the fast kernel
    // CDM_CORRECT_VARIANT (experiments): "0" = one fast instance for up to 64 records; "s<W>" = small instance (<= 15 records) with W waves per SIMD
    const char *varEnv = cdmGetenv("CDM_CORRECT_VARIANT");
    const int smallW = (varEnv && varEnv[0] == 's') ? atoi(varEnv + 1) : (varEnv && varEnv[0] == '0' ? 0 : 6);
    if (db->raw) {
        CDM_HIP(hipMemcpyAsync(out->raw, db->raw, db->words * 16, hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(k_mark_active_raw, dim3((n + 1023) / 1024), dim3(1024), 0, s, alns->off, alns->rec, db->hasN, n, smallW ? 15u : 0u, active.p, activeFast.p, activeSmall.p, counters.p);
    } else
    hipLaunchKernelGGL(k_mark_active, dim3((n + 1023) / 1024), dim3(1024), 0, s, alns->off, n, smallW ? 15u : 0u, active.p, activeFast.p, activeSmall.p, counters.p);
    DevBuf<SeqMeta> meta;
    MetaUniform uni;
    if (int rc = cdm_build_meta(ctx, db, &meta.p, &uni)) return rc;
    CorrectArgs a;
    cdmSetMeta(a, meta.p, uni); a.ext.m = meta.p; a.ext.plain = uni.words; a.codes = db->codes; a.nmask = db->nmask; a.raw = db->raw; a.outRaw = out->raw;
    a.aoff = alns->off; a.rec = alns->rec; a.ry = (alns->ryMism && alns->rySerial == db->serial) ? alns->ryMism : nullptr; a.active = active.p; a.nActive = counters.p; a.accept = accept.p; a.errFlag = counters.p + 1;
    a.outCodes = out->codes; a.outNmask = out->nmask; a.lut = ctx->lutDev; a.seqIdThr = par->seq_id_thr; a.corrRy = par->corr_reads_ry_seq_id;
    // CDM_CORRECT_STAGE_POOL=<words> (tests): lowers the usable stage pool of the fast kernels, 0 stages nothing
    const char *poolEnv = cdmGetenv("CDM_CORRECT_STAGE_POOL");
    a.stagePool = poolEnv ? (uint32_t) std::max(0, atoi(poolEnv)) : ~0u;
    // CDM_CORRECT_STATS=1: count the accepted records of the fast kernels that were not staged, and why (printed to stderr)
    DevBuf<unsigned long long> stats;
    a.stats = nullptr;
    if (const char *e = cdmGetenv("CDM_CORRECT_STATS"); e && atoi(e)) {
        if (!stats.alloc(4)) { cdm_set_error("out of device memory in cdm_correct"); return CDM_ERR_HIP; }
        CDM_HIP(hipMemsetAsync(stats.p, 0, 32, s));
        a.stats = stats.p;
    }
    const int blocks = ctx->cuCount * 8;
    hipEventRecord(ctx->ev0, s);
    const char *padEnv = cdmGetenv("CDM_LDS_PAD");          // experiments: dynamic LDS that lowers the occupancy
    const unsigned pad = padEnv ? (unsigned) atoi(padEnv) : 0u;
    // Every grid is a whole number of rounds of what the device holds at once, cuCount x resident blocks x GRID_ROUNDS: a grid that is no
    // multiple of the resident blocks ends on a short round (16 blocks per CU at 6 resident is 6 + 6 + 4).  One round alone is the slowest:
    // the loops split their list by gridDim, and the waves of one round do not end together - with several rounds the block dispatcher
    // evens that out (50 M reads, the stage's kernels with the deep launch at 1, 2, 4, 8 and 32 rounds of 5 blocks per CU: 37.1, 35.4, 34.0,
    // 33.2 and 33.0 ms; profiles/r07_correct_grids.txt).  `guess` is the size used when the runtime cannot tell the resident blocks.
    int grids[3] = {0, 0, 0};       // small, deep, general (for the stats line)
    // CDM_CORRECT_GRID=<small>,<deep> (experiments): blocks per CU of the two fast launches, 0 = GRID_ROUNDS rounds of the resident ones
    int gridPerCu[2] = {0, 0};
    if (const char *e = cdmGetenv("CDM_CORRECT_GRID")) sscanf(e, "%d,%d", &gridPerCu[0], &gridPerCu[1]);
    auto launchFast = [&](auto kernel, int guess, const uint32_t *list, const unsigned int *nList, int &grid) {
        const int perCu = gridPerCu[&grid - grids];
        grid = perCu > 0 ? ctx->cuCount * perCu : residentGrid(kernel, 64 * FAST_WAVES, pad, ctx->cuCount, guess);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * FAST_WAVES), pad, s, a, list, nList);
    };
    if (smallW == 8) launchFast(k_correct_fast<15, uint8_t, 8, false>, blocks * 2, activeSmall.p, counters.p + 3, grids[0]);
    else if (smallW == 5) launchFast(k_correct_fast<15, uint8_t, 5, false>, blocks * 2, activeSmall.p, counters.p + 3, grids[0]);
    else if (smallW) launchFast(k_correct_fast<15, uint8_t, 6, false>, blocks * 2, activeSmall.p, counters.p + 3, grids[0]);
    // CDM_CORRECT_BIGW (experiments): blocks per CU of the 16..64-record instance.  5 (the default) with the pool that leaves room for five,
    // 4 with a pool for every record at full length; 6 does not fit the LDS with any pool and selects the default instance.
    const char *bigEnv = cdmGetenv("CDM_CORRECT_BIGW");
    const int bigW = bigEnv ? atoi(bigEnv) : 5;
    // CDM_CORRECT_PILEUP=joint|split (A/B runs and tests): the pile-up loop of that instance, split by damage class (the default) or every
    // column through the LDS counters.  The instance of up to 15 records has 8-bit counters and the joint loop alone.
    const char *pileEnv = cdmGetenv("CDM_CORRECT_PILEUP");
    const bool split = !(pileEnv && std::string(pileEnv) == "joint");
    if (bigW == 4 && split) launchFast(k_correct_fast<64, uint16_t, 4, true>, blocks, activeFast.p, counters.p + 2, grids[1]);
    else if (bigW == 4) launchFast(k_correct_fast<64, uint16_t, 4, false>, blocks, activeFast.p, counters.p + 2, grids[1]);
    else if (split) launchFast(k_correct_fast<64, uint16_t, 5, true>, blocks * 2, activeFast.p, counters.p + 2, grids[1]);
    else launchFast(k_correct_fast<64, uint16_t, 5, false>, blocks * 2, activeFast.p, counters.p + 2, grids[1]);
    grids[2] = residentGrid(k_correct, 64 * WAVES_PER_BLOCK, 0, ctx->cuCount, blocks / 2);
    hipLaunchKernelGGL(k_correct, dim3(grids[2]), dim3(64 * WAVES_PER_BLOCK), 0, s, a);
    hipEventRecord(ctx->ev1, s);
    CDM_LAUNCH_CHECK();
    unsigned int flags[2] = {0, 0};
    CDM_HIP(hipMemcpyAsync(flags, counters.p, 8, hipMemcpyDeviceToHost, s));
    { hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) { cdm_set_error("ancient_correction kernel failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; } }
    hipEventElapsedTime(&ctx->lastMs[0], ctx->ev0, ctx->ev1);
    if (a.stats) {
        unsigned long long st[4] = {0, 0, 0, 0};
        CDM_HIP(hipMemcpy(st, stats.p, 32, hipMemcpyDeviceToHost));
        fprintf(stderr, "cdm_correct stats (fast kernels): accepted records %llu, not staged %llu (target with N %llu, more than %d words %llu, past the pool %llu)\n",
                st[0], st[1] + st[2] + st[3], st[1], STAGE_WORDS, st[2], st[3]);
        fprintf(stderr, "cdm_correct grids: small %d, deep %d, general %d blocks on %d CUs\n", grids[0], grids[1], grids[2], ctx->cuCount);
    }
    return CDM_OK;
}
