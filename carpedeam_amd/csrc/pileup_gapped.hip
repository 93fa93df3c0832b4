// The reads across insertions and deletions (cdm_pileup_gapped; not a module of the reference): a banded affine-gap overlap alignment
// with traceback on the seeded pairs rescorediagonal's ungapped test refused - the hits of a listed query that left no counted record
// (include/carpedeam_hip.h; the specification is tests/gapped_model.py).  The steps shared with the other reductions over the pile-up
// are pileup.h's; the work items here run over the HITS' CSR (a chunk of a listed query's hits), for the marking over the records'.
//
//   k_gap_keys     one wave per item of RECORDS: a counted record writes query << 32 | target to keys[record] (the others hold all
//                  ones) and marks counted[target].  The keys are then sorted (radix.h): a set from cdm_rescore keeps its hits' order,
//                  one uploaded through the ABI need not, and a binary search is right for both.
//   per batch (consecutive listed queries whose hit counts sum to at most the bound):
//   k_gap_mark     one wave per item of hits, twice: the candidates per item, then (behind a scan) the candidate list in hit order;
//                  the first pass adds `candidates` and `too_long`
//   k_gap_align    the alignment, G = 16, 32 or 64 lanes a candidate (the power of two >= 2 band + 1), 64 / G candidates a wave, four
//                  waves a block.  A row per read letter j; lane k holds the cell of query letter i = j + Df + k - band:
//                    M  = column(i, j) + H of the lane's own previous row (0 at i = 0 or j = 0: the path starts there)
//                    E  = max(H - open, E - extend) of lane k + 1 of the previous row (one shuffle each)
//                    F  = max over k' < k of H0[k'] - open - extend (k - k' - 1), H0 = max(M, E): one inclusive prefix maximum of
//                         H0[k'] + extend k' over the group (log2 G shuffle steps) read from the left neighbour; exact because
//                         open >= extend - opening from a cell that F itself won never beats extending it
//                    H  = max(M, E, F)
//                  and four trace bits, taken from the finished row (the left neighbour's final H and F): bits 0-1 the state H came
//                  from (M, then D, then I at equal scores), bit 2 E extended, bit 3 F extended (extension before opening).  A lane
//                  packs the bits of eight rows into a word: a group's rows are G / 2 bytes each, in HBM, in a slot of the launch's
//                  trace buffer (the launches take as many candidates as CDM_GAP_TRACE_BUDGET bytes of trace hold).  The end cell is
//                  one 64-bit maximum of score | inverted i | inverted j.  The walk back is one lane's loop of at most L + 2 band + 1
//                  steps over those bits.
//                  Count pass (all candidates, every real diagonal of the hit in rescore's probe order, the greatest score wins): the
//                  walk counts columns, matches, gap letters, operations and words, decides the rescue, adds `rescued` and
//                  `gap_letters`, and offers columns << 40 | inverted hit index to best[target] (64-bit atomicMax) when the target has
//                  no counted record.  The slots of the operations and words come from this count pass plus three exclusive scans.
//                  Emission pass (the rescued only, on the winning diagonal, after the count passes of ALL batches): the same rows
//                  and walk, now writing operations and words from the back of the record's own slots, and the secondary flag.
//   sort, gather   the slots by query << 24 | pos, stable (hit order comes free), then records, operations and words in that order:
//                  pileup_map.hip's shape
// No letter outside [0, n) of the query or [0, L) of the read is loaded; every loop is bounded by L <= 4096 rows, 2 band + 1 lanes or
// the probe count n / 65536 + 2.
#include <list>

#include "pileup.h"
#include "radix.h"

namespace {

constexpr uint32_t GP_MAX_TLEN = 4096;
constexpr int GP_NEG = -(1 << 28);                      // "no path": below every score a path can have, far from overflow
constexpr int GP_NT = 256;                              // threads per block of k_gap_align
constexpr uint64_t GP_BATCH_DEFAULT = 1ull << 26;       // hits per batch
constexpr uint64_t GP_TRACE_DEFAULT = 1ull << 30;       // bytes of trace per launch
constexpr int GP_POS_BITS = 24, GP_INDEX_BITS = 40;
constexpr unsigned long long GP_INDEX_MASK = (1ull << GP_INDEX_BITS) - 1ull;
constexpr uint32_t GP_OP_M = 0, GP_OP_I = 1, GP_OP_D = 2, GP_DELETED = 15;

// CDM_MAP_BATCH=<hits> (tests; cdm_pileup_map's switch): small inputs in several batches.  CDM_GAP_TRACE_BUDGET=<bytes>: several launches.
uint64_t gapBatch() { return envCount("CDM_MAP_BATCH", GP_BATCH_DEFAULT, GP_BATCH_DEFAULT); }
uint64_t gapTraceBudget() { return envCount("CDM_GAP_TRACE_BUDGET", GP_TRACE_DEFAULT, 1ull << 36); }
int gapBitsFor(uint64_t n) { int b = 0; while (b < 64 && (n - 1) >> b) b++; return n > 1 ? b : 0; }

struct GapCand { uint32_t qi, target; uint64_t hit; };         // a candidate: the listed query's index in the batch, the read, the hit

struct GapArgs : ItemArgs {         // (aoff: the records' CSR in k_gap_keys, the hits' in k_gap_mark)
    const uint32_t *codes, *nmask;
    const HitRec *hit;
    uint64_t *keys;                 // [alns->count + 1] sorted query << 32 | target of the counted records, all ones behind them
    uint64_t nKeys;
    uint32_t *counted;              // [n] the target has a counted record on a listed query
    unsigned long long *best;       // [n] columns << 40 | inverted hit index of the target's primary rescued record
    unsigned long long *stats;      // [nq][4]
    uint32_t *itemCand;             // [items + 1] candidates per item, after the scan the item's first
    GapCand *cand;                  // [candidates]; the emission pass: [rescued]
    int32_t *df;                    // the winning diagonal of each
    cdm_gap_rec *res;               // count pass: [candidates]; emission pass: [rescued], the placed records
    uint32_t *okN; uint64_t *opsN, *wordsN;     // [candidates + 1] 1 / operations / words of a rescued candidate, 0 otherwise
    uint32_t *trace; uint64_t traceStride;      // words per group slot
    uint32_t *ops, *words;          // the emission pass's pools
    uint64_t *sortKeys; uint32_t *sortVals;
    cdm_gap_params par;
};

__device__ __forceinline__ unsigned long long gapKey(uint32_t columns, uint64_t h) { return (unsigned long long) columns << GP_INDEX_BITS | (GP_INDEX_MASK - h); }

__global__ __launch_bounds__(64 * PU_WAVES) void k_gap_keys(GapArgs a, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    const ItemRecords it = itemRecords(a, first + local);
    const uint32_t qLen = a.meta[it.q].len;
    for (uint64_t r = it.r0 + lane; r < it.r1; r += 64) {
        const AlnRec rec = a.rec[r];
        Oriented o; uint32_t tLen, tw;
        if (!countedRecord(a.meta, a.n, a.skipExt, a.minSeqId, it.q, qLen, rec, o, tLen, tw)) continue;
        a.keys[r] = (uint64_t) it.q << 32 | rec.target;
        a.counted[rec.target] = 1u;       // (countedRecord: target < n)
    }
}

__device__ __forceinline__ bool gapHasRecord(const GapArgs &a, uint32_t q, uint32_t t) {
    const uint64_t key = (uint64_t) q << 32 | t;
    uint64_t lo = 0, hi = a.nKeys;
    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (a.keys[mid] < key) lo = mid + 1; else hi = mid; }
    return lo < a.nKeys && a.keys[lo] == key;
}

// the candidates among an item's hits: the count, or (EMIT) the list in hit order
template <bool EMIT> __global__ __launch_bounds__(64 * PU_WAVES) void k_gap_mark(GapArgs a, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    const uint64_t item = first + local;
    const ItemRecords it = itemRecords(a, item);
    uint32_t slot0 = EMIT ? a.itemCand[item] : 0u, nLong = 0;
    for (uint64_t hb = it.r0; hb < it.r1; hb += 64) {       // (wave-uniform: the ballot sees all 64 lanes)
        const uint64_t h = hb + lane;
        bool cand = false; uint32_t t = 0;
        if (h < it.r1) {
            t = a.hit[h].target;
            if (t != it.q && t < a.n) {
                const SeqMeta tm = a.meta[t];
                if (!(a.skipExt && (tm.flags & 2u)) && !gapHasRecord(a, it.q, t)) { cand = tm.len <= GP_MAX_TLEN; nLong += !cand; }
            }
        }
        const unsigned long long live = __ballot(cand);
        if (EMIT && cand) { GapCand c; c.qi = it.qi; c.target = t; c.hit = h; a.cand[slot0 + (uint32_t) __popcll(live & ((1ull << lane) - 1ull))] = c; }
        slot0 += (uint32_t) __popcll(live);
    }
    if (!EMIT) {
        const unsigned int tooLong = (unsigned int) cdm_wave_sum((int) nLong);
        if (lane == 0) {
            a.itemCand[item] = slot0;
            unsigned long long *row = a.stats + (uint64_t) it.qi * 4;
            if (slot0) atomicAdd(&row[0], (unsigned long long) slot0);
            if (tooLong) atomicAdd(&row[3], (unsigned long long) tooLong);
        }
    }
}

// a letter of a sequence as the alignment sees it: the code, 4 for an N; reverse: position p of the reverse complement
__device__ __forceinline__ uint32_t gapLetter(const GapArgs &a, uint32_t woff, uint32_t len, bool rev, uint32_t p) {
    const uint32_t at = rev ? len - 1u - p : p;
    if (cdm_isN(a.nmask, woff, at)) return 4u;
    const uint32_t c = cdm_base(a.codes, woff, at);
    return rev ? 3u - c : c;
}

// one pair on one diagonal
struct GapPair { uint32_t qw, tw; int n, L, Df; bool rev; };
// score << 34 | (2^22 - 1 - i) << 12 | (4095 - j): greatest score, then smallest i, then smallest j (sequences hold fewer than 2^22 letters, reads
// here at most 2^12; a path's score lies within +-2^20); 0: no end cell
__device__ __forceinline__ unsigned long long gapEndKey(int score, int i, int j) {
    return (unsigned long long) (score + (1 << 20)) << 34 | (unsigned long long) (0x3FFFFF - i) << 12 | (unsigned long long) (4095 - j);
}
template <int G> __device__ __forceinline__ unsigned long long gapGroupMax(unsigned long long v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        const unsigned long long x = ((unsigned long long) (unsigned int) __shfl_xor((int) (v >> 32), o, G) << 32) | (unsigned int) __shfl_xor((int) (unsigned int) v, o, G);
        v = x > v ? x : v;
    }
    return v;
}

// The rows of a pair: the trace bits into `trace` (the group's slot), -> the end cell's key, equal in all lanes of the group; j0: the
// first row with a cell.  Every lane of the group calls it.
template <int G> __device__ __forceinline__ unsigned long long gapRows(const GapArgs &a, const GapPair &p, uint32_t *__restrict__ trace, int k, int &j0) {
    const int B = (int) a.par.band, W = 2 * B + 1, go = a.par.gap_open, ge = a.par.gap_extend;
    j0 = max(0, -p.Df - B);
    const int j1 = min(p.L - 1, p.n - 1 - p.Df + B);
    if (j1 < j0) return 0ull;
    int Hp = GP_NEG, Ep = GP_NEG;
    uint32_t packed = 0;
    unsigned long long end = 0ull;
    for (int j = j0; j <= j1; j++) {        // (group-uniform bounds: the lanes of a group stay together)
        const int i = j + p.Df + k - B;
        const bool ok = k < W && i >= 0 && i < p.n;
        const uint32_t rc = gapLetter(a, p.tw, (uint32_t) p.L, p.rev, (uint32_t) j);
        const uint32_t qc = ok ? gapLetter(a, p.qw, (uint32_t) p.n, false, (uint32_t) i) : 4u;
        const int Hu = __shfl_down(Hp, 1, G), Eu = __shfl_down(Ep, 1, G);      // (the group's last lane is beyond the band, 2 band + 1 < G, and holds GP_NEG)
        int Mv = ((qc < 4u && qc == rc) ? a.par.match : a.par.mismatch) + ((i > 0 && j > 0) ? Hp : 0);
        int Ev = max(Hu - go, Eu - ge);
        const uint32_t eExt = Eu - ge >= Hu - go ? 4u : 0u;
        int scan = ok ? max(Mv, Ev) + ge * k : GP_NEG;
#pragma unroll
        for (int d = 1; d < G; d <<= 1) { const int o = __shfl_up(scan, d, G); if (k >= d) scan = max(scan, o); }
        const int left = __shfl_up(scan, 1, G);
        int Fv = (ok && k > 0) ? left - go - ge * (k - 1) : GP_NEG;
        int Hv = max(max(Mv, Ev), Fv);
        if (!ok) Mv = Ev = Fv = Hv = GP_NEG;
        const int Hl = __shfl_up(Hv, 1, G), Fl = __shfl_up(Fv, 1, G);
        const uint32_t fExt = (k > 0 && Fl - ge >= Hl - go) ? 8u : 0u;
        const uint32_t src = (Mv >= Ev && Mv >= Fv) ? 0u : Fv >= Ev ? 1u : 2u;
        const int r = j - j0;
        if (ok) packed |= (src | eExt | fExt) << ((r & 7) * 4);
        if ((r & 7) == 7 || j == j1) { trace[(uint64_t) (r >> 3) * G + k] = packed; packed = 0; }
        if (ok && (j == p.L - 1 || i == p.n - 1)) { const unsigned long long key = gapEndKey(Mv, i, j); if (key > end) end = key; }
        Hp = Hv; Ep = Ev;
    }
    return gapGroupMax<G>(end);
}

// what the walk back finds
struct GapWalk { int i0, j0, mCols, matches, inserted, deleted, nOps, nWords; bool ok; };
// One lane walks from the end cell (ie, je) to the start.  EMIT: operations and words are written downwards from opsEnd / wordsEnd,
// never below opsLo / wordsLo; pos: the record's pos (the count pass found it).
template <int G, bool EMIT> __device__ __forceinline__ GapWalk gapWalkBack(const GapArgs &a, const GapPair &p, const uint32_t *__restrict__ trace, int jFirst, int ie, int je,
                                                                        uint32_t *ops, uint64_t opsLo, uint64_t opsEnd, uint32_t *words, uint64_t wordsLo, uint64_t wordsEnd, int pos) {
    const int B = (int) a.par.band;
    GapWalk w = {0, 0, 0, 0, 0, 0, 0, 0, false};
    int i = ie, j = je;
    uint32_t state = GP_OP_M, curOp = GP_OP_M, curLen = 0;
    auto bitsAt = [&](int ci, int cj, uint32_t &bits) {
        const int lane = ci - cj - p.Df + B, r = cj - jFirst;
        if (ci < 0 || ci >= p.n || r < 0 || cj >= p.L || lane < 0 || lane > 2 * B) return false;       // (never, by construction: a path stays on cells of the band)
        bits = (trace[(uint64_t) (r >> 3) * G + lane] >> ((r & 7) * 4)) & 15u;
        return true;
    };
    for (int step = 0, most = p.L + 2 * B + p.L + 2; step < most; step++) {
        uint32_t bits;
        if (!bitsAt(i, j, bits)) return w;
        if (state != curOp) {
            w.nOps++;
            if (EMIT && opsEnd > opsLo) ops[--opsEnd] = curLen << 2 | curOp;
            curOp = state; curLen = 0;
        }
        curLen++;
        bool ext = false;
        if (state == GP_OP_M) {
            const uint32_t qc = gapLetter(a, p.qw, (uint32_t) p.n, false, (uint32_t) i), rc = gapLetter(a, p.tw, (uint32_t) p.L, p.rev, (uint32_t) j);
            w.mCols++;
            if (qc < 4u && qc == rc) w.matches++;
            else { w.nWords++; if (EMIT && wordsEnd > wordsLo) words[--wordsEnd] = (uint32_t) (i - pos) | qc << 24 | rc << 28; }
            if (i == 0 || j == 0) {         // the path starts here
                w.nOps++;
                if (EMIT && opsEnd > opsLo) ops[--opsEnd] = curLen << 2 | curOp;
                w.i0 = i; w.j0 = j; w.ok = true;
                return w;
            }
            i--; j--;
        } else if (state == GP_OP_D) {
            const uint32_t qc = gapLetter(a, p.qw, (uint32_t) p.n, false, (uint32_t) i);
            w.deleted++; w.nWords++;
            if (EMIT && wordsEnd > wordsLo) words[--wordsEnd] = (uint32_t) (i - pos) | qc << 24 | GP_DELETED << 28;
            ext = (bits & 8u) != 0; i--;
        } else {
            w.inserted++;
            ext = (bits & 4u) != 0; j--;
        }
        if (!ext) {
            if (!bitsAt(i, j, bits)) return w;
            state = (bits & 3u) == 0u ? GP_OP_M : (bits & 3u) == 1u ? GP_OP_D : GP_OP_I;
        }
    }
    return w;
}

// the real diagonal of probe `at` of a hit, in rescore's order; false: no overlap
__device__ __forceinline__ bool gapProbe(uint32_t u, int at, int nBelow, int n, int L, bool rev, int &Df) {
    const int D = at < nBelow ? (int) u - 65536 * (at + 1) : (int) u + 65536 * (at - nBelow);
    if (!((D >= 0 && D < n) || (D < 0 && -D < L))) return false;
    Df = rev ? n - L - D : D;
    return true;
}

// G lanes a candidate.  Count pass (EMIT false): candidates [first, first + nThis) of a.cand; emission pass: the rescued.
template <int G, bool EMIT> __global__ __launch_bounds__(GP_NT) void k_gap_align(GapArgs a, uint64_t first, uint64_t nThis) {
    const int k = threadIdx.x & (G - 1);
    const uint64_t local = (uint64_t) blockIdx.x * (GP_NT / G) + threadIdx.x / G;
    if (local >= nThis) return;         // (a whole group leaves)
    const uint64_t c = first + local;
    uint32_t *trace = a.trace + local * a.traceStride;
    const GapCand cd = a.cand[c];
    const HitRec hit = a.hit[cd.hit];
    const SeqMeta qm = a.meta[a.queries[cd.qi]], tm = a.meta[cd.target];
    GapPair p; p.qw = qm.woff; p.tw = tm.woff; p.n = (int) qm.len; p.L = (int) tm.len; p.rev = hit.score < 0; p.Df = 0;
    if (EMIT) {
        p.Df = a.df[c];
        int jFirst;
        const unsigned long long end = gapRows<G>(a, p, trace, k, jFirst);
        waveLdsSync();      // (the walking lane reads what the group's lanes wrote)
        if (k != 0 || end == 0ull) return;
        cdm_gap_rec r = a.res[c];
        const int ie = 0x3FFFFF - (int) ((end >> 12) & 0x3FFFFFull), je = 4095 - (int) (end & 4095ull);
        gapWalkBack<G, true>(a, p, trace, jFirst, ie, je, a.ops, r.ops, r.ops + r.n_ops, a.words, r.words, r.words + r.n_words, (int) r.pos);
        const bool primary = !a.counted[cd.target] && a.best[cd.target] == gapKey(r.columns, cd.hit);
        r.flags = (p.rev ? CDM_MAP_REVERSE : 0u) | (primary ? 0u : CDM_MAP_SECONDARY);
        a.res[c] = r;
        a.sortKeys[c] = (uint64_t) cd.qi << GP_POS_BITS | r.pos; a.sortVals[c] = (uint32_t) c;
        return;
    }
    const uint32_t u = (uint32_t) (unsigned short) (short) hit.diagonal;
    const int nBelow = 1 + p.L / 32768, nProbes = nBelow + p.n / 65536 + 1;
    bool found = false; int bestScore = 0, bestDf = 0; GapWalk bw = {0, 0, 0, 0, 0, 0, 0, 0, false}; int bestIe = 0, bestJe = 0;
    for (int at = 0; at < nProbes; at++) {      // (group-uniform)
        if (!gapProbe(u, at, nBelow, p.n, p.L, p.rev, p.Df)) continue;
        int jFirst;
        const unsigned long long end = gapRows<G>(a, p, trace, k, jFirst);
        waveLdsSync();
        if (end == 0ull) continue;
        const int score = (int) (end >> 34) - (1 << 20);
        if (found && score <= bestScore) continue;
        if (k == 0) {
            bestIe = 0x3FFFFF - (int) ((end >> 12) & 0x3FFFFFull); bestJe = 4095 - (int) (end & 4095ull);
            bw = gapWalkBack<G, false>(a, p, trace, jFirst, bestIe, bestJe, nullptr, 0, 0, nullptr, 0, 0, 0);
        }
        waveLdsSync();      // (the next probe's rows overwrite the slot)
        found = true; bestScore = score; bestDf = p.Df;
    }
    if (k != 0) return;
    const uint32_t columns = (uint32_t) (bw.mCols + bw.inserted);
    const bool rescued = found && bw.ok && bestScore > 0 && columns >= a.par.min_columns &&
                         (uint64_t) bw.matches * 1000ull >= (uint64_t) a.par.min_id_permille * (uint64_t) (bw.mCols + bw.inserted + bw.deleted);
    a.okN[c] = rescued ? 1u : 0u; a.opsN[c] = rescued ? (uint64_t) bw.nOps : 0ull; a.wordsN[c] = rescued ? (uint64_t) bw.nWords : 0ull;
    if (!rescued) return;
    cdm_gap_rec r;
    r.query = cd.qi; r.target = cd.target; r.pos = (uint32_t) bw.i0; r.span = (uint32_t) (bestIe - bw.i0 + 1); r.tstart = (uint32_t) bw.j0; r.tlen = (uint32_t) p.L;
    r.columns = columns; r.nm = (uint32_t) (bw.nWords + bw.inserted); r.flags = 0; r.n_ops = (uint32_t) bw.nOps; r.n_words = (uint32_t) bw.nWords; r.score = bestScore;
    r.ops = 0; r.words = 0;
    a.res[c] = r; a.df[c] = bestDf;
    unsigned long long *row = a.stats + (uint64_t) cd.qi * 4;
    atomicAdd(&row[1], 1ull);
    if (bw.inserted + bw.deleted) atomicAdd(&row[2], (unsigned long long) (bw.inserted + bw.deleted));
    if (!a.counted[cd.target]) atomicMax(&a.best[cd.target], gapKey(columns, cd.hit));
}

// the rescued candidates of a batch behind each other, with their slots in the two pools (the scanned counts)
struct GapPickArgs { const GapCand *cand; const cdm_gap_rec *res; const int32_t *df; const uint32_t *okAt; const uint64_t *opsAt, *wordsAt; GapCand *outCand; cdm_gap_rec *outRec; int32_t *outDf; uint32_t n; };
__global__ __launch_bounds__(DP_NT) void k_gap_pick(GapPickArgs g, uint64_t first) {
    const uint64_t c = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (c >= g.n || g.okAt[c + 1] == g.okAt[c]) return;
    const uint32_t to = g.okAt[c];
    cdm_gap_rec r = g.res[c];
    r.ops = g.opsAt[c]; r.words = g.wordsAt[c];
    g.outRec[to] = r; g.outCand[to] = g.cand[c]; g.outDf[to] = g.df[c];
}

// the sorted order: a tile is DP_NT slots
struct GapGatherArgs {
    const cdm_gap_rec *in; const uint32_t *order, *opsIn, *wordsIn;
    uint64_t *opsPlace, *wordsPlace;        // [n + 1]: n_ops / n_words of the record at every sorted place, after the scans its first word
    cdm_gap_rec *out; uint32_t *opsOut, *wordsOut;
    uint32_t n, firstQuery; uint64_t firstOp, firstWord;        // the batch's first listed query, the words of the batches before it
};
__global__ __launch_bounds__(DP_NT) void k_gap_place(GapGatherArgs g, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i < g.n) { const cdm_gap_rec &r = g.in[g.order[i]]; g.opsPlace[i] = r.n_ops; g.wordsPlace[i] = r.n_words; }
}
__global__ __launch_bounds__(DP_NT) void k_gap_gather(GapGatherArgs g, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i >= g.n) return;
    cdm_gap_rec r = g.in[g.order[i]];
    const uint64_t toOps = g.opsPlace[i], toWords = g.wordsPlace[i];
    for (uint32_t k = 0; k < r.n_ops; k++) g.opsOut[toOps + k] = g.opsIn[r.ops + k];
    for (uint32_t k = 0; k < r.n_words; k++) g.wordsOut[toWords + k] = g.wordsIn[r.words + k];
    r.query += g.firstQuery; r.ops = g.firstOp + toOps; r.words = g.firstWord + toWords;
    g.out[i] = r;
}

// hits per listed query
__global__ void k_gap_hit_counts(const uint64_t *__restrict__ hoff, const uint32_t *__restrict__ queries, uint64_t nq, uint64_t *__restrict__ hits) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq) { const uint32_t q = queries[i]; hits[i] = hoff[q + 1] - hoff[q]; }
}

// the launches of k_gap_align over nItems candidates: as many a launch as the trace buffer holds
template <bool EMIT> void gapLaunchAlign(hipStream_t s, const GapArgs &a, uint64_t nItems, uint64_t perLaunch) {
    const int G = a.par.band <= 7 ? 16 : a.par.band <= 15 ? 32 : 64;
    for (uint64_t first = 0; first < nItems; first += perLaunch) {
        const uint64_t nThis = std::min<uint64_t>(perLaunch, nItems - first);
        const uint64_t perBlock = GP_NT / G;
        const dim3 grid = CDM_GRID((nThis + perBlock - 1) / perBlock, GP_NT);
        if (G == 16) hipLaunchKernelGGL((k_gap_align<16, EMIT>), grid, dim3(GP_NT), 0, s, a, first, nThis);
        else if (G == 32) hipLaunchKernelGGL((k_gap_align<32, EMIT>), grid, dim3(GP_NT), 0, s, a, first, nThis);
        else hipLaunchKernelGGL((k_gap_align<64, EMIT>), grid, dim3(GP_NT), 0, s, a, first, nThis);
    }
}

// what a batch keeps between its count pass and its emission pass
struct GapBatch {
    uint64_t b0 = 0; uint32_t m = 0, nAcc = 0; uint64_t nOps = 0, nWords = 0;
    DevBuf<GapCand> cand; DevBuf<cdm_gap_rec> rec; DevBuf<int32_t> df;
};

}  // namespace

static int cdm_gap_impl(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_hits *hits, const cdm_alns *alns, const uint32_t *queries, uint64_t nq, const cdm_gap_params *par, uint64_t *stats,
                        cdm_gap_rec **recs, uint64_t *nRecsOut, uint32_t **opsOut, uint64_t *nOpsOut, uint32_t **wordsOut, uint64_t *nWordsOut, float *kernelMs) {
    static const char *const WHO = "cdm_pileup_gapped";
    hipStream_t s = ctx->stream;
    const uint32_t chunk = pileupChunk();
    const uint64_t bound = gapBatch();
    QuerySizes qs;
    if (int rc = querySizes(ctx, db, alns, queries, nq, WHO, "record slots", qs)) return rc;
    std::vector<uint64_t> hitN(nq);
    {
        DevBuf<uint64_t> dHitN;
        if (!dHitN.alloc(nq)) { cdm_set_error("%s: out of device memory for %llu queries", WHO, (unsigned long long) nq); return CDM_ERR_HIP; }
        hipLaunchKernelGGL(k_gap_hit_counts, CDM_GRID((nq + 255) / 256, 256), dim3(256), 0, s, (const uint64_t *) hits->off, (const uint32_t *) qs.dq.p, nq, dHitN.p);
        CDM_LAUNCH_CHECK();
        CDM_HIP(hipMemcpyAsync(hitN.data(), dHitN.p, (size_t) nq * 8, hipMemcpyDeviceToHost, s));
        CDM_HIP(hipStreamSynchronize(s));
    }
    for (uint64_t i = 0; i < nq; i++)
        if (hitN[i] >> 32) { cdm_set_error("%s: query %u has %llu hits; the 32-bit candidate slots hold fewer than 2^32", WHO, queries[i], (unsigned long long) hitN[i]); return CDM_ERR_UNSUPPORTED; }
    // the trace slots: rows of the longest read that is examined, G lanes, eight rows a word
    const int G = par->band <= 7 ? 16 : par->band <= 15 ? 32 : 64;
    const uint64_t maxRows = std::min<uint64_t>(std::max<uint32_t>(db->maxLen, 1u), GP_MAX_TLEN), stride = (maxRows + 7) / 8 * (uint64_t) G;
    const uint64_t perLaunch = std::max<uint64_t>(1, std::min<uint64_t>(gapTraceBudget() / (stride * 4), cdmSliceItems((unsigned) G)));
    DevBuf<unsigned long long> best; DevBuf<uint64_t> keys0, keys1; DevBuf<uint32_t> counted, trace;
    const uint64_t nKeys = alns->count;
    if (!best.alloc((size_t) db->n) || !counted.alloc((size_t) db->n) || !keys0.alloc((size_t) nKeys) || !keys1.alloc((size_t) nKeys)) {
        cdm_set_error("%s: out of device memory for the keys of %llu records and %llu sequences", WHO, (unsigned long long) nKeys, (unsigned long long) db->n); return CDM_ERR_HIP;
    }
    CDM_HIP(hipMemsetAsync(best.p, 0, (size_t) db->n * 8, s));
    CDM_HIP(hipMemsetAsync(counted.p, 0, (size_t) db->n * 4, s));
    CDM_HIP(hipMemsetAsync(keys0.p, 0xFF, (size_t) (nKeys + 1) * 8, s));
    float msTotal = 0.f;
    GapArgs a = {};
    a.codes = db->codes; a.nmask = db->nmask; a.hit = hits->rec; a.keys = keys0.p; a.nKeys = nKeys; a.counted = counted.p; a.best = best.p; a.par = *par; a.traceStride = stride;
    // the counted records of ALL listed queries, before any hit is looked at (workItems takes at most 2^30 queries at a time)
    for (uint64_t b0 = 0; b0 < nq;) {
        const uint32_t m = (uint32_t) std::min<uint64_t>(nq - b0, 1ull << 30);
        WorkItems work;
        if (!work.alloc(m)) { cdm_set_error("%s: out of device memory for the work items of %u queries", WHO, m); return CDM_ERR_HIP; }
        if (int rc = workItems(s, alns, qs.dq.p + b0, m, chunk, work)) return rc;
        fillArgs(a, qs.meta.p, db, alns, par->min_seq_id, par->skip_extended_targets, work);
        hipEventRecord(ctx->ev0, s);
        launchWaveItems(s, k_gap_keys, a, work.n);
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        if (int rc = finishTimed(ctx, WHO, "marking", msTotal)) return rc;
        b0 += m;
    }
    {
        bool inFirst = true;
        hipEventRecord(ctx->ev0, s);
        if (int rc = rx::sortKeys<uint64_t>(s, ctx->cuCount, keys0.p, keys1.p, nKeys, 0, 32 + gapBitsFor(db->n), inFirst)) return rc;
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        if (int rc = finishTimed(ctx, WHO, "sort of the record keys", msTotal)) return rc;
        a.keys = inFirst ? keys0.p : keys1.p;
    }
    std::list<GapBatch> kept;
    for (uint64_t b0 = 0; b0 < nq;) {
        // the batch: listed queries while their hits stay within the bound; a single query with more goes alone
        uint32_t m = 0; uint64_t sum = 0;
        for (; b0 + m < nq && m < (1u << 30) && (m == 0 || sum + hitN[b0 + m] <= bound); m++) sum += hitN[b0 + m];
        WorkItems work; cdmscan::ScanTemp stCand, stOk, stOps, stWords;
        DevBuf<unsigned long long> dStats; DevBuf<uint32_t> itemCand;
        if (!work.alloc(m) || !dStats.alloc((size_t) m * 4)) { cdm_set_error("%s: out of device memory for %u queries", WHO, m); return CDM_ERR_HIP; }
        CDM_HIP(hipMemsetAsync(dStats.p, 0, (size_t) m * 32, s));
        if (int rc = workItems(s, (const uint64_t *) hits->off, qs.dq.p + b0, m, chunk, work)) return rc;
        const uint64_t nItems = work.n;
        fillArgs(a, qs.meta.p, db, alns, par->min_seq_id, par->skip_extended_targets, work);
        a.aoff = hits->off;         // (the items are chunks of hits)
        a.stats = dStats.p;
        if (!itemCand.alloc((size_t) nItems + 1)) { cdm_set_error("%s: out of device memory for %llu work items", WHO, (unsigned long long) nItems); return CDM_ERR_HIP; }
        CDM_HIP(hipMemsetAsync(itemCand.p + nItems, 0, 4, s));
        a.itemCand = itemCand.p;
        uint32_t nCand = 0;
        hipEventRecord(ctx->ev0, s);
        launchWaveItems(s, k_gap_mark<false>, a, nItems);
        if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stCand, itemCand.p, itemCand.p, (size_t) nItems + 1)) return rc;        // (in place: scan.h)
        CDM_HIP(hipMemcpyAsync(&nCand, itemCand.p + nItems, 4, hipMemcpyDeviceToHost, s));
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        if (int rc = finishTimed(ctx, WHO, "candidate count", msTotal)) return rc;
        if (sum && nCand > sum) { cdm_set_error("%s: %u candidates of %llu hits", WHO, nCand, (unsigned long long) sum); return CDM_ERR_HIP; }
        if (nCand) {
            DevBuf<GapCand> cand; DevBuf<cdm_gap_rec> res; DevBuf<int32_t> df; DevBuf<uint32_t> okN; DevBuf<uint64_t> opsN, wordsN;
            const uint64_t slots = std::min<uint64_t>(perLaunch, nCand);
            if (!cand.alloc(nCand) || !res.alloc(nCand) || !df.alloc(nCand) || !okN.alloc((size_t) nCand + 1) || !opsN.alloc((size_t) nCand + 1) || !wordsN.alloc((size_t) nCand + 1) ||
                !trace.alloc((size_t) (slots * stride))) {
                cdm_set_error("%s: out of device memory for %u candidates (%llu bytes of trace a launch; CDM_GAP_TRACE_BUDGET lowers it)", WHO, nCand, (unsigned long long) (slots * stride * 4)); return CDM_ERR_HIP;
            }
            CDM_HIP(hipMemsetAsync(okN.p + nCand, 0, 4, s));
            CDM_HIP(hipMemsetAsync(opsN.p + nCand, 0, 8, s));
            CDM_HIP(hipMemsetAsync(wordsN.p + nCand, 0, 8, s));
            a.cand = cand.p; a.res = res.p; a.df = df.p; a.okN = okN.p; a.opsN = opsN.p; a.wordsN = wordsN.p; a.trace = trace.p;
            GapBatch got; got.b0 = b0; got.m = m;
            hipEventRecord(ctx->ev0, s);
            launchWaveItems(s, k_gap_mark<true>, a, nItems);
            gapLaunchAlign<false>(s, a, nCand, perLaunch);
            if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stOk, okN.p, okN.p, (size_t) nCand + 1)) return rc;
            if (int rc = cdmscan::exclusiveScan<uint64_t>(s, stOps, opsN.p, opsN.p, (size_t) nCand + 1)) return rc;
            if (int rc = cdmscan::exclusiveScan<uint64_t>(s, stWords, wordsN.p, wordsN.p, (size_t) nCand + 1)) return rc;
            CDM_HIP(hipMemcpyAsync(&got.nAcc, okN.p + nCand, 4, hipMemcpyDeviceToHost, s));
            CDM_HIP(hipMemcpyAsync(&got.nOps, opsN.p + nCand, 8, hipMemcpyDeviceToHost, s));
            CDM_HIP(hipMemcpyAsync(&got.nWords, wordsN.p + nCand, 8, hipMemcpyDeviceToHost, s));
            hipEventRecord(ctx->ev1, s);
            CDM_LAUNCH_CHECK();
            if (int rc = finishTimed(ctx, WHO, "count pass", msTotal)) return rc;
            if (recs && got.nAcc) {
                kept.emplace_back();
                GapBatch &kb = kept.back();
                kb.b0 = got.b0; kb.m = got.m; kb.nAcc = got.nAcc; kb.nOps = got.nOps; kb.nWords = got.nWords;
                if (!kb.cand.alloc(kb.nAcc) || !kb.rec.alloc(kb.nAcc) || !kb.df.alloc(kb.nAcc)) { cdm_set_error("%s: out of device memory for %u rescued records", WHO, kb.nAcc); return CDM_ERR_HIP; }
                GapPickArgs g;
                g.cand = cand.p; g.res = res.p; g.df = df.p; g.okAt = okN.p; g.opsAt = opsN.p; g.wordsAt = wordsN.p; g.outCand = kb.cand.p; g.outRec = kb.rec.p; g.outDf = kb.df.p; g.n = nCand;
                hipEventRecord(ctx->ev0, s);
                launchTiles(s, k_gap_pick, g, ((uint64_t) nCand + DP_NT - 1) / DP_NT);
                hipEventRecord(ctx->ev1, s);
                CDM_LAUNCH_CHECK();
                if (int rc = finishTimed(ctx, WHO, "selection of the rescued", msTotal)) return rc;
            }
            trace.free();
        }
        CDM_HIP(hipMemcpyAsync(stats + b0 * 4, dStats.p, (size_t) m * 32, hipMemcpyDeviceToHost, s));
        CDM_HIP(hipStreamSynchronize(s));
        b0 += m;
    }
    // the emission: every batch's count pass has run, best[] holds the primary of every read
    for (GapBatch &kb : kept) {
        const uint32_t nRec = kb.nAcc;
        WorkItems work;         // (the kernel's argument block wants the batch's listed queries, nothing else of the items)
        DevBuf<cdm_gap_rec> sorted; DevBuf<uint32_t> ops, words, opsSorted, wordsSorted, v0, v1; DevBuf<uint64_t> k0, k1, opsPlace, wordsPlace; cdmscan::ScanTemp stOps, stWords;
        const uint64_t slots = std::min<uint64_t>(perLaunch, nRec);
        if (!sorted.alloc(nRec) || !ops.alloc((size_t) kb.nOps) || !words.alloc((size_t) kb.nWords) || !opsSorted.alloc((size_t) kb.nOps) || !wordsSorted.alloc((size_t) kb.nWords) || !v0.alloc(nRec) ||
            !v1.alloc(nRec) || !k0.alloc(nRec) || !k1.alloc(nRec) || !opsPlace.alloc((size_t) nRec + 1) || !wordsPlace.alloc((size_t) nRec + 1) || !trace.alloc((size_t) (slots * stride))) {
            cdm_set_error("%s: out of device memory for %u records, %llu operations and %llu words", WHO, nRec, (unsigned long long) kb.nOps, (unsigned long long) kb.nWords); return CDM_ERR_HIP;
        }
        a.queries = qs.dq.p + kb.b0; a.nq = kb.m; a.stats = nullptr;
        a.cand = kb.cand.p; a.res = kb.rec.p; a.df = kb.df.p; a.trace = trace.p; a.ops = ops.p; a.words = words.p; a.sortKeys = k0.p; a.sortVals = v0.p;
        CDM_HIP(hipMemsetAsync(opsPlace.p + nRec, 0, 8, s));
        CDM_HIP(hipMemsetAsync(wordsPlace.p + nRec, 0, 8, s));
        hipEventRecord(ctx->ev0, s);
        gapLaunchAlign<true>(s, a, nRec, perLaunch);
        bool inFirst = true;        // stable on the query and position bits in use; the slots come in hit order
        if (int rc = rx::sortPairs<uint64_t, uint32_t>(s, ctx->cuCount, k0.p, k1.p, v0.p, v1.p, (uint64_t) nRec, 0, GP_POS_BITS + gapBitsFor(kb.m), inFirst)) return rc;
        GapGatherArgs g;
        g.in = kb.rec.p; g.order = inFirst ? v0.p : v1.p; g.opsIn = ops.p; g.wordsIn = words.p; g.opsPlace = opsPlace.p; g.wordsPlace = wordsPlace.p; g.out = sorted.p;
        g.opsOut = opsSorted.p; g.wordsOut = wordsSorted.p; g.n = nRec; g.firstQuery = (uint32_t) kb.b0; g.firstOp = *nOpsOut; g.firstWord = *nWordsOut;
        const uint64_t nTiles = ((uint64_t) nRec + DP_NT - 1) / DP_NT;
        launchTiles(s, k_gap_place, g, nTiles);
        if (int rc = cdmscan::exclusiveScan<uint64_t>(s, stOps, opsPlace.p, opsPlace.p, (size_t) nRec + 1)) return rc;       // (in place)
        if (int rc = cdmscan::exclusiveScan<uint64_t>(s, stWords, wordsPlace.p, wordsPlace.p, (size_t) nRec + 1)) return rc;
        launchTiles(s, k_gap_gather, g, nTiles);
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        if (int rc = appendRecords(s, WHO, "gapped", recs, nRecsOut, (const cdm_gap_rec *) sorted.p, nRec)) return rc;
        for (uint64_t at = 0; at < kb.nOps;) {       // (appendRecords takes fewer than 2^32 at a time)
            const uint32_t nThis = (uint32_t) std::min<uint64_t>(kb.nOps - at, 1ull << 31);
            if (int rc = appendRecords(s, WHO, "operation", opsOut, nOpsOut, (const uint32_t *) opsSorted.p + at, nThis)) return rc;
            at += nThis;
        }
        for (uint64_t at = 0; at < kb.nWords;) {
            const uint32_t nThis = (uint32_t) std::min<uint64_t>(kb.nWords - at, 1ull << 31);
            if (int rc = appendRecords(s, WHO, "mismatch", wordsOut, nWordsOut, (const uint32_t *) wordsSorted.p + at, nThis)) return rc;
            at += nThis;
        }
        if (int rc = finishTimed(ctx, WHO, "emission", msTotal)) return rc;
        trace.free();
    }
    if (kernelMs) *kernelMs = msTotal;
    return CDM_OK;
}

extern "C" int cdm_pileup_gapped(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_hits *hits, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_gap_params *par,
                                 uint64_t *stats, cdm_gap_rec **recs, uint64_t *n_recs, uint32_t **ops, uint64_t *n_ops, uint32_t **words, uint64_t *n_words, float *kernel_ms) {
    static const char *const WHO = "cdm_pileup_gapped";
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, WHO);
    if (!ctx || !db || !hits || !alns || !par || (recs && (!n_recs || !ops || !n_ops || !words || !n_words)) || (!recs && (ops || words)) || (n_queries && (!queries || !stats))) {
        cdm_set_error("%s: NULL argument", WHO); return CDM_ERR_INVALID;
    }
    if (par->band < 1 || par->band > 31) { cdm_set_error("%s: band %u (1 to 31 diagonals on either side)", WHO, par->band); return CDM_ERR_INVALID; }
    if (par->min_id_permille > 1000) { cdm_set_error("%s: min_id_permille %u (0 to 1000)", WHO, par->min_id_permille); return CDM_ERR_INVALID; }
    if (par->match <= 0 || par->mismatch >= 0 || par->match > 64 || par->mismatch < -64) { cdm_set_error("%s: match %d, mismatch %d (0 < match <= 64, -64 <= mismatch < 0)", WHO, par->match, par->mismatch); return CDM_ERR_INVALID; }
    if (par->gap_extend <= 0 || par->gap_open < par->gap_extend || par->gap_open > 64) {
        cdm_set_error("%s: gap_open %d, gap_extend %d (64 >= gap_open >= gap_extend > 0: the row's one pass is exact only then)", WHO, par->gap_open, par->gap_extend); return CDM_ERR_INVALID;
    }
    if (hits->n != db->n) { cdm_set_error("%s: hit CSR has %llu queries, DB has %llu", WHO, (unsigned long long) hits->n, (unsigned long long) db->n); return CDM_ERR_INVALID; }
    if (int rc = pileupCheckArgs(WHO, db, alns, queries, n_queries)) return rc;
    if (hits->count >> GP_INDEX_BITS) {
        cdm_set_error("%s: the set has %llu hits; the primary key holds a hit's index in %d bits", WHO, (unsigned long long) hits->count, GP_INDEX_BITS); return CDM_ERR_UNSUPPORTED;
    }
    if (ops) { *ops = NULL; *n_ops = 0; }
    if (words) { *words = NULL; *n_words = 0; }
    uint32_t *gotOps = NULL, *gotWords = NULL; uint64_t nOps = 0, nWords = 0;
    const int rc = runWithRecords(ctx, n_queries, recs, n_recs, kernel_ms, [&](cdm_gap_rec **got, uint64_t *nGot, float *ms) {
        return cdm_gap_impl(ctx, db, hits, alns, queries, n_queries, par, stats, got, nGot, got ? &gotOps : (uint32_t **) NULL, &nOps, got ? &gotWords : (uint32_t **) NULL, &nWords, ms);
    });
    if (rc == CDM_OK && ops) { *ops = gotOps; *n_ops = nOps; *words = gotWords; *n_words = nWords; } else { free(gotOps); free(gotWords); }
    return rc;
}

extern "C" void cdm_gap_free(cdm_gap_rec *recs, uint32_t *ops, uint32_t *words) { free(recs); free(ops); free(words); }
