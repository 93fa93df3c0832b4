// The gapped step of linclust's `align` on the assembled contigs (host/align.cpp: Matcher::getSWResult's nucleotide branch,
// BandedNucleotideAligner::align over ksw2's banded z-drop extension): what happens between the ungapped seed and the record - the
// reverse extension from the seed's end, the forward extension from the start that one found, the second reverse run where the first
// reached further than the forward one, identities and columns along the edit path - for a batch of independent hits.
//
// One wave per hit, one block per wave.  The recurrence is host/align.cpp's `diagdp` (properties P1-P6 there are the contract) laid over
// the lanes: a row (anti-diagonal) computes at most six blocks of 16 target positions, lane l owns the positions lo16 + l and
// lo16 + 64 + l of the row.  What a position keeps from row to row - its four difference bytes, its last substitution score (P3), its
// score H - lives in a per-wave LDS ring indexed by the position modulo 256, next to the letters of both sequences around the band
// (fetched from the packed DB in runs of 64 as the band moves on; the reverse complement, the doubled query of --wrapped-scoring 1 and the
// reference's off-by-one reversed arrays are index arithmetic).  A row is: read the own and the left neighbour's state as the row before
// left them, barrier, step, write; the row's best cell is one wave maximum over a key that spells P4's order out.
// P6's byte per computed cell goes to HBM (96 bytes a row); the walk back pulls 32 rows at a time through LDS, every lane following the
// same path, and the lanes share the letter comparisons of its diagonal steps.  Hits run in slices whose traces fit a budget.
#include <algorithm>
#include <chrono>
#include <vector>
#include "common.h"
#include "devutil.h"

namespace {
constexpr int ALN_BAND = 64;            // BandedNucleotideAligner.cpp:138-255 calls the extension with this band
constexpr int ALN_RING = 256;           // positions of a ring (a row computes 96 and refreshes 80 positions, 64 more are fetched ahead)
constexpr int ALN_ROW_BYTES = 96;       // trace bytes of a row: six blocks of 16
constexpr int ALN_STAGE_ROWS = 32;      // trace rows in LDS during the walk back
constexpr int ALN_MATCH = 2, ALN_MISMATCH = -3;      // nucleotide.out

struct AlignArgs {
    const uint32_t *woff, *len, *codes, *nmask;
    const cdm_align_hit *hit; cdm_align_result *res;
    const uint64_t *rowOff;             // [hits + 1] trace rows in front of each hit; rowBase: in front of the slice's first hit
    uint64_t rowBase;
    uint8_t *trace;
    uint64_t first, end;                // this launch takes the hits [first, end)
    int open, ext, zdrop;
};
struct Rings {
    uint32_t st[ALN_RING];              // dH | dV << 8 | eT << 16 | eQ << 24 of a target position (P1)
    int32_t H[ALN_RING];
    uint8_t sub[ALN_RING], tLet[ALN_RING], qLet[ALN_RING];
    uint32_t stage[ALN_STAGE_ROWS * ALN_ROW_BYTES / 4];
};
// a hit's two sequences as the module sees them: letters A,C,G,T = 0..3, 4 = the wildcard (the N plane)
struct HitSeqs {
    uint32_t qw, qL0, tw; int qL, tL; bool rc; uint32_t staleQ, staleT;
};
struct ExtIn { int qOff, tOff, qlen, tlen; bool reversed; };
struct ExtOut { int max, max_q, max_t, rows; };

__device__ __forceinline__ uint32_t alnSeqLetter(const AlignArgs &a, uint32_t w, uint32_t p) { return cdm_isN(a.nmask, w, p) ? 4u : cdm_base(a.codes, w, p); }
// letter i of the query as aligned: the (doubled) query or its reverse complement
__device__ __forceinline__ uint32_t alnQuery(const AlignArgs &a, const HitSeqs &s, int i) {
    if (i < 0 || i >= s.qL) return 0u;
    uint32_t p = (uint32_t) (s.rc ? s.qL - 1 - i : i);
    if (p >= s.qL0) p -= s.qL0;
    if (p >= s.qL0) return 0u;
    const uint32_t c = alnSeqLetter(a, s.qw, p);
    return s.rc && c < 4u ? 3u - c : c;
}
__device__ __forceinline__ uint32_t alnTarget(const AlignArgs &a, const HitSeqs &s, int i) {
    if (i < 0 || i >= s.tL) return 0u;
    return alnSeqLetter(a, s.tw, (uint32_t) i);
}
// letter j / p of an extension's query / target; zero behind both (P3).  The reversed arrays hold L + 1 letters, rev[k] = seq[L - k]:
// rev[0] is the byte behind the sequence, which the host's pre-pass hands over
__device__ __forceinline__ uint32_t extQuery(const AlignArgs &a, const HitSeqs &s, const ExtIn &e, int j) {
    if (j < 0 || j >= e.qlen) return 0u;
    if (!e.reversed) return alnQuery(a, s, e.qOff + j);
    const int k = e.qOff + j;
    return k == 0 ? s.staleQ : alnQuery(a, s, s.qL - k);
}
__device__ __forceinline__ uint32_t extTarget(const AlignArgs &a, const HitSeqs &s, const ExtIn &e, int p) {
    if (p < 0 || p >= e.tlen) return 0u;
    if (!e.reversed) return alnTarget(a, s, e.tOff + p);
    const int k = e.tOff + p;
    return k == 0 ? s.staleT : alnTarget(a, s, s.tL - k);
}
__device__ __forceinline__ long long alnWaveMax(long long v) {
    for (int d = 32; d >= 1; d >>= 1) {
        const int lo = __shfl_xor((int) (uint32_t) (unsigned long long) v, d), hi = __shfl_xor((int) (v >> 32), d);
        const long long o = (long long) (((unsigned long long) (uint32_t) hi << 32) | (uint32_t) lo);
        v = o > v ? o : v;
    }
    return v;
}
// the band of row r (P2)
__device__ __forceinline__ void alnBand(int r, int qlen, int tlen, int &lo, int &hi) {
    lo = max(0, r - qlen + 1); hi = min(tlen - 1, r);
    lo = max(lo, (r - ALN_BAND + 1) >> 1); hi = min(hi, (r + ALN_BAND) >> 1);
}

// host/align.cpp extz(): best score and its cell; trace: P6's bytes, row r at trace + 96 r (NULL: not wanted)
__device__ void alnExtend(const AlignArgs &a, const HitSeqs &s, const ExtIn &e, uint8_t *trace, Rings &R, ExtOut &o) {
    o.max = 0; o.max_q = -1; o.max_t = -1; o.rows = 0;
    if (e.qlen <= 0 || e.tlen <= 0) return;
    const int lane = threadIdx.x;
    const int oe = a.open + a.ext;
    const uint32_t open = (uint32_t) a.open & 255u, oe2 = (uint32_t) (2 * oe) & 255u, cap = (uint32_t) (ALN_MATCH + 2 * oe) & 255u;
    __syncthreads();                                    // (the rings may still be read by what ran before)
    for (int i = lane; i < ALN_RING; i += 64) R.qLet[i] = 0;        // query letters in front of the first one
    int tInit = 0, qInit = 0, prevLo16 = -1, prevHi16 = -1;
    const int nrows = e.qlen + e.tlen - 1;
    __syncthreads();
    for (int r = 0; r < nrows; r++) {
        int lo, hi; alnBand(r, e.qlen, e.tlen, lo, hi);
        if (lo > hi) break;
        const int lo16 = lo & ~15, hi16 = hi | 15;
        // positions and letters that enter: fresh state (zero bytes, H unset), letters in runs of 64
        bool entered = false;
        while (tInit <= hi16 + 16) {
            const int p = tInit + lane, slot = p & (ALN_RING - 1);
            R.st[slot] = 0; R.H[slot] = -0x40000000; R.sub[slot] = 0; R.tLet[slot] = (uint8_t) extTarget(a, s, e, p);
            tInit += 64; entered = true;
        }
        while (qInit <= r - lo) {
            const int j = qInit + lane;
            R.qLet[j & (ALN_RING - 1)] = (uint8_t) extQuery(a, s, e, j);
            qInit += 64; entered = true;
        }
        if (entered) __syncthreads();
        const int refreshEnd = lo + ((hi - lo) / 16 + 1) * 16;      // P3: fresh substitution scores for [lo, refreshEnd)
        // read: own state, the left neighbour's as the row before left it
        uint32_t own[2], leftET[2], leftDV[2], sb[2]; int32_t Hown[2], Hleft[2]; bool fresh[2];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int t = lo16 + 64 * k + lane, slot = t & (ALN_RING - 1);
            own[k] = R.st[slot];
            if (t == lo16) {
                leftET[k] = 0; leftDV[k] = 0;
                if (lo16 == 0) leftDV[k] = r ? open : 0u;
                else if (lo16 - 1 >= prevLo16 && lo16 - 1 <= prevHi16) { const uint32_t l = R.st[(t - 1) & (ALN_RING - 1)]; leftET[k] = (l >> 16) & 255u; leftDV[k] = (l >> 8) & 255u; }
            } else { const uint32_t l = R.st[(t - 1) & (ALN_RING - 1)]; leftET[k] = (l >> 16) & 255u; leftDV[k] = (l >> 8) & 255u; }
            fresh[k] = t >= lo && t < refreshEnd;
            if (fresh[k]) {
                const uint32_t x = R.tLet[slot], y = R.qLet[(r - t) & (ALN_RING - 1)];
                sb[k] = (x == 4u || y == 4u) ? 0u : (x == y ? (uint32_t) ALN_MATCH : ((uint32_t) ALN_MISMATCH & 255u));
            } else sb[k] = R.sub[slot];
            Hown[k] = R.H[slot];
            Hleft[k] = (t == hi && hi > 0) ? R.H[(t - 1) & (ALN_RING - 1)] : 0;
        }
        __syncthreads();
        // step (P1), trace byte (P6), scores of the band's cells and the key of P4's order
        long long key = LLONG_MIN;
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int t = lo16 + 64 * k + lane, slot = t & (ALN_RING - 1);
            if (fresh[k]) R.sub[slot] = (uint8_t) sb[k];
            if (t > hi16) continue;
            uint32_t dH = own[k] & 255u, eQ = own[k] >> 24;
            if (t == r) { eQ = 0; dH = r ? open : 0u; }             // the top edge of the matrix enters the computed range
            uint32_t h = (sb[k] + oe2) & 255u;
            const uint32_t viaT = (leftET[k] + leftDV[k]) & 255u, viaQ = (eQ + dH) & 255u;
            uint32_t from = 0;
            if ((int8_t) viaT > (int8_t) h) { from = 1; h = viaT; }
            if ((int8_t) viaQ > (int8_t) h) from = 2;               // (the direction compares signed, the score unsigned)
            if (viaQ > h) h = viaQ;
            if (h > cap) h = cap;
            const uint32_t ndH = (h - leftDV[k]) & 255u, ndV = (h - dH) & 255u;
            const uint32_t opened = (h - open) & 255u, contT = (viaT - opened) & 255u, contQ = (viaQ - opened) & 255u;
            const bool keepT = (int8_t) contT > 0, keepQ = (int8_t) contQ > 0;
            R.st[slot] = ndH | ndV << 8 | (keepT ? contT : 0u) << 16 | (keepQ ? contQ : 0u) << 24;
            if (trace) trace[(size_t) r * ALN_ROW_BYTES + (size_t) (t - lo16)] = (uint8_t) (from | (keepT ? 0x08u : 0u) | (keepQ ? 0x10u : 0u));
            if (t == hi) {
                const int32_t Hn = r == 0 ? (int32_t) ndV - 2 * oe : (hi > 0 ? Hleft[k] + (int32_t) ndH - oe : Hown[k] + (int32_t) ndV - oe);
                R.H[slot] = Hn;
                key = max(key, (long long) Hn * 65536 + 255 * 256 + (t - lo16));
            } else if (r > 0 && t >= lo && t < hi) {
                const int32_t Hn = Hown[k] + (int32_t) ndV - oe;
                R.H[slot] = Hn;
                const int i = t - lo, grouped = (hi - lo) / 4 * 4;
                const int rank = i < grouped ? 1 + (i & 3) * 16 + (i >> 2) : 65 + (i - grouped);     // hi, the four interleaved sweeps, the rest
                key = max(key, (long long) Hn * 65536 + (255 - rank) * 256 + (t - lo16));
            }
        }
        key = alnWaveMax(key);
        const int best = (int) (key >> 16), where = lo16 + (int) (key & 255);
        o.rows = r + 1;
        // P5
        if (best > o.max) { o.max = best; o.max_t = where; o.max_q = r - where; }
        else if (where >= o.max_t && r - where >= o.max_q) {
            const int shift = abs((where - o.max_t) - ((r - where) - o.max_q));
            if (a.zdrop >= 0 && o.max - best > a.zdrop + shift * a.ext) break;
        }
        prevLo16 = lo16; prevHi16 = hi16;
        __syncthreads();
    }
    __syncthreads();
}

// host/align.cpp trace() from cell (t, j), and what the module takes from the edit script: its columns and the identical letters on its
// diagonal steps.  second: the path is the second reverse run's, applied forward from the alignment's start (qBase / tBase: the
// query / target letter of the path's first column)
__device__ void alnWalk(const AlignArgs &a, const HitSeqs &s, const ExtIn &e, const uint8_t *trace, Rings &R, int t, int j, bool second, int qBase, int tBase, int &ids, int &cols) {
    const int lane = threadIdx.x;
    const int t0 = t, j0 = j;
    int stageLo = 1 << 30, inGap = 0, step = 0, myT = -1, myJ = -1, n = 0, same = 0;
    const uint8_t *stage = reinterpret_cast<const uint8_t *>(R.stage);
    auto flush = [&]() {
        if (myT >= 0) {
            const uint32_t x = second ? alnTarget(a, s, tBase + (t0 - myT)) : alnTarget(a, s, tBase + myT);
            const uint32_t y = second ? alnQuery(a, s, qBase + (j0 - myJ)) : alnQuery(a, s, qBase + myJ);
            same += x == y ? 1 : 0;
        }
        myT = -1;
    };
    while (t >= 0 && j >= 0) {
        const int r = t + j;
        if (r < stageLo) {
            __syncthreads();
            stageLo = max(0, r - (ALN_STAGE_ROWS - 1));
            const int words = (r - stageLo + 1) * (ALN_ROW_BYTES / 4);
            const uint32_t *src = reinterpret_cast<const uint32_t *>(trace + (size_t) stageLo * ALN_ROW_BYTES);
            for (int i = lane; i < words; i += 64) R.stage[i] = src[i];
            __syncthreads();
        }
        int lo, hi; alnBand(r, e.qlen, e.tlen, lo, hi);
        const int lo16 = lo & ~15, hi16 = hi | 15;
        uint32_t b = 0; int forced = -1;
        if (t < lo16) forced = 2; else if (t > hi16) forced = 1; else b = stage[(r - stageLo) * ALN_ROW_BYTES + (t - lo16)];
        if (inGap != 0 && !(b & (inGap == 1 ? 0x08u : 0x10u))) inGap = 0;      // the gap ends here
        if (inGap == 0) inGap = (int) (b & 7u);
        if (forced >= 0) inGap = forced;
        if (inGap == 0) { if (lane == (step & 63)) { myT = t; myJ = j; } --t; --j; }
        else if (inGap == 1) --t;
        else --j;
        n++; step++;
        if ((step & 63) == 0) flush();
    }
    flush();
    if (t >= 0) n += t + 1;
    if (j >= 0) n += j + 1;
    ids = cdm_wave_sum(same); cols = n;
}

__global__ __launch_bounds__(64) void k_align(AlignArgs a) {
    __shared__ Rings R;
    const uint64_t h = a.first + blockIdx.x;
    if (h >= a.end) return;
    const cdm_align_hit hit = a.hit[h];
    HitSeqs s;
    s.qw = a.woff[hit.query]; s.qL0 = a.len[hit.query]; s.tw = a.woff[hit.target];
    s.qL = (int) hit.q_len; s.tL = (int) hit.t_len; s.rc = hit.reverse != 0; s.staleQ = hit.stale_q; s.staleT = hit.stale_t;
    const int origLen = hit.wrapped ? s.qL / 2 : s.qL;
    uint8_t *trace = a.trace + (a.rowOff[h] - a.rowBase) * (uint64_t) ALN_ROW_BYTES;
    // BandedNucleotideAligner::align: backwards from the seed's end ...
    const int qStartRev = s.qL - hit.q_end - 1, tStartRev = s.tL - hit.t_end - 1;
    ExtIn rev; rev.reversed = true; rev.qOff = qStartRev; rev.tOff = tStartRev; rev.qlen = s.qL - qStartRev; rev.tlen = s.tL - tStartRev;
    if (hit.wrapped && rev.qlen > origLen) rev.qlen = origLen;
    ExtOut ez, ezAlign;
    alnExtend(a, s, rev, nullptr, R, ez);
    // ... forwards from the start that found ...
    const int qStartPos = s.qL - (qStartRev + ez.max_q) - 1, tStartPos = s.tL - (tStartRev + ez.max_t) - 1;
    ExtIn fwd; fwd.reversed = false; fwd.qOff = qStartPos; fwd.tOff = tStartPos; fwd.qlen = s.qL - qStartPos; fwd.tlen = s.tL - tStartPos;
    if (hit.wrapped && fwd.qlen > origLen) fwd.qlen = origLen;
    alnExtend(a, s, fwd, trace, R, ezAlign);
    int rows = ez.rows + ezAlign.rows, ids = 0, cols = 0;
    // ... and the reverse one again, for its edit script, where it reached further
    if (ez.max_q > ezAlign.max_q && ez.max_t > ezAlign.max_t) {
        alnExtend(a, s, rev, trace, R, ezAlign);
        rows += ezAlign.rows;
        if (ezAlign.max_t >= 0 && ezAlign.max_q >= 0) alnWalk(a, s, rev, trace, R, ezAlign.max_t, ezAlign.max_q, true, qStartPos, tStartPos, ids, cols);
    } else if (ezAlign.max_t >= 0 && ezAlign.max_q >= 0) alnWalk(a, s, fwd, trace, R, ezAlign.max_t, ezAlign.max_q, false, qStartPos, tStartPos, ids, cols);
    if (threadIdx.x == 0) {
        cdm_align_result out;
        out.score = ezAlign.max; out.q_start = qStartPos; out.q_end = qStartPos + ezAlign.max_q; out.t_start = tStartPos; out.t_end = tStartPos + ezAlign.max_t;
        out.identities = ids; out.columns = cols; out.rows = rows;
        a.res[h] = out;
    }
}
}  // namespace

extern "C" int cdm_align_mode(void) {
    const char *e = cdmGetenv("CDM_ALIGN");
    if (!e || !*e) return 0;
    if (std::string(e) == "host") return 1;
    if (std::string(e) == "device") return 2;
    cdm_set_error("CDM_ALIGN=%s: host or device", e);
    return CDM_ERR_INVALID;
}

extern "C" int cdm_align_hits(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_align_params *par, const cdm_align_hit *hits, uint64_t n, cdm_align_result *results, uint64_t *stats) {
    if (!ctx || !db || !par || (n && (!hits || !results))) { cdm_set_error("cdm_align_hits: NULL argument"); return CDM_ERR_INVALID; }
    if (par->band != ALN_BAND) { cdm_set_error("cdm_align_hits: only the band of %d the module uses is implemented (band %d given)", ALN_BAND, par->band); return CDM_ERR_UNSUPPORTED; }
    const int oe = par->gap_open + par->gap_extend;
    if (par->gap_open < 0 || par->gap_extend < 0 || -ALN_MISMATCH > 2 * oe || ALN_MATCH + 2 * oe > 127) {
        cdm_set_error("cdm_align_hits: gap costs %d / %d leave the byte range of the recurrence", par->gap_open, par->gap_extend); return CDM_ERR_UNSUPPORTED;
    }
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n == 0) return CDM_OK;
    // the hits against the DB: every index the kernel forms stays inside its sequences and its trace rows
    std::vector<uint32_t> len((size_t) db->n);
    hipStream_t st = ctx->stream;
    CDM_HIP(hipMemcpyAsync(len.data(), db->len, (size_t) db->n * 4, hipMemcpyDeviceToHost, st));
    CDM_HIP(hipStreamSynchronize(st));
    std::vector<uint64_t> rowOff((size_t) n + 1, 0);       // trace rows in front of each hit: an extension computes fewer than qLen + tLen rows
    for (uint64_t i = 0; i < n; i++) {
        const cdm_align_hit &h = hits[i];
        const bool ok = h.query < db->n && h.target < db->n && h.q_len >= 1 && h.t_len >= 1 && h.q_len <= (uint64_t) len[h.query] * (h.wrapped ? 2u : 1u) && h.t_len <= len[h.target] &&
                        h.q_len < (1u << 30) && h.t_len < (1u << 30) && h.q_end >= -1 && h.q_end < (int64_t) h.q_len && h.t_end >= -1 && h.t_end < (int64_t) h.t_len && h.stale_q <= 4 && h.stale_t <= 4;
        if (!ok) { cdm_set_error("cdm_align_hits: hit %llu is inconsistent with the sequence DB (indices, cut lengths, the seed's ends or the stale letters)", (unsigned long long) i); return CDM_ERR_INVALID; }
        rowOff[i + 1] = rowOff[i] + (uint64_t) (h.wrapped ? h.q_len / 2 : h.q_len) + h.t_len;
    }
    uint64_t budget = 8ull << 30;
    if (const char *e = cdmGetenv("CDM_ALIGN_TRACE_BUDGET")) { const long long v = atoll(e); if (v > 0) budget = (uint64_t) v; }
    // slices: hits while their traces fit the budget (one hit at the least); one trace buffer, sized for the largest, serves them in turn
    std::vector<uint64_t> sliceEnd; uint64_t peak = 0;
    for (uint64_t first = 0; first < n;) {
        uint64_t end = first + 1;
        while (end < n && (rowOff[end + 1] - rowOff[first]) * ALN_ROW_BYTES <= budget) end++;
        peak = std::max(peak, (rowOff[end] - rowOff[first]) * ALN_ROW_BYTES);
        sliceEnd.push_back(end); first = end;
    }
    DevBuf<cdm_align_hit> dHit; DevBuf<cdm_align_result> dRes; DevBuf<uint8_t> trace; DevBuf<uint64_t> dOff;
    if (!dHit.alloc(n) || !dRes.alloc(n) || !dOff.alloc(n + 1) || !trace.alloc(peak + 64)) {
        cdm_set_error("cdm_align_hits: out of device memory (%llu bytes of traces in the largest slice; CDM_ALIGN_TRACE_BUDGET lowers it)", (unsigned long long) peak); return CDM_ERR_HIP;
    }
    CDM_HIP(hipMemcpyAsync(dHit.p, hits, n * sizeof(cdm_align_hit), hipMemcpyHostToDevice, st));
    CDM_HIP(hipMemcpyAsync(dOff.p, rowOff.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    AlignArgs a;
    a.woff = db->woff; a.len = db->len; a.codes = db->codes; a.nmask = db->nmask; a.hit = dHit.p; a.res = dRes.p; a.rowOff = dOff.p; a.trace = trace.p;
    a.open = par->gap_open; a.ext = par->gap_extend; a.zdrop = par->zdrop;
    const uint64_t slices = sliceEnd.size();
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t k = 0, first = 0; k < slices; first = sliceEnd[k++]) {
        const uint64_t end = sliceEnd[k];
        a.rowBase = rowOff[first];
        for (uint64_t f = first, launch = cdmSliceItems(64); f < end; f += launch) {        // (launches of one stream run in order: the next slice waits for this one's traces)
            a.first = f; a.end = std::min(end, f + launch);
            hipLaunchKernelGGL(k_align, CDM_GRID(a.end - a.first, 64), dim3(64), 0, st, a);
            CDM_LAUNCH_CHECK();
        }
    }
    { hipError_t e = hipStreamSynchronize(st); if (e != hipSuccess) { cdm_set_error("cdm_align_hits: kernel failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; } }
    const double kernelS = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    CDM_HIP(hipMemcpyAsync(results, dRes.p, n * sizeof(cdm_align_result), hipMemcpyDeviceToHost, st));
    CDM_HIP(hipStreamSynchronize(st));
    if (stats) {
        uint64_t rows = 0;
        for (uint64_t i = 0; i < n; i++) rows += (uint64_t) results[i].rows;
        stats[0] = slices; stats[1] = rows; stats[2] = peak; stats[3] = (uint64_t) (kernelS * 1e6);
    }
    return CDM_OK;
}
