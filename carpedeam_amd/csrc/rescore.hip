// rescorediagonal (--rescore-mode 3, query DB == target DB) on the device.
//
// Replaces the loop at lib/mmseqs/src/alignment/rescorediagonal.cpp:145-356:
//   per prefilter hit: query strand (:194-202), canBeCovered (:211-213), ungapped end-to-end score on the voted diagonal
//   incl. the +-65536 probing of the 16-bit diagonal (DistanceCalculator.h:93-113,115-175,204-220; scores +2/-3, any X -3),
//   E-value gate (:251, decided through a host-built "minimum passing raw score per query length" table so that the
//   double-precision ALP arithmetic stays on the host), identity count (:278-282), coverage / seq.id. filters (:304-314),
//   reverse-strand coordinate encoding (:294-297).
// One thread per hit; sequences are compared 16 bases at a time on the 2-bit words (XOR + popcount).  Hits whose two
// sequences contain an N take a per-base path.  The same kernel writes the survivors compacted, in hit order, and the per-query
// offsets (k_rescore below); CDM_RESCORE=twopass keeps the earlier form - candidates, counts, a scan, a scatter - for A/B runs.
#include "scan.h"

#include <cfloat>
#include <climits>
#include <cstring>

#include "common.h"
#include "devutil.h"

namespace {

struct RescoreArgs {
    MetaWoff woff; MetaLen len; MetaHasN hasN; MetaRaw hasRaw;      // per-sequence metadata, one record per sequence
    const uint32_t *codes, *nmask; const uint8_t *raw;
    const HitRec *hit;
    const int32_t *minScore;   // [maxLen+1]
    uint64_t nHits;
    uint32_t n;
    float seqIdThr, covThr;
    int covMode, minAlnLen;
    unsigned int *undef;       // [2] number of identity records written with the coordinates -1 (see rescoreHit); OnePass::err
};

__device__ __forceinline__ bool canBeCovered(float covThr, int covMode, float ql, float tl) {   // M/commons/Util.cpp:533-550
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
__device__ __forceinline__ bool hasCoverage(float covThr, int covMode, float qc, float tc) {   // Util.cpp:552-567
    switch (covMode) { case 0: return qc >= covThr && tc >= covThr; case 2: return qc >= covThr; case 1: return tc >= covThr; default: return true; }
}
__device__ __forceinline__ float computeCov(unsigned s, unsigned e, unsigned len) {           // StripedSmithWaterman.cpp:1055-1057
    return (min(len, max(s, e)) - min(s, e) + 1) / (float) len;
}

// oriented base and N flag (per-base path)
__device__ __forceinline__ void orientedBase(const RescoreArgs &a, uint32_t w0, uint32_t L, bool hasN, bool rc, uint32_t i, uint32_t &code, bool &isN) {
    const uint32_t p = rc ? (L - 1 - i) : i;
    code = cdm_base(a.codes, w0, p);
    isN = hasN && cdm_isN(a.nmask, w0, p);
    if (rc) code = 3u - code;
}

struct Diag { unsigned score; unsigned diagLen; unsigned dist; int diagonal; unsigned ident; unsigned ry; bool any; unsigned first, last; };

// ungappedAlignmentByDiagonal + computeGlobalSubstitutionStartEndDistance for one real diagonal
__device__ __forceinline__ void scoreDiagonal(const RescoreArgs &a, uint32_t qw, uint32_t qLen, bool qN, bool rc, uint32_t tw, uint32_t tLen, bool tN,
                                              int diagonal, Diag &best, bool qRaw = false, bool tRaw = false) {
    const unsigned md = (unsigned) abs(diagonal);
    uint32_t qOff, tOff, m;
    if (diagonal >= 0 && md < qLen) { qOff = md; tOff = 0; m = min(tLen, qLen - md); }
    else if (diagonal < 0 && md < tLen) { qOff = 0; tOff = md; m = min(tLen - md, qLen); }
    else return;   // res.score stays 0: never beats max (strict >)
    unsigned mism = 0, identN = 0, ry = 0xFFFFu;
    uint32_t first = 0, last = m - 1;
    if (qRaw || tRaw) {
        // computeGlobalSubstitutionStartEndDistance (DistanceCalculator.h:204-220) leaves a '*' at either end of the overlap out
        const uint8_t q0 = (qRaw && !rc) ? cdm_raw_at(a.raw, qw, qOff) : 0, t0 = tRaw ? cdm_raw_at(a.raw, tw, tOff) : 0;
        const uint8_t q1 = (qRaw && !rc) ? cdm_raw_at(a.raw, qw, qOff + m - 1) : 0, t1 = tRaw ? cdm_raw_at(a.raw, tw, tOff + m - 1) : 0;
        first = (q0 == '*' || t0 == '*') ? 1u : 0u;
        if (last > 0 && (q1 == '*' || t1 == '*')) last--;
    }
    if (!qN && !tN) {
        ry = 0;
        const uint32_t qLast = (qLen + 15) / 16 - 1, tLast = (tLen + 15) / 16 - 1;
        for (uint32_t k = 0; k < m; k += 16) {
            const uint32_t x = cdm_oriented_window16(a.codes, qw, qLen, qLast, rc, qOff + k) ^ cdm_window16(a.codes, tw, tOff + k, tLast);
            uint32_t mm = (x | (x >> 1)) & 0x55555555u;
            const uint32_t rem = m - k;
            uint32_t rr = x & 0x55555555u;                      // RY class = low bit of the code; complementing both keeps it
            if (rem < 16) { mm &= (1u << (2 * rem)) - 1u; rr &= (1u << (2 * rem)) - 1u; }
            mism += __popc(mm); ry += __popc(rr);
        }
    } else {
        for (uint32_t k = first; k <= last && k < m; k++) {
            uint32_t qc, tc; bool qn, tn;
            orientedBase(a, qw, qLen, qN, rc, qOff + k, qc, qn);
            orientedBase(a, tw, tLen, tN, false, tOff + k, tc, tn);
            const bool match = !qn && !tn && qc == tc;
            mism += !match;
            // identity count compares letters: forward N == N; the reversed query spells N as 'X' (rescorediagonal.cpp:173-179)
            if (!qRaw && !tRaw) identN += (qn && tn && !rc);
            else {
                // letters beyond ACGTN: the score above is on the mapped codes (createAsciiSubMat), the identity count on the
                // case-folded original bytes (:278-282) - of the target always, of the query on the forward strand; the reversed
                // query is spelled in mapped, complemented upper-case letters (:173-179)
                uint8_t ql = qn ? (rc ? 'X' : 'N') : (uint8_t) "ACGT"[qc], tl = tn ? 'N' : (uint8_t) "ACGT"[tc];
                if (qRaw && !rc) ql = cdm_raw_at(a.raw, qw, qOff + k);
                if (tRaw) tl = cdm_raw_at(a.raw, tw, tOff + k);
                identN += ((ql & 0xDFu) == (tl & 0xDFu)) - (int) match;
            }
        }
    }
    const uint32_t cols = last + 1u >= first ? last + 1u - first : 0u;
    const long long sc = 2ll * (cols - mism) - 3ll * mism;
    const unsigned score = sc > 0 ? (unsigned) sc : 0u;
    if (score > best.score) { best.score = score; best.diagLen = m; best.dist = md; best.diagonal = diagonal; best.ident = (cols - mism) + identN; best.ry = ry; best.any = true; best.first = first; best.last = last; }
}

// One prefilter hit through the gates of rescorediagonal.cpp:194-314: true when the hit leaves a record, which is then in r / ry.  The
// scoring arithmetic and the gates exist once; both forms of the stage below call this.
__device__ __forceinline__ bool rescoreHit(const RescoreArgs &a, uint32_t q, const HitRec &hit, AlnRec &r, uint16_t &ry) {
    const uint32_t t = hit.target;
    const uint32_t qLen = a.len[q], tLen = a.len[t], qw = a.woff[q], tw = a.woff[t];
    const bool qN = a.hasN[q] != 0, tN = a.hasN[t] != 0;
    const bool qRaw = qN && a.hasRaw[q] != 0, tRaw = tN && a.hasRaw[t] != 0;
    const bool isReverse = hit.score < 0;
    const bool isIdentity = (q == t);
    if (!canBeCovered(a.covThr, a.covMode, (float) qLen, (float) tLen)) return false;
    // computeUngappedAlignment (DistanceCalculator.h:93-113) on the 16-bit diagonal
    const unsigned short u = (unsigned short) (short) hit.diagonal;
    Diag best; best.score = 0; best.diagLen = 0; best.dist = 0; best.diagonal = 0; best.ident = 0; best.ry = 0xFFFFu; best.any = false; best.first = 0; best.last = 0;
    for (unsigned d = 1; d <= 1 + tLen / 32768; d++) scoreDiagonal(a, qw, qLen, qN, isReverse, tw, tLen, tN, (int) (-(int) d * 65536 + (int) u), best, qRaw, tRaw);
    for (unsigned d = 0; d <= qLen / 65536; d++) scoreDiagonal(a, qw, qLen, qN, isReverse, tw, tLen, tN, (int) (d * 65536 + u), best, qRaw, tRaw);
    if (!best.any) {
        // Score 0 on every probe: E-value(0) never passes, but the identity record is written whatever its score (:304).  The
        // reference's alignment then still holds its constructor's values - start = end = -1, distance 0 (DistanceCalculator.h:50) - so
        // the record carries the coordinates -1, an alignment length of 1 and, the one compared "column" being the byte in FRONT of
        // the sequence in both operands (query and target are the same DB entry), identity 1/1.  rescorediagonal's own DB is that
        // record; what indexes a sequence with it downstream is undefined in the reference, and refused here (cdm_alns::undefinedRecords).
        if (!isIdentity) return false;
        r.target = t; r.rawScore = 0; r.ident = 1; r.qStart = r.qEnd = r.dbStart = r.dbEnd = -1; r.seqId = 1.0f;
        ry = 0xFFFFu;
        atomicAdd(a.undef, 1u);
        return true;
    }
    const int startPos = (int) best.first, endPos = (int) best.last;
    const int alnLen = (endPos - startPos) + 1;
    int qs, qe, ds, de;
    if (best.diagonal >= 0) { qs = startPos + (int) best.dist; qe = endPos + (int) best.dist; ds = startPos; de = endPos; }
    else { qs = startPos; qe = endPos; ds = startPos + (int) best.dist; de = endPos + (int) best.dist; }
    const bool hasEvalue = (int) best.score >= a.minScore[qLen];
    float seqId = 0.f;
    if (hasEvalue || isIdentity) seqId = static_cast<float>(best.ident) / static_cast<float>(alnLen);
    const float queryCov = computeCov(qs, qe, qLen), targetCov = computeCov(ds, de, tLen);
    if (isReverse) { qs = (int) qLen - qs - 1; qe = (int) qLen - qe - 1; }
    const bool hasCov = hasCoverage(a.covThr, a.covMode, queryCov, targetCov);
    const bool hasSeqId = (double) seqId >= (double) (a.seqIdThr - FLT_EPSILON);
    const bool hasAlnLen = alnLen >= a.minAlnLen;
    if (!(isIdentity || (hasAlnLen && hasCov && hasSeqId && hasEvalue))) return false;
    r.target = t; r.rawScore = (int) best.score; r.ident = (int) best.ident; r.qStart = qs; r.qEnd = qe; r.dbStart = ds; r.dbEnd = de;
    // what a reader of the text record gets back: fastSeqIdToBuffer truncates to 3 decimals, "1.00" for 1 (Util.cpp:278-307)
    r.seqId = (seqId == 1.0f) ? 1.0f : (float) ((double) (int) (seqId * 1000) / 1000.0);
    ry = (uint16_t) min(best.ry, 0xFFFFu);
    return true;
}

// ---- the one-pass form: score a tile of hits, write the survivors where they end up, and the per-query offsets with them.
// A tile is RS_TILE consecutive hits, thread t of the block takes hit t of it (coalesced loads of hitQuery and hit).  The grid is as many blocks as are resident; a block takes tiles by ticket (an atomicAdd on a zeroed word, the next tile's
// ticket fetched while this one is scored) until none is left, so a tile only ever waits for tiles whose blocks run.  Per tile: score
// - which needs nothing of the other tiles, and is where the time goes -, a block scan that ranks the survivors in hit order, and the
// tile's count published at once (status word = 2 flag bits + count: the word is the whole message).  The records wait in LDS: the
// block scores its NEXT tile first, and only then does one wave look back over the tiles in front (as radix.h's k_rx_compact does) and
// the survivors go to rec[prefix + rank].  Without that delay every tile waits, holding its registers, for the slowest of the ~2000
// tiles in flight in front of it (measured: 35 ms instead of 14, docs/NOTEBOOK.md).  Every thread knows the number of survivors in
// front of its hit h, valid or not: that is off[q'] of every query q' in (owner[h - 1], owner[h]] ([0, owner[0]] for h = 0), which
// also covers the queries without hits; the last tile writes the total behind the last owner.  (One lane writes a whole run of
// hit-less queries: short in sets from kmermatch, where every sequence is its own hit; DESIGN.md "Round 8" on sparse uploaded sets.)
constexpr int RS_NT = 256, RS_WAVES = RS_NT / 64, RS_TILE = RS_NT;      // a hit per thread (two and four were slower: docs/NOTEBOOK.md)
// the occupancy asked of the compiler, and the grid that goes with it (profiles/rescore_onepass_resources.txt)
constexpr int RS_WAVES_PER_SIMD = 7, RS_BLOCKS_PER_CU = RS_WAVES_PER_SIMD * 4 / RS_WAVES;
constexpr unsigned long long RS_AGG = 1ull << 62, RS_PREFIX = 2ull << 62, RS_MASK = (1ull << 62) - 1ull;
constexpr unsigned int RS_SPINS = 1u << 24;     // a look-back that has polled one word this often gives up (OnePass::err): seconds, where a tile in front takes microseconds
struct OnePass {
    AlnRec *rec; uint16_t *ry;          // [nHits + 1]
    uint64_t *off;                      // [n + 1]
    unsigned long long *status;         // [tiles], zeroed
    unsigned int *ticket;               // zeroed
    unsigned long long *total;          // [1]
    unsigned int *err;                  // zeroed
};
// what a thread keeps of a scored tile until its survivors are written: the tile, its survivors, the rank of the thread's hit among
// them (RS_KEPT set: the hit is one of them)
struct TileState { uint32_t tile, tot, pos; };
constexpr uint32_t RS_KEPT = 1u << 31;

// the tiles in front of `tile` (wave 0 of the block): the look-back of radix.h's k_rx_compact over the status words; publishes the
// tile's own prefix and returns the number of survivors in front of the tile in every lane
__device__ __forceinline__ unsigned long long rsLookBack(const OnePass &o, uint32_t tile, uint32_t tot) {
    const int lane = threadIdx.x & 63;
    unsigned long long excl = 0;
    if (tile == 0) return 0;            // (tile 0 published its count as a prefix at once)
    long long t0 = (long long) tile - 1;
    while (true) {
        const long long t = t0 - lane;
        unsigned long long v = RS_PREFIX;
        if (t >= 0) {
            unsigned int spins = 0;
            do {
                v = __hip_atomic_load(&o.status[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((v >> 62) == 0ull && ++spins == RS_SPINS) { atomicOr(o.err, 1u); v = RS_PREFIX; }
            } while ((v >> 62) == 0ull);
        }
        const unsigned long long pm = __ballot((v >> 62) == 2ull);
        const int first = pm ? __ffsll(pm) - 1 : 63;
        const unsigned long long part = cdm_wave_incl_sum<unsigned long long>(lane <= first ? (v & RS_MASK) : 0ull);
        excl += (unsigned long long) __shfl((long long) part, 63, 64);
        if (pm) break;
        t0 -= 64;
    }
    if (lane == 0) __hip_atomic_store(&o.status[tile], RS_PREFIX | (excl + tot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return excl;
}

__global__ __launch_bounds__(RS_NT, RS_WAVES_PER_SIMD) void k_rescore(RescoreArgs a, OnePass o, const uint32_t *__restrict__ hitQuery, uint32_t tiles) {
    // the records of the tile being scored, and of the one whose write is pending
    static_assert((size_t) 2 * RS_NT * 34 * RS_BLOCKS_PER_CU <= CU_LDS_BYTES - 16 * 1024, "the records of two tiles per block, for every resident block");
    __shared__ unsigned int sTicket[2], sCnt[RS_WAVES];
    __shared__ unsigned long long sPrefix;
    __shared__ uint4 sLo[2][RS_NT], sHi[2][RS_NT];
    __shared__ uint16_t sRy[2][RS_NT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // the survivors of a scored tile to their place, and the offsets of the queries that begin in it
    auto writeOut = [&](const TileState &t, int buf) {
        if (wave == 0) { const unsigned long long excl = rsLookBack(o, t.tile, t.tot); if (lane == 0) sPrefix = excl; }
        __syncthreads();
        const unsigned long long prefix = sPrefix;
        const uint64_t h = (uint64_t) t.tile * RS_TILE + (uint64_t) tid;
        if (h < a.nHits) {
            const unsigned long long g = prefix + (t.pos & ~RS_KEPT);
            if (t.pos & RS_KEPT) {          // (a thread reads back what it wrote itself)
                uint4 *dst = reinterpret_cast<uint4 *>(o.rec + g);
                dst[0] = sLo[buf][tid]; dst[1] = sHi[buf][tid];
                o.ry[g] = sRy[buf][tid];
            }
            const uint32_t q = hitQuery[h];
            for (uint32_t p = h ? hitQuery[h - 1] + 1u : 0u; p <= q; p++) o.off[p] = g;
        }
        if (t.tile + 1u == tiles) {         // the last tile: the total, for the queries behind the last owner too
            const unsigned long long total = prefix + t.tot;
            for (uint64_t p = (uint64_t) hitQuery[a.nHits - 1] + 1u + tid; p <= a.n; p += RS_NT) o.off[p] = total;
            if (tid == 0) *o.total = total;
        }
    };

    if (tid == 0) sTicket[0] = atomicAdd(o.ticket, 1u);
    __syncthreads();
    uint32_t tile = sTicket[0];
    TileState cur, prev;
    bool pending = false;
    int it = 0;
    for (; tile < tiles; it++) {
        const int buf = it & 1;
        if (tid == 0) sTicket[buf ^ 1] = atomicAdd(o.ticket, 1u);       // the next tile's ticket travels while this tile is scored
        // ---- score
        const uint64_t h = (uint64_t) tile * RS_TILE + (uint64_t) tid;
        bool ok = false;
        if (h < a.nHits) {
            AlnRec r; uint16_t ry;
            ok = rescoreHit(a, hitQuery[h], a.hit[h], r, ry);
            if (ok) {
                sLo[buf][tid] = make_uint4(r.target, (uint32_t) r.rawScore, (uint32_t) r.ident, (uint32_t) r.qStart);
                sHi[buf][tid] = make_uint4((uint32_t) r.qEnd, (uint32_t) r.dbStart, (uint32_t) r.dbEnd, __float_as_uint(r.seqId));
                sRy[buf][tid] = ry;
            }
        }
        // ---- rank in the tile, in hit order: the waves in front, then the lanes in front; the tile's count is published at once
        const unsigned long long m = __ballot(ok);
        cur.tile = tile;
        cur.pos = __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0u)) | (ok ? RS_KEPT : 0u);
        if (lane == 0) sCnt[wave] = (uint32_t) __popcll(m);
        __syncthreads();
        uint32_t tot = 0;
#pragma unroll
        for (int w = 0; w < RS_WAVES; w++) { if (w == wave) cur.pos += tot; tot += sCnt[w]; }
        cur.tot = tot;
        if (tid == 0) __hip_atomic_store(&o.status[tile], (tile == 0 ? RS_PREFIX : RS_AGG) | (unsigned long long) tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t next = sTicket[buf ^ 1];
        // ---- write the tile before this one: its tiles in front had the time of this scoring to publish
        if (pending) writeOut(prev, buf ^ 1);
        prev = cur; pending = true;
        __syncthreads();
        tile = next;
    }
    if (pending) writeOut(prev, (it & 1) ^ 1);      // the block's last tile
}

// ---- the two-pass form (CDM_RESCORE=twopass: the A/B, and what tests/test_gpu_rescore_onepass.py compares with): a candidate record
// and a valid byte per hit, then k_count_valid, a scan and the scatter kernels below
struct TwoPass {
    AlnRec *tmp;               // [nHits] candidate records
    uint16_t *tmpRy;           // [nHits] purine/pyrimidine mismatches of the candidate (0xFFFF = not counted)
    uint8_t *valid;            // [nHits]
};
__global__ __launch_bounds__(256) void k_rescore_twopass(RescoreArgs a, TwoPass w, const uint32_t *__restrict__ hitQuery) {
    const uint64_t h = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= a.nHits) return;
    AlnRec r; uint16_t ry;
    const bool ok = rescoreHit(a, hitQuery[h], a.hit[h], r, ry);
    w.valid[h] = ok;
    if (ok) { w.tmp[h] = r; w.tmpRy[h] = ry; }
}

// hit -> owning query (CSR expansion): one thread per query
__global__ void k_expand(const uint64_t *__restrict__ off, uint32_t n, uint32_t *__restrict__ owner) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    for (uint64_t h = off[q]; h < off[q + 1]; h++) owner[h] = q;
}
__global__ void k_count_valid(const uint64_t *__restrict__ off, const uint8_t *__restrict__ valid, uint32_t n, uint64_t *__restrict__ cnt) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    uint64_t c = 0;
    for (uint64_t h = off[q]; h < off[q + 1]; h++) c += valid[h];
    cnt[q] = c;
}
// Valid candidate records move to their query's output slice, keeping their order.  A thread per record (its rank = valid
// records of the same query in front of it, a short look back) keeps loads and stores coalesced; queries with more than
// SCATTER_SMALL records (deep pile-ups) are left to a thread per query so that the look back stays short.
constexpr uint32_t SCATTER_SMALL = 256;
__global__ void k_scatter(const uint64_t *__restrict__ off, const uint32_t *__restrict__ owner, const uint8_t *__restrict__ valid, const AlnRec *__restrict__ tmp,
                          const uint16_t *__restrict__ tmpRy, uint64_t nHits, const uint64_t *__restrict__ outOff, AlnRec *__restrict__ out, uint16_t *__restrict__ outRy) {
    const uint64_t h = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= nHits || !valid[h]) return;
    const uint32_t q = owner[h];
    const uint64_t first = off[q];
    if (off[q + 1] - first > SCATTER_SMALL) return;
    uint64_t o = outOff[q];
    for (uint64_t j = first; j < h; j++) o += valid[j];
    out[o] = tmp[h]; outRy[o] = tmpRy[h];
}
__global__ void k_scatter_big(const uint64_t *__restrict__ off, const uint8_t *__restrict__ valid, const AlnRec *__restrict__ tmp, const uint16_t *__restrict__ tmpRy, uint32_t n,
                              const uint64_t *__restrict__ outOff, AlnRec *__restrict__ out, uint16_t *__restrict__ outRy) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n || off[q + 1] - off[q] <= SCATTER_SMALL) return;
    uint64_t o = outOff[q];
    for (uint64_t h = off[q]; h < off[q + 1]; h++) if (valid[h]) { out[o] = tmp[h]; outRy[o] = tmpRy[h]; o++; }
}
__global__ void k_len_hist(const uint32_t *__restrict__ len, uint32_t n, uint32_t *__restrict__ present) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) present[len[i]] = 1;
}

// CDM_RESCORE=twopass: the two-pass form (A/B runs and tests); the default is the one-pass kernel
bool rescoreTwoPass() { const char *e = cdmGetenv("CDM_RESCORE"); return e && !strcmp(e, "twopass"); }

// the two-pass form behind k_expand: candidates, counts, scan, a synchronisation for the total, the scatter into arrays of that size
int rescoreCompactTwoPass(cdm_ctx *ctx, const cdm_hits *hits, RescoreArgs &a, const uint32_t *owner, cdm_alns *res) {
    hipStream_t s = ctx->stream;
    const uint32_t n = a.n; const uint64_t nHits = a.nHits;
    DevBuf<AlnRec> tmp; DevBuf<uint16_t> tmpRy; DevBuf<uint8_t> valid; DevBuf<uint64_t> cnt;
    if (!tmp.alloc(nHits) || !tmpRy.alloc(nHits) || !valid.alloc(nHits) || !cnt.alloc((size_t) n + 1)) { cdm_set_error("cdm_rescore: out of device memory"); return CDM_ERR_HIP; }
    TwoPass w; w.tmp = tmp.p; w.tmpRy = tmpRy.p; w.valid = valid.p;
    hipEventRecord(ctx->ev0, s);
    if (nHits) hipLaunchKernelGGL(k_rescore_twopass, CDM_GRID((nHits + 255) / 256, 256), dim3(256), 0, s, a, w, owner);
    hipEventRecord(ctx->ev1, s);
    hipLaunchKernelGGL(k_count_valid, dim3((n + 255) / 256), dim3(256), 0, s, hits->off, valid.p, n, cnt.p);
    CDM_LAUNCH_CHECK();
    cdmscan::ScanTemp scanTmp;
    CDM_HIP(hipMemsetAsync(cnt.p + n, 0, 8, s));
    if (int rc = cdmscan::exclusiveScan<uint64_t>(s, scanTmp, cnt.p, res->off, (size_t) n + 1)) return rc;
    uint64_t total = 0; unsigned int nUndef = 0;
    CDM_HIP(hipMemcpyAsync(&total, res->off + n, 8, hipMemcpyDeviceToHost, s));
    CDM_HIP(hipMemcpyAsync(&nUndef, a.undef, 4, hipMemcpyDeviceToHost, s));
    { hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) { cdm_set_error("cdm_rescore: kernel failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; } }
    res->count = total; res->undefinedRecords = nUndef;
    if (cdmMalloc(&res->rec, (total + 1) * sizeof(AlnRec)) != hipSuccess || cdmMalloc(&res->ryMism, (total + 1) * sizeof(uint16_t)) != hipSuccess) { cdm_set_error("cdm_rescore: out of device memory"); return CDM_ERR_HIP; }
    if (nHits) hipLaunchKernelGGL(k_scatter, CDM_GRID((nHits + 255) / 256, 256), dim3(256), 0, s, hits->off, owner, valid.p, tmp.p, tmpRy.p, (uint64_t) nHits, res->off, res->rec, res->ryMism);
    hipLaunchKernelGGL(k_scatter_big, dim3((n + 255) / 256), dim3(256), 0, s, hits->off, valid.p, tmp.p, tmpRy.p, n, res->off, res->rec, res->ryMism);
    { hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) { cdm_set_error("cdm_rescore: compaction failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; } }
    return CDM_OK;
}

// the one-pass form behind k_expand.  rec and ryMism are allocated for every hit (the upper bound) before the launch, so the total is
// read in the one synchronisation that ends the call; a result that leaves more than an eighth of that room unused is copied into
// arrays of its own size (strict thresholds; the read iterations keep 96 % of their hits).
int rescoreCompactOnePass(cdm_ctx *ctx, RescoreArgs &a, const uint32_t *owner, cdm_alns *res) {
    hipStream_t s = ctx->stream;
    const uint32_t n = a.n; const uint64_t nHits = a.nHits;
    if (cdmMalloc(&res->rec, (nHits + 1) * sizeof(AlnRec)) != hipSuccess || cdmMalloc(&res->ryMism, (nHits + 1) * sizeof(uint16_t)) != hipSuccess) { cdm_set_error("cdm_rescore: out of device memory"); return CDM_ERR_HIP; }
    unsigned long long total = 0; unsigned int tail[2] = {0, 0};     // tail: a.undef[0] = identity records with the coordinates -1, a.undef[1] = OnePass::err
    if (nHits == 0) {
        hipEventRecord(ctx->ev0, s); hipEventRecord(ctx->ev1, s);
        CDM_HIP(hipMemsetAsync(res->off, 0, ((size_t) n + 1) * 8, s));
        CDM_HIP(hipStreamSynchronize(s));
    }
    else {
        const uint64_t tiles = (nHits + RS_TILE - 1) / RS_TILE;
        DevBuf<unsigned long long> status;      // [tiles] status words, then the ticket and the total
        if (!status.alloc(tiles + 2)) { cdm_set_error("cdm_rescore: out of device memory"); return CDM_ERR_HIP; }
        CDM_HIP(hipMemsetAsync(status.p, 0, (tiles + 2) * 8, s));
        OnePass o; o.rec = res->rec; o.ry = res->ryMism; o.off = res->off; o.status = status.p;
        o.ticket = reinterpret_cast<unsigned int *>(status.p + tiles); o.total = status.p + tiles + 1; o.err = a.undef + 1;
        hipEventRecord(ctx->ev0, s);
        uint64_t grid = std::min<uint64_t>(tiles, (uint64_t) ctx->cuCount * RS_BLOCKS_PER_CU);
        if (const char *e = cdmGetenv("CDM_RESCORE_BLOCKS")) { const long long v = atoll(e); if (v > 0) grid = std::min<uint64_t>(grid, (uint64_t) v); }       // tests: a few blocks, so that small inputs loop
        hipLaunchKernelGGL(k_rescore, CDM_GRID(grid, RS_NT), dim3(RS_NT), 0, s, a, o, owner, (uint32_t) tiles);
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        CDM_HIP(hipMemcpyAsync(&total, o.total, 8, hipMemcpyDeviceToHost, s));
        CDM_HIP(hipMemcpyAsync(tail, a.undef, 8, hipMemcpyDeviceToHost, s));
        { hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) { cdm_set_error("cdm_rescore: kernel failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; } }
        if (tail[1]) { cdm_set_error("cdm_rescore: a tile's look-back gave up waiting for the tile in front of it"); return CDM_ERR_HIP; }
    }
    res->count = total; res->undefinedRecords = tail[0];
    if (nHits - total > nHits / 8) {
        AlnRec *rec = nullptr; uint16_t *ry = nullptr;
        if (cdmMalloc(&rec, (total + 1) * sizeof(AlnRec)) != hipSuccess || cdmMalloc(&ry, (total + 1) * sizeof(uint16_t)) != hipSuccess) { if (rec) cdmFree(rec); cdm_set_error("cdm_rescore: out of device memory"); return CDM_ERR_HIP; }
        hipError_t e = total ? hipMemcpyAsync(rec, res->rec, total * sizeof(AlnRec), hipMemcpyDeviceToDevice, s) : hipSuccess;
        if (e == hipSuccess && total) e = hipMemcpyAsync(ry, res->ryMism, total * sizeof(uint16_t), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { cdmFree(rec); cdmFree(ry); cdm_set_error("cdm_rescore: copying the records failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; }
        cdmFree(res->rec); cdmFree(res->ryMism);
        res->rec = rec; res->ryMism = ry;
    }
    return CDM_OK;
}

}  // namespace

int cdm_rescore_impl(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_hits *hits, const cdm_rescore_params *par, cdm_alns **out) {
    hipStream_t s = ctx->stream;
    const uint32_t n = (uint32_t) db->n;
    const uint64_t nHits = hits->count;
    if (db->maxLen >= (1u << 30)) { cdm_set_error("cdm_rescore: sequence too long"); return CDM_ERR_UNSUPPORTED; }
    if (nHits >= 0xFFFFFF00ull) { cdm_set_error("cdm_rescore: %llu prefilter hits (a call takes fewer than 2^32)", (unsigned long long) nHits); return CDM_ERR_UNSUPPORTED; }
    DevBuf<unsigned int> undef;
    if (!undef.alloc(2)) { cdm_set_error("cdm_rescore: out of device memory"); return CDM_ERR_HIP; }
    CDM_HIP(hipMemsetAsync(undef.p, 0, 8, s));
    DevBuf<uint32_t> dPresent, owner; DevBuf<int32_t> dMin;
    if (!dPresent.alloc(db->maxLen + 1) || !dMin.alloc(db->maxLen + 1) || !owner.alloc(nHits)) { cdm_set_error("cdm_rescore: out of device memory"); return CDM_ERR_HIP; }
    // E-value gate table for the lengths that occur (host ALP arithmetic, host/evalue.cpp)
    std::vector<uint32_t> present(db->maxLen + 1);
    CDM_HIP(hipMemsetAsync(dPresent.p, 0, (size_t) (db->maxLen + 1) * 4, s));
    hipLaunchKernelGGL(k_len_hist, dim3((n + 255) / 256), dim3(256), 0, s, db->len, n, dPresent.p);
    CDM_HIP(hipMemcpyAsync(present.data(), dPresent.p, (size_t) (db->maxLen + 1) * 4, hipMemcpyDeviceToHost, s));
    CDM_HIP(hipStreamSynchronize(s));
    std::vector<int32_t> minScore(db->maxLen + 1, INT_MAX);
    for (uint32_t L = 1; L <= db->maxLen; L++) {
        if (!present[L]) continue;
        // A score of 0 that passes -e: the reference then writes the alignment's constructor values (coordinates -1) for a hit that is no
        // identity hit, after counting the byte in front of both sequences - undefined there, refused here.
        if (cdm_evalue_host(0, L, db->residues) <= par->eval_thr) {
            cdm_set_error("cdm_rescore: -e %g lets a score of 0 pass for sequences of %u letters (E-value %g): the records of such hits are undefined in the reference",
                          par->eval_thr, L, cdm_evalue_host(0, L, db->residues));
            return CDM_ERR_UNSUPPORTED;
        }
        int lo = 0, hi = 2 * (int) L;   // E-value decreases with the score (tests/test_gpu_rescore.py checks it for the lengths used)
        if (!(cdm_evalue_host(hi, L, db->residues) <= par->eval_thr)) continue;
        while (lo < hi) { int mid = (lo + hi) / 2; if (cdm_evalue_host(mid, L, db->residues) <= par->eval_thr) hi = mid; else lo = mid + 1; }
        minScore[L] = lo;
    }
    CDM_HIP(hipMemcpyAsync(dMin.p, minScore.data(), (size_t) (db->maxLen + 1) * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_expand, dim3((n + 255) / 256), dim3(256), 0, s, hits->off, n, owner.p);
    DevBuf<SeqMeta> meta;
    MetaUniform uni;
    if (int rc = cdm_build_meta(ctx, db, &meta.p, &uni)) return rc;
    RescoreArgs a;
    cdmSetMeta(a, meta.p, uni); a.codes = db->codes; a.nmask = db->nmask; a.raw = db->raw; a.hit = hits->rec;
    a.minScore = dMin.p; a.nHits = nHits; a.n = n; a.seqIdThr = par->seq_id_thr; a.covThr = par->cov_thr; a.covMode = par->cov_mode;
    a.minAlnLen = par->min_aln_len; a.undef = undef.p;
    cdm_alns *res = new cdm_alns(); res->n = n;
    struct Guard { cdm_alns *&r; bool armed = true; ~Guard() { if (armed && r) { cdm_alns_free(r); r = nullptr; } } } guard{res};
    if (cdmMalloc(&res->off, ((size_t) n + 1) * 8) != hipSuccess) { cdm_set_error("cdm_rescore: out of device memory"); return CDM_ERR_HIP; }
    res->rySerial = db->serial;
    if (int rc = rescoreTwoPass() ? rescoreCompactTwoPass(ctx, hits, a, owner.p, res) : rescoreCompactOnePass(ctx, a, owner.p, res)) return rc;
    hipEventElapsedTime(&ctx->lastMs[1], ctx->ev0, ctx->ev1);
    guard.armed = false;
    *out = res;
    return CDM_OK;
}

uint32_t cdm_rescore_tile_impl() { return (uint32_t) RS_TILE; }
