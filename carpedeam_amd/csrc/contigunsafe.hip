// ancient_contig_merge --unsafe 1 on the device: the column counts against the majority-vote consensus of a query's extending
// candidates (host/contigmerge.cpp unsafeConsensus / unsafeColumns; nuclassembleUtil.cpp:535-702 and 705-790, 1047-1181).
//
// In that mode only five counts of a record change - nnTot, nnId, nnRy, nCT, nGA of ContigStat - and only for the records that pass
// the first gate and start at an end of the query ("column records"): the safe mode counts them against the query itself
// (contig.hip k_contig_stats), the unsafe mode against a consensus of 3 qLen letters - the query in the middle third, elsewhere the
// majority letter of the candidates that cover the position ('N' below --min-cov-safe and on ties).  This pass overwrites those five
// counts in the call's own statistics; the gate and the queue (contigqueue.hip) then run as in safe mode.
//
// The consensus is never written out.  A work item is a TILE of CU_TILE consecutive consensus positions of one query, over the hull
// of the query's column windows only (the rest of the 3 qLen letters is read by nobody); tiles are spread over the queries by a scan,
// so one long contig does not stall a block.  A block per tile:
//   1. the query's records go through LDS a block's worth at a time; those that contribute to the consensus and cover the tile stay
//      for the batch, and every thread counts the letters at its positions over them - a pile-up of any depth takes several batches;
//   2. each thread derives the consensus letters of its positions (in registers, then LDS);
//   3. the column records that overlap the tile go through LDS the same way, and every thread compares its positions' consensus
//      letters with the record's; the five counts are wave ballots, summed per record in LDS and added to the record with one
//      global atomic per count and tile.
// The letters read are the candidates' once per tile that covers them, as k_contig_stats reads them once per record.
//
// What the device does not restate hands the query back to the host code (contig.hip): a query, column record or contributor with
// letters beyond ACGTN (the raw plane; nucleotideMap and getNuclRevFragment read those bytes as the strings hold them).  A contributor
// that would start before the consensus (the reference indexes its coverage vector with a negative number) makes the call fail as
// the host code does.
#include <algorithm>
#include <chrono>
#include <cstring>

#include "common.h"
#include "devutil.h"
#include "scan.h"
#include "contigqueue.h"

namespace {
constexpr uint32_t CU_NONE = 0xFFFFFFFFu;
constexpr int CU_THREADS = 256;
constexpr int CU_PER_THREAD = 4;
constexpr uint32_t CU_TILE = CU_THREADS * CU_PER_THREAD;           // consensus positions per block
enum : uint32_t { CU_REV = 1u, CU_HASN = 2u, CU_COLUMN = 4u };

// a record as this pass reads it: the target's letters, where it lands in the consensus as a contributor (start) and as a column
// record (c0), both CU_NONE when it does not
struct CuRec { uint32_t woff, len, start, c0, flags; };

struct CuArgs {
    const SeqMeta *meta; const uint32_t *codes, *nmask;
    const uint64_t *aoff; const AlnRec *rec; const uint32_t *owner; uint64_t nRec; uint32_t n;
    float mergeThr, ryThr; uint32_t minCov;
    CuRec *cu;
    uint32_t *lo, *hi;          // [n] the hull of the query's column windows
    uint8_t *handBack;          // [n]
    uint64_t *tiles, *tOff;     // [n + 1]
    uint32_t *tileQ;            // [tiles] the query of every tile
    int *acc;                   // [nRec * 5] nnTot, nnId, nnRy, nCT, nGA
    unsigned int *counters;     // 0 contributor before the consensus, 1 queries handed back, 2 column records, 3 queries with tiles
};

// The letters of a record's target at a thread's CU_PER_THREAD consecutive consensus positions p0 .. p0 + 3, the target placed at
// consensus position `at` in its own orientation (isRev): one 16-letter window from oriented letter max(p0 - at, 0) on.  -> whether
// any of them lies on the target; code[k] (0..3; an N as 0, which nucleotideMap reads as A) and the bit mask of the positions that
// lie on the target (on) and of those that hold an N (isN)
__device__ __forceinline__ bool lettersAt(const CuArgs &a, const CuRec &c, uint32_t at, uint32_t p0, uint32_t code[CU_PER_THREAD], uint32_t &on, uint32_t &isN) {
    const long long k0 = (long long) p0 - at;
    if (k0 + CU_PER_THREAD <= 0 || k0 >= (long long) c.len) return false;
    const bool rev = (c.flags & CU_REV) != 0;
    const uint32_t kk = k0 < 0 ? 0u : (uint32_t) k0;
    const uint32_t win = cdm_oriented_window16(a.codes, c.woff, c.len, (c.len + 15) / 16 - 1, rev, kk);
    on = 0; isN = 0;
#pragma unroll
    for (int k = 0; k < CU_PER_THREAD; k++) {
        const long long kp = k0 + k;
        code[k] = 0;
        if (kp < 0 || kp >= (long long) c.len) continue;
        on |= 1u << k;
        code[k] = (win >> (2 * (uint32_t) (kp - kk))) & 3u;
        if ((c.flags & CU_HASN) && cdm_isN(a.nmask, c.woff, rev ? c.len - 1u - (uint32_t) kp : (uint32_t) kp)) { isN |= 1u << k; code[k] = 0; }
    }
    return true;
}

// ------------------------------------------------------------------------------------------------ a thread per record
// -> whether record r is a column record
__device__ __forceinline__ bool recordOf(const CuArgs &a, const ContigStat *__restrict__ st, uint64_t r) {
    const AlnRec rec = a.rec[r]; const ContigStat s = st[r];
    const uint32_t q = a.owner[r];
    const SeqMeta qm = a.meta[q], tm = a.meta[rec.target];
    const unsigned qLen = qm.len, dbLen = s.dbLen;
    const uint64_t L3 = 3ull * qLen;
    const unsigned alnLength = (unsigned) max(abs(rec.qEnd - rec.qStart), abs(rec.dbEnd - rec.dbStart)) + 1u;
    CuRec o; o.woff = tm.woff; o.len = tm.len; o.start = CU_NONE; o.c0 = CU_NONE;
    o.flags = (s.rev ? CU_REV : 0u) | ((tm.flags & 1u) ? CU_HASN : 0u);
    const float seqId = static_cast<float>(s.idCnt) / alnLength, rySeqId = static_cast<float>(s.idRy) / alnLength;
    if (seqId >= a.mergeThr && rySeqId >= a.ryThr && qm.key != s.dbKey) {                 // :314-321
        const bool right = (unsigned) s.ds == 0 && (unsigned) s.qe == (qLen - 1);          // the positions' tests (:181-190, :339-340)
        const bool left = (unsigned) s.qs == 0 && (unsigned) s.de == (dbLen - 1);
        const bool rightStart = s.ds == 0 && (s.de != static_cast<int>(dbLen) - 1), leftStart = s.qs == 0 && (s.qe != static_cast<int>(qLen) - 1);
        const unsigned offset = dbLen - alnLength;
        // a contributor to the consensus (unsafeConsensus): its letters from `start` on
        if ((rightStart || leftStart) && (right || left)) {
            const long long start = right ? (long long) qLen + s.qs : (long long) qLen - (long long) offset;
            if (start < 0) atomicExch(&a.counters[0], 1u);
            else if ((uint64_t) start < L3) o.start = (uint32_t) start;
        }
        // a column record (unsafeColumns): the target against the consensus from c0 on, up to the consensus' end.  (An offset beyond
        // qLen is the undefined case the gate reports.)
        if ((left || right) && !(offset > qLen)) {
            o.flags |= CU_COLUMN;
            const long long c0 = left ? (long long) (qLen - offset) : (long long) L3 - ((long long) dbLen + (long long) (qLen - offset));
            if (c0 >= 0 && (uint64_t) c0 < L3 && dbLen > 0) {
                o.c0 = (uint32_t) c0;
                atomicMin(&a.lo[q], (uint32_t) c0);
                atomicMax(&a.hi[q], (uint32_t) min((uint64_t) c0 + dbLen, L3));
            }
            if ((qm.flags & 4u) || (tm.flags & 4u)) a.handBack[q] = 1;     // letters beyond ACGTN: the host's strings
        }
    }
    a.cu[r] = o;
    return (o.flags & CU_COLUMN) != 0;
}
__global__ __launch_bounds__(256) void k_cu_rec(CuArgs a, const ContigStat *__restrict__ st) {
    const uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    bool column = false;
    if (r < a.nRec) column = recordOf(a, st, r);
    (void) cdm_wave_append(&a.counters[2], column);     // (the count: one atomic per wave)
}

// a thread per query (and one past the end): the tiles of its hull
__global__ __launch_bounds__(256) void k_cu_tiles(CuArgs a) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t t = 0;
    bool back = false;
    if (q < a.n) {
        back = a.handBack[q] != 0;
        if (!back && a.hi[q] > a.lo[q]) t = (a.hi[q] - a.lo[q] + CU_TILE - 1) / CU_TILE;
    }
    (void) cdm_wave_append(&a.counters[1], back);
    (void) cdm_wave_append(&a.counters[3], t > 0);
    if (q <= a.n) a.tiles[q] = t;
}
// a thread per query: its tiles' entries of the tile -> query map
__global__ __launch_bounds__(256) void k_cu_map(CuArgs a) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.n) return;
    for (uint64_t t = a.tOff[q]; t < a.tOff[q + 1]; t++) a.tileQ[t] = q;
}

// ------------------------------------------------------------------------------------------------ a block per tile
__global__ __launch_bounds__(CU_THREADS) void k_cu_tile(CuArgs a, uint64_t first, uint64_t nTiles) {
    __shared__ CuRec sRec[CU_THREADS];
    __shared__ uint32_t sIdx[CU_THREADS];
    __shared__ uint8_t sCons[CU_TILE];
    __shared__ int sAcc[CU_THREADS][5];
    __shared__ unsigned int sN;
    const uint64_t t = first + blockIdx.x;
    if (t >= nTiles) return;                    // (uniform over the block)
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t q = a.tileQ[t];
    const SeqMeta qm = a.meta[q];
    const uint32_t qLen = qm.len;
    const uint32_t tileLo = a.lo[q] + (uint32_t) (t - a.tOff[q]) * CU_TILE, tileHi = min(tileLo + CU_TILE, a.hi[q]);
    const uint32_t p0 = tileLo + CU_PER_THREAD * tid;          // this thread's positions: p0 .. p0 + CU_PER_THREAD - 1
    const uint64_t r0 = a.aoff[q], r1 = a.aoff[q + 1];
    for (int i = tid; i < CU_THREADS * 5; i += CU_THREADS) (&sAcc[0][0])[i] = 0;
    // ---- 1. the letters of the contributors at this thread's positions (the middle third is the query's: none needed there)
    uint32_t cnt[CU_PER_THREAD][4];
#pragma unroll
    for (int k = 0; k < CU_PER_THREAD; k++) cnt[k][0] = cnt[k][1] = cnt[k][2] = cnt[k][3] = 0;
    const bool allMid = tileLo >= qLen && (uint64_t) tileHi <= 2ull * qLen;
    if (!allMid) {
        for (uint64_t base = r0; base < r1; base += CU_THREADS) {
            if (tid == 0) sN = 0;
            __syncthreads();
            const uint64_t r = base + tid;
            if (r < r1) {
                const CuRec c = a.cu[r];
                if (c.start != CU_NONE && c.start < tileHi && (uint64_t) c.start + c.len > tileLo) sRec[atomicAdd(&sN, 1u)] = c;
            }
            __syncthreads();
            const uint32_t nc = sN;
            if (p0 < tileHi)
                for (uint32_t i = 0; i < nc; i++) {
                    uint32_t code[CU_PER_THREAD], on, isN;
                    if (!lettersAt(a, sRec[i], sRec[i].start, p0, code, on, isN)) continue;
#pragma unroll
                    for (int k = 0; k < CU_PER_THREAD; k++) {
                        const uint32_t p = p0 + k;
                        if ((on >> k) & 1u && p < tileHi && !(p >= qLen && p < 2u * qLen)) {
                            cnt[k][0] += code[k] == 0u; cnt[k][1] += code[k] == 1u; cnt[k][2] += code[k] == 2u; cnt[k][3] += code[k] == 3u;
                        }
                    }
                }
            __syncthreads();
        }
    }
    // ---- 2. the consensus letters (4 = N): calculateConsensus' majority, the query in the middle third
#pragma unroll
    for (int k = 0; k < CU_PER_THREAD; k++) {
        const uint32_t p = p0 + k;
        uint32_t cl = 4;
        if (p < tileHi) {
            if (p >= qLen && p < 2u * qLen) {
                const uint32_t qp = p - qLen;
                cl = ((qm.flags & 1u) && cdm_isN(a.nmask, qm.woff, qp)) ? 4u : cdm_base(a.codes, qm.woff, qp);
            } else if (cnt[k][0] + cnt[k][1] + cnt[k][2] + cnt[k][3] >= a.minCov) {
                uint32_t mx = 0, nuc = 4; int nMax = 0;
                for (int j = 0; j < 4; j++) { if (cnt[k][j] > mx) { mx = cnt[k][j]; nuc = (uint32_t) j; nMax = 1; } else if (cnt[k][j] == mx && mx > 0) nMax++; }
                cl = nMax > 1 ? 4u : nuc;
            }
        }
        sCons[CU_PER_THREAD * tid + k] = (uint8_t) cl;
    }
    // ---- 3. the column records against them
    for (uint64_t base = r0; base < r1; base += CU_THREADS) {
        if (tid == 0) sN = 0;
        __syncthreads();
        const uint64_t r = base + tid;
        if (r < r1) {
            const CuRec c = a.cu[r];
            if (c.c0 != CU_NONE && c.c0 < tileHi && (uint64_t) c.c0 + c.len > tileLo) { const uint32_t slot = atomicAdd(&sN, 1u); sRec[slot] = c; sIdx[slot] = (uint32_t) (r - r0); }
        }
        __syncthreads();
        const uint32_t nc = sN;
        for (uint32_t i = 0; i < nc; i++) {
            uint32_t code[CU_PER_THREAD] = {0, 0, 0, 0}, on = 0, isN = 0;
            if (!(p0 < tileHi && lettersAt(a, sRec[i], sRec[i].c0, p0, code, on, isN))) on = 0;
            int tot = 0, idc = 0, idr = 0, nCT = 0, nGA = 0;
#pragma unroll
            for (int k = 0; k < CU_PER_THREAD; k++) {
                const uint32_t cq = sCons[CU_PER_THREAD * tid + k], tl = code[k];
                const bool def = ((on & ~isN) >> k) & 1u && p0 + k < tileHi && cq != 4u;
                tot += __popcll(__ballot(def)); idc += __popcll(__ballot(def && cq == tl)); idr += __popcll(__ballot(def && (cq & 1u) == (tl & 1u)));
                nCT += __popcll(__ballot(def && cq == 1u && tl == 3u)); nGA += __popcll(__ballot(def && cq == 2u && tl == 0u));
            }
            if (lane == 0 && tot) { atomicAdd(&sAcc[i][0], tot); atomicAdd(&sAcc[i][1], idc); atomicAdd(&sAcc[i][2], idr); atomicAdd(&sAcc[i][3], nCT); atomicAdd(&sAcc[i][4], nGA); }
        }
        __syncthreads();
        if ((uint32_t) tid < nc) {
            int *dst = a.acc + (r0 + sIdx[tid]) * 5;
            for (int j = 0; j < 5; j++) { if (sAcc[tid][j]) atomicAdd(dst + j, sAcc[tid][j]); sAcc[tid][j] = 0; }
        }
        __syncthreads();
    }
}

// a thread per record: the column records' five counts into the statistics the gate reads
__global__ __launch_bounds__(256) void k_cu_store(CuArgs a, ContigStat *__restrict__ st) {
    const uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.nRec || !(a.cu[r].flags & CU_COLUMN)) return;
    const int *v = a.acc + r * 5;
    ContigStat &s = st[r];
    s.nnTot = v[0]; s.nnId = v[1]; s.nnRy = v[2]; s.nCT = v[3]; s.nGA = v[4];
}
}  // namespace

int cdm_contig_unsafe_columns(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const cdm_ancient_params *par, float mergeSeqIdThr, const SeqMeta *meta,
                              const uint32_t *owner, ContigStat *dStats, uint8_t *handBack) {
    hipStream_t s = ctx->stream;
    const uint32_t n = (uint32_t) db->n;
    const uint64_t nRec = alns->count;
    const bool timing = cdmGetenv("CDM_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    DevBuf<CuRec> cu; DevBuf<uint32_t> lo, hi; DevBuf<uint64_t> tiles, tOff; DevBuf<int> acc; DevBuf<unsigned int> counters;
    if (!cu.alloc(nRec) || !lo.alloc(n) || !hi.alloc(n) || !tiles.alloc((size_t) n + 1) || !tOff.alloc((size_t) n + 1) || !acc.alloc(nRec * 5) || !counters.alloc(4)) {
        cdm_set_error("cdm_contig_merge: out of device memory"); return CDM_ERR_HIP;
    }
    CuArgs a;
    a.meta = meta; a.codes = db->codes; a.nmask = db->nmask; a.aoff = alns->off; a.rec = alns->rec; a.owner = owner; a.nRec = nRec; a.n = n;
    a.mergeThr = mergeSeqIdThr; a.ryThr = par->ry_seq_id_thr; a.minCov = (uint32_t) std::max(0, par->min_cov_safe);
    a.tileQ = nullptr; a.cu = cu.p; a.lo = lo.p; a.hi = hi.p; a.handBack = handBack; a.tiles = tiles.p; a.tOff = tOff.p; a.acc = acc.p; a.counters = counters.p;
    CDM_HIP(hipMemsetAsync(counters.p, 0, 16, s));
    if (n) { CDM_HIP(hipMemsetAsync(lo.p, 0xFF, (size_t) n * 4, s)); CDM_HIP(hipMemsetAsync(hi.p, 0, (size_t) n * 4, s)); CDM_HIP(hipMemsetAsync(handBack, 0, n, s)); }
    if (nRec) {
        CDM_HIP(hipMemsetAsync(acc.p, 0, nRec * 5 * sizeof(int), s));
        hipLaunchKernelGGL(k_cu_rec, CDM_GRID((nRec + 255) / 256, 256), dim3(256), 0, s, a, (const ContigStat *) dStats);
    }
    hipLaunchKernelGGL(k_cu_tiles, dim3((n + 256) / 256), dim3(256), 0, s, a);
    cdmscan::ScanTemp st;
    if (cdmscan::exclusiveScan<uint64_t>(s, st, tiles.p, tOff.p, (size_t) n + 1) != CDM_OK) { cdm_set_error("cdm_contig_merge: scan failed"); return CDM_ERR_HIP; }
    uint64_t nTiles = 0; unsigned int hc[4];
    CDM_HIP(hipMemcpyAsync(&nTiles, tOff.p + n, 8, hipMemcpyDeviceToHost, s));
    CDM_HIP(hipMemcpyAsync(hc, counters.p, 16, hipMemcpyDeviceToHost, s));
    CDM_HIP(hipStreamSynchronize(s));
    if (hc[0]) { cdm_set_error("cdm_contig_merge: a target overhangs its query by more than the query's length; the reference pads it with a negative number of letters there (undefined behaviour), not reproduced"); return CDM_ERR_UNSUPPORTED; }
    DevBuf<uint32_t> tileQ;
    if (!tileQ.alloc(nTiles)) { cdm_set_error("cdm_contig_merge: out of device memory"); return CDM_ERR_HIP; }
    a.tileQ = tileQ.p;
    if (n) hipLaunchKernelGGL(k_cu_map, dim3((n + 255) / 256), dim3(256), 0, s, a);
    for (uint64_t first = 0, slice = cdmSliceItems(CU_THREADS); first < nTiles; first += slice)
        hipLaunchKernelGGL(k_cu_tile, CDM_GRID(std::min(slice, nTiles - first), CU_THREADS), dim3(CU_THREADS), 0, s, a, first, nTiles);
    if (nRec) hipLaunchKernelGGL(k_cu_store, CDM_GRID((nRec + 255) / 256, 256), dim3(256), 0, s, a, dStats);
    if (hipStreamSynchronize(s) != hipSuccess) { cdm_set_error("cdm_contig_merge: the unsafe-mode columns failed: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP; }
    if (timing)
        fprintf(stderr, "  contig merge: unsafe consensus columns (device) %.3f s: %u queries, %u column records, %llu tiles, %u queries handed back\n",
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), hc[3], hc[2], (unsigned long long) nTiles, hc[1]);
    return CDM_OK;
}
