// Test-only harness over the device primitives of carpedeam_amd/csrc (radix.h, scan.h, bucket.h, devutil.h): one extern "C" entry
// point per primitive and type combination the product instantiates, and two for the sequence DB constructors that have no C-ABI
// entry (prim_seqdb_select, prim_seqdb_overlay: opaque handles of the library in and out).  Every entry point takes HOST pointers, allocates with the
// library's allocator, copies in, runs the primitive on the stream handed in, synchronises, copies out and returns the primitive's
// own status.  Built by tests/primkit.py into tests/_build/libcdm_primitives.so and linked against libcarpedeam_hip.so (cdmMallocRaw,
// cdmFree, cdm_set_error, cdmGetenv, cdm_seqdb_select, cdm_seqdb_overlay); never loaded by the package or by bench.py.
#include "seqdb.h"
#include "devutil.h"
#include "scan.h"
#include "radix.h"
#include "bucket.h"

namespace {

typedef uint64_t u64;
typedef uint32_t u32;
typedef uint8_t u8;

template <typename T> int up(DevBuf<T> &d, const T *h, size_t n) {
    if (!d.alloc(n)) { cdm_set_error("primitives harness: out of device memory"); return CDM_ERR_HIP; }
    if (n) CDM_HIP(hipMemcpy(d.p, h, n * sizeof(T), hipMemcpyHostToDevice));
    return CDM_OK;
}
template <typename T> int room(DevBuf<T> &d, size_t n) {
    if (!d.alloc(n)) { cdm_set_error("primitives harness: out of device memory"); return CDM_ERR_HIP; }
    CDM_HIP(hipMemset(d.p, 0, (n + 1) * sizeof(T)));
    return CDM_OK;
}
template <typename T> int down(T *h, const T *d, size_t n) {
    if (n) CDM_HIP(hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost));
    return CDM_OK;
}
#define TRY(expr) do { if (int _rc = (expr)) return _rc; } while (0)

// ---------------------------------------------------------------------------------------------- radix.h
template <typename K, typename V>
int sortPairsHost(void *stream, int cuCount, const K *k, const V *v, u64 n, int beginBit, int endBit, K *kOut, V *vOut, int *inFirstOut) {
    hipStream_t s = (hipStream_t) stream;
    DevBuf<K> k0, k1;
    TRY(up(k0, k, n)); TRY(room(k1, n));
    bool inFirst = true;
    if constexpr (rx::HasValue<V>::value) {
        DevBuf<V> v0, v1;
        TRY(up(v0, v, n)); TRY(room(v1, n));
        TRY((rx::sortPairs<K, V>(s, cuCount, k0.p, k1.p, v0.p, v1.p, n, beginBit, endBit, inFirst)));
        CDM_HIP(hipStreamSynchronize(s));
        TRY(down(vOut, inFirst ? v0.p : v1.p, n));
    } else {
        TRY((rx::sortKeys<K>(s, cuCount, k0.p, k1.p, n, beginBit, endBit, inFirst)));
        CDM_HIP(hipStreamSynchronize(s));
    }
    TRY(down(kOut, inFirst ? k0.p : k1.p, n));
    *inFirstOut = inFirst ? 1 : 0;
    return CDM_OK;
}

template <typename K, typename V>
int compactPairsHost(void *stream, const K *k, const V *v, u64 n, K *kOut, V *vOut, u64 *total) {
    hipStream_t s = (hipStream_t) stream;
    DevBuf<K> k0, k1; DevBuf<V> v0, v1; DevBuf<unsigned long long> tot;
    TRY(up(k0, k, n)); TRY(up(v0, v, n)); TRY(room(k1, n)); TRY(room(v1, n)); TRY(room(tot, 1));
    TRY((rx::compactPairs<K, V>(s, k0.p, v0.p, n, k1.p, v1.p, tot.p)));
    CDM_HIP(hipStreamSynchronize(s));
    unsigned long long t = 0;
    TRY(down(&t, tot.p, 1));
    *total = t;
    TRY(down(kOut, k1.p, n)); TRY(down(vOut, v1.p, n));
    return CDM_OK;
}

// ---------------------------------------------------------------------------------------------- scan.h
template <typename T>
int exclScanHost(void *stream, const T *in, T *out, u64 n, int inPlace) {
    hipStream_t s = (hipStream_t) stream;
    DevBuf<T> a, b;
    TRY(up(a, in, n));
    if (!inPlace) TRY(room(b, n));
    T *o = inPlace ? a.p : b.p;
    {
        cdmscan::ScanTemp tmp;          // alive until the stream has been synchronised
        const int rc = cdmscan::exclusiveScan<T>(s, tmp, a.p, o, (size_t) n);
        const hipError_t e = hipStreamSynchronize(s);
        if (rc) return rc;
        CDM_HIP(e);
    }
    return down(out, o, n);
}

// ---------------------------------------------------------------------------------------------- devutil.h
struct FoldArgs { const double *t; u64 rows; int cols; int acc; u64 *m; int32_t *e; u32 *s; double *d; };
__global__ __launch_bounds__(256) void k_x87_fold(FoldArgs a) {
    const u64 r = (u64) blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.rows) return;
    X87 sum = x87_zero();
    for (int j = 0; j < a.cols; j++) {
        const X87 t = x87_from_double(a.t[r * (u64) a.cols + j]);
        sum = a.acc ? x87_acc(sum, t) : x87_add(sum, t);
    }
    a.m[r] = sum.m; a.e[r] = sum.e; a.s[r] = sum.s; a.d[r] = x87_to_double(sum);
}
__global__ __launch_bounds__(256) void k_x87_lt(const u64 *am, const int32_t *ae, const u32 *as, const u64 *bm, const int32_t *be, const u32 *bs, u64 n, u8 *out) {
    const u64 i = (u64) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    X87 a, b; a.m = am[i]; a.e = ae[i]; a.s = as[i]; b.m = bm[i]; b.e = be[i]; b.s = bs[i];
    out[i] = x87_lt(a, b) ? 1 : 0;
}
// one value per thread of every block; out = exclusive prefix inside the block, tot = the block's sum as that thread sees it
template <typename T>
__global__ void k_block_excl_sum(const T *in, T *out, T *tot) {
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    T t;
    out[i] = cdm_block_excl_sum<T>(in[i], t);
    tot[i] = t;
}
template <typename T>
int blockExclSumHost(void *stream, const T *in, u32 blocks, u32 threads, T *out, T *tot) {
    if (threads == 0 || threads % 64 || threads > 1024) { cdm_set_error("primitives harness: block of %u threads", threads); return CDM_ERR_INVALID; }
    hipStream_t s = (hipStream_t) stream;
    const size_t n = (size_t) blocks * threads;
    DevBuf<T> a, o, t;
    TRY(up(a, in, n)); TRY(room(o, n)); TRY(room(t, n));
    if (blocks) hipLaunchKernelGGL(k_block_excl_sum<T>, dim3(blocks), dim3(threads), 0, s, (const T *) a.p, o.p, t.p);
    CDM_HIP(hipGetLastError());
    CDM_HIP(hipStreamSynchronize(s));
    TRY(down(out, o.p, n));
    return down(tot, t.p, n);
}
template <bool BLOCK>
__global__ void k_append(const u8 *pred, u32 *slot, unsigned int *counter) {
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    const bool p = pred[i] != 0;
    const u32 r = BLOCK ? cdm_block_append(counter, p) : cdm_wave_append(counter, p);
    slot[i] = p ? r : 0xFFFFFFFFu;
}
template <bool BLOCK>
int appendHost(void *stream, const u8 *pred, u32 blocks, u32 threads, u32 *slot, u32 *counter) {
    if (threads == 0 || threads % 64 || threads > 1024) { cdm_set_error("primitives harness: block of %u threads", threads); return CDM_ERR_INVALID; }
    hipStream_t s = (hipStream_t) stream;
    const size_t n = (size_t) blocks * threads;
    DevBuf<u8> p; DevBuf<u32> sl; DevBuf<unsigned int> c;
    TRY(up(p, pred, n)); TRY(room(sl, n)); TRY(room(c, 1));
    if (blocks) hipLaunchKernelGGL(k_append<BLOCK>, dim3(blocks), dim3(threads), 0, s, (const u8 *) p.p, sl.p, c.p);
    CDM_HIP(hipGetLastError());
    CDM_HIP(hipStreamSynchronize(s));
    TRY(down(slot, sl.p, n));
    return down(counter, (const u32 *) c.p, 1);
}
enum { OP_REVCOMP16 = 0, OP_SPREAD16 = 1, OP_SQUASH16 = 2 };
__global__ __launch_bounds__(256) void k_bitop(const u32 *in, u64 n, int op, u32 *out) {
    const u64 i = (u64) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 x = in[i];
    out[i] = op == OP_REVCOMP16 ? cdm_revcomp16(x) : op == OP_SPREAD16 ? cdm_spread16(x) : cdm_squash16(x);
}
enum { WIN_PLAIN = 0, WIN_FORWARD = 1, WIN_REVERSE = 2 };
// the 16-base window at every (oriented) start position i < L of one sequence stored from word 0 on
__global__ __launch_bounds__(256) void k_windows(const u32 *codes, u32 L, int mode, u32 *out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L) return;
    const u32 lastWord = (L - 1u) >> 4;
    out[i] = mode == WIN_PLAIN ? cdm_window16(codes, 0u, i, lastWord) : cdm_oriented_window16(codes, 0u, L, lastWord, mode == WIN_REVERSE, i);
}

}  // namespace

#define PRIM_SORT_PAIRS(name, K, V) \
    extern "C" int name(void *stream, int cuCount, const K *k, const V *v, u64 n, int beginBit, int endBit, K *kOut, V *vOut, int *inFirst) { \
        return sortPairsHost<K, V>(stream, cuCount, k, v, n, beginBit, endBit, kOut, vOut, inFirst); }
PRIM_SORT_PAIRS(prim_sort_pairs_u64_u64, u64, u64)
PRIM_SORT_PAIRS(prim_sort_pairs_u64_u32, u64, u32)
PRIM_SORT_PAIRS(prim_sort_pairs_u32_u32, u32, u32)
PRIM_SORT_PAIRS(prim_sort_pairs_u32_u64, u32, u64)
extern "C" int prim_sort_keys_u64(void *stream, int cuCount, const u64 *k, u64 n, int beginBit, int endBit, u64 *kOut, int *inFirst) {
    return sortPairsHost<u64, rx::NoValue>(stream, cuCount, k, nullptr, n, beginBit, endBit, kOut, nullptr, inFirst);
}

#define PRIM_COMPACT_PAIRS(name, K, V) \
    extern "C" int name(void *stream, const K *k, const V *v, u64 n, K *kOut, V *vOut, u64 *total) { return compactPairsHost<K, V>(stream, k, v, n, kOut, vOut, total); }
PRIM_COMPACT_PAIRS(prim_compact_pairs_u64_u64, u64, u64)
PRIM_COMPACT_PAIRS(prim_compact_pairs_u64_u32, u64, u32)
PRIM_COMPACT_PAIRS(prim_compact_pairs_u64_u8, u64, u8)

// keys: n slot keys; headHist: NULL or the [512] head digit counts of the real keys; out: seg[513], *live, result[n] (the first
// *live words are the sorted slot tuples)
extern "C" int prim_sort_slot_keys(void *stream, int cuCount, const u64 *keys, u64 n, int topBit, int lowBits, const u64 *headHist, u32 keepLo, u32 keepHi,
                                   u64 *seg, u64 *live, u64 *result) {
    hipStream_t s = (hipStream_t) stream;
    DevBuf<u64> k0, k1; DevBuf<unsigned long long> hh, sg;
    TRY(up(k0, keys, n)); TRY(room(k1, n)); TRY(room(sg, rx::BINS + 1));
    if (headHist) TRY(up(hh, reinterpret_cast<const unsigned long long *>(headHist), rx::BINS));
    unsigned long long lv = 0; u64 *res = nullptr;
    const int rc = rx::sortSlotKeys(s, cuCount, k0.p, k1.p, n, topBit, lowBits, headHist ? hh.p : nullptr, sg.p, lv, res, nullptr, nullptr, keepLo, keepHi);
    const hipError_t e = hipStreamSynchronize(s);
    if (rc) return rc;
    CDM_HIP(e);
    *live = lv;
    TRY(down(reinterpret_cast<unsigned long long *>(seg), sg.p, rx::BINS + 1));
    if (lv > n) { cdm_set_error("primitives harness: %llu live tuples of %llu slots", lv, (unsigned long long) n); return CDM_ERR_HIP; }
    return down(result, res, lv);
}

extern "C" int prim_excl_scan_u32(void *stream, const u32 *in, u32 *out, u64 n, int inPlace) { return exclScanHost<u32>(stream, in, out, n, inPlace); }
extern "C" int prim_excl_scan_u64(void *stream, const u64 *in, u64 *out, u64 n, int inPlace) {
    return exclScanHost<unsigned long long>(stream, reinterpret_cast<const unsigned long long *>(in), reinterpret_cast<unsigned long long *>(out), n, inPlace);
}
extern "C" int prim_incl_max_scan(void *stream, const u64 *in, u64 *out, u64 n, int inPlace) {
    hipStream_t s = (hipStream_t) stream;
    DevBuf<cdmscan::mx_t> a, b;
    TRY(up(a, reinterpret_cast<const cdmscan::mx_t *>(in), n));
    if (!inPlace) TRY(room(b, n));
    cdmscan::mx_t *o = inPlace ? a.p : b.p;
    {
        cdmscan::ScanTemp tmp;
        const int rc = cdmscan::inclusiveMaxScanFn(s, tmp, cdmscan::LoadArray<cdmscan::mx_t>{a.p}, o, (size_t) n);
        const hipError_t e = hipStreamSynchronize(s);
        if (rc) return rc;
        CDM_HIP(e);
    }
    return down(reinterpret_cast<cdmscan::mx_t *>(out), o, n);
}

extern "C" int prim_bucket_sort_keys(void *stream, const u64 *in, u64 *out, u64 n, int shiftHi, int ign, int top) {
    hipStream_t s = (hipStream_t) stream;
    DevBuf<u64> a, b;
    TRY(up(a, in, n)); TRY(room(b, n));
    TRY(bucket::bucketSortKeys(s, a.p, b.p, n, shiftHi, ign, top));
    CDM_HIP(hipStreamSynchronize(s));
    return down(out, b.p, n);
}

// terms: rows x cols doubles; every row is folded left to right from +0 with x87_add (acc == 0) or x87_acc
extern "C" int prim_x87_fold(void *stream, const double *terms, u64 rows, int cols, int acc, u64 *m, int32_t *e, u32 *sgn, double *d) {
    hipStream_t s = (hipStream_t) stream;
    DevBuf<double> t, dd; DevBuf<u64> mm; DevBuf<int32_t> ee; DevBuf<u32> ss;
    TRY(up(t, terms, rows * (u64) cols)); TRY(room(mm, rows)); TRY(room(ee, rows)); TRY(room(ss, rows)); TRY(room(dd, rows));
    FoldArgs a; a.t = t.p; a.rows = rows; a.cols = cols; a.acc = acc; a.m = mm.p; a.e = ee.p; a.s = ss.p; a.d = dd.p;
    if (rows) hipLaunchKernelGGL(k_x87_fold, dim3((unsigned) ((rows + 255) / 256)), dim3(256), 0, s, a);
    CDM_HIP(hipGetLastError());
    CDM_HIP(hipStreamSynchronize(s));
    TRY(down(m, mm.p, rows)); TRY(down(e, ee.p, rows)); TRY(down(sgn, ss.p, rows));
    return down(d, dd.p, rows);
}
extern "C" int prim_x87_lt(void *stream, const u64 *am, const int32_t *ae, const u32 *as, const u64 *bm, const int32_t *be, const u32 *bs, u64 n, u8 *out) {
    hipStream_t s = (hipStream_t) stream;
    DevBuf<u64> dam, dbm; DevBuf<int32_t> dae, dbe; DevBuf<u32> das, dbs; DevBuf<u8> o;
    TRY(up(dam, am, n)); TRY(up(dae, ae, n)); TRY(up(das, as, n)); TRY(up(dbm, bm, n)); TRY(up(dbe, be, n)); TRY(up(dbs, bs, n)); TRY(room(o, n));
    if (n) hipLaunchKernelGGL(k_x87_lt, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, (const u64 *) dam.p, (const int32_t *) dae.p, (const u32 *) das.p,
                              (const u64 *) dbm.p, (const int32_t *) dbe.p, (const u32 *) dbs.p, n, o.p);
    CDM_HIP(hipGetLastError());
    CDM_HIP(hipStreamSynchronize(s));
    return down(out, o.p, n);
}

extern "C" int prim_block_excl_sum_u32(void *stream, const u32 *in, u32 blocks, u32 threads, u32 *out, u32 *tot) { return blockExclSumHost<u32>(stream, in, blocks, threads, out, tot); }
extern "C" int prim_block_excl_sum_u64(void *stream, const u64 *in, u32 blocks, u32 threads, u64 *out, u64 *tot) {
    return blockExclSumHost<unsigned long long>(stream, reinterpret_cast<const unsigned long long *>(in), blocks, threads, reinterpret_cast<unsigned long long *>(out),
                                                reinterpret_cast<unsigned long long *>(tot));
}
// pred: one byte per thread of blocks x threads; slot = what the append returned where pred is set (0xFFFFFFFF elsewhere)
extern "C" int prim_wave_append(void *stream, const u8 *pred, u32 blocks, u32 threads, u32 *slot, u32 *counter) { return appendHost<false>(stream, pred, blocks, threads, slot, counter); }
extern "C" int prim_block_append(void *stream, const u8 *pred, u32 blocks, u32 threads, u32 *slot, u32 *counter) { return appendHost<true>(stream, pred, blocks, threads, slot, counter); }

// op: 0 cdm_revcomp16, 1 cdm_spread16, 2 cdm_squash16
extern "C" int prim_bitop16(void *stream, const u32 *in, u64 n, int op, u32 *out) {
    if (op < OP_REVCOMP16 || op > OP_SQUASH16) { cdm_set_error("primitives harness: bit operation %d", op); return CDM_ERR_INVALID; }
    hipStream_t s = (hipStream_t) stream;
    DevBuf<u32> a, o;
    TRY(up(a, in, n)); TRY(room(o, n));
    if (n) hipLaunchKernelGGL(k_bitop, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, (const u32 *) a.p, n, op, o.p);
    CDM_HIP(hipGetLastError());
    CDM_HIP(hipStreamSynchronize(s));
    return down(out, o.p, n);
}
// codes: the (L + 15) / 16 words of one sequence of L >= 1 bases; mode: 0 cdm_window16, 1 / 2 cdm_oriented_window16 forward / reverse; out[L]
extern "C" int prim_windows16(void *stream, const u32 *codes, u32 L, int mode, u32 *out) {
    if (L == 0 || mode < WIN_PLAIN || mode > WIN_REVERSE) { cdm_set_error("primitives harness: windows of %u bases, mode %d", L, mode); return CDM_ERR_INVALID; }
    hipStream_t s = (hipStream_t) stream;
    DevBuf<u32> c, o;
    TRY(up(c, codes, (size_t) (L + 15u) / 16u)); TRY(room(o, L));
    hipLaunchKernelGGL(k_windows, dim3((L + 255u) / 256u), dim3(256), 0, s, (const u32 *) c.p, L, mode, o.p);
    CDM_HIP(hipGetLastError());
    CDM_HIP(hipStreamSynchronize(s));
    return down(out, o.p, L);
}

// ---------------------------------------------------------------------------------------------- sequence DB constructors without an ABI entry
// sel: one value per sequence of db (host)
extern "C" int prim_seqdb_select(cdm_ctx *ctx, const cdm_seqdb *db, const u32 *sel, int extValue, cdm_seqdb **out) {
    CDM_HIP(hipSetDevice(ctx->device));
    DevBuf<u32> d;
    TRY(up(d, sel, (size_t) db->n));
    return cdm_seqdb_select(ctx, db, d.p, extValue, out);
}
// grown (and idx) may be NULL: nothing replaced; idx: one entry of base per sequence of grown, ext: one flag per sequence of base (host)
extern "C" int prim_seqdb_overlay(cdm_ctx *ctx, const cdm_seqdb *base, const cdm_seqdb *grown, const u32 *idx, const u8 *ext, cdm_seqdb **out) {
    return cdm_seqdb_overlay(ctx, base, grown, idx, ext, out);
}
