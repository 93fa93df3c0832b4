// The device-resident sequence DB (struct cdm_seqdb, common.h): allocation, 2-bit packing and unpacking of text, and every way a DB is
// made from another - select, overlay, concat, the packed forms to and from device and host memory.  Internal interface: seqdb.h.
// Every constructor is put together from cdm_seqdb_alloc + seqdbAllocPlanes (arrays, then planes once the code words are counted),
// seqdbLayout (lengths -> word offsets), seqdbGather, seqdbPackText / seqdbUnpackText, seqdbLenStats and seqOfWord.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>
#include "seqdb.h"
#include "devutil.h"
#include "scan.h"

// ------------------------------------------------------------------------------------------------ handles and planes
int cdm_seqdb_alloc(cdm_ctx *ctx, uint64_t n, cdm_seqdb **out) {
    static std::atomic<uint64_t> nextSerial{1};
    cdm_seqdb *db = new cdm_seqdb();
    db->serial = nextSerial++;
    db->n = n; db->device = ctx->device;
    if (cdmMalloc(&db->woff, (n + 1) * sizeof(uint32_t)) != hipSuccess || cdmMalloc(&db->len, (n + 1) * sizeof(uint32_t)) != hipSuccess ||
        cdmMalloc(&db->key, (n + 1) * sizeof(uint32_t)) != hipSuccess || cdmMalloc(&db->ext, n + 1) != hipSuccess ||
        cdmMalloc(&db->hasN, n + 8) != hipSuccess) {
        cdm_set_error("out of device memory allocating a %llu-entry sequence DB", (unsigned long long) n);
        cdm_seqdb_free(db); return CDM_ERR_HIP;
    }
    *out = db;
    return CDM_OK;
}
int cdm_seqdb_alloc_raw(cdm_seqdb *db) {
    if (db->raw) return CDM_OK;
    if (cdmMalloc(&db->raw, db->words * 16 + 16) != hipSuccess) { cdm_set_error("out of device memory allocating the original letters of %llu code words", (unsigned long long) db->words); return CDM_ERR_HIP; }
    return CDM_OK;
}
int seqdbAllocPlanes(cdm_seqdb *db, uint64_t words, bool withRaw) {
    db->words = words;
    if (cdmMalloc(&db->codes, (words + 2) * sizeof(uint32_t)) != hipSuccess || cdmMalloc(&db->nmask, seqdbMaskBytes(words)) != hipSuccess) {
        cdm_set_error("out of device memory allocating %llu code words", (unsigned long long) words); return CDM_ERR_HIP;
    }
    return withRaw ? cdm_seqdb_alloc_raw(db) : CDM_OK;
}
int cdm_seqdb_alloc_like(cdm_ctx *ctx, const cdm_seqdb *src, cdm_seqdb **out) {
    cdm_seqdb *db = nullptr;
    int rc = cdm_seqdb_alloc(ctx, src->n, &db);
    if (rc) return rc;
    db->residues = src->residues; db->maxLen = src->maxLen; db->nCount = src->nCount;
    if ((rc = seqdbAllocPlanes(db, src->words, src->raw != nullptr)) != CDM_OK) { cdm_seqdb_free(db); return rc; }
    hipStream_t s = ctx->stream;
    CDM_HIP(hipMemcpyAsync(db->woff, src->woff, (src->n + 1) * 4, hipMemcpyDeviceToDevice, s));
    CDM_HIP(hipMemcpyAsync(db->len, src->len, src->n * 4, hipMemcpyDeviceToDevice, s));
    CDM_HIP(hipMemcpyAsync(db->key, src->key, src->n * 4, hipMemcpyDeviceToDevice, s));
    CDM_HIP(hipMemcpyAsync(db->ext, src->ext, src->n, hipMemcpyDeviceToDevice, s));
    CDM_HIP(hipMemcpyAsync(db->hasN, src->hasN, src->n, hipMemcpyDeviceToDevice, s));
    *out = db;
    return CDM_OK;
}
extern "C" void cdm_seqdb_free(cdm_seqdb *db) {
    if (!db) return;
    hipSetDevice(db->device);
    cdmFree(db->woff); cdmFree(db->len); cdmFree(db->key); cdmFree(db->ext); cdmFree(db->hasN); cdmFree(db->codes); cdmFree(db->nmask); cdmFree(db->raw);
    delete db;
}
extern "C" uint64_t cdm_seqdb_size(const cdm_seqdb *db) { return db->n; }
extern "C" uint64_t cdm_seqdb_residues(const cdm_seqdb *db) { return db->residues; }
extern "C" uint32_t cdm_seqdb_max_len(const cdm_seqdb *db) { return db->maxLen; }
extern "C" uint64_t cdm_seqdb_words(const cdm_seqdb *db) { return db->words; }
extern "C" int cdm_seqdb_has_raw(const cdm_seqdb *db) { return db->raw ? 1 : 0; }

__global__ void k_build_meta(const uint32_t *__restrict__ woff, const uint32_t *__restrict__ len, const uint8_t *__restrict__ hasN, const uint8_t *__restrict__ ext,
                             const uint32_t *__restrict__ key, uint32_t n, SeqMeta *__restrict__ out, uint32_t uniLen, uint32_t uniWords, unsigned int *__restrict__ notUniform) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    SeqMeta m; m.woff = woff[i]; m.len = len[i]; m.flags = (hasN[i] ? 1u : 0u) | (ext[i] ? 2u : 0u) | ((hasN[i] & 2u) ? 4u : 0u); m.key = key[i];
    out[i] = m;
    if (notUniform && (m.len != uniLen || m.woff != i * uniWords || m.flags != 0u)) atomicOr(notUniform, 1u);
}
// CDM_META_UNIFORM=0: the records for every DB (A/B)
int cdm_build_meta(cdm_ctx *ctx, const cdm_seqdb *db, SeqMeta **out, MetaUniform *uniform) {
    SeqMeta *m = nullptr;
    if (cdmMalloc(&m, (db->n + 1) * sizeof(SeqMeta)) != hipSuccess) { cdm_set_error("out of device memory (sequence metadata)"); return CDM_ERR_HIP; }
    // a candidate for the plain uniform form: the lengths sum to n x the longest, no N counted, no row of original letters (nCount is a
    // lower bound, common.h: the kernel's look at the flags decides)
    const char *sw = cdmGetenv("CDM_META_UNIFORM");
    const bool candidate = uniform && db->n && db->maxLen && db->residues == db->n * (uint64_t) db->maxLen && db->nCount == 0 && !db->raw && !(sw && !strcmp(sw, "0")) &&
                           db->n * (uint64_t) ((db->maxLen + 15) / 16) < (1ull << 32);
    DevBuf<unsigned int> bad;
    if (candidate) { if (!bad.alloc(1)) { cdmFree(m); cdm_set_error("out of device memory (sequence metadata)"); return CDM_ERR_HIP; } hipMemsetAsync(bad.p, 0, 4, ctx->stream); }
    if (db->n) hipLaunchKernelGGL(k_build_meta, dim3((unsigned) ((db->n + 255) / 256)), dim3(256), 0, ctx->stream, db->woff, db->len, db->hasN, db->ext, db->key, (uint32_t) db->n, m,
                                  db->maxLen, (db->maxLen + 15) / 16, candidate ? bad.p : nullptr);
    if (uniform) { uniform->words = 0; uniform->len = 0; }
    if (candidate) {
        unsigned int h = 1;
        if (hipMemcpyAsync(&h, bad.p, 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { cdmFree(m); cdm_set_error("sequence metadata: %s", hipGetErrorString(hipGetLastError())); return CDM_ERR_HIP; }
        if (!h) { uniform->words = (db->maxLen + 15) / 16; uniform->len = db->maxLen; }
    }
    *out = m;
    return CDM_OK;
}
extern "C" int cdm_seqdb_meta(cdm_ctx *ctx, const cdm_seqdb *db, uint32_t *lengths, uint32_t *keys, uint8_t *ext) {
    CDM_HIP(hipSetDevice(ctx->device));
    if (lengths) CDM_HIP(hipMemcpyAsync(lengths, db->len, db->n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (keys) CDM_HIP(hipMemcpyAsync(keys, db->key, db->n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (ext) CDM_HIP(hipMemcpyAsync(ext, db->ext, db->n, hipMemcpyDeviceToHost, ctx->stream));
    CDM_HIP(hipStreamSynchronize(ctx->stream));
    return CDM_OK;
}

// ------------------------------------------------------------------------------------------------ shared steps
namespace {
// sum and maximum of the lengths, on the device (the host needs two numbers of a DB it composed, not its 50 M lengths)
__global__ __launch_bounds__(256) void k_len_stats(const uint32_t *__restrict__ len, uint64_t n, unsigned long long *__restrict__ out) {
    unsigned long long sum = 0; unsigned int mx = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) { const uint32_t v = len[i]; sum += v; mx = max(mx, v); }
    sum = cdm_block_sum<unsigned long long>(sum);
    __shared__ unsigned int sMax;
    if (threadIdx.x == 0) sMax = 0;
    __syncthreads();
    atomicMax(&sMax, mx);
    __syncthreads();
    if (threadIdx.x == 0) { atomicAdd(&out[0], sum); atomicMax(&out[1], (unsigned long long) sMax); }
}
template <typename W>
__global__ void k_len_words(const uint32_t *__restrict__ len, uint64_t n, W *__restrict__ w) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) w[i] = i < n ? (len[i] + 15) / 16 : 0;
}
__global__ void k_woff32(const uint64_t *__restrict__ w64, uint64_t n, uint32_t *__restrict__ woff) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) woff[i] = (uint32_t) w64[i];
}
// (the scan's element type spelt out per width: tests/test_primitives_host.py reads the instantiations off the source)
int scanWords(hipStream_t s, cdmscan::ScanTemp &st, const uint32_t *in, uint32_t *out, size_t n) { return cdmscan::exclusiveScan<uint32_t>(s, st, in, out, n); }
int scanWords(hipStream_t s, cdmscan::ScanTemp &st, const uint64_t *in, uint64_t *out, size_t n) { return cdmscan::exclusiveScan<uint64_t>(s, st, in, out, n); }
template <typename W>
int seqdbLayoutT(cdm_ctx *ctx, const uint32_t *len, uint64_t n, uint32_t *woff, uint64_t *words, const char *who) {
    hipStream_t s = ctx->stream;
    constexpr bool wide = sizeof(W) == 8;
    DevBuf<W> w, wo;            // (32 bits: the words per sequence are written to woff and scanned in place)
    if (wide && (!w.alloc(n + 1) || !wo.alloc(n + 1))) { cdm_set_error("%s: out of device memory", who); return CDM_ERR_HIP; }
    W *const in = wide ? w.p : reinterpret_cast<W *>(woff), *const o = wide ? wo.p : reinterpret_cast<W *>(woff);
    hipLaunchKernelGGL(k_len_words<W>, CDM_GRID((n + 256) / 256, 256), dim3(256), 0, s, len, n, in);
    cdmscan::ScanTemp st;
    if (int rc = scanWords(s, st, in, o, (size_t) n + 1)) return rc;
    if (wide) hipLaunchKernelGGL(k_woff32, CDM_GRID((n + 256) / 256, 256), dim3(256), 0, s, reinterpret_cast<const uint64_t *>(o), n, woff);
    W total = 0;
    hipMemcpyAsync(&total, o + n, sizeof(W), hipMemcpyDeviceToHost, s);
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) { cdm_set_error("%s: %s", who, hipGetErrorString(e)); return CDM_ERR_HIP; }
    if (wide && total >= 0xFFFFFF00ull) { cdm_set_error("more than 2^32 code words (68 G bases) in one DB"); return CDM_ERR_UNSUPPORTED; }
    *words = total;
    return CDM_OK;
}
}  // namespace
int seqdbLayout(cdm_ctx *ctx, const uint32_t *len, uint64_t n, uint32_t *woff, uint64_t *words, bool wide, const char *who) {
    return wide ? seqdbLayoutT<uint64_t>(ctx, len, n, woff, words, who) : seqdbLayoutT<uint32_t>(ctx, len, n, woff, words, who);
}
int seqdbLenStats(cdm_ctx *ctx, cdm_seqdb *db) {
    hipStream_t s = ctx->stream;
    DevBuf<unsigned long long> d; unsigned long long h[2] = {0, 0};
    if (!d.alloc(2)) { cdm_set_error("out of device memory"); return CDM_ERR_HIP; }
    CDM_HIP(hipMemsetAsync(d.p, 0, 16, s));
    if (db->n) hipLaunchKernelGGL(k_len_stats, dim3((unsigned) std::min<uint64_t>((db->n + 255) / 256, 4096)), dim3(256), 0, s, (const uint32_t *) db->len, (uint64_t) db->n, d.p);
    CDM_HIP(hipMemcpyAsync(h, d.p, 16, hipMemcpyDeviceToHost, s));
    CDM_HIP(hipStreamSynchronize(s));
    db->residues = h[0]; db->maxLen = (uint32_t) h[1];
    return CDM_OK;
}

// ------------------------------------------------------------------------------------------------ text <-> planes
// one thread per (sequence, word): 16 ASCII letters -> one code word + 16 N bits
__global__ void k_pack(const char *__restrict__ data, const uint64_t *__restrict__ off, const uint32_t *__restrict__ len,
                       const uint32_t *__restrict__ woff, uint64_t n, uint64_t words, uint32_t *__restrict__ codes,
                       uint32_t *__restrict__ nmask, uint8_t *__restrict__ hasN, unsigned long long *__restrict__ counters) {
    uint64_t gw = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (gw >= words) return;
    const uint64_t i = seqOfWord(woff, n, gw);
    const uint32_t w = (uint32_t) (gw - woff[i]);
    const uint32_t L = len[i];
    const char *s = data + off[i] + (uint64_t) w * 16;
    const uint32_t cnt = min(16u, L - min(L, w * 16u));
    uint32_t code = 0, nb = 0, other = 0;
    for (uint32_t j = 0; j < cnt; j++) {
        const char c = s[j];
        uint32_t v = 0;
        switch (c) {
            case 'A': v = 0; break; case 'C': v = 1; break; case 'G': v = 2; break; case 'T': v = 3; break;
            case 'N': nb |= 1u << j; break;
            default:            // NucleotideMatrix::setupLetterMapping (M/commons/NucleotideMatrix.cpp:17-61): toupper, IUPAC codes to one base, the rest to X
                other++;
                switch (c & ~0x20) {    // (the letters below have no non-letter twin under the case bit)
                    case 'A': v = 0; break; case 'C': case 'M': case 'Y': case 'H': v = 1; break;
                    case 'G': case 'K': case 'B': case 'D': case 'V': case 'R': case 'S': v = 2; break;
                    case 'T': case 'U': case 'W': v = 3; break;
                    default: nb |= 1u << j; break;
                }
                if (!((c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'))) { v = 0; nb |= 1u << j; }
                break;
        }
        code |= v << (2 * j);
    }
    codes[gw] = code;
    // two sequence words share one mask word; sequences start on code-word (16 bit) boundaries of the mask
    uint16_t *m16 = reinterpret_cast<uint16_t *>(nmask);
    m16[gw] = (uint16_t) nb;
    if (nb) atomicAdd(&counters[0], (unsigned long long) __popc(nb));
    if (nb || other) atomicOr(reinterpret_cast<unsigned int *>(hasN + (i & ~3ull)), (1u | (other ? 2u : 0u)) << (8 * (i & 3u)));
    if (other) atomicAdd(&counters[1], (unsigned long long) other);
}
// the original bytes of the sequences that carry letters beyond ACGTN, one thread per (sequence, word)
__global__ void k_pack_raw(const char *__restrict__ data, const uint64_t *__restrict__ off, const uint32_t *__restrict__ len,
                           const uint32_t *__restrict__ woff, uint64_t n, uint64_t words, const uint8_t *__restrict__ hasN, uint8_t *__restrict__ raw) {
    uint64_t gw = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (gw >= words) return;
    const uint64_t i = seqOfWord(woff, n, gw);
    if (!(hasN[i] & 2u)) return;
    const uint32_t w = (uint32_t) (gw - woff[i]);
    const uint32_t L = len[i];
    const char *s = data + off[i] + (uint64_t) w * 16;
    const uint32_t cnt = min(16u, L - min(L, w * 16u));
    for (uint32_t j = 0; j < cnt; j++) raw[gw * 16 + j] = (uint8_t) s[j];
}
// Packs text that is on the device (entry i = dText[dOff[i] .. dOff[i] + len[i])) into db, whose per-sequence arrays and codes / nmask
// planes stand: clears and sets the letter flags, counts the N, and gives the sequences with other letters their rows of a raw plane.
// Returns with the stream idle (the caller may free the text).
static int seqdbPackText(cdm_ctx *ctx, cdm_seqdb *db, const char *dText, const uint64_t *dOff, const char *failed) {
    hipStream_t s = ctx->stream;
    const uint64_t n = db->n, words = db->words;
    DevBuf<unsigned long long> dCnt;
    if (!dCnt.alloc(2)) { cdm_set_error("out of device memory packing %llu sequences", (unsigned long long) n); return CDM_ERR_HIP; }
    hipMemsetAsync(dCnt.p, 0, 16, s);
    hipMemsetAsync(db->hasN, 0, n, s);
    if (words) hipLaunchKernelGGL(k_pack, CDM_GRID((words + 255) / 256, 256), dim3(256), 0, s, dText, dOff, db->len, db->woff, n, words, db->codes, db->nmask, db->hasN, dCnt.p);
    unsigned long long cnt[2] = {0, 0};
    hipMemcpyAsync(cnt, dCnt.p, 16, hipMemcpyDeviceToHost, s);
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) { cdm_set_error("%s: %s", failed, hipGetErrorString(e)); return CDM_ERR_HIP; }
    db->nCount = cnt[0];
    if (cnt[1]) {       // lower case / IUPAC codes / other bytes: those sequences keep their original letters beside the mapped codes
        if (int rc = cdm_seqdb_alloc_raw(db)) return rc;
        hipLaunchKernelGGL(k_pack_raw, CDM_GRID((words + 255) / 256, 256), dim3(256), 0, s, dText, dOff, db->len, db->woff, n, words, db->hasN, db->raw);
        e = hipStreamSynchronize(s);
        if (e != hipSuccess) { cdm_set_error("%s: %s", failed, hipGetErrorString(e)); return CDM_ERR_HIP; }
    }
    return CDM_OK;
}

extern "C" int cdm_seqdb_upload(cdm_ctx *ctx, const char *data, const uint64_t *offsets, const uint32_t *lengths, const uint32_t *keys,
                                const uint8_t *ext, uint64_t n, cdm_seqdb **out) {
    if (!ctx || !data || !offsets || !lengths || !keys || !out) { cdm_set_error("cdm_seqdb_upload: NULL argument"); return CDM_ERR_INVALID; }
    if (n == 0) { cdm_set_error("cdm_seqdb_upload: empty sequence DB"); return CDM_ERR_INVALID; }
    if (n >= 0xFFFFFFFFull) { cdm_set_error("cdm_seqdb_upload: more than 2^32-1 sequences"); return CDM_ERR_UNSUPPORTED; }
    CDM_HIP(hipSetDevice(ctx->device));
    std::vector<uint32_t> woff(n + 1);
    uint64_t words = 0, residues = 0, lo = UINT64_MAX, hi = 0; uint32_t maxLen = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (i && keys[i] <= keys[i - 1]) { cdm_set_error("cdm_seqdb_upload: keys must be strictly increasing (entry %llu)", (unsigned long long) i); return CDM_ERR_INVALID; }
        woff[i] = (uint32_t) words;
        words += (lengths[i] + 15) / 16;
        residues += lengths[i];
        maxLen = std::max(maxLen, lengths[i]);
        lo = std::min(lo, offsets[i]); hi = std::max(hi, offsets[i] + lengths[i]);
        if (words >= 0xFFFFFF00ull) { cdm_set_error("cdm_seqdb_upload: more than 2^32 code words (68 G bases) in one DB"); return CDM_ERR_UNSUPPORTED; }
    }
    woff[n] = (uint32_t) words;
    cdm_seqdb *db = nullptr;
    int rc = cdm_seqdb_alloc(ctx, n, &db);
    if (rc) return rc;
    db->residues = residues; db->maxLen = maxLen;
    if ((rc = seqdbAllocPlanes(db, words, false)) != CDM_OK) { cdm_seqdb_free(db); return rc; }
    hipStream_t s = ctx->stream;
    std::vector<uint64_t> rel(n);
    for (uint64_t i = 0; i < n; i++) rel[i] = offsets[i] - lo;
    DevBuf<char> dData; DevBuf<uint64_t> dOff;
    if (!dData.alloc(hi - lo + 16) || !dOff.alloc(n)) {
        cdm_seqdb_free(db); cdm_set_error("out of device memory staging %llu bytes of sequence text", (unsigned long long) (hi - lo)); return CDM_ERR_HIP;
    }
    hipMemcpyAsync(dData.p, data + lo, hi - lo, hipMemcpyHostToDevice, s);
    hipMemcpyAsync(dOff.p, rel.data(), n * 8, hipMemcpyHostToDevice, s);
    hipMemcpyAsync(db->woff, woff.data(), (n + 1) * 4, hipMemcpyHostToDevice, s);
    hipMemcpyAsync(db->len, lengths, n * 4, hipMemcpyHostToDevice, s);
    hipMemcpyAsync(db->key, keys, n * 4, hipMemcpyHostToDevice, s);
    if (ext) hipMemcpyAsync(db->ext, ext, n, hipMemcpyHostToDevice, s); else hipMemsetAsync(db->ext, 0, n, s);
    if ((rc = seqdbPackText(ctx, db, dData.p, dOff.p, "sequence upload/packing failed")) != CDM_OK) { cdm_seqdb_free(db); return rc; }
    *out = db;
    return CDM_OK;
}

// ---- a sequence DB from text that is on the device already (cdm_pairs_to_seqdb: the merged pairs become the DB the reads loop runs on
// without a host round trip).  Entry j: text[off[j] .. off[j] + len[j]) = its letters, key first_key + j, wasExtended ext; packed as
// cdm_seqdb_upload packs.
namespace {
__global__ void k_text_meta(const uint32_t *__restrict__ entLen, uint64_t n, uint32_t firstKey, uint8_t extValue, uint32_t *__restrict__ len, uint32_t *__restrict__ key, uint8_t *__restrict__ ext) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { len[i] = entLen[i]; key[i] = firstKey + (uint32_t) i; ext[i] = extValue; }
}
}  // namespace
int cdm_seqdb_from_device_text(cdm_ctx *ctx, const char *text, const uint64_t *off, const uint32_t *len, uint64_t n, uint32_t firstKey, uint8_t ext, cdm_seqdb **out) {
    if (n == 0 || n >= 0xFFFFFFFFull) { cdm_set_error("a sequence DB of %llu entries", (unsigned long long) n); return CDM_ERR_UNSUPPORTED; }
    CDM_HIP(hipSetDevice(ctx->device));
    cdm_seqdb *db = nullptr;
    int rc = cdm_seqdb_alloc(ctx, n, &db);
    if (rc) return rc;
    hipLaunchKernelGGL(k_text_meta, CDM_GRID((n + 255) / 256, 256), dim3(256), 0, ctx->stream, len, n, firstKey, ext, db->len, db->key, db->ext);
    uint64_t words = 0;
    rc = seqdbLayout(ctx, db->len, n, db->woff, &words, true, "sequence DB from device text");
    if (rc == CDM_OK) rc = seqdbAllocPlanes(db, words, false);
    if (rc == CDM_OK) rc = seqdbPackText(ctx, db, text, off, "sequence DB from device text");
    if (rc == CDM_OK) rc = seqdbLenStats(ctx, db);
    if (rc != CDM_OK) { cdm_seqdb_free(db); return rc; }
    *out = db;
    return CDM_OK;
}

// one thread per (sequence, word): 16 letters + the trailing '\n' after the last base
__global__ void k_unpack(const uint32_t *__restrict__ codes, const uint32_t *__restrict__ nmask, const uint32_t *__restrict__ woff,
                         const uint32_t *__restrict__ len, const uint64_t *__restrict__ outOff, uint64_t n, uint64_t words, char *__restrict__ out,
                         const uint8_t *__restrict__ hasN, const uint8_t *__restrict__ raw) {
    uint64_t gw = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (gw >= words) return;
    const uint64_t i = seqOfWord(woff, n, gw);
    const uint32_t w = (uint32_t) (gw - woff[i]);
    const uint32_t L = len[i];
    const uint32_t cnt = min(16u, L - min(L, w * 16u));
    const uint32_t code = codes[gw];
    const uint32_t nb = reinterpret_cast<const uint16_t *>(nmask)[gw];
    char *o = out + outOff[i] + (uint64_t) w * 16;
    if (raw && (hasN[i] & 2u)) for (uint32_t j = 0; j < cnt; j++) o[j] = (char) raw[gw * 16 + j];
    else for (uint32_t j = 0; j < cnt; j++) o[j] = ((nb >> j) & 1u) ? 'N' : "ACGT"[(code >> (2 * j)) & 3u];
    if (w * 16u + cnt == L) o[cnt] = '\n';
}
// The DB as text on the device, enqueued on the stream: sequence i as "SEQ\n" at text[outOffsets[i]], NUL between the entries.  len: the
// lengths, on the host; total: bytes of the text.  Zero-length sequences own no word: their '\n' is left to the caller, on the host.
struct SeqdbText { std::vector<uint32_t> len; uint64_t total = 0; DevBuf<char> text; DevBuf<uint64_t> off; };
static int seqdbUnpackText(cdm_ctx *ctx, const cdm_seqdb *db, const uint64_t *outOffsets, SeqdbText &t, const char *who) {
    t.len.resize(db->n);
    CDM_HIP(hipMemcpy(t.len.data(), db->len, db->n * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < db->n; i++) t.total = std::max(t.total, outOffsets[i] + t.len[i] + 1);
    if (!t.text.alloc(t.total + 16) || !t.off.alloc(db->n)) { cdm_set_error("out of device memory in %s", who); return CDM_ERR_HIP; }
    hipMemsetAsync(t.text.p, 0, t.total, ctx->stream);
    hipMemcpyAsync(t.off.p, outOffsets, db->n * 8, hipMemcpyHostToDevice, ctx->stream);
    if (db->words) hipLaunchKernelGGL(k_unpack, CDM_GRID((db->words + 255) / 256, 256), dim3(256), 0, ctx->stream, db->codes, db->nmask, db->woff, db->len, t.off.p, db->n, db->words, t.text.p, db->hasN, db->raw);
    return CDM_OK;
}
extern "C" int cdm_seqdb_download(cdm_ctx *ctx, const cdm_seqdb *db, char *out, const uint64_t *outOffsets) {
    CDM_HIP(hipSetDevice(ctx->device));
    SeqdbText t;
    if (int rc = seqdbUnpackText(ctx, db, outOffsets, t, "cdm_seqdb_download")) return rc;
    hipMemcpyAsync(out, t.text.p, t.total, hipMemcpyDeviceToHost, ctx->stream);
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { cdm_set_error("cdm_seqdb_download failed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; }
    for (uint64_t i = 0; i < db->n; i++) if (t.len[i] == 0) out[outOffsets[i]] = '\n';
    return CDM_OK;
}
// The same blob in PIECES, for a caller that writes it out as it comes (round 5: a module process's sequence DB - the copy from the
// device lands in pinned staging buffers of the library at the link's speed, and the caller's sink - a pwrite into the DB's data file -
// runs on piece i while piece i + 1 is on its way; before, the whole text came down into pageable memory at 8 GB/s and was then written
// out at the file system's 4 GB/s, one after the other).  sink(user, data, offset, bytes): consecutive pieces, data valid during the
// call; a non-zero return ends the download with CDM_ERR_INVALID.
extern "C" int cdm_seqdb_download_stream(cdm_ctx *ctx, const cdm_seqdb *db, const uint64_t *outOffsets, uint64_t pieceBytes,
                                         int (*sink)(void *user, const char *data, uint64_t offset, uint64_t bytes), void *user) {
    if (!ctx || !db || !sink || (db->n && !outOffsets)) { cdm_set_error("cdm_seqdb_download_stream: invalid argument"); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    if (db->n == 0) return CDM_OK;
    if (pieceBytes < (1u << 20)) pieceBytes = 64u << 20;
    // (the entries must ascend for the zero-length fix-up below to find them piece by piece; every caller's do)
    for (uint64_t i = 1; i < db->n; i++) if (outOffsets[i] < outOffsets[i - 1]) { cdm_set_error("cdm_seqdb_download_stream: the offsets must ascend"); return CDM_ERR_INVALID; }
    SeqdbText t;
    if (int rc = seqdbUnpackText(ctx, db, outOffsets, t, "cdm_seqdb_download_stream")) return rc;
    const std::vector<uint32_t> &len = t.len; const uint64_t total = t.total; DevBuf<char> &dOut = t.text;
    hipStream_t s = ctx->stream;
    char *pin[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr};
    auto cleanup = [&] { for (int b = 0; b < 2; b++) { if (pin[b]) (void) hipHostFree(pin[b]); if (ev[b]) (void) hipEventDestroy(ev[b]); } };
    pieceBytes = std::min(pieceBytes, total);
    for (int b = 0; b < 2; b++) if (hipHostMalloc((void **) &pin[b], pieceBytes, hipHostMallocDefault) != hipSuccess || hipEventCreateWithFlags(&ev[b], hipEventDisableTiming) != hipSuccess) {
        (void) hipGetLastError(); (void) hipStreamSynchronize(s); cleanup(); cdm_set_error("cdm_seqdb_download_stream: no pinned staging buffer of %llu bytes", (unsigned long long) pieceBytes); return CDM_ERR_HIP;
    }
    const uint64_t pieces = (total + pieceBytes - 1) / pieceBytes;
    auto issue = [&](uint64_t i) { const uint64_t at = i * pieceBytes, nb = std::min(pieceBytes, total - at); hipMemcpyAsync(pin[i & 1], dOut.p + at, nb, hipMemcpyDeviceToHost, s); hipEventRecord(ev[i & 1], s); };
    issue(0);
    uint64_t z = 0;             // next sequence to look at for the zero-length fix-up ('\n' of an empty sequence: it owns no code word)
    int rc = CDM_OK;
    for (uint64_t i = 0; i < pieces && rc == CDM_OK; i++) {
        if (i + 1 < pieces) issue(i + 1);
        if (hipEventSynchronize(ev[i & 1]) != hipSuccess) { cdm_set_error("cdm_seqdb_download_stream failed: %s", hipGetErrorString(hipGetLastError())); rc = CDM_ERR_HIP; break; }
        const uint64_t at = i * pieceBytes, nb = std::min(pieceBytes, total - at);
        while (z < db->n && outOffsets[z] < at + nb) { if (len[z] == 0 && outOffsets[z] >= at) pin[i & 1][outOffsets[z] - at] = '\n'; z++; }
        if (sink(user, pin[i & 1], at, nb) != 0) { cdm_set_error("cdm_seqdb_download_stream: the sink refused a piece at offset %llu", (unsigned long long) at); rc = CDM_ERR_INVALID; }
    }
    (void) hipStreamSynchronize(s);
    cleanup();
    return rc;
}
extern "C" int cdm_seqdb_synth(cdm_ctx *ctx, uint64_t nTotal, uint64_t first, uint64_t n, uint32_t lo, uint32_t hi, uint64_t seed, cdm_seqdb **out) {
    return cdm_synth_impl(ctx, nTotal, first, n, lo, hi, seed, out);
}

// ------------------------------------------------------------------------------------------------ one DB from another: the gather
// Candidate c (of nc) is ONE source sequence: B's entry idxB[c] where idxB is given and idxB[c] is not 0xFFFFFFFF, else A's entry c.  It
// is dropped (take[c] = 0xFFFFFFFF) or gives output entry slot[c] (slot NULL: c) its first take[c] letters (take NULL: all of them); the
// key is A's entry c's either way.  cdm_seqdb_select (a sub-DB of prefixes: A = the DB, slot = the rank among the kept) and
// cdm_seqdb_overlay (A = base, B = the grown sequences) are this.
namespace {
struct GatherArgs {
    cdm_seqdb a, b, dst;
    const uint32_t *idxB, *take, *slot;
    const uint8_t *extOf;       // wasExtended by candidate, or NULL: extValue, and the source's own flag where that is negative
    int extValue;
    bool rebuildFlags;          // letter flags: false = the source's byte; true = 3 with a raw row, else 0, then bit 0 from the mask words written
    uint32_t *len, *woff;       // scratch by candidate, [nc + 1] each (the caller's): letters kept, first code word in dst
    uint32_t nc;
};
struct GatherSrc { const cdm_seqdb *db; uint32_t k; };
__device__ __forceinline__ GatherSrc gatherSrc(const GatherArgs &g, uint32_t c) {
    const uint32_t kb = g.idxB ? g.idxB[c] : 0xFFFFFFFFu;
    return kb == 0xFFFFFFFFu ? GatherSrc{&g.a, c} : GatherSrc{&g.b, kb};
}
__global__ void k_gather_len(const GatherArgs g) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= g.nc) return;
    const GatherSrc s = gatherSrc(g, c);
    g.len[c] = !g.take ? s.db->len[s.k] : g.take[c] == 0xFFFFFFFFu ? 0 : g.take[c];
}
__global__ void k_gather_meta(const GatherArgs g) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == g.nc) g.dst.woff[g.dst.n] = g.woff[c];
    if (c >= g.nc || (g.take && g.take[c] == 0xFFFFFFFFu)) return;
    const GatherSrc s = gatherSrc(g, c);
    const uint32_t r = g.slot ? g.slot[c] : c;
    const uint8_t f = s.db->hasN[s.k];
    g.dst.len[r] = g.len[c]; g.dst.woff[r] = g.woff[c]; g.dst.key[r] = g.a.key[c];
    g.dst.ext[r] = g.extOf ? g.extOf[c] : g.extValue < 0 ? s.db->ext[s.k] : (uint8_t) g.extValue;
    g.dst.hasN[r] = !g.rebuildFlags ? f : (f & 2u) ? 3 : 0;
}
// one wave per candidate (of this launch's slice, from `first` on): codes, the 16-bit mask halves and, where the source sequence has
// one, its raw row.  A kept prefix ends inside its last word: the letters behind it are cleared - which changes nothing in a whole
// sequence, whose packed words are zero beyond its length already.
__global__ void k_gather_copy(const GatherArgs g, uint32_t first) {
    const uint32_t c = first + (uint32_t) (((uint64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (c >= g.nc || (g.take && g.take[c] == 0xFFFFFFFFu)) return;
    const GatherSrc s = gatherSrc(g, c);
    const cdm_seqdb &from = *s.db;
    const uint32_t L = g.len[c], w = (L + 15) / 16, s0 = from.woff[s.k], d0 = g.woff[c], tail = L & 15u;
    for (uint32_t j = lane; j < w; j += 64) {
        uint32_t x = from.codes[s0 + j], m = reinterpret_cast<const uint16_t *>(from.nmask)[s0 + j];
        if (j == w - 1 && tail) { x &= (1u << (2 * tail)) - 1u; m &= (1u << tail) - 1u; }
        g.dst.codes[d0 + j] = x;
        reinterpret_cast<uint16_t *>(g.dst.nmask)[d0 + j] = (uint16_t) m;
    }
    if (from.hasN[s.k] & 2u) for (uint32_t j = lane; j < L; j += 64) g.dst.raw[(uint64_t) d0 * 16 + j] = from.raw[(uint64_t) s0 * 16 + j];
}
__global__ void k_mark_hasN(const uint32_t *__restrict__ woff, const uint32_t *__restrict__ nmask, uint32_t n, uint64_t words, uint8_t *__restrict__ hasN) {
    const uint64_t gw = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (gw >= words || reinterpret_cast<const uint16_t *>(nmask)[gw] == 0) return;
    const uint64_t i = seqOfWord(woff, n, gw);
    if (!hasN[i]) hasN[i] = 1;      // (a sequence that brought its raw row along keeps its 3)
}
// The DB that g describes (g.dst is set here); dKept: where on the device the number of output entries stands, or NULL: all nc candidates.
// Returns with the result complete: residues and maxLen set, the stream idle.
int seqdbGather(cdm_ctx *ctx, GatherArgs g, const uint32_t *dKept, bool withRaw, const char *who, cdm_seqdb **out) {
    hipStream_t s = ctx->stream;
    const uint32_t nc = g.nc;
    uint32_t m = nc; uint64_t words = 0;
    if (nc) hipLaunchKernelGGL(k_gather_len, dim3((nc + 255) / 256), dim3(256), 0, s, g);
    if (dKept) hipMemcpyAsync(&m, dKept, 4, hipMemcpyDeviceToHost, s);
    if (int rc = seqdbLayout(ctx, g.len, nc, g.woff, &words, false, who)) return rc;
    cdm_seqdb *o = nullptr;
    int rc = cdm_seqdb_alloc(ctx, m, &o);
    if (rc == CDM_OK) rc = seqdbAllocPlanes(o, words, withRaw);
    if (rc != CDM_OK) { if (o) cdm_seqdb_free(o); return rc; }
    g.dst = *o;
    hipMemsetAsync(o->nmask, 0, seqdbMaskBytes(words), s);
    hipLaunchKernelGGL(k_gather_meta, dim3((nc + 256) / 256), dim3(256), 0, s, g);
    for (uint64_t first = 0, slice = cdmSliceItems(64); first < nc; first += slice)
        hipLaunchKernelGGL(k_gather_copy, CDM_GRID((std::min<uint64_t>(slice, nc - first) * 64 + 255) / 256, 256), dim3(256), 0, s, g, (uint32_t) first);
    if (g.rebuildFlags && words && m) hipLaunchKernelGGL(k_mark_hasN, CDM_GRID((words + 255) / 256, 256), dim3(256), 0, s, o->woff, o->nmask, m, words, o->hasN);
    if (int rc2 = seqdbLenStats(ctx, o)) { cdm_seqdb_free(o); cdm_set_error("%s: %s", who, hipGetErrorString(hipGetLastError())); return rc2; }
    *out = o;
    return CDM_OK;
}

__global__ void k_sel_from_ext(const uint32_t *__restrict__ len, const uint8_t *__restrict__ ext, uint32_t n, uint32_t *__restrict__ sel) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sel[i] = ext[i] == 1 ? len[i] : 0xFFFFFFFFu;
}
__global__ void k_sel_kept(const uint32_t *__restrict__ sel, uint32_t n, uint32_t *__restrict__ kept) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) kept[i] = i < n && sel[i] != 0xFFFFFFFFu ? 1 : 0;
}
__global__ void k_ov_source(const uint32_t *__restrict__ idx, uint32_t m, uint32_t *__restrict__ src) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) src[idx[j]] = j;
}
}  // namespace
// Sub-DB: sel[i] = 0xFFFFFFFF drops sequence i, any other value keeps its first sel[i] letters (<= len[i]); extValue < 0 keeps the
// wasExtended flags.  The order of the kept sequences is kept.  (nCount stays 0: common.h)
int cdm_seqdb_select(cdm_ctx *ctx, const cdm_seqdb *db, const uint32_t *sel, int extValue, cdm_seqdb **out) {
    CDM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint32_t n = (uint32_t) db->n;
    DevBuf<uint32_t> len, kept, woff, rank;
    if (!len.alloc((size_t) n + 1) || !kept.alloc((size_t) n + 1) || !woff.alloc((size_t) n + 1) || !rank.alloc((size_t) n + 1)) { cdm_set_error("cdm_seqdb_select: out of device memory"); return CDM_ERR_HIP; }
    hipLaunchKernelGGL(k_sel_kept, dim3((n + 256) / 256), dim3(256), 0, s, sel, n, kept.p);
    cdmscan::ScanTemp st;
    if (cdmscan::exclusiveScan<uint32_t>(s, st, kept.p, rank.p, (size_t) n + 1) != CDM_OK) return CDM_ERR_HIP;
    GatherArgs g{};
    g.a = g.b = *db; g.take = sel; g.slot = rank.p; g.extValue = extValue; g.rebuildFlags = true; g.len = len.p; g.woff = woff.p; g.nc = n;
    return seqdbGather(ctx, g, rank.p + n, db->raw != nullptr, "cdm_seqdb_select", out);
}
extern "C" int cdm_seqdb_select_ext(cdm_ctx *ctx, const cdm_seqdb *db, cdm_seqdb **out) {
    CDM_HIP(hipSetDevice(ctx->device));
    const uint32_t n = (uint32_t) db->n;
    DevBuf<uint32_t> sel;
    if (!sel.alloc((size_t) n + 1)) { cdm_set_error("cdm_seqdb_select_ext: out of device memory"); return CDM_ERR_HIP; }
    if (n) hipLaunchKernelGGL(k_sel_from_ext, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, db->len, db->ext, n, sel.p);
    return cdm_seqdb_select(ctx, db, sel.p, 1, out);
}
// ---- overlay: base with some of its sequences replaced (ancient_contig_merge: the grown contigs come up from the host, the others
// never leave the device).  out[i] = grown[j] where idx[j] == i, else base[i]; keys are base's, ext comes from the caller; the letter
// flags are the source sequence's own.
int cdm_seqdb_overlay(cdm_ctx *ctx, const cdm_seqdb *base, const cdm_seqdb *grown, const uint32_t *idxHost, const uint8_t *extHost, cdm_seqdb **out) {
    CDM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint32_t n = (uint32_t) base->n, m = grown ? (uint32_t) grown->n : 0u;
    DevBuf<uint32_t> src, idx, len, woff; DevBuf<uint8_t> ext;
    if (!src.alloc(n) || !idx.alloc(m) || !len.alloc((size_t) n + 1) || !woff.alloc((size_t) n + 1) || !ext.alloc(n)) { cdm_set_error("cdm_seqdb_overlay: out of device memory"); return CDM_ERR_HIP; }
    CDM_HIP(hipMemsetAsync(src.p, 0xFF, (size_t) n * 4, s));
    if (m) CDM_HIP(hipMemcpyAsync(idx.p, idxHost, (size_t) m * 4, hipMemcpyHostToDevice, s));
    CDM_HIP(hipMemcpyAsync(ext.p, extHost, n, hipMemcpyHostToDevice, s));
    if (m) hipLaunchKernelGGL(k_ov_source, dim3((m + 255) / 256), dim3(256), 0, s, idx.p, m, src.p);
    if ((uint64_t) base->words + (grown ? grown->words : 0) >= 0xFFFFFF00ull) { cdm_set_error("cdm_seqdb_overlay: more than 2^32 code words (68 G bases) in one DB"); return CDM_ERR_UNSUPPORTED; }
    GatherArgs g{};
    g.a = *base; g.b = grown ? *grown : *base; g.idxB = src.p; g.extOf = ext.p; g.len = len.p; g.woff = woff.p; g.nc = n;
    cdm_seqdb *o = nullptr;
    if (int rc = seqdbGather(ctx, g, nullptr, base->raw || (grown && grown->raw), "cdm_seqdb_overlay", &o)) return rc;
    o->nCount = base->nCount + (grown ? grown->nCount : 0);
    *out = o;
    return CDM_OK;
}
// ---- the workflow's two selections of the assembled contigs (data/nuclassemble.sh:214-233) on a resident DB.  The script joins the
// index of the result with the index of the source DB on the key and keeps `$3 > $7`, then `$3 > thr + 1`, where column 3 of an index
// is the entry's length: the sequence plus "\n\0", i.e. len + 2.  The +2 stands on both sides of the first comparison and falls out:
// len(result) > len(source).  In the second, len + 2 > thr + 1 is len > thr - 1, for integers len >= thr.  A result key the source
// does not hold is not printed by the join: dropped.  The kept entries keep their keys, wasExtended flags, N and raw planes.
// The source is read for its keys and lengths alone: cdm_seqdb_index_copy gives a DB of just those (and the flags), so that a caller
// need not keep the letters of the DB it started from resident while that DB grows into the result.
extern "C" int cdm_seqdb_index_copy(cdm_ctx *ctx, const cdm_seqdb *db, cdm_seqdb **out) {
    if (!ctx || !db || !out) { cdm_set_error("cdm_seqdb_index_copy: NULL argument"); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    cdm_seqdb *o = nullptr;
    if (int rc = cdm_seqdb_alloc(ctx, db->n, &o)) return rc;
    hipStream_t s = ctx->stream;
    o->residues = db->residues; o->maxLen = db->maxLen;      // (no letters: words = 0, codes / nmask / raw stay NULL)
    CDM_HIP(hipMemsetAsync(o->woff, 0, (db->n + 1) * 4, s));
    CDM_HIP(hipMemsetAsync(o->hasN, 0, db->n + 8, s));
    if (db->n) {
        CDM_HIP(hipMemcpyAsync(o->len, db->len, db->n * 4, hipMemcpyDeviceToDevice, s));
        CDM_HIP(hipMemcpyAsync(o->key, db->key, db->n * 4, hipMemcpyDeviceToDevice, s));
        CDM_HIP(hipMemcpyAsync(o->ext, db->ext, db->n, hipMemcpyDeviceToDevice, s));
    }
    CDM_HIP(hipStreamSynchronize(s));
    *out = o;
    return CDM_OK;
}
namespace {
__global__ void k_keys_ascend(const uint32_t *__restrict__ key, uint32_t n, unsigned int *__restrict__ bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i + 1 < n && key[i] >= key[i + 1]) atomicOr(bad, 1u);
}
// sel[i] = len[i] if result entry i grew beyond its source entry and is long enough, else 0xFFFFFFFF; the source length by binary search
// on the source's ascending keys
__global__ void k_sel_assembled(const uint32_t *__restrict__ len, const uint32_t *__restrict__ key, uint32_t n, const uint32_t *__restrict__ srcKey,
                                const uint32_t *__restrict__ srcLen, uint32_t m, uint32_t minLen, uint32_t *__restrict__ sel) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = key[i], L = len[i];
    uint32_t lo = 0, hi = m;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (srcKey[mid] < k) lo = mid + 1; else hi = mid; }
    const bool keep = lo < m && srcKey[lo] == k && L > srcLen[lo] && L >= minLen && L != 0xFFFFFFFFu;
    sel[i] = keep ? L : 0xFFFFFFFFu;
}
}  // namespace
extern "C" int cdm_seqdb_select_assembled(cdm_ctx *ctx, const cdm_seqdb *result, const cdm_seqdb *source, uint32_t min_len, cdm_seqdb **out, uint64_t *n_kept) {
    if (!ctx || !result || !source || !out) { cdm_set_error("cdm_seqdb_select_assembled: NULL argument"); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint32_t n = (uint32_t) result->n, m = (uint32_t) source->n;
    DevBuf<uint32_t> sel; DevBuf<unsigned int> bad;
    if (!sel.alloc((size_t) n + 1) || !bad.alloc(1)) { cdm_set_error("cdm_seqdb_select_assembled: out of device memory"); return CDM_ERR_HIP; }
    unsigned int unsorted = 0;
    CDM_HIP(hipMemsetAsync(bad.p, 0, 4, s));
    if (m > 1) hipLaunchKernelGGL(k_keys_ascend, dim3((m + 255) / 256), dim3(256), 0, s, source->key, m, bad.p);
    CDM_HIP(hipMemcpyAsync(&unsorted, bad.p, 4, hipMemcpyDeviceToHost, s));
    CDM_HIP(hipStreamSynchronize(s));
    if (unsorted) { cdm_set_error("cdm_seqdb_select_assembled: the keys of the source DB do not ascend strictly (a sequence DB is ordered by key)"); return CDM_ERR_INVALID; }
    if (n) hipLaunchKernelGGL(k_sel_assembled, dim3((n + 255) / 256), dim3(256), 0, s, (const uint32_t *) result->len, (const uint32_t *) result->key, n, (const uint32_t *) source->key, (const uint32_t *) source->len, m, min_len, sel.p);
    CDM_LAUNCH_CHECK();
    cdm_seqdb *o = nullptr;
    const int rc = cdm_seqdb_select(ctx, result, sel.p, -1, &o);
    if (rc != CDM_OK) return rc;
    *out = o;
    if (n_kept) *n_kept = o->n;
    return CDM_OK;
}

// ---- two resident DBs as one: a's entries, then b's.  Every sequence starts on a code word, and the N bits and the raw plane are
// indexed by code word too (16 bits / 16 bytes per word): the three planes of the result are the parts' planes back to back, and only
// b's word offsets move.  Keys 0 .. n - 1, the flags of the parts set by the caller.
namespace {
__global__ void k_concat_meta(const cdm_seqdb a, const cdm_seqdb b, uint8_t extA, uint8_t extB, cdm_seqdb o) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x, n = a.n + b.n;
    if (i > n) return;
    if (i == n) { o.woff[n] = (uint32_t) (a.words + b.words); return; }
    const bool inA = i < a.n;
    const cdm_seqdb &src = inA ? a : b;
    const uint64_t j = inA ? i : i - a.n;
    o.woff[i] = src.woff[j] + (inA ? 0u : (uint32_t) a.words);
    o.len[i] = src.len[j]; o.key[i] = (uint32_t) i; o.ext[i] = inA ? extA : extB; o.hasN[i] = src.hasN[j];
}
}  // namespace
extern "C" int cdm_seqdb_concat(cdm_ctx *ctx, const cdm_seqdb *a, const cdm_seqdb *b, uint8_t ext_a, uint8_t ext_b, cdm_seqdb **out) {
    if (!ctx || !a || !b || !out) { cdm_set_error("cdm_seqdb_concat: NULL argument"); return CDM_ERR_INVALID; }
    if ((a->residues && !a->codes) || (b->residues && !b->codes)) { cdm_set_error("cdm_seqdb_concat: a part holds no letters (an index copy)"); return CDM_ERR_INVALID; }
    const uint64_t n = a->n + b->n, words = a->words + b->words;
    if (n >= 0xFFFFFFFFull) { cdm_set_error("cdm_seqdb_concat: more than 2^32-1 sequences"); return CDM_ERR_UNSUPPORTED; }
    if (words >= 0xFFFFFF00ull) { cdm_set_error("cdm_seqdb_concat: more than 2^32 code words (68 G bases) in one DB"); return CDM_ERR_UNSUPPORTED; }
    CDM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    cdm_seqdb *o = nullptr;
    int rc = cdm_seqdb_alloc(ctx, n, &o);
    if (rc == CDM_OK) rc = seqdbAllocPlanes(o, words, a->raw || b->raw);
    if (rc != CDM_OK) { if (o) cdm_seqdb_free(o); return rc; }
    o->residues = a->residues + b->residues; o->maxLen = std::max(a->maxLen, b->maxLen); o->nCount = a->nCount + b->nCount;
    hipError_t e = hipMemsetAsync(o->nmask, 0, seqdbMaskBytes(words), s);
    const cdm_seqdb *part[2] = {a, b}; uint64_t at = 0;
    for (int k = 0; k < 2 && e == hipSuccess; k++) {
        const cdm_seqdb *p = part[k];
        if (p->words) {
            e = hipMemcpyAsync(o->codes + at, p->codes, p->words * 4, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipMemcpyAsync(reinterpret_cast<uint16_t *>(o->nmask) + at, p->nmask, p->words * 2, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess && p->raw) e = hipMemcpyAsync(o->raw + at * 16, p->raw, p->words * 16, hipMemcpyDeviceToDevice, s);
        }
        at += p->words;
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_concat_meta, CDM_GRID((n + 256) / 256, 256), dim3(256), 0, s, *a, *b, ext_a, ext_b, *o);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { cdm_seqdb_free(o); cdm_set_error("cdm_seqdb_concat: %s", hipGetErrorString(e)); return CDM_ERR_HIP; }
    *out = o;
    return CDM_OK;
}

// ------------------------------------------------------------------------------------------------ the packed form, to and from device and host memory
namespace {
__global__ void k_raw_flags(const uint8_t *__restrict__ hasN, uint64_t n, uint8_t *__restrict__ flags) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[i] = (hasN[i] & 2u) ? 1 : 0;
}
__global__ void k_raw_attach(const uint8_t *__restrict__ flags, uint8_t bits, uint64_t n, uint8_t *__restrict__ hasN) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (flags[i] & bits)) hasN[i] = 3;
}
// the raw plane (device) beside a DB made from the packed form; the rows that count: those with one of `bits` set in their flags byte
int seqdbAttachRaw(cdm_ctx *ctx, cdm_seqdb *db, const void *raw, const void *flags, uint8_t bits) {
    if (int rc = cdm_seqdb_alloc_raw(db)) return rc;
    hipStream_t s = ctx->stream;
    CDM_HIP(hipMemcpyAsync(db->raw, raw, db->words * 16, hipMemcpyDeviceToDevice, s));
    if (db->n) hipLaunchKernelGGL(k_raw_attach, dim3((unsigned) ((db->n + 255) / 256)), dim3(256), 0, s, (const uint8_t *) flags, bits, db->n, db->hasN);
    CDM_HIP(hipStreamSynchronize(s));
    return CDM_OK;
}
// from the packed planes in device memory; devExt: the wasExtended flags, or NULL: extValue for all.  (nCount stays 0: common.h)
int seqdbFromPacked(cdm_ctx *ctx, const void *codes, const void *nmask16, const void *lengths, const void *keys, const void *devExt, uint8_t extValue, uint64_t n, uint64_t words, cdm_seqdb **out) {
    CDM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    cdm_seqdb *o = nullptr;
    int rc = cdm_seqdb_alloc(ctx, n, &o);
    if (rc == CDM_OK) rc = seqdbAllocPlanes(o, words, false);
    if (rc != CDM_OK) { if (o) cdm_seqdb_free(o); return rc; }
    hipError_t e = hipMemcpyAsync(o->len, lengths, n * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(o->key, keys, n * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(o->codes, codes, words * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(o->nmask, 0, seqdbMaskBytes(words), s);
    if (e == hipSuccess) e = hipMemcpyAsync(o->nmask, nmask16, words * 2, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = devExt && n ? hipMemcpyAsync(o->ext, devExt, n, hipMemcpyDeviceToDevice, s) : hipMemsetAsync(o->ext, extValue, n, s);
    if (e == hipSuccess) e = hipMemsetAsync(o->hasN, 0, n, s);
    if (e != hipSuccess) { cdm_seqdb_free(o); cdm_set_error("cdm_seqdb_from_packed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; }
    uint64_t total = 0;
    if ((rc = seqdbLayout(ctx, o->len, n, o->woff, &total, false, "cdm_seqdb_from_packed")) != CDM_OK) { cdm_seqdb_free(o); return rc; }
    if (total != words) { cdm_seqdb_free(o); cdm_set_error("cdm_seqdb_from_packed: lengths need %u code words, %llu given", (uint32_t) total, (unsigned long long) words); return CDM_ERR_INVALID; }
    if (words && n) hipLaunchKernelGGL(k_mark_hasN, CDM_GRID((words + 255) / 256, 256), dim3(256), 0, s, o->woff, o->nmask, (uint32_t) n, words, o->hasN);
    if ((e = hipGetLastError()) != hipSuccess) { cdm_seqdb_free(o); cdm_set_error("cdm_seqdb_from_packed: %s", hipGetErrorString(e)); return CDM_ERR_HIP; }
    if ((rc = seqdbLenStats(ctx, o)) != CDM_OK) { cdm_seqdb_free(o); return rc; }
    *out = o;
    return CDM_OK;
}
}  // namespace
extern "C" int cdm_seqdb_copy_raw(cdm_ctx *ctx, const cdm_seqdb *db, void *raw, void *flags) {
    if (!db->raw) { cdm_set_error("cdm_seqdb_copy_raw: the DB has no letters beyond ACGTN"); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    CDM_HIP(hipMemcpyAsync(raw, db->raw, db->words * 16, hipMemcpyDeviceToDevice, s));
    if (db->n) hipLaunchKernelGGL(k_raw_flags, dim3((unsigned) ((db->n + 255) / 256)), dim3(256), 0, s, db->hasN, db->n, (uint8_t *) flags);
    CDM_HIP(hipStreamSynchronize(s));
    return CDM_OK;
}
extern "C" int cdm_seqdb_attach_raw(cdm_ctx *ctx, cdm_seqdb *db, const void *raw, const void *flags) {
    CDM_HIP(hipSetDevice(ctx->device));
    return seqdbAttachRaw(ctx, db, raw, flags, 0xFF);
}
extern "C" int cdm_seqdb_from_packed(cdm_ctx *ctx, const void *codes, const void *nmask16, const void *lengths, const void *keys, uint64_t n, uint64_t words,
                                     uint8_t extValue, cdm_seqdb **out) {
    return seqdbFromPacked(ctx, codes, nmask16, lengths, keys, nullptr, extValue, n, words, out);
}
extern "C" int cdm_seqdb_from_packed_ext(cdm_ctx *ctx, const void *codes, const void *nmask16, const void *lengths, const void *keys, const void *devExt, uint64_t n,
                                         uint64_t words, cdm_seqdb **out) {
    return seqdbFromPacked(ctx, codes, nmask16, lengths, keys, devExt, 0, n, words, out);
}

// the planes of db the caller has room for (NULL: not wanted), to device or host memory; rawFlags: the DB's own letter flags
static int seqdbCopyOut(cdm_ctx *ctx, const cdm_seqdb *db, hipMemcpyKind kind, void *codes, void *nmask16, void *lengths, void *keys, void *ext, void *raw, void *rawFlags) {
    CDM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (codes && db->words) CDM_HIP(hipMemcpyAsync(codes, db->codes, db->words * 4, kind, s));
    if (nmask16 && db->words) CDM_HIP(hipMemcpyAsync(nmask16, db->nmask, db->words * 2, kind, s));
    if (lengths && db->n) CDM_HIP(hipMemcpyAsync(lengths, db->len, db->n * 4, kind, s));
    if (keys && db->n) CDM_HIP(hipMemcpyAsync(keys, db->key, db->n * 4, kind, s));
    if (ext && db->n) CDM_HIP(hipMemcpyAsync(ext, db->ext, db->n, kind, s));
    if (raw && db->raw && db->words) CDM_HIP(hipMemcpyAsync(raw, db->raw, db->words * 16, kind, s));
    if (rawFlags && db->n) CDM_HIP(hipMemcpyAsync(rawFlags, db->hasN, db->n, kind, s));
    CDM_HIP(hipStreamSynchronize(s));
    return CDM_OK;
}
extern "C" int cdm_seqdb_copy_packed(cdm_ctx *ctx, const cdm_seqdb *db, void *codes, void *nmask16, void *lengths, void *keys) {
    return seqdbCopyOut(ctx, db, hipMemcpyDeviceToDevice, codes, nmask16, lengths, keys, nullptr, nullptr, nullptr);
}
extern "C" int cdm_seqdb_copy_ext(cdm_ctx *ctx, const cdm_seqdb *db, void *devExt) {
    return seqdbCopyOut(ctx, db, hipMemcpyDeviceToDevice, nullptr, nullptr, nullptr, nullptr, devExt, nullptr, nullptr);
}
// The packed form to and from HOST memory (round 5: the binary side-cars a module process leaves next to the DB it wrote, host/sidecar.cpp -
// the next module of the workflow takes the sequences from there instead of parsing and packing the text again).  nmask16 / raw /
// rawFlags may be NULL on both sides (export: not wanted; import: the DB has no letter beyond ACGT / no raw plane).
extern "C" int cdm_seqdb_export_packed(cdm_ctx *ctx, const cdm_seqdb *db, void *codes, void *nmask16, void *lengths, void *keys, void *ext, void *raw, void *rawFlags) {
    if (!ctx || !db) { cdm_set_error("cdm_seqdb_export_packed: invalid argument"); return CDM_ERR_INVALID; }
    return seqdbCopyOut(ctx, db, hipMemcpyDeviceToHost, codes, nmask16, lengths, keys, ext, raw, rawFlags);
}
extern "C" int cdm_seqdb_import_packed(cdm_ctx *ctx, const void *codes, const void *nmask16, const void *lengths, const void *keys, const void *ext, const void *raw,
                                       const void *rawFlags, uint64_t n, uint64_t words, cdm_seqdb **out) {
    if (!ctx || !out || (n && (!lengths || !keys)) || (words && !codes)) { cdm_set_error("cdm_seqdb_import_packed: invalid argument"); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    DevBuf<uint32_t> dCodes, dLen, dKey; DevBuf<uint16_t> dMask; DevBuf<uint8_t> dExt, dRaw, dFlags;
    if (!dCodes.alloc(words) || !dLen.alloc(n) || !dKey.alloc(n) || !dMask.alloc(words) || !dExt.alloc(n) || (raw && (!dRaw.alloc(words * 16) || !dFlags.alloc(n)))) {
        cdm_set_error("cdm_seqdb_import_packed: out of device memory"); return CDM_ERR_HIP;
    }
    if (words) CDM_HIP(hipMemcpyAsync(dCodes.p, codes, words * 4, hipMemcpyHostToDevice, s));
    if (n) { CDM_HIP(hipMemcpyAsync(dLen.p, lengths, n * 4, hipMemcpyHostToDevice, s)); CDM_HIP(hipMemcpyAsync(dKey.p, keys, n * 4, hipMemcpyHostToDevice, s)); }
    if (words) { if (nmask16) CDM_HIP(hipMemcpyAsync(dMask.p, nmask16, words * 2, hipMemcpyHostToDevice, s)); else CDM_HIP(hipMemsetAsync(dMask.p, 0, words * 2, s)); }
    if (n) { if (ext) CDM_HIP(hipMemcpyAsync(dExt.p, ext, n, hipMemcpyHostToDevice, s)); else CDM_HIP(hipMemsetAsync(dExt.p, 0, n, s)); }
    if (raw) { if (words) CDM_HIP(hipMemcpyAsync(dRaw.p, raw, words * 16, hipMemcpyHostToDevice, s)); if (n) CDM_HIP(hipMemcpyAsync(dFlags.p, rawFlags, n, hipMemcpyHostToDevice, s)); }
    CDM_HIP(hipStreamSynchronize(s));
    cdm_seqdb *o = nullptr;
    if (int rc = seqdbFromPacked(ctx, dCodes.p, dMask.p, dLen.p, dKey.p, dExt.p, 0, n, words, &o)) return rc;
    // (the export's flags are the DB's own letter flags: bit 1 = the row of the raw plane counts)
    if (raw) if (int rc = seqdbAttachRaw(ctx, o, dRaw.p, dFlags.p, 2)) { cdm_seqdb_free(o); return rc; }
    *out = o;
    return CDM_OK;
}
