// C-ABI entry points: errors and switches, the allocator's shims, context, damage / E-value shims, hit and alignment containers, stage wrappers.
// The sequence DB container is seqdb.hip; stage kernels live in correct.hip, rescore.hip, kmermatch.hip (with its kmer_*.h stage headers),
// extend.hip, synth.hip.
#include <cstdarg>
#include <atomic>
#include <cstring>
#include <vector>

#include <algorithm>
#include "seqdb.h"

// ------------------------------------------------------------------------------------------------ errors
static thread_local char g_err[1024] = "";
void cdm_set_error(const char *fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
}
extern "C" const char *cdm_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------------ caching allocator, CDM_* switches
#include "pool.h"
const char *cdmGetenv(const char *name) { return cdmenv::get(name); }
extern "C" void cdm_env_refresh(void) { (void) cdmenv::refresh(); }
extern "C" void cdm_pool_stats(uint64_t out[8]) {
    cdmpool::Stats &st = cdmpool::stats();
    out[0] = st.requests.load(); out[1] = st.cached.load(); out[2] = st.mallocs.load(); out[3] = st.mallocBytes.load(); out[4] = st.mallocNs.load(); out[5] = st.trims.load();
    out[6] = out[7] = 0;
    cdmpool::Registry &r = cdmpool::registry();
    std::lock_guard<std::mutex> g(r.m);
    for (cdmpool::Pool *q : r.pools) {
        std::lock_guard<std::mutex> g2(q->m);
        for (const cdmpool::Arena *a : {&q->small, &q->large}) for (const auto &kv : a->blocks) { if (kv.second.state != cdmpool::B_HOLE) out[6] += kv.second.size; if (kv.second.state == cdmpool::B_USED) out[7] += kv.second.size; }
    }
}
extern "C" void cdm_pool_headroom(float factor) { cdmpool::headroom().store(factor > 1.0f ? std::min(factor, 4.0f) : 1.0f, std::memory_order_relaxed); }
hipError_t cdmMallocRaw(void **p, size_t bytes) { return cdmpool::allocate(p, bytes); }
void cdmFree(void *p) { cdmpool::release(p); }
void cdmPoolTrim() { cdmpool::trimMine(); }
float cdmPoolHeadroomSwap(float f) { return cdmpool::headroom().exchange(f, std::memory_order_relaxed); }

// ------------------------------------------------------------------------------------------------ context
// CDM_SEGV_BACKTRACE=1 (diagnosis, scripts/stress_kpart.py): a SIGSEGV / SIGBUS / SIGABRT of the process prints the faulting thread's
// native stack (backtrace_symbols_fd: async-signal-safe) before the default action takes its course.
#include <execinfo.h>
#include <signal.h>
static void cdmFaultHandler(int sig, siginfo_t *info, void *) {
    static const char head[] = "\n*** libcarpedeam_hip: fatal signal, native stack of the faulting thread:\n";
    (void) !write(2, head, sizeof(head) - 1);
    void *frames[64];
    const int n = backtrace(frames, 64);
    backtrace_symbols_fd(frames, n, 2);
    (void) info;
    signal(sig, SIG_DFL);
    raise(sig);
}
static void cdmInstallFaultHandler() {
    static std::once_flag once;
    std::call_once(once, [] {
        if (!cdmGetenv("CDM_SEGV_BACKTRACE")) return;
        void *warm[4]; (void) backtrace(warm, 4);       // (loads libgcc now, not inside the handler)
        struct sigaction sa; memset(&sa, 0, sizeof(sa));
        sa.sa_sigaction = cdmFaultHandler; sa.sa_flags = SA_SIGINFO | SA_NODEFER | SA_RESETHAND;
        sigaction(SIGSEGV, &sa, nullptr); sigaction(SIGBUS, &sa, nullptr); sigaction(SIGABRT, &sa, nullptr);
    });
}
extern "C" int cdm_ctx_create(int device, cdm_ctx **out) {
    if (!out) { cdm_set_error("cdm_ctx_create: out is NULL"); return CDM_ERR_INVALID; }
    cdmInstallFaultHandler();
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        cdm_set_error("no HIP device available: the carpedeam MI355X path has no CPU fallback");
        return CDM_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= count) { cdm_set_error("device ordinal %d out of range (%d devices)", device, count); return CDM_ERR_NO_DEVICE; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { cdm_set_error("hipGetDeviceProperties failed"); return CDM_ERR_NO_DEVICE; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        cdm_set_error("device %d is %s; this library carries gfx950 (MI355X) code objects only", device, prop.gcnArchName);
        return CDM_ERR_NO_DEVICE;
    }
    if (hipSetDevice(device) != hipSuccess) { cdm_set_error("hipSetDevice(%d) failed", device); return CDM_ERR_NO_DEVICE; }
    cdm_ctx *c = new cdm_ctx();
    c->device = device;
    c->cuCount = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&c->ev0) != hipSuccess ||
        hipEventCreate(&c->ev1) != hipSuccess || hipEventCreate(&c->ev2) != hipSuccess || hipEventCreate(&c->ev3) != hipSuccess ||
        hipEventCreate(&c->evS0) != hipSuccess || hipEventCreate(&c->evS1) != hipSuccess ||
        cdmMalloc(&c->lutDev, sizeof(DamageLut)) != hipSuccess) {
        cdm_set_error("context resource creation failed"); delete c; return CDM_ERR_HIP;
    }
    *out = c;
    return CDM_OK;
}
extern "C" void cdm_ctx_destroy(cdm_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) { hipStreamSynchronize(c->stream); hipStreamDestroy(c->stream); }
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    if (c->ev2) hipEventDestroy(c->ev2);
    if (c->ev3) hipEventDestroy(c->ev3);
    if (c->evS0) hipEventDestroy(c->evS0);
    if (c->evS1) hipEventDestroy(c->evS1);
    if (c->lutDev) cdmFree(c->lutDev);
    cdmPoolTrim();
    delete c;
}
extern "C" int cdm_ctx_sync(cdm_ctx *c) { CDM_HIP(hipSetDevice(c->device)); CDM_HIP(hipStreamSynchronize(c->stream)); return CDM_OK; }
extern "C" void *cdm_ctx_stream(cdm_ctx *c) { return (void *) c->stream; }
extern "C" float cdm_ctx_last_kernel_ms(cdm_ctx *c, int which) { return (which >= 0 && which < 18) ? c->lastMs[which] : -1.f; }

extern "C" int cdm_damage_load(cdm_ctx *c, const char *prefix) {
    std::string err;
    int rc = cdm_build_damage(prefix, c->mats, &c->lutHost, &err);
    if (rc != CDM_OK) { cdm_set_error("%s", err.c_str()); return rc; }
    CDM_HIP(hipSetDevice(c->device));
    CDM_HIP(hipMemcpyAsync(c->lutDev, &c->lutHost, sizeof(DamageLut), hipMemcpyHostToDevice, c->stream));
    CDM_HIP(hipStreamSynchronize(c->stream));
    c->haveDamage = true;
    return CDM_OK;
}
extern "C" int cdm_damage_get(cdm_ctx *c, long double *out) {
    if (!c->haveDamage) { cdm_set_error("cdm_damage_get: no damage model loaded"); return CDM_ERR_INVALID; }
    memcpy(out, c->mats, sizeof(c->mats));
    return CDM_OK;
}
extern "C" double cdm_evalue(double raw, double qLen, uint64_t dbRes) { return cdm_evalue_host(raw, qLen, dbRes); }
extern "C" int cdm_bit_score(double raw) { return cdm_bit_score_host(raw); }
extern "C" int cdm_gapped_evalue(int gapOpen, int gapExtend, double raw, double qLen, uint64_t dbRes, double *evalue, int *bits) {
    if (!cdm_gapped_costs_known(gapOpen, gapExtend)) { cdm_set_error("gapped E-values: only nucleotide.out with --gap-open 5 --gap-extend 2 (the costs ancient_assemble passes)"); return CDM_ERR_UNSUPPORTED; }
    if (evalue) *evalue = cdm_evalue_gapped_host(raw, qLen, dbRes);
    if (bits) *bits = cdm_bit_score_gapped_host(raw);
    return CDM_OK;
}

// ------------------------------------------------------------------------------------------------ hits / alignments
// fn(lo, hi) over [0, n) on a few host threads; with `weight` (n + 1 prefix sums) the ranges carry about the same weight each
#include <thread>
template <typename F>
static void cdmHostParallel(uint64_t n, F fn, const uint64_t *weight = nullptr) {
    unsigned T = std::thread::hardware_concurrency();
    if (const char *e = cdmGetenv("OMP_NUM_THREADS")) { const int v = atoi(e); if (v > 0) T = (unsigned) v; }
    T = std::max(1u, std::min(T, 16u));
    if (n < 100000 || T == 1) { fn(0, n); return; }
    std::vector<uint64_t> cut(T + 1, n);
    cut[0] = 0;
    for (unsigned t = 1; t < T; t++) {
        if (!weight) { cut[t] = n * t / T; continue; }
        const uint64_t want = (weight[n] + n) / T * t;
        uint64_t lo = cut[t - 1], hi = n;
        while (lo < hi) { const uint64_t mid = (lo + hi) / 2; if (weight[mid] + mid < want) lo = mid + 1; else hi = mid; }
        cut[t] = lo;
    }
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; t++) th.emplace_back([&, t] { fn(cut[t], cut[t + 1]); });
    fn(cut[0], cut[1]);
    for (auto &x : th) x.join();
}
template <typename H, typename R>
static int csr_upload(cdm_ctx *ctx, uint64_t n, const uint64_t *offsets, const R *recs, H **out) {
    CDM_HIP(hipSetDevice(ctx->device));
    for (uint64_t i = 0; i < n; i++) if (offsets[i + 1] < offsets[i]) { cdm_set_error("CSR offsets not monotone at %llu", (unsigned long long) i); return CDM_ERR_INVALID; }
    H *h = new H(); h->n = n; h->count = offsets[n];
    if (cdmMalloc(&h->off, (n + 1) * 8) != hipSuccess || cdmMalloc(&h->rec, (h->count + 1) * sizeof(R)) != hipSuccess) {
        cdm_set_error("out of device memory for %llu records", (unsigned long long) h->count); cdmFree(h->off); cdmFree(h->rec); delete h; return CDM_ERR_HIP;
    }
    CDM_HIP(hipMemcpyAsync(h->off, offsets, (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (h->count) CDM_HIP(hipMemcpyAsync(h->rec, recs, h->count * sizeof(R), hipMemcpyHostToDevice, ctx->stream));
    CDM_HIP(hipStreamSynchronize(ctx->stream));
    *out = h;
    return CDM_OK;
}
// The kernels index sequences with the record fields: everything that comes from a file is range-checked on the host first
// (a bad index in a hand-written kernel is a GPU fault, not an error code).
static int fetchLens(cdm_ctx *ctx, const cdm_seqdb *db, std::vector<uint32_t> &lens) {
    lens.resize(db->n);
    CDM_HIP(hipMemcpy(lens.data(), db->len, db->n * 4, hipMemcpyDeviceToHost));
    return CDM_OK;
}
extern "C" int cdm_hits_upload(cdm_ctx *ctx, const cdm_seqdb *db, const uint64_t *offsets, const cdm_hit *hits, cdm_hits **out) {
    static_assert(sizeof(cdm_hit) == sizeof(HitRec), "layout");
    if (!ctx || !db || !offsets || !out || (offsets[db->n] && !hits)) { cdm_set_error("cdm_hits_upload: NULL argument"); return CDM_ERR_INVALID; }
    {   // checked by several threads (a file of 10 M reads brings 37 M records)
        const uint64_t total = offsets[db->n];
        std::atomic<uint64_t> bad{UINT64_MAX};
        cdmHostParallel(total, [&](uint64_t lo, uint64_t hi) {
            for (uint64_t i = lo; i < hi; i++)
                if (hits[i].target >= db->n || hits[i].diagonal < -32768 || hits[i].diagonal > 32767) { uint64_t cur = bad.load(); while (i < cur && !bad.compare_exchange_weak(cur, i)) {} return; }
        });
        const uint64_t i = bad.load();
        if (i != UINT64_MAX) {
            cdm_set_error("cdm_hits_upload: record %llu is out of range (target %u of %llu sequences, diagonal %d)", (unsigned long long) i, hits[i].target,
                          (unsigned long long) db->n, hits[i].diagonal);
            return CDM_ERR_INVALID;
        }
    }
    return csr_upload<cdm_hits, HitRec>(ctx, db->n, offsets, reinterpret_cast<const HitRec *>(hits), out);
}
extern "C" uint64_t cdm_hits_count(const cdm_hits *h) { return h->count; }
extern "C" int cdm_hits_download(cdm_ctx *ctx, const cdm_hits *h, uint64_t *offsets, cdm_hit *hits) {
    CDM_HIP(hipSetDevice(ctx->device));
    if (offsets) CDM_HIP(hipMemcpyAsync(offsets, h->off, (h->n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (hits && h->count) CDM_HIP(hipMemcpyAsync(hits, h->rec, h->count * sizeof(HitRec), hipMemcpyDeviceToHost, ctx->stream));
    CDM_HIP(hipStreamSynchronize(ctx->stream));
    return CDM_OK;
}
extern "C" void cdm_hits_free(cdm_hits *h) { if (!h) return; cdmFree(h->off); cdmFree(h->rec); delete h; }

extern "C" int cdm_alns_upload(cdm_ctx *ctx, const cdm_seqdb *db, const uint64_t *offsets, const cdm_aln *alns, cdm_alns **out) {
    static_assert(sizeof(cdm_aln) == sizeof(AlnRec), "layout");
    if (!ctx || !db || !offsets || !out || (offsets[db->n] && !alns)) { cdm_set_error("cdm_alns_upload: NULL argument"); return CDM_ERR_INVALID; }
    {
        CDM_HIP(hipSetDevice(ctx->device));
        std::vector<uint32_t> lens;
        int rc = fetchLens(ctx, db, lens);
        if (rc) return rc;
        std::atomic<uint64_t> badQ{UINT64_MAX};
        auto okRec = [&](uint64_t q, const cdm_aln &r) {
            return r.target < db->n && r.q_start >= 0 && r.q_end >= 0 && (uint32_t) r.q_start < lens[q] && (uint32_t) r.q_end < lens[q] &&
                   r.db_start >= 0 && r.db_end >= r.db_start && (uint32_t) r.db_end < lens[r.target < db->n ? r.target : 0] &&
                   abs(r.q_end - r.q_start) == r.db_end - r.db_start;   // ungapped: both spans have the same length
        };
        cdmHostParallel(db->n, [&](uint64_t lo, uint64_t hi) {
            for (uint64_t q = lo; q < hi; q++)
                for (uint64_t i = offsets[q]; i < offsets[q + 1] && offsets[q + 1] >= offsets[q]; i++)
                    if (!okRec(q, alns[i])) { uint64_t cur = badQ.load(); while (q < cur && !badQ.compare_exchange_weak(cur, q)) {} return; }
        }, offsets);
        if (badQ.load() != UINT64_MAX) {
            const uint64_t q = badQ.load();
            for (uint64_t i = offsets[q]; i < offsets[q + 1]; i++) {
                const cdm_aln &r = alns[i];
                if (okRec(q, r)) continue;
                cdm_set_error("cdm_alns_upload: alignment record %llu of query %llu does not fit the sequence DB (target %u, q %d-%d of %u, db %d-%d)",
                              (unsigned long long) i, (unsigned long long) q, r.target, r.q_start, r.q_end, lens[q], r.db_start, r.db_end);
                return CDM_ERR_INVALID;
            }
        }
    }
    return csr_upload<cdm_alns, AlnRec>(ctx, db->n, offsets, reinterpret_cast<const AlnRec *>(alns), out);
}
extern "C" uint64_t cdm_alns_count(const cdm_alns *a) { return a->count; }
extern "C" int cdm_alns_download(cdm_ctx *ctx, const cdm_alns *a, uint64_t *offsets, cdm_aln *alns) {
    CDM_HIP(hipSetDevice(ctx->device));
    if (offsets) CDM_HIP(hipMemcpyAsync(offsets, a->off, (a->n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (alns && a->count) CDM_HIP(hipMemcpyAsync(alns, a->rec, a->count * sizeof(AlnRec), hipMemcpyDeviceToHost, ctx->stream));
    CDM_HIP(hipStreamSynchronize(ctx->stream));
    return CDM_OK;
}
extern "C" uint32_t cdm_rescore_tile(void) { return cdm_rescore_tile_impl(); }
extern "C" uint64_t cdm_alns_undefined(const cdm_alns *a) { return a->undefinedRecords; }
extern "C" int cdm_alns_ry_download(cdm_ctx *ctx, const cdm_alns *a, uint16_t *ry) {
    if (!ctx || !a || !ry) { cdm_set_error("cdm_alns_ry_download: NULL argument"); return CDM_ERR_INVALID; }
    if (!a->ryMism) { cdm_set_error("cdm_alns_ry_download: the set carries no purine/pyrimidine counts"); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    if (a->count) CDM_HIP(hipMemcpyAsync(ry, a->ryMism, a->count * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
    CDM_HIP(hipStreamSynchronize(ctx->stream));
    return CDM_OK;
}
extern "C" void cdm_alns_free(cdm_alns *a) { if (!a) return; cdmFree(a->off); cdmFree(a->rec); if (a->ryMism) cdmFree(a->ryMism); delete a; }

// ------------------------------------------------------------------------------------------------ stage wrappers
// device time of the whole stage call (HIP events on the context stream around everything the call launched, host round
// trips between its kernels included): lastMs[8..11] = kmermatcher, rescorediagonal, ancient_correction, ancient_read_assemble
static void stageDone(cdm_ctx *ctx, int slot) {
    hipEventRecord(ctx->evS1, ctx->stream);
    if (hipEventSynchronize(ctx->evS1) == hipSuccess) hipEventElapsedTime(&ctx->lastMs[slot], ctx->evS0, ctx->evS1);
}
extern "C" int cdm_correct(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const cdm_ancient_params *par, cdm_seqdb **out) {
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, "cdm_correct");
    if (!ctx || !db || !alns || !par || !out) { cdm_set_error("cdm_correct: NULL argument"); return CDM_ERR_INVALID; }
    if (!ctx->haveDamage) { cdm_set_error("cdm_correct: call cdm_damage_load first"); return CDM_ERR_INVALID; }
    if (alns->n != db->n) { cdm_set_error("cdm_correct: alignment CSR has %llu queries, DB has %llu", (unsigned long long) alns->n, (unsigned long long) db->n); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    cdm_seqdb *o = nullptr;
    int rc = cdm_seqdb_alloc_like(ctx, db, &o);
    if (rc) return rc;
    hipEventRecord(ctx->evS0, ctx->stream);
    rc = cdm_correct_impl(ctx, db, alns, par, o);
    if (rc) { cdm_seqdb_free(o); return rc; }
    stageDone(ctx, 10);
    *out = o;
    return CDM_OK;
}
extern "C" int cdm_rescore(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_hits *hits, const cdm_rescore_params *par, cdm_alns **out) {
    if (!ctx || !db || !hits || !par || !out) { cdm_set_error("cdm_rescore: NULL argument"); return CDM_ERR_INVALID; }
    if (hits->n != db->n) { cdm_set_error("cdm_rescore: hit CSR / DB size mismatch"); return CDM_ERR_INVALID; }
    if (par->seq_id_mode != 0) { cdm_set_error("cdm_rescore: only --seq-id-mode 0 is implemented"); return CDM_ERR_UNSUPPORTED; }
    CDM_HIP(hipSetDevice(ctx->device));
    hipEventRecord(ctx->evS0, ctx->stream);
    const int rc = cdm_rescore_impl(ctx, db, hits, par, out);
    if (rc == CDM_OK) stageDone(ctx, 9);
    return rc;
}
extern "C" int cdm_rescore_hamming(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_hits *hits, const cdm_hamming_params *par, cdm_hits **out) {
    if (!ctx || !db || !hits || !par || !out) { cdm_set_error("cdm_rescore_hamming: NULL argument"); return CDM_ERR_INVALID; }
    if (hits->n != db->n) { cdm_set_error("cdm_rescore_hamming: hit CSR / DB size mismatch"); return CDM_ERR_INVALID; }
    if (par->seq_id_mode < 0 || par->seq_id_mode > 2) { cdm_set_error("cdm_rescore_hamming: --seq-id-mode is 0, 1 or 2"); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    return cdm_rescore_hamming_impl(ctx, db, hits, par, out);
}
extern "C" int cdm_kmermatch(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_kmer_params *par, cdm_hits **out) {
    if (!ctx || !db || !par || !out) { cdm_set_error("cdm_kmermatch: NULL argument"); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    hipEventRecord(ctx->evS0, ctx->stream);
    const int rc = cdm_kmermatch_impl(ctx, db, par, out);
    if (rc == CDM_OK) stageDone(ctx, 8);
    return rc;
}
extern "C" int cdm_extend(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const cdm_ancient_params *par, cdm_seqdb **out, double *scores) {
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, "cdm_extend");
    if (!ctx || !db || !alns || !par || !out) { cdm_set_error("cdm_extend: NULL argument"); return CDM_ERR_INVALID; }
    if (!ctx->haveDamage) { cdm_set_error("cdm_extend: call cdm_damage_load first"); return CDM_ERR_INVALID; }
    CDM_HIP(hipSetDevice(ctx->device));
    hipEventRecord(ctx->evS0, ctx->stream);
    const int rc = cdm_extend_impl(ctx, db, alns, par, out, scores);
    if (rc == CDM_OK) stageDone(ctx, 11);
    return rc;
}
