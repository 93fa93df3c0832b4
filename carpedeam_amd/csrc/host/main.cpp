// carpedeam_mi355x: the module surface of the reference's hot path on the device (reached through the front end `carpedeam`,
// host/front.c, which also forwards every other command to the reference's binary when a deployment has one).
//
//   carpedeam kmermatcher           <seqDB> <prefDB> [flags]                  lib/mmseqs/src/linclust/kmermatcher.cpp:786
//   carpedeam rescorediagonal       <qDB> <tDB> <prefDB> <alnDB> [flags]      lib/mmseqs/src/alignment/rescorediagonal.cpp:381
//   carpedeam ancient_correction    <seqDB> <alnDB> <outDB> [flags]           src/assembler/correction.cpp:492
//   carpedeam ancient_read_assemble <seqDB> <alnDB> <outDB> [flags]           src/assembler/ancientReadsResults.cpp:598
//
// Same positional arguments, flag names, on-disk DB formats and exit codes as the reference modules, so the workflow script
// (data/nuclassemble.sh:105,115,126,136) can call this binary for these four stages.  Each module reads its DBs, hands the
// work to the gfx950 library through the C ABI (include/carpedeam_hip.h) and writes the result DB with the reference's text
// codecs.  There is no CPU path: without an MI355X the module exits with an error, like any other fatal error in the
// reference ("Debug(Debug::ERROR) << ...; EXIT(EXIT_FAILURE)").
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <omp.h>
#include <unistd.h>
#include <dirent.h>
#include <sys/stat.h>
#include <fcntl.h>
#include <string>
#include <thread>
#include <vector>
#include <condition_variable>
#include <mutex>

#include "carpedeam_hip.h"
#include <sys/prctl.h>
#include <sys/wait.h>
#include <signal.h>
#include <cerrno>
#include "mmdb.h"
#include "sidecar.h"
#include "cli.h"
#include "contig_reports.h"
#include "modules.h"
#include "records.h"

namespace {
Args parse(int argc, char **argv) {
    Args a;
    for (int i = 0; i < argc; i++) {
        std::string s = argv[i];
        if (s.size() > 1 && s[0] == '-' && !isdigit((unsigned char) s[1])) { if (i + 1 < argc) { a.flag[s] = argv[i + 1]; i++; } }
        else a.pos.push_back(s);
    }
    return a;
}
const FlagSpec KMERMATCHER_FLAGS[] = {
    {"--kmer-per-seq", 'U', 0, 0}, {"--kmer-per-seq-scale", 'U', 0, 0}, {"--cov-mode", 'U', 0, 0}, {"-k", 'U', 0, 0}, {"-c", 'U', 0, 0}, {"--hash-shift", 'U', 0, 0},
    {"--include-only-extendable", 'U', 0, 0}, {"--ignore-multi-kmer", 'U', 0, 0},
    {"--alph-size", 'N', 0, "nucleotide k-mers are never reduced (kmermatcher.cpp:604)"}, {"--min-seq-id", 'N', 0, "not read by kmermatcher"},
    {"--max-seq-len", 'N', 0, "buffer sizing"}, {"--split-memory-limit", 'N', 0, "the device path is single-split"}, {"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0},
    {"--sub-mat", 'V', "*nucleotide.out*", "only the nucleotide matrix"}, {"--mask", 'V', "0", "tantan masking is not implemented"},
    {"--mask-lower-case", 'V', "0", "lower-case masking is not implemented"}, {"--spaced-kmer-mode", 'V', "0", "spaced k-mers are not implemented"},
    {"--spaced-kmer-pattern", 'V', "", "spaced k-mers are not implemented"}, {"--adjust-kmer-len", 'V', "0", "k-mer length adjustment is not implemented"},
    {"--compressed", 'V', "0", "compressed DBs are not implemented"}, {0, 0, 0, 0}};
const FlagSpec RESCORE_FLAGS[] = {
    {"-e", 'U', 0, 0}, {"-c", 'U', 0, 0}, {"--cov-mode", 'U', 0, 0}, {"--min-seq-id", 'U', 0, 0}, {"--min-aln-len", 'U', 0, 0},
    {"--add-self-matches", 'N', 0, "query DB == target DB: self matches are kept anyway (rescorediagonal.cpp:205)"}, {"--db-load-mode", 'N', 0, 0}, {"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0},
    {"--seq-id-mode", 'V', "0", "only alignment-length normalisation"}, {"--rescore-mode", 'V', "3", "only the end-to-end ungapped mode CarpeDeam uses"},
    {"--wrapped-scoring", 'V', "0", "not implemented"}, {"--filter-hits", 'V', "0", "not implemented"}, {"-a", 'V', "0", "no backtrace in mode 3"},
    {"--sort-results", 'V', "0", "not implemented"}, {"--sub-mat", 'V', "*nucleotide.out*", "only the nucleotide matrix"}, {"--compressed", 'V', "0", "compressed DBs are not implemented"}, {0, 0, 0, 0}};
// the module in linclust's pre-clustering mode (linclust.sh:27-31): --rescore-mode 0 --wrapped-scoring 1
const FlagSpec RESCORE_HAMMING_FLAGS[] = {
    {"-e", 'U', 0, 0}, {"-c", 'U', 0, 0}, {"--cov-mode", 'U', 0, 0}, {"--min-seq-id", 'U', 0, 0}, {"--min-aln-len", 'U', 0, 0}, {"--seq-id-mode", 'U', 0, 0},
    {"--add-self-matches", 'N', 0, "query DB == target DB: self matches are kept anyway (rescorediagonal.cpp:205)"}, {"--db-load-mode", 'N', 0, 0}, {"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0},
    {"--rescore-mode", 'V', "0", "this table is the Hamming mode's"}, {"--wrapped-scoring", 'V', "1", "the Hamming mode is implemented with wrapped scoring only"},
    {"--filter-hits", 'V', "0", "not implemented"}, {"-a", 'V', "0", "no backtrace in this mode"},
    {"--sort-results", 'V', "0", "not implemented"}, {"--sub-mat", 'V', "*nucleotide.out*", "only the nucleotide matrix"}, {"--compressed", 'V', "0", "compressed DBs are not implemented"}, {0, 0, 0, 0}};
const FlagSpec ANCIENT_FLAGS[] = {
    {"--min-seq-id", 'U', 0, 0}, {"--max-seq-len", 'U', 0, 0}, {"--ext-random-align", 'U', 0, 0}, {"--excess-penalty", 'U', 0, 0}, {"--min-ryseq-id-corr-reads", 'U', 0, 0},
    {"--likelihood-ratio-threshold", 'U', 0, 0}, {"--ancient-damage", 'U', 0, 0}, {"--unsafe", 'U', 0, 0}, {"--min-cov-safe", 'U', 0, 0},
    {"--keep-target", 'N', 0, "not read by these modules"}, {"--min-seqid-corr-reads", 'N', 0, "not read by these modules"}, {"--min-merge-seq-id", 'U', 0, 0},
    {"--min-seqid-corr-contigs", 'N', 0, "a workflow flag: it becomes the contig phase's --min-seq-id (Nuclassembler.cpp:124-126); ancient_reads_loop reads it"}, {"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0},
    {"--rescore-mode", 'V', "3", "re-alignment of parked candidates is end-to-end ungapped (ancientReadsResults.cpp:502)"}, {0, 0, 0, 0}};
// The end of a module whose outputs are written and closed: the process leaves HERE - no release of device buffers (giving tens of GB
// back to the driver costs seconds, profiles/r05_time_modules_50M_*), no unmapping of the input files, no destructors of the
// multi-GB host buffers; the operating system and the driver take everything back at once.  (Not under a profiler or sanitizer that
// writes its results from an exit handler - ROCP_TOOL_LIBRARIES / LD_PRELOAD / CDM_NORMAL_EXIT: then the caller releases and returns.)
bool leaveAtOnce() {
    if (getenv("ROCP_TOOL_LIBRARIES") || getenv("CDM_NORMAL_EXIT")) return false;
    const char *pre = getenv("LD_PRELOAD");         // (a profiler's preload counts, any other preloaded library - a deployment's exec guard, an allocator - does not)
    return !(pre && (strstr(pre, "rocprof") || strstr(pre, "roctracer") || strstr(pre, "rocprofiler")));
}
// The caller gets its answer before this process is torn down: the work runs in a CHILD of the process the caller started (forked first
// thing in main, before anything touches the device), the parent waits for one byte - the exit status, sent when every output file is
// written and closed - and leaves with it at once.  Tearing down a module's address space (tens of GB of host buffers and mapped DB
// files at 50 M reads: 0.4-1.3 s, profiles/r05_probe_module_gap.txt) then happens beside the next module of the workflow instead of
// in front of it.  A child that ends without the byte (a crash, an error exit) is waited for and its status handed on.
// Not under a profiler (leaveAtOnce()) and not with CDM_NO_FORK=1.
int g_doneFd = -1;
void reportDone(int rc) {
    if (g_doneFd < 0) return;
    prctl(PR_SET_PDEATHSIG, 0);         // (from here on the parent's leaving is the plan, not an accident)
    const unsigned char b = (unsigned char) rc;
    if (write(g_doneFd, &b, 1) != 1) {}
    close(g_doneFd); g_doneFd = -1;
    close(0); close(1); close(2);       // (a caller that reads this process's output through pipes waits for their last writer)
}
void finishModule(int rc) {
    if (!leaveAtOnce()) return;
    const auto n = std::chrono::steady_clock::now();
    if (getenv("CDM_TIMING")) fprintf(stderr, "  %-32s %.3f s\n", "(since the last lap)", std::chrono::duration<double>(n - g_lastLap).count());
    fprintf(stderr, "Time for processing: %.3fs\n", std::chrono::duration<double>(n - g_t0).count());
    fflush(stdout); fflush(stderr);
    reportDone(rc);
    _exit(rc);
}
// ---- ancient_reads_loop --gpus N: the ranks are host threads of this process, one device each, and the library splits the read
// iterations over them (cdm_reads_iteration_dist, csrc/dist.hip) - over RCCL.  CDM_LOOP_TRANSPORT=threads (tests on a one-GPU box,
// where RCCL has no second device to give a rank): all ranks share the first device and the collectives are these few lines - the
// ranks publish their buffers, meet at a barrier and copy from each other with cdm_dev_copy.
struct RankBarrier {
    std::mutex m; std::condition_variable cv; int world = 1, waiting = 0; long generation = 0;
    void wait() {
        std::unique_lock<std::mutex> l(m);
        const long g = generation;
        if (++waiting == world) { waiting = 0; generation++; cv.notify_all(); }
        else cv.wait(l, [&] { return generation != g; });
    }
};
struct ThreadTransport {
    int world = 1; RankBarrier bar;
    std::vector<const void *> ptr; std::vector<const uint64_t *> off; std::vector<uint64_t> bytes;
    explicit ThreadTransport(int w) : world(w), ptr(w), off(w), bytes(w) { bar.world = w; }
};
struct ThreadRank { ThreadTransport *t; int rank; cdm_ctx *ctx; };
int ttAllGatherHost(void *user, const void *send, void *recv, uint64_t n) {
    ThreadRank *r = (ThreadRank *) user; ThreadTransport &t = *r->t;
    t.ptr[r->rank] = send; t.bar.wait();
    for (int p = 0; p < t.world; p++) memcpy((char *) recv + (size_t) p * n, t.ptr[p], n);
    t.bar.wait();
    return 0;
}
int ttAllToAllDev(void *user, const void *send, const uint64_t *soff, void *recv, const uint64_t *roff, void *) {
    ThreadRank *r = (ThreadRank *) user; ThreadTransport &t = *r->t;
    if (cdm_ctx_sync(r->ctx)) return -1;                 // what this rank sends is complete
    t.ptr[r->rank] = send; t.off[r->rank] = soff; t.bar.wait();
    int rc = 0;
    for (int p = 0; p < t.world && !rc; p++) {
        const uint64_t n = t.off[p][r->rank + 1] - t.off[p][r->rank];
        if (n != roff[p + 1] - roff[p]) rc = -1;
        else if (n) rc = cdm_dev_copy(r->ctx, (char *) recv + roff[p], (const char *) t.ptr[p] + t.off[p][r->rank], n);
    }
    t.bar.wait();                                        // nobody frees its send buffer before everybody has copied
    return rc;
}
int ttAllGatherDev(void *user, const void *send, uint64_t n, void *recv, const uint64_t *roff, void *) {
    ThreadRank *r = (ThreadRank *) user; ThreadTransport &t = *r->t;
    if (cdm_ctx_sync(r->ctx)) return -1;
    t.ptr[r->rank] = send; t.bytes[r->rank] = n; t.bar.wait();
    int rc = 0;
    for (int p = 0; p < t.world && !rc; p++) {
        if (t.bytes[p] != roff[p + 1] - roff[p]) rc = -1;
        else if (t.bytes[p]) rc = cdm_dev_copy(r->ctx, (char *) recv + roff[p], t.ptr[p], t.bytes[p]);
    }
    t.bar.wait();
    return rc;
}
// The device side of a module's start - runtime initialisation and context (0.1-0.2 s), damage tables, sequence upload - in a thread
// of its own, while the main thread maps and parses the module's text DBs.  Errors are kept and raised by join() on the main thread.
// ---- binary side-cars (host/sidecar.h)
// sections of a sequence side-car: keys, lengths, wasExtended flags, letter flags (hasN), code words, [N masks], [raw plane]
bool importSeqSide(cdm_ctx *ctx, const SideFile &f, cdm_seqdb **out) {
    const SideHeader &h = *f.h;
    const bool hasMask = (h.flags & SIDE_F_HAS_NMASK) != 0, hasRaw = (h.flags & SIDE_F_HAS_RAW) != 0;
    return cdm_seqdb_import_packed(ctx, f.section(4), hasMask ? f.section(5) : NULL, f.section(1), f.section(0), f.section(2), hasRaw ? f.section(6) : NULL,
                                   hasRaw ? f.section(3) : NULL, h.n, h.count, out) == CDM_OK;
}
// the device DB `h` as a side-car, in two steps: take() brings the packed form to the host while the device still holds it, write() puts
// it next to the text DB at `path` once that DB's files are complete; a failure of either leaves the text DB on its own
struct SeqSideHost {
    HVec<uint32_t> keys, lens, codes; HVec<uint8_t> ext, flags, raw; HVec<uint16_t> mask;
    uint64_t n = 0, words = 0; bool have = false, hasRaw = false;
    void take(cdm_ctx *ctx, cdm_seqdb *h) {
        have = false;
        if (!sideEnabled()) return;
        n = cdm_seqdb_size(h); words = cdm_seqdb_words(h);
        if (n == 0) return;
        keys.resize(n); lens.resize(n); codes.resize(words + 1); ext.resize(n); flags.resize(n); mask.resize(words + 1);
        hasRaw = cdm_seqdb_has_raw(h) != 0;
        if (hasRaw) raw.resize(words * 16 + 1);
        have = cdm_seqdb_export_packed(ctx, h, codes.data(), mask.data(), lens.data(), keys.data(), ext.data(), hasRaw ? raw.data() : NULL, flags.data()) == CDM_OK;
    }
    // begin(): the sections go out in a thread of their own (the caller writes the text DB meanwhile); commit(): the text DB is complete
    std::thread th; SideHeader hdr; bool bodyOk = false; std::string path;
    void begin(const std::string &p, int dbtype) {
        if (!have) return;
        path = p;
        th = std::thread([this, dbtype] {
            bool anyN = false;
            for (size_t i = 0; i < n && !anyN; i++) anyN = flags[i] != 0;
            const SidePiece pc[7] = {{keys.data(), n * 4}, {lens.data(), n * 4}, {ext.data(), n}, {flags.data(), n}, {codes.data(), words * 4}, {mask.data(), anyN ? words * 2 : 0}, {raw.data(), hasRaw ? words * 16 : 0}};
            bodyOk = sideWriteBody(path, SIDE_SEQ, (anyN ? SIDE_F_HAS_NMASK : 0) | (hasRaw ? SIDE_F_HAS_RAW : 0), n, words, 0, 0, dbtype, pc, 7, &hdr);
        });
    }
    void commit() { if (th.joinable()) { th.join(); if (bodyOk) sideCommit(path, &hdr); } }
    void write(const std::string &p, int dbtype) { begin(p, dbtype); commit(); }
};
// What a module still holds on the device goes back to the driver as soon as its last result is on the host, BEFORE the text is formatted
// and written: memory a process gives back is cleared by the driver before another process gets it (~30 ms per GB, in the background:
// profiles/r05_probe_exit.txt), and the next module of the workflow starts milliseconds after this one ends - it found that clearing in
// its way (0.35 -> 2.5 s for rescorediagonal's kernels behind kmermatcher).  Giving back is quick (10 ms for 140 GB); it is this thread's
// arenas that hold the memory (the kernels ran here), so this thread does it.
struct DeviceEnd {
    void begin(cdm_ctx *ctx, cdm_hits *hits, cdm_alns *alns, cdm_seqdb *a, cdm_seqdb *b) {
        if (hits) cdm_hits_free(hits);
        if (alns) cdm_alns_free(alns);
        if (a) cdm_seqdb_free(a);
        if (b) cdm_seqdb_free(b);
        cdm_ctx_destroy(ctx);
    }
    void join() {}
};
// A sequence DB as a module takes it: from its side-car when that matches the files - index columns from the side-car's arrays, no text
// mapped - else from the text (MmDb::load).
struct SeqInput {
    MmDb db; SideFile side; bool fromSide = false;
    void load(const std::string &path) {
        if (sideOpen(path, SIDE_SEQ, side)) {
            const SideHeader &h = *side.h;
            db.adoptIndex((const uint32_t *) side.section(0), (const uint32_t *) side.section(1), (const uint8_t *) side.section(2), h.n, h.dbtype);
            fromSide = true;
            if (getenv("CDM_TIMING")) fprintf(stderr, "  sequence DB %s: from its side-car\n", path.c_str());
            return;
        }
        std::string err; if (!db.load(path, &err)) die(err);
        if (getenv("CDM_TIMING")) fprintf(stderr, "  sequence DB %s: from the text\n", path.c_str());
    }
};
struct DeviceStart {
    std::thread th; cdm_ctx *ctx = NULL; cdm_seqdb *db = NULL;
    std::string err; int code = 0;
    void fail(int c, const std::string &m) { code = c; err = m; }
    void begin(const SeqInput *in, const std::string *damagePrefix) { begin(in ? &in->db : NULL, damagePrefix, in && in->fromSide ? &in->side : NULL); }
    void begin(const MmDb *seq, const std::string *damagePrefix, const SideFile *side = NULL) {
        th = std::thread([this, seq, damagePrefix, side] {
            const char *dev = getenv("CARPEDEAM_DEVICE");
            if (cdm_ctx_create(dev ? atoi(dev) : 0, &ctx) != CDM_OK) return fail(EXIT_FAILURE, std::string("Can not initialise the MI355X device: ") + cdm_last_error());
            if (damagePrefix && cdm_damage_load(ctx, damagePrefix->c_str()) != CDM_OK) return fail(EXIT_FAILURE, std::string("Profile not 12 fields: ") + cdm_last_error());
            if (!seq) return;
            // (a side-car of another dbtype goes the text's way, which refuses the dbtype before it looks at the text that was never mapped)
            if (side && (seq->dbtype & 0x7FFFFFFF) == 1) { if (!importSeqSide(ctx, *side, &db)) fail(EXIT_FAILURE, std::string("Can not load the sequence DB: ") + cdm_last_error()); return; }
            std::string msg;
            if (const int rc = seqDbToDevice(ctx, *seq, &db, &msg)) fail(rc, msg);
        });
        g_deviceThread = &th;
    }
    void join() {
        if (th.joinable()) th.join();
        g_deviceThread = NULL;
        if (code) { fprintf(stderr, "%s\n", err.c_str()); exit(code); }
    }
};
// The index columns of a device DB (n > 0) as a data file lays its entries out - "SEQ\n\0" each, entry i at offs[i] with elen[i] bytes, the
// NUL among them; fill() returns the bytes of them all
struct SeqDbLayout {
    HVec<uint32_t> keys, elen; HVec<uint8_t> ext; HVec<uint64_t> offs;
    uint64_t fill(cdm_ctx *ctx, cdm_seqdb *h) {
        const uint64_t n = cdm_seqdb_size(h);
        keys.resize(n); elen.resize(n); ext.resize(n); offs.resize(n);
        check(cdm_seqdb_meta(ctx, h, elen.data(), keys.data(), ext.data()), "meta");
        uint64_t tot = 0;
        for (uint64_t i = 0; i < n; i++) { offs[i] = tot; elen[i] += 2; tot += elen[i]; }
        return tot;
    }
};
// the entries of a device DB as DB payloads ("SEQ\n"), appended to c
void appendEntries(cdm_ctx *ctx, cdm_seqdb *h, OutChunk &c) {
    const uint64_t n = cdm_seqdb_size(h);
    if (n == 0) return;
    SeqDbLayout l; const uint64_t tot = l.fill(ctx, h);
    HVec<char> buf(tot);
    check(cdm_seqdb_download(ctx, h, buf.data(), l.offs.data()), "download");
    c.reserve(c.key.size() + n, c.data.size() + tot);
    for (uint64_t i = 0; i < n; i++) c.add(l.keys[i], buf.data() + l.offs[i], l.elen[i] - 1, l.ext[i]);
}
// a device DB as a text DB (+ its side-car): down() takes everything off the device, write() needs the device no more
struct SeqDbOut {
    uint64_t n = 0; SeqDbLayout l; HVec<char> buf; SeqSideHost side;
    void down(cdm_ctx *ctx, cdm_seqdb *h) {
        n = cdm_seqdb_size(h);
        if (n == 0) return;
        // the download buffer has the data file's layout already: "SEQ\n\0" per entry (the NULs are the buffer's zero fill)
        const uint64_t tot = l.fill(ctx, h);
        buf.resize(tot);
        buf[tot - 1] = '\0';           // the download writes [0, tot - 1): "SEQ\n" per entry and the NULs between them; the last entry's NUL is ours
        check(cdm_seqdb_download(ctx, h, buf.data(), l.offs.data()), "download");
        side.take(ctx, h);
    }
    void write(const std::string &path, int dbtype) {
        std::string err;
        if (n == 0) { if (!mmdbWriteChunks(path, dbtype, std::vector<OutChunk>(1), &err)) die(err); return; }
        side.begin(path, dbtype);       // (beside the text: other files)
        if (!mmdbWriteBlob(path, dbtype, buf.data(), buf.size(), l.keys.data(), l.offs.data(), l.elen.data(), l.ext.data(), n, &err)) die(err);
        side.commit();
    }
};
// The same in one go where the DB's data file takes its pieces straight off the device (a RAM-backed file system, where one writer per
// file is the fast way): the text streams through the library's pinned staging buffers into the file (cdm_seqdb_download_stream) while the
// index and the side-car go out in threads of their own - the text never stands in pageable memory.  false: not here (nothing was
// written; down() + write() as before).  The device DB is still needed until this returns.
static int seqDbPieceSink(void *user, const char *data, uint64_t offset, uint64_t bytes) { return mmdbWritePiece(*(int *) user, data, offset, bytes) ? 0 : 1; }
bool streamSeqDb(cdm_ctx *ctx, cdm_seqdb *h, const std::string &path, int dbtype) {
    const uint64_t n = cdm_seqdb_size(h);
    if (n == 0) return false;
    SeqDbLayout l; const uint64_t tot = l.fill(ctx, h);
    int fd = mmdbOpenStreamedData(path, tot);
    if (fd < 0) return false;
    SeqSideHost side; side.take(ctx, h); side.begin(path, dbtype);
    bool okIx = true; std::string errIx;
    std::thread ix([&] { okIx = mmdbWriteBlob(path, dbtype, nullptr, 0, l.keys.data(), l.offs.data(), l.elen.data(), l.ext.data(), n, &errIx, MMDB_DATA_ELSEWHERE); });
    const int rc = cdm_seqdb_download_stream(ctx, h, l.offs.data(), 64u << 20, seqDbPieceSink, &fd);
    const bool okClose = close(fd) == 0;
    ix.join();
    if (rc != CDM_OK) die(std::string("download: ") + cdm_last_error());
    if (!okClose) die("Could not write " + path);
    if (!okIx) die(errIx);
    side.commit();
    return true;
}
void writeSeqDb(cdm_ctx *ctx, cdm_seqdb *h, const std::string &path, int dbtype) { if (streamSeqDb(ctx, h, path, dbtype)) return; SeqDbOut o; o.down(ctx, h); o.write(path, dbtype); }
cdm_ancient_params ancientParams(Args &a) {
    cdm_ancient_params p;
    p.seq_id_thr = fflag(a, "--min-seq-id", 0.9f); p.corr_reads_ry_seq_id = fflag(a, "--min-ryseq-id-corr-reads", 0.99f); p.ry_seq_id_thr = 0.99f;
    p.rand_align_penal = fflag(a, "--ext-random-align", 0.85f); p.excess_penal = fflag(a, "--excess-penalty", 0.0625f);
    p.likelihood_threshold = fflag(a, "--likelihood-ratio-threshold", 0.5f); p.unsafe = (int) iflag(a, "--unsafe", 0);
    p.min_cov_safe = (int) iflag(a, "--min-cov-safe", 5); p.max_seq_len = (uint64_t) iflag(a, "--max-seq-len", 65535);
    return p;
}
// the modules' parameters from their flags (kmermatcher; rescorediagonal's Hamming mode): ancient_assemble_fused reads them the same way
cdm_kmer_params kmerParams(Args &a) {
    cdm_kmer_params p;
    p.kmer_size = (int) iflag(a, "-k", 15); p.kmers_per_seq = (int) iflag(a, "--kmer-per-seq", 21); p.kmers_per_seq_scale = fflag(a, "--kmer-per-seq-scale", 0.2f);
    p.hash_shift = (uint64_t) iflag(a, "--hash-shift", 67); p.ignore_multi_kmer = (int) iflag(a, "--ignore-multi-kmer", 0);
    p.include_only_extendable = (int) iflag(a, "--include-only-extendable", 0); p.cov_mode = (int) iflag(a, "--cov-mode", 0); p.cov_thr = fflag(a, "-c", 0.8f);
    return p;
}
cdm_rescore_params rescoreParams(Args &a) {
    cdm_rescore_params p;
    p.seq_id_thr = fflag(a, "--min-seq-id", 0.0f); p.eval_thr = dflag(a, "-e", 0.001);
    p.cov_mode = (int) iflag(a, "--cov-mode", 0); p.cov_thr = fflag(a, "-c", 0.0f); p.seq_id_mode = (int) iflag(a, "--seq-id-mode", 0); p.min_aln_len = (int) iflag(a, "--min-aln-len", 0);
    return p;
}
cdm_hamming_params hammingParams(Args &a, bool reversePrefilter) {      // the same six flags and the prefilter's strand convention
    const cdm_rescore_params r = rescoreParams(a);
    return {r.seq_id_thr, r.eval_thr, r.cov_mode, r.cov_thr, r.seq_id_mode, r.min_aln_len, reversePrefilter};
}
int kmermatcher(Args &a) {
    if (a.pos.size() < 2) die("Usage: carpedeam kmermatcher <i:sequenceDB> <o:prefilterDB>");
    checkFlags("kmermatcher", a, KMERMATCHER_FLAGS);
    Laps laps;
    DeviceStart dev; dev.begin((const MmDb *) NULL, NULL);                 // (the context comes up while the DB is mapped and its index parsed)
    SeqInput in; in.load(a.pos[0]); MmDb &seq = in.db; std::string err;
    laps.lap(in.fromSide ? "sequence side-car mapped" : "DB files mapped");
    dev.join(); cdm_ctx *ctx = dev.ctx; laps.lap("device context");
    cdm_seqdb *db = NULL;
    if (in.fromSide) { if ((seq.dbtype & 0x7FFFFFFF) != 1) unsupported("The MI355X path works on nucleotide sequence DBs only"); if (!importSeqSide(ctx, in.side, &db)) die(std::string("Can not load the sequence DB: ") + cdm_last_error()); }
    else db = uploadSeqDb(ctx, seq);
    laps.lap("sequences up");
    cdm_kmer_params p = kmerParams(a);
    cdm_hits *hits = NULL;
    check(cdm_kmermatch(ctx, db, &p, &hits), "kmermatcher");
    HVec<uint64_t> off(seq.size() + 1); HVec<cdm_hit> rec(cdm_hits_count(hits));
    check(cdm_hits_download(ctx, hits, off.data(), rec.data()), "download");
    SeqSideHost inSide; if (!in.fromSide) inSide.take(ctx, db);       // (the next modules of the workflow read this DB again)
    laps.lap("kernels, hits down");
    DeviceEnd end; end.begin(ctx, hits, NULL, db, NULL); laps.lap("device memory back to the driver");
    SideThread hitsSide; hitsSide.begin(a.pos[1], [&](SideHeader *h) { return writeHitsSide(a.pos[1], seq, off.data(), rec.data(), 14, h); });
    inSide.begin(a.pos[0], seq.dbtype);
    std::vector<OutChunk> chunks;
    formatPrefDb(seq, off.data(), rec.data(), chunks);
    laps.lap("prefilter text formatted");
    if (!mmdbWriteChunks(a.pos[1], 14, chunks, &err, true)) die(err);   // DBTYPE_PREFILTER_REV_RES (kmermatcher.cpp:682)
    laps.lap("result DB written");
    hitsSide.commit(); inSide.commit();
    laps.lap("(side-cars, written beside: waited)");
    finishModule(EXIT_SUCCESS);
    return EXIT_SUCCESS;
}

int rescorediagonal(Args &a) {
    if (a.pos.size() < 4) die("Usage: carpedeam rescorediagonal <i:queryDB> <i:targetDB> <i:prefilterDB> <o:resultDB>");
    const bool hamming = a.flag.count("--rescore-mode") && a.flag["--rescore-mode"] == "0" && a.flag.count("--wrapped-scoring") && a.flag["--wrapped-scoring"] == "1";
    checkFlags("rescorediagonal", a, hamming ? RESCORE_HAMMING_FLAGS : RESCORE_FLAGS);
    if (a.pos[0] != a.pos[1]) unsupported("rescorediagonal: query and target DB must be the same on the MI355X path");
    if (hamming) {      // linclust's pre-clustering of the assembled contigs: prefilter records in, prefilter records out
        MmDb seq, pref; std::string err; if (!seq.load(a.pos[1], &err)) die(err);
        DeviceStart dev; dev.begin(&seq, NULL);
        if (!pref.load(a.pos[2], &err)) die(err);
        HVec<uint64_t> off; HVec<cdm_hit> rec;
        parsePrefDb(pref, seq, off, rec);
        dev.join(); cdm_ctx *ctx = dev.ctx; cdm_seqdb *db = dev.db;
        cdm_hits *hits = NULL, *kept = NULL;
        check(cdm_hits_upload(ctx, db, off.data(), rec.data(), &hits), "upload");
        cdm_hamming_params p = hammingParams(a, (pref.dbtype & 0x7FFFFFFF) == 14);
        check(cdm_rescore_hamming(ctx, db, hits, &p, &kept), "rescorediagonal");
        HVec<uint64_t> koff(seq.size() + 1); HVec<cdm_hit> krec(cdm_hits_count(kept));
        check(cdm_hits_download(ctx, kept, koff.data(), krec.data()), "download");
        std::vector<OutChunk> chunks;
        formatRescoredPrefDb(seq, pref, koff.data(), krec.data(), chunks);
        if (!mmdbWriteChunks(a.pos[3], pref.dbtype, chunks, &err, true)) die(err);
        cdm_hits_free(kept); cdm_hits_free(hits); cdm_seqdb_free(db); cdm_ctx_destroy(ctx);
        return EXIT_SUCCESS;
    }
    if (!a.flag.count("--rescore-mode")) unsupported("rescorediagonal: --rescore-mode 3 has to be given (the module's default, 0 = Hamming distance, is implemented with --wrapped-scoring 1 only on the MI355X path)");
    Laps laps;
    SeqInput in; in.load(a.pos[1]); MmDb &seq = in.db; MmDb pref; std::string err;
    DeviceStart dev; dev.begin(&in, NULL);                  // context + sequence upload while the prefilter records are read
    HVec<uint64_t> off; HVec<cdm_hit> rec;
    int prefType = 0;
    const bool hitsFromSide = readHitsSide(a.pos[2], seq, off, rec, &prefType);
    if (hitsFromSide) laps.lap("side-cars mapped, prefilter records read");
    else {
        if (!pref.load(a.pos[2], &err)) die(err);
        laps.lap("DB files mapped");
        parsePrefDb(pref, seq, off, rec);
        laps.lap("prefilter text parsed");
    }
    dev.join(); cdm_ctx *ctx = dev.ctx; cdm_seqdb *db = dev.db; laps.lap("(device context, sequences up: waited)");
    cdm_hits *hits = NULL; cdm_alns *alns = NULL;
    check(cdm_hits_upload(ctx, db, off.data(), rec.data(), &hits), "upload"); laps.lap("  (hits up)");
    cdm_rescore_params p = rescoreParams(a);
    check(cdm_rescore(ctx, db, hits, &p, &alns), "rescorediagonal"); laps.lap("  (kernels)");
    HVec<uint64_t> aoff(seq.size() + 1); HVec<cdm_aln> arec(cdm_alns_count(alns));
    check(cdm_alns_download(ctx, alns, aoff.data(), arec.data()), "download");
    const uint64_t dbResidues = cdm_seqdb_residues(db);
    SeqSideHost inSide; if (!in.fromSide) inSide.take(ctx, db);
    laps.lap("hits up, kernels, records down");
    DeviceEnd end; end.begin(ctx, hits, alns, db, NULL); laps.lap("device memory back to the driver");
    std::vector<OutChunk> chunks;
    HVec<cdm_aln> asParsed; if (sideEnabled()) asParsed.resize(arec.size());
    formatAlnDb(seq, hitsFromSide ? NULL : &pref, aoff.data(), arec.data(), dbResidues, chunks, sideEnabled() ? asParsed.data() : NULL);
    laps.lap("alignment text formatted");
    // (an alignment side-car holds every query: only when every query has a prefilter entry - kmermatcher's output - does the text too)
    bool allPresent = hitsFromSide;
    if (!allPresent) { allPresent = true; for (size_t i = 0; i < seq.size() && allPresent; i++) allPresent = pref.idOf(seq.key[i]) >= 0; }
    SideThread alnSide; if (allPresent) alnSide.begin(a.pos[3], [&](SideHeader *h) { return writeAlnsSide(a.pos[3], seq, aoff.data(), asParsed.data(), h); });
    inSide.begin(a.pos[1], seq.dbtype);
    if (!mmdbWriteChunks(a.pos[3], 5, chunks, &err, true)) die(err);
    laps.lap("result DB written");
    alnSide.commit(); inSide.commit();
    laps.lap("(side-cars, written beside: waited)");
    finishModule(EXIT_SUCCESS);
    return EXIT_SUCCESS;
}

int ancientModule(Args &a, int mode) {      // 0 ancient_correction, 1 ancient_read_assemble, 2 ancient_contig_merge
    const bool assemble = mode == 1;
    const char *name = mode == 0 ? "ancient_correction" : mode == 1 ? "ancient_read_assemble" : "ancient_contig_merge";
    if (a.pos.size() < 3) die(std::string("Usage: carpedeam ") + name + " <i:sequenceDB> <i:alnResult> <o:reprSeqDB>");
    checkFlags(name, a, ANCIENT_FLAGS);
    if (mode >= 1 && !a.flag.count("--rescore-mode")) unsupported(std::string(name) + ": --rescore-mode 3 has to be given (the module's default, 0 = Hamming distance, is not implemented on the MI355X path)");
    Laps laps;
    SeqInput in; in.load(a.pos[0]); MmDb &seq = in.db; MmDb aln; std::string err;
    const std::string damage = a.flag.count("--ancient-damage") ? a.flag["--ancient-damage"] : "";
    DeviceStart dev; dev.begin(&in, &damage);               // context, damage tables, sequence upload while the alignment records are read
    HVec<uint64_t> off; HVec<cdm_aln> rec;
    if (readAlnsSide(a.pos[1], seq, off, rec)) laps.lap("side-cars mapped, alignment records read");
    else {
        if (!aln.load(a.pos[1], &err)) die(err);
        laps.lap("DB files mapped");
        parseAlnDb(aln, seq, off, rec); laps.lap("alignment text parsed");
    }
    dev.join(); cdm_ctx *ctx = dev.ctx; cdm_seqdb *db = dev.db; laps.lap("(device context, damage tables, sequences up: waited)");
    cdm_alns *alns = NULL; cdm_seqdb *out = NULL;
    check(cdm_alns_upload(ctx, db, off.data(), rec.data(), &alns), "upload");
    cdm_ancient_params p = ancientParams(a);
    if (assemble) check(cdm_extend(ctx, db, alns, &p, &out, NULL), "ancient_read_assemble");
    else if (mode == 2) check(cdm_contig_merge(ctx, db, alns, &p, fflag(a, "--min-merge-seq-id", 0.99f), &out), "ancient_contig_merge");
    else check(cdm_correct(ctx, db, alns, &p, &out), "ancient_correction");
    laps.lap("records up, kernels");
    SeqSideHost inSide; if (!in.fromSide) inSide.take(ctx, db);
    inSide.begin(a.pos[0], seq.dbtype);
    if (streamSeqDb(ctx, out, a.pos[2], seq.dbtype)) {      // (tmpfs: the text goes from the device into the data file piece by piece)
        laps.lap("sequences down into the DB's data file, index and side-car beside it");
        DeviceEnd end; end.begin(ctx, NULL, alns, db, out); laps.lap("device memory back to the driver");
    } else {
        SeqDbOut o; o.down(ctx, out);
        laps.lap("sequences down");
        DeviceEnd end; end.begin(ctx, NULL, alns, db, out); laps.lap("device memory back to the driver");
        o.write(a.pos[2], seq.dbtype); laps.lap("DB written, its side-car beside it");
    }
    inSide.commit();
    finishModule(EXIT_SUCCESS);
    return EXIT_SUCCESS;
}
// cyclecheck <i:sequenceDB> <o:sequenceDBcycle> (src/assembler/cyclecheck.cpp:30-269; flags: LocalParameters.h:183-187)
const FlagSpec CYCLECHECK_FLAGS[] = {{"--max-seq-len", 'U', 0, 0}, {"--chop-cycle", 'U', 0, 0}, {"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0}, {0, 0, 0, 0}};
int cyclecheck(Args &a) {
    if (a.pos.size() < 2) die("Usage: carpedeam cyclecheck <i:sequenceDB> <o:sequenceDBcycle>");
    checkFlags("cyclecheck", a, CYCLECHECK_FLAGS);
    MmDb seq; std::string err; if (!seq.load(a.pos[0], &err)) die(err);
    if ((seq.dbtype & 0x7FFFFFFF) != 1) die("Module cyclecheck only supports nucleotide input database");
    cdm_ctx *ctx = openCtx();
    cdm_seqdb *db = uploadSeqDb(ctx, seq), *cyc = NULL;
    const long maxLen = std::min(iflag(a, "--max-seq-len", 65535), 0xFFFFFFFFl);
    check(cdm_cyclecheck(ctx, db, (uint32_t) maxLen, iflag(a, "--chop-cycle", 0) != 0, &cyc, NULL, NULL), "cyclecheck");
    writeSeqDb(ctx, cyc, a.pos[1], 1);
    cdm_seqdb_free(cyc); cdm_seqdb_free(db); cdm_ctx_destroy(ctx);
    return EXIT_SUCCESS;
}
// Fused reads loop: the body of `while [ $STEP -lt $NUM_IT_READS ]` of data/nuclassemble.sh:100-146
// - kmermatcher, rescorediagonal, ancient_correction, ancient_read_assemble per iteration - in one process with every
// intermediate resident in HBM; no prefilter/alignment/correction text DB is written, only the final sequence DB.
// Not a module of the reference; the per-stage modules above remain the drop-in surface.
// linclust's host-side tail and the scripts' file modules (host/cluster.cpp); flag lists: Parameters.cpp clust / createsubdb / filterdb /
// threadsandcompression / onlyverbosity
int clusterModules(const std::string &cmd, Args &a) {
    static const FlagSpec CLUST_FLAGS[] = {{"--cluster-mode", 'U', 0, 0}, {"--max-iterations", 'N', 0, "connected-component mode only"}, {"--similarity-type", 'N', 0, "set-cover mode only"},
                                           {"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0}, {"--compressed", 'V', "0", "compressed DBs are not implemented"}, {0, 0, 0, 0}};
    static const FlagSpec SUBDB_FLAGS[] = {{"--subdb-mode", 'U', 0, 0}, {"-v", 'N', 0, 0}, {"--id-mode", 'V', "0", "look-up mode is not implemented"}, {0, 0, 0, 0}};
    static const FlagSpec FILTER_FLAGS[] = {{"--filter-file", 'U', 0, 0}, {"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0}, {"--compressed", 'V', "0", "compressed DBs are not implemented"},
                                            {"--filter-column", 'V', "1", "only the first column"}, {"--positive-filter", 'V', "1", "only positive filtering"}, {0, 0, 0, 0}};
    static const FlagSpec PLAIN_FLAGS[] = {{"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0}, {"--db-load-mode", 'N', 0, 0}, {"--compressed", 'V', "0", "compressed DBs are not implemented"}, {0, 0, 0, 0}};
    // align (Parameters.cpp: par.align): what changes the result of a nucleotide, no-backtrace, no-realign run is read; modes this path
    // does not have are refused
    static const FlagSpec ALIGN_FLAGS[] = {
        {"-e", 'U', 0, 0}, {"--min-seq-id", 'U', 0, 0}, {"--min-aln-len", 'U', 0, 0}, {"--seq-id-mode", 'U', 0, 0}, {"-c", 'U', 0, 0}, {"--cov-mode", 'U', 0, 0}, {"--max-seq-len", 'U', 0, 0},
        {"--max-rejected", 'U', 0, 0}, {"--max-accept", 'U', 0, 0}, {"--wrapped-scoring", 'U', 0, 0}, {"--gap-open", 'U', 0, 0}, {"--gap-extend", 'U', 0, 0}, {"--zdrop", 'U', 0, 0},
        {"--alignment-mode", 'N', 0, "nucleotide alignments always compute score, coverage and identity (Matcher.cpp:88)"}, {"--comp-bias-corr", 'N', 0, "amino acids only"},
        {"--add-self-matches", 'N', 0, "query DB == target DB: the identity hit is kept anyway"}, {"--db-load-mode", 'N', 0, 0}, {"--pca", 'N', 0, "profiles only"}, {"--pcb", 'N', 0, "profiles only"},
        {"--realign-score-bias", 'N', 0, "no realignment"}, {"--realign-max-seqs", 'N', 0, "no realignment"}, {"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0},
        {"-a", 'V', "0", "no backtrace output"}, {"--alignment-output-mode", 'V', "0", "only alignment records"}, {"--alt-ali", 'V', "0", "not supported for nucleotides in the reference either"},
        {"--realign", 'V', "0", "not implemented"}, {"--score-bias", 'V', "0", "not implemented"}, {"--sub-mat", 'V', "*nucleotide.out*", "only the nucleotide matrix"},
        {"--compressed", 'V', "0", "compressed DBs are not implemented"}, {0, 0, 0, 0}};
    std::string err; int rc = 0;
    auto need = [&](size_t n, const char *usage) { if (a.pos.size() < n) die(std::string("Usage: carpedeam ") + usage); };
    auto nuclValue = [&](const char *flag, long dflt) -> long {      // "5" or "nucl:5,aa:11"
        if (!a.flag.count(flag)) return dflt;
        const std::string &v = a.flag[flag];
        const size_t at = v.find("nucl:");
        return strtol(v.c_str() + (at == std::string::npos ? 0 : at + 5), NULL, 10);
    };
    if (cmd == "align") {
        need(4, "align <i:queryDB> <i:targetDB> <i:resultDB> <o:alignmentDB>"); checkFlags("align", a, ALIGN_FLAGS);
        AlignParams P;
        P.covThr = fflag(a, "-c", 0.0f); P.seqIdThr = fflag(a, "--min-seq-id", 0.0f); P.evalThr = dflag(a, "-e", 0.001);
        P.covMode = (int) iflag(a, "--cov-mode", 0); P.seqIdMode = (int) iflag(a, "--seq-id-mode", 0); P.alnLenThr = (int) iflag(a, "--min-aln-len", 0);
        P.wrapped = iflag(a, "--wrapped-scoring", 0) != 0;
        P.gapOpen = (int) nuclValue("--gap-open", 5); P.gapExtend = (int) nuclValue("--gap-extend", 2); P.zdrop = (int) iflag(a, "--zdrop", 40);
        P.maxAccept = (unsigned) iflag(a, "--max-accept", INT_MAX); P.maxReject = (unsigned) iflag(a, "--max-rejected", INT_MAX); P.maxSeqLen = (size_t) iflag(a, "--max-seq-len", 65535);
        rc = alignModule(a.pos[0], a.pos[1], a.pos[2], a.pos[3], P, &err);
    } else if (cmd == "clust") {
        need(3, "clust <i:sequenceDB> <i:resultDB> <o:clusterDB>"); checkFlags("clust", a, CLUST_FLAGS);
        rc = clustModule(a.pos[0], a.pos[1], a.pos[2], (int) iflag(a, "--cluster-mode", 0), &err);
    } else if (cmd == "createsubdb") {
        need(3, "createsubdb <i:subsetFile|DB> <i:DB> <o:DB>"); checkFlags("createsubdb", a, SUBDB_FLAGS);
        rc = createsubdbModule(a.pos[0], a.pos[1], a.pos[2], (int) iflag(a, "--subdb-mode", 0), &err);
    } else if (cmd == "filterdb") {
        need(2, "filterdb <i:resultDB> <o:resultDB> --filter-file <file>"); checkFlags("filterdb", a, FILTER_FLAGS);
        if (!a.flag.count("--filter-file")) unsupported("filterdb: only the --filter-file mode is implemented on the MI355X path");
        rc = filterdbModule(a.pos[0], a.pos[1], a.flag["--filter-file"], &err);
    } else if (cmd == "mergeclusters") {
        need(3, "mergeclusters <i:sequenceDB> <o:clusterDB> <i:clusterDB1> ... <i:clusterDBn>"); checkFlags("mergeclusters", a, PLAIN_FLAGS);
        rc = mergeclustersModule(a.pos[0], a.pos[1], std::vector<std::string>(a.pos.begin() + 2, a.pos.end()), &err);
    } else if (cmd == "result2repseq") {
        need(3, "result2repseq <i:sequenceDB> <i:resultDB> <o:sequenceDB>"); checkFlags("result2repseq", a, PLAIN_FLAGS);
        rc = result2repseqModule(a.pos[0], a.pos[1], a.pos[2], &err);
    } else if (cmd == "rmdb") {
        need(1, "rmdb <i:DB>"); checkFlags("rmdb", a, PLAIN_FLAGS);
        rc = rmdbModule(a.pos[0]);
    } else {
        need(2, "mvdb <i:srcDB> <o:dstDB>"); checkFlags("mvdb", a, PLAIN_FLAGS);
        rc = mvdbModule(a.pos[0], a.pos[1], &err);
    }
    if (rc == 77) unsupported(err);
    if (rc) die(err);
    return EXIT_SUCCESS;
}

bool readsRefused(const FastqReads &r1, const FastqReads &r2, size_t n) {
    // a quality byte >= 0x80: the reference's SSE and scalar paths take different minima for it (combine_reads.cpp:120-245)
    bool bad = false;
#pragma omp parallel for reduction(|| : bad) schedule(dynamic, 65536)
    for (size_t i = 0; i < n; i++) {
        const char *q1 = r1.qual.data() + r1.off[i], *q2 = r2.qual.data() + r2.off[i];
        bool b = false;
        for (uint32_t j = 0; j < r1.len[i]; j++) b |= (q1[j] & 0x80) != 0;
        for (uint32_t j = 0; j < r2.len[i]; j++) b |= (q2[j] & 0x80) != 0;
        bad = bad || b;
    }
    return bad;
}
// the read pairs of mergereads' file pairs (files[2f], files[2f + 1]): both files of a pair parsed at once, pairs[f] = the records taken in
// lockstep; every pair checked in input order as mergereads.cpp:62-70 checks it, then the refusal above - all before anything is written
// or the device is opened.  Returns the number of pairs.
size_t readPairs(const char *module, const std::vector<std::string> &files, std::vector<FastqReads> &r, std::vector<size_t> &pairs) {
    std::string err;
    r.clear(); r.resize(files.size()); pairs.assign(files.size() / 2, 0);
    size_t total = 0;
    for (size_t f = 0; f < pairs.size(); f++) {
        if (!readFastqPair(files[2 * f], files[2 * f + 1], r[2 * f], r[2 * f + 1], &err)) die(err);
        const FastqReads &r1 = r[2 * f], &r2 = r[2 * f + 1];
        pairs[f] = std::min(r1.len.size(), r2.len.size());
        for (size_t i = 0; i < pairs[f]; i++) {
            if (r1.len[i] == 0 || r2.len[i] == 0) die("Invalid sequence record found");
            if (!r1.hasQual[i] || !r2.hasQual[i]) die("Invalid quality record found");
        }
        total += pairs[f];
    }
    for (size_t f = 0; f < pairs.size(); f++)
        if (readsRefused(r[2 * f], r[2 * f + 1], pairs[f])) unsupported(std::string(module) + ": a quality byte >= 0x80 in " + files[2 * f] + " / " + files[2 * f + 1] +
                                                                       " is not supported by the MI355X path (not FASTQ; the reference's SSE and scalar paths disagree on it)");
    return total;
}

// the workflow's own flags for the reads loop (src/commons/LocalParameters.h:283-318) on top of the stage lists
const char *const LOOP_FLAGS[] = {"--k-ancient-reads", "--kmer-per-seq-ancient", "--kmer-per-seq-scale-ancient", "--hash-shift", "--include-only-extendable-ancient-reads",
                                  "-e", "--num-iter-reads-only", "--shuffle", "--num-iterations", "--k-ancient-contigs", "--include-only-extendable-ancient-contigs",
                                  "--cycle-check", "--chop-cycle", "--gpus", NULL};
// What the loop leaves behind: the context, the final DB (the circular contigs not in it) and the circular contigs set aside - on the
// host (`cyclic`), or, for a caller that goes on with them on the device (keepResident), as the device DBs of the iterations that found
// them (`cyclicDev`) together with the keys and lengths of the DB the loop started from (`source`: the createdb / mergereads result,
// without its letters - cdm_seqdb_index_copy).
// keepReads (ancient_assemble_fused --damage-report / --depth-report): the DB the loop started from stays resident WITH its letters (`reads`) instead of
// going with the first iteration.
struct LoopEnd { cdm_ctx *ctx = NULL; cdm_seqdb *db = NULL, *source = NULL, *reads = NULL; bool keepReads = false; OutChunk cyclic; std::vector<cdm_seqdb *> cyclicDev; int dbtype = 1; };
// The loop itself, shared by ancient_reads_loop and ancient_assemble_fused: input parsing or pair merging, the read and contig
// iterations, the script's cyclecheck step and --gpus.  inputs: a sequence DB (fromDb), one reads file, or R1 R2 [R1 R2 ...];
// defaultTotal: --num-iterations where the flag is not given (< 0: the read iterations only).
void runLoop(const char *module, Args &a, const std::vector<std::string> &inputs, bool fromDb, long defaultTotal, bool keepResident, LoopEnd &E, Laps &laps) {
    const std::string mod = module;
    // the contig iterations' buffers grow ~1.5x per iteration: head room in the device-memory cache lets them fit the previous iteration's blocks
    cdm_pool_headroom(getenv("CDM_POOL_HEADROOM") ? (float) atof(getenv("CDM_POOL_HEADROOM")) : 1.6f);
    // input: a sequence DB, or - when there is no <input>.index - FASTA/FASTQ[.gz] reads, parsed and laid out as createdb would
    // (createdb.cpp:150-280, --shuffle 1 by default) and uploaded without a DB on disk in between; three or more positional arguments
    // without an index are paired-end reads R1 R2 [R1 R2 ...] OUT, merged on the device into the DB the loop runs on, with the keys,
    // the order and the wasExtended flags mergereads writes (the workflow's paired-end way in, guidedNuclAssemble.sh:28-32, where
    // --shuffle has no effect either)
    MmDb seq; std::string err;
    int &dbtype = E.dbtype;
    cdm_ctx *&ctx = E.ctx; cdm_seqdb *&db = E.db;
    FastxDb fx;
    const bool paired = !fromDb && inputs.size() >= 2;
    std::vector<FastqReads> pr; std::vector<size_t> prPairs;
    if (paired) {
        const std::vector<std::string> &files = inputs;
        if (files.size() % 2) die(mod + ": " + std::to_string(files.size()) + " read files given: paired-end input takes R1 R2 [R1 R2 ...]");
        // (refused here, before the reads are parsed: each rank would need the merged DB uploaded on its own)
        if (iflag(a, "--gpus", 1) > 1) unsupported(mod + ": --gpus > 1 with paired-end input is not supported by the MI355X path (merge the pairs with mergereads first)");
    }
    auto uploadTo = [&](cdm_ctx *c) -> cdm_seqdb * {       // (the same host copy serves every rank of a --gpus N run)
        if (fromDb) return uploadSeqDb(c, seq);
        cdm_seqdb *d = NULL;
        check(cdm_seqdb_upload(c, fx.blob.data(), fx.off.data(), fx.len.data(), fx.key.data(), NULL, fx.key.size(), &d), "Can not load the reads");
        return d;
    };
    if (fromDb) {
        if (!seq.load(inputs[0], &err)) die(err);
        dbtype = seq.dbtype;
        laps.lap("DB files mapped");
    } else if (paired) {
        if (readPairs(module, inputs, pr, prPairs) == 0) die(mod + ": the read files hold no pair");
        laps.lap("reads files parsed");
    } else {
        if (!readFastxAsDb(std::vector<std::string>(1, inputs[0]), iflag(a, "--shuffle", 1) != 0, fx, &err)) die(err);
        for (auto &l : fx.len) l -= 2;
        laps.lap("reads file parsed");
    }
    ctx = openCtx(); laps.lap("device context");
    if (paired) {
        // one batch: the DB has to be resident anyway.  More than one file pair: their reads side by side in one pair of blobs first.
        FastqReads c1, c2;
        const FastqReads *r1 = &pr[0], *r2 = &pr[1];
        if (prPairs.size() > 1) {
            auto join = [&](FastqReads &dst, int side) {
                size_t bytes = 0, m = 0;
                for (size_t f = 0; f < prPairs.size(); f++) { bytes += pr[2 * f + side].seq.size(); m += prPairs[f]; }
                dst.seq.resize(bytes); dst.qual.resize(bytes); dst.off.reserve(m); dst.len.reserve(m);
                size_t at = 0;
                for (size_t f = 0; f < prPairs.size(); f++) {
                    const FastqReads &s = pr[2 * f + side];
                    memcpy(dst.seq.data() + at, s.seq.data(), s.seq.size()); memcpy(dst.qual.data() + at, s.qual.data(), std::min(s.qual.size(), s.seq.size()));
                    for (size_t i = 0; i < prPairs[f]; i++) { dst.off.push_back(at + s.off[i]); dst.len.push_back(s.len[i]); }
                    at += s.seq.size();
                }
            };
            join(c1, 0); join(c2, 1);
            r1 = &c1; r2 = &c2;
        }
        cdm_pairs *h = NULL;
        check(cdm_pairs_merge(ctx, r1->seq.data(), r1->qual.data(), r1->off.data(), r1->len.data(), r2->seq.data(), r2->qual.data(), r2->off.data(), r2->len.data(),
                              std::accumulate(prPairs.begin(), prPairs.end(), (size_t) 0), NULL, &h), "mergereads");
        check(cdm_pairs_to_seqdb(ctx, h, 0, &db), "mergereads");
        cdm_pairs_free(h);
        laps.lap("pairs merged into the DB");
    } else { db = uploadTo(ctx); laps.lap("sequences up"); }
    check(cdm_damage_load(ctx, a.flag.count("--ancient-damage") ? a.flag["--ancient-damage"].c_str() : ""), "Profile not 12 fields");
    // (the selection of the assembled contigs compares with the lengths of this DB: its keys and lengths stay, its letters go with the first iteration)
    if (keepResident) check(cdm_seqdb_index_copy(ctx, db, &E.source), "index of the source DB");
    cdm_seqdb *const firstDb = db;
    auto releaseInput = [&](cdm_seqdb *d) { if (d == firstDb && E.keepReads && !E.reads) E.reads = d; else cdm_seqdb_free(d); };      // an iteration's input DB once its result stands
    cdm_kmer_params kp;
    kp.kmer_size = (int) iflag(a, "--k-ancient-reads", 20); kp.kmers_per_seq = (int) iflag(a, "--kmer-per-seq-ancient", 200);
    kp.kmers_per_seq_scale = fflag(a, "--kmer-per-seq-scale-ancient", 0.2f); kp.hash_shift = (uint64_t) iflag(a, "--hash-shift", 67);
    kp.ignore_multi_kmer = 1; kp.include_only_extendable = (int) iflag(a, "--include-only-extendable-ancient-reads", 0); kp.cov_mode = 1; kp.cov_thr = 0.0f;
    cdm_rescore_params rp;
    rp.seq_id_thr = fflag(a, "--min-seq-id", 0.9f); rp.eval_thr = dflag(a, "-e", 0.001);
    rp.cov_mode = 1; rp.cov_thr = 0.0f; rp.seq_id_mode = 0; rp.min_aln_len = 0;
    cdm_ancient_params ap = ancientParams(a);
    if (!a.flag.count("--max-seq-len")) ap.max_seq_len = 200000;   // setGuidedNuclAssemblerWorkflowDefaults (GuidedNuclassembler.cpp:29)
    const long iters = iflag(a, "--num-iter-reads-only", 5);       // LocalParameters.h:304
    // --num-iterations N > --num-iter-reads-only M: the contig phase of the workflow loop (data/nuclassemble.sh:148-196) for the
    // remaining N - M iterations - kmermatcher with the contig parameters (Nuclassembler.cpp:118-126), rescorediagonal,
    // ancient_correction, ancient_contig_merge, and the script's cyclecheck() (:19-60; --cycle-check / --chop-cycle, both on by default
    // as setNuclAssemblerWorkflowDefaults has them): circular contigs leave the loop, cut at their split diagonal, and join the output
    // at the end (concatdbs, :204-212)
    const long total = std::max(iters, iflag(a, "--num-iterations", defaultTotal < 0 ? iters : defaultTotal));
    cdm_kmer_params kc = kp;
    kc.kmer_size = (int) iflag(a, "--k-ancient-contigs", 22); kc.include_only_extendable = (int) iflag(a, "--include-only-extendable-ancient-contigs", 1);
    const float mergeThr = fflag(a, "--min-merge-seq-id", 0.99f);
    // the workflow builds the contig phase's rescorediagonal / assembler parameter strings after `par.seqIdThr = par.corrContigSeqId`
    // (Nuclassembler.cpp:124-126): there --min-seq-id IS --min-seqid-corr-contigs (LocalParameters.h default 0.9)
    cdm_rescore_params rc = rp; cdm_ancient_params ac = ap;
    rc.seq_id_thr = ac.seq_id_thr = fflag(a, "--min-seqid-corr-contigs", 0.9f);
    const bool cycleCheck = iflag(a, "--cycle-check", 1) != 0, chopCycle = iflag(a, "--chop-cycle", 1) != 0;
    OutChunk &cyclic = E.cyclic;
    // the circular contigs an iteration set aside: to the host, or kept on the device for the caller
    auto setAside = [&](cdm_ctx *c, cdm_seqdb *cyc) {
        if (cdm_seqdb_size(cyc)) fprintf(stderr, "         %llu circular contigs set aside\n", (unsigned long long) cdm_seqdb_size(cyc));
        if (keepResident && cdm_seqdb_size(cyc)) { E.cyclicDev.push_back(cyc); return; }
        appendEntries(c, cyc, cyclic);
        cdm_seqdb_free(cyc);
    };
    // --gpus N: the read iterations over N ranks = N host threads of this process, a device each; every rank holds the whole DB and
    // the library splits the work (cdm_reads_iteration_dist: kmermatcher by k-mer range, one all-to-all of group keys, the other stages
    // on the owned queries, the new DBs all-gathered - the single-device result), the contig iterations likewise since round 5
    // (cdm_contig_iteration_dist: ancient_contig_merge's queue runs on the device, on the owned queries), the script's cyclecheck step on
    // every rank.  This thread is rank 0.
    const int gpus = (int) std::max<long>(1, iflag(a, "--gpus", 1));
    long firstLocal = 0;
    if (gpus > 1 || getenv("CDM_LOOP_FORCE_COMM")) {
        const char *tr = getenv("CDM_LOOP_TRANSPORT");
        const bool threadsTransport = tr && !strcmp(tr, "threads");
        // CDM_LOOP_TRANSPORT=standin (tests): the library's RCCL transport over its in-process stand-in for RCCL's calls - the ranks share
        // device 0, as with "threads", but what runs is the transport a deployment runs
        void *standin = (tr && !strcmp(tr, "standin")) ? cdm_comm_standin_group(gpus) : NULL;
        const bool oneDevice = threadsTransport || standin;
        unsigned char uid[128];
        if (!oneDevice) check(cdm_comm_unique_id(uid), "RCCL");
        ThreadTransport tt(gpus);
        const std::string damage = a.flag.count("--ancient-damage") ? a.flag["--ancient-damage"] : "";
        auto rankBody = [&](int r, cdm_ctx *c, cdm_seqdb *&d) {
            ThreadRank me{&tt, r, c};
            cdm_comm *cm = NULL;
            if (threadsTransport) { cdm_comm_ops ops{&me, ttAllGatherHost, ttAllToAllDev, ttAllGatherDev}; check(cdm_comm_create_ops(c, r, gpus, &ops, &cm), "communicator"); }
            else if (standin) check(cdm_comm_create_standin(c, standin, r, &cm), "communicator");
            else check(cdm_comm_create_rccl(c, r, gpus, uid, &cm), "RCCL communicator");
            for (long it = 0; it < total && cdm_seqdb_size(d) > 0; it++) {
                cdm_alns *alns = NULL; cdm_seqdb *next = NULL;
                const bool contigs = it >= iters;
                const auto tIt = std::chrono::steady_clock::now();
                if (contigs) check(cdm_contig_iteration_dist(c, cm, d, &kc, &rc, &ac, mergeThr, &alns, NULL, &next), "contig iteration over the ranks");
                else check(cdm_reads_iteration_dist(c, cm, d, &kp, &rp, &ap, NULL, &alns, NULL, &next), "reads iteration over the ranks");
                if (r == 0) fprintf(stderr, "STEP: %ld  sequences %llu  residues %llu -> %llu  alignments of rank 0's queries %llu  (%.3f s on %d ranks%s)\n",
                                    it, (unsigned long long) cdm_seqdb_size(d), (unsigned long long) cdm_seqdb_residues(d), (unsigned long long) cdm_seqdb_residues(next),
                                    (unsigned long long) cdm_alns_count(alns), std::chrono::duration<double>(std::chrono::steady_clock::now() - tIt).count(), gpus,
                                    threadsTransport ? ", in-process transport on one device" : standin ? ", the RCCL transport over its in-process stand-in, one device" : ", RCCL");
                cdm_alns_free(alns); releaseInput(d);
                d = next;
                if (contigs && cycleCheck) {        // every rank holds the whole merged DB: the same check, the same rest on all of them; rank 0 keeps the circular contigs
                    cdm_seqdb *cyc = NULL, *rest = NULL;
                    check(cdm_cyclecheck(c, d, (uint32_t) std::min<uint64_t>(ap.max_seq_len, 0xFFFFFFFFull), chopCycle, &cyc, &rest, NULL), "cyclecheck");
                    if (r == 0) setAside(c, cyc); else cdm_seqdb_free(cyc);
                    cdm_seqdb_free(d);
                    d = rest;
                }
            }
            cdm_comm_free(cm);
        };
        std::vector<std::thread> helpers;
        for (int r = 1; r < gpus; r++) helpers.emplace_back([&, r] {
            cdm_ctx *c = openCtx(oneDevice ? 0 : r);
            check(cdm_damage_load(c, damage.c_str()), "Profile not 12 fields");
            cdm_seqdb *d = uploadTo(c);
            rankBody(r, c, d);
            cdm_seqdb_free(d); cdm_ctx_destroy(c);
        });
        rankBody(0, ctx, db);
        for (auto &h : helpers) h.join();
        firstLocal = total;
    }
    for (long it = firstLocal; it < total && cdm_seqdb_size(db) > 0; it++) {
        cdm_hits *hits = NULL; cdm_alns *alns = NULL; cdm_seqdb *corr = NULL, *next = NULL;
        const bool contigs = it >= iters;
        const auto tIt = std::chrono::steady_clock::now();
        check(cdm_kmermatch(ctx, db, contigs ? &kc : &kp, &hits), "kmermatcher");
        check(cdm_rescore(ctx, db, hits, contigs ? &rc : &rp, &alns), "rescorediagonal");
        cdm_hits_free(hits);
        check(cdm_correct(ctx, db, alns, contigs ? &ac : &ap, &corr), "ancient_correction");
        if (contigs) check(cdm_contig_merge(ctx, corr, alns, &ac, mergeThr, &next), "ancient_contig_merge");
        else check(cdm_extend(ctx, corr, alns, &ap, &next, NULL), "ancient_read_assemble");
        fprintf(stderr, "STEP: %ld  sequences %llu  residues %llu -> %llu  alignments %llu  (%.3f s; device stages: kmermatcher %.0f, rescorediagonal %.0f, ancient_correction %.0f, %s %.0f ms)\n",
                it, (unsigned long long) cdm_seqdb_size(db), (unsigned long long) cdm_seqdb_residues(db), (unsigned long long) cdm_seqdb_residues(next), (unsigned long long) cdm_alns_count(alns),
                std::chrono::duration<double>(std::chrono::steady_clock::now() - tIt).count(), cdm_ctx_last_kernel_ms(ctx, 8), cdm_ctx_last_kernel_ms(ctx, 9), cdm_ctx_last_kernel_ms(ctx, 10),
                contigs ? "contig statistics" : "ancient_read_assemble", cdm_ctx_last_kernel_ms(ctx, contigs ? 12 : 11));
        cdm_alns_free(alns); cdm_seqdb_free(corr); releaseInput(db);
        db = next;
        if (contigs && cycleCheck) {
            cdm_seqdb *cyc = NULL, *rest = NULL;
            check(cdm_cyclecheck(ctx, db, (uint32_t) std::min<uint64_t>(ap.max_seq_len, 0xFFFFFFFFull), chopCycle, &cyc, &rest, NULL), "cyclecheck");
            setAside(ctx, cyc);
            cdm_seqdb_free(db);
            db = rest;
        }
    }
    laps.lap("iterations");
}
// concatdbs --preserve-keys of two sets of entries (the linear and the circular contigs), in key order
void concatByKey(const OutChunk &all, const OutChunk &cyclic, OutChunk &merged) {
    std::vector<std::pair<uint32_t, std::pair<const OutChunk *, size_t>>> order;
    std::vector<size_t> offA(all.key.size() + 1, 0), offC(cyclic.key.size() + 1, 0);
    for (size_t i = 0; i < all.key.size(); i++) { offA[i + 1] = offA[i] + all.len[i]; order.push_back({all.key[i], {&all, i}}); }
    for (size_t i = 0; i < cyclic.key.size(); i++) { offC[i + 1] = offC[i] + cyclic.len[i]; order.push_back({cyclic.key[i], {&cyclic, i}}); }
    std::stable_sort(order.begin(), order.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
    for (const auto &o : order) {
        const OutChunk &c = *o.second.first; const size_t i = o.second.second;
        merged.add(o.first, c.data.data() + (&c == &all ? offA[i] : offC[i]), c.len[i] - 1, c.ext[i]);
    }
}
int readsLoop(Args &a) {
    if (a.pos.size() < 2) die("Usage: carpedeam ancient_reads_loop <i:sequenceDB|reads[.gz]|R1 R2 [R1 R2 ...]> <o:sequenceDB> --ancient-damage <prefix> [--num-iter-reads-only N]");
    checkFlags("ancient_reads_loop", a, ANCIENT_FLAGS, LOOP_FLAGS);
    struct stat st;
    Laps laps;
    const bool fromDb = stat((a.pos[0] + ".index").c_str(), &st) == 0;
    const bool paired = !fromDb && a.pos.size() >= 3;
    const std::string outPath = paired ? a.pos.back() : a.pos[1];
    LoopEnd E;
    runLoop("ancient_reads_loop", a, paired ? std::vector<std::string>(a.pos.begin(), a.pos.end() - 1) : std::vector<std::string>(1, a.pos[0]), fromDb, -1, false, E, laps);
    std::string err;
    if (E.cyclic.key.empty()) { writeSeqDb(E.ctx, E.db, outPath, E.dbtype); laps.lap("sequences down, DB written"); }
    else {   // concatdbs --preserve-keys of the linear and the circular contigs, written in key order
        OutChunk all; appendEntries(E.ctx, E.db, all);
        std::vector<OutChunk> merged(1);
        concatByKey(all, E.cyclic, merged[0]);
        if (!mmdbWriteChunks(outPath, E.dbtype, merged, &err)) die(err);
    }
    cdm_seqdb_free(E.db); cdm_ctx_destroy(E.ctx);
    return EXIT_SUCCESS;
}
}  // namespace

namespace {
const FlagSpec CREATEDB_FLAGS[] = {   // Parameters.cpp:733-737 createdb
    {"--shuffle", 'U', 0, 0}, {"--dbtype", 'U', 0, 0}, {"--createdb-mode", 'V', "0", "only the copying mode"},
    {"--write-lookup", 'V', "1", "the .lookup file is always written"}, {"--id-offset", 'V', "0", "not implemented"}, {"--compressed", 'V', "0", "compressed DBs are not implemented"},
    {"-v", 'N', 0, 0}, {"--threads", 'N', 0, 0}, {0, 0, 0, 0}};
const FlagSpec PLAIN_FLAGS[] = {{"-v", 'N', 0, 0}, {"--threads", 'N', 0, 0}, {"--compressed", 'V', "0", "compressed DBs are not implemented"}, {"--use-fasta-header", 'V', "0", "not implemented"}, {0, 0, 0, 0}};
// The side-car of a sequence DB straight from its text, on the host (createdb has no device): the letters packed as cdm_seqdb_upload
// packs them (seqdb.hip k_pack: A, C, G, T = 0..3, 16 per word, every sequence on a word boundary; 'N' = code 0 + a bit of the N mask).
// Only for DBs of upper-case ACGTN - any other letter takes the device's mapping and its raw plane (the first module that uploads the
// DB then writes the side-car).
void seqSideFromText(const std::string &path) {
    if (!sideEnabled()) return;
    MmDb db; std::string err;
    if (!db.load(path, &err) || (db.dbtype & 0x7FFFFFFF) != 1 || db.size() == 0) return;
    const size_t n = db.size();
    HVec<uint32_t> lens(n), woff(n + 1); HVec<uint8_t> ext(n), flags(n);
    woff[0] = 0;
    for (size_t i = 0; i < n; i++) { lens[i] = db.len[i] >= 2 ? (uint32_t) (db.len[i] - 2) : 0; ext[i] = db.ext[i]; const uint64_t w = (uint64_t) woff[i] + (lens[i] + 15) / 16; if (w > 0xFFFFFFFFull) return; woff[i + 1] = (uint32_t) w; }
    const uint64_t words = woff[n];
    HVec<uint32_t> codes(words + 1); HVec<uint16_t> mask(words + 1);
    bool other = false, anyN = false;
#pragma omp parallel for reduction(|| : other, anyN) schedule(dynamic, 4096)
    for (size_t i = 0; i < n; i++) {
        const char *sq = db.entry(i);
        const uint32_t L = lens[i];
        uint8_t fl = 0;
        for (uint32_t w = 0; w * 16 < L; w++) {
            uint32_t code = 0, nb = 0;
            const uint32_t cnt = std::min(16u, L - w * 16);
            for (uint32_t j = 0; j < cnt; j++) {
                uint32_t v = 0;
                switch (sq[w * 16 + j]) { case 'A': v = 0; break; case 'C': v = 1; break; case 'G': v = 2; break; case 'T': v = 3; break; case 'N': nb |= 1u << j; break; default: other = true; }
                code |= v << (2 * j);
            }
            codes[woff[i] + w] = code; mask[woff[i] + w] = (uint16_t) nb;
            if (nb) fl = 1;
        }
        flags[i] = fl; anyN = anyN || fl;
    }
    if (other) return;
    const SidePiece pc[7] = {{db.key.data(), n * 4}, {lens.data(), n * 4}, {ext.data(), n}, {flags.data(), n}, {codes.data(), words * 4}, {mask.data(), anyN ? words * 2 : 0}, {NULL, 0}};
    sideWrite(path, SIDE_SEQ, anyN ? SIDE_F_HAS_NMASK : 0, n, words, 0, 0, db.dbtype, pc, 7);
}
int createdb(Args &a) {
    if (a.pos.size() < 2) die("Usage: carpedeam createdb <i:fastaFile1[.gz]> ... <i:fastaFileN[.gz]> <o:sequenceDB>");
    checkFlags("createdb", a, CREATEDB_FLAGS);
    std::vector<std::string> files(a.pos.begin(), a.pos.end() - 1);
    std::string err;
    const long dbType = iflag(a, "--dbtype", 0);        // 0 = guess from the first entries, as createdb does (createdb.cpp:40-45)
    if (dbType != 0 && dbType != 2) unsupported("createdb: --dbtype " + std::to_string(dbType) + " is not supported by the MI355X path (nucleotide sequences only; accepted: 0, 2)");
    if (createdbModule(files, a.pos.back(), iflag(a, "--shuffle", 1) != 0, (int) dbType, &err)) die(err);
    seqSideFromText(a.pos.back());
    return EXIT_SUCCESS;
}
int convert2fasta(Args &a) {
    if (a.pos.size() < 2) die("Usage: carpedeam convert2fasta <i:sequenceDB> <o:fastaFile>");
    checkFlags("convert2fasta", a, PLAIN_FLAGS);
    std::string err;
    if (convert2fastaModule(a.pos[0], a.pos[1], &err)) die(err);
    return EXIT_SUCCESS;
}
// ---- mergereads (src/assembler/mergereads.cpp): paired-end reads merged with FLASH's combine_reads (lib/flash) on the device
// (csrc/pairmerge.hip, cdm_pairs_merge).  File pair i is (files[2i], files[2i + 1]).  The reference counts the output among its file
// names (mergereads.cpp:38-48), so with an odd number of inputs its last pair is (last input, output DB): refused here with the
// reference's message for the usual case, an output that is not there yet.  The records of a pair's files are taken in lockstep until
// either file ends.  Entries: a combined pair gives its consensus under R1's
// name, any other pair R1 and the reverse-complemented R2 under their names; keys 0, 1, ... in input order; "SEQ\n\0" / "name\n\0";
// every entry wasExtended = 1 (DBWriter::writeEnd(id, 0, true), DBWriter.h:30); no .lookup, no .source.
//   CDM_MERGE_BATCH=<pairs>: pairs per device batch (default: 8 M pairs, or fewer so that a batch holds at most 2 GB of read bytes)
static int pieceSink(void *user, const char *data, uint64_t offset, uint64_t bytes) {
    const std::pair<int, uint64_t> &f = *(const std::pair<int, uint64_t> *) user;
    return mmdbWritePiece(f.first, data, f.second + offset, bytes) ? 0 : 1;
}
int mergereads(Args &a) {
    static const FlagSpec MERGEREADS_FLAGS[] = {{"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0}, {0, 0, 0, 0}};     // LocalParameters onlythreads
    checkFlags("mergereads", a, MERGEREADS_FLAGS);
    if (a.pos.size() < 2) die("Usage: carpedeam mergereads <i:fastqFile1_R1[.gz]> <i:fastqFile1_R2[.gz]> ... <o:sequenceDB>");
    const std::string outPath = a.pos.back();
    std::vector<std::string> files(a.pos.begin(), a.pos.end() - 1);
    if (files.size() % 2) {
        struct stat st;
        if (stat(outPath.c_str(), &st) != 0) die(outPath + ": No such file or directory");      // what the reference says opening it as the last R2
        // the output exists: the reference reads it as the last pair's R2 while it writes it anew - not reproduced
        unsupported("mergereads: an odd number of input files (" + std::to_string(files.size()) + ") with an existing output DB is not supported by the MI355X path "
                    "(the reference would read " + outPath + " as the last R2)");
    }
    Laps laps;
    std::string err;
    std::vector<FastqReads> r; std::vector<size_t> pairs;
    const size_t total = readPairs("mergereads", files, r, pairs);
    laps.lap("reads files parsed");
    cdm_ctx *ctx = total ? openCtx() : NULL;
    if (ctx) laps.lap("device context");
    const int dataFd = open(outPath.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
    if (dataFd < 0) die("Could not open " + outPath + " for writing");
    HVec<uint64_t> eOff; HVec<uint32_t> eLen, hLen; HVec<uint64_t> hOff; HVec<char> hBlob;
    eOff.reserve(2 * total + 1); eLen.reserve(2 * total + 1); hOff.reserve(2 * total + 1); hLen.reserve(2 * total + 1);
    uint64_t textAt = 0;
    const long batchEnv = getenv("CDM_MERGE_BATCH") ? atol(getenv("CDM_MERGE_BATCH")) : 0;
    double devMs = 0;
    std::vector<uint8_t> status; std::vector<uint32_t> elen;
    for (size_t f = 0; f < pairs.size(); f++) {
        const FastqReads &r1 = r[2 * f], &r2 = r[2 * f + 1];
        for (size_t lo = 0; lo < pairs[f];) {
            size_t hi = lo, bytes = 0;
            const size_t maxPairs = batchEnv > 0 ? (size_t) batchEnv : (size_t) 8 << 20;
            while (hi < pairs[f] && hi - lo < maxPairs && (batchEnv > 0 || hi == lo || bytes + r1.len[hi] + r2.len[hi] <= ((size_t) 2 << 30))) { bytes += r1.len[hi] + r2.len[hi]; hi++; }
            const size_t m = hi - lo;
            cdm_pairs *h = NULL;
            check(cdm_pairs_merge(ctx, r1.seq.data(), r1.qual.data(), r1.off.data() + lo, r1.len.data() + lo, r2.seq.data(), r2.qual.data(), r2.off.data() + lo,
                                  r2.len.data() + lo, m, NULL, &h), "mergereads");
            devMs += cdm_pairs_kernel_ms(h);
            const uint64_t ents = cdm_pairs_entries(h);
            status.resize(m); elen.resize(ents);
            check(cdm_pairs_download(ctx, h, status.data(), NULL, NULL, elen.data()), "mergereads: download");
            std::pair<int, uint64_t> sinkAt(dataFd, textAt);
            check(cdm_pairs_download_stream(ctx, h, 64u << 20, pieceSink, &sinkAt), "mergereads: download");
            cdm_pairs_free(h);
            // the index columns of the sequence DB and the header entries: R1's name for a combined pair, R1's and R2's names otherwise
            size_t e = 0;
            auto name = [&](const FastqReads &rr, size_t i) {
                const char *p = rr.hdr.data() + rr.hoff[i];
                size_t k = 0; while (p[k] != ' ' && p[k] != '\n') k++;         // the stored header is "name[ comment]\n"
                hOff.push_back(hBlob.size()); hLen.push_back((uint32_t) k + 2);
                if (hBlob.capacity() - hBlob.size() < k + 2) hBlob.reserve(std::max(hBlob.capacity() * 2, hBlob.size() + k + 2 + (16u << 20)));
                hBlob.insert(hBlob.end(), p, p + k); hBlob.push_back('\n'); hBlob.push_back('\0');
            };
            for (size_t i = 0; i < m; i++) {
                name(r1, lo + i);
                if (!status[i]) name(r2, lo + i);
                for (int k = status[i] ? 1 : 2; k > 0; k--, e++) { eOff.push_back(textAt); eLen.push_back(elen[e] + 2); textAt += elen[e] + 2; }
            }
            lo = hi;
        }
    }
    if (ctx) laps.lap("pairs merged on the device, text written");
    if (close(dataFd) != 0) die("Could not write " + outPath);
    const size_t n = eOff.size();
    HVec<uint32_t> keys(n); HVec<uint8_t> ext(n);
    for (size_t i = 0; i < n; i++) { keys[i] = (uint32_t) i; ext[i] = 1; }
    if (!mmdbWriteBlob(outPath, 1, NULL, 0, keys.data(), eOff.data(), eLen.data(), ext.data(), n, &err, MMDB_DATA_ELSEWHERE)) die(err);
    if (!mmdbWriteBlob(outPath + "_h", 12, n ? hBlob.data() : "", hBlob.size(), keys.data(), hOff.data(), hLen.data(), ext.data(), n, &err)) die(err);
    laps.lap("index and header DB written");
    seqSideFromText(outPath);
    if (getenv("CDM_TIMING")) fprintf(stderr, "  %llu pairs -> %llu entries; merge kernels %.3f ms on the device\n", (unsigned long long) total, (unsigned long long) n, devMs);
    if (ctx) cdm_ctx_destroy(ctx);
    return EXIT_SUCCESS;
}
int createhdb(Args &a) {
    if (a.pos.size() < 2) die("Usage: carpedeam createhdb <i:sequenceDB> [<i:sequenceDBcycle>] <o:headerDB>");
    checkFlags("createhdb", a, PLAIN_FLAGS);
    std::string err;
    if (createhdbModule(a.pos[0], a.pos.size() > 2 ? a.pos[1] : "", a.pos.back(), &err)) die(err);
    return EXIT_SUCCESS;
}

// ---- ancient_assemble_fused: reads to contig FASTA in this one process.  `ancient_assemble` of the reference
// (src/workflow/GuidedNuclassembler.cpp) is three drivers that write shell scripts and start some hundred module processes; here the
// loop above runs first, then - on the DBs it left resident - the two selections of data/nuclassemble.sh:214-233
// (cdm_seqdb_select_assembled), and on the selected contigs what data/guidedNuclAssemble.sh:180-218 runs: linclust
// (lib/mmseqs/data/workflow/linclust.sh with CLUSTER_PAR, GuidedNuclassembler.cpp:33-40,176-181), result2repseq, createhdb, convert2fasta.
// Only the selected contigs leave the device; the final DB of the loop is never written.  No script, no other process: the steps of the
// tail are the module functions of this binary, each called with the parameter string the reference's drivers build for it (recorded
// from the reference in tests/golden/fused/calls_*.json; tests/test_fused_cli.py compares) and read through the module's own flag table.
// Not a module of the reference: `ancient_assemble` itself stays with the reference binary (host/front.c).
//   CDM_FUSED_DRY_RUN=1 | cycle: the steps of the tail and their parameter strings on stdout, nothing run (paths under $TMP)
#define FUSED_REFUSED(name) {name, 'R', 0, "a flag of the reference's ancient_assemble that ancient_assemble_fused does not take"}
const FlagSpec FUSED_FLAGS[] = {
    // the loop's (ANCIENT_FLAGS + LOOP_FLAGS)
    {"--min-seq-id", 'U', 0, 0}, {"--max-seq-len", 'U', 0, 0}, {"--ext-random-align", 'U', 0, 0}, {"--excess-penalty", 'U', 0, 0}, {"--min-ryseq-id-corr-reads", 'U', 0, 0},
    {"--likelihood-ratio-threshold", 'U', 0, 0}, {"--ancient-damage", 'U', 0, 0}, {"--unsafe", 'U', 0, 0}, {"--min-cov-safe", 'U', 0, 0}, {"--min-merge-seq-id", 'U', 0, 0},
    {"--keep-target", 'N', 0, "not read by the modules of the loop"}, {"--min-seqid-corr-reads", 'N', 0, "not read by the modules of the loop"}, {"--min-seqid-corr-contigs", 'U', 0, 0},
    {"--rescore-mode", 'V', "3", "re-alignment of parked candidates is end-to-end ungapped (ancientReadsResults.cpp:502)"},
    {"--k-ancient-reads", 'U', 0, 0}, {"--kmer-per-seq-ancient", 'U', 0, 0}, {"--kmer-per-seq-scale-ancient", 'U', 0, 0}, {"--hash-shift", 'U', 0, 0},
    {"--include-only-extendable-ancient-reads", 'U', 0, 0}, {"-e", 'U', 0, 0}, {"--num-iter-reads-only", 'U', 0, 0}, {"--shuffle", 'U', 0, 0}, {"--num-iterations", 'U', 0, 0},
    {"--k-ancient-contigs", 'U', 0, 0}, {"--include-only-extendable-ancient-contigs", 'U', 0, 0}, {"--cycle-check", 'U', 0, 0}, {"--chop-cycle", 'U', 0, 0}, {"--gpus", 'U', 0, 0},
    // the tail's
    {"--damage-report", 'U', 0, 0}, {"--damage-ends", 'U', 0, 0}, {"--depth-report", 'U', 0, 0}, {"--depth-edge", 'U', 0, 0},
    {"--variant-report", 'U', 0, 0}, {"--variant-sites", 'U', 0, 0}, {"--min-depth", 'U', 0, 0}, {"--min-alt-count", 'U', 0, 0}, {"--min-alt-percent", 'U', 0, 0}, {"--mask-ends", 'U', 0, 0},
    {"--break-report", 'U', 0, 0}, {"--break-anchor", 'U', 0, 0}, {"--break-edge", 'U', 0, 0}, {"--min-span", 'U', 0, 0}, {"--min-span-percent", 'U', 0, 0},
    {"--min-contig-len", 'U', 0, 0}, {"--clust-min-seq-id", 'U', 0, 0}, {"--clust-min-cov", 'U', 0, 0}, {"--zdrop", 'U', 0, 0}, {"--threads", 'U', 0, 0}, {"--remove-tmp-files", 'U', 0, 0},
    {"-v", 'U', 0, 0},
    {"--cluster-mode", 'V', "2", "the redundancy reduction clusters greedily, linclust's mode for --cov-mode 1"}, {"--cov-mode", 'V', "1", "the workflow's coverage mode throughout"},
    {"--gap-open", 'V', "5", "gapped E-values are known for the costs 5 / 2 only"}, {"--gap-extend", 'V', "2", "gapped E-values are known for the costs 5 / 2 only"},
    {"-a", 'V', "0", "no backtrace output"}, {"--compressed", 'V', "0", "compressed DBs are not implemented"},
    // known to the reference's list (LocalParameters.h guidedNuclAssembleworkflow), not handled here
    FUSED_REFUSED("--alph-size"), FUSED_REFUSED("--spaced-kmer-mode"), FUSED_REFUSED("--spaced-kmer-pattern"), FUSED_REFUSED("--mask"), FUSED_REFUSED("--mask-lower-case"),
    FUSED_REFUSED("--split-memory-limit"), FUSED_REFUSED("--add-self-matches"), FUSED_REFUSED("--seq-id-mode"), FUSED_REFUSED("--min-aln-len"), FUSED_REFUSED("--kmer-per-seq"),
    FUSED_REFUSED("--kmer-per-seq-scale"), FUSED_REFUSED("--adjust-kmer-len"), FUSED_REFUSED("--include-only-extendable"), FUSED_REFUSED("--ignore-multi-kmer"), FUSED_REFUSED("-k"),
    FUSED_REFUSED("-c"), FUSED_REFUSED("--min-length"), FUSED_REFUSED("--max-length"), FUSED_REFUSED("--max-gaps"), FUSED_REFUSED("--contig-start-mode"), FUSED_REFUSED("--contig-end-mode"),
    FUSED_REFUSED("--orf-start-mode"), FUSED_REFUSED("--forward-frames"), FUSED_REFUSED("--reverse-frames"), FUSED_REFUSED("--translation-table"), FUSED_REFUSED("--translate"),
    FUSED_REFUSED("--use-all-table-starts"), FUSED_REFUSED("--id-offset"), FUSED_REFUSED("--dbtype"), FUSED_REFUSED("--createdb-mode"), FUSED_REFUSED("--contig-output-mode"),
    FUSED_REFUSED("--sub-mat"), FUSED_REFUSED("--db-load-mode"), FUSED_REFUSED("--delete-tmp-inc"), FUSED_REFUSED("--mpi-runner"), FUSED_REFUSED("--create-lookup"),
    FUSED_REFUSED("--write-lookup"), FUSED_REFUSED("--filter-hits"), FUSED_REFUSED("--sort-results"), FUSED_REFUSED("--wrapped-scoring"), FUSED_REFUSED("--db-mode"),
    FUSED_REFUSED("--min-ryseq-id"), {0, 0, 0, 0}};
// one module call of the tail: positional arguments and the parameter string
struct TailStep { std::string module; std::vector<std::string> pos; std::string flags; };
Args stepArgs(const TailStep &s) {
    Args a; a.pos = s.pos;
    std::vector<std::string> tok; size_t at = 0;
    while (at < s.flags.size()) { const size_t e = std::min(s.flags.find(' ', at), s.flags.size()); if (e > at) tok.push_back(s.flags.substr(at, e - at)); at = e + 1; }
    for (size_t i = 0; i + 1 < tok.size(); i += 2) a.flag[tok[i]] = tok[i + 1];      // (every flag of these strings takes a value)
    return a;
}
// the numbers as the reference's SSTR() prints them (an ostringstream's default notation: %g)
std::string asG(double v) { char b[40]; snprintf(b, sizeof(b), "%g", v); return b; }
// The tail as the reference runs it for these flags: linclust's own line first (the driver whose steps follow: listed, not run), then
// linclust.sh:24-87 and guidedNuclAssemble.sh:190-215.  T: the command's directory.
std::vector<TailStep> fusedTail(Args &a, const std::string &T, bool withCycle) {
    // linclust is started with CLUSTER_PAR alone (guidedNuclAssemble.sh:186), the `reduceredundancy` list (LocalParameters.h:193-209):
    // of the user's flags --clust-min-seq-id, --clust-min-cov, --max-seq-len, --zdrop, --threads and --remove-tmp-files reach it.  What
    // that list does not carry - -e, --hash-shift, -v - its modules get with linclust's own defaults (0.001, 67, 3), whatever the
    // user gave the workflow; the user's -v reaches result2repseq, createhdb and convert2fasta (THREADS_PAR, VERBOSITY_PAR).
    const std::string sid = asG(fflag(a, "--clust-min-seq-id", 0.97f)), cov = asG(fflag(a, "--clust-min-cov", 0.99f)), ev = "0.001", hashShift = "67", lv = "3";
    const std::string maxLen = std::to_string(iflag(a, "--max-seq-len", 200000)), zdrop = std::to_string(iflag(a, "--zdrop", 200));
    const std::string threads = std::to_string(std::max(1, omp_get_max_threads())), v = a.flag.count("-v") ? a.flag["-v"] : "3", rm = std::to_string(iflag(a, "--remove-tmp-files", 0));
    const std::string SUB = "--sub-mat nucl:nucleotide.out,aa:blosum62.out", TCV = "--threads " + threads + " --compressed 0 -v " + lv;
    const std::string IN = T + "/nuclassembly", C = T + "/clu_tmp", STEP = C + "/input_step_redundancy", REP = T + "/nuclassembly_rep";
    std::vector<TailStep> t;
    t.push_back({"linclust", {IN, T + "/clu", C}, "--alph-size nucl:5,aa:13 --cluster-mode 2 -k 20 --kmer-per-seq 200 --kmer-per-seq-scale 0.200 --ignore-multi-kmer 1 --min-seq-id " + sid +
                 " --cov-mode 1 -c " + cov + " --max-seq-len " + maxLen + " --wrapped-scoring 1 --gap-open 5 --gap-extend 2 --zdrop " + zdrop + " --threads " + threads + " --remove-tmp-files " + rm});
    t.push_back({"kmermatcher", {IN, C + "/pref"}, SUB + " --alph-size nucl:5,aa:13 --min-seq-id " + sid + " --kmer-per-seq 200 --spaced-kmer-mode 0 --kmer-per-seq-scale 0.200 --adjust-kmer-len 0 --mask 0 "
                 "--mask-lower-case 0 --cov-mode 1 -k 20 -c " + cov + " --max-seq-len " + maxLen + " --hash-shift " + hashShift + " --split-memory-limit 0 --include-only-extendable 0 --ignore-multi-kmer 1 " + TCV});
    t.push_back({"rescorediagonal", {IN, IN, C + "/pref", C + "/pref_rescore1"}, SUB + " --rescore-mode 0 --wrapped-scoring 1 --filter-hits 0 -e " + ev + " -c " + cov + " -a 0 --cov-mode 1 --min-seq-id " + sid +
                 " --min-aln-len 0 --seq-id-mode 0 --add-self-matches 0 --sort-results 0 --db-load-mode 0 " + TCV});
    const std::string CLUST = "--cluster-mode 2 --max-iterations 1000 --similarity-type 2 " + TCV;
    t.push_back({"clust", {IN, C + "/pref_rescore1", C + "/pre_clust"}, CLUST});
    t.push_back({"createsubdb", {C + "/order_redundancy", IN, STEP}, "-v " + lv + " --subdb-mode 1"});
    t.push_back({"createsubdb", {C + "/order_redundancy", C + "/pref", C + "/pref_filter1"}, "-v " + lv + " --subdb-mode 1"});
    t.push_back({"filterdb", {C + "/pref_filter1", C + "/pref_filter2"}, "--filter-file " + C + "/order_redundancy " + TCV});
    t.push_back({"align", {STEP, STEP, C + "/pref_filter2", C + "/aln"}, SUB + " -a 0 --alignment-mode 2 --alignment-output-mode 0 --wrapped-scoring 1 -e " + ev + " --min-seq-id " + sid +
                 " --min-aln-len 0 --seq-id-mode 0 --alt-ali 0 -c " + cov + " --cov-mode 1 --max-seq-len " + maxLen + " --comp-bias-corr 1 --max-rejected 2147483647 --max-accept 2147483647 --add-self-matches 0 "
                 "--db-load-mode 0 --pca 1 --pcb 1.5 --score-bias 0 --realign 0 --realign-score-bias -0.2 --realign-max-seqs 2147483647 --gap-open 5 --gap-extend 2 --zdrop " + zdrop + " " + TCV});
    t.push_back({"clust", {STEP, C + "/aln", C + "/clust"}, CLUST});
    t.push_back({"mergeclusters", {IN, T + "/clu", C + "/pre_clust", C + "/clust"}, TCV});
    t.push_back({"result2repseq", {IN, T + "/clu", REP}, "--threads " + threads + " -v " + v});
    if (withCycle) t.push_back({"createhdb", {REP, REP + "_cycle", REP}, "-v " + v});
    else t.push_back({"createhdb", {REP, REP}, "-v " + v});
    t.push_back({"convert2fasta", {REP, REP + ".fasta"}, "-v " + v});
    return t;
}
// the first column of every line of an index file
bool indexKeys(const std::string &path, std::vector<std::string> &lines, std::vector<uint32_t> &keys) {
    FILE *f = fopen(path.c_str(), "r");
    if (!f) return false;
    char *line = NULL; size_t cap = 0;
    while (getline(&line, &cap, f) != -1) { lines.push_back(line); keys.push_back((uint32_t) strtoul(line, NULL, 10)); }
    free(line); fclose(f);
    return true;
}
// the command's own directory and what it holds (--remove-tmp-files 1): plain files and links, one level of sub-directories
void removeOwnDir(const std::string &dir, int depth = 0) {
    if (DIR *d = opendir(dir.c_str())) {
        while (struct dirent *e = readdir(d)) {
            const std::string nm = e->d_name;
            if (nm == "." || nm == "..") continue;
            const std::string p = dir + "/" + nm;
            struct stat st;
            if (lstat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode)) { if (depth < 1) removeOwnDir(p, depth + 1); }
            else unlink(p.c_str());
        }
        closedir(d);
    }
    rmdir(dir.c_str());
}
int assembleFused(Args &a) {
    static const char *const USAGE = "Usage: carpedeam ancient_assemble_fused <reads.fast(a|q)[.gz]> <o:fastaFile> <tmpDir> [flags]\n"
                                     "       carpedeam ancient_assemble_fused <R1> <R2> [<R1> <R2> ...] <o:fastaFile> <tmpDir> [flags]";
    if (a.pos.empty()) die(USAGE);
    checkFlags("ancient_assemble_fused", a, FUSED_FLAGS);
    // GuidedNuclassembler.cpp:85-99: the file names count the output and the directory
    if (a.pos.size() < 3) die(std::string("Too few input files provided.\n") + USAGE);
    if ((a.pos.size() - 2) % 2 != 0 && a.pos.size() != 3) die(std::string("Too many input files provided.\nFor paired-end input provide READSETA_1.fastq READSETA_2.fastq ... OUTPUT.fasta tmpDir\n"
                                                                          "For single input use READSET.fast(q|a) OUTPUT.fasta tmpDir"));
    const std::vector<std::string> inputs(a.pos.begin(), a.pos.end() - 2);
    const std::string outFile = a.pos[a.pos.size() - 2], tmpDir = a.pos.back();
    // --damage-report <file>: after the FASTA, the per-contig coverage and damage tables of the final representatives against the reads the
    // loop started from (contig_damage's four steps on the resident reads); without the flag nothing is kept resident and no call is made
    const bool report = a.flag.count("--damage-report") != 0;
    const std::string reportFile = report ? a.flag["--damage-report"] : "";
    PileAsk ask;
    ask.damageOut = report ? &reportFile : NULL; ask.ends = damageEnds(a, "ancient_assemble_fused");
    // --depth-report <file>: likewise contig_depth's table of the final representatives against those reads; with both flags the two
    // reductions read one alignment set
    const bool depthRep = a.flag.count("--depth-report") != 0;
    const std::string depthFile = depthRep ? a.flag["--depth-report"] : "";
    ask.depthOut = depthRep ? &depthFile : NULL; ask.edge = depthEdge(a, "ancient_assemble_fused");
    // --variant-report <file> [--variant-sites <file>]: likewise contig_variants' summary and sites of the final representatives (no
    // consensus FASTA: that would be a second assembly output)
    const bool variantRep = a.flag.count("--variant-report") != 0;
    if (a.flag.count("--variant-sites") && !variantRep) die("ancient_assemble_fused: --variant-sites comes with --variant-report");
    const std::string variantFile = variantRep ? a.flag["--variant-report"] : "", variantSites = a.flag.count("--variant-sites") ? a.flag["--variant-sites"] : "";
    VariantOut variantOut;
    variantOut.opt = variantOpts(a, "ancient_assemble_fused");
    variantOut.summary = &variantFile; variantOut.sites = variantSites.empty() ? NULL : &variantSites; variantOut.consensus = NULL;
    ask.variants = variantRep ? &variantOut : NULL;
    // --break-report <file>: likewise contig_breaks' summary and break records of the final representatives (no split FASTA: that would
    // be a second assembly output)
    const bool breakRep = a.flag.count("--break-report") != 0;
    const std::string breakFile = breakRep ? a.flag["--break-report"] : "";
    BreakOut breakOut;
    breakOut.opt = breakOpts(a, "ancient_assemble_fused");
    breakOut.minPiece = 1; breakOut.summary = &breakFile; breakOut.split = NULL; breakOut.track = NULL;
    ask.breaks = breakRep ? &breakOut : NULL;
    const bool anyReport = report || depthRep || variantRep || breakRep;
    // (the parameter strings are split at blanks again, and linclust's filterdb carries a path under <tmpDir> in its string)
    if (tmpDir.find_first_of(" \t\n") != std::string::npos) die("ancient_assemble_fused: a <tmpDir> with white space in its name is not taken: " + tmpDir);
    if (const char *dry = getenv("CDM_FUSED_DRY_RUN")) {        // "cycle": the tail as it runs with circular contigs among the selection
        for (const TailStep &s : fusedTail(a, "$TMP", !strcmp(dry, "cycle"))) {
            printf("%s", s.module.c_str());
            for (const std::string &p : s.pos) printf(" %s", p.c_str());
            printf(" %s\n", s.flags.c_str());
        }
        return EXIT_SUCCESS;
    }
    struct stat st;
    if (stat(outFile.c_str(), &st) == 0) die(outFile + " exists already!");                         // guidedNuclAssemble.sh:24
    if (stat(tmpDir.c_str(), &st) != 0 && mkdir(tmpDir.c_str(), 0777) != 0) die("Can not create tmp directory " + tmpDir);
    std::string T = tmpDir + "/ancient_assemble_fused_XXXXXX";
    if (!mkdtemp(&T[0])) die("Can not create a directory under " + tmpDir);
    if (mkdir((T + "/clu_tmp").c_str(), 0777) != 0) die("Can not create " + T + "/clu_tmp");
    Laps laps;
    LoopEnd E;
    E.keepReads = anyReport;
    runLoop("ancient_assemble_fused", a, inputs, false, 10, true, E, laps);       // the workflow's defaults: --num-iterations 10 (GuidedNuclassembler.cpp:12), --num-iter-reads-only 5
    cdm_ctx *ctx = E.ctx;
    // ---- "select only assembled sequences" / "... fullfilling a minimum length threshold" (nuclassemble.sh:214-224) on the final DB
    // and on the circular contigs the iterations set aside (the script concatenates them first: the keys of the two are disjoint, and what
    // the selection keeps is brought into key order below, as concatdbs --preserve-keys + createsubdb leave it)
    const uint32_t minLen = (uint32_t) std::min<long>(std::max<long>(iflag(a, "--min-contig-len", 500), 0), 0xFFFFFFFEl);       // LocalParameters.h:288
    cdm_seqdb *selected = NULL; uint64_t kept = 0;
    check(cdm_seqdb_select_assembled(ctx, E.db, E.source, minLen, &selected, &kept), "selection of the assembled contigs");
    if (anyReport && !E.reads) E.reads = E.db;        // (a loop of no iteration: its DB is the reads)
    else cdm_seqdb_free(E.db);
    cdm_ctx *const reportCtx = anyReport ? ctx : NULL;
    OutChunk linear, circular, both;
    appendEntries(ctx, selected, linear);
    for (cdm_seqdb *c : E.cyclicDev) {
        cdm_seqdb *s = NULL;
        check(cdm_seqdb_select_assembled(ctx, c, E.source, minLen, &s, NULL), "selection of the assembled contigs");
        appendEntries(ctx, s, circular);
        cdm_seqdb_free(s); cdm_seqdb_free(c);
    }
    cdm_seqdb_free(E.source);
    fprintf(stderr, "%llu assembled contigs of at least %u letters (%llu circular)\n", (unsigned long long) (linear.key.size() + circular.key.size()), minLen, (unsigned long long) circular.key.size());
    laps.lap("assembled contigs selected");
    const bool removeTmp = iflag(a, "--remove-tmp-files", 0) != 0;
    if (linear.key.empty() && circular.key.empty()) {
        // nothing to reduce: the reference's whole program ends with status 0 and an empty FASTA here (tests/golden/fused/cases.json)
        cdm_seqdb_free(selected);
        if (!writeText(outFile, "")) die("Could not write " + outFile);
        if (anyReport) { pileReports(ctx, NULL, NULL, 20, 0.9f, ask, laps); cdm_seqdb_free(E.reads); }
        cdm_ctx_destroy(ctx);
        if (removeTmp) removeOwnDir(T);
        return EXIT_SUCCESS;
    }
    std::string err;
    const std::vector<TailStep> tail = fusedTail(a, T, !circular.key.empty());
    const std::string IN = T + "/nuclassembly", C = T + "/clu_tmp", REP = T + "/nuclassembly_rep";
    {
        concatByKey(linear, circular, both);
        std::vector<OutChunk> one(1); one[0] = std::move(both);
        if (!mmdbWriteChunks(IN, E.dbtype, one, &err)) die(err);
        if (!circular.key.empty()) {      // nuclassemble.sh:231: the index lines of the selected circular contigs
            std::vector<uint32_t> ck(circular.key.begin(), circular.key.end()); std::sort(ck.begin(), ck.end());
            std::vector<std::string> lines; std::vector<uint32_t> keys; std::string text;
            if (!indexKeys(IN + ".index", lines, keys)) die("Could not read " + IN + ".index");
            for (size_t i = 0; i < keys.size(); i++) if (std::binary_search(ck.begin(), ck.end(), keys[i])) text += lines[i];
            if (!writeText(IN + "_cycle.index", text)) die("Could not write " + IN + "_cycle.index");
        }
    }
    MmDb asmDb; if (!asmDb.load(IN, &err)) die(err);
    // the DB linclust's device stages run on: the selection as it stands on the device; with circular contigs among it, the few
    // selected contigs in their key order, uploaded
    cdm_seqdb *db = selected;
    if (!circular.key.empty()) { cdm_seqdb_free(selected); db = uploadSeqDb(ctx, asmDb); }
    {
        std::vector<uint32_t> keys(asmDb.size());
        check(cdm_seqdb_meta(ctx, db, NULL, keys.data(), NULL), "meta");
        if (cdm_seqdb_size(db) != asmDb.size() || !std::equal(keys.begin(), keys.end(), asmDb.key.begin())) die("ancient_assemble_fused: the selected contigs are not in key order on the device");
    }
    cdm_hits *hits = NULL;
    for (const TailStep &s : tail) {
        Args sa = stepArgs(s);
        if (s.module == "linclust") continue;
        if (s.module == "kmermatcher") {
            checkFlags("kmermatcher", sa, KMERMATCHER_FLAGS);
            const cdm_kmer_params p = kmerParams(sa);
            check(cdm_kmermatch(ctx, db, &p, &hits), "kmermatcher");
            HVec<uint64_t> off(asmDb.size() + 1); HVec<cdm_hit> rec(cdm_hits_count(hits));
            check(cdm_hits_download(ctx, hits, off.data(), rec.data()), "download");
            std::vector<OutChunk> chunks;
            formatPrefDb(asmDb, off.data(), rec.data(), chunks);
            if (!mmdbWriteChunks(s.pos[1], 14, chunks, &err, true)) die(err);
        } else if (s.module == "rescorediagonal") {     // linclust's Hamming pre-clustering, on the hits as they stand on the device
            checkFlags("rescorediagonal", sa, RESCORE_HAMMING_FLAGS);
            MmDb pref; if (!pref.load(s.pos[2], &err)) die(err);
            const cdm_hamming_params p = hammingParams(sa, (pref.dbtype & 0x7FFFFFFF) == 14);
            cdm_hits *keptHits = NULL;
            check(cdm_rescore_hamming(ctx, db, hits, &p, &keptHits), "rescorediagonal");
            HVec<uint64_t> koff(asmDb.size() + 1); HVec<cdm_hit> krec(cdm_hits_count(keptHits));
            check(cdm_hits_download(ctx, keptHits, koff.data(), krec.data()), "download");
            std::vector<OutChunk> chunks;
            formatRescoredPrefDb(asmDb, pref, koff.data(), krec.data(), chunks);
            if (!mmdbWriteChunks(s.pos[3], pref.dbtype, chunks, &err, true)) die(err);
            // the device's part is done: everything after this works on cluster lists and the contig DB's files
            cdm_hits_free(keptHits); cdm_hits_free(hits); hits = NULL; cdm_seqdb_free(db); db = NULL; if (!anyReport) cdm_ctx_destroy(ctx);      // (the reports' reads stay, with the context)
            ctx = NULL;
            laps.lap("linclust: kmermatcher, Hamming rescore");
        } else if (s.module == "createhdb") {
            if (s.pos.size() > 2) {     // guidedNuclAssemble.sh:197-199: the representatives that are circular contigs
                std::vector<std::string> cl, rl; std::vector<uint32_t> ckeys, rkeys; std::string text;
                if (!indexKeys(IN + "_cycle.index", cl, ckeys) || !indexKeys(REP + ".index", rl, rkeys)) die("Could not read " + REP + ".index");
                std::sort(ckeys.begin(), ckeys.end());
                for (size_t i = 0; i < rkeys.size(); i++) if (std::binary_search(ckeys.begin(), ckeys.end(), rkeys[i])) text += rl[i];
                if (!writeText(REP + "_cycle.index", text)) die("Could not write " + REP + "_cycle.index");
            }
            createhdb(sa);
        } else if (s.module == "convert2fasta") convert2fasta(sa);
        else {
            clusterModules(s.module, sa);
            if (s.module == "clust" && s.pos[2] == C + "/pre_clust") {      // linclust.sh:39: awk '{ print $1 }' pre_clust.index > order_redundancy
                std::vector<std::string> lines; std::vector<uint32_t> keys; std::string text;
                if (!indexKeys(s.pos[2] + ".index", lines, keys)) die("Could not read " + s.pos[2] + ".index");
                for (uint32_t k : keys) text += std::to_string(k) + "\n";
                if (!writeText(C + "/order_redundancy", text)) die("Could not write " + C + "/order_redundancy");
            }
        }
    }
    laps.lap("linclust's tail, representatives, headers, FASTA");
    if (rename((REP + ".fasta").c_str(), outFile.c_str()) != 0) {       // (another file system: copied)
        FILE *in = fopen((REP + ".fasta").c_str(), "rb"), *out = fopen(outFile.c_str(), "wb");
        if (!in || !out) die("Could not move result to " + outFile);
        char buf[1 << 16]; size_t n; bool ok = true;
        while ((n = fread(buf, 1, sizeof(buf), in)) > 0) ok = ok && fwrite(buf, 1, n, out) == n;
        fclose(in);
        if (fclose(out) != 0 || !ok) die("Could not move result to " + outFile);
        unlink((REP + ".fasta").c_str());
    }
    if (anyReport) {       // rank 0's context (the loop's helpers of a --gpus N run are gone): the FASTA as contig_damage would read it, the reads as they stand
        SeqSet contigs;
        const bool have = loadSeqSet(reportCtx, outFile, false, true, contigs);
        pileReports(reportCtx, have ? &contigs : NULL, E.reads, 20, 0.9f, ask, laps);
        if (contigs.db) cdm_seqdb_free(contigs.db);
        cdm_seqdb_free(E.reads); cdm_ctx_destroy(reportCtx);
    }
    if (removeTmp) removeOwnDir(T);
    return EXIT_SUCCESS;
}
}  // namespace

// see reportDone(): true in the process that goes on with the work
static bool workInChild() {
    if (!leaveAtOnce() || getenv("CDM_NO_FORK")) return true;
    int fds[2];
    if (pipe(fds) != 0) return true;
    fflush(stdout); fflush(stderr);
    const pid_t pid = fork();
    if (pid < 0) { close(fds[0]); close(fds[1]); return true; }
    if (pid == 0) { close(fds[0]); g_doneFd = fds[1]; prctl(PR_SET_PDEATHSIG, SIGKILL); if (getppid() == 1) _exit(EXIT_FAILURE); return true; }
    close(fds[1]);
    unsigned char b = 0; ssize_t r;
    while ((r = read(fds[0], &b, 1)) < 0 && errno == EINTR) {}
    if (r == 1) _exit((int) b);
    int st = 0;
    while (waitpid(pid, &st, 0) < 0) if (errno != EINTR) _exit(EXIT_FAILURE);
    if (WIFSIGNALED(st)) { signal(WTERMSIG(st), SIG_DFL); raise(WTERMSIG(st)); _exit(128 + WTERMSIG(st)); }
    _exit(WEXITSTATUS(st));
}
int main(int argc, char **argv) {
    // (ancient_assemble_fused is one process from the reads to the FASTA: it has nobody to hand an early answer to)
    if (!(argc >= 2 && !strcmp(argv[1], "ancient_assemble_fused"))) workInChild();
    if (argc < 2) { fprintf(stderr, "usage: carpedeam <kmermatcher|rescorediagonal|ancient_correction|ancient_read_assemble|ancient_contig_merge|cyclecheck|ancient_reads_loop|ancient_assemble_fused|contig_damage|contig_depth|contig_variants|contig_breaks|contig_map|contig_indels|contig_dedup|contig_links|contig_join|createdb|mergereads|convert2fasta|createhdb|clust|createsubdb|filterdb|mergeclusters|result2repseq|rmdb|mvdb> <args>\n"); return EXIT_FAILURE; }
    const std::string cmd = argv[1];
    Args a = parse(argc - 2, argv + 2);
    {   // --threads / MMSEQS_NUM_THREADS as in Parameters.cpp:2121-2132: the host side (DB parsing, text codecs) uses them
        long th = a.flag.count("--threads") ? strtol(a.flag["--threads"].c_str(), NULL, 10) : 0;
        if (th <= 0) if (const char *e = getenv("MMSEQS_NUM_THREADS")) th = strtol(e, NULL, 10);
        omp_set_dynamic(0);      // every slice of the per-thread loops below has its thread
        if (th > 0) { omp_set_num_threads((int) th); setenv("OMP_NUM_THREADS", std::to_string(th).c_str(), 1); }      // (the library's own loops read it)
    }
    auto t0 = std::chrono::steady_clock::now(); g_t0 = t0;
    int rc;
    if (cmd == "kmermatcher") rc = kmermatcher(a);
    else if (cmd == "rescorediagonal") rc = rescorediagonal(a);
    else if (cmd == "ancient_correction") rc = ancientModule(a, 0);
    else if (cmd == "ancient_read_assemble") rc = ancientModule(a, 1);
    else if (cmd == "ancient_contig_merge") rc = ancientModule(a, 2);
    else if (cmd == "ancient_reads_loop") rc = readsLoop(a);
    else if (cmd == "ancient_assemble_fused") rc = assembleFused(a);
    else if (cmd == "contig_damage") rc = contigDamage(a);
    else if (cmd == "contig_depth") rc = contigDepth(a);
    else if (cmd == "contig_variants") rc = contigVariants(a);
    else if (cmd == "contig_breaks") rc = contigBreaks(a);
    else if (cmd == "contig_map") rc = contigMap(a);
    else if (cmd == "contig_indels") rc = contigIndels(a);
    else if (cmd == "contig_dedup") rc = contigDedup(a);
    else if (cmd == "contig_links") rc = contigLinks(a);
    else if (cmd == "contig_join") rc = contigJoin(a);
    else if (cmd == "align" || cmd == "clust" || cmd == "createsubdb" || cmd == "filterdb" || cmd == "mergeclusters" || cmd == "result2repseq" || cmd == "rmdb" || cmd == "mvdb") rc = clusterModules(cmd, a);
    else if (cmd == "createdb") rc = createdb(a);
    else if (cmd == "convert2fasta") rc = convert2fasta(a);
    else if (cmd == "createhdb") rc = createhdb(a);
    else if (cmd == "mergereads") rc = mergereads(a);
    else if (cmd == "cyclecheck") rc = cyclecheck(a);
    else { fprintf(stderr, "Invalid Command: %s\n", cmd.c_str()); return EXIT_FAILURE; }
    fprintf(stderr, "Time for processing: %.3fs\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    // Every output file is written and closed, every handle and the context released: leave without the static destructors (the
    // HIP runtime's own tear-down is where one module run in ~1 500 of the fuzz campaigns ended with a signal after its work was done)
    // (not under a profiler that writes its results from an exit handler: ROCP_TOOL_LIBRARIES / a profiler's LD_PRELOAD / CDM_NORMAL_EXIT)
    if (!leaveAtOnce()) return rc;
    fflush(stdout); fflush(stderr);
    reportDone(rc);
    _exit(rc);
}
