// The command-line plumbing the units of the host binary share (host/main.cpp: the reference's modules and the process around them;
// host/contig_reports.cpp: the contig reports): fatal exits, arguments and flag tables, the CDM_TIMING laps, context and sequence upload.
#pragma once
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "carpedeam_hip.h"
#include "mmdb.h"

inline std::thread *g_deviceThread = NULL;   // a module's device start-up running beside the main thread (DeviceStart): joined before any exit
inline void quiesce() { if (g_deviceThread && g_deviceThread->joinable() && g_deviceThread->get_id() != std::this_thread::get_id()) g_deviceThread->join(); }
[[noreturn]] inline void die(const std::string &msg) { quiesce(); fprintf(stderr, "%s\n", msg.c_str()); exit(EXIT_FAILURE); }
// a call the device path does not implement, found before any work was done: status 77 tells the front end (host/front.c) that the
// reference binary - if the deployment has one - may take this call instead
[[noreturn]] inline void unsupported(const std::string &msg) { quiesce(); fprintf(stderr, "%s\n", msg.c_str()); exit(77); }
inline void check(int rc, const char *what) { if (rc != CDM_OK) die(std::string(what) + ": " + cdm_last_error()); }

struct Args { std::vector<std::string> pos; std::map<std::string, std::string> flag; };
// Per-module flag tables (the reference's own lists: lib/mmseqs/src/commons/Parameters.cpp:871-892 kmermatcher, :422-439
// rescorediagonal, src/commons/LocalParameters.h:155-171 assembleresults = ancient_correction / ancient_read_assemble).
//   'U' used by the MI355X path;  'N' accepted, no effect on this path in the reference either (or only on resources);
//   'V' accepted only with one of the listed values (anything else would be computed differently: refused);
//   'R' a flag the reference's list for the command knows and this path does not handle: refused whatever its value.
// A flag that is not in the module's list is an error, as in Parameters::parseParameters (:1703 "Unrecognized parameter").
struct FlagSpec { const char *name; char kind; const char *allowed; const char *why; };
inline void checkFlags(const char *module, const Args &a, const FlagSpec *spec, const char *const *extra = NULL) {
    for (const auto &kv : a.flag) {
        const FlagSpec *f = spec;
        while (f->name && kv.first != f->name) f++;
        bool known = f->name != NULL;
        for (const char *const *e = extra; !known && e && *e; e++) known = kv.first == *e;
        if (!known) die("Unrecognized parameter \"" + kv.first + "\"");
        if (f->name && f->kind == 'R') unsupported(std::string(module) + ": " + kv.first + " is not supported by the MI355X path (" + f->why + ")");
        if (f->name && f->kind == 'V') {
            const std::string al = f->allowed;
            const bool ok = (al.size() >= 2 && al[0] == '*') ? kv.second.find(al.substr(1, al.size() - 2)) != std::string::npos : kv.second == al;
            if (!ok) unsupported(std::string(module) + ": " + kv.first + " " + kv.second + " is not supported by the MI355X path (" + f->why + "; accepted: " + (al.empty() ? "\"\"" : al) + ")");
        }
    }
}
inline float fflag(Args &a, const char *n, float d) { return a.flag.count(n) ? strtof(a.flag[n].c_str(), NULL) : d; }
inline long iflag(Args &a, const char *n, long d) { return a.flag.count(n) ? strtol(a.flag[n].c_str(), NULL, 10) : d; }
inline double dflag(Args &a, const char *n, double d) { return a.flag.count(n) ? strtod(a.flag[n].c_str(), NULL) : d; }
// an integer flag with the values the device path takes: lo to hi, or the module refuses it with `what`
inline long rangedFlag(Args &a, const char *module, const char *flag, long dflt, long lo, long hi, const char *what) {
    const long v = iflag(a, flag, dflt);
    if (v < lo || v > hi) unsupported(std::string(module) + ": " + flag + " " + a.flag[flag] + " is not supported by the MI355X path (" + what + ")");
    return v;
}

// CDM_TIMING=1: where a module's wall time goes (stderr)
inline std::chrono::steady_clock::time_point g_t0, g_lastLap;
struct Laps {
    bool on; std::chrono::steady_clock::time_point t;
    Laps() : on(getenv("CDM_TIMING") != NULL), t(std::chrono::steady_clock::now()) {
        if (on && g_t0.time_since_epoch().count()) fprintf(stderr, "  %-32s %.3f s\n", "(arguments, flags)", std::chrono::duration<double>(t - g_t0).count());
        g_lastLap = t;
    }
    void lap(const char *what) {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        fprintf(stderr, "  %-32s %.3f s\n", what, std::chrono::duration<double>(n - t).count()); t = n; g_lastLap = n;
    }
};
inline cdm_ctx *openCtx(int offset = 0) {
    cdm_ctx *ctx = NULL;
    const char *dev = getenv("CARPEDEAM_DEVICE");
    check(cdm_ctx_create((dev ? atoi(dev) : 0) + offset, &ctx), "Can not initialise the MI355X device");
    return ctx;
}
// the sequences of a text DB on the device: 0 and *out, or an exit status (77: not a nucleotide DB, refused before the text is touched) and its message
inline int seqDbToDevice(cdm_ctx *ctx, const MmDb &db, cdm_seqdb **out, std::string *msg) {
    if ((db.dbtype & 0x7FFFFFFF) != 1) { *msg = "The MI355X path works on nucleotide sequence DBs only (dbtype " + std::to_string(db.dbtype & 0x7FFFFFFF) + " given)"; return 77; }
    std::vector<uint32_t> lens(db.size());
    for (size_t i = 0; i < db.size(); i++) lens[i] = db.len[i] >= 2 ? (uint32_t) (db.len[i] - 2) : 0;   // DBReader::getSeqLen
    if (cdm_seqdb_upload(ctx, db.data(), db.off.data(), lens.data(), db.key.data(), db.ext.data(), db.size(), out) == CDM_OK) return 0;
    *msg = std::string("Can not load the sequence DB: ") + cdm_last_error();
    return EXIT_FAILURE;
}
inline cdm_seqdb *uploadSeqDb(cdm_ctx *ctx, const MmDb &db) {
    cdm_seqdb *h = NULL; std::string msg;
    if (const int rc = seqDbToDevice(ctx, db, &h, &msg)) { if (rc == 77) unsupported(msg); die(msg); }
    return h;
}
inline bool writeText(const std::string &path, const std::string &text) {
    FILE *f = fopen(path.c_str(), "w");
    if (!f) return false;
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    return fclose(f) == 0 && ok;
}
