// host/records.cpp: the record codecs of the module surface - the text of the prefilter and alignment DBs (QueryMatcher.h:114-126,
// Matcher.cpp:274-404) to and from the CSR record arrays of the C ABI, and the same arrays as binary side-cars (host/sidecar.h).
// Host code only: no context, no device call (tests/test_records_host.py runs it without a GPU).
#pragma once
#include <cmath>
#include <cstdlib>
#include <thread>

#include "carpedeam_hip.h"
#include "mmdb.h"
#include "sidecar.h"

// ---- readers for the tab-separated records (strtol / strtod walk the locale machinery: 10x the time of these)
// unsigned / signed decimal at d; d moves behind the digits (no digits: 0, as strtol gives)
inline unsigned long parseU(const char *&d) { unsigned long v = 0; while (*d >= '0' && *d <= '9') v = v * 10 + (unsigned long) (*d++ - '0'); return v; }
inline long parseI(const char *&d) { bool neg = false; if (*d == '-') { neg = true; d++; } else if (*d == '+') d++; const long v = (long) parseU(d); return neg ? -v : v; }
// a plain decimal "digits[.digits]" with at most 15 significant digits is mantissa / 10^k, both exact doubles: the division is
// correctly rounded, i.e. the very double strtod returns.  Anything else (exponents, inf, nan, long mantissas) goes to strtod.
inline double parseDecimal(const char *&d) {
    static const double P10[] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15};
    const char *p = d; unsigned long m = 0; int digits = 0, frac = 0;
    while (*p >= '0' && *p <= '9') { m = m * 10 + (unsigned long) (*p++ - '0'); digits++; }
    if (*p == '.') { p++; while (*p >= '0' && *p <= '9') { m = m * 10 + (unsigned long) (*p++ - '0'); digits++; frac++; } }
    if (digits == 0 || digits > 15 || *p == 'e' || *p == 'E' || (*p != '\t' && *p != '\n' && *p != '\0')) { char *e; const double v = strtod(d, &e); d = e; return v; }
    d = p;
    return (double) m / P10[frac];
}
inline void skipField(const char *&d) { while (*d && *d != '\t' && *d != '\n') d++; }
inline char *seqIdText(float s, char *p) {   // Util::fastSeqIdToBuffer + the tab overwriting its last char (Util.cpp:278-307, Matcher.cpp:362-363)
    if (s == 1.0) { memcpy(p, "1.00", 4); return p + 4; }
    *p++ = '0'; *p++ = '.';
    if (s < 0.10) *p++ = '0';
    if (s < 0.01) *p++ = '0';
    return itoa((int) (s * 1000), p);
}
// computeRawScoreFromBitScore as the consumers of the alignment text do (correction.cpp:222)
inline int rawScoreFromBits(int bits) {
    const double lam = 0x1.4478764a1b24ap-1, logk = log(0x1.a1c1e68ea2ab1p-2), LN2 = std::log(2.0);
    return static_cast<int>((logk + bits * LN2) / lam + 0.5);
}

// QueryMatcher::parsePrefilterHits / Matcher::parseAlignmentRecord: the text as CSR over the query ids (die()s on a target key the
// sequence DB lacks and on an entry that does not end where its index length says)
void parsePrefDb(const MmDb &pref, const MmDb &seq, HVec<uint64_t> &off, HVec<cdm_hit> &rec);
void parseAlnDb(const MmDb &aln, const MmDb &seq, HVec<uint64_t> &off, HVec<cdm_aln> &rec);
// QueryMatcher::prefilterHitToBuffer per hit, one DB entry per query (kmermatcher.cpp:815-930)
void formatPrefDb(const MmDb &seq, const uint64_t *off, const cdm_hit *rec, std::vector<OutChunk> &chunks);
// the same records for the result of the Hamming mode: one entry per query that has a prefilter entry (rescorediagonal.cpp:350), flag 0
void formatRescoredPrefDb(const MmDb &seq, const MmDb &pref, const uint64_t *off, const cdm_hit *rec, std::vector<OutChunk> &chunks);
// Matcher::resultToBuffer per record, one DB entry per query that has a prefilter entry (rescorediagonal.cpp:145-356)
// (asParsed, if given: every record as parseAlnDb would read it back from the text written here - raw score recomputed from the bit
// score, the coordinates, and in `ident` the identity in thousandths as the text truncates it: what writeAlnsSide takes.
// pref == NULL: every query has a prefilter entry - the hits came from kmermatcher's own side-car.)
void formatAlnDb(const MmDb &seq, const MmDb *pref, const uint64_t *aoff, const cdm_aln *arec, uint64_t dbRes, std::vector<OutChunk> &chunks, cdm_aln *asParsed = NULL);

// ---- record side-cars: the CSR a consumer's parser would produce from the text, as cdm_hits_upload / cdm_alns_upload take it
bool writeHitsSide(const std::string &path, const MmDb &seq, const uint64_t *off, const cdm_hit *rec, int dbtype, SideHeader *hdr);
bool writeAlnsSide(const std::string &path, const MmDb &seq, const uint64_t *off, const cdm_aln *asParsed, SideHeader *hdr);
// hits / alignments of the DB at `path` from its side-car if that belongs to these files and to this sequence DB
bool readHitsSide(const std::string &path, const MmDb &seq, HVec<uint64_t> &off, HVec<cdm_hit> &rec, int *dbtype);
bool readAlnsSide(const std::string &path, const MmDb &seq, HVec<uint64_t> &off, HVec<cdm_aln> &rec);
// the record side-cars beside the text: their sections are built and written in a thread while the caller formats and writes the text DB
struct SideThread {
    std::thread th; SideHeader hdr; bool ok = false; std::string path;
    template <typename F> void begin(const std::string &p, F body) { if (!sideEnabled()) return; path = p; th = std::thread([this, body] { ok = body(&hdr); }); }
    void commit() { if (th.joinable()) { th.join(); if (ok) sideCommit(path, &hdr); } }
};
