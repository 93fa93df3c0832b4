// The record codecs of the module surface (host/records.h): one parse skeleton and one format skeleton over the queries' record lists,
// the per-record bodies of the prefilter and alignment text, and the record side-cars.
#include <algorithm>
#include <cstdio>
#include <omp.h>

#include "records.h"
#include "cli.h"

// Slices of the queries that carry about the same number of RECORDS each (off = CSR offsets of the records; a query costs one more
// unit).  The record lists are anything but even: kmermatcher's representatives - the longest, lowest-id sequences - hold the hits of
// whole k-mer groups, so at 10 M reads the first sixteenth of the queries owned most of the text and threads beyond the first
// added nothing.
static std::vector<size_t> balancedSlices(const uint64_t *off, size_t n, int T) {
    std::vector<size_t> b(T + 1, n);
    b[0] = 0;
    const uint64_t total = off[n] + n;
    for (int t = 1; t < T; t++) {
        const uint64_t want = total / (uint64_t) T * (uint64_t) t;
        size_t lo = b[t - 1], hi = n;
        while (lo < hi) { const size_t mid = (lo + hi) / 2; if (off[mid] + mid < want) lo = mid + 1; else hi = mid; }
        b[t] = lo;
    }
    return b;
}
// number of records (= lines) of entry i of a result DB
static inline uint32_t countLines(const MmDb &db, int64_t i) {
    if (i < 0) return 0;
    const char *d = db.entry((size_t) i), *e = d + (db.len[(size_t) i] ? db.len[(size_t) i] - 1 : 0);
    uint32_t n = 0;
    while (d < e) { const char *nl = (const char *) memchr(d, '\n', (size_t) (e - d)); n++; d = nl ? nl + 1 : e; }
    return n;
}
// CSR offsets of the queries' record lists: the lines are counted first (memchr speed), the records then go straight to their place
static void countRecords(const MmDb &res, const MmDb &seq, HVec<uint64_t> &off) {
    const size_t n = seq.size();
    off.resize(n + 1);
    off[0] = 0;
#pragma omp parallel for schedule(dynamic, 4096)
    for (size_t i = 0; i < n; i++) off[i + 1] = countLines(res, res.idOf(seq.key[i]));
    for (size_t i = 0; i < n; i++) off[i + 1] += off[i];
}
// The parse skeleton: the result DB `res` as CSR over the queries of `seq`.  line(d, r) reads the record at d into r, leaves d behind
// what it read and returns -1, or the target key that the sequence DB lacks.
template <typename Rec, typename Line> static void parseDb(const MmDb &res, const MmDb &seq, HVec<uint64_t> &off, HVec<Rec> &rec, Line line) {
    const int T = std::max(1, omp_get_max_threads());
    countRecords(res, seq, off);
    rec.resize(off[seq.size()]);
    long badKey = -1, badEntry = -1;
    const std::vector<size_t> cut = balancedSlices(off.data(), seq.size(), T);
#pragma omp parallel for schedule(static, 1) num_threads(T)     // a loop over the slices: a smaller team still visits them all
    for (int t = 0; t < T; t++) {
        const size_t lo = cut[t], hi = cut[t + 1];
        for (size_t i = lo; i < hi; i++) {
            if (off[i + 1] == off[i]) continue;
            const char *d = res.entry((size_t) res.idOf(seq.key[i]));
            Rec *out = rec.data() + off[i], *const end = rec.data() + off[i + 1];
            while (*d && out < end) {
                Rec r;
                const long unknown = line(d, r);
                if (unknown >= 0) {
#pragma omp critical
                    badKey = unknown;
                    break;
                }
                *out++ = r;
                while (*d && *d != '\n') d++;
                if (*d == '\n') d++;
            }
            // the index length and the entry's NUL must agree (an embedded NUL or a wrong length would leave records unparsed or unfilled)
            if (badKey < 0 && (out != end || *d)) {
#pragma omp critical
                badEntry = (long) seq.key[i];
            }
        }
    }
    if (badKey >= 0) die("Invalid database read for key " + std::to_string(badKey));
    if (badEntry >= 0) die("Invalid database read: the entry of key " + std::to_string(badEntry) + " does not end where its index length says");
}
// The format skeleton: one chunk per thread, one DB entry per query i that has(i), wasExtended flag ext(i).  lines(hi) gives the record
// writer of a slice that ends before query hi - what it keeps from record to record is its thread's own -, and that writer's
// line(i, r, w) puts record r of query i at w in at most maxRec bytes and returns the end of what it wrote.
template <typename Has, typename Ext, typename Lines>
static void formatDb(const MmDb &seq, const uint64_t *off, size_t maxRec, std::vector<OutChunk> &chunks, Has has, Ext ext, Lines lines) {
    const int T = std::max(1, omp_get_max_threads());
    chunks.clear(); chunks.resize(T);
    const std::vector<size_t> cut = balancedSlices(off, seq.size(), T);
#pragma omp parallel for schedule(static, 1) num_threads(T)     // a loop over the slices: a smaller team still visits them all
    for (int t = 0; t < T; t++) {
        const size_t lo = cut[t], hi = cut[t + 1];
        OutChunk &c = chunks[t];
        c.reserve(hi - lo, (off[hi] - off[lo]) * maxRec + (hi - lo));
        auto line = lines(hi);
        for (size_t i = lo; i < hi; i++) {
            if (!has(i)) continue;
            char *const w0 = c.open((off[i + 1] - off[i]) * maxRec), *w = w0;
            for (uint64_t r = off[i]; r < off[i + 1]; r++) w = line(i, r, w);
            c.close(seq.key[i], w0, w, ext(i));
        }
    }
}
static const size_t MAXHIT = 10 + 1 + 11 + 1 + 6 + 1;      // "%u\t%d\t%d\n" with a short diagonal
static inline auto hitLines(const MmDb &seq, const cdm_hit *rec) {      // QueryMatcher::prefilterHitToBuffer
    return [&seq, rec](size_t) {
        return [&seq, rec](size_t, uint64_t h, char *w) {
            w = utoa(seq.keyOf(rec[h].target), w); *w++ = '\t'; w = itoa(rec[h].score, w); *w++ = '\t'; w = itoa((short) rec[h].diagonal, w); *w++ = '\n';
            return w;
        };
    };
}
void parsePrefDb(const MmDb &pref, const MmDb &seq, HVec<uint64_t> &off, HVec<cdm_hit> &rec) {
    parseDb(pref, seq, off, rec, [&seq](const char *&d, cdm_hit &h) -> long {
        const uint32_t tkey = (uint32_t) parseU(d); if (*d == '\t') d++; h.score = (int) parseI(d); if (*d == '\t') d++; h.diagonal = (short) parseI(d);
        const int64_t tt = seq.idOf(tkey);
        h.target = (uint32_t) tt;
        return tt < 0 ? (long) tkey : -1;
    });
}
void parseAlnDb(const MmDb &aln, const MmDb &seq, HVec<uint64_t> &off, HVec<cdm_aln> &rec) {   // Matcher.cpp:274-353
    parseDb(aln, seq, off, rec, [&seq](const char *&d, cdm_aln &r) -> long {
        auto tab = [&] { if (*d == '\t') d++; };
        const uint32_t tkey = (uint32_t) parseU(d); tab();
        const int bits = (int) parseI(d); tab();
        r.seq_id = (float) parseDecimal(d); tab();
        skipField(d); tab();                                   // the E-value is not read back
        r.q_start = (int) parseI(d); tab(); r.q_end = (int) parseI(d); tab(); skipField(d); tab();
        r.db_start = (int) parseI(d); tab(); r.db_end = (int) parseI(d); tab(); skipField(d);
        const int64_t tt = seq.idOf(tkey);
        r.target = (uint32_t) tt; r.ident = -1; r.raw_score = rawScoreFromBits(bits);
        return tt < 0 ? (long) tkey : -1;
    });
}
void formatPrefDb(const MmDb &seq, const uint64_t *off, const cdm_hit *rec, std::vector<OutChunk> &chunks) {
    // representatives' records carry wasExtended 0, fill-in records the sequence's flag (kmermatcher.cpp:727, DBWriter default)
    formatDb(seq, off, MAXHIT, chunks, [](size_t) { return true; }, [&seq, off](size_t i) -> uint8_t { return (off[i + 1] - off[i] > 1) ? 0 : seq.ext[i]; }, hitLines(seq, rec));
}
void formatRescoredPrefDb(const MmDb &seq, const MmDb &pref, const uint64_t *off, const cdm_hit *rec, std::vector<OutChunk> &chunks) {
    formatDb(seq, off, MAXHIT, chunks, [&](size_t i) { return pref.idOf(seq.keyOf(i)) >= 0; }, [](size_t) -> uint8_t { return 0; }, hitLines(seq, rec));
}
void formatAlnDb(const MmDb &seq, const MmDb *pref, const uint64_t *aoff, const cdm_aln *arec, uint64_t dbRes, std::vector<OutChunk> &chunks, cdm_aln *asParsed) {
    const size_t MAXREC = 10 + 11 + 5 + 14 + 6 * 11 + 10;      // key, bits, seq.id., E-value, six coordinates, separators
    // the E-value text and bit score of (raw score, query length) recur all over a read set: formatted once per thread
    struct EvalText { int qLen = -1, score = -1, bits = 0; unsigned char n = 0; char txt[15]; };
    formatDb(seq, aoff, MAXREC, chunks, [&](size_t i) { return !pref || pref->idOf(seq.key[i]) >= 0; }, [](size_t) -> uint8_t { return 0; },
             [=, &seq](size_t hi) { return [=, &seq, cache = std::vector<EvalText>(1u << 14)](size_t i, uint64_t r, char *w) mutable {   // Matcher::resultToBuffer (Matcher.cpp:356-404)
        const int qLen = (int) (seq.len[i] - 2);
        const cdm_aln &x = arec[r];
        if (r + 16 < aoff[hi]) __builtin_prefetch(&seq.len[arec[r + 16].target]);      // (a random look-up per record: on its way 16 records ahead)
        const int alnLen = std::max(abs(x.q_end - x.q_start), abs(x.db_end - x.db_start)) + 1;
        const float sid = static_cast<float>(x.ident) / static_cast<float>(alnLen);
        w = utoa(seq.keyOf(x.target), w); *w++ = '\t';
        EvalText &ev = cache[((uint32_t) x.raw_score * 2654435761u ^ (uint32_t) qLen * 40503u) >> 18];
        if (ev.qLen != qLen || ev.score != x.raw_score) {
            ev.qLen = qLen; ev.score = x.raw_score; ev.bits = cdm_bit_score(x.raw_score);
            ev.n = (unsigned char) snprintf(ev.txt, sizeof(ev.txt), "%.3E", cdm_evalue(x.raw_score, qLen, dbRes));
        }
        w = itoa(ev.bits, w); *w++ = '\t';
        w = seqIdText(sid, w); *w++ = '\t';
        memcpy(w, ev.txt, ev.n); w += ev.n; *w++ = '\t';
        w = itoa(x.q_start, w); *w++ = '\t'; w = itoa(x.q_end, w); *w++ = '\t'; w = itoa(qLen, w); *w++ = '\t';
        w = itoa(x.db_start, w); *w++ = '\t'; w = itoa(x.db_end, w); *w++ = '\t'; w = itoa((int) (seq.len[x.target] - 2), w); *w++ = '\n';
        if (asParsed) {
            cdm_aln p = x;
            p.raw_score = rawScoreFromBits(ev.bits); p.ident = (int) seqIdTo1000(sid); p.seq_id = seqIdFrom1000((uint32_t) p.ident);
            asParsed[r] = p;
        }
        return w;
    }; });
}

bool writeHitsSide(const std::string &path, const MmDb &seq, const uint64_t *off, const cdm_hit *rec, int dbtype, SideHeader *hdr) {
    if (!sideEnabled()) return false;
    const uint64_t n = seq.size(), count = off[n];
    bool fits = true;
#pragma omp parallel for reduction(&& : fits) schedule(static)
    for (uint64_t i = 0; i < count; i++) { cdm_hit h = rec[i]; h.diagonal = (short) h.diagonal; fits = fits && fitsHit8(h); }
    const uint64_t hash = sideKeyHash(seq.key.data(), n);
    if (fits) {
        HVec<SideHit8> c(count);
#pragma omp parallel for schedule(static)
        for (uint64_t i = 0; i < count; i++) { c[i].target = rec[i].target; c[i].score = (int16_t) rec[i].score; c[i].diagonal = (int16_t) (short) rec[i].diagonal; }
        const SidePiece pc[2] = {{off, (n + 1) * 8}, {c.data(), count * sizeof(SideHit8)}};
        return sideWriteBody(path, SIDE_HITS, SIDE_F_COMPACT, n, count, n, hash, dbtype, pc, 2, hdr);
    } else {
        HVec<cdm_hit> c(count);
#pragma omp parallel for schedule(static)
        for (uint64_t i = 0; i < count; i++) { c[i] = rec[i]; c[i].diagonal = (short) rec[i].diagonal; }       // (the text holds the diagonal as a short: QueryMatcher.h:114-126)
        const SidePiece pc[2] = {{off, (n + 1) * 8}, {c.data(), count * sizeof(cdm_hit)}};
        return sideWriteBody(path, SIDE_HITS, 0, n, count, n, hash, dbtype, pc, 2, hdr);
    }
}
bool writeAlnsSide(const std::string &path, const MmDb &seq, const uint64_t *off, const cdm_aln *asParsed, SideHeader *hdr) {
    if (!sideEnabled()) return false;
    const uint64_t n = seq.size(), count = off[n];
    bool fits = true;
#pragma omp parallel for reduction(&& : fits) schedule(static)
    for (uint64_t i = 0; i < count; i++) {
        const cdm_aln &r = asParsed[i];
        auto s16 = [](int v) { return v >= -32768 && v <= 32767; };
        fits = fits && r.raw_score >= 0 && r.raw_score <= 65535 && s16(r.q_start) && s16(r.q_end) && s16(r.db_start) && s16(r.db_end);
    }
    const uint64_t hash = sideKeyHash(seq.key.data(), n);
    if (fits) {
        HVec<SideAln16> c(count);
#pragma omp parallel for schedule(static)
        for (uint64_t i = 0; i < count; i++) {
            const cdm_aln &r = asParsed[i];
            c[i].target = r.target; c[i].rawScore = (uint16_t) r.raw_score; c[i].seqId1000 = (uint16_t) r.ident;       // (ident carries the identity in thousandths here, see formatAlnDb)
            c[i].qStart = (int16_t) r.q_start; c[i].qEnd = (int16_t) r.q_end; c[i].dbStart = (int16_t) r.db_start; c[i].dbEnd = (int16_t) r.db_end;
        }
        const SidePiece pc[2] = {{off, (n + 1) * 8}, {c.data(), count * sizeof(SideAln16)}};
        return sideWriteBody(path, SIDE_ALNS, SIDE_F_COMPACT, n, count, n, hash, 5, pc, 2, hdr);
    } else {
        const SidePiece pc[2] = {{off, (n + 1) * 8}, {asParsed, count * sizeof(cdm_aln)}};
        return sideWriteBody(path, SIDE_ALNS, 0, n, count, n, hash, 5, pc, 2, hdr);
    }
}
// the side-car of kind `kind` of the DB at `path`, if it belongs to these files and to this sequence DB: mapped, its offsets copied and
// checked, room made for its records
template <typename Rec> static bool openRecordSide(const std::string &path, uint32_t kind, const MmDb &seq, SideFile &f, HVec<uint64_t> &off, HVec<Rec> &rec) {
    if (!sideOpen(path, kind, f)) return false;
    const SideHeader &h = *f.h;
    if (h.n != seq.size() || h.seqN != seq.size() || h.seqKeyHash != sideKeyHash(seq.key.data(), seq.size())) return false;
    off.resize(h.n + 1); rec.resize(h.count);
    memcpy(off.data(), f.section(0), (h.n + 1) * 8);
    return off[h.n] == h.count;
}
bool readHitsSide(const std::string &path, const MmDb &seq, HVec<uint64_t> &off, HVec<cdm_hit> &rec, int *dbtype) {
    SideFile f;
    if (!openRecordSide(path, SIDE_HITS, seq, f, off, rec)) return false;
    const SideHeader &h = *f.h;
    if (h.flags & SIDE_F_COMPACT) {
        const SideHit8 *c = (const SideHit8 *) f.section(1);
#pragma omp parallel for schedule(static)
        for (uint64_t i = 0; i < h.count; i++) { rec[i].target = c[i].target; rec[i].score = c[i].score; rec[i].diagonal = c[i].diagonal; }
    } else memcpy(rec.data(), f.section(1), h.count * sizeof(cdm_hit));
    *dbtype = h.dbtype;
    return true;
}
bool readAlnsSide(const std::string &path, const MmDb &seq, HVec<uint64_t> &off, HVec<cdm_aln> &rec) {
    SideFile f;
    if (!openRecordSide(path, SIDE_ALNS, seq, f, off, rec)) return false;
    const SideHeader &h = *f.h;
    if (h.flags & SIDE_F_COMPACT) {
        const SideAln16 *c = (const SideAln16 *) f.section(1);
#pragma omp parallel for schedule(static)
        for (uint64_t i = 0; i < h.count; i++) {
            cdm_aln r;
            r.target = c[i].target; r.raw_score = c[i].rawScore; r.ident = -1; r.q_start = c[i].qStart; r.q_end = c[i].qEnd; r.db_start = c[i].dbStart; r.db_end = c[i].dbEnd;
            r.seq_id = seqIdFrom1000(c[i].seqId1000);
            rec[i] = r;
        }
    } else {
        const cdm_aln *c = (const cdm_aln *) f.section(1);
#pragma omp parallel for schedule(static)
        for (uint64_t i = 0; i < h.count; i++) { cdm_aln r = c[i]; r.seq_id = seqIdFrom1000((uint32_t) r.ident); r.ident = -1; rec[i] = r; }
    }
    return true;
}
