// The contig reports of the host binary (none is a module of the reference): contig_damage, contig_depth, contig_variants,
// contig_breaks, contig_map, contig_indels, contig_dedup, contig_links and contig_join, and pileReports, which ancient_assemble_fused (host/main.cpp) calls for its final
// contigs.  Every report stands on one pile-up: the contigs and the reads become one DB (contigs first, wasExtended 1; reads behind
// them, 0), kmermatcher and rescorediagonal run on it with the reads loop's flags, and a cdm_pileup_* reduction counts, per contig,
// the overlaps of the reads that seed on it: seeded UNGAPPED overlaps at the identity threshold, not a gapped mapping; a read counts
// on the longest sequence of each k-mer group it falls into (kmermatcher's representative rule), possibly on several contigs.
// --gapped 1 (all but contig_damage; contig_indels always): the set keeps its hits, cdm_pileup_gapped aligns the seeded pairs that
// test refused across insertions and deletions within a band, and the rescued reads count as well.  --dedup 1 (all but contig_indels):
// cdm_alns_dedup takes the duplicate reads out of the set before any reduction sees it; contig_dedup writes what it found.  contig_links
// joins a read's records on different contigs (cdm_pileup_links): which contig ends belong together; contig_join asks the letters at those
// ends (cdm_pileup_junctions) and writes the contigs joined along the links (host/contig_join.cpp).  The tables hold integers only.
#include <algorithm>
#include <cctype>
#include <numeric>
#include <omp.h>
#include <sys/stat.h>

#include "contig_join.h"
#include "contig_reports.h"

bool loadSeqSet(cdm_ctx *ctx, const std::string &path, bool shuffle, bool wantNames, SeqSet &in) {
    struct stat st; std::string err;
    if (stat((path + ".index").c_str(), &st) == 0) {
        MmDb seq; if (!seq.load(path, &err)) die(err);
        if (seq.size() == 0) return false;
        in.db = uploadSeqDb(ctx, seq);
        in.keys.assign(seq.key.begin(), seq.key.end());
        if (wantNames) {
            MmDb hdr;
            const bool haveHdr = stat((path + "_h.index").c_str(), &st) == 0 && hdr.load(path + "_h", &err);
            in.names.resize(seq.size());
            for (size_t i = 0; i < seq.size(); i++) {
                const int64_t h = haveHdr ? hdr.idOf(seq.key[i]) : -1;
                if (h >= 0) { const char *p = hdr.entry((size_t) h); size_t l = 0; while (l + 1 < hdr.len[(size_t) h] && p[l] && !isspace((unsigned char) p[l])) l++; in.names[i].assign(p, l); }
                if (in.names[i].empty()) in.names[i] = std::to_string(seq.key[i]);
            }
        }
        return true;
    }
    if (stat(path.c_str(), &st) != 0) die("Cannot open " + path);
    if (st.st_size == 0) return false;
    FastxDb fx;
    if (!readFastxNamed(std::vector<std::string>(1, path), shuffle, fx, wantNames ? &in.names : NULL, &err)) die(err);
    for (auto &l : fx.len) l -= 2;
    check(cdm_seqdb_upload(ctx, fx.blob.data(), fx.off.data(), fx.len.data(), fx.key.data(), NULL, fx.key.size(), &in.db), "Can not load the sequences");
    in.keys.assign(fx.key.begin(), fx.key.end());
    for (size_t i = 0; i < in.names.size(); i++) if (in.names[i].empty()) in.names[i] = std::to_string(in.keys[i]);
    return true;
}
long damageEnds(Args &a, const char *module) { return rangedFlag(a, module, "--damage-ends", 16, 1, 64, "the tables hold 1 to 64 positions from either end of a read"); }
long depthEdge(Args &a, const char *module) { return rangedFlag(a, module, "--depth-edge", 0, 0, 1048576, "0 to 1048576 positions are left out at either end of a contig"); }
VariantOpts variantOpts(Args &a, const char *module) {
    VariantOpts o;
    o.maskEnds = rangedFlag(a, module, "--mask-ends", 0, 0, 64, "0 to 64 read positions are left out at either end of a read");
    o.minDepth = rangedFlag(a, module, "--min-depth", 3, 1, 1000000, "a called position has 1 to 1000000 bases");
    o.minAltCount = rangedFlag(a, module, "--min-alt-count", 2, 1, 1000000, "a second allele has 1 to 1000000 bases");
    o.minAltPercent = rangedFlag(a, module, "--min-alt-percent", 20, 0, 100, "a percentage of the depth is 0 to 100");
    return o;
}
// The default anchor is reasoned, not measured: a read with w columns beyond a false join expects 0.75 w mismatches there, and at the
// identity threshold t a read of L columns is dropped when 0.75 w > (1 - t) L; w = 16 covers L <= 120 at t = 0.9.
BreakOpts breakOpts(Args &a, const char *module) {
    BreakOpts o;
    o.anchor = rangedFlag(a, module, "--break-anchor", 16, 1, 1024, "a spanning read has 1 to 1024 columns on either side of a boundary");
    o.edge = rangedFlag(a, module, "--break-edge", 50, 1, 1048576, "1 to 1048576 boundaries are left out at either end of a contig");
    if (o.edge < o.anchor) unsupported(std::string(module) + ": --break-edge " + std::to_string(o.edge) + " is not supported by the MI355X path (it is --break-anchor, here " + std::to_string(o.anchor) +
                                       ", at the least: nearer to a contig's end no read has its anchor on both sides)");
    o.minSpan = rangedFlag(a, module, "--min-span", 1, 1, 1000000, "a boundary is held by 1 to 1000000 spanning reads");
    o.minSpanPercent = rangedFlag(a, module, "--min-span-percent", 0, 0, 100, "a percentage of the depth is 0 to 100");
    return o;
}
// what a map report writes: the SAM file, with the read group when one is named, without the secondary lines when asked
struct MapOut { const std::string *sam, *readGroup; bool primaryOnly; GapOpts gap; };
// what an indel report writes: the summary always, the other two files when named (gap.on always: the report is about the rescued reads)
struct IndelOut { long minDepth, minCount, minPercent; GapOpts gap; const std::string *summary, *sites, *consensus; };
// what a link report writes: the table always, the other two files when named
struct LinkOut { long anchor, overhang, maxEnds, minReads; const std::string *table, *ends, *gfa; };
// what a join report writes: the table always, the other two files when named
struct JoinOut { long anchor, overhang, maxEnds, minLinkReads, overlapPercent; const std::string *table, *joined, *paths; };

namespace {
const char LETTER[] = "ACGTN";
// an integer behind a line, after a tab where the line is a TSV line
void put(std::string &to, unsigned long long v, bool tab = true) { char num[32]; if (tab) to.push_back('\t'); to.append(num, (size_t) (utoa(v, num) - num)); }
// a file the command writes when its flag names one
const std::string *flagPath(Args &a, const char *flag) { return a.flag.count(flag) ? &a.flag[flag] : NULL; }
void writeOrDie(const std::string *path, const std::string &text) { if (path && !writeText(*path, text)) die("Could not write " + *path); }

// The three library calls the reports share: the contigs (wasExtended 1) and the reads (0) as one DB, kmermatcher and
// rescorediagonal on it with the reads loop's flags.  The caller frees both results.
// keepHits: the prefilter hits stay in the set (cdm_pileup_gapped looks at the ones rescorediagonal refused).
struct PileSet { cdm_seqdb *both = NULL; cdm_alns *alns = NULL; cdm_hits *hits = NULL; };
PileSet pileupAlignments(cdm_ctx *ctx, cdm_seqdb *contigs, cdm_seqdb *reads, int kmerSize, float minSeqId, bool keepHits) {
    PileSet p; cdm_hits *hits = NULL;
    check(cdm_seqdb_concat(ctx, contigs, reads, 1, 0, &p.both), "contigs and reads as one DB");
    cdm_kmer_params kp;         // the reads loop's kmermatcher flags (stageflags.K_FLAGS)
    kp.kmer_size = kmerSize; kp.kmers_per_seq = 200; kp.kmers_per_seq_scale = 0.2f; kp.hash_shift = 67; kp.ignore_multi_kmer = 1; kp.include_only_extendable = 0; kp.cov_mode = 1; kp.cov_thr = 0.0f;
    cdm_rescore_params rp;      // its rescorediagonal flags (R_FLAGS)
    rp.seq_id_thr = minSeqId; rp.eval_thr = 0.001; rp.cov_mode = 1; rp.cov_thr = 0.0f; rp.seq_id_mode = 0; rp.min_aln_len = 0;
    check(cdm_kmermatch(ctx, p.both, &kp, &hits), "kmermatcher");
    check(cdm_rescore(ctx, p.both, hits, &rp, &p.alns), "rescorediagonal");
    if (keepHits) p.hits = hits; else cdm_hits_free(hits);
    return p;
}
void freePileSet(PileSet &p) { if (p.hits) cdm_hits_free(p.hits); if (p.alns) cdm_alns_free(p.alns); if (p.both) cdm_seqdb_free(p.both); p = PileSet(); }
// The gapped flags of a command.  whatGapped: what --gapped 0 and 1 mean to the module; NULL: the module (contig_indels) has no such
// flag, its gapped alignment is always on.  Either --gap-* flag without --gapped 1 is refused: it sets an alignment that is off.
GapOpts gapOpts(Args &a, const char *module, const char *whatGapped) {
    GapOpts g;
    g.on = !whatGapped || rangedFlag(a, module, "--gapped", 0, 0, 1, whatGapped) != 0;
    for (const char *flag : {"--gap-band", "--gap-min-columns"})
        if (!g.on && a.flag.count(flag)) unsupported(std::string(module) + ": " + flag + " without --gapped 1 is not supported by the MI355X path (the flag sets the gapped alignment, which is off)");
    g.band = rangedFlag(a, module, "--gap-band", 8, 1, 31, "the gapped alignment looks at 1 to 31 diagonals on either side of the seed's");
    g.minColumns = rangedFlag(a, module, "--gap-min-columns", 32, 1, 4096, "a rescued read has 1 to 4096 letters aligned at the least");
    g.minSeqId = fflag(a, "--min-seq-id", 0.9f);
    return g;
}
// --dedup 0|1 of a command.  Together with --gapped 1 it is refused: the candidates of the gapped alignment are the hits that left no
// record in the set, so a record this flag removed would come back as a rescued read.
bool dedupFlag(Args &a, const char *module, bool gapped) {
    const bool on = rangedFlag(a, module, "--dedup", 0, 0, 1, "0 counts every record, 1 leaves the duplicate reads out") != 0;
    if (on && gapped) unsupported(std::string(module) + ": --dedup 1 with --gapped 1 is not supported by the MI355X path (rescue candidates are the hits without a record, so a removed "
                                  "record would be rescued, and rescued reads need a duplicate rule of their own)");
    return on;
}
const char *const TABLE_GAPPED = "0 counts the ungapped overlaps alone, 1 adds the reads rescued across insertions and deletions";

// a sequence's name, or its key where the set carries no names
const std::string &seqName(const SeqSet &c, uint64_t i, std::string &tmp) { if (i < c.names.size()) return c.names[i]; tmp = std::to_string(c.keys[i]); return tmp; }
// The contigs of a report run: their number (0: no contigs, the reports are their header lines alone), the reductions' query list
// (every contig) and the lengths, brought down once.
struct Frame {
    const SeqSet *set = NULL; uint64_t nc = 0; std::vector<uint32_t> q, lens;
    Frame(cdm_ctx *ctx, const SeqSet *contigs) : set(contigs) {
        if (!(contigs && contigs->db && cdm_seqdb_size(contigs->db))) return;
        nc = cdm_seqdb_size(contigs->db);
        q.resize(nc); lens.resize(nc);
        std::iota(q.begin(), q.end(), 0u);
        check(cdm_seqdb_meta(ctx, contigs->db, lens.data(), NULL, NULL), "meta");
    }
    const std::string &name(uint64_t i, std::string &tmp) const { return seqName(*set, i, tmp); }
    // the columns every table begins with: name, key, length
    void row(std::string &to, uint64_t i) const { std::string tmp; to += name(i, tmp); put(to, set->keys[i]); put(to, lens[i]); }
};

// The set of a PileSet without the duplicate reads on the contigs (cdm_alns_dedup with what the reports pass to every reduction: reads
// only as targets, no second identity threshold), swapped in before any reduction; stats (may be NULL): nc x 4, the contigs' statistics.
void dedupSet(cdm_ctx *ctx, PileSet &ps, const Frame &c, uint64_t *stats) {
    std::vector<uint64_t> own;
    if (!stats) { own.resize(c.nc * 4); stats = own.data(); }
    cdm_dedup_params dp; dp.min_seq_id = 0.0f; dp.skip_extended_targets = 1;
    cdm_alns *kept = NULL; float ms = 0.f;
    check(cdm_alns_dedup(ctx, ps.both, ps.alns, c.q.data(), c.nc, &dp, &kept, stats, NULL, &ms), "duplicate reads");
    if (getenv("CDM_TIMING")) fprintf(stderr, "  duplicate reads: %llu records, %llu removed, dedup kernels %.3f ms\n", (unsigned long long) cdm_alns_count(ps.alns),
                                      (unsigned long long) (cdm_alns_count(ps.alns) - cdm_alns_count(kept)), ms);
    cdm_alns_free(ps.alns);
    ps.alns = kept;
}
// ---- contig_dedup: what --dedup 1 takes out of the other reports' set, cdm_alns_dedup over the contigs.  One TSV line per contig:
// the records of its row, those that count, the groups that stay, the duplicates and the largest group.
const FlagSpec DEDUP_FLAGS[] = {{"--min-seq-id", 'U', 0, 0}, {"-k", 'U', 0, 0}, {"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0}, {0, 0, 0, 0}};
// no contigs: the header line alone.  The set of ps is the one without the duplicates afterwards.
void dedupTable(cdm_ctx *ctx, const Frame &c, PileSet &ps, const std::string &outPath, Laps &laps) {
    std::string text = "name\tkey\tlength\trecords\tcounted\tkept\tduplicates\tlargest\n";
    if (c.nc) {
        std::vector<uint64_t> off(cdm_seqdb_size(ps.both) + 1), stats(c.nc * 4);
        check(cdm_alns_download(ctx, ps.alns, off.data(), NULL), "download of the set's offsets");
        dedupSet(ctx, ps, c, stats.data());
        for (uint64_t i = 0; i < c.nc; i++) {
            c.row(text, i); put(text, off[i + 1] - off[i]);
            for (int col = 0; col < 4; col++) put(text, stats[i * 4 + col]);
            text.push_back('\n');
        }
        laps.lap("duplicate report: groups, table");
    }
    writeOrDie(&outPath, text);
}

// The rescued reads of a PileSet that kept its hits: cdm_pileup_gapped over the contigs with nucleotide.out's scores and the gap
// costs of `align`; candidates and gapLetters: the sums of the per-contig statistics.
struct Rescued {
    cdm_gap_rec *recs = NULL; uint32_t *ops = NULL, *words = NULL; uint64_t n = 0, nOps = 0, nWords = 0, candidates = 0, gapLetters = 0; float ms = 0.f;
    Rescued() = default;
    Rescued(const Rescued &) = delete;
    void release() { cdm_gap_free(recs, ops, words); recs = NULL; ops = words = NULL; }
    ~Rescued() { release(); }
};
void rescueReads(cdm_ctx *ctx, const PileSet &ps, const Frame &c, const GapOpts &g, Rescued &r) {
    cdm_gap_params gp;
    gp.min_seq_id = 0.0f; gp.skip_extended_targets = 1; gp.band = (uint32_t) g.band; gp.min_columns = (uint32_t) g.minColumns;
    gp.min_id_permille = (uint32_t) (g.minSeqId * 1000 + 0.5); gp.match = 2; gp.mismatch = -3; gp.gap_open = 5; gp.gap_extend = 2;
    std::vector<uint64_t> gstats(c.nc * 4);
    check(cdm_pileup_gapped(ctx, ps.both, ps.hits, ps.alns, c.q.data(), c.nc, &gp, gstats.data(), &r.recs, &r.n, &r.ops, &r.nOps, &r.words, &r.nWords, &r.ms), "gapped pile-up");
    for (uint64_t i = 0; i < c.nc; i++) { r.candidates += gstats[i * 4]; r.gapLetters += gstats[i * 4 + 2]; }
}
// One of the three table reductions (depth, base counts, break points) over the records of a set, and over the rescued reads as well
// when gap.on: plain(&ms) or gapped(rescued, &ms) makes the library call.  The timing line names what the reduction found (items,
// NULL: nothing to name) and its kernels.
template <class Plain, class Gapped>
void tableReduction(cdm_ctx *ctx, const PileSet &ps, const Frame &c, const GapOpts &gap, const char *report, const char *items, const uint64_t *nItems, const char *kernels, Plain plain, Gapped gapped) {
    Rescued r; float ms = 0.f;
    if (gap.on) { rescueReads(ctx, ps, c, gap, r); gapped(r, &ms); }
    else plain(&ms);
    if (!getenv("CDM_TIMING")) return;
    char line[512]; size_t n = 0;
    n += snprintf(line + n, sizeof(line) - n, "  %s report: %llu records", report, (unsigned long long) cdm_alns_count(ps.alns));
    if (gap.on) n += snprintf(line + n, sizeof(line) - n, ", %llu candidates, %llu rescued", (unsigned long long) r.candidates, (unsigned long long) r.n);
    if (items) n += snprintf(line + n, sizeof(line) - n, ", %llu %s", (unsigned long long) *nItems, items);
    if (gap.on) n += snprintf(line + n, sizeof(line) - n, ", gapped kernels %.3f ms", r.ms);
    fprintf(stderr, "%s, %s kernels %.3f ms\n", line, kernels, ms);
}
// A device DB's sequences as the device compares them: their packed codes and N bits come down, no byte of the input is looked at.
struct PackedLetters {
    std::vector<uint32_t> codes, lens; std::vector<uint16_t> nbits; std::vector<uint64_t> woff;
    PackedLetters(cdm_ctx *ctx, cdm_seqdb *db, const char *what) : codes(cdm_seqdb_words(db) + 1), lens(cdm_seqdb_size(db)), nbits(codes.size()), woff(lens.size() + 1, 0) {
        check(cdm_seqdb_export_packed(ctx, db, codes.data(), nbits.data(), lens.data(), NULL, NULL, NULL, NULL), what);
        for (size_t i = 0; i < lens.size(); i++) woff[i + 1] = woff[i] + (lens[i] + 15u) / 16u;      // (every sequence starts on a word boundary: 16 letters a code word, 16 N bits beside it)
    }
    // letters [from, from + n) of sequence s behind `to`; reverse: the other strand, complemented from the stretch's end
    void append(std::string &to, uint64_t s, uint32_t from, uint32_t n, bool reverse) const {
        const uint32_t *cw = codes.data() + woff[s]; const uint16_t *nw = nbits.data() + woff[s];
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t p = from + (reverse ? n - 1u - i : i), b = (cw[p >> 4] >> ((p & 15u) * 2u)) & 3u;
            to.push_back((nw[p >> 4] >> (p & 15u)) & 1u ? 'N' : LETTER[reverse ? 3u - b : b]);
        }
    }
};
// bedGraph lines of one contig's runs of equal value, zero runs included: name, start, end (0-based, half-open), value
void bedGraphRuns(std::string &to, const std::string &name, const uint32_t *d, uint32_t len) {
    for (uint32_t start = 0, p = 1; p <= len; p++)
        if (p == len || d[p] != d[start]) { to += name; put(to, start); put(to, p); put(to, d[start]); to.push_back('\n'); start = p; }
}
// the contigs' own bytes (raw plane included): contig i from at[i], lens[i] + 1 bytes
std::string contigLetters(cdm_ctx *ctx, const Frame &c, std::vector<uint64_t> &at) {
    at.assign(c.nc + 1, 0);
    for (uint64_t i = 0; i < c.nc; i++) at[i + 1] = at[i] + c.lens[i] + 1ull;
    std::string letters(at.back(), '\0');
    check(cdm_seqdb_download(ctx, c.set->db, &letters[0], at.data()), "download of the contigs");
    return letters;
}
// ---- contig_damage: per-contig coverage and damage tables, cdm_pileup_profile over the contigs.  One TSV line per contig.
const FlagSpec DAMAGE_FLAGS[] = {{"--damage-ends", 'U', 0, 0}, {"--dedup", 'U', 0, 0}, {"--min-seq-id", 'U', 0, 0}, {"-k", 'U', 0, 0}, {"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0}, {0, 0, 0, 0}};
void damageTable(cdm_ctx *ctx, const Frame &c, const PileSet &ps, long ends, const std::string &outPath, Laps &laps) {
    std::string text = "name\tkey\tlength\treads\tcolumns";
    for (long d = 1; d <= ends; d++) { const std::string n = std::to_string(d); text += "\t5p_C_" + n + "\t5p_CT_" + n + "\t3p_G_" + n + "\t3p_GA_" + n; }
    text += "\n";
    if (c.nc) {
        const size_t cells = (size_t) 2 * (size_t) ends * 16;
        std::vector<uint64_t> counts(c.nc * cells), nReads(c.nc), nCols(c.nc);
        cdm_pileup_params pp; pp.ends = (int32_t) ends; pp.min_seq_id = 0.0f; pp.skip_extended_targets = 1;
        check(cdm_pileup_profile(ctx, ps.both, ps.alns, c.q.data(), c.nc, &pp, counts.data(), nReads.data(), nCols.data()), "pile-up profile");
        if (getenv("CDM_TIMING")) fprintf(stderr, "  damage report: %llu records, pile-up kernel %.3f ms\n", (unsigned long long) cdm_alns_count(ps.alns), cdm_ctx_last_kernel_ms(ctx, 16));
        for (uint64_t i = 0; i < c.nc; i++) {
            c.row(text, i); put(text, nReads[i]); put(text, nCols[i]);
            const uint64_t *c5 = counts.data() + i * cells, *c3 = c5 + (size_t) ends * 16;
            for (long d = 0; d < ends; d++) {       // [d][x][y], A,C,G,T = 0..3: C under any read base / under T; G under any / under A
                const uint64_t *cc = c5 + d * 16 + 1 * 4, *g = c3 + d * 16 + 2 * 4;
                put(text, cc[0] + cc[1] + cc[2] + cc[3]); put(text, cc[3]); put(text, g[0] + g[1] + g[2] + g[3]); put(text, g[0]);
            }
            text.push_back('\n');
        }
        laps.lap("damage report: pile-up, table");
    }
    writeOrDie(&outPath, text);
}
// ---- contig_depth: per-contig depth, breadth and depth variance, cdm_pileup_depth over the contigs per read set.  One TSV line per
// contig: the caller divides (mean = sum / window, variance = (sumsq - sum^2 / window) / (window - 1)).
const FlagSpec DEPTH_FLAGS[] = {{"--depth-edge", 'U', 0, 0}, {"--dedup", 'U', 0, 0}, {"--min-seq-id", 'U', 0, 0}, {"-k", 'U', 0, 0}, {"--depth-track", 'U', 0, 0}, {"--gapped", 'U', 0, 0}, {"--gap-band", 'U', 0, 0}, {"--gap-min-columns", 'U', 0, 0}, {"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0}, {0, 0, 0, 0}};
// one read set's statistics (nc x 8) and, when asked for, the depth of every contig position back to back
void depthSample(cdm_ctx *ctx, const Frame &c, const PileSet &ps, long edge, const GapOpts &gap, std::vector<uint64_t> &stats, std::vector<uint32_t> *track) {
    stats.assign(c.nc * 8, 0);
    if (track) track->assign(cdm_seqdb_residues(c.set->db) + 1, 0);
    uint32_t *const tr = track ? track->data() : NULL;
    cdm_depth_params dp; dp.edge = (int32_t) edge; dp.min_seq_id = 0.0f; dp.skip_extended_targets = 1;
    tableReduction(ctx, ps, c, gap, "depth", NULL, NULL, "depth",
        [&](float *ms) { check(cdm_pileup_depth(ctx, ps.both, ps.alns, c.q.data(), c.nc, &dp, stats.data(), tr), "pile-up depth"); *ms = cdm_ctx_last_kernel_ms(ctx, 17); },
        [&](const Rescued &r, float *ms) { check(cdm_pileup_depth_gapped(ctx, ps.both, ps.alns, c.q.data(), c.nc, r.recs, r.n, r.ops, r.nOps, &dp, stats.data(), tr, ms), "pile-up depth"); });
}
// the depth TSV of the read sets and, when asked for, the bedGraph of the runs of equal depth; no contigs: the header line alone, an empty track
void depthFiles(const Frame &c, const std::vector<std::vector<uint64_t>> &stats, const std::string &outPath, const std::string *trackOut, const std::vector<uint32_t> &track) {
    std::string text = "name\tkey\tlength\twindow", bed, tmp;
    static const char *const COLS[7] = {"reads", "columns", "breadth", "covered", "sum", "sumsq", "max"};
    static const int AT[7] = {0, 1, 2, 4, 5, 6, 7};
    for (size_t s = 1; s <= stats.size(); s++) for (const char *col : COLS) text += std::string("\t") + col + "_" + std::to_string(s);
    text += "\n";
    uint64_t at = 0;
    for (uint64_t i = 0; i < c.nc; at += c.lens[i], i++) {
        c.row(text, i); put(text, stats[0][i * 8 + 3]);
        for (const auto &sample : stats) for (int col : AT) put(text, sample[i * 8 + col]);
        text.push_back('\n');
        if (trackOut) bedGraphRuns(bed, c.name(i, tmp), track.data() + at, c.lens[i]);
    }
    writeOrDie(&outPath, text);
    writeOrDie(trackOut, bed);
}
// ---- contig_variants: per-position base counts and variant sites, cdm_pileup_bases over the contigs: one summary line per contig,
// with --sites one line per position where the reads disagree with the contig (D) or among themselves (V), with --consensus the
// contigs with the reads' majority letter at the D positions.  No call where no read seeds.
const FlagSpec VARIANT_FLAGS[] = {{"--min-depth", 'U', 0, 0}, {"--min-alt-count", 'U', 0, 0}, {"--min-alt-percent", 'U', 0, 0}, {"--mask-ends", 'U', 0, 0}, {"--sites", 'U', 0, 0},
                                  {"--consensus", 'U', 0, 0}, {"--gapped", 'U', 0, 0}, {"--gap-band", 'U', 0, 0}, {"--gap-min-columns", 'U', 0, 0}, {"--min-seq-id", 'U', 0, 0}, {"-k", 'U', 0, 0}, {"--threads", 'N', 0, 0},
                                  {"-v", 'N', 0, 0}, {"--dedup", 'U', 0, 0}, {0, 0, 0, 0}};
// no contigs: the summary's header line alone, an empty sites file, an empty FASTA
void variantReport(cdm_ctx *ctx, const Frame &c, const PileSet &ps, const VariantOut &v, Laps &laps) {
    std::string text = "name\tkey\tlength\treads\tcolumns\tbases\tmismatches\tcalled\tdiffers\tvariable\n", sitesText, fasta;
    if (c.nc) {
        std::vector<uint64_t> stats(c.nc * 8);
        cdm_bases_params bp; bp.mask_ends = (int32_t) v.opt.maskEnds; bp.min_depth = (int32_t) v.opt.minDepth; bp.min_alt_count = (int32_t) v.opt.minAltCount;
        bp.min_alt_percent = (int32_t) v.opt.minAltPercent; bp.min_seq_id = 0.0f; bp.skip_extended_targets = 1;
        const bool wantSites = v.sites || v.consensus;
        cdm_site *sites = NULL; uint64_t nSites = 0;
        cdm_site **const sitesTo = wantSites ? &sites : NULL; uint64_t *const nSitesTo = wantSites ? &nSites : NULL;
        tableReduction(ctx, ps, c, v.gap, "variant", "sites", &nSites, "base count",
            [&](float *ms) { check(cdm_pileup_bases(ctx, ps.both, ps.alns, c.q.data(), c.nc, &bp, stats.data(), NULL, sitesTo, nSitesTo, ms), "pile-up base counts"); },
            [&](const Rescued &r, float *ms) { check(cdm_pileup_bases_gapped(ctx, ps.both, ps.alns, c.q.data(), c.nc, r.recs, r.n, r.ops, r.nOps, &bp, stats.data(), NULL, sitesTo, nSitesTo, ms), "pile-up base counts"); });
        std::string tmp;
        for (uint64_t i = 0; i < c.nc; i++) {
            c.row(text, i);
            for (int col = 0; col < 7; col++) put(text, stats[i * 8 + col]);
            text.push_back('\n');
        }
        if (v.sites)
            for (uint64_t k = 0; k < nSites; k++) {     // name, pos (1-based), ref, major, flags, depth, forward A C G T, reverse a c g t
                const cdm_site &st = sites[k];
                const uint32_t fl = st.info >> 8;
                sitesText += c.name(st.query, tmp);
                put(sitesText, (unsigned long long) st.pos + 1);
                sitesText.push_back('\t'); sitesText.push_back(LETTER[st.info & 15u]);
                sitesText.push_back('\t'); sitesText.push_back(LETTER[(st.info >> 4) & 15u]);
                sitesText.push_back('\t'); if (fl & CDM_SITE_DIFFERS) sitesText.push_back('D'); if (fl & CDM_SITE_VARIABLE) sitesText.push_back('V');
                unsigned long long d = 0; for (uint32_t n : st.counts) d += n;
                put(sitesText, d);
                for (uint32_t n : st.counts) put(sitesText, n);
                sitesText.push_back('\n');
            }
        if (v.consensus) {      // the contigs' own bytes, the reads' majority letter at the D positions
            std::vector<uint64_t> at;
            std::string letters = contigLetters(ctx, c, at);
            for (uint64_t k = 0; k < nSites; k++)
                if ((sites[k].info >> 8) & CDM_SITE_DIFFERS) letters[at[sites[k].query] + sites[k].pos] = LETTER[(sites[k].info >> 4) & 15u];
            for (uint64_t i = 0; i < c.nc; i++) { fasta.push_back('>'); fasta += c.name(i, tmp); fasta.push_back('\n'); fasta.append(letters, at[i], c.lens[i] + 1ull); }
        }
        cdm_sites_free(sites);
        laps.lap("variant report: base counts, tables");
    }
    writeOrDie(v.summary, text); writeOrDie(v.sites, sitesText); writeOrDie(v.consensus, fasta);
}
// ---- contig_breaks: contig break points from spanning reads, cdm_pileup_breaks over the contigs: one summary line per contig and,
// behind it, one `#break` line per run of boundaries that too few reads span with --break-anchor columns on either side (J: the reads
// cover the stretch and none spans it - the signature of a chimeric join; G: a stretch without reads); with --split the contigs cut
// at their breaks, with --span-track the spanning coverage of every boundary.  Reads shorter than twice the anchor span nothing, and
// there is no break call where no read seeds.
const FlagSpec BREAK_FLAGS[] = {{"--break-anchor", 'U', 0, 0}, {"--break-edge", 'U', 0, 0}, {"--min-span", 'U', 0, 0}, {"--min-span-percent", 'U', 0, 0}, {"--split", 'U', 0, 0},
                                {"--min-piece", 'U', 0, 0}, {"--span-track", 'U', 0, 0}, {"--dedup", 'U', 0, 0}, {"--gapped", 'U', 0, 0}, {"--gap-band", 'U', 0, 0}, {"--gap-min-columns", 'U', 0, 0}, {"--min-seq-id", 'U', 0, 0}, {"-k", 'U', 0, 0}, {"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0}, {0, 0, 0, 0}};
// no contigs: the summary's header line alone, an empty FASTA, an empty track
void breakReport(cdm_ctx *ctx, const Frame &c, const PileSet &ps, const BreakOut &o, Laps &laps) {
    std::string text = "name\tkey\tlength\treads\tcolumns\twindow\tweak\tbreaks\tjoins\tmin_span\tsum_span\n", fasta, bed;
    if (c.nc) {
        std::vector<uint32_t> track;
        std::vector<uint64_t> stats(c.nc * 8);
        if (o.track) track.assign(cdm_seqdb_residues(c.set->db) + 1, 0);
        uint32_t *const tr = o.track ? track.data() : NULL;
        cdm_breaks_params bp; bp.anchor = (int32_t) o.opt.anchor; bp.edge = (int32_t) o.opt.edge; bp.min_span = (int32_t) o.opt.minSpan; bp.min_span_percent = (int32_t) o.opt.minSpanPercent;
        bp.min_seq_id = 0.0f; bp.skip_extended_targets = 1;
        cdm_break *br = NULL; uint64_t nBr = 0;
        tableReduction(ctx, ps, c, o.gap, "break", "breaks", &nBr, "break point",
            [&](float *ms) { check(cdm_pileup_breaks(ctx, ps.both, ps.alns, c.q.data(), c.nc, &bp, stats.data(), tr, &br, &nBr, ms), "pile-up break points"); },
            [&](const Rescued &r, float *ms) { check(cdm_pileup_breaks_gapped(ctx, ps.both, ps.alns, c.q.data(), c.nc, r.recs, r.n, r.ops, r.nOps, &bp, stats.data(), tr, &br, &nBr, ms), "pile-up break points"); });
        std::string tmp, letters;
        std::vector<uint64_t> at;
        if (o.split) letters = contigLetters(ctx, c, at);
        uint64_t k = 0, trackAt = 0;
        for (uint64_t i = 0; i < c.nc; trackAt += c.lens[i], i++) {
            const std::string &name = c.name(i, tmp);
            c.row(text, i);
            for (int col = 0; col < 8; col++) put(text, stats[i * 8 + col]);
            text.push_back('\n');
            const uint64_t k0 = k;
            for (; k < nBr && br[k].query == i; k++) {      // 1-based boundaries
                const cdm_break &b = br[k];
                text += "#break\t"; text += name;
                put(text, (unsigned long long) b.first + 1); put(text, (unsigned long long) b.last + 1); put(text, b.min_span); put(text, b.uncovered); put(text, b.depth_left); put(text, b.depth_right);
                text.push_back('\t'); text.push_back(b.flags & CDM_BREAK_GAP ? 'G' : 'J'); text.push_back('\n');
            }
            if (o.split) {      // a piece ends at position first - 1, the next begins at position last: the letters between, which no read spans, are dropped
                uint64_t from = 0, piece = 0;
                for (uint64_t j = k0; j <= k; j++) {
                    const uint64_t to = j < k ? br[j].first : c.lens[i];
                    piece++;
                    if (to - from >= (uint64_t) o.minPiece) {
                        fasta.push_back('>'); fasta += name;
                        if (k > k0) { fasta.push_back('_'); fasta += std::to_string(piece); }
                        fasta.push_back('\n'); fasta.append(letters, at[i] + from, to - from); fasta.push_back('\n');
                    }
                    if (j < k) from = br[j].last;
                }
            }
            if (o.track) bedGraphRuns(bed, name, track.data() + trackAt, c.lens[i]);      // the runs of equal span
        }
        cdm_breaks_free(br);
        laps.lap("break report: break points, tables");
    }
    writeOrDie(o.summary, text); writeOrDie(o.split, fasta); writeOrDie(o.track, bed);
}
// ---- contig_map: the reads on the contigs as a SAM file, cdm_pileup_map over the contigs: one line per counted record in coordinate
// order, soft clips around the overlap, NM and MD from the mismatch words, one primary line per read.  SEQ is the read as the device
// compared it - the letters its codes and N bits stand for - so SEQ, CIGAR and MD agree by construction.  No line for a read that
// seeds nowhere.  --gapped 1: the rescued reads come as lines of their own (CIGAR with I and D, MD with ^, a trailing
// XG:i:<gap letters>), merged into the others by (contig, position), the ungapped line first on equal keys.
const FlagSpec MAP_FLAGS[] = {{"--read-group", 'U', 0, 0}, {"--primary-only", 'U', 0, 0}, {"--dedup", 'U', 0, 0}, {"--gapped", 'U', 0, 0}, {"--gap-band", 'U', 0, 0}, {"--gap-min-columns", 'U', 0, 0}, {"--min-seq-id", 'U', 0, 0}, {"-k", 'U', 0, 0}, {"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0}, {0, 0, 0, 0}};
// SAM names a reference sequence once, and so does a link: two contigs of one name end the command
void mapCheckNames(const SeqSet &contigs, const char *module = "contig_map", const char *what = "a SAM file") {
    std::vector<std::string> names; std::string tmp;
    for (uint64_t i = 0; i < contigs.keys.size(); i++) names.push_back(seqName(contigs, i, tmp));
    std::sort(names.begin(), names.end());
    for (size_t i = 1; i < names.size(); i++)
        if (names[i] == names[i - 1]) die(std::string(module) + ": two contigs are named " + names[i] + "; " + what + " can not tell them apart");
}
// no contigs: the header lines without @SQ
void mapReport(cdm_ctx *ctx, const Frame &c, const SeqSet *reads, const PileSet &ps, const MapOut &o, Laps &laps) {
    std::string text = "@HD\tVN:1.6\tSO:coordinate\n", tmp;
    std::vector<std::string> part;        // the record lines, a chunk a host thread
    const uint64_t nc = c.nc;
    for (uint64_t i = 0; i < nc; i++) { text += "@SQ\tSN:"; text += c.name(i, tmp); text += "\tLN:"; put(text, c.lens[i], false); text.push_back('\n'); }
    if (o.readGroup) text += "@RG\tID:" + *o.readGroup + "\n";
    text += "@PG\tID:carpedeam\tPN:carpedeam\n";
    if (nc) {
        std::vector<uint64_t> stats(nc * 4);
        cdm_map_params mp; mp.min_seq_id = 0.0f; mp.skip_extended_targets = 1;
        cdm_map_rec *recs = NULL; uint32_t *mism = NULL; uint64_t nRecs = 0, nMism = 0; float ms = 0.f;
        check(cdm_pileup_map(ctx, ps.both, ps.alns, c.q.data(), nc, &mp, stats.data(), &recs, &nRecs, &mism, &nMism, &ms), "pile-up map");
        if (getenv("CDM_TIMING")) fprintf(stderr, "  map report: %llu records, %llu lines, %llu mismatches, map kernels %.3f ms\n", (unsigned long long) cdm_alns_count(ps.alns), (unsigned long long) nRecs, (unsigned long long) nMism, ms);
        // --gapped 1: the rescued reads, and the order of the two streams merged by (contig, pos), an ungapped record first on equal keys
        // (entry: index << 1 | rescued)
        Rescued g;
        std::vector<uint64_t> merged;
        if (o.gap.on) {
            rescueReads(ctx, ps, c, o.gap, g);
            if (getenv("CDM_TIMING")) fprintf(stderr, "  map report: %llu refused hits aligned, %llu rescued with %llu gap letters, gapped kernels %.3f ms\n", (unsigned long long) g.candidates, (unsigned long long) g.n, (unsigned long long) g.gapLetters, g.ms);
            merged.reserve(nRecs + g.n);
            for (uint64_t i = 0, j = 0; i < nRecs || j < g.n;) {
                const bool plain = j == g.n || (i < nRecs && (recs[i].query < g.recs[j].query || (recs[i].query == g.recs[j].query && recs[i].pos <= g.recs[j].pos)));
                merged.push_back(plain ? i++ << 1 : j++ << 1 | 1u);
            }
        }
        const uint64_t nLines = nRecs + g.n;
        const PackedLetters letters(ctx, reads->db, "download of the reads");
        // the lines on the host threads, in contiguous chunks of records
        const int T = std::max(1, omp_get_max_threads());
        part.resize((size_t) T);
#pragma omp parallel for schedule(static, 1) num_threads(T)     // a loop over the chunks: a smaller team still visits them all
        for (int t = 0; t < T; t++) {
            std::string &to = part[(size_t) t]; std::string name;
            // what the two kinds of line share: QNAME to MAPQ in front of CIGAR; RNEXT to SEQ behind it; QUAL, NM, MD from the words of
            // the record (a mismatch, or a deleted letter, which joins the ^ in front of it when it follows a deleted letter on the contig)
            // over `span` contig letters, and RG
            auto lineHead = [&](uint32_t target, uint32_t flags, uint32_t query, uint32_t pos) {
                to += seqName(*reads, (uint64_t) target - nc, name);       // (reads only as targets: behind the contigs in the joint DB)
                to.push_back('\t'); put(to, (flags & CDM_MAP_REVERSE ? 16u : 0u) | (flags & CDM_MAP_SECONDARY ? 256u : 0u), false);
                to.push_back('\t'); to += c.name(query, name);
                to.push_back('\t'); put(to, (unsigned long long) pos + 1, false);
                to += "\t255\t";
            };
            auto lineSeq = [&](uint32_t target, uint32_t tlen, uint32_t flags) {       // the read in the contig's orientation
                to += "\t*\t0\t0\t";
                letters.append(to, (uint64_t) target - nc, 0, tlen, (flags & CDM_MAP_REVERSE) != 0);
            };
            auto lineTail = [&](uint32_t nm, const uint32_t *words, uint32_t nWords, uint32_t span) {
                to += "\t*\tNM:i:"; put(to, nm, false);
                to += "\tMD:Z:";
                uint32_t from = 0; bool inDeletion = false;
                for (uint32_t j = 0; j < nWords; j++) {     // the matches in front of a word, then the contig's letter there
                    const uint32_t w = words[j], col = w & 0xFFFFFFu; const bool deleted = (w >> 28) == 15u;
                    if (!(deleted && inDeletion && col == from)) { put(to, col - from, false); if (deleted) to.push_back('^'); }
                    to.push_back(LETTER[std::min(4u, (w >> 24) & 15u)]);
                    from = col + 1u; inDeletion = deleted;
                }
                put(to, span - from, false);
                if (o.readGroup) { to += "\tRG:Z:"; to += *o.readGroup; }
            };
            for (uint64_t k = nLines * (uint64_t) t / (uint64_t) T, end = nLines * (uint64_t) (t + 1) / (uint64_t) T; k < end; k++) {
                const uint64_t entry = o.gap.on ? merged[k] : k << 1;
                if (entry & 1u) {       // a rescued read: CIGAR from its operations, XG the gap letters
                    const cdm_gap_rec &r = g.recs[entry >> 1];
                    if (o.primaryOnly && (r.flags & CDM_MAP_SECONDARY)) continue;
                    lineHead(r.target, r.flags, r.query, r.pos);
                    if (r.tstart) { put(to, r.tstart, false); to.push_back('S'); }
                    uint32_t gaps = 0;
                    for (uint32_t j = 0; j < r.n_ops; j++) {
                        const uint32_t w = g.ops[r.ops + j];
                        put(to, w >> 2, false); to.push_back("MID"[w & 3u]);
                        if (w & 3u) gaps += w >> 2;
                    }
                    if (const uint32_t right = r.tlen - r.tstart - r.columns) { put(to, right, false); to.push_back('S'); }
                    lineSeq(r.target, r.tlen, r.flags);
                    lineTail(r.nm, g.words + r.words, r.n_words, r.span);
                    to += "\tXG:i:"; put(to, gaps, false);
                    to.push_back('\n');
                    continue;
                }
                const cdm_map_rec &r = recs[entry >> 1];
                if (o.primaryOnly && (r.flags & CDM_MAP_SECONDARY)) continue;
                lineHead(r.target, r.flags, r.query, r.pos);
                const uint32_t right = r.tlen - r.tstart - r.columns;
                if (r.tstart) { put(to, r.tstart, false); to.push_back('S'); }
                put(to, r.columns, false); to.push_back('M');
                if (right) { put(to, right, false); to.push_back('S'); }
                lineSeq(r.target, r.tlen, r.flags);
                lineTail(r.nm, mism + r.mm, r.nm, r.columns);
                to.push_back('\n');
            }
        }
        g.release();
        cdm_map_free(recs, mism);
        laps.lap("map report: records, lines");
    }
    // the header, then the chunks in order: the text is never joined in memory
    FILE *f = fopen(o.sam->c_str(), "w");
    bool ok = f != NULL && fwrite(text.data(), 1, text.size(), f) == text.size();
    for (size_t t = 0; ok && t < part.size(); t++) { ok = fwrite(part[t].data(), 1, part[t].size(), f) == part[t].size(); std::string().swap(part[t]); }
    if (f && fclose(f) != 0) ok = false;
    if (!ok) die("Could not write " + *o.sam);
}
// ---- contig_indels: insertion and deletion sites of the contigs and the contigs polished at them.  The chain of contig_map
// --gapped 1, then cdm_pileup_indels over the contigs: one summary line per contig, with --sites one line per supported insertion or
// deletion (S) and whether more than half of the crossing reads carry it (M), with --consensus the contigs with their M sites applied.
// Substitutions are not touched: contig_variants --consensus does those.  A read seeded twice on one contig counts twice, as it has
// two SAM lines.  The defaults are those of contig_variants' second allele, reasoned, not measured.
const FlagSpec INDEL_FLAGS[] = {{"--min-depth", 'U', 0, 0}, {"--min-indel-count", 'U', 0, 0}, {"--min-indel-percent", 'U', 0, 0}, {"--gap-band", 'U', 0, 0}, {"--gap-min-columns", 'U', 0, 0},
                                {"--sites", 'U', 0, 0}, {"--consensus", 'U', 0, 0}, {"--min-seq-id", 'U', 0, 0}, {"-k", 'U', 0, 0}, {"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0}, {0, 0, 0, 0}};
// no contigs: the summary's header line alone, an empty sites file, an empty FASTA
void indelReport(cdm_ctx *ctx, const Frame &c, const PileSet &ps, const IndelOut &o, Laps &laps) {
    std::string text = "name\tkey\tlength\treads\tcolumns\trescued\tinsertions\tdeletions\tinserted_letters\tdeleted_letters\tplaces\tsupported\tmajor\tapplied\tnew_length\n", sitesText, fasta;
    if (c.nc) {
        std::vector<uint64_t> stats(c.nc * 10);
        Rescued g; float ms = 0.f;
        rescueReads(ctx, ps, c, o.gap, g);
        cdm_indel_params ip; ip.min_depth = (int32_t) o.minDepth; ip.min_count = (int32_t) o.minCount; ip.min_percent = (int32_t) o.minPercent; ip.min_seq_id = 0.0f; ip.skip_extended_targets = 1;
        cdm_indel_site *sites = NULL; uint8_t *codes = NULL; uint64_t nSites = 0, nCodes = 0;
        check(cdm_pileup_indels(ctx, ps.both, ps.alns, c.q.data(), c.nc, g.recs, g.n, g.ops, g.nOps, &ip, stats.data(), NULL, &sites, &nSites, &codes, &nCodes, &ms), "pile-up indel sites");
        if (getenv("CDM_TIMING")) fprintf(stderr, "  indel report: %llu records, %llu rescued, %llu sites, gapped kernels %.3f ms, indel kernels %.3f ms\n", (unsigned long long) cdm_alns_count(ps.alns), (unsigned long long) g.n, (unsigned long long) nSites, g.ms, ms);
        g.release();
        std::string tmp;
        if (o.sites) {      // name, pos (1-based), kind, length, letters, count, cross, others, flags; a deletion shows the contig's letters as the device compared them
            const PackedLetters own(ctx, c.set->db, "download of the contigs' codes");
            for (uint64_t k = 0; k < nSites; k++) {
                const cdm_indel_site &st = sites[k];
                const uint32_t kind = st.info & 15u, len = (st.info >> 4) & 0xFFFu, fl = st.info >> 16;
                sitesText += c.name(st.query, tmp);
                put(sitesText, (unsigned long long) st.pos + 1);
                sitesText.push_back('\t'); sitesText.push_back(kind == CDM_INDEL_INS ? 'I' : 'D');
                put(sitesText, len);
                sitesText.push_back('\t');
                if (kind == CDM_INDEL_INS) for (uint32_t j = 0; j < st.n_letters; j++) sitesText.push_back(LETTER[std::min<uint32_t>(4u, codes[st.letters + j])]);
                else own.append(sitesText, st.query, st.pos, len, false);
                put(sitesText, st.count); put(sitesText, st.cross); put(sitesText, st.others);
                sitesText.push_back('\t'); sitesText.push_back('S'); if (fl & CDM_INDEL_MAJOR) sitesText.push_back('M');
                sitesText.push_back('\n');
            }
        }
        // the polished contigs: the M sites in site order behind a cursor; a site inside a stretch an earlier deletion removed is skipped
        std::vector<uint64_t> at;
        std::string letters;
        if (o.consensus) letters = contigLetters(ctx, c, at);
        uint64_t k = 0;
        for (uint64_t i = 0; i < c.nc; i++) {
            uint64_t next = 0, applied = 0, newLen = 0;
            if (o.consensus) { fasta.push_back('>'); fasta += c.name(i, tmp); fasta.push_back('\n'); }
            for (; k < nSites && sites[k].query == i; k++) {
                const cdm_indel_site &st = sites[k];
                if (!((st.info >> 16) & CDM_INDEL_MAJOR) || st.pos < next) continue;
                if (o.consensus) fasta.append(letters, at[i] + next, st.pos - next);
                newLen += st.pos - next; applied++;
                if ((st.info & 15u) == CDM_INDEL_INS) {
                    if (o.consensus) for (uint32_t j = 0; j < st.n_letters; j++) fasta.push_back(LETTER[std::min<uint32_t>(4u, codes[st.letters + j])]);
                    newLen += st.n_letters; next = st.pos;
                } else next = (uint64_t) st.pos + ((st.info >> 4) & 0xFFFu);
            }
            if (o.consensus) fasta.append(letters, at[i] + next, c.lens[i] + 1ull - next);        // (with the byte that ends the contig)
            newLen += c.lens[i] - next;
            c.row(text, i);
            for (int col = 0; col < 10; col++) put(text, stats[i * 10 + col]);
            put(text, applied); put(text, newLen);
            text.push_back('\n');
        }
        cdm_indel_free(sites, codes);
        laps.lap("indel report: gapped records, sites, tables");
    }
    writeOrDie(o.summary, text); writeOrDie(o.sites, sitesText); writeOrDie(o.consensus, fasta);
}
// ---- contig_links: which contig ends belong together, cdm_pileup_links over the contigs.  One TSV line per link: the two contigs with
// their orientations, the reads that bridge them, those seen in the canonical direction, and the gap between the two ends (negative:
// the overlap) as the most frequent value with its count, the minimum, the maximum and the sum.  With --ends one line per contig with its
// end records, with --gfa the contigs as segments and the links whose most frequent gap is an overlap or 0 as L lines (GFA 1 has no
// form for letters between two segments: those links are in the table only).  Rescued reads take no part, a contig is never linked to
// itself, and the letters of two overlapping ends are not compared: a link is what the reads say.  The defaults are reasoned, not
// measured: the anchor is contig_breaks'; an overhang of 1 letter is enough because a link needs the read's head record on a second
// contig anyway; two reads keep a lone chimeric read out.
const FlagSpec LINK_FLAGS[] = {{"--link-anchor", 'U', 0, 0}, {"--link-overhang", 'U', 0, 0}, {"--link-max-ends", 'U', 0, 0}, {"--min-link-reads", 'U', 0, 0}, {"--ends", 'U', 0, 0}, {"--gfa", 'U', 0, 0},
                               {"--dedup", 'U', 0, 0}, {"--min-seq-id", 'U', 0, 0}, {"-k", 'U', 0, 0}, {"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0}, {0, 0, 0, 0}};
// a signed integer behind a tab
void putSigned(std::string &to, long long v) { to.push_back('\t'); to += std::to_string(v); }
// no contigs: an empty table, an empty ends file, the GFA header line alone
void linkReport(cdm_ctx *ctx, const Frame &c, const PileSet &ps, const LinkOut &o, Laps &laps) {
    std::string text, endsText, gfa = "H\tVN:Z:1.0\n";
    if (c.nc) {
        std::vector<uint64_t> stats(c.nc * 6); uint64_t totals[5] = {0, 0, 0, 0, 0};
        cdm_links_params lp; lp.anchor = (int32_t) o.anchor; lp.overhang = (int32_t) o.overhang; lp.max_ends = (int32_t) o.maxEnds; lp.min_reads = (int32_t) o.minReads;
        lp.min_seq_id = 0.0f; lp.skip_extended_targets = 1;
        cdm_link *links = NULL; uint64_t nLinks = 0; float ms = 0.f;
        check(cdm_pileup_links(ctx, ps.both, ps.alns, c.q.data(), c.nc, &lp, stats.data(), totals, &links, &nLinks, &ms), "pile-up links");
        if (getenv("CDM_TIMING")) fprintf(stderr, "  link report: %llu records, %llu end records, %llu crowded reads, %llu pairs, %llu links, %llu returned, link kernels %.3f ms\n", (unsigned long long) cdm_alns_count(ps.alns),
                                          (unsigned long long) totals[0], (unsigned long long) totals[1], (unsigned long long) totals[3], (unsigned long long) totals[4], (unsigned long long) nLinks, ms);
        std::string tmp;
        // nameA oA nameB oB: the four columns a table line and an L line begin with
        auto edge = [&](std::string &to, const cdm_link &k) {
            to += c.name(k.a, tmp); to.push_back('\t'); to.push_back(k.info & 1u ? '-' : '+'); to.push_back('\t');
            to += c.name(k.b, tmp); to.push_back('\t'); to.push_back(k.info & 2u ? '-' : '+');
        };
        for (uint64_t k = 0; k < nLinks; k++) {
            const cdm_link &l = links[k];
            edge(text, l); put(text, l.reads); put(text, l.forward); putSigned(text, l.gap_mode); put(text, l.mode_reads); putSigned(text, l.gap_min); putSigned(text, l.gap_max); putSigned(text, l.gap_sum);
            text.push_back('\n');
        }
        if (o.ends)
            for (uint64_t i = 0; i < c.nc; i++) {
                c.row(endsText, i);
                for (int col = 0; col < 6; col++) put(endsText, stats[i * 6 + col]);
                endsText.push_back('\n');
            }
        if (o.gfa) {        // the contigs' own bytes
            std::vector<uint64_t> at;
            const std::string letters = contigLetters(ctx, c, at);
            for (uint64_t i = 0; i < c.nc; i++) {
                gfa += "S\t"; gfa += c.name(i, tmp); gfa.push_back('\t'); gfa.append(letters, at[i], c.lens[i]); gfa += "\tLN:i:"; put(gfa, c.lens[i], false); gfa.push_back('\n');
            }
            for (uint64_t k = 0; k < nLinks; k++) {
                const cdm_link &l = links[k];
                if (l.gap_mode > 0) continue;
                gfa += "L\t"; edge(gfa, l); put(gfa, (unsigned long long) -(long long) l.gap_mode); gfa += "M\tRC:i:"; put(gfa, l.reads, false); gfa.push_back('\n');
            }
        }
        cdm_link_free(links);
        laps.lap("link report: links, tables");
    }
    writeOrDie(o.table, text); writeOrDie(o.ends, endsText); writeOrDie(o.gfa, gfa);
}
// ---- contig_join: the contigs joined along their links.  contig_links' chain, then every returned link gets one decision (host/contig_join.h:
// A ambiguous, W weak, C contained, X the letters disagree, S short, O circle, J joined): cdm_pileup_links returns the links contig_links
// writes (min_reads is --min-link-reads: a lone chimeric read makes no end ambiguous), the links that pass A, W and C are the junctions of
// cdm_pileup_junctions with gap = gap_mode, and the paths of J links are written as one record each.  --join-overlap-percent 90 is reasoned,
// not measured: it is the identity the bridging reads themselves had to pass at --min-seq-id 0.9.
const FlagSpec JOIN_FLAGS[] = {{"--link-anchor", 'U', 0, 0}, {"--link-overhang", 'U', 0, 0}, {"--link-max-ends", 'U', 0, 0}, {"--min-link-reads", 'U', 0, 0}, {"--joined", 'U', 0, 0}, {"--paths", 'U', 0, 0},
                               {"--join-overlap-percent", 'U', 0, 0}, {"--dedup", 'U', 0, 0}, {"--min-seq-id", 'U', 0, 0}, {"-k", 'U', 0, 0}, {"--threads", 'N', 0, 0}, {"-v", 'N', 0, 0}, {0, 0, 0, 0}};
// no contigs: three empty files
void joinReport(cdm_ctx *ctx, const Frame &c, const PileSet &ps, const JoinOut &o, Laps &laps) {
    std::string text, fasta, pathsText;
    if (c.nc) {
        std::vector<uint64_t> stats(c.nc * 6); uint64_t totals[5] = {0, 0, 0, 0, 0};
        cdm_links_params lp; lp.anchor = (int32_t) o.anchor; lp.overhang = (int32_t) o.overhang; lp.max_ends = (int32_t) o.maxEnds; lp.min_reads = (int32_t) o.minLinkReads;
        lp.min_seq_id = 0.0f; lp.skip_extended_targets = 1;
        cdm_link *links = NULL; uint64_t nLinks = 0; float linkMs = 0.f, ms = 0.f;
        check(cdm_pileup_links(ctx, ps.both, ps.alns, c.q.data(), c.nc, &lp, stats.data(), totals, &links, &nLinks, &linkMs), "pile-up links");
        JoinPlan plan;
        joinFirst(links, nLinks, c.lens, o.minLinkReads, plan);
        std::vector<cdm_junction_res> res(plan.juncs.size());
        uint8_t *fills = NULL;
        check(cdm_pileup_junctions(ctx, ps.both, ps.alns, c.q.data(), c.nc, &lp, plan.juncs.data(), plan.juncs.size(), res.data(), &fills, NULL, &ms), "pile-up junctions");
        if (getenv("CDM_TIMING")) {
            unsigned long long voters = 0, letters = 0;
            for (const cdm_junction_res &r : res) { voters += r.voters; letters += r.fill_len; }
            fprintf(stderr, "  join report: %llu links, %llu junctions, %llu voters, %llu fill letters, link kernels %.3f ms, junction kernels %.3f ms\n", (unsigned long long) nLinks,
                    (unsigned long long) res.size(), voters, letters, linkMs, ms);
        }
        joinDecide(links, nLinks, c.lens, res.data(), fills, o.overlapPercent, plan);
        std::vector<std::string> names(c.nc); std::string tmp;
        for (uint64_t i = 0; i < c.nc; i++) names[i] = c.name(i, tmp);
        std::vector<uint64_t> at; std::string letters;
        if (o.joined) letters = contigLetters(ctx, c, at);
        const JoinContigs jc = {&names, &letters, &at, &c.lens};
        text = joinTable(jc, links, nLinks, res.data(), plan);
        if (o.joined) fasta = joinFasta(jc, plan);
        if (o.paths) pathsText = joinPaths(jc, plan);
        cdm_junction_free(fills, NULL);
        cdm_link_free(links);
        laps.lap("join report: links, junctions, paths");
    }
    writeOrDie(o.table, text); writeOrDie(o.joined, fasta); writeOrDie(o.paths, pathsText);
}
// A contig_* command: the usage line unless the positional arguments are right (argsOk), the flag check, what the command asks for
// from its flags (fill: every refusal, before a device is opened), the context and the contigs, then the command's read sets (body).
template <class Fill, class Body> int contigCommand(Args &a, const char *module, bool argsOk, const char *usage, const FlagSpec *flags, Fill fill, Body body) {
    if (!argsOk) die(usage);
    checkFlags(module, a, flags);
    PileAsk ask;
    fill(ask);
    Laps laps;
    cdm_ctx *ctx = openCtx();
    SeqSet contigs;
    const bool have = loadSeqSet(ctx, a.pos[0], false, true, contigs);
    body(ctx, have ? &contigs : NULL, ask, laps);
    if (contigs.db) cdm_seqdb_free(contigs.db);
    cdm_ctx_destroy(ctx);
    return EXIT_SUCCESS;
}
// the commands with one read set: exactly (or at least) three positional arguments
template <class Fill> int contigReport(Args &a, const char *module, bool exactly, const char *usage, const FlagSpec *flags, Fill fill) {
    return contigCommand(a, module, exactly ? a.pos.size() == 3 : a.pos.size() >= 3, usage, flags, fill, [&](cdm_ctx *ctx, const SeqSet *contigs, PileAsk &ask, Laps &laps) {
        SeqSet reads;
        if (contigs && !loadSeqSet(ctx, a.pos[1], true, ask.map != NULL, reads)) die(std::string(module) + ": " + a.pos[1] + " holds no reads");      // (the map's lines carry the reads' names)
        ask.mapReads = &reads;
        laps.lap("inputs read, sequences up");
        pileReports(ctx, contigs, reads.db, (int) iflag(a, "-k", 20), fflag(a, "--min-seq-id", 0.9f), ask, laps);
        if (reads.db) cdm_seqdb_free(reads.db);
    });
}
}  // namespace

void pileReports(cdm_ctx *ctx, const SeqSet *contigs, cdm_seqdb *reads, int kmerSize, float minSeqId, const PileAsk &ask, Laps &laps) {
    const Frame c(ctx, contigs);
    PileSet ps;
    if (c.nc) {
        if (ask.map) mapCheckNames(*contigs);
        if (ask.links) mapCheckNames(*contigs, "contig_links", "a link");
        if (ask.join) mapCheckNames(*contigs, "contig_join", "a join");
        const bool keepHits = (ask.map && ask.map->gap.on) || ask.indels || (ask.depthOut && ask.depthGap.on) || (ask.variants && ask.variants->gap.on) || (ask.breaks && ask.breaks->gap.on);
        ps = pileupAlignments(ctx, contigs->db, reads, kmerSize, minSeqId, keepHits);
        const std::pair<const void *, const char *> reports[] = {{ask.damageOut, "damage"}, {ask.depthOut, "depth"}, {ask.variants, "variant"}, {ask.breaks, "break"}, {ask.indels, "indel"}, {ask.map, "map"},
                                                                 {ask.dedupOut, "duplicate"}, {ask.links, "link"}, {ask.join, "join"}};
        for (const auto &r : reports)       // the lap carries the name of the first report that was asked for
            if (r.first) { laps.lap((std::string(r.second) + " report: kmermatcher, rescorediagonal").c_str()); break; }
        if (ask.dedup && !ask.dedupOut) { dedupSet(ctx, ps, c, NULL); laps.lap("duplicate reads out of the set"); }      // before any reduction
    }
    if (ask.dedupOut) dedupTable(ctx, c, ps, *ask.dedupOut, laps);
    if (ask.damageOut) damageTable(ctx, c, ps, ask.ends, *ask.damageOut, laps);
    if (ask.depthOut) {
        std::vector<std::vector<uint64_t>> stats(1); std::vector<uint32_t> track;
        if (c.nc) depthSample(ctx, c, ps, ask.edge, ask.depthGap, stats[0], ask.trackOut ? &track : NULL);
        depthFiles(c, stats, *ask.depthOut, ask.trackOut, track);
        laps.lap("depth report: depth, table");
    }
    if (ask.variants) variantReport(ctx, c, ps, *ask.variants, laps);
    if (ask.breaks) breakReport(ctx, c, ps, *ask.breaks, laps);
    if (ask.map) mapReport(ctx, c, ask.mapReads, ps, *ask.map, laps);
    if (ask.indels) indelReport(ctx, c, ps, *ask.indels, laps);
    if (ask.links) linkReport(ctx, c, ps, *ask.links, laps);
    if (ask.join) joinReport(ctx, c, ps, *ask.join, laps);
    freePileSet(ps);
}
int contigDamage(Args &a) {
    return contigReport(a, "contig_damage", false, "Usage: carpedeam contig_damage <i:contigs DB|fast(a|q)[.gz]> <i:reads DB|fast(a|q)[.gz]> <o:tsvFile> [--damage-ends 16] [--min-seq-id 0.9] [-k 20]", DAMAGE_FLAGS,
                        [&](PileAsk &ask) { ask.ends = damageEnds(a, "contig_damage"); ask.dedup = dedupFlag(a, "contig_damage", false); ask.damageOut = &a.pos[2]; });
}
// N read sets, each freed before the next is loaded: a column group per set in one table
int contigDepth(Args &a) {
    return contigCommand(a, "contig_depth", a.pos.size() >= 3, "Usage: carpedeam contig_depth <i:contigs DB|fast(a|q)[.gz]> <i:reads DB|fast(a|q)[.gz]> [<i:reads> ...] <o:tsvFile> [--depth-edge 0] [--min-seq-id 0.9] [-k 20] [--depth-track <bedGraph>] [--gapped 0] [--gap-band 8] [--gap-min-columns 32]",
                         DEPTH_FLAGS, [&](PileAsk &ask) {
        ask.edge = depthEdge(a, "contig_depth");
        ask.depthGap = gapOpts(a, "contig_depth", TABLE_GAPPED);
        ask.dedup = dedupFlag(a, "contig_depth", ask.depthGap.on);
        ask.depthOut = &a.pos.back(); ask.trackOut = flagPath(a, "--depth-track");
        if (ask.trackOut && a.pos.size() > 3) unsupported("contig_depth: --depth-track with " + std::to_string(a.pos.size() - 2) + " read sets is not supported by the MI355X path (the track is written for one read set)");
    }, [&](cdm_ctx *ctx, const SeqSet *contigs, PileAsk &ask, Laps &laps) {
        laps.lap("contigs read, sequences up");
        const Frame c(ctx, contigs);
        std::vector<std::vector<uint64_t>> stats(a.pos.size() - 2); std::vector<uint32_t> track;
        for (size_t s = 0; contigs && s < stats.size(); s++) {
            SeqSet reads;
            if (!loadSeqSet(ctx, a.pos[1 + s], true, false, reads)) die("contig_depth: " + a.pos[1 + s] + " holds no reads");
            PileSet ps = pileupAlignments(ctx, contigs->db, reads.db, (int) iflag(a, "-k", 20), fflag(a, "--min-seq-id", 0.9f), ask.depthGap.on);
            laps.lap("depth report: reads up, kmermatcher, rescorediagonal");
            if (ask.dedup) dedupSet(ctx, ps, c, NULL);      // per read set: duplicates are copies within one library
            depthSample(ctx, c, ps, ask.edge, ask.depthGap, stats[s], ask.trackOut ? &track : NULL);
            freePileSet(ps); cdm_seqdb_free(reads.db);
            laps.lap("depth report: depth");
        }
        depthFiles(c, stats, *ask.depthOut, ask.trackOut, track);
        laps.lap("depth report: table");
    });
}
int contigVariants(Args &a) {
    VariantOut v;
    return contigReport(a, "contig_variants", true, "Usage: carpedeam contig_variants <i:contigs DB|fast(a|q)[.gz]> <i:reads DB|fast(a|q)[.gz]> <o:tsvFile> [--min-depth 3] [--min-alt-count 2] [--min-alt-percent 20] [--mask-ends 0] "
                        "[--sites <tsvFile>] [--consensus <fastaFile>] [--gapped 0] [--gap-band 8] [--gap-min-columns 32] [--min-seq-id 0.9] [-k 20]", VARIANT_FLAGS, [&](PileAsk &ask) {
        v.opt = variantOpts(a, "contig_variants");
        v.gap = gapOpts(a, "contig_variants", TABLE_GAPPED);
        ask.dedup = dedupFlag(a, "contig_variants", v.gap.on);
        v.summary = &a.pos[2]; v.sites = flagPath(a, "--sites"); v.consensus = flagPath(a, "--consensus");
        ask.variants = &v;
    });
}
int contigBreaks(Args &a) {
    BreakOut o;
    return contigReport(a, "contig_breaks", true, "Usage: carpedeam contig_breaks <i:contigs DB|fast(a|q)[.gz]> <i:reads DB|fast(a|q)[.gz]> <o:tsvFile> [--break-anchor 16] [--break-edge 50] [--min-span 1] [--min-span-percent 0] "
                        "[--split <fastaFile>] [--min-piece 1] [--span-track <bedGraph>] [--gapped 0] [--gap-band 8] [--gap-min-columns 32] [--min-seq-id 0.9] [-k 20]", BREAK_FLAGS, [&](PileAsk &ask) {
        o.opt = breakOpts(a, "contig_breaks");
        o.gap = gapOpts(a, "contig_breaks", TABLE_GAPPED);
        ask.dedup = dedupFlag(a, "contig_breaks", o.gap.on);
        o.minPiece = rangedFlag(a, "contig_breaks", "--min-piece", 1, 1, 1048576, "a piece that is written has 1 to 1048576 letters at the least");
        o.summary = &a.pos[2]; o.split = flagPath(a, "--split"); o.track = flagPath(a, "--span-track");
        ask.breaks = &o;
    });
}
int contigMap(Args &a) {
    MapOut o;
    return contigReport(a, "contig_map", true, "Usage: carpedeam contig_map <i:contigs DB|fast(a|q)[.gz]> <i:reads DB|fast(a|q)[.gz]> <o:samFile> [--read-group <id>] [--primary-only 0] [--gapped 0] [--gap-band 8] [--gap-min-columns 32] [--min-seq-id 0.9] [-k 20] [--threads N]",
                        MAP_FLAGS, [&](PileAsk &ask) {
        o.primaryOnly = rangedFlag(a, "contig_map", "--primary-only", 0, 0, 1, "0 writes every line, 1 leaves the secondary lines out") != 0;
        o.readGroup = flagPath(a, "--read-group");
        if (o.readGroup && (o.readGroup->empty() || o.readGroup->find('\t') != std::string::npos))
            unsupported("contig_map: --read-group \"" + *o.readGroup + "\" is not supported by the MI355X path (a read group's ID is at least one character and holds no tab)");
        o.gap = gapOpts(a, "contig_map", "0 writes the ungapped overlaps alone, 1 adds the reads rescued across insertions and deletions");
        ask.dedup = dedupFlag(a, "contig_map", o.gap.on);
        o.sam = &a.pos[2];
        ask.map = &o;
    });
}
int contigDedup(Args &a) {
    return contigReport(a, "contig_dedup", true, "Usage: carpedeam contig_dedup <i:contigs DB|fast(a|q)[.gz]> <i:reads DB|fast(a|q)[.gz]> <o:tsvFile> [--min-seq-id 0.9] [-k 20] [--threads N]. "
                        "The duplicate reads it counts are the ones that --dedup 1 leaves out of contig_damage, contig_depth, contig_variants, contig_breaks and contig_map.", DEDUP_FLAGS,
                        [&](PileAsk &ask) { ask.dedupOut = &a.pos[2]; });
}
int contigLinks(Args &a) {
    LinkOut o;
    return contigReport(a, "contig_links", true, "Usage: carpedeam contig_links <i:contigs DB|fast(a|q)[.gz]> <i:reads DB|fast(a|q)[.gz]> <o:tsvFile> [--link-anchor 16] [--link-overhang 1] [--link-max-ends 16] [--min-link-reads 2] "
                        "[--ends <tsvFile>] [--gfa <gfaFile>] [--dedup 0] [--min-seq-id 0.9] [-k 20] [--threads N]", LINK_FLAGS, [&](PileAsk &ask) {
        o.anchor = rangedFlag(a, "contig_links", "--link-anchor", 16, 1, 1024, "an end record has 1 to 1024 columns on its contig");
        o.overhang = rangedFlag(a, "contig_links", "--link-overhang", 1, 1, 1024, "an end record's read has 1 to 1024 letters beyond the contig's end");
        o.maxEnds = rangedFlag(a, "contig_links", "--link-max-ends", 16, 2, 64, "a read that makes links has 2 to 64 end records at the most");
        o.minReads = rangedFlag(a, "contig_links", "--min-link-reads", 2, 1, 1000000, "a link that is written has 1 to 1000000 reads at the least");
        ask.dedup = dedupFlag(a, "contig_links", false);
        o.table = &a.pos[2]; o.ends = flagPath(a, "--ends"); o.gfa = flagPath(a, "--gfa");
        ask.links = &o;
    });
}
int contigJoin(Args &a) {
    JoinOut o;
    return contigReport(a, "contig_join", true, "Usage: carpedeam contig_join <i:contigs DB|fast(a|q)[.gz]> <i:reads DB|fast(a|q)[.gz]> <o:tsvFile> [--joined <fastaFile>] [--paths <tsvFile>] [--join-overlap-percent 90] "
                        "[--link-anchor 16] [--link-overhang 1] [--link-max-ends 16] [--min-link-reads 2] [--dedup 0] [--min-seq-id 0.9] [-k 20] [--threads N]", JOIN_FLAGS, [&](PileAsk &ask) {
        o.overlapPercent = rangedFlag(a, "contig_join", "--join-overlap-percent", 90, 0, 100, "a percentage of the overlap's columns is 0 to 100");
        o.anchor = rangedFlag(a, "contig_join", "--link-anchor", 16, 1, 1024, "an end record has 1 to 1024 columns on its contig");
        o.overhang = rangedFlag(a, "contig_join", "--link-overhang", 1, 1, 1024, "an end record's read has 1 to 1024 letters beyond the contig's end");
        o.maxEnds = rangedFlag(a, "contig_join", "--link-max-ends", 16, 2, 64, "a read that makes links has 2 to 64 end records at the most");
        o.minLinkReads = rangedFlag(a, "contig_join", "--min-link-reads", 2, 1, 1000000, "a link that is written has 1 to 1000000 reads at the least");
        ask.dedup = dedupFlag(a, "contig_join", false);
        o.table = &a.pos[2]; o.joined = flagPath(a, "--joined"); o.paths = flagPath(a, "--paths");
        ask.join = &o;
    });
}
int contigIndels(Args &a) {
    IndelOut o;
    return contigReport(a, "contig_indels", true, "Usage: carpedeam contig_indels <i:contigs DB|fast(a|q)[.gz]> <i:reads DB|fast(a|q)[.gz]> <o:tsvFile> [--min-depth 3] [--min-indel-count 2] [--min-indel-percent 20] "
                        "[--gap-band 8] [--gap-min-columns 32] [--sites <tsvFile>] [--consensus <fastaFile>] [--min-seq-id 0.9] [-k 20] [--threads N]", INDEL_FLAGS, [&](PileAsk &ask) {
        o.minDepth = rangedFlag(a, "contig_indels", "--min-depth", 3, 1, 1000000, "a called place is crossed by 1 to 1000000 reads");
        o.minCount = rangedFlag(a, "contig_indels", "--min-indel-count", 2, 1, 1000000, "a supported insertion or deletion has 1 to 1000000 reads");
        o.minPercent = rangedFlag(a, "contig_indels", "--min-indel-percent", 20, 0, 100, "a percentage of the crossing reads is 0 to 100");
        o.gap = gapOpts(a, "contig_indels", NULL);
        o.summary = &a.pos[2]; o.sites = flagPath(a, "--sites"); o.consensus = flagPath(a, "--consensus");
        ask.indels = &o;
    });
}
