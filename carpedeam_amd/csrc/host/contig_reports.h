// host/contig_reports.cpp: the nine contig_* commands, and what ancient_assemble_fused (host/main.cpp) needs to write the same reports
// for its final contigs - the sequence loader, the option parsers under its own module name, PileAsk and pileReports.
#pragma once
#include "cli.h"

int contigDamage(Args &a);
int contigDepth(Args &a);
int contigVariants(Args &a);
int contigBreaks(Args &a);
int contigMap(Args &a);
int contigIndels(Args &a);
int contigDedup(Args &a);
int contigLinks(Args &a);
int contigJoin(Args &a);

// a set of sequences on the device with the names and keys its report lines carry
struct SeqSet { cdm_seqdb *db = NULL; std::vector<std::string> names; std::vector<uint32_t> keys; };
// path: a sequence DB (names from its header DB where it has one) or FASTA/FASTQ[.gz] (shuffle: createdb's order, as the loop lays its
// reads out).  false: the input holds no sequence.
bool loadSeqSet(cdm_ctx *ctx, const std::string &path, bool shuffle, bool wantNames, SeqSet &in);

// --gapped 0|1 with --gap-band and --gap-min-columns: the reads rescued across insertions and deletions (cdm_pileup_gapped) beside
// the ungapped overlaps; on: the rescued reads count as well (the alignment set keeps its hits)
struct GapOpts { bool on = false; long band = 8, minColumns = 32; float minSeqId = 0.9f; };
long damageEnds(Args &a, const char *module);
long depthEdge(Args &a, const char *module);
struct VariantOpts { long maskEnds, minDepth, minAltCount, minAltPercent; };
VariantOpts variantOpts(Args &a, const char *module);
struct BreakOpts { long anchor, edge, minSpan, minSpanPercent; };
BreakOpts breakOpts(Args &a, const char *module);
// what a variant and a break report write: the summary always, the other two files when named
struct VariantOut { VariantOpts opt; const std::string *summary, *sites, *consensus; GapOpts gap; };
struct BreakOut { BreakOpts opt; long minPiece; const std::string *summary, *split, *track; GapOpts gap; };
struct MapOut;
struct IndelOut;
struct LinkOut;
struct JoinOut;
// What a pileReports call is asked for (NULL: not asked for): the damage table with its ends, the depth table with its edge and
// track, the variant, the break and the indel reports, the map report with the read set whose names and letters its lines carry, the
// duplicate table, the link report, the join report.  dedup: the duplicate reads (cdm_alns_dedup over the contigs) leave the set before any reduction sees it.
struct PileAsk {
    bool dedup = false; const std::string *dedupOut = NULL;
    const std::string *damageOut = NULL; long ends = 0;
    const std::string *depthOut = NULL; long edge = 0; const std::string *trackOut = NULL; GapOpts depthGap;
    const VariantOut *variants = NULL; const BreakOut *breaks = NULL;
    const MapOut *map = NULL; const SeqSet *mapReads = NULL;
    const IndelOut *indels = NULL;
    const LinkOut *links = NULL;
    const JoinOut *join = NULL;
};
// The reports of one read set against one set of contigs: kmermatcher and rescorediagonal once, then each reduction that was asked
// for on the same alignment set.  contigs == NULL: the header lines alone.  Neither DB is freed here.
void pileReports(cdm_ctx *ctx, const SeqSet *contigs, cdm_seqdb *reads, int kmerSize, float minSeqId, const PileAsk &ask, Laps &laps);
