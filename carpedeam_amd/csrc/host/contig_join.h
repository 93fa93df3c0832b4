// host/contig_join.cpp: what `carpedeam contig_join` decides and writes once the device has spoken - links (cdm_pileup_links), contig
// lengths and junction results (cdm_pileup_junctions) become decisions, paths and the three files.  No device call, no file access: the
// unit is tested on the CPU (tests/cpu/join_driver.cpp).
//
// Every returned link gets exactly one decision; the steps run in this order and nothing cascades (a refused link still makes its ends
// ambiguous).  A link touches A's right end when oA is +, its left end when -; B's left end when oB is +, its right end when -.
//   A  ambiguous   another returned link touches one of its two ends
//   W  weak        mode_reads < minLinkReads: the bridging reads do not agree on one gap
//   C  contained   -gap_mode > min(lenA, lenB)
//      the links that are left are the JUNCTIONS of the device call, with gap = gap_mode
//   X  the letters disagree   gap_mode < 0 and matches x 100 < overlapPercent x columns
//   S  short       contigs in file order: where a contig's two remaining links have overlaps that together exceed its length, the link with
//                  fewer reads goes, among equals the later in the table
//   O  circle      each end has at most one link now; where the links close a circle the walk starts at its contig with the smallest
//                  file index, +, and leaves through its right end: the link at that contig's left end is opened
//   J  joined      everything left
// Of a path's two end contigs the one with the smaller file index starts, + when the path leaves through its right end, - otherwise.  A
// link walked against its canonical direction is (b, flip oB) -> (a, flip oA): the same overlap, the reverse complement of its fill.
// The joined letters are the oriented first contig, then per junction the fill and the oriented next contig without its first k letters
// (the overlap is taken from the contig in front).  Contig bytes are the input's own; joinRevComp is on bytes.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "carpedeam_hip.h"

// reverse complement on bytes, case kept: A<->T, C<->G, the IUPAC pairs R<->Y, K<->M, B<->V, D<->H; S W N and every other byte unchanged
std::string joinRevComp(const char *s, size_t n);

struct JoinMember { uint32_t contig; char o; uint32_t trim; std::string fill; };      // trim: letters dropped at its front; fill: voted letters in front of it
struct JoinPlan {
    std::vector<char> dec;                          // per link: A W C X S O J (0 while undecided)
    std::vector<cdm_junction> juncs;                // joinFirst: the junctions, ascending as the links are
    std::vector<uint64_t> at;                       // the link of every junction
    std::vector<std::vector<JoinMember>> paths;     // joinDecide: ordered by the start contig's file index
    std::vector<int64_t> linkPath;                  // per link: the path of a J link, -1 otherwise
};
// steps A, W, C and the junctions
void joinFirst(const cdm_link *links, uint64_t nLinks, const std::vector<uint32_t> &lens, long minLinkReads, JoinPlan &p);
// steps X, S, O, J and the paths; res (one per junction) and letters are cdm_pileup_junctions'
void joinDecide(const cdm_link *links, uint64_t nLinks, const std::vector<uint32_t> &lens, const cdm_junction_res *res, const uint8_t *letters, long overlapPercent, JoinPlan &p);

// The contigs as the writers take them: names, and the bytes of contig i at letters[at[i] .. at[i] + lens[i])
struct JoinContigs { const std::vector<std::string> *names; const std::string *letters; const std::vector<uint64_t> *at; const std::vector<uint32_t> *lens; };
std::string joinPathName(const JoinContigs &c, const std::vector<JoinMember> &path);       // <start contig's name>_join<number of contigs>
// joins.tsv: nameA oA nameB oB reads gap_mode mode_reads columns matches fill_min fill_n decision joined_name, one line per link
std::string joinTable(const JoinContigs &c, const cdm_link *links, uint64_t nLinks, const cdm_junction_res *res, const JoinPlan &p);
// --joined: every contig outside a path as it is, every path as one record, by the file index of the (start) contig; a record is two lines
std::string joinFasta(const JoinContigs &c, const JoinPlan &p);
// --paths: joined_name ordinal name o start length trim fill per member; ordinal and start are 1-based, length is the contig's own
std::string joinPaths(const JoinContigs &c, const JoinPlan &p);
