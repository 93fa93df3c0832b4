// Driver of tests/test_join_host.py over host/contig_join.cpp: reads a case from a text file, runs joinFirst, takes the junction results
// the test supplies per link, runs joinDecide and prints the decisions, junctions, paths and the three files.
//   <overlap percent> <min link reads>
//   <contigs>            then per contig:  <name> <letters>
//   <links>              then per link:    a b info reads forward mode_reads gap_mode gap_min gap_max gap_sum
//   <results>            then per result:  link columns matches voters flags fill_len fill_min fill_n fill|-
#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>

#include "../../carpedeam_amd/csrc/host/contig_join.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: join_driver <case file>\n"); return 2; }
    std::ifstream in(argv[1]);
    long percent, minReads; size_t nc, nl, nr;
    in >> percent >> minReads >> nc;
    std::vector<std::string> names(nc); std::vector<uint64_t> at(nc + 1, 0); std::vector<uint32_t> lens(nc); std::string letters;
    for (size_t i = 0; i < nc; i++) { std::string s; in >> names[i] >> s; lens[i] = (uint32_t) s.size(); at[i] = letters.size(); letters += s; letters.push_back('\n'); }
    at[nc] = letters.size();
    in >> nl;
    std::vector<cdm_link> links(nl);
    for (cdm_link &k : links) { long long sum; in >> k.a >> k.b >> k.info >> k.reads >> k.forward >> k.mode_reads >> k.gap_mode >> k.gap_min >> k.gap_max >> sum; k.gap_sum = sum; k.reserved = 0; }
    in >> nr;
    std::map<uint64_t, std::pair<cdm_junction_res, std::string>> given;
    for (size_t i = 0; i < nr; i++) {
        uint64_t link; cdm_junction_res r; std::string f;
        in >> link >> r.columns >> r.matches >> r.voters >> r.flags >> r.fill_len >> r.fill_min >> r.fill_n >> f;
        r.reserved = 0; r.fill_off = 0;
        given[link] = std::make_pair(r, f == "-" ? std::string() : f);
    }
    if (!in) { fprintf(stderr, "join_driver: the case file does not parse\n"); return 2; }
    JoinPlan p;
    joinFirst(links.data(), nl, lens, minReads, p);
    std::vector<cdm_junction_res> res; std::string pool;
    for (uint64_t i : p.at) {
        if (!given.count(i)) { fprintf(stderr, "join_driver: no result for the junction of link %llu\n", (unsigned long long) i); return 3; }
        cdm_junction_res r = given[i].first;
        r.fill_off = pool.size(); pool += given[i].second;
        res.push_back(r);
    }
    for (const cdm_junction &j : p.juncs) printf("junc %u %u %u %d\n", j.a, j.b, j.info, j.gap);
    joinDecide(links.data(), nl, lens, res.data(), (const uint8_t *) pool.data(), percent, p);
    printf("dec %s\n", std::string(p.dec.begin(), p.dec.end()).c_str());
    for (size_t k = 0; k < p.paths.size(); k++)
        for (const JoinMember &m : p.paths[k]) printf("path %zu %u %c %u %s\n", k, m.contig, m.o, m.trim, m.fill.empty() ? "-" : m.fill.c_str());
    const JoinContigs c = {&names, &letters, &at, &lens};
    std::cout << "==joins\n" << joinTable(c, links.data(), nl, res.data(), p) << "==joined\n" << joinFasta(c, p) << "==paths\n" << joinPaths(c, p) << "==end\n";
    return 0;
}
