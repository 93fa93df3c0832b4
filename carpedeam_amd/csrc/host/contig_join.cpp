// The host rules of `carpedeam contig_join` (contig_join.h holds them in words): decisions, paths and the three files.
#include <algorithm>

#include "contig_join.h"

std::string joinRevComp(const char *s, size_t n) {
    static const char FROM[] = "ATCGRYKMBVDHatcgrykmbvdh", TO[] = "TAGCYRMKVBHDtagcyrmkvbhd";
    unsigned char map[256];
    for (int i = 0; i < 256; i++) map[i] = (unsigned char) i;
    for (size_t i = 0; FROM[i]; i++) map[(unsigned char) FROM[i]] = (unsigned char) TO[i];
    std::string out(n, '\0');
    for (size_t i = 0; i < n; i++) out[i] = (char) map[(unsigned char) s[n - 1 - i]];
    return out;
}

namespace {
// a contig end: contig << 1 | (1 for the right end)
uint64_t endA(const cdm_link &k) { return (uint64_t) k.a << 1 | (k.info & 1u ? 0u : 1u); }
uint64_t endB(const cdm_link &k) { return (uint64_t) k.b << 1 | (k.info & 2u ? 1u : 0u); }
uint64_t overlapOf(const cdm_link &k) { return k.gap_mode < 0 ? (uint64_t) -(int64_t) k.gap_mode : 0u; }

// the undecided link at every contig end (-1: none)
struct Ends {
    std::vector<int64_t> at;
    Ends(const cdm_link *links, uint64_t n, size_t nc, const std::vector<char> &dec) : at(2 * nc, -1) {
        for (uint64_t i = 0; i < n; i++) if (!dec[i]) { at[endA(links[i])] = (int64_t) i; at[endB(links[i])] = (int64_t) i; }
    }
    void drop(const cdm_link &k) { at[endA(k)] = -1; at[endB(k)] = -1; }        // (an end has one undecided link at the most: the others are A)
    int64_t left(uint64_t c) const { return at[c << 1]; }
    int64_t right(uint64_t c) const { return at[c << 1 | 1u]; }
};
// From contig c in orientation o through its leaving end: false at a free end; otherwise the link, the next contig and its orientation,
// and whether the link is walked in its canonical direction.
bool step(const cdm_link *links, const Ends &e, uint32_t c, char o, int64_t &link, uint32_t &next, char &no, bool &canonical) {
    const uint64_t end = (uint64_t) c << 1 | (o == '+' ? 1u : 0u);
    link = e.at[end];
    if (link < 0) return false;
    const cdm_link &k = links[link];
    canonical = endA(k) == end;
    if (canonical) { next = k.b; no = k.info & 2u ? '-' : '+'; }
    else { next = k.a; no = k.info & 1u ? '+' : '-'; }       // (b, flip oB) -> (a, flip oA)
    return true;
}
void putNum(std::string &to, long long v) { to.push_back('\t'); to += std::to_string(v); }
}  // namespace

void joinFirst(const cdm_link *links, uint64_t nLinks, const std::vector<uint32_t> &lens, long minLinkReads, JoinPlan &p) {
    p = JoinPlan();
    p.dec.assign(nLinks, 0); p.linkPath.assign(nLinks, -1);
    std::vector<uint32_t> touched(2 * lens.size(), 0);
    for (uint64_t i = 0; i < nLinks; i++) { touched[endA(links[i])]++; touched[endB(links[i])]++; }
    for (uint64_t i = 0; i < nLinks; i++) {
        const cdm_link &k = links[i];
        if (touched[endA(k)] > 1 || touched[endB(k)] > 1) p.dec[i] = 'A';
        else if ((long) k.mode_reads < minLinkReads) p.dec[i] = 'W';
        else if (overlapOf(k) > std::min(lens[k.a], lens[k.b])) p.dec[i] = 'C';
        else { cdm_junction j; j.a = k.a; j.b = k.b; j.info = k.info; j.gap = k.gap_mode; p.juncs.push_back(j); p.at.push_back(i); }
    }
}

void joinDecide(const cdm_link *links, uint64_t nLinks, const std::vector<uint32_t> &lens, const cdm_junction_res *res, const uint8_t *letters, long overlapPercent, JoinPlan &p) {
    const size_t nc = lens.size();
    std::vector<std::string> fill(nLinks);
    for (size_t j = 0; j < p.at.size(); j++) {
        const uint64_t i = p.at[j];
        if (links[i].gap_mode < 0 && (uint64_t) res[j].matches * 100u < (uint64_t) overlapPercent * res[j].columns) p.dec[i] = 'X';
        if (res[j].fill_len) fill[i].assign((const char *) letters + res[j].fill_off, res[j].fill_len);
    }
    Ends e(links, nLinks, nc, p.dec);
    for (uint64_t c = 0; c < nc; c++) {         // S
        const int64_t l = e.left(c), r = e.right(c);
        if (l < 0 || r < 0 || overlapOf(links[l]) + overlapOf(links[r]) <= lens[c]) continue;
        const int64_t lo = std::min(l, r), hi = std::max(l, r);
        const int64_t goes = links[lo].reads < links[hi].reads ? lo : hi;
        p.dec[goes] = 'S'; e.drop(links[goes]);
    }
    std::vector<char> seen(nc, 0);
    for (uint32_t c = 0; c < nc; c++) {         // O
        if (seen[c]) continue;
        std::vector<uint32_t> members(1, c);
        uint32_t cur = c, next; char o = '+', no; int64_t link; bool canonical;
        while (step(links, e, cur, o, link, next, no, canonical)) {
            cur = next; o = no;
            if (cur == c) { const int64_t opened = e.left(c); p.dec[opened] = 'O'; e.drop(links[opened]); break; }
            if (seen[cur]) break;       // an open path that an earlier walk went along already: no circle
            members.push_back(cur);
        }
        for (uint32_t m : members) seen[m] = 1;     // (circle or not: no contig is walked from twice, the loop is linear in the links)
    }
    std::vector<char> done(nc, 0);
    for (uint32_t c = 0; c < nc; c++) {         // the paths: an end contig starts unless the other end of its path has the smaller index
        if (done[c] || (e.left(c) < 0) == (e.right(c) < 0)) continue;
        std::vector<JoinMember> path;
        std::vector<int64_t> used;
        uint32_t cur = c, next; char o = e.right(c) >= 0 ? '+' : '-', no; int64_t link; bool canonical;
        path.push_back(JoinMember{c, o, 0u, std::string()});
        while (step(links, e, cur, o, link, next, no, canonical)) {
            cur = next; o = no;
            used.push_back(link);
            path.push_back(JoinMember{cur, o, (uint32_t) overlapOf(links[link]), canonical ? fill[link] : joinRevComp(fill[link].data(), fill[link].size())});
        }
        if (cur < c) continue;
        for (const JoinMember &m : path) done[m.contig] = 1;
        for (int64_t i : used) p.linkPath[i] = (int64_t) p.paths.size();
        p.paths.push_back(path);
    }
    for (char &d : p.dec) if (!d) d = 'J';
}

std::string joinPathName(const JoinContigs &c, const std::vector<JoinMember> &path) { return (*c.names)[path[0].contig] + "_join" + std::to_string(path.size()); }

std::string joinTable(const JoinContigs &c, const cdm_link *links, uint64_t nLinks, const cdm_junction_res *res, const JoinPlan &p) {
    std::string text;
    std::vector<int64_t> junctionOf(nLinks, -1);
    for (size_t j = 0; j < p.at.size(); j++) junctionOf[p.at[j]] = (int64_t) j;
    for (uint64_t i = 0; i < nLinks; i++) {
        const cdm_link &k = links[i];
        text += (*c.names)[k.a]; text.push_back('\t'); text.push_back(k.info & 1u ? '-' : '+'); text.push_back('\t');
        text += (*c.names)[k.b]; text.push_back('\t'); text.push_back(k.info & 2u ? '-' : '+');
        putNum(text, k.reads); putNum(text, k.gap_mode); putNum(text, k.mode_reads);
        const cdm_junction_res *r = junctionOf[i] >= 0 ? &res[junctionOf[i]] : NULL;
        putNum(text, r ? r->columns : 0); putNum(text, r ? r->matches : 0); putNum(text, r ? r->fill_min : 0); putNum(text, r ? r->fill_n : 0);
        text.push_back('\t'); text.push_back(p.dec[i]); text.push_back('\t');
        text += p.dec[i] == 'J' ? joinPathName(c, p.paths[p.linkPath[i]]) : std::string("-");
        text.push_back('\n');
    }
    return text;
}

std::string joinFasta(const JoinContigs &c, const JoinPlan &p) {
    const size_t nc = c.lens->size();
    std::vector<int64_t> startOf(nc, -1); std::vector<char> inside(nc, 0);
    for (size_t k = 0; k < p.paths.size(); k++) { startOf[p.paths[k][0].contig] = (int64_t) k; for (const JoinMember &m : p.paths[k]) inside[m.contig] = 1; }
    std::string fasta;
    for (size_t i = 0; i < nc; i++) {
        if (startOf[i] < 0 && inside[i]) continue;
        fasta.push_back('>');
        if (startOf[i] < 0) { fasta += (*c.names)[i]; fasta.push_back('\n'); fasta.append(*c.letters, (*c.at)[i], (*c.lens)[i]); fasta.push_back('\n'); continue; }
        const std::vector<JoinMember> &path = p.paths[startOf[i]];
        fasta += joinPathName(c, path); fasta.push_back('\n');
        for (const JoinMember &m : path) {
            const char *s = c.letters->data() + (*c.at)[m.contig]; const size_t n = (*c.lens)[m.contig];
            fasta += m.fill;
            if (m.o == '+') fasta.append(s + m.trim, n - m.trim); else fasta.append(joinRevComp(s, n), m.trim, std::string::npos);
        }
        fasta.push_back('\n');
    }
    return fasta;
}

std::string joinPaths(const JoinContigs &c, const JoinPlan &p) {
    std::string text;
    for (const std::vector<JoinMember> &path : p.paths) {
        const std::string name = joinPathName(c, path);
        uint64_t at = 0;
        for (size_t n = 0; n < path.size(); n++) {
            const JoinMember &m = path[n];
            at += m.fill.size();
            text += name; putNum(text, (long long) n + 1); text.push_back('\t'); text += (*c.names)[m.contig]; text.push_back('\t'); text.push_back(m.o);
            putNum(text, (long long) at + 1); putNum(text, (*c.lens)[m.contig]); putNum(text, m.trim); putNum(text, (long long) m.fill.size());
            text.push_back('\n');
            at += (*c.lens)[m.contig] - m.trim;
        }
    }
    return text;
}
