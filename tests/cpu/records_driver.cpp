// Driver of tests/test_records_host.py: the record codecs of the host binary (carpedeam_amd/csrc/host/records.cpp) on DB files, without a
// device.  CSR arrays travel as raw files: <x>.off = uint64[n + 1], <x>.rec = cdm_hit[] / cdm_aln[] (numpy.fromfile).
//   records_driver THREADS parse-pref   seqDB prefDB out                  -> out.off out.rec
//   records_driver THREADS parse-aln    seqDB alnDB out                   -> out.off out.rec
//   records_driver THREADS format-pref  seqDB in outDB dbtype             in.off in.rec -> outDB
//   records_driver THREADS format-resc  seqDB prefDB in outDB dbtype      (formatRescoredPrefDb)
//   records_driver THREADS format-aln   seqDB prefDB|- in dbResidues outDB [parsed]   -> outDB, parsed.rec = the asParsed array
//   records_driver THREADS hits-side-w  seqDB DB in dbtype                the side-car of DB, as kmermatcher writes it beside the text
//   records_driver THREADS hits-side-r  seqDB DB out                      -> out.off out.rec, prints the dbtype; status 3: refused
//   records_driver THREADS alns-side-w  seqDB DB in                       (in.rec = an asParsed array)
//   records_driver THREADS alns-side-r  seqDB DB out
//   records_driver THREADS decimals     file                              one text per line -> "%a consumed" per line (parseDecimal)
#include <cstdio>
#include <fstream>
#include <omp.h>
#include "../../carpedeam_amd/csrc/host/records.h"
#include "../../carpedeam_amd/csrc/host/cli.h"

template <typename T> static void readRaw(const std::string &path, HVec<T> &v) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) die("can not read " + path);
    v.resize((size_t) f.tellg() / sizeof(T));
    f.seekg(0); f.read((char *) v.data(), (std::streamsize) (v.size() * sizeof(T)));
}
template <typename T> static void writeRaw(const std::string &path, const T *p, size_t n) {
    std::ofstream f(path, std::ios::binary);
    f.write((const char *) p, (std::streamsize) (n * sizeof(T)));
    if (!f) die("can not write " + path);
}
template <typename Rec> static void dump(const std::string &out, const HVec<uint64_t> &off, const HVec<Rec> &rec) { writeRaw(out + ".off", off.data(), off.size()); writeRaw(out + ".rec", rec.data(), rec.size()); }
static void load(MmDb &db, const std::string &path) { std::string err; if (!db.load(path, &err)) die(err); }
static void writeDb(const std::string &path, int dbtype, const std::vector<OutChunk> &chunks) { std::string err; if (!mmdbWriteChunks(path, dbtype, chunks, &err, true)) die(err); }

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    omp_set_dynamic(0); omp_set_num_threads(atoi(argv[1]));
    const std::string cmd = argv[2];
    std::vector<std::string> a(argv + 3, argv + argc);
    if (cmd == "decimals") {
        std::ifstream f(a[0]); std::string line;
        while (std::getline(f, line)) { const char *d = line.c_str(); const double v = parseDecimal(d); printf("%a %d\n", v, (int) (d - line.c_str())); }
        return 0;
    }
    MmDb seq; load(seq, a[0]);
    HVec<uint64_t> off; HVec<cdm_hit> hits; HVec<cdm_aln> alns; std::vector<OutChunk> chunks;
    if (cmd == "parse-pref" || cmd == "parse-aln") {
        MmDb res; load(res, a[1]);
        if (cmd == "parse-pref") { parsePrefDb(res, seq, off, hits); dump(a[2], off, hits); }
        else { parseAlnDb(res, seq, off, alns); dump(a[2], off, alns); }
    } else if (cmd == "format-pref") {
        readRaw(a[1] + ".off", off); readRaw(a[1] + ".rec", hits);
        formatPrefDb(seq, off.data(), hits.data(), chunks); writeDb(a[2], atoi(a[3].c_str()), chunks);
    } else if (cmd == "format-resc") {
        MmDb pref; load(pref, a[1]);
        readRaw(a[2] + ".off", off); readRaw(a[2] + ".rec", hits);
        formatRescoredPrefDb(seq, pref, off.data(), hits.data(), chunks); writeDb(a[3], atoi(a[4].c_str()), chunks);
    } else if (cmd == "format-aln") {
        MmDb pref; if (a[1] != "-") load(pref, a[1]);
        readRaw(a[2] + ".off", off); readRaw(a[2] + ".rec", alns);
        HVec<cdm_aln> parsed(a.size() > 5 ? alns.size() : 0);
        formatAlnDb(seq, a[1] != "-" ? &pref : NULL, off.data(), alns.data(), strtoull(a[3].c_str(), NULL, 10), chunks, a.size() > 5 ? parsed.data() : NULL);
        writeDb(a[4], 5, chunks);
        if (a.size() > 5) writeRaw(a[5] + ".rec", parsed.data(), parsed.size());
    } else if (cmd == "hits-side-w" || cmd == "alns-side-w") {
        readRaw(a[2] + ".off", off);
        SideThread side; const int dbtype = a.size() > 3 ? atoi(a[3].c_str()) : 0;
        if (cmd == "hits-side-w") { readRaw(a[2] + ".rec", hits); side.begin(a[1], [&](SideHeader *h) { return writeHitsSide(a[1], seq, off.data(), hits.data(), dbtype, h); }); }
        else { readRaw(a[2] + ".rec", alns); side.begin(a[1], [&](SideHeader *h) { return writeAlnsSide(a[1], seq, off.data(), alns.data(), h); }); }
        side.commit();
    } else if (cmd == "hits-side-r") {
        int dbtype = 0;
        if (!readHitsSide(a[1], seq, off, hits, &dbtype)) return 3;
        dump(a[2], off, hits); printf("%d\n", dbtype);
    } else if (cmd == "alns-side-r") {
        if (!readAlnsSide(a[1], seq, off, alns)) return 3;
        dump(a[2], off, alns);
    } else return 2;
    return 0;
}
