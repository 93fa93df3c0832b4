// The modules that live in units of their own, as host/main.cpp calls them: 0, or a status with *err set (77: a mode that is not implemented)
#pragma once
#include <climits>
#include <string>
#include <vector>

// host/ingest.cpp
int createdbModule(const std::vector<std::string> &files, const std::string &outPath, bool shuffle, int dbType, std::string *err);
int convert2fastaModule(const std::string &dbPath, const std::string &outPath, std::string *err);
int createhdbModule(const std::string &seqPath, const std::string &cyclePath, const std::string &outPath, std::string *err);
// host/cluster.cpp: the host-side modules of linclust's tail and the workflow scripts' file modules
int clustModule(const std::string &seqPath, const std::string &alnPath, const std::string &outPath, int mode, std::string *err);
int createsubdbModule(const std::string &orderArg, const std::string &inPath, const std::string &outPath, int subDbMode, std::string *err);
int filterdbModule(const std::string &inPath, const std::string &outPath, const std::string &filterFile, std::string *err);
int mergeclustersModule(const std::string &seqPath, const std::string &outPath, const std::vector<std::string> &steps, std::string *err);
int result2repseqModule(const std::string &seqPath, const std::string &cluPath, const std::string &outPath, std::string *err);
int rmdbModule(const std::string &db);
int mvdbModule(const std::string &src, const std::string &dst, std::string *err);
// host/align.cpp: linclust's gapped alignment step on the assembled contigs
struct AlignParams {
    float covThr = 0.f, seqIdThr = 0.f; double evalThr = 0.001; int covMode = 0, seqIdMode = 0, alnLenThr = 0; bool wrapped = false, includeIdentity = false;
    int gapOpen = 5, gapExtend = 2, zdrop = 40; unsigned maxAccept = INT_MAX, maxReject = INT_MAX; size_t maxSeqLen = 65535;
};
int alignModule(const std::string &qPath, const std::string &tPath, const std::string &prefPath, const std::string &outPath, const AlignParams &P, std::string *err);
