// Insertion and deletion sites of the read pile-up (cdm_pileup_indels; not a module of the reference): the gapped records of
// cdm_pileup_gapped reduced as the ungapped ones are reduced elsewhere (include/carpedeam_hip.h).  What it shares with the other
// reductions over the read pile-up is in pileup.h.  Per batch of listed queries:
//   cross     signed marks in len + 1 cells per query (+1 at qs + 1 and -1 at qe + 1 of a counted ungapped record, a wave per work
//             item; +1 at pos + 1 and -1 at pos + span of a gapped record, a thread per record), every query's cells sum to zero, ONE
//             prefix sum over the batch's cells: cross[b] = the exclusive prefix at cell b + 1, as depth[p] in pileup_depth.hip
//   events    a thread per gapped record walks its few operations twice: a count pass, an exclusive scan, an emit pass that writes
//             key = query << 31 | p << 7 | (kind - 1) << 6 | g with the event's index as payload; record index and read offset of an
//             event stay in side arrays.  One stable radix sort over the key bits in use
//   alleles   head flags where the key steps, a scan, the first event of every allele; places the same way over the alleles with the
//             key without g.  A thread per place looks at its alleles (at most 62: one per length), picks the best, writes flags and
//             the query's figures and marks the supported; two scans place the site records and their letter slots
//   letters   a wave per supported site: the lanes take the events of an inserted allele, the base counts of its g offsets go to LDS
//             as [62][4], the first g lanes vote
// The records are caller data: indelCheckRecords (pileup.h) refuses, on the host, every record the walks above could follow out of bounds.
#include "pileup.h"
#include "radix.h"

namespace {

constexpr uint64_t ID_CELLS_DEFAULT = 1ull << 28, ID_CELLS_MAX = 1ull << 32;
constexpr int ID_G_BITS = 6, ID_POS_SHIFT = 7, ID_QUERY_SHIFT = 31, ID_STATS = 10;      // (ID_MAX_GAP = 62, pileup.h, fits the 6 bits of the key)

// CDM_INDEL_POSITIONS=<cells> (tests): small inputs in several batches
uint64_t indelPositions() { return envCount("CDM_INDEL_POSITIONS", ID_CELLS_DEFAULT, ID_CELLS_MAX); }
int indelBitsFor(uint64_t n) { int b = 1; while (b < 33 && (1ull << b) < n) b++; return b; }

struct IndelArgs : TiledArgs {      // (items: the ungapped marks; tiles: the track; blocks of DP_NT threads: everything per record, event, allele, place)
    const uint32_t *codes, *nmask;
    const cdm_gap_rec *grec;        // the batch's gapped records [nG]
    const uint32_t *gops;           // the caller's whole operation pool
    uint32_t nG, firstQuery, minDepth, minCount, minPct;
    uint32_t *cells;                // [base[nq]]
    unsigned long long *stats;      // [nq][10]
    uint32_t *track;                // NULL, or [base[nq] - nq]
    uint32_t *evAt;                 // [nG + 1]: events of a record, after the scan its first event
    uint64_t *keys; uint32_t *vals; // [nEv] as emitted
    uint32_t *evRec, *evOff;        // [nEv] record (of the batch) and read offset of an event, by the event's index
    const uint64_t *skeys; const uint32_t *svals;       // sorted
    uint32_t nEv, nAlleles, nPlaces;
    const uint32_t *aStart;         // [nAlleles + 1] first sorted event of an allele
    const uint32_t *pStart;         // [nPlaces + 1] first allele of a place
    cdm_indel_site *pSite; uint32_t *pBest;     // [nPlaces] the place's record, its best allele
    uint32_t *sMark;                // [nPlaces + 1]: 0/1 supported, after the scan the place's site record
    uint64_t *lMark;                // [nPlaces + 1]: letters of the place's record, after the scan its first letter in the batch
    cdm_indel_site *sites; uint32_t *siteAllele; uint8_t *letters;     // [nSites], [nSites], [letters of the batch]
    uint64_t firstLetter;           // letters of the batches in front
};

// marks of the ungapped records: one wave per item (listed query, chunk of its records), lanes take records.  A record with qs == qe
// crosses nothing: its two marks fall on one cell.
__global__ __launch_bounds__(64 * PU_WAVES) void k_indel_marks(IndelArgs a, uint64_t first, uint64_t nThis) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    const ItemRecords it = itemRecords(a, first + local);
    const uint32_t qi = it.qi, q = it.q, qLen = a.meta[q].len;
    uint32_t *cell = a.cells + a.base[qi];
    unsigned int nReads = 0; unsigned long long nCols = 0;
    for (uint64_t r = it.r0 + lane; r < it.r1; r += 64) {
        const AlnRec rec = a.rec[r];
        Oriented o; uint32_t tLen, tw;
        if (!countedRecord(a.meta, a.n, a.skipExt, a.minSeqId, q, qLen, rec, o, tLen, tw)) continue;
        nReads++; nCols += (uint32_t) (o.qe - o.qs) + 1u;
        atomicAdd(&cell[(uint32_t) o.qs + 1u], 1u);                   // (results unused: atomics without return)
        atomicAdd(&cell[(uint32_t) o.qe + 1u], 0xFFFFFFFFu);          // qs <= qe < qLen: at the most the query's closing cell
    }
    addReadsColumns(&a.stats[(uint64_t) qi * ID_STATS], &a.stats[(uint64_t) qi * ID_STATS + 1], nReads, nCols, lane);
}

// gapped records, a thread per record: its two marks, the number of its events, the query's five figures (one atomic of each per wave
// where its lanes share a query - the records are sorted by query)
__global__ __launch_bounds__(DP_NT) void k_indel_count(IndelArgs a, uint64_t first) {
    const int lane = threadIdx.x & 63;
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    const bool live = i < a.nG;
    uint32_t qi = 0, nI = 0, nD = 0, lI = 0, lD = 0;
    if (live) {
        const cdm_gap_rec r = a.grec[i];
        qi = r.query - a.firstQuery;
        uint32_t *cell = a.cells + a.base[qi];
        atomicAdd(&cell[r.pos + 1u], 1u);                   // span >= 1, pos + span <= len: inside the query's cells
        atomicAdd(&cell[r.pos + r.span], 0xFFFFFFFFu);
        for (uint32_t j = 0; j < r.n_ops; j++) {            // (what indelWalk visits, without positions)
            const uint32_t w = a.gops[r.ops + j], g = w >> 2, op = w & 3u;
            if (op == ID_OP_I) { nI++; lI += g; } else if (op != ID_OP_M) { nD++; lD += g; }
        }
        a.evAt[i] = nI + nD;
    }
    const unsigned long long all = __ballot(live);
    if (!all) return;
    const uint32_t qi0 = (uint32_t) __shfl((int) qi, __ffsll((long long) all) - 1, 64);
    unsigned long long *row = a.stats + (uint64_t) qi * ID_STATS;
    if (!__ballot(live && qi != qi0)) {
        // (an operation has a letter at the least and a record's letters lie on two sequences of fewer than 2^22: every sum below 2^31)
        const uint32_t n = (uint32_t) __popcll(all), sI = (uint32_t) cdm_wave_sum((int) nI), sD = (uint32_t) cdm_wave_sum((int) nD), sLI = (uint32_t) cdm_wave_sum((int) lI), sLD = (uint32_t) cdm_wave_sum((int) lD);
        if (lane == __ffsll((long long) all) - 1) {
            atomicAdd(&row[2], (unsigned long long) n);
            if (sI) { atomicAdd(&row[3], (unsigned long long) sI); atomicAdd(&row[5], (unsigned long long) sLI); }
            if (sD) { atomicAdd(&row[4], (unsigned long long) sD); atomicAdd(&row[6], (unsigned long long) sLD); }
        }
    } else if (live) {
        atomicAdd(&row[2], 1ull);
        if (nI) { atomicAdd(&row[3], (unsigned long long) nI); atomicAdd(&row[5], (unsigned long long) lI); }
        if (nD) { atomicAdd(&row[4], (unsigned long long) nD); atomicAdd(&row[6], (unsigned long long) lD); }
    }
}

// the same walk behind the scan: keys, payloads and the side arrays of the record's events, in the record's order
__global__ __launch_bounds__(DP_NT) void k_indel_emit(IndelArgs a, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i >= a.nG) return;
    const cdm_gap_rec r = a.grec[i];
    const uint64_t qkey = (uint64_t) (r.query - a.firstQuery) << ID_QUERY_SHIFT;
    uint32_t e = a.evAt[i];
    const uint32_t end = a.evAt[i + 1];
    indelWalk(r, a.gops, [&](uint32_t p, uint32_t kind, uint32_t g, uint32_t off) {
        if (e >= end) return;       // (the count pass walked the same words)
        a.keys[e] = qkey | (uint64_t) p << ID_POS_SHIFT | (uint64_t) (kind - 1u) << ID_G_BITS | g;
        a.vals[e] = e; a.evRec[e] = (uint32_t) i; a.evOff[e] = off;
        e++;
    });
}

// the track: cross[b] of every boundary of a tile's positions
__global__ __launch_bounds__(DP_NT) void k_indel_track(IndelArgs a, uint64_t first) {
    const Tile t = tileOf(a, first + blockIdx.x);
    const uint32_t *__restrict__ cell = a.cells + t.base + 1;
    uint32_t *__restrict__ out = a.track + (t.base - t.qi);
#pragma unroll
    for (int j = 0; j < DP_PER; j++) {
        const uint64_t b = t.p0 + threadIdx.x + (uint64_t) DP_NT * j;
        if (b < t.len) out[b] = cell[b];
    }
}

// Segments of a sorted array: head[i] = 1 where item i starts one, item i being keys[at ? at[i] : i] >> shift; after the exclusive
// scan of head (head[n] = 0 in front of it) item i starts segment head[i] exactly where head[i + 1] steps, and start[] receives the
// first item of every segment, start[head[n]] = n.
struct HeadArgs { const uint64_t *keys; const uint32_t *at; uint32_t n; int shift; uint32_t *head; uint32_t *start; };
__global__ __launch_bounds__(DP_NT) void k_indel_heads(HeadArgs a, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t mine = a.keys[a.at ? a.at[i] : i] >> a.shift;
    a.head[i] = i == 0 || mine != a.keys[a.at ? a.at[i - 1] : i - 1] >> a.shift;
}
__global__ __launch_bounds__(DP_NT) void k_indel_starts(HeadArgs a, uint64_t first) {
    const uint64_t i = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t seg = a.head[i], next = a.head[i + 1];
    if (next != seg) a.start[seg] = (uint32_t) i;
    if (i + 1 == a.n) a.start[next] = a.n;
}

// A thread per place: its alleles come in ascending g, so the first of the largest counts is the best; flags, the place's record, the
// marks of the two scans, the query's three figures (one atomic of each per wave where its lanes share a query).
__global__ __launch_bounds__(DP_NT) void k_indel_places(IndelArgs a, uint64_t first) {
    const int lane = threadIdx.x & 63;
    const uint64_t pl = (first + blockIdx.x) * DP_NT + threadIdx.x;
    const bool live = pl < a.nPlaces;
    uint32_t qi = 0, supported = 0, major = 0;
    if (live) {
        const uint32_t a0 = a.pStart[pl], a1 = a.pStart[pl + 1];
        uint32_t best = a0, count = 0;
        for (uint32_t al = a0; al < a1 && al - a0 < ID_MAX_GAP; al++) {        // (one allele per length 1..62)
            const uint32_t c = a.aStart[al + 1] - a.aStart[al];
            if (c > count) { count = c; best = al; }
        }
        const uint64_t key = a.skeys[a.aStart[best]];
        const uint32_t g = (uint32_t) key & ((1u << ID_G_BITS) - 1u), kind = ((uint32_t) (key >> ID_G_BITS) & 1u) + 1u, p = (uint32_t) (key >> ID_POS_SHIFT) & 0xFFFFFFu;
        qi = (uint32_t) (key >> ID_QUERY_SHIFT);
        const uint32_t cross = a.cells[a.base[qi] + p + 1u];         // (an event has 1 <= p <= len - 1)
        uint32_t f = 0;
        if (cross >= a.minDepth) {
            f = CDM_INDEL_CALLED;
            if (count >= a.minCount && (unsigned long long) count * 100ull >= (unsigned long long) a.minPct * cross) {
                f |= CDM_INDEL_SUPPORTED;
                if (2ull * count > cross) f |= CDM_INDEL_MAJOR;
            }
        }
        supported = (f & CDM_INDEL_SUPPORTED) != 0; major = (f & CDM_INDEL_MAJOR) != 0;
        cdm_indel_site s;
        s.query = a.firstQuery + qi; s.pos = p; s.info = kind | g << 4 | f << 16; s.count = count; s.cross = cross;
        s.others = a.aStart[a1] - a.aStart[a0] - count; s.n_letters = kind == CDM_INDEL_INS ? g : 0u; s.reserved = 0u; s.letters = 0ull;
        a.pSite[pl] = s; a.pBest[pl] = best;
        a.sMark[pl] = supported; a.lMark[pl] = supported ? (uint64_t) s.n_letters : 0ull;
    }
    const unsigned long long all = __ballot(live);
    if (!all) return;
    const uint32_t qi0 = (uint32_t) __shfl((int) qi, __ffsll((long long) all) - 1, 64);
    unsigned long long *row = a.stats + (uint64_t) qi * ID_STATS;
    if (!__ballot(live && qi != qi0)) {
        const uint32_t n = (uint32_t) __popcll(all), s = (uint32_t) cdm_wave_sum((int) supported), m = (uint32_t) cdm_wave_sum((int) major);
        if (lane == __ffsll((long long) all) - 1) { atomicAdd(&row[7], (unsigned long long) n); if (s) atomicAdd(&row[8], (unsigned long long) s); if (m) atomicAdd(&row[9], (unsigned long long) m); }
    } else if (live) {
        atomicAdd(&row[7], 1ull);
        if (supported) atomicAdd(&row[8], 1ull);
        if (major) atomicAdd(&row[9], 1ull);
    }
}

// the records of the supported places to where the scans put them
__global__ __launch_bounds__(DP_NT) void k_indel_sites(IndelArgs a, uint64_t first) {
    const uint64_t pl = (first + blockIdx.x) * DP_NT + threadIdx.x;
    if (pl >= a.nPlaces) return;
    const uint32_t at = a.sMark[pl];
    if (a.sMark[pl + 1] == at) return;
    cdm_indel_site s = a.pSite[pl];
    s.letters = a.firstLetter + a.lMark[pl];
    a.sites[at] = s; a.siteAllele[at] = a.pBest[pl];
}

// letters: one wave per site record of this launch's slice; a deletion has none.  The lanes take the allele's events; every event
// adds its g read letters to the wave's [62][4] counters in LDS, and lane k < g votes offset k.  indelCheckRecords: the letters of an
// insertion lie at tstart <= offset .. offset + g - 1 < tstart + columns <= tlen, the target's length.
__global__ __launch_bounds__(64 * PU_WAVES) void k_indel_letters(IndelArgs a, uint64_t first, uint64_t nThis) {
    __shared__ uint32_t sCount[PU_WAVES][ID_MAX_GAP * 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t local = (uint64_t) blockIdx.x * PU_WAVES + wave;
    if (local >= nThis) return;
    const cdm_indel_site s = a.sites[first + local];
    const uint32_t g = min(s.n_letters, ID_MAX_GAP);
    if (g == 0) return;
    uint32_t *cnt = sCount[wave];
    for (uint32_t k = lane; k < g * 4u; k += 64) cnt[k] = 0u;
    waveLdsSync();
    const uint32_t al = a.siteAllele[first + local];
    for (uint32_t e = a.aStart[al] + lane, e1 = a.aStart[al + 1]; e < e1; e += 64) {
        const uint32_t ev = a.svals[e];
        const cdm_gap_rec r = a.grec[a.evRec[ev]];
        const uint32_t off = a.evOff[ev], w = a.meta[r.target].woff, rev = r.flags & CDM_MAP_REVERSE;
        for (uint32_t k = 0; k < g; k++) {
            const uint32_t p = rev ? r.tlen - 1u - (off + k) : off + k;
            if (cdm_isN(a.nmask, w, p)) continue;
            const uint32_t b = cdm_base(a.codes, w, p);
            atomicAdd(&cnt[k * 4u + (rev ? 3u - b : b)], 1u);
        }
    }
    waveLdsSync();
    if ((uint32_t) lane < g) {
        uint32_t best = 4u, most = 0u;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++) { const uint32_t c = cnt[(uint32_t) lane * 4u + b]; if (c > most) { most = c; best = b; } }       // the lowest code among equal largest
        a.letters[s.letters - a.firstLetter + lane] = (uint8_t) best;
    }
}

// ---------------------------------------------------------------------------------------------- host
void launchHeads(hipStream_t s, void (*kernel)(HeadArgs, uint64_t), const HeadArgs &h) { launchTiles(s, kernel, h, ((uint64_t) h.n + DP_NT - 1) / DP_NT); }

}  // namespace

static int cdm_indels_impl(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t nq, const cdm_gap_rec *recs, uint64_t nRecs, const uint32_t *ops, uint64_t nOps,
                           const cdm_indel_params *par, uint64_t *stats, uint32_t *track, cdm_indel_site **sites, uint64_t *nSitesOut, uint8_t **lettersOut, uint64_t *nLettersOut, float *kernelMs) {
    static const char *const WHO = "cdm_pileup_indels";
    hipStream_t s = ctx->stream;
    const uint32_t chunk = pileupChunk();
    const uint64_t bound = indelPositions();
    // the records are checked before anything goes up or is launched
    GappedRecords gr; gr.recs = recs; gr.nRecs = nRecs; gr.ops = ops; gr.nOps = nOps;
    if (int rc = gr.check(WHO, db, queries, nq)) return rc;
    QuerySizes qs;
    if (int rc = querySizes(ctx, db, alns, queries, nq, WHO, "cells", qs)) return rc;
    if (int rc = gr.upload(s, WHO)) return rc;
    const DevBuf<cdm_gap_rec> &dRecs = gr.dRecs; const DevBuf<uint32_t> &dOps = gr.dOps;
    float msTotal = 0.f; uint64_t trackAt = 0, g0 = 0;
    for (uint64_t b0 = 0; b0 < nq;) {
        // the batch: listed queries while their cells stay within the bound; a single query longer than the bound goes alone.  The gapped
        // records are sorted by query: the batch's are one contiguous range
        BatchPlan plan; WorkItems work; cdmscan::ScanTemp stCells, stEv, stAllele, stPlace, stSite, stLetter;
        plan.cut(qs.len, b0, 1u, [](uint64_t len) { return len + 1ull; }, bound);
        const uint32_t m = plan.m; const uint64_t nCells = plan.cells, nTrack = nCells - m;
        const uint64_t g1 = gr.end(g0, b0 + m);
        const uint32_t nG = (uint32_t) (g1 - g0);       // (fewer than 2^31 operation words: fewer records)
        const uint64_t recTiles = ((uint64_t) nG + DP_NT - 1) / DP_NT;
        DevBuf<uint32_t> cells, dTrack, evAt; DevBuf<unsigned long long> dStats;
        if (!work.alloc(m) || !plan.alloc() || !cells.alloc(nCells) || !dStats.alloc((size_t) m * ID_STATS) || !evAt.alloc((size_t) nG + 1) || (track && !dTrack.alloc(nTrack))) {
            cdm_set_error("%s: out of device memory for the %llu cells of %u queries and %u gapped records", WHO, (unsigned long long) nCells, m, nG); return CDM_ERR_HIP;
        }
        if (int rc = plan.upload(s)) return rc;
        CDM_HIP(hipMemsetAsync(cells.p, 0, (size_t) nCells * 4, s));
        CDM_HIP(hipMemsetAsync(dStats.p, 0, (size_t) m * ID_STATS * 8, s));
        CDM_HIP(hipMemsetAsync(evAt.p + nG, 0, 4, s));              // (the closing word: the scan leaves the batch's number of events there)
        if (int rc = workItems(s, alns, qs.dq.p + b0, m, chunk, work)) return rc;
        IndelArgs a = {};
        fillArgs(a, qs.meta.p, db, alns, par->min_seq_id, par->skip_extended_targets, work, plan);
        a.codes = db->codes; a.nmask = db->nmask; a.grec = dRecs.p ? dRecs.p + g0 : nullptr; a.gops = dOps.p; a.nG = nG; a.firstQuery = (uint32_t) b0;
        a.minDepth = (uint32_t) par->min_depth; a.minCount = (uint32_t) par->min_count; a.minPct = (uint32_t) par->min_percent;
        a.cells = cells.p; a.stats = dStats.p; a.track = track ? dTrack.p : nullptr; a.evAt = evAt.p; a.firstLetter = *nLettersOut;
        uint32_t nEv = 0;
        hipEventRecord(ctx->ev0, s);
        launchWaveItems(s, k_indel_marks, a, work.n);
        if (nG) {
            launchTiles(s, k_indel_count, a, recTiles);
            if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stEv, evAt.p, evAt.p, (size_t) nG + 1)) return rc;       // (in place: scan.h)
            CDM_HIP(hipMemcpyAsync(&nEv, evAt.p + nG, 4, hipMemcpyDeviceToHost, s));
        }
        if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stCells, cells.p, cells.p, (size_t) nCells)) return rc;
        if (track) launchTiles(s, k_indel_track, a, plan.nTiles);
        hipEventRecord(ctx->ev1, s);
        CDM_LAUNCH_CHECK();
        if (track && nTrack) CDM_HIP(hipMemcpyAsync(track + trackAt, dTrack.p, (size_t) nTrack * 4, hipMemcpyDeviceToHost, s));
        if (int rc = finishTimed(ctx, WHO, "marks", msTotal)) return rc;
        DevBuf<uint64_t> k0, k1, lMark; DevBuf<uint32_t> v0, v1, evRec, evOff, aHead, aStart, pHead, pStart, pBest, sMark, siteAllele; DevBuf<cdm_indel_site> pSite, dSites; DevBuf<uint8_t> dLetters;
        if (nEv) {
            // events, their sort, the alleles
            if (!k0.alloc(nEv) || !k1.alloc(nEv) || !v0.alloc(nEv) || !v1.alloc(nEv) || !evRec.alloc(nEv) || !evOff.alloc(nEv) || !aHead.alloc((size_t) nEv + 1)) {
                cdm_set_error("%s: out of device memory for %u events", WHO, nEv); return CDM_ERR_HIP;
            }
            a.keys = k0.p; a.vals = v0.p; a.evRec = evRec.p; a.evOff = evOff.p; a.nEv = nEv;
            CDM_HIP(hipMemsetAsync(aHead.p + nEv, 0, 4, s));
            bool inFirst = true;        // stable on the key bits in use: the events of an allele stay in record order
            hipEventRecord(ctx->ev0, s);
            launchTiles(s, k_indel_emit, a, recTiles);
            if (int rc = rx::sortPairs<uint64_t, uint32_t>(s, ctx->cuCount, k0.p, k1.p, v0.p, v1.p, (uint64_t) nEv, 0, ID_QUERY_SHIFT + indelBitsFor(m), inFirst)) return rc;
            a.skeys = inFirst ? k0.p : k1.p; a.svals = inFirst ? v0.p : v1.p;
            HeadArgs h = {a.skeys, nullptr, nEv, 0, aHead.p, nullptr};
            launchHeads(s, k_indel_heads, h);
            if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stAllele, aHead.p, aHead.p, (size_t) nEv + 1)) return rc;
            CDM_HIP(hipMemcpyAsync(&a.nAlleles, aHead.p + nEv, 4, hipMemcpyDeviceToHost, s));
            hipEventRecord(ctx->ev1, s);
            CDM_LAUNCH_CHECK();
            if (int rc = finishTimed(ctx, WHO, "event sort", msTotal)) return rc;
            const uint32_t nAlleles = a.nAlleles;
            if (nAlleles < 1 || nAlleles > nEv) { cdm_set_error("%s: %u alleles of %u events", WHO, nAlleles, nEv); return CDM_ERR_HIP; }
            // the places
            if (!aStart.alloc((size_t) nAlleles + 1) || !pHead.alloc((size_t) nAlleles + 1)) { cdm_set_error("%s: out of device memory for %u alleles", WHO, nAlleles); return CDM_ERR_HIP; }
            CDM_HIP(hipMemsetAsync(pHead.p + nAlleles, 0, 4, s));
            h.start = aStart.p;
            HeadArgs hp = {a.skeys, aStart.p, nAlleles, ID_G_BITS, pHead.p, nullptr};
            hipEventRecord(ctx->ev0, s);
            launchHeads(s, k_indel_starts, h);
            launchHeads(s, k_indel_heads, hp);
            if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stPlace, pHead.p, pHead.p, (size_t) nAlleles + 1)) return rc;
            CDM_HIP(hipMemcpyAsync(&a.nPlaces, pHead.p + nAlleles, 4, hipMemcpyDeviceToHost, s));
            hipEventRecord(ctx->ev1, s);
            CDM_LAUNCH_CHECK();
            if (int rc = finishTimed(ctx, WHO, "alleles", msTotal)) return rc;
            const uint32_t nPlaces = a.nPlaces;
            if (nPlaces < 1 || nPlaces > nAlleles) { cdm_set_error("%s: %u places of %u alleles", WHO, nPlaces, nAlleles); return CDM_ERR_HIP; }
            // the best allele of every place, the marks of the supported, the site records
            if (!pStart.alloc((size_t) nPlaces + 1) || !pSite.alloc(nPlaces) || !pBest.alloc(nPlaces) || !sMark.alloc((size_t) nPlaces + 1) || !lMark.alloc((size_t) nPlaces + 1)) {
                cdm_set_error("%s: out of device memory for %u places", WHO, nPlaces); return CDM_ERR_HIP;
            }
            CDM_HIP(hipMemsetAsync(sMark.p + nPlaces, 0, 4, s));
            CDM_HIP(hipMemsetAsync(lMark.p + nPlaces, 0, 8, s));
            hp.start = pStart.p;
            a.aStart = aStart.p; a.pStart = pStart.p; a.pSite = pSite.p; a.pBest = pBest.p; a.sMark = sMark.p; a.lMark = lMark.p;
            const uint64_t placeTiles = ((uint64_t) nPlaces + DP_NT - 1) / DP_NT;
            uint32_t nSites = 0; uint64_t nLetters = 0;
            hipEventRecord(ctx->ev0, s);
            launchHeads(s, k_indel_starts, hp);
            launchTiles(s, k_indel_places, a, placeTiles);
            if (sites) {
                if (int rc = cdmscan::exclusiveScan<uint32_t>(s, stSite, sMark.p, sMark.p, (size_t) nPlaces + 1)) return rc;
                if (int rc = cdmscan::exclusiveScan<uint64_t>(s, stLetter, lMark.p, lMark.p, (size_t) nPlaces + 1)) return rc;
                CDM_HIP(hipMemcpyAsync(&nSites, sMark.p + nPlaces, 4, hipMemcpyDeviceToHost, s));
                CDM_HIP(hipMemcpyAsync(&nLetters, lMark.p + nPlaces, 8, hipMemcpyDeviceToHost, s));
            }
            hipEventRecord(ctx->ev1, s);
            CDM_LAUNCH_CHECK();
            if (int rc = finishTimed(ctx, WHO, "places", msTotal)) return rc;
            if (nSites > nPlaces || nLetters > (uint64_t) nSites * ID_MAX_GAP) { cdm_set_error("%s: %u sites with %llu letters of %u places", WHO, nSites, (unsigned long long) nLetters, nPlaces); return CDM_ERR_HIP; }
            if (nSites) {       // the records of this batch behind those of the batches before it
                if (!dSites.alloc(nSites) || !siteAllele.alloc(nSites) || !dLetters.alloc((size_t) nLetters)) { cdm_set_error("%s: out of device memory for %u site records and %llu letters", WHO, nSites, (unsigned long long) nLetters); return CDM_ERR_HIP; }
                a.sites = dSites.p; a.siteAllele = siteAllele.p; a.letters = dLetters.p;
                hipEventRecord(ctx->ev0, s);
                launchTiles(s, k_indel_sites, a, placeTiles);
                if (nLetters) launchWaveItems(s, k_indel_letters, a, (uint64_t) nSites);
                hipEventRecord(ctx->ev1, s);
                CDM_LAUNCH_CHECK();
                if (int rc = appendRecords(s, WHO, "site", sites, nSitesOut, (const cdm_indel_site *) dSites.p, nSites)) return rc;
                for (uint64_t at = 0; at < nLetters;) {       // (appendRecords takes fewer than 2^32 at a time)
                    const uint32_t nThis = (uint32_t) std::min<uint64_t>(nLetters - at, 1ull << 31);
                    if (int rc = appendRecords(s, WHO, "letter", lettersOut, nLettersOut, (const uint8_t *) dLetters.p + at, nThis)) return rc;
                    at += nThis;
                }
                if (int rc = finishTimed(ctx, WHO, "emission", msTotal)) return rc;
            }
        }
        CDM_HIP(hipMemcpyAsync(stats + b0 * ID_STATS, dStats.p, (size_t) m * ID_STATS * 8, hipMemcpyDeviceToHost, s));
        CDM_HIP(hipStreamSynchronize(s));
        trackAt += nTrack; b0 += m; g0 = g1;
    }
    if (kernelMs) *kernelMs = msTotal;
    return CDM_OK;
}

extern "C" int cdm_pileup_indels(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries, const cdm_gap_rec *recs, uint64_t n_recs,
                                 const uint32_t *ops, uint64_t n_ops, const cdm_indel_params *par, uint64_t *stats, uint32_t *track, cdm_indel_site **sites, uint64_t *n_sites,
                                 uint8_t **letters, uint64_t *n_letters, float *kernel_ms) {
    static const char *const WHO = "cdm_pileup_indels";
    if (alns) CDM_REFUSE_UNDEFINED_ALNS(alns, WHO);
    if (!ctx || !db || !alns || !par || (n_recs && (!recs || !ops)) || (sites && (!n_sites || !letters || !n_letters)) || (!sites && letters) || (n_queries && (!queries || !stats))) {
        cdm_set_error("%s: NULL argument", WHO); return CDM_ERR_INVALID;
    }
    if (par->min_depth < 1 || par->min_depth > 1000000) { cdm_set_error("%s: min_depth = %d; a called place is crossed by 1 to 1000000 reads", WHO, par->min_depth); return CDM_ERR_INVALID; }
    if (par->min_count < 1 || par->min_count > 1000000) { cdm_set_error("%s: min_count = %d; a supported allele has 1 to 1000000 reads", WHO, par->min_count); return CDM_ERR_INVALID; }
    if (par->min_percent < 0 || par->min_percent > 100) { cdm_set_error("%s: min_percent = %d; a percentage of the crossing reads is 0 to 100", WHO, par->min_percent); return CDM_ERR_INVALID; }
    if (int rc = pileupCheckArgs(WHO, db, alns, queries, n_queries)) return rc;
    if (n_ops >> 31) { cdm_set_error("%s: %llu operation words; the 32-bit event slots hold fewer than 2^31", WHO, (unsigned long long) n_ops); return CDM_ERR_UNSUPPORTED; }
    if (letters) { *letters = NULL; *n_letters = 0; }
    uint8_t *gotLetters = NULL; uint64_t nLetters = 0;
    const int rc = runWithRecords(ctx, n_queries, sites, n_sites, kernel_ms, [&](cdm_indel_site **got, uint64_t *nGot, float *ms) {
        return cdm_indels_impl(ctx, db, alns, queries, n_queries, recs, n_recs, ops, n_ops, par, stats, track, got, nGot, got ? &gotLetters : (uint8_t **) NULL, &nLetters, ms);
    });
    if (rc == CDM_OK && letters) { *letters = gotLetters; *n_letters = nLetters; } else free(gotLetters);
    return rc;
}

extern "C" void cdm_indel_free(cdm_indel_site *sites, uint8_t *letters) { free(sites); free(letters); }
