// The device-resident sequence DB container (seqdb.hip): what the other units take from it.  struct cdm_seqdb itself is in common.h.
#pragma once
#include "common.h"

int cdm_seqdb_alloc(cdm_ctx *ctx, uint64_t n, cdm_seqdb **out);      // the five per-sequence arrays; no letters yet
// bytes of the N mask of `words` code words: 16 bits per word, and one 32-bit word more that the window helpers may read
inline uint64_t seqdbMaskBytes(uint64_t words) { return ((words * 16 + 31) / 32 + 1) * 4; }
// codes (two words more than `words`: read past by the window helpers), nmask and, if asked for, raw; sets db->words.  Contents
// undefined.  On failure the error is set and the caller frees db.
int seqdbAllocPlanes(cdm_seqdb *db, uint64_t words, bool withRaw);
int cdm_seqdb_alloc_raw(cdm_seqdb *db);      // the raw plane for db->words code words (contents undefined)
int cdm_seqdb_alloc_like(cdm_ctx *ctx, const cdm_seqdb *src, cdm_seqdb **out);  // same n/lengths/layout, codes uninitialised
// lengths on the device -> woff[0 .. n] and the total, synchronously.  wide: scanned in 64 bits, and more than 2^32 code words refused.
int seqdbLayout(cdm_ctx *ctx, const uint32_t *len, uint64_t n, uint32_t *woff, uint64_t *words, bool wide, const char *who);
int seqdbLenStats(cdm_ctx *ctx, cdm_seqdb *db);      // residues and maxLen of db from its device lengths, synchronously

// ---- constructors without a C-ABI entry
// entry j = text[off[j] .. off[j] + len[j]) (device pointers), key first_key + j, wasExtended ext: packed as cdm_seqdb_upload packs
int cdm_seqdb_from_device_text(cdm_ctx *ctx, const char *text, const uint64_t *off, const uint32_t *len, uint64_t n, uint32_t firstKey, uint8_t ext, cdm_seqdb **out);
// sub-DB: sel[i] (device) = 0xFFFFFFFF drops sequence i, else keeps its first sel[i] letters; extValue < 0 keeps the wasExtended flags
int cdm_seqdb_select(cdm_ctx *ctx, const cdm_seqdb *db, const uint32_t *sel, int extValue, cdm_seqdb **out);
// base with sequence idxHost[j] replaced by grown's sequence j (grown may be NULL); keys are base's, the wasExtended flags the caller's
int cdm_seqdb_overlay(cdm_ctx *ctx, const cdm_seqdb *base, const cdm_seqdb *grown, const uint32_t *idxHost, const uint8_t *extHost, cdm_seqdb **out);

// sequence that owns code word gw: the last i with woff[i] <= gw
__device__ __forceinline__ uint64_t seqOfWord(const uint32_t *__restrict__ woff, uint64_t n, uint64_t gw) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) { uint64_t mid = (lo + hi) >> 1; if (woff[mid] <= gw) lo = mid; else hi = mid; }
    return lo;
}
