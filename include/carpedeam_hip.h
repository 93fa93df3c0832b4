/*
 * carpedeam_hip.h -- C ABI of the MI355X (gfx950) implementation of CarpeDeam's hot path
 *
 *     kmermatcher -> rescorediagonal -> ancient_correction -> ancient_read_assemble
 *
 * This is the drop-in boundary.  The reference has no FFI: its "plugin" surface is the
 * module function  int fn(int argc, const char **argv, const Command&)  (lib/mmseqs/src/commons/Command.h:92-103)
 * whose body is an OpenMP loop over a DBReader.  Each entry point below replaces one such loop; the reference
 * lines it replaces are cited per function.  INTEGRATION.md shows the few lines a maintainer adds to the
 * reference's module bodies to call them.
 *
 * Conventions
 *   - plain C, POD structs, opaque handles; no exceptions cross the boundary.
 *   - every function returns 0 on success, a negative cdm_status otherwise; cdm_last_error() gives the text
 *     (thread local).  There is NO CPU fallback: without a usable gfx950 device cdm_ctx_create fails.
 *   - handles own device memory (HBM); *_download copies into caller-allocated host buffers.
 *   - sequences are addressed by *index* (position in the key-sorted DB index, i.e. DBReader's local id,
 *     lib/mmseqs/src/commons/DBReader.cpp:238-) on the device; keys travel alongside for the host codecs.
 *   - a context is bound to one device and one HIP stream; one context per host thread.
 */
#ifndef CARPEDEAM_HIP_H
#define CARPEDEAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum cdm_status {
    CDM_OK = 0,
    CDM_ERR_NO_DEVICE = -1,   /* no gfx950 device / HIP runtime failure at create */
    CDM_ERR_HIP = -2,         /* HIP API or kernel launch failure */
    CDM_ERR_INVALID = -3,     /* invalid argument / inconsistent input */
    CDM_ERR_UNSUPPORTED = -4, /* input outside what the device path implements (see cdm_last_error) */
    CDM_ERR_IO = -5           /* damage profile could not be read / parsed */
} cdm_status;

typedef struct cdm_ctx cdm_ctx;
typedef struct cdm_seqdb cdm_seqdb; /* 2-bit packed sequence DB resident in HBM */
typedef struct cdm_hits cdm_hits;   /* prefilter hits (kmermatcher output), CSR by query */
typedef struct cdm_alns cdm_alns;   /* ungapped alignments (rescorediagonal output), CSR by query */

const char *cdm_last_error(void);
int cdm_ctx_create(int device_ordinal, cdm_ctx **out);
void cdm_ctx_destroy(cdm_ctx *ctx);
/* blocks until all work queued on the context's stream is done */
int cdm_ctx_sync(cdm_ctx *ctx);
/* the hipStream_t the context launches on (as void*), for callers that time with HIP events */
void *cdm_ctx_stream(cdm_ctx *ctx);
/* device time in ms of the dominant kernel(s) of the last stage call, measured with HIP events on the context stream;
 * which = 0: ancient_correction pile-up/call kernel, 1: rescore kernel, 2: kmermatcher sorts, 3: kmer extraction,
 * 4: extension kernel, 5: kmermatcher sort 1 on the k-mer slots (the library's own onesweep radix passes, csrc/radix.h: histogram +
 * pass launches), 6: sort 2 (run records, their radix sort, aggregation / unit sorters), 7: sort 1 on the whole-sequence hash tuples;
 * 8..11: the WHOLE stage call (everything it launched, host round trips between kernels included) of kmermatcher, rescorediagonal,
 * ancient_correction, ancient_read_assemble; 13: the radix PASS launches of sort 1 on the k-mer slots alone, summed, 14: how many
 * launches that sum covers, 15: the bytes those launches move at the least, in GB - every pair or tuple they sort read once and
 * written once per launch (bench.py's roofline figure); 16: cdm_pileup_profile's counting kernel; 17: cdm_pileup_depth's kernels (marks, prefix
 * sum, statistics), summed over its batches.
 * Returns a negative value when that stage has not run. */
float cdm_ctx_last_kernel_ms(cdm_ctx *ctx, int which);

/* ---------------------------------------------------------------------------------------------------------
 * Sequence DB.  Replaces DBReader<unsigned int>::getData/getSeqLen/getDbKey/getExtData random access
 * (lib/mmseqs/src/commons/DBReader.h:193-213, DBReader.cpp:1001-1012) inside the four stage loops.
 *
 * data      : the DB data file as mapped (entries "SEQUENCE\n\0")
 * offsets[i]: byte offset of entry i in data;  lengths[i]: sequence length WITHOUT "\n\0"
 * keys[i]   : DB key of entry i; entries must be ordered by key (the order DBReader's index has after open()).
 * ext[i]    : the fork's 4th index column "wasExtended" (DBReader.cpp:808-817); may be NULL (= all 0)
 * 'N' is kept as an exception bit beside the 2-bit codes.  Any other byte (lower case, IUPAC codes, ...) is mapped as
 * NucleotideMatrix::setupLetterMapping does (lib/mmseqs/src/commons/NucleotideMatrix.cpp:17-61) for kmermatcher, the
 * diagonal score and reverse complements, and the sequence keeps its original bytes in a side plane for the consumers
 * that look at them (nucleotideMap[c] of the assembler modules, letter identity, the letters copied to the output);
 * cdm_seqdb_download gives them back; the multi-GPU exchange carries them in a section of its own (cdm_seqdb_copy_raw).
 */
int cdm_seqdb_upload(cdm_ctx *ctx, const char *data, const uint64_t *offsets, const uint32_t *lengths,
                     const uint32_t *keys, const uint8_t *ext, uint64_t n, cdm_seqdb **out);
/* Synthetic reads generated on the device with the counter-based generator specified in carpedeam_amd/synth.py
 * (SURVEY.md 8(d)): n reads, fixed length len_lo == len_hi or uniform in [len_lo, len_hi], 20x coverage genome,
 * dhigh damage.  Keys are 0..n-1, ext = 0.  first_read lets a rank generate its own shard [first_read, first_read+n)
 * of a larger corpus (the genome is that of the whole corpus of n_total reads). */
int cdm_seqdb_synth(cdm_ctx *ctx, uint64_t n_total, uint64_t first_read, uint64_t n, uint32_t len_lo, uint32_t len_hi,
                    uint64_t seed, cdm_seqdb **out);
uint64_t cdm_seqdb_size(const cdm_seqdb *db);
uint64_t cdm_seqdb_residues(const cdm_seqdb *db); /* sum of sequence lengths (DBReader::getAminoAcidDBSize) */
uint32_t cdm_seqdb_max_len(const cdm_seqdb *db);
/* lengths/keys/ext: caller arrays of size n (any may be NULL) */
int cdm_seqdb_meta(cdm_ctx *ctx, const cdm_seqdb *db, uint32_t *lengths, uint32_t *keys, uint8_t *ext);
/* ASCII download: out must hold sum(len[i] + 1) bytes; entry i is written at out_offsets[i] followed by '\n' */
int cdm_seqdb_download(cdm_ctx *ctx, const cdm_seqdb *db, char *out, const uint64_t *out_offsets);
/* the same blob in consecutive pieces of (about) piece_bytes through pinned staging buffers of the library: sink(user, data, offset,
 * bytes) gets piece i while piece i + 1 is on its way (data is valid during the call; non-zero return: the download ends with an error).
 * out_offsets must ascend.  What a module process writes its sequence DB with (csrc/host/main.cpp). */
int cdm_seqdb_download_stream(cdm_ctx *ctx, const cdm_seqdb *db, const uint64_t *out_offsets, uint64_t piece_bytes,
                              int (*sink)(void *user, const char *data, uint64_t offset, uint64_t bytes), void *user);
void cdm_seqdb_free(cdm_seqdb *db);
/* Multi-GPU hand-off (one process per GPU, RCCL all-gather of per-shard contigs): the sequences with wasExtended == 1
 * (the contigs an ancient_read_assemble pass produced) as a new DB; its packed form copied into caller-provided DEVICE
 * buffers (e.g. torch tensors that RCCL then all-gathers); and a DB rebuilt from such packed device buffers.
 * Packed form: codes = 16 bases per uint32 (A,C,G,T = 0..3), every sequence starting on a word boundary, nmask = one
 * uint16 per code word (bit j = base j is 'N'), lengths and keys one uint32 per sequence. */
int cdm_seqdb_select_ext(cdm_ctx *ctx, const cdm_seqdb *db, cdm_seqdb **out);
/* The workflow's selection of the assembled contigs (data/nuclassemble.sh:214-233) on resident DBs: of `result` (the final DB of the
 * loop) the entries that are longer than the entry of the same key in `source` (the DB the loop started from; a key `source` does
 * not hold is dropped) and at least min_len letters long (--min-contig-len), in their order, with their keys, wasExtended flags, N
 * and original letters.  The keys of `source` must ascend strictly (CDM_ERR_INVALID otherwise); only its keys and lengths are read
 * (cdm_seqdb_index_copy).  *n_kept (may be NULL) = cdm_seqdb_size(*out); nothing kept is a valid, empty DB. */
/* keys, lengths and wasExtended flags of db as a DB WITHOUT letters: good for cdm_seqdb_meta / cdm_seqdb_size and as the `source` of
 * cdm_seqdb_select_assembled, for nothing that reads sequences. */
int cdm_seqdb_index_copy(cdm_ctx *ctx, const cdm_seqdb *db, cdm_seqdb **out);
int cdm_seqdb_select_assembled(cdm_ctx *ctx, const cdm_seqdb *result, const cdm_seqdb *source, uint32_t min_len, cdm_seqdb **out, uint64_t *n_kept);
uint64_t cdm_seqdb_words(const cdm_seqdb *db);
int cdm_seqdb_copy_packed(cdm_ctx *ctx, const cdm_seqdb *db, void *dev_codes, void *dev_nmask16, void *dev_lengths, void *dev_keys);
int cdm_seqdb_from_packed(cdm_ctx *ctx, const void *dev_codes, const void *dev_nmask16, const void *dev_lengths, const void *dev_keys,
                          uint64_t n, uint64_t words, uint8_t ext_value, cdm_seqdb **out);
/* A DB with letters beyond ACGTN (cdm_seqdb_has_raw != 0) has more to hand over than the packed form holds: the original bytes,
 * 16 per code word (dev_raw: words * 16 bytes; rows of sequences without such letters are undefined), and one byte per sequence
 * saying whether its row counts (dev_flags: n bytes).  cdm_seqdb_attach_raw gives them to a DB rebuilt by cdm_seqdb_from_packed*;
 * an exchange that leaves them out would silently turn 'acgt' into what NucleotideMatrix maps it to. */
int cdm_seqdb_has_raw(const cdm_seqdb *db);
int cdm_seqdb_copy_raw(cdm_ctx *ctx, const cdm_seqdb *db, void *dev_raw, void *dev_flags);
int cdm_seqdb_attach_raw(cdm_ctx *ctx, cdm_seqdb *db, const void *dev_raw, const void *dev_flags);
/* the same with one wasExtended flag per sequence (device array of n bytes, NULL = all 0), and the flags of a DB copied out:
 * the query-sharded stages of a multi-GPU run hand whole DB slices around, flags included */
int cdm_seqdb_from_packed_ext(cdm_ctx *ctx, const void *dev_codes, const void *dev_nmask16, const void *dev_lengths, const void *dev_keys,
                              const void *dev_ext, uint64_t n, uint64_t words, cdm_seqdb **out);
int cdm_seqdb_copy_ext(cdm_ctx *ctx, const cdm_seqdb *db, void *dev_ext);
/* The same packed form to and from HOST buffers: what a module process leaves in a binary side-car next to the sequence DB it read or wrote
 * (csrc/host/sidecar.cpp), so that the next module of data/nuclassemble.sh:100-146 uploads 2 bits per base instead of parsing and packing
 * the text DB again (lib/mmseqs/src/commons/DBReader.cpp:108-133, DBWriter.cpp:322-427 stay the format every reference module reads).
 * nmask16 / raw / raw_flags may be NULL: export - not wanted; import - no letter beyond ACGT / no raw plane.  raw_flags of an export:
 * one byte per sequence, bit 0 = the sequence has a letter beyond ACGT, bit 1 = its row of the raw plane counts. */
/* a's entries, then b's, as one DB on the device: keys 0 .. n_a + n_b - 1, the wasExtended flags of the two parts set to ext_a and
 * ext_b, N and original letters carried along (a raw plane in either part gives the result one).  What a caller runs kmermatcher /
 * rescorediagonal on to lay one set of sequences over another (contigs and the reads they were built from: cdm_pileup_profile).
 * Both parts must hold their letters (not a cdm_seqdb_index_copy); fewer than 2^32 - 1 sequences and 2^32 code words in all. */
int cdm_seqdb_concat(cdm_ctx *ctx, const cdm_seqdb *a, const cdm_seqdb *b, uint8_t ext_a, uint8_t ext_b, cdm_seqdb **out);
int cdm_seqdb_export_packed(cdm_ctx *ctx, const cdm_seqdb *db, void *codes, void *nmask16, void *lengths, void *keys, void *ext, void *raw, void *raw_flags);
int cdm_seqdb_import_packed(cdm_ctx *ctx, const void *codes, const void *nmask16, const void *lengths, const void *keys, const void *ext, const void *raw,
                            const void *raw_flags, uint64_t n, uint64_t words, cdm_seqdb **out);

/* ---------------------------------------------------------------------------------------------------------
 * Damage model.  Replaces the per-thread initDeamProbabilities + getSeqErrorProf calls
 * (src/assembler/correction.cpp:184-197, ancientReadsResults.cpp:161-173; nuclassembleUtil.cpp:821-1007,49-65).
 * prefix is --ancient-damage: files <prefix>5p.prof and <prefix>3p.prof; "" means no damage (zero matrices).
 * The host side of the library builds the 11+11 substitution matrices in the reference's mixed
 * long double/double arithmetic and from them the log look-up tables the kernels use.
 */
int cdm_damage_load(cdm_ctx *ctx, const char *prefix);
/* the 2 x 11 x 4 x 4 matrices as long double (fwd then rev), for tests */
int cdm_damage_get(cdm_ctx *ctx, long double *out352);

/* ---------------------------------------------------------------------------------------------------------
 * kmermatcher.  Replaces doComputation + writeKmerMatcherResult + the fill-in loop
 * (lib/mmseqs/src/linclust/kmermatcher.cpp:391-451, 453-562, 815-930, 717-729) in single-split semantics.
 */
typedef struct cdm_kmer_params {
    int32_t kmer_size;               /* -k (20 for reads, 22 for contigs) */
    int32_t kmers_per_seq;           /* --kmer-per-seq */
    float kmers_per_seq_scale;       /* --kmer-per-seq-scale */
    uint64_t hash_shift;             /* --hash-shift (xxhash seed) */
    int32_t ignore_multi_kmer;       /* --ignore-multi-kmer */
    int32_t include_only_extendable; /* --include-only-extendable */
    int32_t cov_mode;                /* --cov-mode */
    float cov_thr;                   /* -c */
} cdm_kmer_params;

/* one prefilter line "targetKey \t score \t diagonal" (lib/mmseqs/src/prefiltering/QueryMatcher.h:35-39,114-126);
 * score < 0 means the query has to be reverse-complemented */
typedef struct cdm_hit {
    uint32_t target; /* sequence index (not key) */
    int32_t score;
    int32_t diagonal; /* already truncated to short as the reference stores it */
} cdm_hit;

int cdm_kmermatch(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_kmer_params *par, cdm_hits **out);
/* offsets: n+1 entries (CSR by query index); every query has at least its self hit as first record */
int cdm_hits_upload(cdm_ctx *ctx, const cdm_seqdb *db, const uint64_t *offsets, const cdm_hit *hits, cdm_hits **out);
uint64_t cdm_hits_count(const cdm_hits *h);
int cdm_hits_download(cdm_ctx *ctx, const cdm_hits *h, uint64_t *offsets, cdm_hit *hits);
void cdm_hits_free(cdm_hits *h);

/* kmermatcher split over several GPUs without changing its result (the reference's MPI path splits the k-mer
 * space the same way, lib/mmseqs/src/linclust/kmermatcher.cpp:634-663, but merges per-split results lossily - here the
 * single-split semantics are kept).  Every rank holds the whole sequence DB.
 *   cdm_kmermatch_part   doComputation's first half (:391-430) on the k-mer range part/nparts (ranges are equal slices of the
 *                        2k-bit k-mer space in k-mer order; the whole-sequence hash tuples belong to the last range): extraction,
 *                        sort 1, assignGroup -> (rep, id, diagonal, strand) group keys of this range
 *   cdm_kpart_info       info[0] real tuples of the range, [1] kept group keys, [2] 1 if a real tuple lies below the range, [3] n
 *   cdm_kpart_stale      the left-over list of the reference's run-past-the-end scan (kmermatcher.cpp:875-887) from local
 *                        k-mer-order index J of this range: out[0] count, out[1] sequence id, out[2..63] positions, out[66] = 1 if
 *                        the scan consumed every tuple up to the end of the range (then it goes on in the next range)
 *   cdm_kpart_gather     the group keys grouped by representative (k-mer order inside); offsets[r]..offsets[r+1] is the slice
 *                        for the rank that owns representatives [r n/nranks, (r+1) n/nranks); *dev_keys is a DEVICE pointer
 *                        owned by the handle (send buffer of the all-to-all)
 *   cdm_kpart_sort       second half, sort 2 (:431), on the keys received from all ranks, concatenated in rank order (device
 *                        buffer).  head (cdm_kpart_cont_cap() + 3 values): the start of the sorted array while the target id
 *                        stays that of the first tuple - what the per-target scan of the rank in front runs into
 *                        (head[0] count, head[1] that id, head[2] = 1 if it is the whole array, head[3..] entries);
 *                        info[0] = sorted tuples, info[1] = target id of the last one
 *   cdm_kpart_vote       writeKmerMatcherResult (:815-930): hits of the representatives this rank owns (every other sequence gets
 *                        its self hit only).  cont: what this rank's last scan runs into, built from the later ranks' heads
 *                        (cont[0] entries, cont[1] = this rank's last target id, cont[2] = 1 if the scan then goes on into the
 *                        left-over list, cont[3..] entries; NULL = nothing but the left-over list behind this rank's tuples);
 *                        stale = the combined left-over list (65 values as above)
 */
typedef struct cdm_kpart cdm_kpart;
int cdm_kmermatch_part(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_kmer_params *par, int part, int nparts, cdm_kpart **out);
/* The same first half with the extraction split by READS (what cdm_kmermatch_dist does): rank r extracts the k-mers of ITS block of the
 * sequences only - block r of nranks of the (length descending, id ascending) order fillKmerPositionArray's result is sorted into
 * (kmermatcher.cpp:391-430), the blocks cut so that they hold about the same number of k-mer slots - and orders its tuples by
 * CDM_KPART_SLICES equal slices of the k-mer space (its top 8 bits: one radix pass).  cdm_kpart_outgoing names the send buffers (offsets[s]..offsets[s+1] = the tuples of
 * slice s, keys 8 bytes and values *val_bytes each; the whole-sequence hash tuples sort behind every k-mer).  The CALLER cuts the
 * ranks' k-mer ranges as runs of slices from all ranks' counts (canonical k-mers crowd the low end of the k-mer space: equal slices
 * are not equal shares), sends every range to its rank and the hash tuples to the last one; cdm_kmermatch_split_finish takes what
 * arrived, CONCATENATED IN RANK ORDER (device buffers; `below` = 1 if any rank holds a tuple of a range in front of this one), and
 * leaves the handle where cdm_kmermatch_part leaves it (rank r of nranks ranges). */
#define CDM_KPART_SLICES 256
int cdm_kmermatch_split_begin(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_kmer_params *par, int rank, int nranks, cdm_kpart **out);
int cdm_kpart_outgoing(const cdm_kpart *h, uint64_t *offsets, const void **keys, const void **vals, int *val_bytes,
                       const void **hash_keys, const void **hash_vals, uint64_t *n_hash);
int cdm_kpart_set_range(cdm_kpart *h, int rank, int nranks);     /* before split_finish: finish as range `rank` of `nranks` (a handle begun as block 0 of 1: all sequences) */
int cdm_kmermatch_split_finish(cdm_ctx *ctx, cdm_kpart *h, const void *keys, const void *vals, uint64_t m,
                               const void *hash_keys, const void *hash_vals, uint64_t n_hash, int below);
int cdm_kpart_info(const cdm_kpart *h, uint64_t info[4]);
int cdm_kpart_stale(cdm_ctx *ctx, cdm_kpart *h, uint64_t J, uint32_t out[67]);
int cdm_kpart_gather(cdm_ctx *ctx, cdm_kpart *h, int nranks, uint64_t *offsets, const void **dev_keys);
/* the same with the owners' ranges given: offsets[t] = first key whose representative is >= bounds[t] (nb ascending sequence ids; the
 * keys are grouped by representative on the first call).  cdm_kmermatch_dist calls it twice: with 4097 equal bounds for a histogram of
 * keys per id range, then with the nranks + 1 bounds it cut from all ranks' histograms. */
int cdm_kpart_gather_at(cdm_ctx *ctx, cdm_kpart *h, int nb, const uint64_t *bounds, uint64_t *offsets, const void **dev_keys);
int cdm_kpart_sort(cdm_ctx *ctx, cdm_kpart *h, const void *dev_keys, uint64_t n_keys, uint32_t *head, uint64_t info[2]);
int cdm_kpart_vote(cdm_ctx *ctx, cdm_kpart *h, const uint32_t *cont, const uint32_t *stale, cdm_hits **out);
int cdm_kpart_cont_cap(void);
/* sort 1 on the 8-byte slot layout (a DB of one read length, 14 <= k <= 20): *low_bits = how many of the 2k k-mer bits the global radix
 * passes leave to the grouping kernel - max(0, 2k - 27), or what the A/B switch CDM_SLOT_LOWBITS=<n> asks for.  CDM_ERR_INVALID for a k
 * the layout does not take and for a switch outside 0 <= 2k - 9 - n <= 18.  Needs no device. */
int cdm_kmer_slot_split(int k, int *low_bits);
void cdm_kpart_free(cdm_kpart *h);
/* tuning: head room of the library's device-memory cache for callers whose inputs grow from call to call (the contig iterations of
 * the workflow loop): large blocks are allocated `factor` times the request, so the next, larger request fits a cached block instead of
 * mapping device memory anew.  1 = off (default); process-wide. */
void cdm_pool_headroom(float factor);
/* the allocator's counters since the process began: [0] requests, [1] served without the driver, [2] calls that asked the driver for
 * memory, [3] their bytes, [4] the nanoseconds they took, [5] times free memory was given back after an out-of-memory; and now:
 * [6] bytes mapped into the arenas of all threads, [7] bytes of them in blocks that are in use (head room included) */
void cdm_pool_stats(uint64_t out[8]);
/* The library reads its CDM_* switches (A/B and test aids) from the environment ONCE per process, not with getenv() on
 * its call paths (getenv is not safe beside a setenv elsewhere in the process).  cdm_env_refresh() reads them again - for tests and A/B
 * runs that change a switch inside one process; call it while no other thread is inside the library. */
void cdm_env_refresh(void);
/* device-to-device copy on the context's stream (synchronises it): moves library-owned buffers into caller tensors */
int cdm_dev_copy(cdm_ctx *ctx, void *dst, const void *src, uint64_t bytes);

/* ---------------------------------------------------------------------------------------------------------
 * rescorediagonal (--rescore-mode 3, query DB == target DB).  Replaces the loop at
 * lib/mmseqs/src/alignment/rescorediagonal.cpp:145-356 (DistanceCalculator.h:93-175,204-220).
 */
typedef struct cdm_rescore_params {
    float seq_id_thr; /* --min-seq-id */
    double eval_thr;  /* -e */
    int32_t cov_mode; /* --cov-mode */
    float cov_thr;    /* -c */
    int32_t seq_id_mode; /* --seq-id-mode (0 only) */
    int32_t min_aln_len; /* --min-aln-len */
} cdm_rescore_params;

/* one alignment record = the ten text columns of Matcher::resultToBuffer (lib/mmseqs/src/alignment/Matcher.cpp:356-404)
 * minus lengths (taken from the seq DB); raw_score/ident let the host derive bit score, E-value and seq.id. text.
 * q_start > q_end encodes a reverse-strand hit as in the reference (rescorediagonal.cpp:294-297). */
typedef struct cdm_aln {
    uint32_t target;  /* sequence index */
    int32_t raw_score;
    int32_t ident;    /* identical columns */
    int32_t q_start, q_end, db_start, db_end;
    float seq_id;     /* value a reader of the text record gets: (float)strtod(fastSeqIdToBuffer(ident/alnLen)) */
} cdm_aln;

/* CDM_ERR_UNSUPPORTED (the message names -e) when eval_thr lets a raw score of 0 pass for the length of any sequence in db, whether or not a
 * hit has it as its query: the reference's record for such a hit that is no identity hit is undefined (coordinates -1, read outside both). */
int cdm_rescore(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_hits *hits, const cdm_rescore_params *par, cdm_alns **out);
/* What cdm_rescore keeps beside the records, and the size of its kernel's tile (for tests that place inputs on tile boundaries):
 * hits per block of the scoring kernel; the number of identity records written with the coordinates -1 (a sequence that scores 0
 * against itself); the purine/pyrimidine mismatch count of every record, cdm_alns_count values (0xFFFF = not counted; fails with
 * CDM_ERR_INVALID for a set that has none, i.e. one made by cdm_alns_upload). */
uint32_t cdm_rescore_tile(void);
uint64_t cdm_alns_undefined(const cdm_alns *a);
int cdm_alns_ry_download(cdm_ctx *ctx, const cdm_alns *a, uint16_t *ry);
/* rescorediagonal --rescore-mode 0 --wrapped-scoring 1 (query DB == target DB): linclust's Hamming-distance pre-clustering of the
 * assembled contigs (lib/mmseqs/data/workflow/linclust.sh:27-31; rescorediagonal.cpp:145-356 in that mode,
 * DistanceCalculator::computeUngappedWrappedAlignment, DistanceCalculator.h:57-91).  Output: the hits that pass, as prefilter
 * records (target, 100 * seq. id. signed by the strand, diagonal), same CSR over the queries. */
typedef struct cdm_hamming_params {
    float seq_id_thr;   /* --min-seq-id */
    double eval_thr;    /* -e (the mode's E-value is 0: only a negative threshold drops everything) */
    int32_t cov_mode;   /* --cov-mode */
    float cov_thr;      /* -c */
    int32_t seq_id_mode; /* --seq-id-mode 0 | 1 | 2 */
    int32_t min_aln_len; /* --min-aln-len */
    int32_t reverse_prefilter; /* the prefilter DB's type is DBTYPE_PREFILTER_REV_RES (kmermatcher's): a negative score = reverse-strand hit */
} cdm_hamming_params;
int cdm_rescore_hamming(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_hits *hits, const cdm_hamming_params *par, cdm_hits **out);
int cdm_alns_upload(cdm_ctx *ctx, const cdm_seqdb *db, const uint64_t *offsets, const cdm_aln *alns, cdm_alns **out);
uint64_t cdm_alns_count(const cdm_alns *a);
int cdm_alns_download(cdm_ctx *ctx, const cdm_alns *a, uint64_t *offsets, cdm_aln *alns);
void cdm_alns_free(cdm_alns *a);
/* host helpers for the text codec of the alignment DB: E-value, bit score (EvalueComputation.h:18-40 over ALP) */
double cdm_evalue(double raw_score, double query_len, uint64_t db_residues);
/* E-value and bit score of a GAPPED nucleotide alignment (the `align` step of linclust; Alignment.cpp:273: EvalueComputation with gap
 * costs): implemented for --gap-open 5 --gap-extend 2, whose Gumbel parameters are ALP's estimate taken from the reference's object code */
int cdm_gapped_evalue(int gap_open, int gap_extend, double raw_score, double query_len, uint64_t db_residues, double *evalue, int *bit_score);
int cdm_bit_score(double raw_score);

/* ---------------------------------------------------------------------------------------------------------
 * align (linclust's gapped step on the assembled contigs; nucleotides, no backtrace output).  Replaces what
 * BandedNucleotideAligner::align does between the ungapped seed and the result (lib/mmseqs/src/alignment/
 * BandedNucleotideAligner.cpp:138-255 over lib/mmseqs/lib/ksw2/ksw2_extz2_sse.cpp:45-284) for a batch of independent hits: the reverse
 * extension from the seed's end, the forward one from the start that found, the second reverse run where the first reached further,
 * identities and columns of the edit script.  csrc/align.hip; the seed, E-values, filters and the text stay with the caller
 * (csrc/host/align.cpp).  nucleotide.out's scores (+2 / -3, N a wildcard), band 64.
 *
 * A hit: query and target by index; reverse = the query is reverse-complemented; wrapped = --wrapped-scoring 1 (the query is its
 * sequence twice); q_len / t_len = the lengths as aligned (the doubled query cut at 2 x --max-seq-len, the target at its cut);
 * q_end / t_end = the seed's last column in the aligned query / the target.  The reference runs its reverse extension on arrays
 * shifted by one letter, whose first element is the byte behind the sequence in the worker thread's buffer - left there by an
 * earlier, longer sequence: stale_q / stale_t are those letters (A,C,G,T = 0..3, 4 = N; 0 in a fresh buffer).
 * stats (may be NULL): [0] slices the hits ran in, [1] anti-diagonal rows computed, [2] trace bytes of the largest slice,
 * [3] microseconds from the first launch to the last slice's end.
 */
typedef struct cdm_align_params {
    int32_t gap_open, gap_extend; /* --gap-open, --gap-extend */
    int32_t zdrop;                /* --zdrop */
    int32_t band;                 /* 64 */
} cdm_align_params;
typedef struct cdm_align_hit {
    uint32_t query, target;
    uint32_t q_len, t_len;
    int32_t q_end, t_end;
    uint8_t reverse, wrapped, stale_q, stale_t;
} cdm_align_hit;
typedef struct cdm_align_result {
    int32_t score;                  /* raw score of the gapped alignment */
    int32_t q_start, q_end, t_start, t_end;
    int32_t identities, columns;    /* aaIds and the length of the edit script */
    int32_t rows;                   /* anti-diagonal rows the hit's extensions computed */
} cdm_align_result;
int cdm_align_hits(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_align_params *par, const cdm_align_hit *hits, uint64_t n,
                   cdm_align_result *results, uint64_t *stats);
/* the CDM_ALIGN switch of the `align` module from the library's snapshot of the environment: 0 unset (the module takes its host
 * path), 1 host, 2 device; CDM_ERR_INVALID for any other value */
int cdm_align_mode(void);

/* ---------------------------------------------------------------------------------------------------------
 * ancient_correction.  Replaces the loop at src/assembler/correction.cpp:200-476 (mostLikeliBaseRead :7-123).
 * Output: a new sequence DB with identical keys/lengths/flags and corrected bases.
 */
typedef struct cdm_ancient_params {
    float seq_id_thr;            /* --min-seq-id */
    float corr_reads_ry_seq_id;  /* --min-ryseq-id-corr-reads */
    float ry_seq_id_thr;         /* rySeqIdThr (not settable on the module's command line; 0.99) */
    float rand_align_penal;      /* --ext-random-align */
    float excess_penal;          /* --excess-penalty */
    float likelihood_threshold;  /* --likelihood-ratio-threshold */
    int32_t unsafe;              /* --unsafe: 1 = consensusCaller's majority vote over the extending targets (nuclassembleUtil.cpp:570-702) */
    int32_t min_cov_safe;        /* --min-cov-safe */
    uint64_t max_seq_len;        /* --max-seq-len */
} cdm_ancient_params;

int cdm_correct(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const cdm_ancient_params *par, cdm_seqdb **out);

/* ---------------------------------------------------------------------------------------------------------
 * Coverage and damage tables of the read pile-up (not a module of the reference; csrc/pileup.hip).  For every listed query the
 * records of its row that ancient_correction would orient and pile up (correction.cpp:229-242) are COUNTED instead: a record r of
 * query q counts when r.target != q, r.seq_id >= min_seq_id (float comparison; 0 takes all) and - with skip_extended_targets - the
 * target's wasExtended flag is 0.  For each of its columns c = 0 .. qe - qs: op = ds + c is the column on the oriented target,
 * p = rev ? tLen - 1 - op : op the position in the read's own orientation, y the read's own code at p, x the query's code at qs + c,
 * complemented when rev (the query base as the read's strand sees it).  A column with an N on either side counts in `columns` only;
 * any other adds one to c5[p][x][y] when p < ends and one to c3[tLen - 1 - p][x][y] when tLen - 1 - p < ends (a short read lands in
 * both).  Letters are the mapped codes and N bits (the NucleotideMatrix view), never the raw plane.
 *   counts   n_queries x 2 x ends x 16 uint64: per query the 5' table, then the 3' table, each [d][x][y] with A,C,G,T = 0..3
 *   reads    n_queries uint64: records counted;  columns: n_queries uint64: sum of qe - qs + 1 over them
 * ends in 1..64; a query index >= the DB's size or listed twice is CDM_ERR_INVALID; n_queries == 0 is CDM_OK (nothing is launched);
 * a set with the coordinates -1 record is refused as cdm_correct refuses it.  The 5' C->T rate at distance d is
 * c5[d][C][T] / sum_y c5[d][C][y], the 3' G->A rate c3[d][G][A] / sum_y c3[d][G][y]; the library hands out the integers.
 * Coverage here is coverage by seeded ungapped overlaps at the set's identity threshold, not by a gapped mapping.
 * Device time of the counting kernel: cdm_ctx_last_kernel_ms(ctx, 16). */
typedef struct cdm_pileup_params { int32_t ends; float min_seq_id; int32_t skip_extended_targets; } cdm_pileup_params;
int cdm_pileup_profile(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries,
                       const cdm_pileup_params *par, uint64_t *counts, uint64_t *reads, uint64_t *columns);

/* ---------------------------------------------------------------------------------------------------------
 * Depth of coverage at every position of the listed queries, and its statistics (not a module of the reference; csrc/pileup_depth.hip).
 * A record r of a listed query q of `len` letters counts under exactly the rule of cdm_pileup_profile: r.target != q,
 * r.seq_id >= min_seq_id (float against float), with skip_extended_targets the target's wasExtended flag is 0, and the oriented
 * record fits both sequences.  The oriented record covers the query positions qs..qe; depth[i] = the number of counted records with
 * qs <= i <= qe.  A position counts whether or not it holds an N (as `columns` does).
 * The statistics window is the whole query when len <= 2 * edge, else the positions edge .. len - 1 - edge (binning tools take mean
 * and variance away from the contig ends, where reads cannot overhang); no query of at least one letter gets an empty window.
 *   stats   n_queries x 8 uint64, per listed query:
 *             0 reads    records counted (cdm_pileup_profile's)      1 columns  sum of qe - qs + 1 over them (cdm_pileup_profile's; the
 *                                                                               sum of depth over the whole query)
 *             2 breadth  positions of the whole query with depth >= 1  3 window   positions in the statistics window
 *             4 covered  window positions with depth >= 1              5 sum      sum of depth over the window
 *             6 sumsq    sum of depth^2 over the window                7 max      largest depth in the window
 *   depth   NULL, or the depth of every position as uint32: the listed queries back to back in listed order (the sum of their lengths)
 * The library hands out integers; the caller divides: mean = sum / window, variance = (sumsq - sum^2 / window) / (window - 1).
 * edge < 0, a query index >= the DB's size or listed twice are CDM_ERR_INVALID; n_queries == 0 is CDM_OK (nothing is launched); a set
 * with the coordinates -1 record is refused as cdm_pileup_profile refuses it.  Two bounds are refused with CDM_ERR_UNSUPPORTED, never
 * wrapped: a listed query with 2^32 records or more (the depth cells are 32 bits wide), and a query whose max * sum does not fit
 * 64 bits (the upper bound of sumsq, checked in 128-bit arithmetic after the kernels).  Neither is reachable at test size, and
 * neither is tested.
 * As with the damage tables, this is coverage by seeded ungapped overlaps at the set's identity threshold, not by a gapped mapping.
 * Device time of the kernels: cdm_ctx_last_kernel_ms(ctx, 17). */
typedef struct cdm_depth_params { int32_t edge; float min_seq_id; int32_t skip_extended_targets; } cdm_depth_params;
int cdm_pileup_depth(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries,
                     const cdm_depth_params *par, uint64_t *stats, uint32_t *depth);

/* ---------------------------------------------------------------------------------------------------------
 * Per-position base counts and variant sites of the read pile-up (not a module of the reference; csrc/pileup_bases.hip): which bases the
 * reads put on every position of the listed queries, and the positions where that disagrees with the query or among the reads.
 * A record counts under exactly the rule of cdm_pileup_profile and cdm_pileup_depth.  Column c = i - qs of a counted, oriented record
 * on query position i: op = ds + c, p = rev ? tLen - 1 - op : op the position in the read's own orientation.  The column is left out
 * when the read has its N bit at p, and - with mask_ends = m > 0 - when p < m or tLen - 1 - p < m (genotyping of ancient DNA leaves
 * the damaged read ends out).  Otherwise b = the read's mapped code at p, complemented (3 - b) when rev - the read base as the
 * query's strand sees it - and counts[i][rev * 4 + b] += 1: forward counters A,C,G,T, then reverse counters A,C,G,T.  The query's own
 * letter plays no part in the counts; letters are the mapped codes and N bits, never the raw plane.
 * Per position, with t[b] = counts[i][b] + counts[i][4 + b] and d = sum of t: ref = the query's code, 4 when its N bit is set;
 * major = the base with the largest t, among equal largest ref if it is one of them, else the lowest code; second = the largest t
 * over the three other bases.  Flags, integers only (the percent rule in 64 bits):
 *   CDM_SITE_CALLED   d >= min_depth
 *   CDM_SITE_DIFFERS  called, major != ref (a query N differs from any base) and t[major] strictly greater than the other three
 *   CDM_SITE_VARIABLE called, second >= min_alt_count and second * 100 >= min_alt_percent * d
 *   stats   n_queries x 8 uint64, per listed query:
 *             0 reads, 1 columns   cdm_pileup_profile's and cdm_pileup_depth's values (masked and N columns included)
 *             2 bases              sum of all counters of the query
 *             3 mismatches         sum of d - t[ref] over the positions with ref != 4
 *             4 called, 5 differs, 6 variable   positions with that flag
 *             7 flagged            positions with DIFFERS or VARIABLE: the query's number of site records
 *   counts  NULL, or uint32 [sum of the listed queries' lengths][8]: the queries back to back in listed order
 *   sites   NULL, or receives a malloc'ed array (cdm_sites_free) of one record per flagged position in listed query order, then
 *           ascending pos: query = the index into `queries`, info = ref | major << 4 | flags << 8, counts = the position's row.
 *           *n_sites = their number; n_queries == 0 or no flagged position: *sites = NULL, *n_sites = 0.  n_sites may be NULL only
 *           when sites is
 *   kernel_ms  NULL, or receives the device time of the kernels (cdm_ctx_last_kernel_ms has no slot for this call)
 * mask_ends in 0..64, min_depth >= 1, min_alt_count >= 1, min_alt_percent in 0..100; anything else, a NULL argument, a query index
 * >= the DB's size or listed twice is CDM_ERR_INVALID; n_queries == 0 is CDM_OK (nothing is launched); a set with the coordinates -1
 * record is refused as cdm_pileup_profile refuses it; a listed query with 2^32 records or more is CDM_ERR_UNSUPPORTED (the counters
 * are 32 bits wide; not reachable at test size, not tested).  As with the two tables above, the pile-up is the set's seeded
 * ungapped overlaps at its identity threshold, not a gapped mapping: no indels, and no call where no read seeds. */
#define CDM_SITE_CALLED 1u
#define CDM_SITE_DIFFERS 2u
#define CDM_SITE_VARIABLE 4u
typedef struct cdm_bases_params {
    int32_t mask_ends;        /* 0..64: read positions left out at either end of a read */
    int32_t min_depth;        /* >= 1 */
    int32_t min_alt_count;    /* >= 1 */
    int32_t min_alt_percent;  /* 0..100 */
    float   min_seq_id;
    int32_t skip_extended_targets;
} cdm_bases_params;
typedef struct cdm_site { uint32_t query, pos, info, counts[8]; } cdm_site;   /* 44 bytes */
int  cdm_pileup_bases(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries,
                      const cdm_bases_params *par, uint64_t *stats, uint32_t *counts, cdm_site **sites, uint64_t *n_sites, float *kernel_ms);
void cdm_sites_free(cdm_site *sites);

/* ---------------------------------------------------------------------------------------------------------
 * Contig break points from spanning reads (not a module of the reference; csrc/pileup_depth.hip): is a query one molecule, or two stitched
 * together?  A read that crosses a false join collects mismatches on the far side and falls below the set's identity threshold, so
 * across a false join reads cover both flanks but none spans the boundary with a real anchor on either side - which depth cannot see.
 * A record counts under exactly the rule of the three reductions above; the oriented record covers the query positions qs..qe.
 * Boundary b of a query of `len` letters, 1 <= b <= len - 1, lies between the positions b - 1 and b.  With w = anchor:
 *   span[b]   the number of counted records with qs + w <= b <= qe + 1 - w: at least w columns on either side of the boundary (a
 *             record of fewer than 2 w columns spans nothing)
 *   depth[i]  as in cdm_pileup_depth
 *   window    the boundaries with edge <= b <= len - edge; empty when len < 2 * edge or len < 2
 *   weak      a window boundary with span[b] < min_span, or - with min_span_percent > 0 - with
 *             span[b] * 100 < min_span_percent * min(depth[b - 1], depth[b]) (64 bits)
 *   break     a maximal run first..last of consecutive weak boundaries of one query: min_span = the smallest span of the run,
 *             uncovered = the positions first .. last - 1 with depth 0, depth_left = depth[first - 1], depth_right = depth[last],
 *             flags = CDM_BREAK_GAP where uncovered > 0, else CDM_BREAK_JOIN (the reads cover the stretch and none spans it: the
 *             signature of a chimeric join)
 *   stats   n_queries x 8 uint64, per listed query:
 *             0 reads, 1 columns   cdm_pileup_depth's values       2 window    boundaries examined
 *             3 weak               weak boundaries                 4 breaks    runs of them
 *             5 joins              runs flagged CDM_BREAK_JOIN     6 min_span  smallest span over the window, 0 where it is empty
 *             7 sum_span           sum of span over the window
 *   track   NULL, or uint32 [sum of the listed queries' lengths]: per listed query span[b] for b = 0 .. len - 1 (span[0] = 0), the
 *           queries back to back in listed order
 *   breaks  NULL, or receives a malloc'ed array (cdm_breaks_free) of one record per break in listed query order, then ascending
 *           first; query = the index into `queries`.  *n_breaks = their number; none: *breaks = NULL, *n_breaks = 0.  n_breaks may be
 *           NULL only when breaks is
 *   kernel_ms  NULL, or receives the device time of the kernels
 * anchor in 1..1024, edge in anchor..1048576, min_span in 1..1000000, min_span_percent in 0..100; anything else, a NULL argument, a
 * query index >= the DB's size or listed twice is CDM_ERR_INVALID; n_queries == 0 is CDM_OK (nothing is launched); a set with the
 * coordinates -1 record is refused as cdm_pileup_profile refuses it; a listed query with 2^32 records or more is CDM_ERR_UNSUPPORTED
 * (the cells are 32 bits wide; not reachable at test size, not tested).  The pile-up is the set's seeded ungapped overlaps at its
 * identity threshold, not a gapped mapping: reads shorter than 2 * anchor span nothing, and there is no break call where no read
 * seeds - a stretch without reads is reported as a gap, whatever its cause. */
#define CDM_BREAK_JOIN 1u
#define CDM_BREAK_GAP 2u
typedef struct cdm_breaks_params {
    int32_t anchor;            /* 1..1024: columns a spanning read has on either side of a boundary */
    int32_t edge;              /* anchor..1048576: boundaries left out at either end of a query */
    int32_t min_span;          /* 1..1000000 */
    int32_t min_span_percent;  /* 0..100 */
    float   min_seq_id;
    int32_t skip_extended_targets;
} cdm_breaks_params;
typedef struct cdm_break { uint32_t query, first, last, min_span, uncovered, depth_left, depth_right, flags; } cdm_break;   /* 32 bytes */
int  cdm_pileup_breaks(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries,
                       const cdm_breaks_params *par, uint64_t *stats, uint32_t *track, cdm_break **breaks, uint64_t *n_breaks, float *kernel_ms);
void cdm_breaks_free(cdm_break *breaks);

/* ---------------------------------------------------------------------------------------------------------
 * The reads on the queries as alignment records (not a module of the reference; csrc/pileup_map.hip): the pile-up itself, completed
 * with what a SAM line needs and the alignment set does not carry.  A record counts under exactly the rule of the four reductions
 * above.  One cdm_map_rec per counted record of a listed query, from its oriented form (qs, qe, ds, de; reverse when qStart > qEnd):
 *   query    the index into `queries`                      target   the read's index in db
 *   pos      qs, 0-based                                   columns  qe - qs + 1
 *   tstart   the oriented ds: the letters of the read, in the query's orientation, in front of the overlap
 *   tlen     the read's length                             flags    CDM_MAP_REVERSE iff the record is reverse; CDM_MAP_SECONDARY below
 * Letters are the mapped codes and N bits of the DB, never the raw plane.  Column c, 0 <= c < columns, sits on query position pos + c:
 *   ref      the query's code there (A,C,G,T = 0..3), or 4 when its N bit is set
 *   read     the read's code at p = reverse ? tlen - 1 - (tstart + c) : tstart + c, complemented (3 - code) when reverse, or 4 when
 *            the read's N bit is set at p
 *   the column is a mismatch iff ref == 4 || read == 4 || ref != read (the rule of samtools calmd: an N matches nothing)
 *   nm       the number of mismatch columns
 *   mm       the index of the record's first word in `mism`; the record owns nm words there, ascending in c, each
 *            c | ref << 24 | read << 28 (sequences of 4 M letters and more are refused at upload, so c fits 24 bits)
 * Order: listed query order, then ascending pos, then the order the records have in the alignment set (stable).  The mismatch words
 * follow the same order, so mm is the running sum of nm.
 * Primary and secondary: per target, over all its counted records on all listed queries OF THE CALL, the primary is the one with the
 * most columns, among equals the one with the smallest index in the set's record array; every other record of that target carries
 * CDM_MAP_SECONDARY.  Records on queries that are not listed take no part.
 *   stats   n_queries x 4 uint64, per listed query:
 *             0 reads, 1 columns   cdm_pileup_depth's values       2 mismatches  sum of nm       3 primary  records without the
 *             secondary flag
 *   recs    NULL (statistics only), or receives a malloc'ed array of the records; *n_recs = their number; none: *recs = NULL,
 *           *n_recs = 0
 *   mism    NULL only when recs is; receives a malloc'ed array of the mismatch words; *n_mism = their number; none: *mism = NULL.
 *           Both arrays are released with cdm_map_free (either may be NULL).  n_recs and n_mism may be NULL only when recs is.  The
 *           arrays are the caller's only when the call returns CDM_OK
 *   kernel_ms  NULL, or receives the device time of the kernels
 * A NULL argument, a query index >= the DB's size or listed twice is CDM_ERR_INVALID; n_queries == 0 is CDM_OK (nothing is launched);
 * a set with the coordinates -1 record is refused as cdm_pileup_profile refuses it; a listed query with 2^32 records or more is
 * CDM_ERR_UNSUPPORTED (the record slots are 32 bits wide), and so is a set of 2^40 records or more (the primary is found with one
 * 64-bit maximum per target of columns << 40 | (2^40 - 1 - record index)); neither is reachable at test size, neither is tested.
 * The records are the set's seeded ungapped overlaps at its identity threshold: no insertions or deletions here (the seeded pairs that
 * test refused are cdm_pileup_gapped's, below), and no record where no read seeds. */
#define CDM_MAP_REVERSE   1u
#define CDM_MAP_SECONDARY 2u
typedef struct cdm_map_params {
    float   min_seq_id;
    int32_t skip_extended_targets;
} cdm_map_params;
typedef struct cdm_map_rec { uint32_t query, target, pos, columns, tstart, tlen, nm, flags; uint64_t mm; } cdm_map_rec;   /* 40 bytes */
int  cdm_pileup_map(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries,
                    const cdm_map_params *par, uint64_t *stats, cdm_map_rec **recs, uint64_t *n_recs, uint32_t **mism, uint64_t *n_mism,
                    float *kernel_ms);
void cdm_map_free(cdm_map_rec *recs, uint32_t *mism);

/* ---------------------------------------------------------------------------------------------------------
 * Duplicate reads out of an alignment set (not a module of the reference; csrc/pileup_dedup.hip): a second set over the same DB
 * without the PCR copies on the listed queries.  Every reduction above takes a cdm_alns, so the set this call returns reaches each of
 * them unchanged.  The rule is DeDup's for merged reads - both ends and the strand agree - on the records a set holds.  For a listed
 * query q of qLen letters and a record that counts under the rule of the reductions above (min_seq_id, skip_extended_targets), with
 * the oriented form (qs, qe, ds, de; reverse when qStart > qEnd) on a target of tLen letters:
 *   u        = qs - ds, the read's unclipped start on the query, signed: -(tLen - 1) .. qLen - 1; its unclipped end is u + tLen - 1
 *   group    the counted records of q with equal (reverse, u, tLen)
 *   survivor the record of a group with the largest ident, among equals the one with the smallest index in the set's record array;
 *            every other record of the group is removed
 * So clipping at a query's end makes no duplicates (two reads of different lengths that show the same qs..qe differ in u or tLen), a
 * forward and a reverse record on the same coordinates both stay, and two records of one target at one place are a group like any
 * other.  Records that do not count are never removed and displace nothing.  Rows of queries that are not listed are copied whole.
 * The order inside every row is kept; a set without duplicates comes back equal in every byte; the call is idempotent.
 *   out     receives a new set over the same DB, released with cdm_alns_free; `alns` is not touched.  The per-record purine/pyrimidine
 *           counts follow their records (cdm_alns_ry_download on *out: the input's values at the kept records); a set without them
 *           gives a set without them
 *   stats   n_queries x 4 uint64, per listed query: 0 counted, 1 kept (the number of groups), 2 removed, 3 largest (the largest group)
 *   keep    NULL, or one byte per record of `alns` in its order: 1 = the record is in *out, 0 = it was removed
 *   kernel_ms  NULL, or receives the device time of the kernels
 * A NULL argument other than keep and kernel_ms, alns of another size than db, an index-only DB, a query index >= the DB's size or
 * listed twice is CDM_ERR_INVALID; n_queries == 0 is CDM_OK: *out is a copy of the set and nothing is launched; a set with the
 * coordinates -1 record is refused as cdm_pileup_profile refuses it; a listed query with 2^32 records or more is CDM_ERR_UNSUPPORTED
 * (the record slots are 32 bits wide; not reachable at test size, not tested), and so is, with n_queries > 0, a DB whose longest
 * sequence has 2^22 letters or more (the group key holds tLen in 22 bits and u in 23; no upload refuses such a DB, cdm_kmermatch
 * does) - refused before anything is launched, kernel_ms 0.
 * Not covered: the reads cdm_pileup_gapped rescues (they have no record in a set), marking instead of removing, a survivor chosen
 * by base quality (a sequence DB carries none), optical duplicates. */
typedef struct cdm_dedup_params {
    float   min_seq_id;
    int32_t skip_extended_targets;
} cdm_dedup_params;
int  cdm_alns_dedup(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries,
                    const cdm_dedup_params *par, cdm_alns **out, uint64_t *stats, uint8_t *keep, float *kernel_ms);

/* ---------------------------------------------------------------------------------------------------------
 * Contig links from the reads that bridge two query ends (not a module of the reference; csrc/pileup_links.hip): which ends of the
 * listed queries belong together, in which orientation, and how many letters lie between them or by how many they overlap - the
 * edges of the assembly graph, from the pile-up the reductions above count.  All integers.  For the listed query at list index i, of
 * qLen letters, and a record that counts under the rule of the reductions above (min_seq_id, skip_extended_targets), with the
 * oriented form (qs, qe, ds, de; rev when qStart > qEnd) on a target (the read) of tLen letters:
 *   u        = qs - ds, the read's unclipped start on the query (cdm_alns_dedup's u)
 *   L        = max(0, -u), the read letters beyond the query's left end;  R = max(0, u + tLen - qLen), those beyond its right end
 *   cols     = qe - qs + 1
 *   end record  cols >= anchor, and exactly one of L >= overhang (it hangs left) and R >= overhang (it hangs right); h = that L or R.
 *            A record that hangs both ways (a read longer than its query) is counted in both_ends and otherwise ignored
 *   tail / head  in the read's own orientation the record is a TAIL record when (hangs right) != rev, a HEAD record otherwise
 *   o        the query's orientation on the read: + when !rev, - when rev
 * A read's end records are those of all listed queries together (records in rows of queries that are not listed are not read: a read
 * between a listed and an unlisted query makes no link).  A read with more than max_ends end records is CROWDED: it makes no pair.
 * Every other read makes a PAIR from every (tail record on list index x, head record on list index y):
 *   x == y   a self pair: counted in totals[2], nothing else (cyclecheck is the tool for circles)
 *   x != y   the edge (x, oX) -> (y, oY) with gap = hX + hY - tLen: that many read letters between the two queries when positive,
 *            the queries abut at 0, they overlap by -gap letters when negative
 *   canonical form  a < b: with x < y the edge as it stands, and the pair is FORWARD; otherwise (y, flip oY) -> (x, flip oX), the same
 *            gap - the same junction read from the other strand
 * Every pair counts: a read seeded twice on a query counts twice, as everywhere in the pile-up.  A LINK is the set of pairs with equal
 * canonical (a, oA, b, oB):
 *   a, b     indices into `queries`                       info      bit 0: oA is -, bit 1: oB is -
 *   reads    its pairs                                    forward   those that were forward
 *   gap_min, gap_max, gap_sum   minimum, maximum and 64-bit sum of the pairs' gaps
 *   gap_mode the gap with the most pairs, among equals the smallest;  mode_reads  the pairs with that gap;  reserved  0
 *   links   NULL (statistics only; n_links may then be NULL as well), or receives a malloc'ed array (cdm_link_free) of the links with
 *           reads >= min_reads, ascending by (a, oA, b, oB) with + before -; *n_links = their number; none: *links = NULL, *n_links = 0.
 *           The array is the caller's only when the call returns CDM_OK
 *   stats   n_queries x 6 uint64, per listed query:
 *             0 reads, 1 columns   cdm_pileup_depth's values       2 left_ends   end records that hang left
 *             3 right_ends         end records that hang right     4 both_ends   records that hang both ways
 *             5 links              returned links with the query as a or b
 *   totals  5 uint64: 0 end records, 1 crowded reads, 2 self pairs, 3 pairs that entered a link, 4 links before min_reads
 *   kernel_ms  NULL, or receives the device time of the kernels
 * The call is deterministic (integer sums and maxima only), and `alns` is not touched; the set cdm_alns_dedup returns is a set like
 * any other.  anchor and overhang in 1..1024, max_ends in 2..64, min_reads in 1..1000000; anything else, a NULL argument other than
 * links, n_links and kernel_ms, alns of another size than db, an index-only DB, a query index >= the DB's size or listed twice is
 * CDM_ERR_INVALID; n_queries == 0 is CDM_OK (nothing is launched, the totals are 0); a set with the coordinates -1 record is refused
 * as cdm_pileup_profile refuses it.  CDM_ERR_UNSUPPORTED, before anything is launched and with kernel_ms 0: with n_queries > 0 a DB
 * whose longest sequence has 2^22 letters or more (an end record holds h in 22 bits, a pair its gap in 23), and more than 2^24 listed
 * queries (a list index has 24 bits in an end record and in a link's key).  CDM_ERR_UNSUPPORTED once they are counted: a listed query
 * with 2^32 records or more, 2^32 end records or more, 2^32 pairs or more (the places of the two sorts are 32 bits wide); none of
 * the three is reachable at test size, none is tested.
 * Not covered: the reads cdm_pileup_gapped rescues, links of a query with itself, paired-end distance links (the reads are merged).
 * A link is what the reads say: whether the letters of two overlapping ends agree, and the letters between two ends, are
 * cdm_pileup_junctions' (below), and `carpedeam contig_join` joins the queries' letters along the links. */
typedef struct cdm_links_params {
    int32_t anchor;      /* 1..1024: columns a record needs on its contig */
    int32_t overhang;    /* 1..1024: read letters beyond the contig's end */
    int32_t max_ends;    /* 2..64: a read with more end records makes no pair */
    int32_t min_reads;   /* 1..1000000: the links that are returned */
    float   min_seq_id;
    int32_t skip_extended_targets;
} cdm_links_params;
typedef struct cdm_link { uint32_t a, b, info, reads, forward, mode_reads; int32_t gap_mode, gap_min, gap_max, reserved; int64_t gap_sum; } cdm_link;   /* 48 bytes */
int  cdm_pileup_links(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries,
                      const cdm_links_params *par, uint64_t *stats, uint64_t *totals, cdm_link **links, uint64_t *n_links, float *kernel_ms);
void cdm_link_free(cdm_link *links);

/* ---------------------------------------------------------------------------------------------------------
 * What the letters say at a junction (not a module of the reference; csrc/pileup_junctions.hip): the letters of two overlapping query
 * ends compared, or the letters between two ends voted from the reads that bridge them.  A JUNCTION is a canonical link of
 * cdm_pileup_links with ONE gap value: a < b are indices into `queries`, info bit 0: oA is -, bit 1: oB is - (cdm_link's convention).
 * The junctions ascend strictly by (a, oA, b, oB), + before -.  ctx, db, alns, queries, n_queries and par are cdm_pileup_links' own;
 * par->min_reads is ignored.  All integers.  The ORIENTED form of a query is the query for +, its reverse complement for - (the 2-bit
 * code c becomes 3 - c, an N stays N); the link reads: oriented A, then oriented B.  With lenA and lenB the two queries' lengths:
 *   gap < 0   an overlap of k = -gap letters.  k > min(lenA, lenB): the junction is CONTAINED - columns = 0, matches = 0, flags bit 0
 *             (CDM_JUNCTION_CONTAINED).  Otherwise columns = k and matches = the j < k at which oriented A[lenA - k + j] and oriented
 *             B[j] are the same base and neither is N (an N on either side is a mismatch, as in cdm_pileup_map's NM)
 *   gap > 0   a fill of gap letters.  The VOTERS are the pairs of cdm_pileup_links' rule (same end records, same crowded reads, every
 *             pair counts) whose canonical edge is the junction's and whose gap is the junction's.  A pair of a tail record with hX
 *             and a head record with hY of a read of tLen letters has the letters read[tLen - hX .. hY) between the two queries -
 *             gap letters, in the read's own orientation.  A forward pair (x < y) gives them as they stand, a pair that needed the
 *             flip their reverse complement.  Per offset 0 .. gap-1 five 32-bit counts: A, C, G, T, N.  The voted letter is the base
 *             with the largest count, the lowest code among equals; N where no voter has a base there (cdm_pileup_indels' rule for
 *             inserted letters).  The offset's WINNING COUNT is that largest base count (0 where the letter is N)
 *   gap == 0  nothing to compare, nothing to vote
 * res, one cdm_junction_res per junction:
 *   columns, matches   as above (0 unless gap < 0)       flags    bit 0 contained         reserved  0
 *   voters    the pairs of the junction's edge with the junction's gap, whatever its sign: for a junction made of a returned link
 *             with gap = gap_mode it is the link's mode_reads
 *   fill_off, fill_len   the junction's letters in `letters` (fill_len = gap for gap > 0, else 0; fill_off = the sum of the fill_len in front)
 *   fill_min  the smallest winning count over the fill's offsets, 0 without a fill         fill_n   the offsets voted N
 *   letters   receives a malloc'ed array of sum(fill_len) bytes, ASCII ACGTN (NULL where that is 0)
 *   counts    NULL, or receives a malloc'ed array of sum(fill_len) x 5 uint32: A, C, G, T, N per letter (NULL where that is 0)
 *             Both arrays are the caller's only when the call returns CDM_OK, and go back through cdm_junction_free
 *   kernel_ms NULL, or receives the device time of the kernels
 * The call is deterministic (integer sums, minima and maxima only: two calls give byte-equal arrays), and `alns` is not touched.
 * CDM_ERR_INVALID: a NULL argument other than counts and kernel_ms (junctions and res may be NULL with n_junctions == 0, queries with
 * n_queries == 0), anchor, overhang or max_ends out of cdm_pileup_links' ranges, a >= b, b >= n_queries, info > 3, junctions out of
 * order or repeated, and what cdm_pileup_links refuses about db, alns and queries.  CDM_ERR_UNSUPPORTED, before anything is launched
 * and with kernel_ms 0: a DB whose longest sequence has 2^22 letters or more, more than 2^24 listed queries (cdm_pileup_links' two),
 * 2^32 junctions or more, |gap| >= 2^22 (no pair has such a gap), and more than 2^26 fill letters in all - reasoned from the 20 bytes of counters a letter
 * takes, not measured.  CDM_ERR_UNSUPPORTED once they are counted, as in cdm_pileup_links: a listed query with 2^32 records or more, 2^32
 * end records or more (not reachable at test size, not tested).  n_queries == 0 or n_junctions == 0 is CDM_OK: nothing is launched.
 * Not covered: the reads cdm_pileup_gapped rescues, a gapped comparison of the two ends (an overlap with an insertion shows as
 * mismatches), quality-weighted votes. */
#define CDM_JUNCTION_CONTAINED 1u
typedef struct cdm_junction { uint32_t a, b, info; int32_t gap; } cdm_junction;      /* 16 bytes */
typedef struct cdm_junction_res { uint32_t columns, matches, voters, flags; uint64_t fill_off; uint32_t fill_len, fill_min, fill_n, reserved; } cdm_junction_res;   /* 40 bytes */
int  cdm_pileup_junctions(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries,
                          const cdm_links_params *par, const cdm_junction *junctions, uint64_t n_junctions, cdm_junction_res *res,
                          uint8_t **letters, uint32_t **counts, float *kernel_ms);
void cdm_junction_free(uint8_t *letters, uint32_t *counts);

/* ---------------------------------------------------------------------------------------------------------
 * The reads across insertions and deletions (not a module of the reference; csrc/pileup_gapped.hip): a banded affine-gap overlap
 * alignment with traceback on the seeded pairs the ungapped test refused.  `hits` is the prefilter result `alns` was rescored from (or
 * any hit set of the same DB).  A hit (q, t, score, diagonal) of a listed query q is a CANDIDATE when t != q, t is a sequence of the
 * DB, t is not left out by skip_extended_targets, the set holds no counted record of (q, t) - the rule of the reductions above with
 * min_seq_id - and t has at most 4096 letters (a longer t is counted in too_long and not examined).  Every hit is its own candidate.
 * The alignment of a candidate: the query Q runs forward (n letters), the read R (L letters) is in the query's orientation - reverse-
 * complemented when hit.score < 0.  Letters are the mapped codes and N bits, never the raw plane.
 *   diagonals  the hit's diagonal is 16 bits wide; the real diagonals are the ones cdm_rescore probes, u - 65536 d for d = 1 ..
 *              1 + L / 32768, then u + 65536 d for d = 0 .. n / 65536 (u = (uint16) diagonal), those with a non-empty overlap, in that
 *              order.  A forward hit's diagonal D is the query-forward diagonal Df = D, a reverse hit's is Df = n - L - D
 *   band       the cells (i, j), 0 <= i < n, 0 <= j < L, |i - j - Df| <= band
 *   paths      a path starts with a column (Q[i] over R[j]) at a cell with j = 0 or i = 0 and ends with a column at a cell with
 *              j = L - 1 or i = n - 1; the read letters in front of the start and behind the end are soft clips
 *   scores     a column of two equal letters of which neither is N: match; every other column: mismatch; a gap of g letters:
 *              -(gap_open + gap_extend (g - 1))
 *   ties       the end cell is the one with the greatest score, then the smallest i, then the smallest j; walking back from it, the
 *              state a cell was reached from is a column (M) before a query letter without read letter (D) before a read letter without
 *              query letter (I), and inside a gap its extension before its opening; among the real diagonals the greatest score wins,
 *              among equals the first in probe order
 * The candidate is RESCUED when score > 0, columns >= min_columns and matches x 1000 >= min_id_permille x (M columns + inserted +
 * deleted letters), all integers.  One cdm_gap_rec per rescued candidate:
 *   query    the index into `queries`                     target   the read's index in db
 *   pos      the query position of the first column       span     the query letters from pos to the last column (M and D)
 *   tstart   the read letters in front of the first column, in the query's orientation      tlen   L
 *   columns  the read letters in M and I                  score    the path's score
 *   flags    CDM_MAP_REVERSE iff hit.score < 0; CDM_MAP_SECONDARY below
 *   ops      the index of the record's first word in `ops`; n_ops words there, each length << 2 | op with M = 0, I = 1, D = 2;
 *            neighbouring operations are merged, the first and the last are M
 *   words    the index of the record's first word in `words`; n_words words there, ascending in c, the offset on the query from pos:
 *            c | ref << 24 | read << 28 for a mismatch column (ref, read as in cdm_map_rec) and c | ref << 24 | 15 << 28 for a deleted
 *            query letter - an MD string with ^ needs nothing but the words
 *   nm       n_words plus the inserted letters
 * Order: listed query order, then ascending pos, then the hit's index in the set.  Both word arrays follow that order.
 * Primary and secondary: a rescued record can be primary only when its target has no counted (ungapped) record on any listed query of
 * the call; among such a target's rescued records the one with the most columns is primary, among equals the one with the smallest
 * hit index; every other rescued record carries CDM_MAP_SECONDARY.  So beside cdm_pileup_map's records of the same call every read
 * still has exactly one primary record, and none of cdm_pileup_map's changes.
 *   stats   n_queries x 4 uint64, per listed query: 0 candidates, 1 rescued, 2 gap_letters (inserted plus deleted letters of the
 *           rescued records), 3 too_long
 *   recs    NULL (statistics only), or receives a malloc'ed array of the records; ops / words (NULL only when recs is) receive the
 *           two word arrays; all three are released with cdm_gap_free and are the caller's only when the call returns CDM_OK
 * band outside 1..31, min_id_permille above 1000, match <= 0, mismatch >= 0, gap_extend <= 0 or gap_open < gap_extend (the kernel's
 * one-pass row is exact only with open >= extend), or one of the four above 64 in magnitude (a path's score is kept in 21 bits beside
 * its end cell) is CDM_ERR_INVALID, as is a NULL argument, a query index >= the DB's size or listed
 * twice, and hits or alignments of another DB size.  A listed query with 2^32 hits or more, or a hit set of 2^40 or more, is
 * CDM_ERR_UNSUPPORTED; the set with the coordinates -1 record is refused as cdm_pileup_map refuses it.
 * Not covered: reads of more than 4096 letters and a mapping quality.  The depth, variant and break tables take these records through
 * their *_gapped calls, below; cdm_pileup_profile counts ungapped records only. */
typedef struct cdm_gap_params {
    float    min_seq_id;
    int32_t  skip_extended_targets;
    uint32_t band, min_columns, min_id_permille;
    int32_t  match, mismatch, gap_open, gap_extend;     /* mismatch < 0; the gap costs > 0 */
} cdm_gap_params;
typedef struct cdm_gap_rec { uint32_t query, target, pos, span, tstart, tlen, columns, nm, flags, n_ops, n_words; int32_t score;
                             uint64_t ops, words; } cdm_gap_rec;   /* 64 bytes */
int  cdm_pileup_gapped(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_hits *hits, const cdm_alns *alns, const uint32_t *queries,
                       uint64_t n_queries, const cdm_gap_params *par, uint64_t *stats, cdm_gap_rec **recs, uint64_t *n_recs,
                       uint32_t **ops, uint64_t *n_ops, uint32_t **words, uint64_t *n_words, float *kernel_ms);
void cdm_gap_free(cdm_gap_rec *recs, uint32_t *ops, uint32_t *words);

/* ---------------------------------------------------------------------------------------------------------
 * Insertion and deletion sites of the read pile-up (not a module of the reference; csrc/pileup_indels.hip): which insertion and
 * deletion alleles the rescued reads put on which position of the listed queries, how many reads cross that place at all, which
 * alleles are supported, and the letters the majority wants inserted.  `alns` is the ungapped set, counted by exactly the rule of the
 * reductions above; recs / ops are the host arrays cdm_pileup_gapped returned for the same `queries` (the words are not needed).  Every
 * record given counts, primary or secondary, as every ungapped record counts on every query it lies on.  All figures are integers.
 * Boundary b of a query of `len` letters, 1 <= b <= len - 1, lies between the positions b - 1 and b, as in cdm_pileup_breaks.
 *   cross[b]  the counted ungapped records with qs < b <= qe plus the given gapped records with pos < b <= pos + span - 1; cross[0] = 0
 *   event     one I or D operation of a gapped record, found by walking its operations from pos and tstart: a D of g letters whose
 *             first deleted query letter is p gives (p, D, g); an I of g letters in front of query position p gives (p, I, g) and
 *             carries the read offset of its first letter, in the query's orientation.  The operations begin and end with M, so
 *             pos < p <= pos + span - 1, and an allele's count never exceeds cross[p]
 *   allele    the events of one (query, p, kind, g); count = their number
 *   place     one (query, p, kind).  Its best allele has the largest count, among equals the smallest g; others = the place's events
 *             in its other alleles.  Flags of the best allele:
 *               CDM_INDEL_CALLED     cross[p] >= min_depth
 *               CDM_INDEL_SUPPORTED  called, count >= min_count and count * 100 >= min_percent * cross[p] (64 bits)
 *               CDM_INDEL_MAJOR      supported and 2 * count > cross[p]
 *   letters   of a best I allele, for every offset k < g: the base counts over the allele's events of the read letter at that offset
 *             (the mapped code, complemented when the record is reverse; a letter with its N bit set is left out); the largest count
 *             wins, among equals the lowest code; 4 (N) where every event had an N.  A D allele has no letters: the host has the query
 *   stats   n_queries x 10 uint64, per listed query:
 *             0 reads, 1 columns   cdm_pileup_depth's values       2 rescued   the gapped records given
 *             3 insertions, 4 deletions   events of each kind      5 inserted_letters, 6 deleted_letters
 *             7 places             8 supported   the query's site records      9 major
 *   track   NULL, or uint32 [sum of the listed queries' lengths]: per listed query cross[b] for b = 0 .. len - 1, the queries back
 *           to back in listed order
 *   sites   NULL, or receives a malloc'ed array of one record per SUPPORTED place in listed query order, then ascending pos, then I
 *           before D: query = the index into `queries`, pos = p, info = kind | g << 4 | flags << 16 (kind CDM_INDEL_INS or
 *           CDM_INDEL_DEL), count, cross = cross[p], others, n_letters = g for an I and 0 for a D, letters = the index of the record's
 *           first letter in `letters`.  *letters receives a malloc'ed array of the codes 0..4, *n_letters their number.  Both arrays
 *           are released with cdm_indel_free (either may be NULL) and are the caller's only when the call returns CDM_OK.  n_sites,
 *           letters and n_letters may be NULL only when sites is
 *   kernel_ms  NULL, or receives the device time of the kernels
 * The records are caller data and are checked on the host, in one pass, before anything is sent to the device: query < n_queries;
 * target < the DB's size and tlen == the target's length; records ascending by (query, pos); ops + n_ops within the pool and
 * n_ops >= 1; every operation M, I or D with a length >= 1; the first and the last M; no two neighbours of one code; M + D = span and
 * M + I = columns; pos + span <= the query's length and tstart + columns <= tlen; no I or D of more than 62 letters (twice the largest
 * band, the longest gap a banded path can hold).  The first record that fails is named and the call returns CDM_ERR_INVALID, as for
 * min_depth or min_count outside 1..1000000, min_percent outside 0..100, a NULL argument, a query index >= the DB's size or listed
 * twice.  n_queries == 0 is CDM_OK (nothing is launched); n_recs == 0 is valid (cross from the ungapped records, no sites); a set with
 * the coordinates -1 record is refused as cdm_pileup_profile refuses it; a listed query with 2^32 records or more, or 2^31 operation
 * words or more, is CDM_ERR_UNSUPPORTED (neither is reachable at test size, neither is tested).
 * Not covered: substitutions (cdm_pileup_bases), and a read seeded twice on one query counts twice, as it has two records. */
#define CDM_INDEL_INS 1u
#define CDM_INDEL_DEL 2u
#define CDM_INDEL_CALLED 1u
#define CDM_INDEL_SUPPORTED 2u
#define CDM_INDEL_MAJOR 4u
typedef struct cdm_indel_params {
    int32_t min_depth;        /* 1..1000000 */
    int32_t min_count;        /* 1..1000000 */
    int32_t min_percent;      /* 0..100 */
    float   min_seq_id;
    int32_t skip_extended_targets;
} cdm_indel_params;
typedef struct cdm_indel_site { uint32_t query, pos, info, count, cross, others, n_letters, reserved; uint64_t letters; } cdm_indel_site;   /* 40 bytes */
int  cdm_pileup_indels(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries,
                       const cdm_gap_rec *recs, uint64_t n_recs, const uint32_t *ops, uint64_t n_ops, const cdm_indel_params *par,
                       uint64_t *stats, uint32_t *track, cdm_indel_site **sites, uint64_t *n_sites, uint8_t **letters, uint64_t *n_letters,
                       float *kernel_ms);
void cdm_indel_free(cdm_indel_site *sites, uint8_t *letters);

/* ---------------------------------------------------------------------------------------------------------
 * The rescued reads in the depth, variant and break tables (not modules of the reference; csrc/pileup_depth.hip, csrc/pileup_bases.hip):
 * cdm_pileup_depth, cdm_pileup_bases and cdm_pileup_breaks over the ungapped set PLUS gapped records.  recs / ops are the host arrays
 * cdm_pileup_gapped returned for the same `queries`, exactly as cdm_pileup_indels takes them.  The parameter structs, result layouts,
 * record types, free functions and flag meanings are those of the three calls above; every ungapped record counts exactly as there,
 * and every gapped record given counts as well, primary or secondary (a read counts on every query it lies on).
 * A record's operations are walked from p = pos and o = tstart: M of g letters gives the columns j < g, column j on query position
 * p + j with the read's oriented offset o + j, then both advance; I advances o; D advances p.  With C the number of M columns,
 * m_1 < .. < m_C their query positions, and r = reverse ? tlen - 1 - offset : offset the position in the read's own orientation:
 *   depth     depth[i] += 1 for every M column on position i.  A deleted query letter gets no depth from the read (it has no base
 *             there; the default of samtools depth), so depth[i] >= the sum of position i's eight counters still holds
 *   reads     stats 0 of all three: the ungapped value plus one per gapped record of the query
 *   columns   stats 1 of all three: the ungapped value plus C per record - still the sum of depth over the query
 *   span      a gapped record with C >= 2 w, w = anchor, spans the boundaries m_w + 1 <= b <= m_(C - w + 1): at least w M columns
 *             strictly left of b and at least w at or right of it; for a record of one M operation this is qs + w <= b <= qe + 1 - w.
 *             Weak boundaries, runs, uncovered, depth_left, depth_right and the flags come from the summed depth and span exactly as
 *             in cdm_pileup_breaks: a deleted stretch that reads span has depth 0 and a positive span, is not weak and gives no break
 *   bases     an M column on position i is left out when the read's N bit is set at r, and - with mask_ends = m > 0 - when r < m or
 *             tlen - 1 - r < m; otherwise counts[i][rev * 4 + b] += 1 with b the read's mapped code at r, complemented when reverse.
 *             Inserted letters have no query position and count nowhere.  Classification, stats 2..7 and the sites are unchanged
 *   kernel_ms NULL, or receives the device time of the kernels, those over the gapped records included (0 behind a refusal)
 * The records are caller data and get cdm_pileup_indels' one-pass host check before anything goes to the device: the first record that
 * fails is named and the call returns CDM_ERR_INVALID.  With n_recs == 0 each call returns what its ungapped counterpart returns,
 * array for array; n_queries == 0 is CDM_OK (nothing is launched).  A listed query whose ungapped plus gapped records reach 2^32, or
 * 2^31 operation words or more, is CDM_ERR_UNSUPPORTED (the cells are 32 bits wide; not reachable at test size, not tested).
 * Not covered: cdm_pileup_profile (the damage table is a rate, and the rescued reads are a small share of it), and a mapping quality. */
int  cdm_pileup_depth_gapped(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries,
                             const cdm_gap_rec *recs, uint64_t n_recs, const uint32_t *ops, uint64_t n_ops, const cdm_depth_params *par,
                             uint64_t *stats, uint32_t *depth, float *kernel_ms);
int  cdm_pileup_bases_gapped(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries,
                             const cdm_gap_rec *recs, uint64_t n_recs, const uint32_t *ops, uint64_t n_ops, const cdm_bases_params *par,
                             uint64_t *stats, uint32_t *counts, cdm_site **sites, uint64_t *n_sites, float *kernel_ms);
int  cdm_pileup_breaks_gapped(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const uint32_t *queries, uint64_t n_queries,
                              const cdm_gap_rec *recs, uint64_t n_recs, const uint32_t *ops, uint64_t n_ops, const cdm_breaks_params *par,
                              uint64_t *stats, uint32_t *track, cdm_break **breaks, uint64_t *n_breaks, float *kernel_ms);

/* ---------------------------------------------------------------------------------------------------------
 * ancient_read_assemble.  Replaces the loops at src/assembler/ancientReadsResults.cpp:178-581.
 * db must be the corrected DB.  Output: new sequence DB (extended sequences get ext=1, others are copied through).
 * scores (optional, may be NULL): for tests, the per-candidate likelihood of the first scoring round
 * (calcLikelihoodConsensus, nuclassembleUtil.cpp:203-374): one double sLenNorm per alignment record, NaN where the
 * record is not a candidate.
 */
int cdm_extend(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const cdm_ancient_params *par, cdm_seqdb **out,
               double *scores);

/* ---------------------------------------------------------------------------------------------------------
 * ancient_contig_merge (contig phase of the workflow, data/nuclassemble.sh:148-196).  Replaces the loop at
 * src/assembler/ancientContigsResults.cpp:94-509.  db must be the corrected contig DB.  The per-alignment column work
 * (orientation, identities, the counts of updateSeqIdConsensus / ancientMatchCount) runs on the device, and since round 5 so do the
 * queue - a Beta-posterior comparator built on the C library's lgammaf / logf (:25-70), not a strict weak ordering: the device reads
 * those two functions from tables of the library's own values and replays libstdc++'s heap step for step (csrc/contigqueue.hip) -
 * and the extension loop (:276-470), in both modes: par->unsafe = 1 counts its columns against the majority-vote consensus of the
 * extending candidates on the device as well (csrc/contigunsafe.hip).  The library's host code (the same libstdc++ priority queue as
 * the reference) runs for small calls in a process that has not filled the tables yet and for the rare query the device hands back
 * (CDM_CONTIG_QUEUE=host|device pins either).  Same result either way.
 * merge_seq_id_thr is --min-merge-seq-id; par->ry_seq_id_thr, max_seq_len, unsafe, min_cov_safe are used from par.
 */
int cdm_contig_merge(cdm_ctx *ctx, const cdm_seqdb *db, const cdm_alns *alns, const cdm_ancient_params *par, float merge_seq_id_thr,
                     cdm_seqdb **out);

/* ---------------------------------------------------------------------------------------------------------
 * cyclecheck (data/nuclassemble.sh:19-60, after every contig iteration).  Replaces the loop at src/assembler/cyclecheck.cpp:75-258
 * (k = 22 as setCycleCheckDefaults fixes it): *cyclic receives the contigs the module writes - cut at the split diagonal when
 * chop_cycle (--chop-cycle) is set, whole otherwise, wasExtended 0 - and, if rest is not NULL, *rest the others (what the workflow's
 * "_noneCycle" index selects), both in the order of db.  Contigs of max_seq_len (--max-seq-len) letters or more are never cyclic
 * (:107-112).  split (host, db size entries, may be NULL) receives the split diagonal of every contig, 0 = not cyclic.
 */
int cdm_cyclecheck(cdm_ctx *ctx, const cdm_seqdb *db, uint32_t max_seq_len, int chop_cycle, cdm_seqdb **cyclic, cdm_seqdb **rest, uint32_t *split);

/* ---------------------------------------------------------------------------------------------------------
 * Multi-GPU inside the library: one rank per device (one process per GPU, or one host thread per GPU of one process), RCCL over
 * xGMI called directly (csrc/dist.hip).  The reference shards inside its modules - kmermatcher by k-mer range
 * (lib/mmseqs/src/linclust/kmermatcher.cpp:634-663, merged :742-784), rescorediagonal by query range
 * (lib/mmseqs/src/alignment/rescorediagonal.cpp:399-421) - and so do these calls: every rank holds the whole sequence DB, the result is
 * bit-identical to the single-device calls (kmermatcher's first half: every rank extracts its block of the sequences, all-to-alls
 * carry the k-mer tuples to the rank of their k-mer range - cdm_kmermatch_split_* -; ONE all-to-all of the group keys to the owners of
 * their representatives; the owned ranges of the stages' result DBs all-gathered).
 *   cdm_comm_unique_id       rank 0: the 128 bytes of ncclGetUniqueId, to be handed to every rank by whatever launched them
 *   cdm_comm_create_rccl     a rank's communicator (ncclCommInitRank on the context's device; librccl is loaded on first use)
 *   cdm_comm_create_ops      the same over collectives the caller supplies (tests: W ranks on one device; another collective library)
 *   cdm_kmermatch_dist       kmermatcher over the ranks: the hits of the representatives this rank OWNS, self hits for all others; the
 *                            union is cdm_kmermatch's result.  Owned = a range of sequence ids per rank, cut by this call so that every
 *                            rank owns about the same number of group keys (representatives are the longest, then lowest ids: equal id
 *                            ranges gave the first of 8 ranks 88 % of them at 50 M reads); cdm_comm_owned reports the ranges
 *   cdm_comm_owned           bounds[world + 1]: rank r owns the sequences [bounds[r], bounds[r + 1]) of a DB of n sequences - as the
 *                            communicator's last cdm_kmermatch_dist on such a DB cut them, equal ranges before any; CDM_ERR_INVALID for a
 *                            DB of another size than the one the ranges were cut for
 * A failure on one rank (out of memory for an exchange buffer, a refusal that depends on the rank's data) is agreed on before the next
 * collective is entered: every rank returns an error from the same call, none is left waiting in RCCL.
 *   cdm_seqdb_allgather_owned   the owned ranges (cdm_comm_owned) of the ranks' DBs (same number of sequences on every rank) -> the complete DB
 *   cdm_reads_iteration_dist    one iteration of the reads loop (data/nuclassemble.sh:100-146) over the ranks; hits / alns hold the
 *                            owned queries' records, corr / next are complete on every rank and equal the single-device DBs
 *   cdm_contig_iteration_dist   one iteration of the contig loop (data/nuclassemble.sh:148-196) over the ranks, up to ancient_contig_merge:
 *                            the reference's loop over independent queries (ancientContigsResults.cpp:94-509) sharded by owned queries like
 *                            the other stages; corr / next complete on every rank; the script's cyclecheck step is the caller's
 */
typedef struct cdm_comm cdm_comm;
typedef struct cdm_comm_ops {
    void *user;
    /* host buffers: recv[p * bytes ..] = rank p's send (bytes each) */
    int (*all_gather_host)(void *user, const void *send, void *recv, uint64_t bytes);
    /* device buffers, byte offsets [world + 1]: peer p gets send[send_off[p], send_off[p + 1]) and fills recv[recv_off[p], recv_off[p + 1]);
     * enqueued on `stream` (a hipStream_t) or complete on return */
    int (*all_to_all_dev)(void *user, const void *send, const uint64_t *send_off, void *recv, const uint64_t *recv_off, void *stream);
    /* device buffers: recv[recv_off[p], recv_off[p + 1]) = rank p's send (send_bytes of them differ between the ranks) */
    int (*all_gather_dev)(void *user, const void *send, uint64_t send_bytes, void *recv, const uint64_t *recv_off, void *stream);
} cdm_comm_ops;
int cdm_comm_unique_id(void *id128);
int cdm_comm_create_rccl(cdm_ctx *ctx, int rank, int world, const void *id128, cdm_comm **out);
int cdm_comm_create_ops(cdm_ctx *ctx, int rank, int world, const cdm_comm_ops *ops, cdm_comm **out);
/* tests: the RCCL transport's own code (its buffers, its pieces of 256 MB, its offsets) over a stand-in for RCCL's send / recv /
 * all-gather inside ONE process - the ranks are host threads that share a device, which RCCL itself refuses.  group: from
 * cdm_comm_standin_group(world), shared by the world's ranks. */
void *cdm_comm_standin_group(int world);
int cdm_comm_create_standin(cdm_ctx *ctx, void *group, int rank, cdm_comm **out);
void cdm_comm_free(cdm_comm *c);
int cdm_comm_rank(const cdm_comm *c);
int cdm_comm_world(const cdm_comm *c);
int cdm_comm_owned(const cdm_comm *c, uint64_t n, uint64_t *bounds);
/* what the communicator's last cdm_kmermatch_dist did: 0 nothing yet, 1 every rank ran kmermatcher whole (two ranks; a DB that takes the wide
 * group key), 2 every rank extracted all reads and kept its range of the k-mer space, 3 the reads were split and the k-mer tuples travelled,
 * 4 equal slices of the k-mer space by value (cdm_kmermatch_part), 5 the first half by ranges of the k-mer space, the kept group keys (wide form
 * included) all-gathered, sort 2 and the vote on every rank (DBs that take the wide group key) */
int cdm_comm_last_path(const cdm_comm *c);
int cdm_kmermatch_dist(cdm_ctx *ctx, cdm_comm *comm, const cdm_seqdb *db, const cdm_kmer_params *par, cdm_hits **out);
int cdm_seqdb_allgather_owned(cdm_ctx *ctx, cdm_comm *comm, const cdm_seqdb *local, cdm_seqdb **out);
int cdm_reads_iteration_dist(cdm_ctx *ctx, cdm_comm *comm, const cdm_seqdb *db, const cdm_kmer_params *kpar, const cdm_rescore_params *rpar,
                             const cdm_ancient_params *apar, cdm_hits **hits, cdm_alns **alns, cdm_seqdb **corr, cdm_seqdb **next);
int cdm_contig_iteration_dist(cdm_ctx *ctx, cdm_comm *comm, const cdm_seqdb *db, const cdm_kmer_params *kpar, const cdm_rescore_params *rpar,
                              const cdm_ancient_params *apar, float merge_seq_id_thr, cdm_alns **alns, cdm_seqdb **corr, cdm_seqdb **next);

/* ---------------------------------------------------------------------------------------------------------
 * Paired-end merging: the module mergereads (src/assembler/mergereads.cpp) - FLASH's combine_reads with the parameters fixed at
 * mergereads.cpp:20-24 (min overlap 15, max overlap 65, max mismatch density 0.10f, no outies, no capped mismatch qualities) - for
 * one batch of pairs.  csrc/pairmerge.hip.
 *
 * Input, pair i: R1 = seq1[off1[i] .. + len1[i]) with its qualities at the same offsets in qual1, R2 likewise in seq2 / qual2, AS READ:
 * the device reverse-complements R2 with FLASH's table (lib/flash/read.cpp:4-13: IUPAC codes and lower case to their complements,
 * U -> A, every other byte to '.') and reverses its qualities.  Lengths must be >= 1 (mergereads: "Invalid sequence record found").
 *
 * pair_align (lib/flash/combine_reads.cpp:266-334): shifts i = max(0, L1 - L2) .. L1 - min_overlap; the overlap length is L1 - i minus
 * the positions where either base is 'N' (upper case only); a shift counts when that length is >= min_overlap; with
 * score_len = (float) min(length, max_overlap), density = mismatches / score_len and qual = sum of min(q1, q2) over the mismatches /
 * score_len, both in float, mismatches comparing raw bytes, qualities the raw ASCII bytes (Phred+33 not subtracted).  The shift with the
 * smallest (density, qual), the first one on ties, is taken when its density is <= max_mismatch_density.
 * generate_combined_read (:338-446): R1's prefix, the overlap (equal bases kept, else the base of the higher quality - signed char -,
 * on equal qualities R2's unless it is 'N'), R2's tail.  Qualities of the combined read are not produced (mergereads writes none).
 *
 * Output, in mergereads' entry order (mergereads.cpp:77-114): a combined pair gives one entry (the consensus), any other pair two
 * (R1 as read, then the reverse-complemented R2); entry text "SEQ\n\0", back to back.
 *
 * Quality bytes >= 0x80 are refused (CDM_ERR_UNSUPPORTED): the reference's SSE path takes their minimum unsigned and its scalar path
 * signed (combine_reads.cpp:120-245), so no single answer exists for them; valid FASTQ never has them.
 */
typedef struct cdm_pairs cdm_pairs;   /* one merged batch, resident in HBM */
typedef struct cdm_merge_params {
    int min_overlap;              /* 15 */
    int max_overlap;              /* 65 */
    float max_mismatch_density;   /* 0.10f */
} cdm_merge_params;
/* par may be NULL: mergereads' values.  min_overlap, max_overlap >= 1 and 0 <= max_mismatch_density <= 1e6 (NaN and inf are
 * CDM_ERR_INVALID) */
int cdm_pairs_merge(cdm_ctx *ctx, const char *seq1, const char *qual1, const uint64_t *off1, const uint32_t *len1,
                    const char *seq2, const char *qual2, const uint64_t *off2, const uint32_t *len2, uint64_t n,
                    const cdm_merge_params *par, cdm_pairs **out);
uint64_t cdm_pairs_count(const cdm_pairs *h);     /* pairs */
uint64_t cdm_pairs_entries(const cdm_pairs *h);   /* output entries: pairs + pairs not combined */
uint64_t cdm_pairs_bytes(const cdm_pairs *h);     /* bytes of the entries' text */
float cdm_pairs_kernel_ms(const cdm_pairs *h);    /* device time of the merge (kernels and scans), ms */
/* any argument may be NULL.  status[n]: 1 combined, 0 not; merged_len[n]: the consensus length (0: not combined);
 * text[bytes]: the entries' text; entry_len[entries]: sequence length of each entry (without "\n\0") */
int cdm_pairs_download(cdm_ctx *ctx, const cdm_pairs *h, uint8_t *status, uint32_t *merged_len, char *text, uint32_t *entry_len);
/* the text in pieces of piece_bytes through pinned staging buffers, as cdm_seqdb_download_stream */
int cdm_pairs_download_stream(cdm_ctx *ctx, const cdm_pairs *h, uint64_t piece_bytes,
                              int (*sink)(void *user, const char *data, uint64_t offset, uint64_t bytes), void *user);
/* the entries as a resident sequence DB - no host round trip.  Keys first_key, first_key + 1, ...; wasExtended 1 on every entry, as
 * mergereads writes its DB (DBWriter::writeEnd(id, 0, true), mergereads.cpp:82-110; DBWriter.h:30) */
int cdm_pairs_to_seqdb(cdm_ctx *ctx, const cdm_pairs *h, uint32_t first_key, cdm_seqdb **out);
void cdm_pairs_free(cdm_pairs *h);

#ifdef __cplusplus
}
#endif
#endif
