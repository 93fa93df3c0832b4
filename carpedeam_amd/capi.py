"""ctypes binding of the C ABI (include/carpedeam_hip.h) -- used by tests and bench.py.

There is no CPU fallback: importing works anywhere (so that `-m "not gpu"` tests can check that the library loads and
exports its symbols), but every compute entry point needs a gfx950 device and raises CdmError otherwise.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CDM_LIB", os.path.join(HERE, "libcarpedeam_hip.so"))      # CDM_LIB: another build of the library (bisecting)

HIT_DTYPE = np.dtype([("target", "<u4"), ("score", "<i4"), ("diagonal", "<i4")])
ALN_DTYPE = np.dtype([("target", "<u4"), ("raw_score", "<i4"), ("ident", "<i4"), ("q_start", "<i4"), ("q_end", "<i4"),
                      ("db_start", "<i4"), ("db_end", "<i4"), ("seq_id", "<f4")])


class KmerParams(C.Structure):
    _fields_ = [("kmer_size", C.c_int32), ("kmers_per_seq", C.c_int32), ("kmers_per_seq_scale", C.c_float), ("hash_shift", C.c_uint64),
                ("ignore_multi_kmer", C.c_int32), ("include_only_extendable", C.c_int32), ("cov_mode", C.c_int32), ("cov_thr", C.c_float)]

    @classmethod
    def reads_default(cls):
        return cls(20, 200, 0.2, 67, 1, 0, 1, 0.0)


class RescoreParams(C.Structure):
    _fields_ = [("seq_id_thr", C.c_float), ("eval_thr", C.c_double), ("cov_mode", C.c_int32), ("cov_thr", C.c_float),
                ("seq_id_mode", C.c_int32), ("min_aln_len", C.c_int32)]

    @classmethod
    def default(cls):
        return cls(0.9, 0.001, 1, 0.0, 0, 0)


class HammingParams(C.Structure):
    _fields_ = [("seq_id_thr", C.c_float), ("eval_thr", C.c_double), ("cov_mode", C.c_int32), ("cov_thr", C.c_float),
                ("seq_id_mode", C.c_int32), ("min_aln_len", C.c_int32), ("reverse_prefilter", C.c_int32)]

    @classmethod
    def linclust(cls):
        """what `ancient_assemble` passes to linclust's pre-clustering (GuidedNuclassembler.cpp:176-181, Linclust.cpp:103-112)"""
        return cls(0.97, 0.001, 1, 0.99, 0, 0, 1)


class AlignParams(C.Structure):
    """cdm_align_params: gap costs, z-drop and band of linclust's `align` as `ancient_assemble` runs it"""
    _fields_ = [("gap_open", C.c_int32), ("gap_extend", C.c_int32), ("zdrop", C.c_int32), ("band", C.c_int32)]

    @classmethod
    def linclust(cls):
        return cls(5, 2, 200, 64)


class AlignHit(C.Structure):
    """cdm_align_hit: one seeded hit of the gapped step (sequence indices, strand, cut lengths, the seed's ends, the stale letters)"""
    _fields_ = [("query", C.c_uint32), ("target", C.c_uint32), ("q_len", C.c_uint32), ("t_len", C.c_uint32), ("q_end", C.c_int32), ("t_end", C.c_int32),
                ("reverse", C.c_uint8), ("wrapped", C.c_uint8), ("stale_q", C.c_uint8), ("stale_t", C.c_uint8)]


ALIGN_HIT_DTYPE = np.dtype([("query", "<u4"), ("target", "<u4"), ("q_len", "<u4"), ("t_len", "<u4"), ("q_end", "<i4"), ("t_end", "<i4"),
                            ("reverse", "u1"), ("wrapped", "u1"), ("stale_q", "u1"), ("stale_t", "u1")])
ALIGN_RESULT_DTYPE = np.dtype([("score", "<i4"), ("q_start", "<i4"), ("q_end", "<i4"), ("t_start", "<i4"), ("t_end", "<i4"), ("identities", "<i4"),
                               ("columns", "<i4"), ("rows", "<i4")])


class AncientParams(C.Structure):
    _fields_ = [("seq_id_thr", C.c_float), ("corr_reads_ry_seq_id", C.c_float), ("ry_seq_id_thr", C.c_float), ("rand_align_penal", C.c_float),
                ("excess_penal", C.c_float), ("likelihood_threshold", C.c_float), ("unsafe", C.c_int32), ("min_cov_safe", C.c_int32),
                ("max_seq_len", C.c_uint64)]

    @classmethod
    def default(cls):
        return cls(0.9, 0.99, 0.99, 0.85, 0.0625, 0.5, 0, 5, 200000)


class PileupParams(C.Structure):
    """cdm_pileup_params: positions counted from either end of a read, the records' identity threshold, reads only as targets"""
    _fields_ = [("ends", C.c_int32), ("min_seq_id", C.c_float), ("skip_extended_targets", C.c_int32)]


class DepthParams(C.Structure):
    """cdm_depth_params: positions left out of the statistics window at either end of a contig, the records' identity threshold, reads
    only as targets"""
    _fields_ = [("edge", C.c_int32), ("min_seq_id", C.c_float), ("skip_extended_targets", C.c_int32)]


class BasesParams(C.Structure):
    """cdm_bases_params: read positions left out at either end of a read, the three thresholds of the site flags, the records' identity
    threshold, reads only as targets"""
    _fields_ = [("mask_ends", C.c_int32), ("min_depth", C.c_int32), ("min_alt_count", C.c_int32), ("min_alt_percent", C.c_int32),
                ("min_seq_id", C.c_float), ("skip_extended_targets", C.c_int32)]


class Site(C.Structure):
    """cdm_site: one flagged position"""
    _fields_ = [("query", C.c_uint32), ("pos", C.c_uint32), ("info", C.c_uint32), ("counts", C.c_uint32 * 8)]


SITE_DTYPE = np.dtype([("query", "<u4"), ("pos", "<u4"), ("info", "<u4"), ("counts", "<u4", (8,))])
SITE_CALLED, SITE_DIFFERS, SITE_VARIABLE = 1, 2, 4


class BreaksParams(C.Structure):
    """cdm_breaks_params: columns a spanning read has on either side of a boundary, boundaries left out at either end of a query, the two
    thresholds of a weak boundary, the records' identity threshold, reads only as targets"""
    _fields_ = [("anchor", C.c_int32), ("edge", C.c_int32), ("min_span", C.c_int32), ("min_span_percent", C.c_int32),
                ("min_seq_id", C.c_float), ("skip_extended_targets", C.c_int32)]


class Break(C.Structure):
    """cdm_break: one run of weak boundaries"""
    _fields_ = [(n, C.c_uint32) for n in ("query", "first", "last", "min_span", "uncovered", "depth_left", "depth_right", "flags")]


BREAK_DTYPE = np.dtype([(n, "<u4") for n in ("query", "first", "last", "min_span", "uncovered", "depth_left", "depth_right", "flags")])
BREAK_JOIN, BREAK_GAP = 1, 2


class MapParams(C.Structure):
    """cdm_map_params: the records' identity threshold, reads only as targets"""
    _fields_ = [("min_seq_id", C.c_float), ("skip_extended_targets", C.c_int32)]


class MapRec(C.Structure):
    """cdm_map_rec: one read on one query"""
    _fields_ = [(n, C.c_uint32) for n in ("query", "target", "pos", "columns", "tstart", "tlen", "nm", "flags")] + [("mm", C.c_uint64)]


MAP_DTYPE = np.dtype([(n, "<u4") for n in ("query", "target", "pos", "columns", "tstart", "tlen", "nm", "flags")] + [("mm", "<u8")])
MAP_REVERSE, MAP_SECONDARY = 1, 2


class DedupParams(C.Structure):
    """cdm_dedup_params: the records' identity threshold, reads only as targets"""
    _fields_ = [("min_seq_id", C.c_float), ("skip_extended_targets", C.c_int32)]


class LinksParams(C.Structure):
    """cdm_links_params: columns an end record has on its query, read letters beyond the query's end, the most end records of a read that
    makes pairs, the pairs of a returned link, the records' identity threshold, reads only as targets"""
    _fields_ = [("anchor", C.c_int32), ("overhang", C.c_int32), ("max_ends", C.c_int32), ("min_reads", C.c_int32), ("min_seq_id", C.c_float),
                ("skip_extended_targets", C.c_int32)]

    @classmethod
    def default(cls, anchor=16, overhang=1, max_ends=16, min_reads=2, min_seq_id=0.0, skip_extended_targets=False):
        """the values `carpedeam contig_links` passes without flags (it passes skip_extended_targets = 1)"""
        return cls(int(anchor), int(overhang), int(max_ends), int(min_reads), float(min_seq_id), int(bool(skip_extended_targets)))


class Link(C.Structure):
    """cdm_link: the pairs of one canonical edge (a, oA) -> (b, oB)"""
    _fields_ = [(n, C.c_uint32) for n in ("a", "b", "info", "reads", "forward", "mode_reads")] + [(n, C.c_int32) for n in ("gap_mode", "gap_min", "gap_max", "reserved")] + [
        ("gap_sum", C.c_int64)]


LINK_DTYPE = np.dtype([(n, "<u4") for n in ("a", "b", "info", "reads", "forward", "mode_reads")] + [(n, "<i4") for n in ("gap_mode", "gap_min", "gap_max", "reserved")] + [
    ("gap_sum", "<i8")])
LINK_A_MINUS, LINK_B_MINUS = 1, 2


class Junction(C.Structure):
    """cdm_junction: a canonical link (a, oA) -> (b, oB) with one gap value"""
    _fields_ = [(n, C.c_uint32) for n in ("a", "b", "info")] + [("gap", C.c_int32)]


class JunctionRes(C.Structure):
    """cdm_junction_res: what the letters say at a junction"""
    _fields_ = [(n, C.c_uint32) for n in ("columns", "matches", "voters", "flags")] + [("fill_off", C.c_uint64)] + [(n, C.c_uint32) for n in ("fill_len", "fill_min", "fill_n", "reserved")]


JUNCTION_DTYPE = np.dtype([(n, "<u4") for n in ("a", "b", "info")] + [("gap", "<i4")])
JUNCTION_RES_DTYPE = np.dtype([(n, "<u4") for n in ("columns", "matches", "voters", "flags")] + [("fill_off", "<u8")] + [(n, "<u4") for n in ("fill_len", "fill_min", "fill_n", "reserved")])
JUNCTION_CONTAINED = 1


class GapParams(C.Structure):
    """cdm_gap_params: the records' identity threshold, reads only as targets, the band, the two thresholds of a rescue, the scores"""
    _fields_ = [("min_seq_id", C.c_float), ("skip_extended_targets", C.c_int32), ("band", C.c_uint32), ("min_columns", C.c_uint32), ("min_id_permille", C.c_uint32),
                ("match", C.c_int32), ("mismatch", C.c_int32), ("gap_open", C.c_int32), ("gap_extend", C.c_int32)]

    @classmethod
    def default(cls, min_seq_id=0.0, skip_extended_targets=False, band=8, min_columns=32, min_id_permille=900, match=2, mismatch=-3, gap_open=5, gap_extend=2):
        """the values `carpedeam contig_map --gapped 1` passes: nucleotide.out's scores, the gap costs of `align`"""
        return cls(float(min_seq_id), int(bool(skip_extended_targets)), band, min_columns, min_id_permille, match, mismatch, gap_open, gap_extend)


class GapRec(C.Structure):
    """cdm_gap_rec: one rescued read on one query"""
    _fields_ = [(n, C.c_uint32) for n in ("query", "target", "pos", "span", "tstart", "tlen", "columns", "nm", "flags", "n_ops", "n_words")] + [
        ("score", C.c_int32), ("ops", C.c_uint64), ("words", C.c_uint64)]


GAP_DTYPE = np.dtype([(n, "<u4") for n in ("query", "target", "pos", "span", "tstart", "tlen", "columns", "nm", "flags", "n_ops", "n_words")] + [
    ("score", "<i4"), ("ops", "<u8"), ("words", "<u8")])
GAP_OP_M, GAP_OP_I, GAP_OP_D = 0, 1, 2


class IndelParams(C.Structure):
    """cdm_indel_params: the three thresholds of the site flags, the records' identity threshold, reads only as targets"""
    _fields_ = [("min_depth", C.c_int32), ("min_count", C.c_int32), ("min_percent", C.c_int32), ("min_seq_id", C.c_float), ("skip_extended_targets", C.c_int32)]

    @classmethod
    def default(cls, min_depth=3, min_count=2, min_percent=20, min_seq_id=0.0, skip_extended_targets=False):
        """the values `carpedeam contig_indels` passes without flags"""
        return cls(int(min_depth), int(min_count), int(min_percent), float(min_seq_id), int(bool(skip_extended_targets)))


class IndelSite(C.Structure):
    """cdm_indel_site: one supported place"""
    _fields_ = [(n, C.c_uint32) for n in ("query", "pos", "info", "count", "cross", "others", "n_letters", "reserved")] + [("letters", C.c_uint64)]


INDEL_DTYPE = np.dtype([(n, "<u4") for n in ("query", "pos", "info", "count", "cross", "others", "n_letters", "reserved")] + [("letters", "<u8")])
INDEL_INS, INDEL_DEL = 1, 2
INDEL_CALLED, INDEL_SUPPORTED, INDEL_MAJOR = 1, 2, 4


EXPORTS = [
    "cdm_last_error", "cdm_ctx_create", "cdm_ctx_destroy", "cdm_ctx_sync", "cdm_ctx_stream", "cdm_ctx_last_kernel_ms",
    "cdm_seqdb_upload", "cdm_seqdb_synth", "cdm_seqdb_size", "cdm_seqdb_residues", "cdm_seqdb_max_len", "cdm_seqdb_meta",
    "cdm_seqdb_download", "cdm_seqdb_download_stream", "cdm_seqdb_free", "cdm_seqdb_select_ext", "cdm_seqdb_select_assembled", "cdm_seqdb_index_copy", "cdm_seqdb_words", "cdm_seqdb_copy_packed", "cdm_seqdb_from_packed", "cdm_damage_load", "cdm_damage_get", "cdm_kmermatch", "cdm_hits_upload", "cdm_hits_count",
    "cdm_hits_download", "cdm_hits_free", "cdm_rescore", "cdm_rescore_tile", "cdm_alns_undefined", "cdm_alns_ry_download", "cdm_alns_upload", "cdm_alns_count", "cdm_alns_download", "cdm_alns_free",
    "cdm_evalue", "cdm_bit_score", "cdm_gapped_evalue", "cdm_correct", "cdm_extend",
    "cdm_kmermatch_part", "cdm_kmermatch_split_begin", "cdm_kpart_outgoing", "cdm_kmermatch_split_finish", "cdm_kpart_info", "cdm_kpart_stale", "cdm_kpart_gather", "cdm_kpart_sort", "cdm_kpart_vote", "cdm_kpart_cont_cap", "cdm_kmer_slot_split", "cdm_kpart_free", "cdm_dev_copy",
    "cdm_seqdb_from_packed_ext", "cdm_seqdb_copy_ext", "cdm_seqdb_export_packed", "cdm_seqdb_import_packed", "cdm_contig_merge", "cdm_cyclecheck", "cdm_seqdb_has_raw", "cdm_seqdb_copy_raw", "cdm_seqdb_attach_raw",
    "cdm_rescore_hamming", "cdm_align_hits", "cdm_align_mode", "cdm_pool_headroom", "cdm_pool_stats", "cdm_env_refresh",
    "cdm_pairs_merge", "cdm_pairs_count", "cdm_pairs_entries", "cdm_pairs_bytes", "cdm_pairs_kernel_ms", "cdm_pairs_download",
    "cdm_pairs_download_stream", "cdm_pairs_to_seqdb", "cdm_pairs_free",
    "cdm_pileup_profile", "cdm_pileup_depth", "cdm_pileup_bases", "cdm_sites_free", "cdm_pileup_breaks", "cdm_breaks_free", "cdm_pileup_map", "cdm_map_free", "cdm_alns_dedup", "cdm_pileup_links", "cdm_link_free", "cdm_pileup_junctions", "cdm_junction_free", "cdm_pileup_gapped", "cdm_gap_free", "cdm_pileup_indels", "cdm_indel_free", "cdm_pileup_depth_gapped", "cdm_pileup_bases_gapped", "cdm_pileup_breaks_gapped", "cdm_seqdb_concat",
    "cdm_comm_unique_id", "cdm_comm_create_rccl", "cdm_comm_create_ops", "cdm_comm_free", "cdm_comm_rank", "cdm_comm_world", "cdm_kmermatch_dist",
    "cdm_seqdb_allgather_owned", "cdm_reads_iteration_dist", "cdm_contig_iteration_dist", "cdm_comm_owned", "cdm_comm_last_path", "cdm_kpart_gather_at", "cdm_comm_standin_group", "cdm_comm_create_standin", "cdm_kpart_set_range",
]


AG_HOST_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
A2A_DEV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p)
AG_DEV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p)


class CommOps(C.Structure):
    """cdm_comm_ops (include/carpedeam_hip.h): the collectives of a caller-supplied transport"""
    _fields_ = [("user", C.c_void_p), ("all_gather_host", AG_HOST_FN), ("all_to_all_dev", A2A_DEV_FN), ("all_gather_dev", AG_DEV_FN)]


class CdmError(RuntimeError):
    pass


_lib = None


class MergeParams(C.Structure):
    """cdm_merge_params: mergereads' fixed values by default (mergereads.cpp:20-24)"""
    _fields_ = [("min_overlap", C.c_int), ("max_overlap", C.c_int), ("max_mismatch_density", C.c_float)]

    @classmethod
    def default(cls):
        return cls(15, 65, 0.10)


def lib():
    """Load libcarpedeam_hip.so (built in-tree by carpedeam_amd.build); fail loudly when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CdmError("libcarpedeam_hip.so not built: run `python -m carpedeam_amd.build` (no CPU fallback exists)")
        l = C.CDLL(LIB_PATH)
        vp, u64p, u32p, u8p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        l.cdm_last_error.restype = C.c_char_p
        l.cdm_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
        l.cdm_ctx_destroy.argtypes = [vp]
        l.cdm_ctx_destroy.restype = None
        l.cdm_ctx_sync.argtypes = [vp]
        l.cdm_ctx_stream.argtypes = [vp]
        l.cdm_ctx_stream.restype = vp
        l.cdm_ctx_last_kernel_ms.argtypes = [vp, C.c_int]
        l.cdm_ctx_last_kernel_ms.restype = C.c_float
        l.cdm_seqdb_upload.argtypes = [vp, vp, vp, vp, vp, vp, C.c_uint64, C.POINTER(vp)]
        l.cdm_seqdb_synth.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(vp)]
        for f in (l.cdm_seqdb_size, l.cdm_seqdb_residues, l.cdm_hits_count, l.cdm_alns_count):
            f.argtypes = [vp]
            f.restype = C.c_uint64
        l.cdm_seqdb_max_len.argtypes = [vp]
        l.cdm_seqdb_max_len.restype = C.c_uint32
        l.cdm_seqdb_meta.argtypes = [vp, vp, vp, vp, vp]
        l.cdm_seqdb_download.argtypes = [vp, vp, vp, vp]
        for f in (l.cdm_seqdb_free, l.cdm_hits_free, l.cdm_alns_free):
            f.argtypes = [vp]
            f.restype = None
        l.cdm_seqdb_select_ext.argtypes = [vp, vp, C.POINTER(vp)]
        l.cdm_seqdb_index_copy.argtypes = [vp, vp, C.POINTER(vp)]
        l.cdm_seqdb_select_assembled.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(vp), u64p]
        l.cdm_seqdb_words.argtypes = [vp]
        l.cdm_seqdb_words.restype = C.c_uint64
        l.cdm_seqdb_copy_packed.argtypes = [vp, vp, vp, vp, vp, vp]
        l.cdm_seqdb_has_raw.argtypes = [vp]
        l.cdm_seqdb_copy_raw.argtypes = [vp, vp, vp, vp]
        l.cdm_seqdb_attach_raw.argtypes = [vp, vp, vp, vp]
        l.cdm_seqdb_from_packed.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint8, C.POINTER(vp)]
        l.cdm_pairs_merge.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, C.POINTER(MergeParams), C.POINTER(vp)]
        for f in (l.cdm_pairs_count, l.cdm_pairs_entries, l.cdm_pairs_bytes):
            f.argtypes = [vp]
            f.restype = C.c_uint64
        l.cdm_pairs_kernel_ms.argtypes = [vp]
        l.cdm_pairs_kernel_ms.restype = C.c_float
        l.cdm_pairs_download.argtypes = [vp, vp, vp, vp, vp, vp]
        l.cdm_pairs_to_seqdb.argtypes = [vp, vp, C.c_uint32, C.POINTER(vp)]
        l.cdm_pairs_free.argtypes = [vp]
        l.cdm_pairs_free.restype = None
        l.cdm_damage_load.argtypes = [vp, C.c_char_p]
        l.cdm_damage_get.argtypes = [vp, vp]
        l.cdm_kmermatch.argtypes = [vp, vp, C.POINTER(KmerParams), C.POINTER(vp)]
        l.cdm_hits_upload.argtypes = [vp, vp, vp, vp, C.POINTER(vp)]
        l.cdm_hits_download.argtypes = [vp, vp, vp, vp]
        l.cdm_rescore.argtypes = [vp, vp, vp, C.POINTER(RescoreParams), C.POINTER(vp)]
        l.cdm_rescore_tile.argtypes = []
        l.cdm_rescore_tile.restype = C.c_uint32
        l.cdm_alns_undefined.argtypes = [vp]
        l.cdm_alns_undefined.restype = C.c_uint64
        l.cdm_alns_ry_download.argtypes = [vp, vp, vp]
        l.cdm_rescore_hamming.argtypes = [vp, vp, vp, C.POINTER(HammingParams), C.POINTER(vp)]
        l.cdm_align_hits.argtypes = [vp, vp, C.POINTER(AlignParams), vp, C.c_uint64, vp, vp]
        l.cdm_align_mode.argtypes = []
        l.cdm_pool_headroom.argtypes = [C.c_float]
        l.cdm_pool_headroom.restype = None
        l.cdm_alns_upload.argtypes = [vp, vp, vp, vp, C.POINTER(vp)]
        l.cdm_alns_download.argtypes = [vp, vp, vp, vp]
        l.cdm_evalue.argtypes = [C.c_double, C.c_double, C.c_uint64]
        l.cdm_evalue.restype = C.c_double
        l.cdm_bit_score.argtypes = [C.c_double]
        l.cdm_correct.argtypes = [vp, vp, vp, C.POINTER(AncientParams), C.POINTER(vp)]
        l.cdm_extend.argtypes = [vp, vp, vp, C.POINTER(AncientParams), C.POINTER(vp), vp]
        l.cdm_kmermatch_part.argtypes = [vp, vp, C.POINTER(KmerParams), C.c_int, C.c_int, C.POINTER(vp)]
        if hasattr(l, "cdm_kmermatch_split_begin"):
            l.cdm_kmermatch_split_begin.argtypes = [vp, vp, C.POINTER(KmerParams), C.c_int, C.c_int, C.POINTER(vp)]
            l.cdm_kpart_outgoing.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64)]
            l.cdm_kmermatch_split_finish.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint64, C.c_int]
        l.cdm_kpart_info.argtypes = [vp, vp]
        l.cdm_kpart_stale.argtypes = [vp, vp, C.c_uint64, vp]
        l.cdm_kpart_gather.argtypes = [vp, vp, C.c_int, vp, C.POINTER(vp)]
        l.cdm_kpart_sort.argtypes = [vp, vp, vp, C.c_uint64, vp, vp]
        l.cdm_kpart_vote.argtypes = [vp, vp, vp, vp, C.POINTER(vp)]
        l.cdm_kpart_free.argtypes = [vp]
        l.cdm_kpart_free.restype = None
        l.cdm_dev_copy.argtypes = [vp, vp, vp, C.c_uint64]
        l.cdm_kmer_slot_split.argtypes = [C.c_int, C.POINTER(C.c_int)]
        l.cdm_seqdb_from_packed_ext.argtypes = [vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_uint64, C.POINTER(vp)]
        l.cdm_seqdb_copy_ext.argtypes = [vp, vp, vp]
        l.cdm_pileup_profile.argtypes = [vp, vp, vp, vp, C.c_uint64, C.POINTER(PileupParams), vp, vp, vp]
        l.cdm_pileup_depth.argtypes = [vp, vp, vp, vp, C.c_uint64, C.POINTER(DepthParams), vp, vp]
        l.cdm_pileup_bases.argtypes = [vp, vp, vp, vp, C.c_uint64, C.POINTER(BasesParams), vp, vp, C.POINTER(C.POINTER(Site)), u64p, C.POINTER(C.c_float)]
        l.cdm_sites_free.argtypes = [C.POINTER(Site)]
        l.cdm_sites_free.restype = None
        l.cdm_pileup_breaks.argtypes = [vp, vp, vp, vp, C.c_uint64, C.POINTER(BreaksParams), vp, vp, C.POINTER(C.POINTER(Break)), u64p, C.POINTER(C.c_float)]
        l.cdm_breaks_free.argtypes = [C.POINTER(Break)]
        l.cdm_breaks_free.restype = None
        l.cdm_pileup_map.argtypes = [vp, vp, vp, vp, C.c_uint64, C.POINTER(MapParams), vp, C.POINTER(C.POINTER(MapRec)), u64p, C.POINTER(u32p), u64p, C.POINTER(C.c_float)]
        l.cdm_map_free.argtypes = [C.POINTER(MapRec), u32p]
        l.cdm_map_free.restype = None
        l.cdm_alns_dedup.argtypes = [vp, vp, vp, vp, C.c_uint64, C.POINTER(DedupParams), C.POINTER(vp), vp, vp, C.POINTER(C.c_float)]
        l.cdm_pileup_links.argtypes = [vp, vp, vp, vp, C.c_uint64, C.POINTER(LinksParams), vp, vp, C.POINTER(C.POINTER(Link)), u64p, C.POINTER(C.c_float)]
        l.cdm_link_free.argtypes = [C.POINTER(Link)]
        l.cdm_link_free.restype = None
        l.cdm_pileup_junctions.argtypes = [vp, vp, vp, vp, C.c_uint64, C.POINTER(LinksParams), vp, C.c_uint64, vp, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(u32p), C.POINTER(C.c_float)]
        l.cdm_junction_free.argtypes = [C.POINTER(C.c_uint8), u32p]
        l.cdm_junction_free.restype = None
        l.cdm_pileup_gapped.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.POINTER(GapParams), vp, C.POINTER(C.POINTER(GapRec)), u64p, C.POINTER(u32p), u64p, C.POINTER(u32p), u64p,
                                        C.POINTER(C.c_float)]
        l.cdm_gap_free.argtypes = [C.POINTER(GapRec), u32p, u32p]
        l.cdm_gap_free.restype = None
        l.cdm_pileup_indels.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(IndelParams), vp, vp, C.POINTER(C.POINTER(IndelSite)), u64p,
                                        C.POINTER(C.POINTER(C.c_uint8)), u64p, C.POINTER(C.c_float)]
        l.cdm_indel_free.argtypes = [C.POINTER(IndelSite), C.POINTER(C.c_uint8)]
        l.cdm_indel_free.restype = None
        gapped = [vp, C.c_uint64, vp, C.c_uint64]       # recs, n_recs, ops, n_ops in front of the parameters
        l.cdm_pileup_depth_gapped.argtypes = [vp, vp, vp, vp, C.c_uint64] + gapped + [C.POINTER(DepthParams), vp, vp, C.POINTER(C.c_float)]
        l.cdm_pileup_bases_gapped.argtypes = [vp, vp, vp, vp, C.c_uint64] + gapped + [C.POINTER(BasesParams), vp, vp, C.POINTER(C.POINTER(Site)), u64p, C.POINTER(C.c_float)]
        l.cdm_pileup_breaks_gapped.argtypes = [vp, vp, vp, vp, C.c_uint64] + gapped + [C.POINTER(BreaksParams), vp, vp, C.POINTER(C.POINTER(Break)), u64p, C.POINTER(C.c_float)]
        l.cdm_seqdb_concat.argtypes = [vp, vp, vp, C.c_uint8, C.c_uint8, C.POINTER(vp)]
        l.cdm_pileup_chunk_records.argtypes = []
        l.cdm_pileup_chunk_records.restype = C.c_uint32
        l.cdm_contig_merge.argtypes = [vp, vp, vp, C.POINTER(AncientParams), C.c_float, C.POINTER(vp)]
        l.cdm_cyclecheck.argtypes = [vp, vp, C.c_uint32, C.c_int, C.POINTER(vp), C.POINTER(vp), vp]
        if hasattr(l, "cdm_comm_create_ops"):
            l.cdm_comm_unique_id.argtypes = [vp]
            l.cdm_comm_create_rccl.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
            l.cdm_comm_create_ops.argtypes = [vp, C.c_int, C.c_int, C.POINTER(CommOps), C.POINTER(vp)]
            l.cdm_comm_free.argtypes = [vp]
            l.cdm_comm_free.restype = None
            l.cdm_kmermatch_dist.argtypes = [vp, vp, vp, C.POINTER(KmerParams), C.POINTER(vp)]
            l.cdm_seqdb_allgather_owned.argtypes = [vp, vp, vp, C.POINTER(vp)]
            if hasattr(l, "cdm_comm_owned"):
                l.cdm_comm_owned.argtypes = [vp, C.c_uint64, vp]
                l.cdm_comm_world.argtypes = [vp]
            l.cdm_reads_iteration_dist.argtypes = [vp, vp, vp, C.POINTER(KmerParams), C.POINTER(RescoreParams), C.POINTER(AncientParams), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
            l.cdm_contig_iteration_dist.argtypes = [vp, vp, vp, C.POINTER(KmerParams), C.POINTER(RescoreParams), C.POINTER(AncientParams), C.c_float, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        try:
            l.cdm_env_refresh.restype = None
        except AttributeError:          # (CDM_LIB names an older build of the library - bisecting: it reads its switches with getenv)
            pass
        _lib = l
    # The library snapshots its CDM_* switches once per process (no getenv on its call paths, csrc/pool.h).  Tests and A/B runs change
    # them between calls of one process: when os.environ's CDM_* entries differ from what the library last saw, it reads them again.
    global _env_seen
    env = {k: v for k, v in os.environ.items() if k.startswith("CDM_")}
    if env != _env_seen:
        _env_seen = env
        if hasattr(_lib, "cdm_env_refresh"):
            _lib.cdm_env_refresh()
    return _lib


_env_seen = None


def _gapped_args(gapped):
    """(recs, ops) -> the four arguments recs, n_recs, ops, n_ops of the *_gapped calls (a pointer of data_as keeps its array alive)"""
    recs = np.ascontiguousarray(gapped[0], GAP_DTYPE).reshape(-1)
    ops = np.ascontiguousarray(gapped[1], np.uint32).reshape(-1)
    return _ptr(recs) if len(recs) else None, len(recs), _ptr(ops) if len(ops) else None, len(ops)


def pileup_chunk_records():
    """records per work item of cdm_pileup_profile's kernel as the next call cuts them (CDM_PILEUP_CHUNK; tests)"""
    return int(lib().cdm_pileup_chunk_records())


def kmer_slot_split(k):
    """k-mer bits that sort 1 on the slot layout leaves to the grouping kernel at this k (cdm_kmer_slot_split; reads CDM_SLOT_LOWBITS)"""
    n = C.c_int(-1)
    _check(lib().cdm_kmer_slot_split(int(k), C.byref(n)))
    return n.value


def pool_stats():
    """the device-memory allocator's counters (cdm_pool_stats)"""
    a = np.zeros(8, np.uint64)
    lib().cdm_pool_stats(a.ctypes.data_as(C.c_void_p))
    return {"requests": int(a[0]), "served_without_driver": int(a[1]), "driver_calls": int(a[2]), "driver_bytes": int(a[3]), "driver_seconds": a[4] / 1e9, "trims": int(a[5]),
            "mapped_bytes": int(a[6]), "in_use_bytes": int(a[7])}


def _check(rc):
    if rc != 0:
        raise CdmError("cdm error %d: %s" % (rc, lib().cdm_last_error().decode()))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class SeqDb:
    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def __del__(self):
        if getattr(self, "h", None) and lib is not None:      # (at interpreter shutdown the module's globals are gone already)
            lib().cdm_seqdb_free(self.h)
            self.h = None

    @property
    def n(self):
        return int(lib().cdm_seqdb_size(self.h))

    @property
    def residues(self):
        return int(lib().cdm_seqdb_residues(self.h))

    @property
    def words(self):
        return int(lib().cdm_seqdb_words(self.h))

    def select_ext(self):
        """the contigs (wasExtended == 1) as a new device DB"""
        h = C.c_void_p()
        _check(lib().cdm_seqdb_select_ext(self.ctx.h, self.h, C.byref(h)))
        return SeqDb(self.ctx, h)

    def copy_ext(self, ext_ptr):
        _check(lib().cdm_seqdb_copy_ext(self.ctx.h, self.h, ext_ptr))

    def copy_packed(self, codes_ptr, nmask_ptr, len_ptr, key_ptr):
        """copy the packed form into DEVICE buffers (raw pointers, e.g. torch tensor .data_ptr())"""
        _check(lib().cdm_seqdb_copy_packed(self.ctx.h, self.h, codes_ptr, nmask_ptr, len_ptr, key_ptr))

    @property
    def has_raw(self):
        """the DB carries letters beyond ACGTN (their original bytes travel beside the packed form: copy_raw / attach_raw)"""
        return bool(lib().cdm_seqdb_has_raw(self.h))

    def copy_raw(self, raw_ptr, flags_ptr):
        _check(lib().cdm_seqdb_copy_raw(self.ctx.h, self.h, raw_ptr, flags_ptr))

    def attach_raw(self, raw_ptr, flags_ptr):
        _check(lib().cdm_seqdb_attach_raw(self.ctx.h, self.h, raw_ptr, flags_ptr))

    def meta(self):
        n = self.n
        lens, keys, ext = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint8)
        _check(lib().cdm_seqdb_meta(self.ctx.h, self.h, _ptr(lens), _ptr(keys), _ptr(ext)))
        return lens, keys, ext

    def download_into(self, buf, offs):
        """sequence i as "SEQ\\n" at buf[offs[i]:] (uint8 / uint64 numpy arrays owned by the caller; the library writes the whole range up to the last entry's end: bytes between entries come out as NUL)"""
        _check(lib().cdm_seqdb_download(self.ctx.h, self.h, _ptr(buf), _ptr(offs)))

    def download(self):
        """-> (list of bytes sequences, keys, ext)"""
        if self.n == 0:
            return [], np.zeros(0, np.uint32), np.zeros(0, np.uint8)
        lens, keys, ext = self.meta()
        offs = np.zeros(self.n, np.uint64)
        offs[1:] = np.cumsum(lens[:-1].astype(np.uint64) + 1)
        total = int(lens.astype(np.uint64).sum() + self.n)
        buf = np.empty(total, np.uint8)
        _check(lib().cdm_seqdb_download(self.ctx.h, self.h, _ptr(buf), _ptr(offs)))
        raw = buf.tobytes()
        seqs = [raw[int(o):int(o) + int(l)] for o, l in zip(offs, lens)]
        return seqs, keys, ext


class _Csr:
    free = None
    count_fn = None
    download_fn = None
    dtype = None

    def __init__(self, ctx, handle, n):
        self.ctx, self.h, self.n = ctx, handle, n

    def __del__(self):
        if getattr(self, "h", None) and lib is not None:
            getattr(lib(), self.free)(self.h)
            self.h = None

    @property
    def count(self):
        return int(getattr(lib(), self.count_fn)(self.h))

    def download(self):
        off = np.empty(self.n + 1, np.uint64)
        rec = np.empty(self.count, self.dtype)
        _check(getattr(lib(), self.download_fn)(self.ctx.h, self.h, _ptr(off), _ptr(rec)))
        return off, rec


class Hits(_Csr):
    free, count_fn, download_fn, dtype = "cdm_hits_free", "cdm_hits_count", "cdm_hits_download", HIT_DTYPE


class Alns(_Csr):
    free, count_fn, download_fn, dtype = "cdm_alns_free", "cdm_alns_count", "cdm_alns_download", ALN_DTYPE

    @property
    def undefined_records(self):
        """identity records written with the coordinates -1 (cdm_alns_undefined)"""
        return int(lib().cdm_alns_undefined(self.h))

    def download_ry(self):
        """the purine/pyrimidine mismatch count of every record of a set made by Ctx.rescore (0xFFFF = not counted)"""
        ry = np.empty(self.count, np.uint16)
        _check(lib().cdm_alns_ry_download(self.ctx.h, self.h, _ptr(ry)))
        return ry


KPART_SLICES = 256          # CDM_KPART_SLICES


class KPart:
    """One k-mer range of a split kmermatcher run (cdm_kpart)."""

    def __init__(self, ctx, handle, db):
        self.ctx, self.h, self.db = ctx, handle, db

    def __del__(self):
        if getattr(self, "h", None) and lib is not None:
            lib().cdm_kpart_free(self.h)
            self.h = None

    def info(self):
        a = np.zeros(4, np.uint64)
        _check(lib().cdm_kpart_info(self.h, _ptr(a)))
        return {"real": int(a[0]), "kept": int(a[1]), "any_below": bool(a[2]), "n": int(a[3])}

    def outgoing(self):
        """after Ctx.kmermatch_split_begin -> (offsets[KPART_SLICES + 1], keys ptr, values ptr, bytes per value, hash keys ptr, hash values
        ptr, hash tuples): this rank's tuples ordered by fine slices of the k-mer space (the ranks' ranges are runs of slices)"""
        off = np.zeros(KPART_SLICES + 1, np.uint64)
        k, v, hk, hv = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        vb, nh = C.c_int(), C.c_uint64()
        _check(lib().cdm_kpart_outgoing(self.h, _ptr(off), C.byref(k), C.byref(v), C.byref(vb), C.byref(hk), C.byref(hv), C.byref(nh)))
        return off, k.value or 0, v.value or 0, vb.value, hk.value or 0, hv.value or 0, nh.value

    def split_finish(self, keys_ptr, vals_ptr, m, hash_keys_ptr, hash_vals_ptr, n_hash, below):
        _check(lib().cdm_kmermatch_split_finish(self.ctx.h, self.h, keys_ptr, vals_ptr, int(m), hash_keys_ptr, hash_vals_ptr, int(n_hash), int(bool(below))))

    def stale(self, j):
        a = np.zeros(67, np.uint32)
        _check(lib().cdm_kpart_stale(self.ctx.h, self.h, int(j), _ptr(a)))
        return a

    def gather(self, nranks):
        """-> (offsets[nranks + 1], device pointer of the group keys grouped by representative)"""
        off = np.zeros(nranks + 1, np.uint64)
        p = C.c_void_p()
        _check(lib().cdm_kpart_gather(self.ctx.h, self.h, nranks, _ptr(off), C.byref(p)))
        return off, p.value or 0

    def sort(self, keys_ptr, n_keys):
        """sort 2 on the received keys -> (head list, sorted tuples, target id of the last one)"""
        head = np.zeros(lib().cdm_kpart_cont_cap() + 3, np.uint32)
        info = np.zeros(2, np.uint64)
        _check(lib().cdm_kpart_sort(self.ctx.h, self.h, keys_ptr, int(n_keys), _ptr(head), _ptr(info)))
        return head, int(info[0]), int(info[1])

    def vote(self, cont, stale):
        st = np.ascontiguousarray(stale[:65], np.uint32)
        ct = None if cont is None else np.ascontiguousarray(cont, np.uint32)
        h = C.c_void_p()
        _check(lib().cdm_kpart_vote(self.ctx.h, self.h, _ptr(ct), _ptr(st), C.byref(h)))
        return Hits(self.ctx, h, self.db.n)


class Ctx:
    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib().cdm_ctx_create(device, C.byref(h)))
        self.h = h

    def __del__(self):
        if getattr(self, "h", None) and lib is not None:
            lib().cdm_ctx_destroy(self.h)
            self.h = None

    def sync(self):
        _check(lib().cdm_ctx_sync(self.h))

    def last_kernel_ms(self, which):
        return float(lib().cdm_ctx_last_kernel_ms(self.h, which))

    def damage_load(self, prefix):
        _check(lib().cdm_damage_load(self.h, prefix.encode()))

    def damage_get(self):
        out = np.empty(352, np.longdouble)
        _check(lib().cdm_damage_get(self.h, _ptr(out)))
        return out.reshape(2, 11, 4, 4)

    # ---- sequence DB
    def upload_seqs(self, seqs, keys=None, ext=None):
        """seqs: list of bytes/str; builds the 'SEQ\\n\\0' data blob the way the DB data file holds it."""
        bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        n = len(bs)
        lens = np.array([len(b) for b in bs], np.uint32)
        offs = np.zeros(n, np.uint64)
        offs[1:] = np.cumsum(lens[:-1].astype(np.uint64) + 2)
        data = np.frombuffer(b"".join(b + b"\n\0" for b in bs), np.uint8)
        keys = np.arange(n, dtype=np.uint32) if keys is None else np.asarray(keys, np.uint32)
        ext = None if ext is None else np.asarray(ext, np.uint8)
        h = C.c_void_p()
        _check(lib().cdm_seqdb_upload(self.h, _ptr(data), _ptr(offs), _ptr(lens), _ptr(keys), _ptr(ext), n, C.byref(h)))
        return SeqDb(self, h)

    def merge_pairs(self, pairs, par=None, to_seqdb=False, first_key=0):
        """mergereads on the device for one batch.  pairs: [((seq1, qual1), (seq2, qual2))] as read (bytes).  Returns (status, entries):
        status[i] = 1 when pair i was combined; entries = [seq] in mergereads' order (the consensus, or R1 and R2 reverse-complemented) -
        or, with to_seqdb, a resident SeqDb of them (keys first_key, first_key + 1, ...; wasExtended 1)."""
        n = len(pairs)
        blobs = []
        for side in (0, 1):
            seqs = [bytes(p[side][0]) for p in pairs]
            quals = [bytes(p[side][1]) for p in pairs]
            lens = np.array([len(x) for x in seqs], np.uint32)
            offs = np.zeros(n, np.uint64)
            if n > 1:
                offs[1:] = np.cumsum(lens[:-1].astype(np.uint64))
            sb = np.frombuffer(b"".join(seqs) + b"\0", np.uint8)
            qb = np.frombuffer(b"".join(quals) + b"\0", np.uint8)
            blobs.append((sb, qb, offs, lens))
        (s1, q1, o1, l1), (s2, q2, o2, l2) = blobs
        par = par or MergeParams.default()
        h = C.c_void_p()
        _check(lib().cdm_pairs_merge(self.h, _ptr(s1), _ptr(q1), _ptr(o1), _ptr(l1), _ptr(s2), _ptr(q2), _ptr(o2), _ptr(l2), n, C.byref(par), C.byref(h)))
        try:
            status = np.zeros(n + 1, np.uint8)
            ne, nb = lib().cdm_pairs_entries(h), lib().cdm_pairs_bytes(h)
            if to_seqdb:
                _check(lib().cdm_pairs_download(self.h, h, _ptr(status), None, None, None))
                d = C.c_void_p()
                _check(lib().cdm_pairs_to_seqdb(self.h, h, first_key, C.byref(d)))
                return status[:n], SeqDb(self, d)
            text = np.zeros(nb + 1, np.uint8)
            elen = np.zeros(ne + 1, np.uint32)
            _check(lib().cdm_pairs_download(self.h, h, _ptr(status), None, _ptr(text), _ptr(elen)))
            raw, out, at = text.tobytes(), [], 0
            for k in range(ne):
                out.append(raw[at:at + int(elen[k])])
                at += int(elen[k]) + 2
            return status[:n], out
        finally:
            lib().cdm_pairs_free(h)

    def upload_keyed_seqdb(self, keyed):
        """keyed: dict key -> (payload incl. newline, ext) as mmdb.read_db / load_keyed give it."""
        ks = sorted(keyed)
        return self.upload_seqs([keyed[k][0].rstrip(b"\n") for k in ks], ks, [keyed[k][1] for k in ks])

    def synth(self, n, lo, hi, seed, n_total=None, first=0):
        h = C.c_void_p()
        _check(lib().cdm_seqdb_synth(self.h, n if n_total is None else n_total, first, n, lo, hi, seed, C.byref(h)))
        return SeqDb(self, h)

    def from_packed(self, codes_ptr, nmask_ptr, len_ptr, key_ptr, n, words, ext_value=1):
        h = C.c_void_p()
        _check(lib().cdm_seqdb_from_packed(self.h, codes_ptr, nmask_ptr, len_ptr, key_ptr, n, words, ext_value, C.byref(h)))
        return SeqDb(self, h)

    def contig_merge(self, db, alns, par=None, merge_seq_id=0.99):
        par = par or AncientParams.default()
        h = C.c_void_p()
        _check(lib().cdm_contig_merge(self.h, db.h, alns.h, C.byref(par), merge_seq_id, C.byref(h)))
        return SeqDb(self, h)

    def cyclecheck(self, db, max_seq_len=65535, chop_cycle=False):
        """(cyclic contigs [cut at the split diagonal if chop_cycle], the other contigs, split diagonal per contig)"""
        import numpy as np
        c, r = C.c_void_p(), C.c_void_p()
        split = np.zeros(max(db.n, 1), dtype=np.uint32)
        _check(lib().cdm_cyclecheck(self.h, db.h, max_seq_len, 1 if chop_cycle else 0, C.byref(c), C.byref(r), split.ctypes.data))
        return SeqDb(self, c), SeqDb(self, r), split[:db.n]

    def index_copy(self, db):
        """keys, lengths and flags of db as a DB without letters (the `source` of select_assembled)"""
        h = C.c_void_p()
        _check(lib().cdm_seqdb_index_copy(self.h, db.h, C.byref(h)))
        return SeqDb(self, h)

    def select_assembled(self, result, source, min_len):
        """the workflow's selection of the assembled contigs (data/nuclassemble.sh:214-233): the entries of `result` that outgrew the
        entry of the same key in `source` and hold at least min_len letters, as a new device DB (possibly empty)"""
        h, kept = C.c_void_p(), C.c_uint64(0)
        _check(lib().cdm_seqdb_select_assembled(self.h, result.h, source.h, min_len, C.byref(h), C.byref(kept)))
        db = SeqDb(self, h)
        assert db.n == kept.value
        return db

    def from_packed_ext(self, codes_ptr, nmask_ptr, len_ptr, key_ptr, ext_ptr, n, words):
        h = C.c_void_p()
        _check(lib().cdm_seqdb_from_packed_ext(self.h, codes_ptr, nmask_ptr, len_ptr, key_ptr, ext_ptr, n, words, C.byref(h)))
        return SeqDb(self, h)

    def dev_copy(self, dst_ptr, src_ptr, nbytes):
        _check(lib().cdm_dev_copy(self.h, dst_ptr, src_ptr, nbytes))

    def kmermatch_part(self, db, part, nparts, par=None):
        """phase A of kmermatcher on k-mer range part/nparts (multi-GPU runs, carpedeam_amd/shard.py)"""
        par = par or KmerParams.reads_default()
        h = C.c_void_p()
        _check(lib().cdm_kmermatch_part(self.h, db.h, C.byref(par), part, nparts, C.byref(h)))
        return KPart(self, h, db)

    def kmermatch_split_begin(self, db, rank, nranks, par=None):
        """the same first half with the extraction split by reads: this rank's block of the sequences, the tuples ordered by the k-mer
        range they go to (KPart.outgoing, then KPart.split_finish on what arrived)"""
        par = par or KmerParams.reads_default()
        h = C.c_void_p()
        _check(lib().cdm_kmermatch_split_begin(self.h, db.h, C.byref(par), rank, nranks, C.byref(h)))
        return KPart(self, h, db)

    # ---- containers
    def upload_hits(self, db, off, rec):
        off = np.ascontiguousarray(off, np.uint64)
        rec = np.ascontiguousarray(rec, HIT_DTYPE)
        h = C.c_void_p()
        _check(lib().cdm_hits_upload(self.h, db.h, _ptr(off), _ptr(rec), C.byref(h)))
        return Hits(self, h, db.n)

    def upload_alns(self, db, off, rec):
        off = np.ascontiguousarray(off, np.uint64)
        rec = np.ascontiguousarray(rec, ALN_DTYPE)
        h = C.c_void_p()
        _check(lib().cdm_alns_upload(self.h, db.h, _ptr(off), _ptr(rec), C.byref(h)))
        return Alns(self, h, db.n)

    # ---- stages
    def kmermatch(self, db, par=None):
        par = par or KmerParams.reads_default()
        h = C.c_void_p()
        _check(lib().cdm_kmermatch(self.h, db.h, C.byref(par), C.byref(h)))
        return Hits(self, h, db.n)

    def rescore(self, db, hits, par=None):
        par = par or RescoreParams.default()
        h = C.c_void_p()
        _check(lib().cdm_rescore(self.h, db.h, hits.h, C.byref(par), C.byref(h)))
        return Alns(self, h, db.n)

    @staticmethod
    def rescore_tile():
        """hits per block of cdm_rescore's kernel"""
        return int(lib().cdm_rescore_tile())

    def rescore_hamming(self, db, hits, par=None):
        par = par or HammingParams.linclust()
        h = C.c_void_p()
        _check(lib().cdm_rescore_hamming(self.h, db.h, hits.h, C.byref(par), C.byref(h)))
        return Hits(self, h, db.n)

    def align_hits(self, db, hits, par=None):
        """the gapped extensions of `align` for seeded hits (a structured array of ALIGN_HIT_DTYPE); returns (results of
        ALIGN_RESULT_DTYPE, {"slices", "rows", "trace_bytes", "seconds"})"""
        par = par or AlignParams.linclust()
        hits = np.ascontiguousarray(hits, ALIGN_HIT_DTYPE)
        res = np.zeros(len(hits), ALIGN_RESULT_DTYPE)
        stats = np.zeros(4, np.uint64)
        _check(lib().cdm_align_hits(self.h, db.h, C.byref(par), _ptr(hits), len(hits), _ptr(res), _ptr(stats)))
        return res, {"slices": int(stats[0]), "rows": int(stats[1]), "trace_bytes": int(stats[2]), "seconds": stats[3] / 1e6}

    def correct(self, db, alns, par=None):
        par = par or AncientParams.default()
        h = C.c_void_p()
        _check(lib().cdm_correct(self.h, db.h, alns.h, C.byref(par), C.byref(h)))
        return SeqDb(self, h)

    def concat(self, a, b, ext_a, ext_b):
        """a's entries, then b's, as one resident DB: keys 0 .. n_a + n_b - 1, the wasExtended flags of the parts set to ext_a / ext_b"""
        h = C.c_void_p()
        _check(lib().cdm_seqdb_concat(self.h, a.h, b.h, int(ext_a), int(ext_b), C.byref(h)))
        return SeqDb(self, h)

    def pileup_profile(self, db, alns, queries, ends=16, min_seq_id=0.0, skip_extended_targets=False):
        """coverage and damage tables of the listed queries (cdm_pileup_profile) -> (counts[nq, 2, ends, 4, 4] - 5' table, 3' table, each
        [distance from that end of the read][query base as the read's strand sees it][read base] -, reads[nq], columns[nq]), uint64"""
        q = np.ascontiguousarray(queries, np.uint32).reshape(-1)
        nq = len(q)
        shape = (nq, 2, max(int(ends), 0), 4, 4)
        counts, reads, columns = np.zeros(shape, np.uint64), np.zeros(nq, np.uint64), np.zeros(nq, np.uint64)
        par = PileupParams(int(ends), float(min_seq_id), int(bool(skip_extended_targets)))
        _check(lib().cdm_pileup_profile(self.h, db.h, alns.h, _ptr(q), nq, C.byref(par), _ptr(counts), _ptr(reads), _ptr(columns)))
        return counts, reads, columns

    def pileup_depth(self, db, alns, queries, edge=0, min_seq_id=0.0, skip_extended_targets=False, track=False, gapped=None):
        """depth statistics of the listed queries (cdm_pileup_depth) -> stats[nq, 8] uint64: reads, columns, breadth, window, covered,
        sum, sumsq, max; with track also the depth at every position, a list of uint32 arrays, one per listed query.  gapped: None, or
        (recs, ops) as pileup_gapped returned them for the same queries - cdm_pileup_depth_gapped, whose device time
        self.depth_kernel_ms then holds"""
        q = np.ascontiguousarray(queries, np.uint32).reshape(-1)
        nq = len(q)
        stats = np.zeros((nq, 8), np.uint64)
        lens, depth = None, None
        if track:
            if nq and int(q.max()) < db.n:         # (an index beyond the DB is the library's to refuse: nothing is written then)
                lens = db.meta()[0][q].astype(np.int64)
            else:
                lens = np.zeros(nq, np.int64)
            depth = np.zeros(max(int(lens.sum()), 1), np.uint32)
        par = DepthParams(int(edge), float(min_seq_id), int(bool(skip_extended_targets)))
        if gapped is None:
            _check(lib().cdm_pileup_depth(self.h, db.h, alns.h, _ptr(q), nq, C.byref(par), _ptr(stats), _ptr(depth)))
        else:
            ms = C.c_float(0.0)
            rc = lib().cdm_pileup_depth_gapped(self.h, db.h, alns.h, _ptr(q), nq, *_gapped_args(gapped), C.byref(par), _ptr(stats), _ptr(depth), C.byref(ms))
            self.depth_kernel_ms = float(ms.value)          # (0 behind a refusal: no kernel ran)
            _check(rc)
        if not track:
            return stats
        ends = np.cumsum(lens)
        return stats, [depth[int(e - l):int(e)].copy() for l, e in zip(lens, ends)]

    def pileup_bases(self, db, alns, queries, mask_ends=0, min_depth=3, min_alt_count=2, min_alt_percent=20, min_seq_id=0.0, skip_extended_targets=False,
                     counts=False, sites=False, gapped=None):
        """base counts and variant sites of the listed queries (cdm_pileup_bases; with gapped = (recs, ops) as pileup_gapped returned them
        for the same queries cdm_pileup_bases_gapped) -> stats[nq, 8] uint64: reads, columns, bases,
        mismatches, called, differs, variable, flagged; with counts also a list of uint32 [length, 8] arrays, one per listed query
        (forward A,C,G,T, reverse A,C,G,T); with sites also the site records as an array of SITE_DTYPE.  The order of the extras in the
        returned tuple is counts, sites.  self.bases_kernel_ms holds the device time of the call's kernels"""
        q = np.ascontiguousarray(queries, np.uint32).reshape(-1)
        nq = len(q)
        stats = np.zeros((nq, 8), np.uint64)
        lens, table = None, None
        if counts:
            if nq and int(q.max()) < db.n:         # (an index beyond the DB is the library's to refuse: nothing is written then)
                lens = db.meta()[0][q].astype(np.int64)
            else:
                lens = np.zeros(nq, np.int64)
            table = np.zeros((max(int(lens.sum()), 1), 8), np.uint32)
        par = BasesParams(int(mask_ends), int(min_depth), int(min_alt_count), int(min_alt_percent), float(min_seq_id), int(bool(skip_extended_targets)))
        ptr, n_sites, ms = C.POINTER(Site)(), C.c_uint64(0), C.c_float(0.0)
        tail = (C.byref(par), _ptr(stats), _ptr(table), C.byref(ptr) if sites else None, C.byref(n_sites) if sites else None, C.byref(ms))
        if gapped is None:
            rc = lib().cdm_pileup_bases(self.h, db.h, alns.h, _ptr(q), nq, *tail)
        else:
            rc = lib().cdm_pileup_bases_gapped(self.h, db.h, alns.h, _ptr(q), nq, *_gapped_args(gapped), *tail)
        self.bases_kernel_ms = float(ms.value)          # (0 behind a refusal of the gapped call: no kernel ran)
        _check(rc)
        out = [stats]
        if counts:
            ends = np.cumsum(lens)
            out.append([table[int(e - l):int(e)].copy() for l, e in zip(lens, ends)])
        if sites:
            n = int(n_sites.value)
            assert (n == 0) == (not ptr)
            recs = np.empty(n, SITE_DTYPE)
            if n:
                C.memmove(recs.ctypes.data, ptr, n * C.sizeof(Site))
                lib().cdm_sites_free(ptr)
            out.append(recs)
        return out[0] if len(out) == 1 else tuple(out)

    def pileup_breaks(self, db, alns, queries, anchor=16, edge=50, min_span=1, min_span_percent=0, min_seq_id=0.0, skip_extended_targets=False,
                      track=False, breaks=False, gapped=None):
        """break points of the listed queries (cdm_pileup_breaks; with gapped = (recs, ops) as pileup_gapped returned them for the same
        queries cdm_pileup_breaks_gapped) -> stats[nq, 8] uint64: reads, columns, window, weak, breaks, joins,
        min_span, sum_span; with track also the span at every boundary b = 0 .. len - 1, a list of uint32 arrays, one per listed query;
        with breaks also the break records as an array of BREAK_DTYPE.  The order of the extras in the returned tuple is track, breaks.
        self.breaks_kernel_ms holds the device time of the call's kernels"""
        q = np.ascontiguousarray(queries, np.uint32).reshape(-1)
        nq = len(q)
        stats = np.zeros((nq, 8), np.uint64)
        lens, span = None, None
        if track:
            if nq and int(q.max()) < db.n:         # (an index beyond the DB is the library's to refuse: nothing is written then)
                lens = db.meta()[0][q].astype(np.int64)
            else:
                lens = np.zeros(nq, np.int64)
            span = np.zeros(max(int(lens.sum()), 1), np.uint32)
        par = BreaksParams(int(anchor), int(edge), int(min_span), int(min_span_percent), float(min_seq_id), int(bool(skip_extended_targets)))
        ptr, n_breaks, ms = C.POINTER(Break)(), C.c_uint64(0), C.c_float(0.0)
        tail = (C.byref(par), _ptr(stats), _ptr(span), C.byref(ptr) if breaks else None, C.byref(n_breaks) if breaks else None, C.byref(ms))
        if gapped is None:
            rc = lib().cdm_pileup_breaks(self.h, db.h, alns.h, _ptr(q), nq, *tail)
        else:
            rc = lib().cdm_pileup_breaks_gapped(self.h, db.h, alns.h, _ptr(q), nq, *_gapped_args(gapped), *tail)
        self.breaks_kernel_ms = float(ms.value)         # (0 behind a refusal of the gapped call: no kernel ran)
        _check(rc)
        out = [stats]
        if track:
            ends = np.cumsum(lens)
            out.append([span[int(e - l):int(e)].copy() for l, e in zip(lens, ends)])
        if breaks:
            n = int(n_breaks.value)
            assert (n == 0) == (not ptr)
            recs = np.empty(n, BREAK_DTYPE)
            if n:
                C.memmove(recs.ctypes.data, ptr, n * C.sizeof(Break))
                lib().cdm_breaks_free(ptr)
            out.append(recs)
        return out[0] if len(out) == 1 else tuple(out)

    def pileup_map(self, db, alns, queries, min_seq_id=0.0, skip_extended_targets=False, records=False):
        """the reads on the listed queries as alignment records (cdm_pileup_map) -> stats[nq, 4] uint64: reads, columns, mismatches,
        primary; with records (stats, recs, mism): the records as an array of MAP_DTYPE in listed query order, then by pos, then in the
        set's order, and their mismatch words (uint32: column | ref << 24 | read << 28).  self.map_kernel_ms holds the device time of
        the call's kernels"""
        q = np.ascontiguousarray(queries, np.uint32).reshape(-1)
        nq = len(q)
        stats = np.zeros((nq, 4), np.uint64)
        par = MapParams(float(min_seq_id), int(bool(skip_extended_targets)))
        ptr, words, n_recs, n_words, ms = C.POINTER(MapRec)(), C.POINTER(C.c_uint32)(), C.c_uint64(0), C.c_uint64(0), C.c_float(0.0)
        _check(lib().cdm_pileup_map(self.h, db.h, alns.h, _ptr(q), nq, C.byref(par), _ptr(stats), C.byref(ptr) if records else None,
                                    C.byref(n_recs) if records else None, C.byref(words) if records else None, C.byref(n_words) if records else None, C.byref(ms)))
        self.map_kernel_ms = float(ms.value)
        if not records:
            return stats
        n, nw = int(n_recs.value), int(n_words.value)
        assert (n == 0) == (not ptr) and (nw == 0) == (not words)
        recs, mism = np.empty(n, MAP_DTYPE), np.empty(nw, np.uint32)
        if n:
            C.memmove(recs.ctypes.data, ptr, n * C.sizeof(MapRec))
        if nw:
            C.memmove(mism.ctypes.data, words, nw * 4)
        lib().cdm_map_free(ptr, words)
        return stats, recs, mism

    def alns_dedup(self, db, alns, queries, min_seq_id=0.0, skip_extended_targets=False, keep=False):
        """the set without the duplicate reads on the listed queries (cdm_alns_dedup) -> (Alns, stats[nq, 4] uint64: counted, kept, removed,
        largest); with keep (Alns, stats, keep): one uint8 per record of `alns`, 1 = the record is in the new set.  self.dedup_kernel_ms
        holds the device time of the call's kernels"""
        q = np.ascontiguousarray(queries, np.uint32).reshape(-1)
        nq = len(q)
        stats = np.zeros((nq, 4), np.uint64)
        flags = np.zeros(alns.count, np.uint8)
        par = DedupParams(float(min_seq_id), int(bool(skip_extended_targets)))
        h, ms = C.c_void_p(), C.c_float(0.0)
        self.dedup_kernel_ms = 0.0
        _check(lib().cdm_alns_dedup(self.h, db.h, alns.h, _ptr(q), nq, C.byref(par), C.byref(h), _ptr(stats), _ptr(flags) if keep else None, C.byref(ms)))
        self.dedup_kernel_ms = float(ms.value)
        out = Alns(self, h, alns.n)
        return (out, stats, flags) if keep else (out, stats)

    def pileup_links(self, db, alns, queries, par=None, links=False):
        """the links between the listed queries from the reads that bridge two of their ends (cdm_pileup_links; par: LinksParams, None =
        LinksParams.default()) -> (stats[nq, 6] uint64: reads, columns, left_ends, right_ends, both_ends, links; totals[5] uint64: end
        records, crowded reads, self pairs, pairs in links, links before min_reads); with links (stats, totals, links): the links at
        min_reads as an array of LINK_DTYPE, ascending by (a, oA, b, oB).  self.links_kernel_ms holds the device time of the call's kernels"""
        q = np.ascontiguousarray(queries, np.uint32).reshape(-1)
        nq = len(q)
        stats, totals = np.zeros((nq, 6), np.uint64), np.zeros(5, np.uint64)
        par = LinksParams.default() if par is None else par
        ptr, n_links, ms = C.POINTER(Link)(), C.c_uint64(0), C.c_float(0.0)
        self.links_kernel_ms = 0.0
        _check(lib().cdm_pileup_links(self.h, db.h, alns.h, _ptr(q), nq, C.byref(par), _ptr(stats), _ptr(totals), C.byref(ptr) if links else None,
                                      C.byref(n_links) if links else None, C.byref(ms)))
        self.links_kernel_ms = float(ms.value)
        if not links:
            return stats, totals
        n = int(n_links.value)
        assert (n == 0) == (not ptr)
        recs = np.empty(n, LINK_DTYPE)
        if n:
            C.memmove(recs.ctypes.data, ptr, n * C.sizeof(Link))
            lib().cdm_link_free(ptr)
        return stats, totals, recs

    def pileup_junctions(self, db, alns, queries, junctions, par=None, counts=False):
        """what the letters say at the junctions (cdm_pileup_junctions; junctions: an array of JUNCTION_DTYPE, ascending by (a, oA, b, oB);
        par: LinksParams, None = LinksParams.default(), min_reads is ignored) -> (res: JUNCTION_RES_DTYPE per junction, letters: uint8
        ASCII ACGTN, the voted fills back to back); with counts (res, letters, counts[letters, 5] uint32: A, C, G, T, N).
        self.junctions_kernel_ms holds the device time of the call's kernels"""
        q = np.ascontiguousarray(queries, np.uint32).reshape(-1)
        j = np.ascontiguousarray(junctions, JUNCTION_DTYPE).reshape(-1)
        res = np.zeros(len(j), JUNCTION_RES_DTYPE)
        par = LinksParams.default() if par is None else par
        lp, cp, ms = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint32)(), C.c_float(0.0)
        self.junctions_kernel_ms = 0.0
        _check(lib().cdm_pileup_junctions(self.h, db.h, alns.h, _ptr(q), len(q), C.byref(par), _ptr(j), len(j), _ptr(res), C.byref(lp), C.byref(cp) if counts else None, C.byref(ms)))
        self.junctions_kernel_ms = float(ms.value)
        n = int(res["fill_len"].sum())
        assert (n == 0) == (not lp) and (not cp or counts)
        letters, cnt = np.empty(n, np.uint8), np.empty((n, 5), np.uint32)
        if n:
            C.memmove(letters.ctypes.data, lp, n)
            if counts:
                C.memmove(cnt.ctypes.data, cp, n * 20)
            lib().cdm_junction_free(lp, cp)
        return (res, letters, cnt) if counts else (res, letters)

    def pileup_gapped(self, db, hits, alns, queries, par=None, records=False):
        """the reads across insertions and deletions (cdm_pileup_gapped): the banded gapped alignment of the hits of the listed queries
        that left no counted record -> stats[nq, 4] uint64: candidates, rescued, gap_letters, too_long; with records (stats, recs, ops,
        words): the rescued as an array of GAP_DTYPE in listed query order, then by pos, then in hit order, their operation words
        (uint32: length << 2 | op) and their mismatch / deletion words (uint32: offset | ref << 24 | read << 28, read 15 = deleted).
        self.gapped_kernel_ms holds the device time of the call's kernels"""
        q = np.ascontiguousarray(queries, np.uint32).reshape(-1)
        nq = len(q)
        stats = np.zeros((nq, 4), np.uint64)
        par = par or GapParams.default()
        ptr, ops, words = C.POINTER(GapRec)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
        n_recs, n_ops, n_words, ms = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_float(0.0)
        ref = (lambda x: C.byref(x)) if records else (lambda x: None)
        _check(lib().cdm_pileup_gapped(self.h, db.h, hits.h, alns.h, _ptr(q), nq, C.byref(par), _ptr(stats), ref(ptr), ref(n_recs), ref(ops), ref(n_ops), ref(words), ref(n_words),
                                       C.byref(ms)))
        self.gapped_kernel_ms = float(ms.value)
        if not records:
            return stats
        n, no, nw = int(n_recs.value), int(n_ops.value), int(n_words.value)
        assert (n == 0) == (not ptr) and (no == 0) == (not ops) and (nw == 0) == (not words)
        recs, o, w = np.empty(n, GAP_DTYPE), np.empty(no, np.uint32), np.empty(nw, np.uint32)
        if n:
            C.memmove(recs.ctypes.data, ptr, n * C.sizeof(GapRec))
        if no:
            C.memmove(o.ctypes.data, ops, no * 4)
        if nw:
            C.memmove(w.ctypes.data, words, nw * 4)
        lib().cdm_gap_free(ptr, ops, words)
        return stats, recs, o, w

    def pileup_indels(self, db, alns, queries, recs, ops, par=None, track=False, sites=False):
        """insertion and deletion sites of the listed queries (cdm_pileup_indels) from the ungapped set and the gapped records and
        operation words pileup_gapped returned for the same queries -> stats[nq, 10] uint64: reads, columns, rescued, insertions,
        deletions, inserted_letters, deleted_letters, places, supported, major; with track also cross at every boundary b = 0 .. len - 1,
        a list of uint32 arrays, one per listed query; with sites also the site records as an array of INDEL_DTYPE and their letters
        (uint8 codes 0..4).  The order of the extras in the returned tuple is track, sites, letters.  self.indels_kernel_ms holds the
        device time of the call's kernels"""
        q = np.ascontiguousarray(queries, np.uint32).reshape(-1)
        nq = len(q)
        stats = np.zeros((nq, 10), np.uint64)
        recs = np.ascontiguousarray(recs, GAP_DTYPE).reshape(-1)
        ops = np.ascontiguousarray(ops, np.uint32).reshape(-1)
        lens, cross = None, None
        if track:
            if nq and int(q.max()) < db.n:         # (an index beyond the DB is the library's to refuse: nothing is written then)
                lens = db.meta()[0][q].astype(np.int64)
            else:
                lens = np.zeros(nq, np.int64)
            cross = np.zeros(max(int(lens.sum()), 1), np.uint32)
        par = par or IndelParams.default()
        ptr, letters, n_sites, n_letters, ms = C.POINTER(IndelSite)(), C.POINTER(C.c_uint8)(), C.c_uint64(0), C.c_uint64(0), C.c_float(0.0)
        ref = (lambda x: C.byref(x)) if sites else (lambda x: None)
        rc = lib().cdm_pileup_indels(self.h, db.h, alns.h, _ptr(q), nq, _ptr(recs) if len(recs) else None, len(recs), _ptr(ops) if len(ops) else None, len(ops), C.byref(par),
                                     _ptr(stats), _ptr(cross), ref(ptr), ref(n_sites), ref(letters), ref(n_letters), C.byref(ms))
        self.indels_kernel_ms = float(ms.value)         # (0 behind a refusal: no kernel ran)
        _check(rc)
        out = [stats]
        if track:
            ends = np.cumsum(lens)
            out.append([cross[int(e - l):int(e)].copy() for l, e in zip(lens, ends)])
        if sites:
            n, nl = int(n_sites.value), int(n_letters.value)
            assert (n == 0) == (not ptr) and (nl == 0) == (not letters)
            got, codes = np.empty(n, INDEL_DTYPE), np.empty(nl, np.uint8)
            if n:
                C.memmove(got.ctypes.data, ptr, n * C.sizeof(IndelSite))
            if nl:
                C.memmove(codes.ctypes.data, letters, nl)
            lib().cdm_indel_free(ptr, letters)
            out += [got, codes]
        return out[0] if len(out) == 1 else tuple(out)

    def extend(self, db, alns, par=None, want_scores=False):
        par = par or AncientParams.default()
        h = C.c_void_p()
        scores = np.full(alns.count, np.nan, np.float64) if want_scores else None
        _check(lib().cdm_extend(self.h, db.h, alns.h, C.byref(par), C.byref(h), _ptr(scores)))
        out = SeqDb(self, h)
        return (out, scores) if want_scores else out


class Comm:
    """cdm_comm: a rank's communicator for the library's own multi-GPU calls (csrc/dist.hip)."""

    def __init__(self, ctx, handle, rank, world, keep=None):
        self.ctx, self.h, self.rank, self.world, self._keep = ctx, handle, rank, world, keep

    def __del__(self):
        if getattr(self, "h", None) and lib is not None:
            lib().cdm_comm_free(self.h)
            self.h = None

    @staticmethod
    def unique_id():
        """rank 0: the 128 bytes every rank's Comm.rccl() needs (ncclGetUniqueId)"""
        b = C.create_string_buffer(128)
        _check(lib().cdm_comm_unique_id(b))
        return b.raw

    @classmethod
    def rccl(cls, ctx, rank, world, unique_id):
        """RCCL, called by the library itself (one device per rank)"""
        h = C.c_void_p()
        _check(lib().cdm_comm_create_rccl(ctx.h, rank, world, C.create_string_buffer(bytes(unique_id), 128), C.byref(h)))
        return cls(ctx, h, rank, world)

    @staticmethod
    def standin_group(world):
        """shared by the ranks (threads) of one test: the in-process stand-in for RCCL's point-to-point calls"""
        lib().cdm_comm_standin_group.restype = C.c_void_p
        lib().cdm_comm_standin_group.argtypes = [C.c_int]
        return lib().cdm_comm_standin_group(world)

    @classmethod
    def standin(cls, ctx, group, rank, world):
        """the RCCL transport's code over the stand-in (several ranks as threads on ONE device)"""
        lib().cdm_comm_create_standin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        h = C.c_void_p()
        _check(lib().cdm_comm_create_standin(ctx.h, group, rank, C.byref(h)))
        return cls(ctx, h, rank, world)

    @classmethod
    def from_transport(cls, ctx, rank, world, t):
        """A transport written in Python (tests: several ranks on ONE device): t.all_gather_host(bytes) -> list of the ranks' bytes;
        t.all_to_all_dev(send_ptr, send_off, recv_ptr, recv_off) and t.all_gather_dev(send_ptr, send_bytes, recv_ptr, recv_off) move
        device memory (byte offsets, world + 1 of them) and return when the data has arrived."""
        def ag_host(user, send, recv, nbytes):
            try:
                parts = t.all_gather_host(C.string_at(send, nbytes))
                for p, b in enumerate(parts):
                    C.memmove(recv + p * nbytes, b, nbytes)
                return 0
            except BaseException as e:      # noqa: BLE001 - an exception must not cross the C frames
                t.error = e
                return -1

        def a2a(user, send, soff, recv, roff, stream):
            try:
                ctx.sync()
                t.all_to_all_dev(send or 0, [int(soff[i]) for i in range(world + 1)], recv or 0, [int(roff[i]) for i in range(world + 1)])
                return 0
            except BaseException as e:      # noqa: BLE001
                t.error = e
                return -1

        def ag_dev(user, send, nbytes, recv, roff, stream):
            try:
                ctx.sync()
                t.all_gather_dev(send or 0, int(nbytes), recv or 0, [int(roff[i]) for i in range(world + 1)])
                return 0
            except BaseException as e:      # noqa: BLE001
                t.error = e
                return -1

        ops = CommOps(None, AG_HOST_FN(ag_host), A2A_DEV_FN(a2a), AG_DEV_FN(ag_dev))
        h = C.c_void_p()
        _check(lib().cdm_comm_create_ops(ctx.h, rank, world, C.byref(ops), C.byref(h)))
        return cls(ctx, h, rank, world, keep=(ops, t))

    def kmermatch(self, db, par=None):
        """kmermatcher over the ranks: this rank's share of the hits (its representatives' rows; self hits elsewhere)"""
        par = par or KmerParams.reads_default()
        h = C.c_void_p()
        _check(lib().cdm_kmermatch_dist(self.ctx.h, self.h, db.h, C.byref(par), C.byref(h)))
        return Hits(self.ctx, h, db.n)

    def allgather_owned(self, db_local):
        h = C.c_void_p()
        _check(lib().cdm_seqdb_allgather_owned(self.ctx.h, self.h, db_local.h, C.byref(h)))
        return SeqDb(self.ctx, h)

    def owned(self, n):
        """bounds[world + 1]: rank r owns the sequences [bounds[r], bounds[r + 1]) of a DB of n sequences (cdm_comm_owned: as this
        communicator's last kmermatch on such a DB cut them - equal shares of the group keys -, equal id ranges before any)"""
        b = np.zeros(lib().cdm_comm_world(self.h) + 1, np.uint64)
        _check(lib().cdm_comm_owned(self.h, int(n), _ptr(b)))
        return b

    def last_path(self):
        """what the last kmermatch over the ranks did (cdm_comm_last_path)"""
        lib().cdm_comm_last_path.argtypes = [C.c_void_p]
        return {0: None, 1: "replicate", 2: "all", 3: "split", 4: "part", 5: "ranges"}[int(lib().cdm_comm_last_path(self.h))]

    def reads_iteration(self, db, kpar=None, rpar=None, apar=None):
        """one iteration of the reads loop over the ranks -> (hits, alns, corrected DB, next DB); the DBs are complete on every rank"""
        kpar, rpar, apar = kpar or KmerParams.reads_default(), rpar or RescoreParams.default(), apar or AncientParams.default()
        hh, ah, ch, nh = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().cdm_reads_iteration_dist(self.ctx.h, self.h, db.h, C.byref(kpar), C.byref(rpar), C.byref(apar), C.byref(hh), C.byref(ah), C.byref(ch), C.byref(nh)))
        return Hits(self.ctx, hh, db.n), Alns(self.ctx, ah, db.n), SeqDb(self.ctx, ch), SeqDb(self.ctx, nh)

    def contig_iteration(self, db, kpar, rpar=None, apar=None, merge_seq_id=0.99):
        """one iteration of the contig loop over the ranks, up to ancient_contig_merge -> (alns, corrected DB, merged DB); the DBs are complete on every rank"""
        rpar, apar = rpar or RescoreParams.default(), apar or AncientParams.default()
        ah, ch, nh = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().cdm_contig_iteration_dist(self.ctx.h, self.h, db.h, C.byref(kpar), C.byref(rpar), C.byref(apar), merge_seq_id, C.byref(ah), C.byref(ch), C.byref(nh)))
        return Alns(self.ctx, ah, db.n), SeqDb(self.ctx, ch), SeqDb(self.ctx, nh)


# ------------------------------------------------------------------------------------------------ text codecs (tests)
def parse_pref_db(keyed, keys):
    """Prefilter DB text (QueryMatcher.h:81-126) -> CSR (offsets, HIT_DTYPE) over the key-sorted sequence index."""
    idx = {int(k): i for i, k in enumerate(keys)}
    off = np.zeros(len(keys) + 1, np.uint64)
    recs = []
    for i, k in enumerate(keys):
        payload = keyed.get(int(k), (b"", 0))[0]
        for line in payload.decode().split("\n"):
            if not line:
                continue
            t, s, d = line.split("\t")
            recs.append((idx[int(t)], int(s), int(d)))
        off[i + 1] = len(recs)
    return off, np.array(recs, HIT_DTYPE) if recs else np.empty(0, HIT_DTYPE)


def hits_to_text(off, rec, keys):
    out = {}
    for i, k in enumerate(keys):
        lines = ["%d\t%d\t%d" % (keys[r["target"]], r["score"], r["diagonal"]) for r in rec[int(off[i]):int(off[i + 1])]]
        out[int(k)] = ("\n".join(lines) + "\n").encode() if lines else b""
    return out


def parse_aln_db(keyed, keys):
    """Alignment DB text (Matcher.cpp:274-404) -> CSR (offsets, ALN_DTYPE).  raw_score is re-derived from the bit score
    the way the reference's consumers do (correction.cpp:222); ident is not in the text (-1)."""
    idx = {int(k): i for i, k in enumerate(keys)}
    off = np.zeros(len(keys) + 1, np.uint64)
    recs = []
    ln2 = float(np.log(2.0))
    lam, logk = float.fromhex("0x1.4478764a1b24ap-1"), float(np.log(float.fromhex("0x1.a1c1e68ea2ab1p-2")))
    for i, k in enumerate(keys):
        payload = keyed.get(int(k), (b"", 0))[0]
        for line in payload.decode().split("\n"):
            if not line:
                continue
            f = line.split("\t")
            raw = int((logk + int(f[1]) * ln2) / lam + 0.5)
            recs.append((idx[int(f[0])], raw, -1, int(f[4]), int(f[5]), int(f[7]), int(f[8]), np.float32(float(f[2]))))
        off[i + 1] = len(recs)
    return off, np.array(recs, ALN_DTYPE) if recs else np.empty(0, ALN_DTYPE)


def fast_seqid_text(seq_id):
    """Util::fastSeqIdToBuffer + the tab that eats the last written char (Util.cpp:278-307, Matcher.cpp:362-363)."""
    s = np.float32(seq_id)
    if s == np.float32(1.0):
        return "1.00"
    out = "0."
    if s < np.float32(0.10):
        out += "0"
    if s < np.float32(0.01):
        out += "0"
    return out + str(int(np.float32(s * np.float32(1000))))


def alns_to_text(off, rec, keys, lens, db_residues):
    """CSR alignments -> alignment DB text as Matcher::resultToBuffer writes it."""
    l = lib()
    out = {}
    for i, k in enumerate(keys):
        lines = []
        for r in rec[int(off[i]):int(off[i + 1])]:
            qs, qe, ds, de = int(r["q_start"]), int(r["q_end"]), int(r["db_start"]), int(r["db_end"])
            aln_len = max(abs(qe - qs), abs(de - ds)) + 1
            sid = np.float32(np.float32(int(r["ident"])) / np.float32(aln_len)) if r["ident"] >= 0 else np.float32(r["seq_id"])
            ev = l.cdm_evalue(float(r["raw_score"]), float(lens[i]), db_residues)
            lines.append("%d\t%d\t%s\t%.3E\t%d\t%d\t%d\t%d\t%d\t%d" % (keys[r["target"]], l.cdm_bit_score(float(r["raw_score"])), fast_seqid_text(sid), ev,
                                                                    qs, qe, lens[i], ds, de, lens[r["target"]]))
        out[int(k)] = ("\n".join(lines) + "\n").encode() if lines else b""
    return out
