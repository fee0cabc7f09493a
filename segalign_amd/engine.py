"""ctypes binding of libsegalign_hip.so with the reference's own entry-point names.

This is plumbing for tests and bench.py: every function forwards 1:1 to the C-ABI of include/segalign_amd.h
(which in turn replaces, symbol by symbol, the engine boundary of gsneha26/SegAlign -- see INTEGRATION.md).
There is NO fallback: if the HIP library is missing or no GPU is present, calls fail loudly.

Reference symbol                       -> here
  g_InitializeInterface(num_gpu)        -> InitializeInterface        (common/seed_filter_interface.cu:49-80)
  g_InitializeProcessor(...)            -> InitializeProcessor        (src/seed_filter.cu:830-897)
  g_SendRefWriteRequest(seq,addr,len)   -> SendRefWriteRequest        (common/seed_filter_interface.cu:82-101)
  GenerateShapePos(shape)               -> GenerateShapePos           (common/ntcoding.cpp:21-37)
  GenerateSeedPosTable(...)             -> GenerateSeedPosTable       (common/seed_pos_table.cu:49-109)
  g_SendQueryWriteRequest(addr,len,buf) -> SendQueryWriteRequest      (src/seed_filter.cu:899-919)
  g_SeedAndFilter(seeds,rev,buf)        -> SeedAndFilter              (src/seed_filter.cu:682-828)
  g_ClearRef / g_ClearQuery / g_ShutdownProcessor
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsegalign_hip.so")

SEG_DTYPE = np.dtype([("ref_start", "<u4"), ("query_start", "<u4"), ("len", "<u4"), ("score", "<i4")])

# every symbol include/segalign_amd.h declares (tests check the library exports all of them)
C_ABI_SYMBOLS = [
    "sa_select_devices", "sa_initialize_interface", "sa_initialize_processor", "sa_shutdown_processor", "sa_send_ref_write_request",
    "sa_clear_ref", "sa_generate_shape_pos", "sa_generate_seed_pos_table", "sa_send_query_write_request",
    "sa_clear_query", "sa_seed_and_filter", "sa_seed_and_filter_range", "sa_free_segments",
    "sa_rm_send_query_write_request", "sa_rm_clear_query", "sa_rm_seed_and_filter", "sa_set_max_hits",
    "sa_get_max_hits", "sa_max_hits_for_mem", "sa_get_last_call_stats", "sa_get_last_call_trace", "sa_set_count_examined",
    "sa_profile_enable", "sa_profile_reset", "sa_profile_num_entries", "sa_profile_get", "sa_profile_busy_ms", "sa_get_ref_len",
    "sa_get_num_index", "sa_get_index_table_size", "sa_copy_ref_codes", "sa_copy_index_table", "sa_copy_pos_table",
    "sa_copy_query_codes", "sa_get_query_len", "sa_device_make_seeds", "sa_version",
    "sa_rm_mask_interval", "sa_rm_coverage_intervals", "sa_free_intervals", "sa_get_filter_mode",
    "sa_seed_interval", "sa_seed_and_filter_chunks", "sa_max_chunks_per_call", "sa_get_chunks_per_call", "sa_extend_hits", "sa_order_hsps",
    "sa_order_hsps_segs", "sa_scan_counts",
    "sa_get_lookup_mode", "sa_get_neighbourhood_entries",
    "sa_get_table_build_info", "sa_copy_neighbourhood_starts", "sa_copy_neighbourhood_records",
    "sa_probe_call", "sa_free_probe_call",
    "sa_copy_image", "sa_get_code_presence", "sa_get_class_scores",
    "sa_seed_calls", "sa_count_call_hits", "sa_count_chunk_hits", "sa_get_wga_chunk", "sa_release_arena", "sa_set_option", "sa_reset_option", "sa_get_option", "sa_option_count", "sa_option_name", "sa_get_audit", "sa_get_forwards",
    "sa_gapped_extend", "sa_free_gapped", "sa_gapped_align", "sa_free_gapped_align", "sa_gapped_align_greedy",
    "sa_chain_hsps", "sa_free_chain", "sa_chain_hsps_all", "sa_free_chain_all",
    "sa_chain_hsps_costs", "sa_chain_hsps_all_costs", "sa_chain_gap_preset",
    "sa_chain_hsps_ovl", "sa_chain_hsps_all_ovl", "sa_trim_chains", "sa_free_trim",
    "sa_fill_chains", "sa_free_fill",
    "sa_stitch_chains", "sa_free_stitch",
    "sa_net_chains", "sa_free_net",
    "sa_net_subset", "sa_free_net_subset",
    "sa_net_classify", "sa_free_net_class",
    "sa_lift_intervals", "sa_free_lift",
    "sa_diff_alignments", "sa_free_diff",
]
IVL_DTYPE = np.dtype([("query_start", "<u4"), ("len", "<u4")])  # struct Segment, repeat_masker_src/graph.h:32-35
STRAND_PLUS, STRAND_MINUS, STRAND_BOTH = 1, 2, 3
PATH_LIST_REGROWN, PATH_DEDUP_FALLBACK, PATH_CHAIN_BUCKET_OVERFLOW, PATH_CHAIN_SLICED, PATH_HEAD_BITS_REGROWN, PATH_GENERAL_FALLBACK = 1, 2, 4, 8, 16, 32


GAPPED_DTYPE = np.dtype([("ref_start", "<u4"), ("ref_end", "<u4"), ("query_start", "<u4"), ("query_end", "<u4"), ("score", "<i4"),
                         ("hsp_index", "<u4"), ("flags", "<u4"), ("cells", "<u4")])  # sa_gapped_alignment
GAPPED_EXTENT_CAP, GAPPED_BAND_CAP, GAPPED_CONTINUED = 1, 2, 4


class GappedParams(C.Structure):
    _fields_ = [("gap_open", C.c_int32), ("gap_extend", C.c_int32), ("ydrop", C.c_int32), ("gappedthresh", C.c_int32),
                ("max_extent", C.c_uint32), ("max_band", C.c_uint32)]


class GappedStats(C.Structure):
    _fields_ = [("anchors", C.c_uint64), ("cells", C.c_uint64), ("extent_capped", C.c_uint64), ("band_capped", C.c_uint64),
                ("returned", C.c_uint64), ("kernel_ms", C.c_double)]


PATH_DTYPE = np.dtype([("op_offset", "<u8"), ("n_left", "<u4"), ("n_right", "<u4"), ("matches", "<u4"), ("mismatches", "<u4"),
                       ("gap_opens", "<u4"), ("gap_bases", "<u4")])  # sa_gapped_path
GAPPED_OP_M, GAPPED_OP_I, GAPPED_OP_D = 0, 1, 2


class GappedAlignStats(C.Structure):
    _fields_ = [("extend", GappedStats), ("trace_ms", C.c_double), ("walk_ms", C.c_double), ("trace_bytes", C.c_uint64),
                ("trace_batches", C.c_uint64)]


class GappedGreedyStats(C.Structure):
    _fields_ = [("align", GappedAlignStats), ("covered", C.c_uint64), ("below_thresh", C.c_uint64), ("skipped", C.c_uint64),
                ("priority_batches", C.c_uint64), ("cover_segments", C.c_uint64), ("cover_ms", C.c_double)]


CHAIN_MEMBER_DTYPE = np.dtype([("hsp_index", "<u4"), ("group", "<u4"), ("f", "<i8")])  # sa_chain_member
CHAIN_NODE_DTYPE = np.dtype([("f", "<i8"), ("pred", "<i4"), ("pad", "<u4")])  # sa_chain_node
CHAIN_RECORD_DTYPE = np.dtype([("group", "<u4"), ("head", "<u4"), ("first_member", "<u4"), ("n_members", "<u4"), ("score", "<i8"),
                               ("joined", "<i4"), ("pad", "<u4")])  # sa_chain_record
CHAIN_ALL_MEMBER_DTYPE = np.dtype([("hsp_index", "<u4"), ("group", "<u4"), ("chain", "<u4"), ("pad", "<u4"), ("f", "<i8")])  # sa_chain_all_member
CHAIN_NONE = 0xFFFFFFFF  # chain_of of a member of a chain dropped by min_score


class ChainParams(C.Structure):
    _fields_ = [("diag_pen", C.c_int32), ("anti_pen", C.c_int32), ("max_gap", C.c_uint32), ("pad", C.c_uint32), ("min_score", C.c_int64)]


CHAIN_GAP_POINTS = 16


class ChainGapCosts(C.Structure):  # sa_chain_gap_costs
    _fields_ = [("n", C.c_uint32), ("pad", C.c_uint32), ("pos", C.c_uint32 * CHAIN_GAP_POINTS), ("q_gap", C.c_int64 * CHAIN_GAP_POINTS),
                ("t_gap", C.c_int64 * CHAIN_GAP_POINTS), ("both_gap", C.c_int64 * CHAIN_GAP_POINTS)]


CHAIN_MAX_OVERLAP = 4096


class ChainOverlap(C.Structure):  # sa_chain_overlap
    _fields_ = [("max_overlap", C.c_uint32), ("reserved", C.c_uint32)]


TRIM_CHAIN_DTYPE = np.dtype([("score", "<i8"), ("trimmed_links", "<u4"), ("bases_cut", "<u4")])  # sa_trim_chain
TRIM_LINK_DTYPE = np.dtype([("o", "<u4"), ("x", "<u4"), ("gap_r", "<u4"), ("gap_q", "<u4")])  # sa_trim_link
TRIM_LINKS = 1


class TrimStats(C.Structure):  # sa_trim_stats
    _fields_ = [("chains", C.c_uint64), ("members", C.c_uint64), ("links", C.c_uint64), ("trimmed_links", C.c_uint64),
                ("cut_members", C.c_uint64), ("bases_cut", C.c_uint64), ("kernel_ms", C.c_double)]


FILL_CHAIN_DTYPE = np.dtype([("score", "<i8"), ("fills", "<u4"), ("fill_bases", "<u4")])  # sa_fill_chain
FILL_LINK_DTYPE = np.dtype([("dt", "<u4"), ("dq", "<u4"), ("flags", "<u4"), ("n_hsps", "<u4"), ("n_fill", "<u4"), ("pad", "<u4"),
                            ("cells", "<u8")])  # sa_fill_link
FILL_HSP_DTYPE = np.dtype([("ref_start", "<u4"), ("query_start", "<u4"), ("len", "<u4"), ("score", "<i4"), ("link", "<u4"),
                           ("pad", "<u4")])  # sa_fill_hsp
FILL_LINKS, FILL_HSPS = 1, 2
FILL_LONG, FILL_LARGE, FILL_CROWDED = 1, 2, 4
FILL_NONE = 0xFFFFFFFF  # origin of an entry that is a fill


class FillParams(C.Structure):  # sa_fill_params
    _fields_ = [("thresh", C.c_int32), ("xdrop", C.c_int32), ("max_side", C.c_uint32), ("max_link_hsps", C.c_uint32),
                ("max_cells", C.c_uint64), ("min_fill", C.c_int64)]


class FillStats(C.Structure):  # sa_fill_stats
    _fields_ = [("links", C.c_uint64), ("swept", C.c_uint64), ("long_links", C.c_uint64), ("large_links", C.c_uint64),
                ("crowded_links", C.c_uint64), ("cells", C.c_uint64), ("hsps", C.c_uint64), ("fills", C.c_uint64),
                ("filled_links", C.c_uint64), ("count_ms", C.c_double), ("emit_ms", C.c_double), ("chain_ms", C.c_double)]


class ChainStats(C.Structure):
    _fields_ = [("hsps", C.c_uint64), ("groups", C.c_uint64), ("chains", C.c_uint64), ("members", C.c_uint64), ("pair_evals", C.c_uint64),
                ("tile_steps", C.c_uint64), ("kernel_ms", C.c_double)]


class ChainAllStats(C.Structure):
    _fields_ = [("chain", ChainStats), ("chains_all", C.c_uint64), ("joined", C.c_uint64), ("peel_rounds", C.c_uint64), ("peel_ms", C.c_double)]


STITCH_RECORD_DTYPE = np.dtype([("chain", "<u4"), ("first_member", "<u4"), ("n_members", "<u4"), ("flags", "<u4"), ("ref_start", "<u4"),
                                ("ref_end", "<u4"), ("query_start", "<u4"), ("query_end", "<u4"), ("score", "<i8"), ("op_offset", "<u8"),
                                ("n_ops", "<u4"), ("matches", "<u4"), ("mismatches", "<u4"), ("gap_opens", "<u4"), ("gap_bases", "<u4"),
                                ("pad", "<u4")])  # sa_stitch_record
STITCH_LINK_DTYPE = np.dtype([("chain", "<u4"), ("member", "<u4"), ("dt", "<u4"), ("dq", "<u4"), ("score", "<i4"), ("flags", "<u4"),
                              ("cells", "<u8")])  # sa_stitch_link
STITCH_LONG, STITCH_DEAD, STITCH_LOW = 1, 2, 4
STITCH_NEVER = -(1 << 31)  # min_link_score that breaks no link


class StitchParams(C.Structure):
    _fields_ = [("gap_open", C.c_int32), ("gap_extend", C.c_int32), ("max_link", C.c_uint32), ("min_link_score", C.c_int32)]


class StitchStats(C.Structure):
    _fields_ = [("links", C.c_uint64), ("swept", C.c_uint64), ("long_links", C.c_uint64), ("dead_links", C.c_uint64),
                ("low_links", C.c_uint64), ("cells", C.c_uint64), ("records", C.c_uint64), ("member_ms", C.c_double),
                ("sweep_ms", C.c_double), ("walk_ms", C.c_double), ("trace_bytes", C.c_uint64), ("batches", C.c_uint64)]


DIFF_SPAN_DTYPE = np.dtype([("ref_start", "<u4"), ("query_start", "<u4"), ("op_offset", "<u8"), ("n_ops", "<u4"), ("pad", "<u4")])  # sa_diff_span
DIFF_EVENT_DTYPE = np.dtype([("span", "<u4"), ("ref_pos", "<u4"), ("query_pos", "<u4"), ("len", "<u4"), ("column", "<u4"), ("kind", "u1"),
                             ("tcode", "u1"), ("qcode", "u1"), ("pad", "u1")])  # sa_diff_event
DIFF_SUMMARY_DTYPE = np.dtype([("first_event", "<u8"), ("n_events", "<u4"), ("columns", "<u4"), ("matches", "<u4"), ("transitions", "<u4"),
                               ("transversions", "<u4"), ("others", "<u4"), ("ins_runs", "<u4"), ("ins_bases", "<u4"), ("del_runs", "<u4"),
                               ("del_bases", "<u4")])  # sa_diff_summary
DIFF_PER_BASE, DIFF_NO_EVENTS = 1, 2
DIFF_SUB, DIFF_OTHER, DIFF_INS, DIFF_DEL = 0, 1, 2, 3
DIFF_NO_CODE = 8


class DiffParams(C.Structure):  # sa_diff_params
    _fields_ = [("flags", C.c_uint32), ("chunk", C.c_uint32)]


class DiffStats(C.Structure):  # sa_diff_stats
    _fields_ = [("spans", C.c_uint64), ("ops", C.c_uint64), ("columns", C.c_uint64), ("work_items", C.c_uint64), ("events", C.c_uint64),
                ("pairs", C.c_uint64 * 64), ("prep_ms", C.c_float), ("count_ms", C.c_float), ("emit_ms", C.c_float), ("pad", C.c_float)]


NET_FILL_DTYPE = np.dtype([("group", "<u4"), ("chain", "<u4"), ("parent", "<i4"), ("depth", "<u4"), ("start", "<u4"), ("end", "<u4"),
                           ("ali", "<u4"), ("first_block", "<u4"), ("n_blocks", "<u4"), ("pad", "<u4"), ("score", "<i8")])  # sa_net_fill


class NetParams(C.Structure):
    _fields_ = [("min_space", C.c_uint32), ("min_fill", C.c_uint32)]


class NetStats(C.Structure):
    _fields_ = [("chains", C.c_uint64), ("blocks", C.c_uint64), ("groups", C.c_uint64), ("fills", C.c_uint64), ("spaces", C.c_uint64),
                ("rounds", C.c_uint64), ("max_depth", C.c_uint64), ("filled", C.c_uint64), ("prep_ms", C.c_float), ("net_ms", C.c_float)]


SUBSET_CHAIN_DTYPE = np.dtype([("fill", "<u4"), ("chain", "<u4"), ("group", "<u4"), ("run", "<u4"), ("first_member", "<u4"),
                               ("n_members", "<u4"), ("ref_start", "<u4"), ("ref_end", "<u4"), ("query_start", "<u4"), ("query_end", "<u4"),
                               ("score", "<i8"), ("clipped", "<u4"), ("pad", "<u4")])  # sa_subset_chain
SUBSET_SPLIT = 1


class SubsetStats(C.Structure):
    _fields_ = [("fills", C.c_uint64), ("runs", C.c_uint64), ("members", C.c_uint64), ("cut_members", C.c_uint64),
                ("bases_rescored", C.c_uint64), ("splits", C.c_uint64), ("subset_ms", C.c_double)]


NET_CLASS_DTYPE = np.dtype([("ostart", "<u4"), ("oend", "<u4"), ("oover", "<u4"), ("ofar", "<u4"), ("odup", "<u4"), ("ogroup", "<u4"),
                            ("type", "u1"), ("strand", "u1"), ("keep", "u1"), ("pad", "u1"), ("pad2", "<u4")])  # sa_net_class
NETCLASS_FILTER = 1
NETCLASS_TOP, NETCLASS_SYN, NETCLASS_INV, NETCLASS_NONSYN = 0, 1, 2, 3
NETCLASS_NAMES = ("top", "syn", "inv", "nonSyn")
NETCLASS_THRESHOLDS = ("min_score", "min_top_score", "min_size", "min_ali", "max_far")


class NetClassParams(C.Structure):
    _fields_ = [("min_score", C.c_int64), ("min_top_score", C.c_int64), ("min_size", C.c_uint32), ("min_ali", C.c_uint32),
                ("max_far", C.c_uint32), ("pad", C.c_uint32)]


class NetClassStats(C.Structure):
    _fields_ = [("fills", C.c_uint64), ("blocks", C.c_uint64), ("events", C.c_uint64), ("ogroups", C.c_uint64), ("n_type", C.c_uint64 * 4),
                ("kept", C.c_uint64), ("dup_bases", C.c_uint64), ("class_ms", C.c_float), ("pad", C.c_uint32)]


LIFT_RECORD_DTYPE = np.dtype([("status", "<u4"), ("n_touch", "<u4"), ("n_qualify", "<u4"), ("first_hit", "<u4"), ("chain", "<u4"),
                              ("ogroup", "<u4"), ("ostart", "<u4"), ("oend", "<u4"), ("mapped", "<u4"), ("first_block", "<u4"),
                              ("n_blocks", "<u4"), ("strand", "u1"), ("pad", "u1", (3,))])  # sa_lift_record
LIFT_HIT_DTYPE = np.dtype([("interval", "<u4"), ("chain", "<u4"), ("ostart", "<u4"), ("oend", "<u4"), ("mapped", "<u4"),
                           ("first_block", "<u4"), ("n_blocks", "<u4"), ("out_block", "<u4")])  # sa_lift_hit
LIFT_BLOCK_DTYPE = np.dtype([("start", "<u4"), ("end", "<u4"), ("ostart", "<u4"), ("oend", "<u4")])  # sa_lift_block
LIFT_MULTIPLE, LIFT_BLOCKS = 1, 2
LIFT_UNMAPPED, LIFT_PARTIAL, LIFT_MAPPED, LIFT_DUPLICATED = 0, 1, 2, 3
LIFT_NAMES = ("unmapped", "partial", "mapped", "duplicated")
LIFT_NONE = 0xFFFFFFFF


class LiftParams(C.Structure):
    _fields_ = [("num", C.c_uint32), ("den", C.c_uint32)]


class LiftStats(C.Structure):
    _fields_ = [("intervals", C.c_uint64), ("chains", C.c_uint64), ("blocks", C.c_uint64), ("candidates", C.c_uint64),
                ("touches", C.c_uint64), ("n_status", C.c_uint64 * 4), ("hits", C.c_uint64), ("out_blocks", C.c_uint64),
                ("prep_ms", C.c_float), ("lift_ms", C.c_float)]


class CallStats(C.Structure):
    _fields_ = [("num_seeds", C.c_uint64), ("num_hits", C.c_uint64), ("num_survivors", C.c_uint64),
                ("num_anchors", C.c_uint64), ("num_examined", C.c_uint64), ("num_examined_filter", C.c_uint64),
                ("num_candidates", C.c_uint64), ("num_entropy", C.c_uint64), ("num_iter", C.c_uint32),
                ("device", C.c_int), ("lookup_path", C.c_int), ("path_flags", C.c_uint32), ("num_forwarded", C.c_uint64)]


class CallTrace(C.Structure):  # sa_call_trace
    _fields_ = [("segments", C.c_uint32), ("batches", C.c_uint32), ("reruns", C.c_uint32), ("rerun_first_batch", C.c_int32),
                ("rerun_last_batch", C.c_int32), ("overflowed", C.c_uint32), ("slices", C.c_uint32), ("spec_tried", C.c_uint32),
                ("spec_refused", C.c_uint32), ("second_copy", C.c_uint32), ("route", C.c_uint32), ("l2_max", C.c_uint32)]


TRACE_OVER_SURVIVORS, TRACE_OVER_CANDIDATES, TRACE_OVER_ENTROPY, TRACE_OVER_SECOND_LEVEL = 1, 2, 4, 8
ROUTE_NONE, ROUTE_SPEC_CHAIN, ROUTE_CHAIN_AFTER_SYNC, ROUTE_LIBRARY_SORTS, ROUTE_RAW, ROUTE_RM_SORT, ROUTE_RM_COVERAGE = range(7)


class TableBuildInfo(C.Structure):  # sa_table_build_info
    _fields_ = [("build", C.c_int32), ("unsorted_partitions", C.c_uint32), ("nbr_fill", C.c_int32), ("left_skip", C.c_uint32)]


# sa_probe_call (test entry, DESIGN.md 4.4'): the front of a table-direct call and what it wrote
PROBE_OK, PROBE_NO_TABLE, PROBE_NOT_ELIGIBLE, PROBE_EMPTY_RANGE, PROBE_TOO_MANY_CHUNKS = 0, 1, 2, 3, 4
PROBE_MAX_ITER, PROBE_PLAN_OVERFLOW, PROBE_VALID = 8, 0xFFFFFFFF, 1 << 63
PROBE_PLAN_DTYPE = np.dtype([("hit_base", "<u8"), ("num_hits", "<u8"), ("upto", "<u8", (PROBE_MAX_ITER,)), ("num_valid", "<u4"), ("m_lo", "<u4"),
                             ("m_hi", "<u4"), ("n_iter", "<u4")])  # sa_probe_plan
PROBE_BOUND_DTYPE = np.dtype([("hits", "<u8"), ("nonempty", "<u4"), ("valid", "<u4")])  # sa_probe_bound
PROBE_REC_DTYPE = np.dtype([("prefix", "<u4"), ("qpos", "<u4"), ("off", "<u8")])  # sa_probe_record


class ProbeResult(C.Structure):  # sa_probe_result
    _fields_ = [("status", C.c_int32), ("slot", C.c_int32), ("ret", C.c_uint32), ("words", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32),
                ("chunk", C.c_uint32), ("num_chunks", C.c_uint32), ("hits", C.c_uint64), ("num_records", C.c_uint32), ("lookup_mode", C.c_uint32),
                ("regrown", C.c_uint32), ("num_seg_end", C.c_uint32), ("head_words_before", C.c_uint64), ("head_words_after", C.c_uint64),
                ("num_head_words", C.c_uint64), ("num_td_chunk", C.c_uint64), ("plans", C.c_void_p), ("bounds", C.c_void_p), ("records", C.c_void_p),
                ("head_bits", C.c_void_p), ("td_chunk", C.c_void_p), ("seg_end", C.c_void_p), ("t_off", C.c_void_p), ("t_cnt", C.c_void_p)]


# sa_copy_image (test entry, DESIGN.md 4.1'): the images the send entries build from a block, whole spans
IMAGES = ("ref", "ref8", "ref_rc", "query", "query_rc", "query4", "query4_rc", "ref4", "ref4_rc", "ref2", "query2", "query2_rc", "refq2",
          "refq2_rc")  # SA_IMAGE_*: the index is the id


class ImageInfo(C.Structure):  # sa_image_info
    _fields_ = [("bytes", C.c_uint64), ("stride", C.c_uint64), ("origin", C.c_uint64), ("len", C.c_uint32), ("copies", C.c_uint32)]


TABLE_BUILD_NONE, TABLE_BUILD_TWO_LEVEL, TABLE_BUILD_THREE_LEVEL, TABLE_BUILD_ATOMIC, TABLE_BUILD_ATOMIC_GAVE_UP = 0, 1, 2, 3, 4
NBR_FILL_NONE, NBR_FILL_ALIAS, NBR_FILL_POSITIONS, NBR_FILL_CTX_ONE_STAGE, NBR_FILL_CTX_DENSE, NBR_FILL_CTX_SPARSE = 0, 1, 2, 3, 4, 5
CTX_DTYPE = np.dtype([("pos", "<u4"), ("w", "<u4", (7,))])  # CtxRec: a neighbourhood entry with its target context

_lib = None


def lib():
    """Load the HIP library.  Raises if it has not been built -- there is no CPU path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libsegalign_hip.so is missing (%s). Build it with `python -m segalign_amd.build` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.sa_initialize_interface.restype = C.c_int
    L.sa_initialize_interface.argtypes = [C.c_int]
    L.sa_select_devices.argtypes = [C.POINTER(C.c_int), C.c_int]
    L.sa_initialize_processor.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.sa_send_ref_write_request.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32]
    L.sa_generate_shape_pos.restype = C.c_int
    L.sa_generate_shape_pos.argtypes = [C.c_char_p]
    L.sa_generate_seed_pos_table.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int, C.c_int]
    L.sa_send_query_write_request.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32]
    L.sa_clear_query.argtypes = [C.c_uint32]
    L.sa_seed_and_filter.restype = C.c_size_t
    L.sa_seed_and_filter.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
    L.sa_seed_and_filter_range.restype = C.c_size_t
    L.sa_seed_and_filter_range.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
    L.sa_free_segments.argtypes = [C.c_void_p]
    L.sa_seed_and_filter_chunks.restype = C.c_size_t
    L.sa_seed_and_filter_chunks.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.sa_seed_interval.restype = C.c_size_t
    L.sa_seed_interval.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_void_p),
                                   C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(CallStats)]
    L.sa_rm_seed_and_filter.restype = C.c_size_t
    L.sa_rm_seed_and_filter.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.sa_rm_mask_interval.restype = C.c_size_t
    L.sa_rm_mask_interval.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_void_p),
                                      C.c_void_p]
    L.sa_rm_coverage_intervals.restype = C.c_size_t
    L.sa_rm_coverage_intervals.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.sa_free_intervals.argtypes = [C.c_void_p]
    L.sa_set_max_hits.argtypes = [C.c_int64]
    L.sa_get_max_hits.restype = C.c_int64
    L.sa_max_hits_for_mem.restype = C.c_int
    L.sa_max_hits_for_mem.argtypes = [C.c_uint64]
    L.sa_get_last_call_stats.argtypes = [C.POINTER(CallStats)]
    L.sa_get_last_call_trace.argtypes = [C.POINTER(CallTrace)]
    L.sa_set_count_examined.argtypes = [C.c_int]
    L.sa_profile_enable.argtypes = [C.c_int]
    L.sa_profile_num_entries.restype = C.c_int
    L.sa_profile_get.restype = C.c_int
    L.sa_profile_get.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.sa_profile_busy_ms.restype = C.c_double
    L.sa_profile_busy_ms.argtypes = [C.c_char_p]
    for f in ("sa_get_ref_len", "sa_get_num_index", "sa_get_index_table_size"):
        getattr(L, f).restype = C.c_uint32
    L.sa_get_query_len.restype = C.c_uint32
    L.sa_get_query_len.argtypes = [C.c_uint32]
    L.sa_copy_ref_codes.argtypes = [C.c_int, C.c_void_p]
    L.sa_copy_index_table.argtypes = [C.c_int, C.c_void_p]
    L.sa_copy_pos_table.argtypes = [C.c_int, C.c_void_p]
    L.sa_copy_query_codes.argtypes = [C.c_int, C.c_uint32, C.c_int, C.c_void_p]
    L.sa_device_make_seeds.restype = C.c_size_t
    L.sa_device_make_seeds.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, C.c_size_t]
    L.sa_order_hsps.restype = C.c_size_t
    L.sa_order_hsps.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.sa_order_hsps_segs.restype = C.c_size_t
    L.sa_order_hsps_segs.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int,
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_int)]
    L.sa_scan_counts.restype = C.c_int
    L.sa_scan_counts.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    L.sa_extend_hits.restype = C.c_size_t
    L.sa_extend_hits.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
    L.sa_get_neighbourhood_entries.restype = C.c_uint64
    L.sa_get_table_build_info.restype = C.c_int
    L.sa_get_table_build_info.argtypes = [C.POINTER(TableBuildInfo)]
    L.sa_copy_neighbourhood_starts.restype = C.c_int
    L.sa_copy_neighbourhood_starts.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
    L.sa_copy_neighbourhood_records.restype = C.c_int
    L.sa_copy_neighbourhood_records.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
    L.sa_probe_call.restype = C.c_int
    L.sa_probe_call.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.POINTER(ProbeResult)]
    L.sa_free_probe_call.argtypes = [C.POINTER(ProbeResult)]
    L.sa_copy_image.restype = C.c_int
    L.sa_copy_image.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(ImageInfo)]
    L.sa_get_code_presence.restype = C.c_int
    L.sa_get_code_presence.argtypes = [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.sa_get_class_scores.restype = C.c_int
    L.sa_get_class_scores.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_int32)]
    L.sa_version.restype = C.c_char_p
    L.sa_seed_calls.restype = C.c_size_t
    L.sa_seed_calls.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(CallStats)]
    L.sa_count_call_hits.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_void_p]
    L.sa_count_chunk_hits.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    L.sa_get_wga_chunk.restype = C.c_uint32
    L.sa_set_option.restype = C.c_int
    L.sa_set_option.argtypes = [C.c_char_p, C.c_int64]
    L.sa_reset_option.restype = C.c_int
    L.sa_reset_option.argtypes = [C.c_char_p]
    L.sa_get_option.restype = C.c_int64
    L.sa_get_option.argtypes = [C.c_char_p]
    L.sa_option_count.restype = C.c_int
    L.sa_option_name.restype = C.c_char_p
    L.sa_option_name.argtypes = [C.c_int, C.POINTER(C.c_int)]
    L.sa_get_audit.restype = C.c_size_t
    L.sa_get_audit.argtypes = [C.c_void_p, C.c_size_t]
    L.sa_get_forwards.restype = C.c_size_t
    L.sa_get_forwards.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.sa_gapped_extend.restype = C.c_size_t
    L.sa_gapped_extend.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(GappedParams), C.c_int, C.POINTER(C.c_void_p),
                                   C.POINTER(GappedStats)]
    L.sa_free_gapped.argtypes = [C.c_void_p]
    L.sa_gapped_align.restype = C.c_size_t
    L.sa_gapped_align.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(GappedParams), C.c_int, C.POINTER(C.c_void_p),
                                  C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(GappedAlignStats)]
    L.sa_free_gapped_align.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.sa_gapped_align_greedy.restype = C.c_size_t
    L.sa_gapped_align_greedy.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(GappedParams), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(GappedGreedyStats)]
    L.sa_chain_hsps.restype = C.c_size_t
    L.sa_chain_hsps.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(ChainParams), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                C.POINTER(ChainStats)]
    L.sa_free_chain.argtypes = [C.c_void_p, C.c_void_p]
    L.sa_chain_hsps_all.restype = C.c_size_t
    L.sa_chain_hsps_all.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(ChainParams), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                    C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(ChainAllStats)]
    L.sa_free_chain_all.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sa_chain_hsps_costs.restype = C.c_size_t
    L.sa_chain_hsps_costs.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(ChainParams), C.POINTER(ChainGapCosts),
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(ChainStats)]
    L.sa_chain_hsps_all_costs.restype = C.c_size_t
    L.sa_chain_hsps_all_costs.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(ChainParams), C.POINTER(ChainGapCosts),
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_void_p), C.POINTER(ChainAllStats)]
    L.sa_chain_hsps_ovl.restype = C.c_size_t
    L.sa_chain_hsps_ovl.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(ChainParams), C.POINTER(ChainGapCosts),
                                    C.POINTER(ChainOverlap), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(ChainStats)]
    L.sa_chain_hsps_all_ovl.restype = C.c_size_t
    L.sa_chain_hsps_all_ovl.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(ChainParams), C.POINTER(ChainGapCosts),
                                        C.POINTER(ChainOverlap), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(ChainAllStats)]
    L.sa_trim_chains.restype = C.c_size_t
    L.sa_trim_chains.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(ChainParams),
                                 C.POINTER(ChainGapCosts), C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_size_t), C.POINTER(TrimStats)]
    L.sa_free_trim.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.sa_fill_chains.restype = C.c_size_t
    L.sa_fill_chains.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(ChainParams),
                                 C.POINTER(ChainGapCosts), C.POINTER(FillParams), C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                 C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(FillStats)]
    L.sa_free_fill.argtypes = [C.c_void_p] * 6
    L.sa_chain_gap_preset.restype = C.c_int
    L.sa_chain_gap_preset.argtypes = [C.c_char_p, C.POINTER(ChainGapCosts)]
    L.sa_stitch_chains.restype = C.c_size_t
    L.sa_stitch_chains.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(StitchParams),
                                   C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                   C.POINTER(C.c_size_t), C.POINTER(StitchStats)]
    L.sa_free_stitch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.sa_diff_alignments.restype = C.c_size_t
    L.sa_diff_alignments.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(DiffParams),
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(DiffStats)]
    L.sa_free_diff.argtypes = [C.c_void_p, C.c_void_p]
    L.sa_net_chains.restype = C.c_size_t
    L.sa_net_chains.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(NetParams),
                                C.POINTER(C.c_void_p), C.POINTER(NetStats)]
    L.sa_free_net.argtypes = [C.c_void_p]
    L.sa_net_subset.restype = C.c_size_t
    L.sa_net_subset.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int,
                                C.c_uint32, C.POINTER(ChainParams), C.POINTER(ChainGapCosts), C.c_uint32, C.POINTER(C.c_void_p),
                                C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(SubsetStats)]
    L.sa_free_net_subset.argtypes = [C.c_void_p, C.c_void_p]
    L.sa_net_classify.restype = C.c_size_t
    L.sa_net_classify.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                  C.c_size_t, C.POINTER(NetClassParams), C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(NetClassStats)]
    L.sa_free_net_class.argtypes = [C.c_void_p]
    L.sa_lift_intervals.restype = C.c_size_t
    L.sa_lift_intervals.argtypes = [C.c_void_p] * 8 + [C.c_size_t] + [C.c_void_p] * 3 + [C.c_size_t, C.POINTER(LiftParams), C.c_uint32,
                                                                                        C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                                                        C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                                                                        C.POINTER(C.c_size_t), C.POINTER(LiftStats)]
    L.sa_free_lift.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    _lib = L
    return L


# ---- the reference surface --------------------------------------------------------------------------------------
def select_devices(ids):
    """One process per GPU: make the next InitializeInterface use exactly these HIP device ordinals."""
    arr = (C.c_int * len(ids))(*ids)
    lib().sa_select_devices(arr, len(ids))


def InitializeInterface(num_gpu=-1):
    return lib().sa_initialize_interface(num_gpu)


def InitializeProcessor(transition, wga_chunk, seed_size, sub_mat, xdrop, hspthresh, noentropy):
    m = np.ascontiguousarray(sub_mat, dtype=np.int32)
    assert m.size == 64
    lib().sa_initialize_processor(int(bool(transition)), wga_chunk, seed_size, m.ctypes.data, xdrop, hspthresh,
                                  int(bool(noentropy)))


def ShutdownProcessor():
    lib().sa_shutdown_processor()


def _as_u8(buf):
    """ASCII host buffer -> contiguous uint8 ndarray (kept alive by the caller for the duration of the call)."""
    if isinstance(buf, np.ndarray):
        return np.ascontiguousarray(buf, dtype=np.uint8)
    return np.frombuffer(bytes(buf), dtype=np.uint8)


def SendRefWriteRequest(seq, addr, length):
    a = _as_u8(seq)
    lib().sa_send_ref_write_request(a.ctypes.data, addr, length)
    return a


def ClearRef():
    lib().sa_clear_ref()


def GenerateShapePos(shape):
    return lib().sa_generate_shape_pos(shape.encode())


def GenerateSeedPosTable(ref_str, start_addr, ref_length, step, shape_size, kmer_size):
    a = _as_u8(ref_str)
    lib().sa_generate_seed_pos_table(a.ctypes.data, start_addr, ref_length, step, shape_size, kmer_size)


def SendQueryWriteRequest(query_buffer, addr, length, buffer):
    a = _as_u8(query_buffer)
    lib().sa_send_query_write_request(a.ctypes.data, addr, length, buffer)


def ClearQuery(buffer):
    lib().sa_clear_query(buffer)


def _take(n, out):
    if n == 0 or not out.value:
        return np.zeros(0, dtype=SEG_DTYPE)
    buf = (C.c_char * (n * SEG_DTYPE.itemsize)).from_address(out.value)
    segs = np.frombuffer(buf, dtype=SEG_DTYPE).copy()
    lib().sa_free_segments(out)
    return segs


def SeedAndFilter(seed_offset_vector, rev, buffer):
    """-> structured array; element 0 is the header {len = #anchors, score = #hits} (seed_filter.cu:806-809)."""
    s = np.ascontiguousarray(seed_offset_vector, dtype=np.uint64)
    out = C.c_void_p()
    n = lib().sa_seed_and_filter(s.ctypes.data, s.size, int(bool(rev)), buffer, C.byref(out))
    return _take(n, out)


def SeedAndFilterRange(start, end, rev, buffer):
    """Additive entry: device-side seeding of query positions [start,end). Empty array when the
    chunk holds no valid seed (the reference would not call the engine then, seeder.cpp:76)."""
    out = C.c_void_p()
    n = lib().sa_seed_and_filter_range(start, end, int(bool(rev)), buffer, C.byref(out))
    return _take(n, out)


def SeedAndFilterChunks(start, end, rev, buffer):
    """Up to sa_max_chunks_per_call() consecutive chunks of one strand in one pass; returns one vector per chunk, each
    identical to SeedAndFilterRange of that chunk (empty array for a chunk without seeds)."""
    k = lib().sa_max_chunks_per_call()
    outs = (C.c_void_p * k)()
    counts = (C.c_size_t * k)()
    lib().sa_seed_and_filter_chunks(start, end, int(bool(rev)), buffer, outs, counts)
    res = []
    for c in range(k):
        res.append(_take(counts[c], C.c_void_p(outs[c])) if outs[c] else np.zeros(0, dtype=SEG_DTYPE))
    return res


class CallDesc(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("rev", C.c_int)]


class CallResult(C.Structure):
    _fields_ = [("hsps", C.c_void_p), ("num_hsps", C.c_size_t), ("num_hits", C.c_uint64), ("device", C.c_int32), ("reserved", C.c_int32)]


def CountCallHits(calls, buffer=0, threads=4, per_chunk=False):
    """Seed hits of every call [(start, end, rev), ...], lookup only (no filtering, no extension): the weights a multi-GPU host
    deals the calls of a pass by.  per_chunk: the hits of every wga_chunk piece of every call instead, concatenated."""
    n = len(calls)
    descs = (CallDesc * max(n, 1))(*[CallDesc(int(a), int(b), int(bool(r))) for (a, b, r) in calls])
    hits = (C.c_uint64 * max(n, 1))()
    if not per_chunk:
        lib().sa_count_call_hits(descs, n, buffer, threads, hits)
        return [int(hits[i]) for i in range(n)]
    k = lib().sa_max_chunks_per_call()
    ch = (C.c_uint64 * max(n * k, 1))()
    lib().sa_count_chunk_hits(descs, n, buffer, threads, hits, ch)
    chunk = lib().sa_get_wga_chunk()
    out = []
    for i, (a, b, r) in enumerate(calls):
        kk = (int(b) - int(a) + chunk - 1) // chunk if b > a else 0
        out.extend(int(ch[i * k + c]) for c in range(kk))
    return out


def ReleaseArena():
    lib().sa_release_arena()


def SeedCalls(calls, buffer=0, threads=4, hits_out=None, devices_out=None):
    """calls: [(start, end, rev), ...], each up to sa_max_chunks_per_call() chunks of one strand; `threads` of them in flight on
    the engine's worker pool.  -> ([HSP array per call (chunks concatenated, headers removed)], summed stats dict).
    hits_out: a list that receives the seed hits of every call (sa_call_result.num_hits)."""
    n = len(calls)
    descs = (CallDesc * max(n, 1))(*[CallDesc(int(a), int(b), int(bool(r))) for (a, b, r) in calls])
    res = (CallResult * max(n, 1))()
    st = CallStats()
    lib().sa_seed_calls(descs, n, buffer, threads, res, C.byref(st))
    outs = []
    for i in range(n):
        if res[i].num_hsps:
            buf = (C.c_char * (res[i].num_hsps * SEG_DTYPE.itemsize)).from_address(res[i].hsps)
            outs.append(np.frombuffer(buf, dtype=SEG_DTYPE).copy())
        else:
            outs.append(np.zeros(0, dtype=SEG_DTYPE))
        lib().sa_free_segments(res[i].hsps)
    if hits_out is not None:
        hits_out.extend(int(res[i].num_hits) for i in range(n))
    if devices_out is not None:
        devices_out.extend(int(res[i].device) for i in range(n))
    return outs, {k: getattr(st, k) for k, _ in CallStats._fields_}


def OrderHsps(records, rm=False, path=1):
    """The ordering stage alone on `records` (SEG_DTYPE) as one dedup scope: sort -> adjacent-pair unique -> sort (sa_order_hsps)."""
    h = np.ascontiguousarray(records, dtype=SEG_DTYPE)
    out = C.c_void_p()
    n = lib().sa_order_hsps(h.ctypes.data if h.size else None, h.size, int(bool(rm)), int(path), C.byref(out))
    if not out.value:
        return np.zeros(0, dtype=SEG_DTYPE)
    res = np.frombuffer((C.c_char * (n * SEG_DTYPE.itemsize)).from_address(out.value), dtype=SEG_DTYPE).copy() if n else np.zeros(0, dtype=SEG_DTYPE)
    lib().sa_free_segments(out)
    return res


def OrderHspsSegs(records, seg, nsegs, rm=False, path=1, threads=0, seg_max=0, count_on_device=False):
    """The ordering stage on records of `nsegs` dedup scopes (seg[i] < nsegs) the way a call runs it (sa_order_hsps_segs; test entry).
    -> (records, the segment of each, records kept per segment, refused).  A refused path-0 call returns no records."""
    h = np.ascontiguousarray(records, dtype=SEG_DTYPE)
    sg = np.ascontiguousarray(seg, dtype=np.uint32)
    assert sg.shape == h.shape
    counts = np.zeros(int(nsegs), dtype=np.uint32)
    out, oseg, refused = C.c_void_p(), C.c_void_p(), C.c_int(0)
    n = lib().sa_order_hsps_segs(h.ctypes.data if h.size else None, sg.ctypes.data if sg.size else None, h.size, int(nsegs), int(bool(rm)),
                                 int(path), int(threads), int(seg_max), int(bool(count_on_device)), C.byref(out), C.byref(oseg),
                                 counts.ctypes.data if counts.size else None, C.byref(refused))
    res, rseg = np.zeros(0, dtype=SEG_DTYPE), np.zeros(0, dtype=np.uint32)
    if out.value and n:
        res = np.frombuffer((C.c_char * (n * SEG_DTYPE.itemsize)).from_address(out.value), dtype=SEG_DTYPE).copy()
        rseg = np.frombuffer((C.c_char * (n * 4)).from_address(oseg.value), dtype=np.uint32).copy()
    lib().sa_free_segments(out)
    lib().sa_free_segments(oseg)
    return res, rseg, counts, bool(refused.value)


def ScanCounts(counts, skew=0, width=32):
    """The exclusive prefix scan alone on uint32 `counts`, read at a 256-byte-aligned address plus `skew` words (sa_scan_counts; test entry).
    -> (the n + 1 sums as uint32 or uint64, dict(temp_guard, out_guard, input): each True when it came back unchanged)"""
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    out = np.zeros(c.size + 1, dtype=np.uint64 if int(width) == 64 else np.uint32)
    intact = np.zeros(3, dtype=np.uint32)
    lib().sa_scan_counts(c.ctypes.data if c.size else None, c.size, int(skew), int(width), out.ctypes.data, intact.ctypes.data)
    return out, dict(temp_guard=bool(intact[0]), out_guard=bool(intact[1]), input=bool(intact[2]))


def ExtendHits(hits, rev, buffer):
    """Extension stage alone for anchors [(ref_loc, query_loc), ...]: passing records, unordered (header removed)."""
    h = np.ascontiguousarray(hits, dtype=np.uint32).reshape(-1, 2)
    out = C.c_void_p()
    n = lib().sa_extend_hits(h.ctypes.data, h.shape[0], int(bool(rev)), buffer, C.byref(out))
    return _take(n, out)[1:]


def _flat(st):
    """A stats struct as one dict, nested structs' fields inlined in order."""
    out = {}
    for k, _ in st._fields_:
        v = getattr(st, k)
        out.update(_flat(v) if isinstance(v, C.Structure) else {k: v})
    return out


def _gapped(fn, free, hsps, rev, buffer, params, st, *extra, paths=True):
    """One call of a gapped entry on SEG_DTYPE hsps: -> (records, paths, ops) as arrays (paths=False: records alone), st filled."""
    h = np.ascontiguousarray(hsps, dtype=SEG_DTYPE)
    p = GappedParams(*(int(x) for x in params))
    out, pth, ops, n_ops = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
    tail = (C.byref(out), C.byref(pth), C.byref(ops), C.byref(n_ops)) if paths else (C.byref(out),)
    n = fn(h.ctypes.data if h.size else None, h.size, int(bool(rev)), buffer, C.byref(p), *extra, *tail, C.byref(st))

    def take(ptr, count, dtype):
        if not count or not ptr.value:
            return np.zeros(0, dtype=dtype)
        return np.frombuffer((C.c_char * (count * dtype.itemsize)).from_address(ptr.value), dtype=dtype).copy()
    recs = take(out, n, GAPPED_DTYPE)
    if not paths:
        free(out)
        return recs
    res = recs, take(pth, n, PATH_DTYPE), take(ops, n_ops.value, np.dtype("<u4"))
    free(out, pth, ops)
    return res


def GappedExtend(hsps, rev, buffer, gap_open=400, gap_extend=30, ydrop=9430, gappedthresh=3000, max_extent=0, max_band=0, raw=False):
    """Gapped y-drop extension of HSP anchors on the device (sa_gapped_extend; contract in include/segalign_amd.h).
    hsps: SEG_DTYPE records (len = bases - 1) on strand `rev` of query `buffer`.  -> (GAPPED_DTYPE array, stats dict).
    raw: one record per HSP in input order; otherwise threshold, one record per extent, output order."""
    st = GappedStats()
    recs = _gapped(lib().sa_gapped_extend, lib().sa_free_gapped, hsps, rev, buffer,
                   (gap_open, gap_extend, ydrop, gappedthresh, max_extent, max_band), st, int(bool(raw)), paths=False)
    return recs, _flat(st)


def GappedAlign(hsps, rev, buffer, gap_open=400, gap_extend=30, ydrop=9430, gappedthresh=3000, max_extent=0, max_band=0, raw=False):
    """GappedExtend plus the alignment path of every record (sa_gapped_align; contract in include/segalign_amd.h).
    -> (GAPPED_DTYPE records, PATH_DTYPE paths, uint32 ops, stats dict).  Record k's ops are
    ops[paths[k].op_offset:][:n_left + n_right], the left side's runs first; decode them with cigar()."""
    st = GappedAlignStats()
    res = _gapped(lib().sa_gapped_align, lib().sa_free_gapped_align, hsps, rev, buffer,
                  (gap_open, gap_extend, ydrop, gappedthresh, max_extent, max_band), st, int(bool(raw)))
    return (*res, _flat(st))


def GappedAlignGreedy(hsps, rev, buffer, gap_open=400, gap_extend=30, ydrop=9430, gappedthresh=3000, max_extent=0, max_band=0):
    """GappedAlign's records and paths, but anchors are extended best first and one that lies on an alignment accepted before it is
    skipped (sa_gapped_align_greedy; contract in include/segalign_amd.h).  -> (GAPPED_DTYPE records, PATH_DTYPE paths,
    uint32 ops, stats dict): GappedAlign's stats plus covered, below_thresh, skipped, priority_batches, cover_segments, cover_ms."""
    st = GappedGreedyStats()
    res = _gapped(lib().sa_gapped_align_greedy, lib().sa_free_gapped_align, hsps, rev, buffer,
                  (gap_open, gap_extend, ydrop, gappedthresh, max_extent, max_band), st)
    return (*res, _flat(st))


def _chain_input(hsps, groups, diag_pen, anti_pen, max_gap, min_score):
    h = np.ascontiguousarray(hsps, dtype=SEG_DTYPE)
    g = None if groups is None else np.ascontiguousarray(groups, dtype=np.uint32)
    if g is not None and g.shape != h.shape:
        raise ValueError("groups: one entry per HSP")
    return h, g, ChainParams(int(diag_pen), int(anti_pen), int(max_gap), 0, int(min_score))


def _chain_overlap(max_overlap):
    """max_overlap as an int in 0 .. CHAIN_MAX_OVERLAP; ValueError otherwise (the library would end the process)."""
    mo = int(max_overlap)
    if not 0 <= mo <= CHAIN_MAX_OVERLAP:
        raise ValueError("max_overlap: %d is not in 0 .. %d" % (mo, CHAIN_MAX_OVERLAP))
    return mo


def _chain_take(ptr, count, dtype):
    """A copy of count records at a malloc-ed result pointer."""
    dtype = np.dtype(dtype)
    if not count or not ptr.value:
        return np.zeros(0, dtype=dtype)
    return np.frombuffer((C.c_char * (count * dtype.itemsize)).from_address(ptr.value), dtype=dtype).copy()


def chain_gap_costs(table):
    """A gap-cost table for ChainHsps / ChainHspsAll (sa_chain_gap_costs; contract in include/segalign_amd.h).
    table: "loose" or "medium" (the presets of sa_chain_gap_preset), a dict {"pos", "q_gap", "t_gap", "both_gap"} of equally long
    sequences (1 .. 16 break points), or a ChainGapCosts, which is returned as it is.  The values are checked by the entry, not here."""
    if isinstance(table, ChainGapCosts):
        return table
    t = ChainGapCosts()
    if isinstance(table, str):
        if lib().sa_chain_gap_preset(table.encode(), C.byref(t)) != 0:
            raise ValueError("chain_gap_costs: no preset %r (loose, medium)" % table)
        return t
    cols = [list(table[k]) for k in ("pos", "q_gap", "t_gap", "both_gap")]
    n = len(cols[0])
    if any(len(c) != n for c in cols):
        raise ValueError("chain_gap_costs: pos, q_gap, t_gap and both_gap must be equally long")
    if n > CHAIN_GAP_POINTS:
        raise ValueError("chain_gap_costs: at most %d break points" % CHAIN_GAP_POINTS)
    t.n = n
    for k in range(n):
        t.pos[k], t.q_gap[k], t.t_gap[k], t.both_gap[k] = (int(c[k]) for c in cols)
    return t


def parse_linear_gap(text):
    """A gap-cost table in axtChain's -linearGap file layout, as segalign_host --gpu_chain_costs=FILE reads it: lines `tableSize N`,
    `smallSize N` (read and ignored), then `position`, `qGap`, `tGap` and `bothGap` with tableSize integers each; blank lines and lines
    starting with # are skipped.  -> the dict chain_gap_costs takes.  ValueError for anything else."""
    want = {"tableSize": None, "smallSize": None, "position": None, "qGap": None, "tGap": None, "bothGap": None}
    for line in text.splitlines():
        w = line.split()
        if not w or w[0].startswith("#"):
            continue
        if w[0] not in want or want[w[0]] is not None:
            raise ValueError("linearGap: unknown or repeated line %r" % w[0])
        try:
            want[w[0]] = [int(x) for x in w[1:]]
        except ValueError:
            raise ValueError("linearGap: %s: not an integer" % w[0])
    for k in ("tableSize", "position", "qGap", "tGap", "bothGap"):
        if want[k] is None:
            raise ValueError("linearGap: no %s line" % k)
    if len(want["tableSize"]) != 1 or (want["smallSize"] is not None and len(want["smallSize"]) != 1):
        raise ValueError("linearGap: tableSize and smallSize take one value")
    n = want["tableSize"][0]
    if not 1 <= n <= CHAIN_GAP_POINTS:
        raise ValueError("linearGap: tableSize %d is not in 1 .. %d" % (n, CHAIN_GAP_POINTS))
    for k in ("position", "qGap", "tGap", "bothGap"):
        if len(want[k]) != n:
            raise ValueError("linearGap: %s has %d values, tableSize is %d" % (k, len(want[k]), n))
    return {"pos": want["position"], "q_gap": want["qGap"], "t_gap": want["tGap"], "both_gap": want["bothGap"]}


def ChainHsps(hsps, groups=None, diag_pen=0, anti_pen=0, max_gap=0, min_score=0, nodes=False, gap_costs=None, max_overlap=0):
    """The best collinear chain of every group of HSPs (sa_chain_hsps; contract in include/segalign_amd.h).
    hsps: SEG_DTYPE records; groups: one uint32 per HSP (None: all in group 0).  -> (CHAIN_MEMBER_DTYPE members, stats dict), or with
    nodes=True (members, CHAIN_NODE_DTYPE nodes in input order, stats dict).  gap_costs: what chain_gap_costs takes, for a link's
    piecewise-linear gap cost on top of the linear terms (sa_chain_hsps_costs); None: none.  max_overlap: the most bases
    two linked HSPs may share on an axis, 0 .. CHAIN_MAX_OVERLAP (sa_chain_hsps_ovl); 0 calls the entries above as
    before.  Needs InitializeInterface only."""
    h, g, p = _chain_input(hsps, groups, diag_pen, anti_pen, max_gap, min_score)
    max_overlap = _chain_overlap(max_overlap)
    mem, nod, st = C.c_void_p(), C.c_void_p(), ChainStats()
    if max_overlap:
        m = lib().sa_chain_hsps_ovl(h.ctypes.data if h.size else None, h.size, g.ctypes.data if g is not None and g.size else None,
                                    C.byref(p), C.byref(chain_gap_costs(gap_costs)) if gap_costs is not None else None,
                                    C.byref(ChainOverlap(max_overlap, 0)), C.byref(mem), C.byref(nod) if nodes else None, C.byref(st))
    elif gap_costs is not None:
        m = lib().sa_chain_hsps_costs(h.ctypes.data if h.size else None, h.size, g.ctypes.data if g is not None and g.size else None,
                                      C.byref(p), C.byref(chain_gap_costs(gap_costs)), C.byref(mem), C.byref(nod) if nodes else None,
                                      C.byref(st))
    else:
        m = lib().sa_chain_hsps(h.ctypes.data if h.size else None, h.size, g.ctypes.data if g is not None and g.size else None, C.byref(p),
                                C.byref(mem), C.byref(nod) if nodes else None, C.byref(st))
    res_m, res_n = _chain_take(mem, m, CHAIN_MEMBER_DTYPE), _chain_take(nod, h.size, CHAIN_NODE_DTYPE)
    lib().sa_free_chain(mem, nod)
    return (res_m, res_n, _flat(st)) if nodes else (res_m, _flat(st))


def ChainHspsAll(hsps, groups=None, diag_pen=0, anti_pen=0, max_gap=0, min_score=0, nodes=False, gap_costs=None, max_overlap=0):
    """All collinear chains of every group of HSPs, peeled best first (sa_chain_hsps_all; contract in include/segalign_amd.h,
    DESIGN.md 16).  Arguments as ChainHsps.  -> (CHAIN_RECORD_DTYPE chains, CHAIN_ALL_MEMBER_DTYPE members, uint32 chain_of in input
    order (CHAIN_NONE: the HSP's chain scores below min_score), stats dict); with nodes=True the CHAIN_NODE_DTYPE nodes come before
    chain_of.  gap_costs as for ChainHsps (sa_chain_hsps_all_costs), max_overlap too (sa_chain_hsps_all_ovl).  Needs
    InitializeInterface only."""
    h, g, p = _chain_input(hsps, groups, diag_pen, anti_pen, max_gap, min_score)
    ch, mem, nod, cof, st, nc = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), ChainAllStats(), C.c_size_t(0)
    max_overlap = _chain_overlap(max_overlap)
    if max_overlap:
        m = lib().sa_chain_hsps_all_ovl(h.ctypes.data if h.size else None, h.size, g.ctypes.data if g is not None and g.size else None,
                                        C.byref(p), C.byref(chain_gap_costs(gap_costs)) if gap_costs is not None else None,
                                        C.byref(ChainOverlap(max_overlap, 0)), C.byref(ch), C.byref(nc), C.byref(mem),
                                        C.byref(nod) if nodes else None, C.byref(cof), C.byref(st))
    elif gap_costs is not None:
        m = lib().sa_chain_hsps_all_costs(h.ctypes.data if h.size else None, h.size, g.ctypes.data if g is not None and g.size else None,
                                          C.byref(p), C.byref(chain_gap_costs(gap_costs)), C.byref(ch), C.byref(nc), C.byref(mem),
                                          C.byref(nod) if nodes else None, C.byref(cof), C.byref(st))
    else:
        m = lib().sa_chain_hsps_all(h.ctypes.data if h.size else None, h.size, g.ctypes.data if g is not None and g.size else None,
                                    C.byref(p), C.byref(ch), C.byref(nc), C.byref(mem), C.byref(nod) if nodes else None, C.byref(cof),
                                    C.byref(st))
    res_c, res_m = _chain_take(ch, nc.value, CHAIN_RECORD_DTYPE), _chain_take(mem, m, CHAIN_ALL_MEMBER_DTYPE)
    res_n, res_o = _chain_take(nod, h.size, CHAIN_NODE_DTYPE), _chain_take(cof, h.size, np.uint32)
    lib().sa_free_chain_all(ch, mem, nod, cof)
    return (res_c, res_m, res_n, res_o, _flat(st)) if nodes else (res_c, res_m, res_o, _flat(st))


def TrimChains(hsps, members, first, rev, buffer=0, diag_pen=0, anti_pen=0, gap_costs=None, links=False):
    """Cuts the overlaps between consecutive members of chains at the best crossover (sa_trim_chains; contract in
    include/segalign_amd.h).  hsps: SEG_DTYPE records; members, first: the chains as chain_csr gives them; rev, buffer:
    the resident query strand and buffer; the penalties and gap_costs the chains were made under.  -> (SEG_DTYPE trimmed HSPs, one per
    member entry: go on with members = arange(M) and first unchanged; TRIM_CHAIN_DTYPE chains; stats dict), with links=True the
    TRIM_LINK_DTYPE links before the stats."""
    h = np.ascontiguousarray(hsps, dtype=SEG_DTYPE)
    mem, fst = np.ascontiguousarray(members, dtype=np.uint32), np.ascontiguousarray(first, dtype=np.uint32)
    if fst.size == 0 or (fst.size and int(fst[-1]) != mem.size):
        raise ValueError("first: one more entry than chains, the last one the number of members")
    p = ChainParams(int(diag_pen), int(anti_pen), 0, 0, 0)
    out, ch, lk, nl, st = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(0), TrimStats()
    m = lib().sa_trim_chains(h.ctypes.data if h.size else None, h.size, mem.ctypes.data if mem.size else None, fst.ctypes.data, fst.size - 1,
                             int(bool(rev)), int(buffer), C.byref(p), C.byref(chain_gap_costs(gap_costs)) if gap_costs is not None else None,
                             TRIM_LINKS if links else 0, C.byref(out), C.byref(ch), C.byref(lk), C.byref(nl), C.byref(st))
    res_h, res_c = _chain_take(out, m, SEG_DTYPE), _chain_take(ch, fst.size - 1 if m else 0, TRIM_CHAIN_DTYPE)
    res_l = _chain_take(lk, nl.value, TRIM_LINK_DTYPE)
    lib().sa_free_trim(out, ch, lk)
    return (res_h, res_c, res_l, _flat(st)) if links else (res_h, res_c, _flat(st))


def FillChains(hsps, members, first, rev, buffer=0, thresh=3000, xdrop=910, diag_pen=0, anti_pen=0, max_gap=0, gap_costs=None, min_fill=0,
               max_side=0, max_cells=0, max_link_hsps=0, links=False, found=False):
    """Fills the links of chains with HSPs from a sweep of every diagonal of the space between consecutive members (sa_fill_chains;
    contract in include/segalign_amd.h).  hsps, members, first, rev, buffer as for TrimChains; thresh, xdrop: the scan;
    the penalties, max_gap and gap_costs choose a link's fill as ChainHsps would, min_fill is its least score; max_side, max_cells,
    max_link_hsps: 0 takes the default.  -> (SEG_DTYPE entries of the filled chains: go on with members = arange(E) and first_out;
    uint32 first_out; uint32 origin (FILL_NONE for a fill); FILL_CHAIN_DTYPE chains; with links=True the FILL_LINK_DTYPE links; with
    found=True the FILL_HSP_DTYPE found HSPs; stats dict)."""
    h = np.ascontiguousarray(hsps, dtype=SEG_DTYPE)
    mem, fst = np.ascontiguousarray(members, dtype=np.uint32), np.ascontiguousarray(first, dtype=np.uint32)
    if fst.size == 0 or (fst.size and int(fst[-1]) != mem.size):
        raise ValueError("first: one more entry than chains, the last one the number of members")
    p = ChainParams(int(diag_pen), int(anti_pen), int(max_gap), 0, 0)
    fp = FillParams(int(thresh), int(xdrop), int(max_side), int(max_link_hsps), int(max_cells), int(min_fill))
    out, fo, org, ch, lk, fd = (C.c_void_p() for _ in range(6))
    nl, nf, st = C.c_size_t(0), C.c_size_t(0), FillStats()
    e = lib().sa_fill_chains(h.ctypes.data if h.size else None, h.size, mem.ctypes.data if mem.size else None, fst.ctypes.data, fst.size - 1,
                             int(bool(rev)), int(buffer), C.byref(p), C.byref(chain_gap_costs(gap_costs)) if gap_costs is not None else None,
                             C.byref(fp), (FILL_LINKS if links else 0) | (FILL_HSPS if found else 0), C.byref(out), C.byref(fo), C.byref(org),
                             C.byref(ch), C.byref(lk), C.byref(nl), C.byref(fd), C.byref(nf), C.byref(st))
    res = [_chain_take(out, e, SEG_DTYPE), _chain_take(fo, fst.size if fo.value else 0, np.uint32), _chain_take(org, e, np.uint32),
           _chain_take(ch, fst.size - 1, FILL_CHAIN_DTYPE)]
    if links:
        res.append(_chain_take(lk, nl.value, FILL_LINK_DTYPE))
    if found:
        res.append(_chain_take(fd, nf.value, FILL_HSP_DTYPE))
    lib().sa_free_fill(out, fo, org, ch, lk, fd)
    if res[1].size == 0:
        res[1] = np.zeros(1, dtype=np.uint32)
    return tuple(res) + (_flat(st),)


def chain_csr(members):
    """The members ChainHsps (one chain per group) or ChainHspsAll (field chain) returns, as StitchChains takes them:
    -> (members: uint32 HSP indices, first: uint32 offsets, one more than there are chains)."""
    m = np.asarray(members)
    key = m["chain"] if "chain" in m.dtype.names else m["group"]
    starts = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if m.size else np.zeros(0, dtype=np.int64)
    return m["hsp_index"].astype(np.uint32), np.concatenate([starts, [m.size]]).astype(np.uint32)


def StitchChains(hsps, members, first, rev, buffer=0, gap_open=400, gap_extend=30, max_link=0, min_link_score=None, links=False):
    """Every chain as one gapped alignment through all its members (sa_stitch_chains; contract in include/segalign_amd.h).
    hsps: SEG_DTYPE records on strand `rev` of query `buffer`; chain c is members[first[c]:first[c + 1]] (see chain_csr).
    -> (STITCH_RECORD_DTYPE records, uint32 ops, stats dict), with links=True (records, ops, STITCH_LINK_DTYPE links, stats dict).
    Record k's ops are ops[op_offset:][:n_ops]; decode them with cigar()."""
    h = np.ascontiguousarray(hsps, dtype=SEG_DTYPE)
    m = np.ascontiguousarray(members, dtype=np.uint32)
    f = np.ascontiguousarray(first, dtype=np.uint32)
    if f.size < 1 or int(f[-1]) != m.size:
        raise ValueError("first: one offset per chain and the number of members at the end")
    p = StitchParams(int(gap_open), int(gap_extend), int(max_link), STITCH_NEVER if min_link_score is None else int(min_link_score))
    rec, ops, lnk, n_ops, n_links, st = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_size_t(0), StitchStats()
    n = lib().sa_stitch_chains(h.ctypes.data if h.size else None, h.size, m.ctypes.data if m.size else None, f.ctypes.data, f.size - 1,
                               int(bool(rev)), buffer, C.byref(p), C.byref(rec), C.byref(ops), C.byref(n_ops),
                               C.byref(lnk) if links else None, C.byref(n_links) if links else None, C.byref(st))
    res_r, res_o = _chain_take(rec, n, STITCH_RECORD_DTYPE), _chain_take(ops, n_ops.value, np.dtype("<u4"))
    res_l = _chain_take(lnk, n_links.value, STITCH_LINK_DTYPE)
    lib().sa_free_stitch(rec, ops, lnk)
    return (res_r, res_o, res_l, _flat(st)) if links else (res_r, res_o, _flat(st))


def diff_spans(records, paths=None):
    """The alignments of a producer as DiffAlignments takes them, over the producer's ops: GappedAlign / GappedAlignGreedy records with
    their paths (n_ops = n_left + n_right), or StitchChains records alone.  -> DIFF_SPAN_DTYPE spans."""
    r = np.asarray(records)
    src = r if paths is None else np.asarray(paths)
    if src.shape != r.shape:
        raise ValueError("paths: one per record")
    sp = np.zeros(r.size, dtype=DIFF_SPAN_DTYPE)
    sp["ref_start"], sp["query_start"], sp["op_offset"] = r["ref_start"], r["query_start"], src["op_offset"]
    sp["n_ops"] = src["n_ops"] if paths is None else src["n_left"] + src["n_right"]
    return sp


def DiffAlignments(spans, ops, rev, buffer=0, per_base=False, events=True, chunk=0):
    """Where alignments differ from the two resident sequences, what each is made of, and the pair counts of their aligned columns
    (sa_diff_alignments; contract in include/segalign_amd.h).  spans: DIFF_SPAN_DTYPE (see diff_spans) over ops, uint32
    (run << 2) | op on strand `rev` of query `buffer`; per_base: every substitution column is its own event; events=False: summaries
    and statistics only.  -> (DIFF_EVENT_DTYPE events, DIFF_SUMMARY_DTYPE summaries, stats dict; stats["pairs"] is a uint64 array of 64
    counts by tcode * 8 + qcode)."""
    sp = np.ascontiguousarray(spans, dtype=DIFF_SPAN_DTYPE)
    o = np.ascontiguousarray(ops, dtype=np.uint32)
    p = DiffParams((DIFF_PER_BASE if per_base else 0) | (0 if events else DIFF_NO_EVENTS), int(chunk))
    ev, sm, st = C.c_void_p(), C.c_void_p(), DiffStats()
    n = lib().sa_diff_alignments(sp.ctypes.data if sp.size else None, sp.size, o.ctypes.data if o.size else None, o.size, int(bool(rev)),
                                 int(buffer), C.byref(p), C.byref(ev), C.byref(sm), C.byref(st))
    res_e, res_s = _chain_take(ev, n, DIFF_EVENT_DTYPE), _chain_take(sm, sp.size, DIFF_SUMMARY_DTYPE)
    lib().sa_free_diff(ev, sm)
    out = {k: getattr(st, k) for k, _ in DiffStats._fields_ if k not in ("pairs", "pad")}
    out["pairs"] = np.array(st.pairs[:], dtype=np.uint64)
    return res_e, res_s, out


def net_blocks(hsps, members, first, axis="target"):
    """The chains of chain_csr as NetChains takes them on one axis: every member HSP gives the block [start, start + len + 1) there.
    Rank order makes the blocks of a chain ascending and disjoint on both axes.  -> (block_start, block_end), uint32, first unchanged."""
    if axis not in ("target", "query"):
        raise ValueError("axis: target or query")
    h = np.ascontiguousarray(hsps, dtype=SEG_DTYPE)[np.asarray(members, dtype=np.int64)]
    if int(np.asarray(first)[-1]) != h.size:
        raise ValueError("first: one offset per chain and the number of members at the end")
    start = h["ref_start" if axis == "target" else "query_start"].astype(np.uint32)
    return start, (start + h["len"] + np.uint32(1)).astype(np.uint32)


def NetChains(first, block_start, block_end, score, group=None, min_space=1, min_fill=1):
    """The chains of every group netted into fills and gaps on one axis (sa_net_chains; contract in include/segalign_amd.h).
    Chain c is the half-open blocks first[c] .. first[c + 1] - 1 of block_start / block_end (see net_blocks); score: one int64 per chain;
    group: one uint32 per chain (None: one group).  -> (NET_FILL_DTYPE fills ordered by (group, start), stats dict).  Needs
    InitializeInterface only."""
    f = np.ascontiguousarray(first, dtype=np.uint32)
    bs = np.ascontiguousarray(block_start, dtype=np.uint32)
    be = np.ascontiguousarray(block_end, dtype=np.uint32)
    sc = np.ascontiguousarray(score, dtype=np.int64)
    g = None if group is None else np.ascontiguousarray(group, dtype=np.uint32)
    n = f.size - 1
    if n < 0 or sc.size != n or (g is not None and g.size != n) or bs.size != be.size or bs.size < int(f.max()):
        raise ValueError("first: one offset per chain and one more; score, group: one entry per chain; blocks: first[-1] of each")
    p, out, st = NetParams(int(min_space), int(min_fill)), C.c_void_p(), NetStats()
    k = lib().sa_net_chains(f.ctypes.data, bs.ctypes.data if bs.size else None, be.ctypes.data if be.size else None,
                            sc.ctypes.data if n else None, g.ctypes.data if g is not None and n else None, n, C.byref(p), C.byref(out),
                            C.byref(st))
    res = _chain_take(out, k, NET_FILL_DTYPE)
    lib().sa_free_net(out)
    return res, _flat(st)


def NetSubset(hsps, members, first, fills, rev, buffer=0, axis="target", split=True, diag_pen=0, anti_pen=0, gap_costs=None):
    """Every fill of a net as sub-chains of its chain: clipped to the fill, rescored, ready for StitchChains (sa_net_subset; contract in
    include/segalign_amd.h).  hsps, members, first: as StitchChains takes them; fills: what NetChains returned for
    net_blocks(hsps, members, first, axis); split: cut a fill where a child lies in one of its gaps; diag_pen, anti_pen, gap_costs: the
    penalties the chains were made under.  -> (SEG_DTYPE out_hsps, SUBSET_CHAIN_DTYPE chains, stats dict); see subset_csr."""
    if axis not in ("target", "query"):
        raise ValueError("axis: target or query")
    h = np.ascontiguousarray(hsps, dtype=SEG_DTYPE)
    m = np.ascontiguousarray(members, dtype=np.uint32)
    f = np.ascontiguousarray(first, dtype=np.uint32)
    fl = np.ascontiguousarray(fills, dtype=NET_FILL_DTYPE)
    if f.size < 1 or int(f[-1]) != m.size:
        raise ValueError("first: one offset per chain and the number of members at the end")
    p = ChainParams(int(diag_pen), int(anti_pen), 0, 0, 0)
    out, rec, n_out, st = C.c_void_p(), C.c_void_p(), C.c_size_t(0), SubsetStats()
    n = lib().sa_net_subset(h.ctypes.data if h.size else None, h.size, m.ctypes.data if m.size else None, f.ctypes.data, f.size - 1,
                            fl.ctypes.data if fl.size else None, fl.size, int(axis == "query"), int(bool(rev)), buffer, C.byref(p),
                            None if gap_costs is None else C.byref(chain_gap_costs(gap_costs)), SUBSET_SPLIT if split else 0,
                            C.byref(out), C.byref(n_out), C.byref(rec), C.byref(st))
    res_h, res_c = _chain_take(out, n_out.value, SEG_DTYPE), _chain_take(rec, n, SUBSET_CHAIN_DTYPE)
    lib().sa_free_net_subset(out, rec)
    return res_h, res_c, _flat(st)


def subset_csr(chains):
    """The sub-chains of NetSubset as StitchChains and net_blocks take them, over NetSubset's out_hsps:
    -> (members: 0 .. m - 1, first: the runs' offsets and m at the end), uint32."""
    c = np.asarray(chains)
    m = int(c["first_member"][-1]) + int(c["n_members"][-1]) if c.size else 0
    return np.arange(m, dtype=np.uint32), np.concatenate([c["first_member"], [m]]).astype(np.uint32)


def net_other_blocks(hsps, members, first, axis="target", strand=None, size=None):
    """net_blocks on the OTHER axis than `axis`, as NetClassify takes it.  strand: one 0 / 1 per chain (None: all 0); for a chain with
    strand 1 every block [s, e) becomes [size[chain] - e, size[chain] - s), the flip of a minus-strand chain into the plus orientation,
    so that its blocks descend.  size: one length per chain (that of the sequence the chain lies on), needed with strand.
    -> (oblock_start, oblock_end), uint32."""
    if axis not in ("target", "query"):
        raise ValueError("axis: target or query")
    s, e = net_blocks(hsps, members, first, "query" if axis == "target" else "target")
    if strand is None:
        return s, e
    f = np.asarray(first, dtype=np.int64)
    st = np.asarray(strand, dtype=np.uint8)
    if size is None or st.size != f.size - 1 or np.asarray(size).size != st.size:
        raise ValueError("strand, size: one entry per chain")
    chain = np.repeat(np.arange(st.size), np.diff(f))
    flip = st[chain] != 0
    n = np.asarray(size, dtype=np.int64)[chain]
    if np.any(flip & (e.astype(np.int64) > n)):
        raise ValueError("size: a block of a strand-1 chain ends past it")
    os_ = np.where(flip, n - e.astype(np.int64), s.astype(np.int64))
    oe = np.where(flip, n - s.astype(np.int64), e.astype(np.int64))
    return os_.astype(np.uint32), oe.astype(np.uint32)


def NetClassify(first, block_start, block_end, oblock_start, oblock_end, fills, ogroup=None, ostrand=None, filter=None):
    """Every fill of a net classed against its parent on the other axis (top / syn / inv / nonSyn), with the bases it shares with other
    fills there and the synteny filter's keep mark (sa_net_classify; contract in include/segalign_amd.h).
    first, block_start, block_end: what NetChains took; oblock_start, oblock_end: the same blocks on the other axis (net_other_blocks);
    fills: what NetChains returned; ogroup: one uint32 per chain, the sequence it lies on on the other axis (None: all 0); ostrand: one
    0 / 1 per chain (None: all 0); filter: a dict of min_score, min_top_score, min_size, min_ali, max_far (missing ones 0), or None for
    no filter.  -> (NET_CLASS_DTYPE classes, stats dict).  Needs InitializeInterface only."""
    f = np.ascontiguousarray(first, dtype=np.uint32)
    arr = [np.ascontiguousarray(x, dtype=np.uint32) for x in (block_start, block_end, oblock_start, oblock_end)]
    fl = np.ascontiguousarray(fills, dtype=NET_FILL_DTYPE)
    g = None if ogroup is None else np.ascontiguousarray(ogroup, dtype=np.uint32)
    sd = None if ostrand is None else np.ascontiguousarray(ostrand, dtype=np.uint8)
    n = f.size - 1
    if n < 0 or any(x.size != arr[0].size for x in arr) or arr[0].size < int(f.max()) or any(x is not None and x.size != n for x in (g, sd)):
        raise ValueError("first: one offset per chain and one more; ogroup, ostrand: one entry per chain; blocks: first[-1] of each, on both axes")
    p = NetClassParams()
    if filter is not None:
        if set(filter) - set(NETCLASS_THRESHOLDS):
            raise ValueError("filter: %s" % ", ".join(NETCLASS_THRESHOLDS))
        for k in NETCLASS_THRESHOLDS:
            setattr(p, k, int(filter.get(k, 0)))
    out, st = C.c_void_p(), NetClassStats()
    ptr = [x.ctypes.data if x.size else None for x in arr]
    k = lib().sa_net_classify(f.ctypes.data, ptr[0], ptr[1], ptr[2], ptr[3], g.ctypes.data if g is not None and n else None,
                              sd.ctypes.data if sd is not None and n else None, n, fl.ctypes.data if fl.size else None, fl.size,
                              C.byref(p), NETCLASS_FILTER if filter is not None else 0, C.byref(out), C.byref(st))
    res = _chain_take(out, k, NET_CLASS_DTYPE)
    lib().sa_free_net_class(out)
    stats = _flat(st)
    stats["n_type"] = [int(x) for x in st.n_type]
    return res, stats


def net_select(fills, keep):
    """The fills with keep != 0, in the same order, parent remapped to the new indices: -> (fills', index of every kept fill in the
    input).  keep must be closed under subtrees (NetClassify's is): a kept fill's parent is kept, so the result is a net of its own that
    NetSubset takes unchanged."""
    fl = np.ascontiguousarray(fills, dtype=NET_FILL_DTYPE)
    k = np.asarray(keep).astype(bool)
    if k.shape != fl.shape:
        raise ValueError("keep: one entry per fill")
    index = np.flatnonzero(k)
    new = np.cumsum(k) - 1
    out = fl[index].copy()
    has = out["parent"] >= 0
    if np.any(~k[out["parent"][has]]):
        raise ValueError("keep: a kept fill whose parent is dropped")
    out["parent"][has] = new[out["parent"][has]]
    return out, index.astype(np.uint32)


def LiftIntervals(first, block_start, block_end, oblock_start, oblock_end, iv_start, iv_end, group=None, ogroup=None, ostrand=None,
                  iv_group=None, min_match=(95, 100), multiple=False, blocks=False):
    """Intervals of one axis carried through chains to the other axis (sa_lift_intervals; contract in include/segalign_amd.h, DESIGN.md
    23).  first, block_start, block_end, oblock_start, oblock_end, ogroup, ostrand: the chains as NetClassify takes them (net_blocks,
    net_other_blocks); group: one uint32 per chain, the sequence it lies on on the axis (None: all 0); iv_start, iv_end: the half-open
    intervals, iv_group: their sequences (None: all 0); min_match: (num, den), the least fraction of an interval a chain must hold;
    multiple: a hit per qualifying chain of every interval, not only the one of a MAPPED interval; blocks: also the clipped block pairs
    of every hit.  -> (LIFT_RECORD_DTYPE records, LIFT_HIT_DTYPE hits, LIFT_BLOCK_DTYPE blocks or None, stats dict).  Needs
    InitializeInterface only."""
    f = np.ascontiguousarray(first, dtype=np.uint32)
    arr = [np.ascontiguousarray(x, dtype=np.uint32) for x in (block_start, block_end, oblock_start, oblock_end)]
    g, og, ig = (None if x is None else np.ascontiguousarray(x, dtype=np.uint32) for x in (group, ogroup, iv_group))
    sd = None if ostrand is None else np.ascontiguousarray(ostrand, dtype=np.uint8)
    ivs, ive = np.ascontiguousarray(iv_start, dtype=np.uint32), np.ascontiguousarray(iv_end, dtype=np.uint32)
    n = f.size - 1
    if n < 0 or any(x.size != arr[0].size for x in arr) or arr[0].size < int(f.max()) or any(x is not None and x.size != n for x in (g, og, sd)):
        raise ValueError("first: one offset per chain and one more; group, ogroup, ostrand: one entry per chain; blocks: first[-1] of each, on both axes")
    if ivs.size != ive.size or (ig is not None and ig.size != ivs.size):
        raise ValueError("iv_start, iv_end, iv_group: one entry per interval")
    p = LiftParams(int(min_match[0]), int(min_match[1]))
    rec, hit, blk, nh, nb, st = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_size_t(0), LiftStats()
    ptr = [x.ctypes.data if x.size else None for x in arr]
    per_chain = [x.ctypes.data if x is not None and n else None for x in (g, og, sd)]
    k = lib().sa_lift_intervals(f.ctypes.data, ptr[0], ptr[1], ptr[2], ptr[3], per_chain[0], per_chain[1], per_chain[2], n,
                                ig.ctypes.data if ig is not None and ig.size else None, ivs.ctypes.data if ivs.size else None,
                                ive.ctypes.data if ive.size else None, ivs.size, C.byref(p),
                                (LIFT_MULTIPLE if multiple else 0) | (LIFT_BLOCKS if blocks else 0), C.byref(rec), C.byref(hit), C.byref(nh),
                                C.byref(blk), C.byref(nb), C.byref(st))
    res = (_chain_take(rec, k, LIFT_RECORD_DTYPE), _chain_take(hit, nh.value, LIFT_HIT_DTYPE),
           _chain_take(blk, nb.value, LIFT_BLOCK_DTYPE) if blocks else None)
    lib().sa_free_lift(rec, hit, blk)
    stats = _flat(st)
    stats["n_status"] = [int(x) for x in st.n_status]
    return res + (stats,)


def cigar(ops):
    """Run-length ops (uint32 (length << 2) | op) as a CIGAR string: M aligned pair, I query base, D target base."""
    return "".join("%d%s" % (int(x) >> 2, "MID"[int(x) & 3]) for x in ops)


def SeedInterval(start, end, q_len, strands=STRAND_BOTH, buffer=0, threads=2):
    """seeder_body::operator() (src/seeder.cpp:12-127) for one query interval, chunk calls issued from C++ threads.
    Returns (plus-strand HSPs, minus-strand HSPs, summed statistics)."""
    fw, rc = C.c_void_p(), C.c_void_p()
    nf, nr = C.c_size_t(), C.c_size_t()
    st = CallStats()
    lib().sa_seed_interval(start, end, q_len, strands, buffer, threads, C.byref(fw), C.byref(nf), C.byref(rc), C.byref(nr),
                           C.byref(st))

    def take(ptr, n):
        if n == 0:
            lib().sa_free_segments(ptr)
            return np.zeros(0, dtype=SEG_DTYPE)
        buf = (C.c_char * (n * SEG_DTYPE.itemsize)).from_address(ptr.value)
        a = np.frombuffer(buf, dtype=SEG_DTYPE).copy()
        lib().sa_free_segments(ptr)
        return a

    return take(fw, nf.value), take(rc, nr.value), {f[0]: getattr(st, f[0]) for f in CallStats._fields_}


# ---- repeat masker ----------------------------------------------------------------------------------------------
def RmSendQueryWriteRequest():
    lib().sa_rm_send_query_write_request()


def RmClearQuery():
    lib().sa_rm_clear_query()


def RmSeedAndFilter(seed_offset_vector, rev, ref_start, ref_end):
    s = np.ascontiguousarray(seed_offset_vector, dtype=np.uint64)
    out = C.c_void_p()
    n = lib().sa_rm_seed_and_filter(s.ctypes.data, s.size, int(bool(rev)), ref_start, ref_end, C.byref(out))
    return _take(n, out)


def _take_intervals(n, out):
    if n == 0 or not out.value:
        return np.zeros(0, dtype=IVL_DTYPE)
    buf = (C.c_char * (n * IVL_DTYPE.itemsize)).from_address(out.value)
    iv = np.frombuffer(buf, dtype=IVL_DTYPE).copy()
    lib().sa_free_intervals(out)
    return iv


def RmMaskInterval(start_pos, end_pos, ref_start, ref_end, strands=STRAND_BOTH, M=1):
    """Device-side seeder_body::operator() of the repeat masker (repeat_masker_src/seeder.cpp:28-195) for one interval.
    Returns (intervals, dict(num_seeds, num_hits, num_hsps))."""
    out = C.c_void_p()
    tot = (C.c_uint64 * 3)()
    n = lib().sa_rm_mask_interval(start_pos, end_pos, ref_start, ref_end, strands, M, C.byref(out), tot)
    return _take_intervals(n, out), dict(num_seeds=tot[0], num_hits=tot[1], num_hsps=tot[2])


def RmCoverageIntervals(hsps, block_len, M=1):
    """repeat_masker_src/seeder.cpp:153-188 on the device for HSPs the host collected (headers removed)."""
    h = np.ascontiguousarray(hsps, dtype=SEG_DTYPE)
    out = C.c_void_p()
    n = lib().sa_rm_coverage_intervals(h.ctypes.data if h.size else None, h.size, block_len, M, C.byref(out))
    return _take_intervals(n, out)


# ---- knobs / introspection ---------------------------------------------------------------------------------------
def set_max_hits(v):
    lib().sa_set_max_hits(v)


def get_max_hits():
    return lib().sa_get_max_hits()


def max_hits_for_mem(total_global_mem):
    return lib().sa_max_hits_for_mem(total_global_mem)


def last_call_stats():
    st = CallStats()
    lib().sa_get_last_call_stats(C.byref(st))
    return {k: getattr(st, k) for k, _ in CallStats._fields_}


def last_call_trace():
    """Which way the calling thread's last hot call went through the call core (sa_get_last_call_trace; test entry)."""
    tr = CallTrace()
    lib().sa_get_last_call_trace(C.byref(tr))
    return {k: int(getattr(tr, k)) for k, _ in CallTrace._fields_}


def lookup_mode():
    """0 general (seed words), 1 table-direct, 2 table-direct with target context (see sa_get_lookup_mode)."""
    return int(lib().sa_get_lookup_mode())


def neighbourhood_entries():
    return int(lib().sa_get_neighbourhood_entries())


def table_build_info():
    """How the resident tables of device 0 were made (sa_get_table_build_info; test entry): {"build": TABLE_BUILD_*,
    "unsorted_partitions", "nbr_fill": NBR_FILL_*, "left_skip"}."""
    st = TableBuildInfo()
    if lib().sa_get_table_build_info(C.byref(st)) != 0:
        raise RuntimeError("sa_get_table_build_info before InitializeInterface")
    return {k: int(getattr(st, k)) for k, _ in TableBuildInfo._fields_}


def copy_neighbourhood_starts(first_key=0, count=None, dev=0):
    """nbr_start[first_key : first_key + count] (uint64; count None: up to and including the closing word at 4^kmer_size)."""
    if count is None:
        count = int(lib().sa_get_index_table_size()) + 1 - int(first_key)
    out = np.empty(max(int(count), 0), dtype=np.uint64)
    if lib().sa_copy_neighbourhood_starts(dev, int(first_key), int(count), out.ctypes.data) != 0:
        raise RuntimeError("sa_copy_neighbourhood_starts failed (table not built, or range outside it)")
    return out


def copy_neighbourhood_records(first_entry=0, count=None, dev=0):
    """Entries [first_entry, first_entry + count) of the neighbourhood table (count None: to its end) -> (mode, array): CTX_DTYPE
    records in lookup mode 2, uint32 seed start positions in mode 1."""
    if count is None:
        count = neighbourhood_entries() - int(first_entry)
    buf = np.empty(max(int(count), 0) * 8, dtype=np.uint32)  # (room for the larger of the two)
    mode = lib().sa_copy_neighbourhood_records(dev, int(first_entry), int(count), buf.ctypes.data)
    if mode not in (1, 2):
        raise RuntimeError("sa_copy_neighbourhood_records failed (table not built, or range outside it)")
    return mode, (buf.view(CTX_DTYPE).copy() if mode == 2 else buf[:max(int(count), 0)].copy())


def ProbeCall(start, end, rev=False, buffer=0, rm=False):
    """The front of a table-direct call alone (sa_probe_call; test entry): [start, end) of a strand of the resident query (rm: of the
    target itself) is clipped and cut into wga_chunk-sized chunks as SeedAndFilterChunks does it, probed, compacted and planned.
    -> dict with "status" (PROBE_*); with PROBE_OK also the scalars of sa_probe_result and the arrays "plans" (PROBE_PLAN_DTYPE),
    "bounds" (PROBE_BOUND_DTYPE), "records" (PROBE_REC_DTYPE, sentinel included), "head_bits" (uint32), "td_chunk" (uint32), "seg_end"
    (uint64), "t_off" (uint64, PROBE_VALID set for a valid window), "t_cnt" (uint32)."""
    r = ProbeResult()
    status = lib().sa_probe_call(int(start), int(end), int(bool(rev)), int(buffer), int(bool(rm)), C.byref(r))
    if status != PROBE_OK:
        return {"status": int(status)}
    try:
        def take(ptr, count, dtype):
            dtype = np.dtype(dtype)
            if not count:
                return np.zeros(0, dtype=dtype)
            return np.frombuffer((C.c_char * (int(count) * dtype.itemsize)).from_address(ptr), dtype=dtype).copy()
        out = {k: int(getattr(r, k)) for k, t in ProbeResult._fields_ if t is not C.c_void_p}
        n = out["end"] - out["start"]
        out.update(plans=take(r.plans, r.num_chunks, PROBE_PLAN_DTYPE), bounds=take(r.bounds, r.num_chunks + 1, PROBE_BOUND_DTYPE),
                   records=take(r.records, r.num_records + 1, PROBE_REC_DTYPE), head_bits=take(r.head_bits, r.num_head_words, np.uint32),
                   td_chunk=take(r.td_chunk, r.num_td_chunk, np.uint32), seg_end=take(r.seg_end, min(r.num_seg_end, 512), np.uint64),
                   t_off=take(r.t_off, n, np.uint64), t_cnt=take(r.t_cnt, n, np.uint32))
        return out
    finally:
        lib().sa_free_probe_call(C.byref(r))


def copy_image(name, buffer=0, dev=0):
    """The whole span of one image of the resident blocks (sa_copy_image; test entry; `name` in IMAGES) -> (info, bytes): info = {"bytes",
    "stride", "origin", "len", "copies"}, bytes a uint8 array of the span.  None when the image is not resident."""
    info = ImageInfo()
    image = IMAGES.index(name)
    if lib().sa_copy_image(dev, image, int(buffer), None, 0, C.byref(info)) != 0:
        return None
    out = np.empty(int(info.bytes), dtype=np.uint8)
    if lib().sa_copy_image(dev, image, int(buffer), out.ctypes.data, out.size, C.byref(info)) != 0:
        raise RuntimeError("sa_copy_image failed")
    return {k: int(getattr(info, k)) for k, _ in ImageInfo._fields_}, out


def code_presence(dev=0):
    """(ref_present, [query_present of every buffer]): the masks the host holds (sa_get_code_presence; test entry)."""
    r = C.c_uint32()
    q = (C.c_uint32 * 2)()
    if lib().sa_get_code_presence(dev, C.byref(r), q) != 0:
        raise RuntimeError("sa_get_code_presence: device out of range")
    return int(r.value), [int(v) for v in q]


def class_scores(present_t, present_q):
    """The class filter's class scores for two presence masks under the resident matrix (sa_get_class_scores; test entry)."""
    cls = (C.c_int32 * 4)()
    if lib().sa_get_class_scores(int(present_t), int(present_q), cls) != 0:
        raise RuntimeError("sa_get_class_scores before InitializeProcessor")
    return [int(v) for v in cls]


def filter_mode():
    return int(lib().sa_get_filter_mode())


def set_count_examined(on):
    lib().sa_set_count_examined(int(bool(on)))


def profile_enable(on=True):
    lib().sa_profile_enable(int(bool(on)))


def profile_reset():
    lib().sa_profile_reset()


def profile_entries():
    """{kernel name: (total_ms, launches)} measured with HIP events on the engine's own streams."""
    out = {}
    L = lib()
    for i in range(L.sa_profile_num_entries()):
        name = C.create_string_buffer(64)
        ms = C.c_double()
        n = C.c_uint64()
        if L.sa_profile_get(i, name, 64, C.byref(ms), C.byref(n)) == 0:
            out[name.value.decode()] = (ms.value, n.value)
    return out


def profile_busy_ms(name):
    """ms during which at least one launch of the scope was running (union over the slots' streams)."""
    return float(lib().sa_profile_busy_ms(name.encode()))


def copy_ref_codes(dev=0):
    out = np.empty(lib().sa_get_ref_len(), dtype=np.uint8)
    lib().sa_copy_ref_codes(dev, out.ctypes.data)
    return out


def copy_index_table(dev=0):
    out = np.empty(lib().sa_get_index_table_size(), dtype=np.uint32)
    lib().sa_copy_index_table(dev, out.ctypes.data)
    return out


def copy_pos_table(dev=0):
    out = np.empty(lib().sa_get_num_index(), dtype=np.uint32)
    if out.size:
        lib().sa_copy_pos_table(dev, out.ctypes.data)
    return out


def copy_query_codes(buffer, rev, dev=0):
    out = np.empty(lib().sa_get_query_len(buffer), dtype=np.uint8)
    lib().sa_copy_query_codes(dev, buffer, int(bool(rev)), out.ctypes.data)
    return out


def device_make_seeds(start, end, rev, buffer, per=13):
    cap = max((end - start) * per, 1)
    out = np.empty(cap, dtype=np.uint64)
    n = lib().sa_device_make_seeds(start, end, int(bool(rev)), buffer, out.ctypes.data, cap)
    return out[:min(n, cap)].copy()


# ---- options (include/segalign_amd.h: one table, resolved at InitializeProcessor) -------------------------------
def set_option(name, value):
    if lib().sa_set_option(name.encode(), int(value)) != 0:
        raise KeyError("unknown engine option %r" % name)


def reset_option(name=None):
    lib().sa_reset_option(name.encode() if name else None)


def get_option(name):
    return int(lib().sa_get_option(name.encode()))


def options():
    """{name: test_only} of every option the engine knows."""
    out = {}
    for i in range(lib().sa_option_count()):
        t = C.c_int(0)
        name = lib().sa_option_name(i, C.byref(t)).decode()  # (first: an assignment evaluates its right side before the subscript)
        out[name] = bool(t.value)
    return out


def get_audit(cap=1 << 22):
    """(ref_loc, query_loc) of the hits the filter levels rejected in this thread's last table-direct call (option audit_cap)."""
    buf = np.empty((cap, 2), dtype=np.uint32)
    n = lib().sa_get_audit(buf.ctypes.data, cap)
    return buf[:min(n, cap)].copy(), int(n)


L2REC_DTYPE = np.dtype([("ref_loc", "<u4"), ("query_loc", "<u4"), ("hidx", "<u4"), ("state", "<u4"), ("meta", "<u4")])


def get_forwards(cap=1 << 22):
    """(records, total, sub_counts) of the hand-over list of this thread's last context-table call (option fwd_keep): the records the
    class filter gave the second level, in sub-list order (sa_get_forwards documents the 20-byte record), how many the call kept,
    and the 256 raw sub-list counters."""
    buf = np.empty(cap, dtype=L2REC_DTYPE)
    counts = np.zeros(256, dtype=np.uint32)
    n = lib().sa_get_forwards(buf.ctypes.data, cap, counts.ctypes.data)
    return buf[:min(n, cap)].copy(), int(n), counts
