"""ctypes binding of libvsx.so (the C-ABI declared in include/vsx.h).

The shared library is built IN-TREE (vsearch_amd/libvsx.so, `make -C vsearch_amd/csrc` or
__graft_entry__.build()).  There is no CPU fallback: if the library is missing, loading fails
loudly; if no gfx950 device is visible every compute entry point returns VSX_ENODEVICE.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# VSX_LIBRARY: another build of the same library (A/B builds of the kernels under build/variants/); default: the in-tree one
LIB_PATH = os.environ.get("VSX_LIBRARY") or os.path.join(HERE, "libvsx.so")

VSX_OK, VSX_EINVAL, VSX_ENODEVICE, VSX_ENOMEM, VSX_EHIP = 0, -1, -2, -3, -4
SENTINEL = 32767

# every symbol include/vsx.h declares
SYMBOLS = [
    "vsx_version_string", "vsx_device_count", "vsx_last_error", "vsx_create", "vsx_destroy",
    "vsx_seqset_create", "vsx_seqset_create_both_strands", "vsx_seqset_create_from_device", "vsx_seqset_destroy", "vsx_seqset_count",
    "vsx_plan_create", "vsx_plan_run", "vsx_plan_sync", "vsx_plan_fetch", "vsx_plan_export_hits", "vsx_plan_export_runs",
    "vsx_cigar_from_runs", "vsx_plan_destroy",
    "vsx_align_pairs", "vsx_align_pairs_filtered", "vsx_align_pairs_ranked", "vsx_ranked_free", "vsx_plan_set_filter", "vsx_results_free", "vsx_plan_describe",
]
# include/vsx_search.h, exact sequence search (--search_exact); part of SEARCH_SYMBOLS
EXACT_SYMBOLS = ["vsx_search_exact", "vsx_search_exact_last_stats", "vsx_internal_search_exact_host"]
# include/vsx_search.h
SEARCH_SYMBOLS = ["vsx_search_opts_default", "vsx_searcher_create", "vsx_searcher_destroy", "vsx_searcher_db_text", "vsx_search_batch",
                  "vsx_search_batch_meta", "vsx_searcher_set_meta",
                  "vsx_hits_free", "vsx_search_candidates", "vsx_search_candidates_batch", "vsx_candidates_free", "vsx_lma_align", "vsx_allpairs_block", "vsx_allpairs_rows", "vsx_allpairs_stream", "vsx_cluster_fast", "vsx_cluster_out_free", "vsx_msa", "vsx_msa_out_free",
                  "vsx_msa_device", "vsx_msa_device_batch", "vsx_dust_mask", "vsx_abundance_ratio_cmp",
                  "vsx_multi_searcher_create", "vsx_multi_searcher_destroy", "vsx_multi_searcher_devices", "vsx_multi_searcher_replica",
                  "vsx_multi_search_batch", "vsx_multi_allpairs",
                  "vsx_chimera_opts_default", "vsx_uchime_ref", "vsx_chimera_last_stats",
                  "vsx_chimera_denovo_opts_default", "vsx_uchime_denovo", "vsx_chimera_denovo_last_stats",
                  "vsx_chimeras_long_opts_default", "vsx_chimeras_denovo", "vsx_chimeras_denovo_last_stats",
                  "vsx_internal_chimeras_long_host"] + EXACT_SYMBOLS
# include/vsx_merge.h (a list of its own: SYMBOLS stays exactly what include/vsx.h declares; build() checks both)
MERGE_SYMBOLS = ["vsx_merge_opts_default", "vsx_merge_pairs", "vsx_merge_out_free", "vsx_merge_last_stats"]
# include/vsx_filter.h
FILTER_SYMBOLS = ["vsx_fastx_filter_opts_default", "vsx_fastx_filter", "vsx_fastx_filter_out_free", "vsx_fastx_filter_last_stats"]
# include/vsx_eestats.h
EESTATS_SYMBOLS = ["vsx_fastq_eestats_opts_default", "vsx_fastq_eestats", "vsx_fastq_eestats_out_free", "vsx_fastq_eestats_last_stats"]
EESTATS_WANT_EESTATS, EESTATS_WANT_EESTATS2 = 1, 2
# include/vsx_fastq_stats.h
FASTQ_STATS_SYMBOLS = ["vsx_fastq_stats_opts_default", "vsx_fastq_stats", "vsx_fastq_stats_out_free", "vsx_fastq_stats_last_stats",
                       "vsx_fastq_chars_opts_default", "vsx_fastq_chars", "vsx_fastq_chars_out_free", "vsx_fastq_chars_last_stats"]


# include/vsx_derep.h
DEREP_SYMBOLS = ["vsx_derep_opts_default", "vsx_derep", "vsx_derep_out_free", "vsx_derep_last_stats", "vsx_internal_derep_thresholds"]
DEREP_THRESHOLDS = 129             # VSX_DEREP_THRESHOLDS
# include/vsx_derep_prefix.h
OTUTAB_SYMBOLS = ["vsx_otutab_opts_default", "vsx_otutab", "vsx_otutab_result_free", "vsx_otutab_last_stats", "vsx_internal_otutab_host"]
DEREP_PREFIX_SYMBOLS = ["vsx_derep_prefix_opts_default", "vsx_derep_prefix", "vsx_derep_prefix_out_free", "vsx_derep_prefix_last_stats"]
# include/vsx_sintax.h
SINTAX_SYMBOLS = ["vsx_sintax_opts_default", "vsx_sintax", "vsx_sintax_result_free", "vsx_sintax_last_stats", "vsx_internal_sintax_host",
                  "vsx_internal_sintax_intern"]
SINTAX_RANKS, SINTAX_ROUNDS, SINTAX_NONE = 9, 100, 0xffffffff
# include/vsx_orient.h
ORIENT_SYMBOLS = ["vsx_orient_opts_default", "vsx_orient_result_free", "vsx_orient_last_stats", "vsx_orient", "vsx_internal_orient_host",
                  "vsx_internal_orient_matchcounts"]
# include/vsx_hitout.h
HITOUT_SYMBOLS = ["vsx_hitout_opts_default", "vsx_hits_render", "vsx_hit_text_free", "vsx_hits_render_last_stats",
                  "vsx_internal_hits_render_host"]
HITOUT_ROWS, HITOUT_SYMBOLS_ROW, HITOUT_SAM, HITOUT_NONE = 1, 2, 4, 0xFFFFFFFFFFFFFFFF      # VSX_HITOUT_ROWS / _SYMBOLS / _SAM / _NONE
# include/vsx_mask.h
MASK_SYMBOLS = ["vsx_fastx_mask_opts_default", "vsx_fastx_mask", "vsx_fastx_mask_out_free", "vsx_fastx_mask_last_stats"]
# include/vsx_getseqs.h
GETSEQS_SYMBOLS = ["vsx_getseqs_opts_default", "vsx_getseqs", "vsx_getseqs_out_free", "vsx_getseqs_last_stats"]
# include/vsx_cut.h
CUT_SYMBOLS = ["vsx_cut_opts_default", "vsx_cut_pattern_check", "vsx_cut", "vsx_cut_out_free", "vsx_cut_last_stats"]
# include/vsx_chimalns.h
CHIMALNS_SYMBOLS = ["vsx_chimalns_opts_default", "vsx_chimera_alns", "vsx_chimalns_out_free", "vsx_chimalns_last_stats",
                    "vsx_internal_chimalns_host", "vsx_internal_chimalns_device"]
CHIMALNS_Y, CHIMALNS_BORDERLINE, CHIMALNS_N, CHIMALNS_MAX_COLS = 1, 2, 4, 8192      # VSX_CHIMALNS_*
# include/vsx_sortby.h
SORTBY_SYMBOLS = ["vsx_sortby_opts_default", "vsx_sortby", "vsx_sortby_out_free", "vsx_sortby_last_stats"]
SORTBY_SIZE, SORTBY_LENGTH, SORTBY_LENGTH_ASC = 0, 1, 2                                 # VSX_SORTBY_*
SORTBY_MAX_ROUNDS, SORTBY_STAT_ROUNDS = 32, 8
# include/vsx_lca.h
LCA_SYMBOLS = ["vsx_lca_opts_default", "vsx_lca_index_create", "vsx_lca_index_destroy", "vsx_lca", "vsx_lca_result_free", "vsx_lca_last_stats",
               "vsx_internal_lca_host", "vsx_internal_lca_index_split"]
LCA_LEVELS, LCA_NONE = 9, 0xFFFFFFFF                                                     # VSX_LCA_LEVELS / _NONE
CUT_WANT_FWD, CUT_WANT_REV, CUT_WANT_REV_TEXT, CUT_WANT_DISCARDED_REV_TEXT = 1, 2, 4, 8
CUT_DEVICE_MAX_PATTERN = 64
MASK_WANT_TEXT, MASK_WANT_BITS = 1, 2                                                    # VSX_MASK_WANT_TEXT / _BITS
ORIENT_MAX_QLEN, ORIENT_CLASSES, ORIENT_CLASS_QLEN = 16384, 3, (512, 4096, 16384)      # VSX_ORIENT_MAX_QLEN, the count kernel's length classes


class Candidates(C.Structure):
    """vsx_candidates (include/vsx_search.h)"""
    _fields_ = [("n_queries", C.c_uint64), ("start", C.POINTER(C.c_uint64)), ("target", C.POINTER(C.c_uint32)),
                ("count", C.POINTER(C.c_uint32)), ("seconds", C.c_double), ("kernel_ms", C.c_double),
                ("index_build_ms", C.c_double), ("index_postings", C.c_uint64), ("postings_streamed", C.c_uint64),
                ("bytes_streamed", C.c_uint64)]


class SearchOpts(C.Structure):
    """vsx_search_opts (include/vsx_search.h): the Parameters fields the search path reads"""
    _fields_ = [("id", C.c_double), ("weak_id", C.c_double), ("maxaccepts", C.c_int64), ("maxrejects", C.c_int64),
                ("wordlength", C.c_int64), ("minwordmatches", C.c_int64), ("iddef", C.c_int32), ("soft_mask", C.c_int32),
                ("maxsubs", C.c_int64), ("maxgaps", C.c_int64), ("mincols", C.c_int64), ("maxdiffs", C.c_int64),
                ("query_cov", C.c_double), ("target_cov", C.c_double), ("maxid", C.c_double), ("mid", C.c_double),
                ("leftjust", C.c_int32), ("rightjust", C.c_int32),
                ("minqt", C.c_double), ("maxqt", C.c_double), ("minsl", C.c_double), ("maxsl", C.c_double),
                ("idprefix", C.c_int64), ("idsuffix", C.c_int64), ("selfid", C.c_int32), ("threads", C.c_int32),
                ("window", C.c_int64), ("gap_infinite", C.c_uint32), ("strand_both", C.c_uint32),
                ("maxqsize", C.c_int64), ("mintsize", C.c_int64), ("minsizeratio", C.c_double), ("maxsizeratio", C.c_double),
                ("self", C.c_int32), ("sizeorder", C.c_int32), ("cluster_unoise", C.c_int32), ("qmask", C.c_int32),
                ("unoise_alpha", C.c_double), ("hardmask", C.c_int32)]


class ChimeraOpts(C.Structure):
    """vsx_chimera_opts (include/vsx_search.h): searcher options + the UCHIME scoring parameters"""
    _fields_ = [("search", SearchOpts), ("minh", C.c_double), ("mindiv", C.c_double), ("mindiffs", C.c_int64),
                ("xn", C.c_double), ("dn", C.c_double), ("window", C.c_int64)]


class ChimeraResult(C.Structure):
    """vsx_chimera_result (include/vsx_search.h): one query's chimera_result_s with parents as database indices"""
    _fields_ = [("score", C.c_double), ("parent_a", C.c_uint32), ("parent_b", C.c_uint32), ("closest", C.c_uint32),
                ("status", C.c_int32), ("id_query_model", C.c_double), ("id_query_a", C.c_double), ("id_query_b", C.c_double),
                ("id_a_b", C.c_double), ("id_query_top", C.c_double), ("left_yes", C.c_int32), ("left_no", C.c_int32),
                ("left_abstain", C.c_int32), ("right_yes", C.c_int32), ("right_no", C.c_int32), ("right_abstain", C.c_int32),
                ("divergence", C.c_double), ("flag", C.c_char), ("pad", C.c_char * 7)]


class ChimeraStats(C.Structure):
    """vsx_chimera_stats (include/vsx_search.h)"""
    _fields_ = [("seconds_search", C.c_double), ("seconds_align", C.c_double), ("seconds_eval", C.c_double),
                ("seconds_total", C.c_double), ("windows", C.c_uint64), ("parts", C.c_uint64), ("pairs_aligned", C.c_uint64),
                ("sentinel_pairs", C.c_uint64), ("queries_kernel", C.c_uint64), ("queries_host", C.c_uint64)]


class ChimeraDenovoOpts(C.Structure):
    """vsx_chimera_denovo_opts (include/vsx_search.h): vsx_chimera_opts + variant (1 uchime, 2 uchime2, 3 uchime3) + abskew"""
    _fields_ = [("base", ChimeraOpts), ("variant", C.c_int32), ("abskew", C.c_double)]


class ChimeraDenovoStats(C.Structure):
    """vsx_chimera_denovo_stats (include/vsx_search.h)"""
    _fields_ = [("seconds_rank", C.c_double), ("seconds_members", C.c_double), ("seconds_search", C.c_double),
                ("seconds_align", C.c_double), ("seconds_eval", C.c_double), ("seconds_reconcile", C.c_double),
                ("seconds_total", C.c_double), ("windows", C.c_uint64), ("passes", C.c_uint64), ("passes_max", C.c_uint64),
                ("queries_reevaluated", C.c_uint64), ("parts", C.c_uint64), ("pairs_searched", C.c_uint64),
                ("pairs_aligned", C.c_uint64), ("sentinel_pairs", C.c_uint64), ("queries_kernel", C.c_uint64),
                ("queries_host", C.c_uint64)]


CHIMERAS_LONG_MAX_PARENTS = 20
CHIMERAS_LONG_MAX_QLEN = 2048      # VSX_CHIMERAS_LONG_MAX_QLEN
CHIMERAS_LONG_MAX_CAND = 64        # VSX_CHIMERAS_LONG_MAX_CAND


class ChimerasLongOpts(C.Structure):
    """vsx_chimeras_long_opts (include/vsx_search.h): searcher options + the --chimeras_denovo parameters"""
    _fields_ = [("search", SearchOpts), ("parts", C.c_int32), ("parents_max", C.c_int32), ("length_min", C.c_int32),
                ("pad", C.c_int32), ("diff_pct", C.c_double), ("abskew", C.c_double), ("window", C.c_int64)]


class ChimerasLongResult(C.Structure):
    """vsx_chimeras_long_result (include/vsx_search.h)"""
    _fields_ = [("status", C.c_int32), ("flag", C.c_char), ("pad", C.c_char * 3), ("n_parents", C.c_int32), ("alnlen", C.c_int32),
                ("parent", C.c_uint32 * CHIMERAS_LONG_MAX_PARENTS), ("start", C.c_int32 * CHIMERAS_LONG_MAX_PARENTS),
                ("len", C.c_int32 * CHIMERAS_LONG_MAX_PARENTS), ("id_query_parent", C.c_double * CHIMERAS_LONG_MAX_PARENTS),
                ("id_query_top", C.c_double), ("divergence", C.c_double)]


class ChimalnsOpts(C.Structure):
    """vsx_chimalns_opts (include/vsx_chimalns.h)"""
    _fields_ = [("xn", C.c_double), ("dn", C.c_double), ("alignwidth", C.c_int32), ("select", C.c_uint32), ("window", C.c_int64),
                ("threads", C.c_int32), ("pad", C.c_int32)]


class ChimalnsOut(C.Structure):
    """vsx_chimalns_out (include/vsx_chimalns.h)"""
    _fields_ = [("n", C.c_uint64), ("text_bytes", C.c_uint64), ("n_lines", C.c_uint64), ("record", C.POINTER(C.c_uint64)),
                ("alnlen", C.POINTER(C.c_uint32)), ("text_off", C.POINTER(C.c_uint64)), ("text", C.POINTER(C.c_char)),
                ("line_first", C.POINTER(C.c_uint64)), ("line_end", C.POINTER(C.c_uint32)), ("best_i", C.POINTER(C.c_int32)),
                ("h", C.POINTER(C.c_double)), ("counts", C.POINTER(C.c_int32))]


class ChimalnsStats(C.Structure):
    """vsx_chimalns_stats (include/vsx_chimalns.h)"""
    _fields_ = [("seconds_align", C.c_double), ("seconds_kernel", C.c_double), ("seconds_download", C.c_double),
                ("seconds_host", C.c_double), ("seconds_total", C.c_double), ("windows", C.c_uint64), ("records_selected", C.c_uint64),
                ("records_kernel", C.c_uint64), ("records_host", C.c_uint64), ("sentinel_pairs", C.c_uint64),
                ("host_long_query", C.c_uint64), ("host_long_alignment", C.c_uint64), ("host_forced", C.c_uint64)]


class MergeOpts(C.Structure):
    """vsx_merge_opts (include/vsx_merge.h): the Parameters fields the merge core reads"""
    _fields_ = [("fastq_ascii", C.c_int64), ("fastq_qmin", C.c_int64), ("fastq_qmax", C.c_int64), ("fastq_qminout", C.c_int64),
                ("fastq_qmaxout", C.c_int64), ("fastq_minovlen", C.c_int64), ("fastq_maxdiffs", C.c_int64),
                ("fastq_maxdiffpct", C.c_double), ("fastq_minmergelen", C.c_int64), ("fastq_maxmergelen", C.c_int64),
                ("fastq_maxee", C.c_double), ("fastq_truncqual", C.c_int64), ("fastq_maxns", C.c_int64),
                ("fastq_minlen", C.c_int64), ("fastq_maxlen", C.c_int64), ("fastq_allowmergestagger", C.c_int32),
                ("pad", C.c_int32), ("window", C.c_int64)]


class MergeRecord(C.Structure):
    """vsx_merge_record (include/vsx_merge.h)"""
    _fields_ = [("merged", C.c_int32), ("reason", C.c_int32), ("fwd_trunc", C.c_int32), ("rev_trunc", C.c_int32),
                ("merged_length", C.c_int32), ("overlap_length", C.c_int32), ("fwd_errors", C.c_int32), ("rev_errors", C.c_int32),
                ("ee_merged", C.c_double), ("ee_fwd", C.c_double), ("ee_rev", C.c_double), ("blob_off", C.c_uint64)]


class MergeOut(C.Structure):
    """vsx_merge_out (include/vsx_merge.h)"""
    _fields_ = [("n", C.c_uint64), ("rec", C.POINTER(MergeRecord)), ("seq_blob", C.POINTER(C.c_char)),
                ("qual_blob", C.POINTER(C.c_char)), ("blob_bytes", C.c_uint64)]


class MergeStats(C.Structure):
    """vsx_merge_stats (include/vsx_merge.h)"""
    _fields_ = [("seconds_stage", C.c_double), ("seconds_kernel", C.c_double), ("seconds_unpack", C.c_double),
                ("seconds_total", C.c_double), ("pairs", C.c_uint64), ("windows", C.c_uint64), ("diagonals_scored", C.c_uint64),
                ("pairs_host", C.c_uint64)]


class FilterOpts(C.Structure):
    """vsx_fastx_filter_opts (include/vsx_filter.h): the Parameters fields the filter's analysis reads"""
    _fields_ = [(n, C.c_int64) for n in ("ascii", "qmin", "qmax", "stripleft", "stripright", "trunclen", "trunclen_keep", "truncqual",
                                         "minqual", "minlen", "maxlen", "maxns", "minsize", "maxsize")] + \
               [(n, C.c_double) for n in ("maxee", "maxee_rate", "truncee", "truncee_rate")] + [("window", C.c_int64)]


class FilterReads(C.Structure):
    """vsx_fastx_reads (include/vsx_filter.h): one side of the input"""
    _fields_ = [("seq", C.c_void_p), ("qual", C.c_void_p), ("bytes", C.c_uint64), ("off", C.c_void_p), ("len", C.c_void_p),
                ("abundance", C.c_void_p)]


class FilterRecord(C.Structure):
    """vsx_fastx_filter_record (include/vsx_filter.h)"""
    _fields_ = [("start", C.c_int32), ("length", C.c_int32), ("ee", C.c_double), ("discarded", C.c_uint8), ("truncated", C.c_uint8),
                ("pad", C.c_uint8 * 6)]


class FilterOut(C.Structure):
    """vsx_fastx_filter_out (include/vsx_filter.h)"""
    _fields_ = [("n", C.c_uint64), ("fwd", C.POINTER(FilterRecord)), ("rev", C.POINTER(FilterRecord)),
                ("pair_discarded", C.POINTER(C.c_uint8)), ("kept", C.c_uint64), ("kept_truncated", C.c_uint64), ("discarded", C.c_uint64)]


class FilterStats(C.Structure):
    """vsx_fastx_filter_stats (include/vsx_filter.h)"""
    _fields_ = [("seconds_stage", C.c_double), ("seconds_h2d", C.c_double), ("seconds_kernel", C.c_double),
                ("seconds_d2h_output", C.c_double), ("seconds_total", C.c_double), ("reads", C.c_uint64), ("windows", C.c_uint64),
                ("reads_host", C.c_uint64)]


class EEStatsOpts(C.Structure):
    """vsx_fastq_eestats_opts (include/vsx_eestats.h)"""
    _fields_ = [(n, C.c_int64) for n in ("ascii", "qmin", "qmax", "len_shortest", "len_longest", "len_increment")] + \
               [("ee_cutoffs", C.POINTER(C.c_double)), ("n_ee_cutoffs", C.c_uint64), ("want", C.c_uint32), ("pad", C.c_uint32),
                ("window", C.c_int64), ("hist_budget", C.c_uint64)]


class EEStatsOut(C.Structure):
    """vsx_fastq_eestats_out (include/vsx_eestats.h)"""
    _fields_ = [("n", C.c_uint64), ("symbols", C.c_uint64), ("len_min", C.c_uint64), ("len_max", C.c_uint64),
                ("qual_cols", C.c_uint64), ("reads_at", C.POINTER(C.c_uint64)), ("qual_counts", C.POINTER(C.c_uint64)),
                ("sum_ee", C.POINTER(C.c_double)), ("ee_bins", C.POINTER(C.c_int64)), ("len_steps", C.c_uint64),
                ("n_ee_cutoffs", C.c_uint64), ("cutoff_counts", C.POINTER(C.c_uint64))]


class EEStatsStats(C.Structure):
    """vsx_fastq_eestats_stats (include/vsx_eestats.h)"""
    _fields_ = [(n, C.c_double) for n in ("seconds_stage", "seconds_h2d", "seconds_walk", "seconds_sum", "seconds_quantile",
                                          "seconds_d2h_output", "seconds_total")] + \
               [(n, C.c_uint64) for n in ("reads", "windows", "reads_host")]


class FastqStatsOpts(C.Structure):
    """vsx_fastq_stats_opts (include/vsx_fastq_stats.h)"""
    _fields_ = [(n, C.c_int64) for n in ("ascii", "qmin", "qmax", "window")]


class FastqStatsOut(C.Structure):
    """vsx_fastq_stats_out (include/vsx_fastq_stats.h)"""
    _fields_ = [("n", C.c_uint64), ("symbols", C.c_uint64), ("len_min", C.c_uint64), ("len_max", C.c_uint64),
                ("length_counts", C.POINTER(C.c_uint64)), ("symbol_counts", C.POINTER(C.c_uint64)), ("sum_ee", C.POINTER(C.c_double)),
                ("ee_counts", C.POINTER(C.c_uint64)), ("q_counts", C.POINTER(C.c_uint64))]


class FastqStatsStats(C.Structure):
    """vsx_fastq_stats_stats (include/vsx_fastq_stats.h)"""
    _fields_ = [(n, C.c_double) for n in ("seconds_stage", "seconds_h2d", "seconds_walk", "seconds_sum", "seconds_d2h_output",
                                          "seconds_total")] + \
               [(n, C.c_uint64) for n in ("reads", "windows", "reads_host")]


class FastqCharsOpts(C.Structure):
    """vsx_fastq_chars_opts (include/vsx_fastq_stats.h)"""
    _fields_ = [("tail", C.c_int64), ("window", C.c_int64)]


class FastqCharsOut(C.Structure):
    """vsx_fastq_chars_out (include/vsx_fastq_stats.h)"""
    _fields_ = [("n", C.c_uint64), ("total_chars", C.c_uint64), ("seq_counts", C.c_uint64 * 256), ("qual_counts", C.c_uint64 * 256),
                ("tail_counts", C.c_uint64 * 256), ("maxrun", C.c_int32 * 256), ("qmin_n", C.c_uint8), ("qmax_n", C.c_uint8),
                ("pad", C.c_uint8 * 6)]


class FastqCharsStats(C.Structure):
    """vsx_fastq_chars_stats (include/vsx_fastq_stats.h)"""
    _fields_ = [(n, C.c_double) for n in ("seconds_stage", "seconds_h2d", "seconds_kernel", "seconds_d2h_output", "seconds_total")] + \
               [(n, C.c_uint64) for n in ("reads", "windows", "reads_host")]


class DerepOpts(C.Structure):
    """vsx_derep_opts (include/vsx_derep.h)"""
    _fields_ = [(n, C.c_int32) for n in ("strand_both", "by_label", "want_quality", "qout_max")] + \
               [(n, C.c_int64) for n in ("minseqlength", "maxseqlength", "minuniquesize", "maxuniquesize", "topn", "ascii", "asciiout",
                                         "qminout", "qmaxout", "window")]


class DerepOut(C.Structure):
    """vsx_derep_out (include/vsx_derep.h)"""
    _fields_ = [(n, C.c_uint64) for n in ("n", "kept", "nucleotides", "shortest", "longest", "discarded_short", "discarded_long",
                                          "sumsize", "maxsize")] + \
               [("median", C.c_double), ("selected", C.c_uint64), ("n_clusters", C.c_uint64)] + \
               [(n, C.POINTER(C.c_uint64)) for n in ("rep", "size", "count", "member_start", "member")] + \
               [("strand", C.POINTER(C.c_uint8)), ("qual_off", C.POINTER(C.c_uint64)), ("qual_blob", C.POINTER(C.c_char)),
                ("qual_bytes", C.c_uint64)]


class DerepStats(C.Structure):
    """vsx_derep_stats (include/vsx_derep.h)"""
    _fields_ = [(n, C.c_double) for n in ("seconds_stage", "seconds_h2d", "seconds_hash", "seconds_group", "seconds_account",
                                          "seconds_quality", "seconds_output", "seconds_total")] + \
               [(n, C.c_uint64) for n in ("windows", "slots_visited", "candidates_compared", "reads_host")]


class DerepPrefixOpts(C.Structure):
    """vsx_derep_prefix_opts (include/vsx_derep_prefix.h)"""
    _fields_ = [("sizein", C.c_int32), ("pad", C.c_int32)] + \
               [(n, C.c_int64) for n in ("minseqlength", "maxseqlength", "minuniquesize", "maxuniquesize", "topn", "window")]


class DerepPrefixOut(C.Structure):
    """vsx_derep_prefix_out (include/vsx_derep_prefix.h)"""
    _fields_ = [(n, C.c_uint64) for n in ("n", "kept", "nucleotides", "shortest", "longest", "discarded_short", "discarded_long",
                                          "sumsize", "maxsize")] + \
               [("median", C.c_double), ("selected", C.c_uint64), ("n_clusters", C.c_uint64)] + \
               [(n, C.POINTER(C.c_uint64)) for n in ("rep", "size", "count", "member_start", "member", "rank")]


class DerepPrefixStats(C.Structure):
    """vsx_derep_prefix_stats (include/vsx_derep_prefix.h)"""
    _fields_ = [(n, C.c_double) for n in ("seconds_rank", "seconds_stage", "seconds_h2d", "seconds_hash", "seconds_group", "seconds_claim",
                                          "seconds_resolve", "seconds_output", "seconds_total")] + \
               [(n, C.c_uint64) for n in ("windows", "nodes", "distinct_lengths", "probes", "candidates_compared", "reads_host",
                                          "host_no_context", "host_environment", "host_read_count", "host_memory")]


class Labels(C.Structure):
    """vsx_labels (include/vsx_otutab.h): label k = blob[offsets[k] .. offsets[k] + lengths[k])"""
    _fields_ = [("n", C.c_uint64), ("blob", C.c_void_p), ("bytes", C.c_uint64), ("offsets", C.c_void_p), ("lengths", C.c_void_p)]


class OtutabOpts(C.Structure):
    """vsx_otutab_opts (include/vsx_otutab.h)"""
    _fields_ = [("threads", C.c_int32), ("pad", C.c_int32)]


class OtutabResult(C.Structure):
    """vsx_otutab_result (include/vsx_otutab.h)"""
    _fields_ = [(n, C.c_uint64) for n in ("n_queries", "n_targets", "n_samples", "n_otus")] + [("has_tax", C.c_int32), ("pad", C.c_int32)] + \
               [f for s in ("sample", "otu", "tax") for f in ((s + "_blob", C.POINTER(C.c_char)), (s + "_bytes", C.c_uint64),
                                                              (s + "_off", C.POINTER(C.c_uint64)), (s + "_len", C.POINTER(C.c_uint32)))] + \
               [("n_cells", C.c_uint64), ("nz_otu", C.POINTER(C.c_uint32)), ("nz_sample", C.POINTER(C.c_uint32)),
                ("nz_count", C.POINTER(C.c_uint64)), ("q_sample", C.POINTER(C.c_uint32)), ("t_otu", C.POINTER(C.c_uint32))]


class OtutabStats(C.Structure):
    """vsx_otutab_stats (include/vsx_otutab.h)"""
    _fields_ = [(n, C.c_double) for n in ("seconds_stage", "seconds_scan", "seconds_group", "seconds_rank", "seconds_accumulate",
                                          "seconds_output", "seconds_total")] + \
               [(n, C.c_uint64) for n in ("query_groups", "target_groups", "targets_in_adds", "adds_sorted", "labels_device", "labels_host",
                                          "host_no_context", "host_environment", "host_label_count", "host_memory")]


class GetseqsOpts(C.Structure):
    """vsx_getseqs_opts (include/vsx_getseqs.h)"""
    _fields_ = [("mode", C.c_int32), ("substr", C.c_int32), ("field", C.c_void_p), ("field_len", C.c_uint64), ("subseq_start", C.c_int64),
                ("subseq_end", C.c_int64), ("window", C.c_int64), ("threads", C.c_int32), ("pad", C.c_int32)]


class GetseqsOut(C.Structure):
    """vsx_getseqs_out (include/vsx_getseqs.h); rec: n records of four uint32 (matched, ordinal, start, length)"""
    _fields_ = [("n", C.c_uint64), ("rec", C.c_void_p), ("kept", C.c_uint64), ("discarded", C.c_uint64)]


class GetseqsStats(C.Structure):
    """vsx_getseqs_stats (include/vsx_getseqs.h)"""
    _fields_ = [(n, C.c_double) for n in ("seconds_stage", "seconds_table", "seconds_match", "seconds_ordinals", "seconds_output",
                                          "seconds_total")] + \
               [(n, C.c_uint64) for n in ("headers_device", "headers_host", "host_no_context", "host_environment", "host_count", "host_memory",
                                          "host_needle_length", "host_header_length", "host_lengths", "labels_in_table", "distinct_lengths",
                                          "table_slots", "probes", "verifications")]


class CutOpts(C.Structure):
    """vsx_cut_opts (include/vsx_cut.h)"""
    _fields_ = [("pattern", C.c_char_p), ("pattern_len", C.c_uint64), ("want", C.c_uint32), ("threads", C.c_int32), ("window", C.c_int64)]


class CutOut(C.Structure):
    """vsx_cut_out (include/vsx_cut.h); fwd / rev: records of (uint64 seq, uint32 start, uint32 length)"""
    _fields_ = [("n", C.c_uint64), ("matches", C.c_void_p), ("n_fwd", C.c_uint64), ("fwd", C.c_void_p), ("n_rev", C.c_uint64), ("rev", C.c_void_p),
                ("n_uncut", C.c_uint64), ("uncut", C.c_void_p), ("text", C.c_void_p), ("text_bytes", C.c_uint64), ("rev_off", C.c_void_p),
                ("discarded_off", C.c_void_p), ("cut", C.c_uint64), ("uncut_total", C.c_uint64), ("total_matches", C.c_uint64)]


class CutStats(C.Structure):
    """vsx_cut_stats (include/vsx_cut.h)"""
    _fields_ = [(n, C.c_double) for n in ("seconds_stage", "seconds_h2d", "seconds_match", "seconds_rank", "seconds_fragments", "seconds_emit",
                                          "seconds_output", "seconds_total")] + \
               [(n, C.c_uint64) for n in ("sequences", "symbols", "blocks", "items", "tile", "pattern_length", "host_no_context",
                                          "host_environment", "host_count", "host_memory", "host_pattern_length")]


class SortbyOpts(C.Structure):
    """vsx_sortby_opts (include/vsx_sortby.h)"""
    _fields_ = [("order", C.c_int32), ("threads", C.c_int32), ("minsize", C.c_int64), ("maxsize", C.c_int64), ("topn", C.c_int64)]


class SortbyOut(C.Structure):
    """vsx_sortby_out (include/vsx_sortby.h)"""
    _fields_ = [("n", C.c_uint64), ("n_kept", C.c_uint64), ("n_out", C.c_uint64), ("order", C.c_void_p), ("median", C.c_double)]


class SortbyStats(C.Structure):
    """vsx_sortby_stats (include/vsx_sortby.h)"""
    _fields_ = [(n, C.c_double) for n in ("seconds_stage", "seconds_h2d", "seconds_numeric", "seconds_refine", "seconds_host_finish",
                                          "seconds_output", "seconds_total")] + \
               [(n, C.c_uint64) for n in ("items", "kept", "label_bytes", "rounds", "max_rounds", "active_numeric")] + \
               [("active", C.c_uint64 * SORTBY_STAT_ROUNDS)] + \
               [(n, C.c_uint64) for n in ("capped_items", "host_no_context", "host_environment", "host_count", "host_memory",
                                          "host_long_prefix")]


class LcaOpts(C.Structure):
    """vsx_lca_opts (include/vsx_lca.h)"""
    _fields_ = [("lca_cutoff", C.c_double), ("maxhits", C.c_int64), ("top_hits_only", C.c_int32), ("threads", C.c_int32), ("window", C.c_uint64)]


class LcaResult(C.Structure):
    """vsx_lca_result (include/vsx_lca.h)"""
    _fields_ = [("n_queries", C.c_uint64)] + [(n, C.POINTER(C.c_uint32)) for n in ("n_top", "depth", "matches", "target", "start", "len")]


class LcaStats(C.Structure):
    """vsx_lca_stats (include/vsx_lca.h)"""
    _fields_ = [(n, C.c_double) for n in ("seconds_index_stage", "seconds_index_split", "seconds_index_number", "seconds_index_total",
                                          "seconds_stage", "seconds_h2d", "seconds_vote", "seconds_d2h", "seconds_output", "seconds_total")] + \
               [(n, C.c_uint64) for n in ("labels", "labels_device", "labels_host", "windows", "queries_device", "queries_host", "hits_device",
                                          "hits_host", "host_no_context", "host_environment", "host_count", "host_memory", "host_collision")]


class HitoutOpts(C.Structure):
    """vsx_hitout_opts (include/vsx_hitout.h)"""
    _fields_ = [("want", C.c_uint32), ("threads", C.c_int32), ("window", C.c_uint64)]


class HitText(C.Structure):
    """vsx_hit_text (include/vsx_hitout.h)"""
    _fields_ = [("n_queries", C.c_uint64), ("n_hits", C.c_uint64), ("want", C.c_uint32), ("both", C.c_uint32),
                ("row_blob", C.POINTER(C.c_char)), ("row_bytes", C.c_uint64), ("row_len", C.POINTER(C.c_uint32)),
                ("qrow_off", C.POINTER(C.c_uint64)), ("trow_off", C.POINTER(C.c_uint64)),
                ("sym_off", C.POINTER(C.c_uint64)), ("aln_off", C.POINTER(C.c_uint64)),
                ("md_blob", C.POINTER(C.c_char)), ("md_bytes", C.c_uint64), ("md_off", C.POINTER(C.c_uint64)), ("md_len", C.POINTER(C.c_uint32)),
                ("qtext", C.POINTER(C.c_char)), ("qtext_bytes", C.c_uint64), ("qplus_off", C.POINTER(C.c_uint64)),
                ("qminus_off", C.POINTER(C.c_uint64))]


class HitoutStats(C.Structure):
    """vsx_hitout_stats (include/vsx_hitout.h)"""
    _fields_ = [(n, C.c_double) for n in ("seconds_mask", "seconds_stage", "seconds_h2d", "seconds_rows", "seconds_md_count",
                                          "seconds_md_fill", "seconds_d2h", "seconds_host", "seconds_total")] + \
               [(n, C.c_uint64) for n in ("windows", "hits_device", "hits_host", "db_text_uploaded", "host_no_context",
                                          "host_environment", "host_hit_count", "host_memory")]


class SeqMeta(C.Structure):
    """vsx_seq_meta (include/vsx_search.h): abundances / labels of a set of sequences"""
    _fields_ = [("abundance", C.POINTER(C.c_uint64)), ("label", C.POINTER(C.c_char_p))]


class Hit(C.Structure):
    _fields_ = [("query", C.c_uint32), ("target", C.c_uint32), ("count", C.c_uint32),
                ("accepted", C.c_uint8), ("weak", C.c_uint8), ("used_fallback", C.c_uint8), ("strand", C.c_uint8),
                ("nwscore", C.c_int32), ("nwdiff", C.c_int32), ("nwgaps", C.c_int32), ("nwindels", C.c_int32),
                ("nwalignmentlength", C.c_int32), ("matches", C.c_int32), ("mismatches", C.c_int32),
                ("internal_alignmentlength", C.c_int32), ("internal_gaps", C.c_int32), ("internal_indels", C.c_int32),
                ("trim_q_left", C.c_int32), ("trim_q_right", C.c_int32), ("trim_t_left", C.c_int32), ("trim_t_right", C.c_int32),
                ("shortest", C.c_int32), ("longest", C.c_int32),
                ("nwid", C.c_double), ("id", C.c_double), ("id0", C.c_double), ("id1", C.c_double), ("id2", C.c_double),
                ("id3", C.c_double), ("id4", C.c_double), ("cigar_off", C.c_uint64)]


class Hits(C.Structure):
    _fields_ = [("n_queries", C.c_uint64), ("n_hits", C.c_uint64), ("first", C.POINTER(C.c_uint64)),
                ("hit", C.POINTER(Hit)), ("cigar_blob", C.POINTER(C.c_char)), ("cigar_bytes", C.c_uint64),
                ("pairs_aligned", C.c_uint64), ("cells_aligned", C.c_uint64), ("stages", C.c_uint64),
                ("sentinel_pairs", C.c_uint64), ("seconds_kmer", C.c_double), ("seconds_align", C.c_double),
                ("seconds_total", C.c_double)]


class ExactStats(C.Structure):
    """vsx_exact_stats (include/vsx_search.h)"""
    _fields_ = [(n, C.c_double) for n in ("seconds_index", "seconds_stage", "seconds_kernel", "seconds_marshal", "seconds_total")] + \
               [(n, C.c_uint64) for n in ("windows", "queries_device", "queries_host", "strands_probed", "slots_visited",
                                          "candidates_compared", "hits", "queries_matched")]


class SintaxOpts(C.Structure):
    """vsx_sintax_opts (include/vsx_sintax.h)"""
    _fields_ = [("strand_both", C.c_int32), ("sintax_random", C.c_int32), ("want_candidates", C.c_int32), ("pad", C.c_int32),
                ("randseed", C.c_uint64), ("window", C.c_int64)]


class SintaxRecord(C.Structure):
    _fields_ = [("strand", C.c_int32), ("classified", C.c_int32), ("boot_count", C.c_uint32 * 2), ("best_count", C.c_uint32 * 2),
                ("rank_seq", C.c_uint32 * SINTAX_RANKS), ("rank_count", C.c_uint32 * SINTAX_RANKS)]


class SintaxResult(C.Structure):
    _fields_ = [("n_queries", C.c_uint64), ("n_classified", C.c_uint64), ("rec", C.POINTER(SintaxRecord)),
                ("candidates", C.POINTER(C.c_uint32))]


class SintaxStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("queries_device", "queries_host_random", "queries_host_wordlength", "queries_host_dblen",
                                          "queries_host_forced", "windows", "strands_sampled", "rounds_counted", "tiles")] + \
               [(n, C.c_double) for n in ("seconds_stage", "seconds_sample", "seconds_count", "seconds_vote", "seconds_output",
                                          "seconds_index", "seconds_total")]


class OrientOpts(C.Structure):
    """vsx_orient_opts (include/vsx_orient.h)"""
    _fields_ = [("qmask", C.c_int32), ("want_text", C.c_int32), ("window", C.c_int64)]


class OrientRecord(C.Structure):
    _fields_ = [("count_fwd", C.c_uint32), ("count_rev", C.c_uint32), ("strand", C.c_int32)]


class OrientResult(C.Structure):
    _fields_ = [("n_queries", C.c_uint64), ("n_fwd", C.c_uint64), ("n_rev", C.c_uint64), ("n_none", C.c_uint64),
                ("rec", C.POINTER(OrientRecord)), ("text", C.c_void_p), ("qual", C.c_void_p)]


class OrientStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("queries_device", "queries_host_wordlength", "queries_host_qlen", "queries_host_forced")] + \
               [("queries_class", C.c_uint64 * ORIENT_CLASSES)] + \
               [(n, C.c_uint64) for n in ("windows", "words_distinct", "build_chunks", "build_keys")] + \
               [(n, C.c_double) for n in ("seconds_build", "seconds_stage", "seconds_count", "seconds_emit", "seconds_output",
                                          "seconds_total")]


class MaskOpts(C.Structure):
    """vsx_fastx_mask_opts (include/vsx_mask.h)"""
    _fields_ = [("qmask", C.c_int32), ("hardmask", C.c_int32), ("min_unmasked_pct", C.c_double), ("max_unmasked_pct", C.c_double),
                ("want", C.c_uint32), ("pad", C.c_uint32), ("window", C.c_int64)]


class MaskRecord(C.Structure):
    _fields_ = [("unmasked", C.c_uint32), ("verdict", C.c_uint32)]


class MaskOut(C.Structure):
    _fields_ = [("n", C.c_uint64), ("rec", C.POINTER(MaskRecord)), ("text", C.c_void_p), ("bits", C.c_void_p), ("text_bytes", C.c_uint64),
                ("kept", C.c_uint64), ("discarded_less", C.c_uint64), ("discarded_more", C.c_uint64)]


class MaskStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("seconds_stage", "seconds_h2d", "seconds_mask", "seconds_apply", "seconds_d2h_output",
                                          "seconds_total")] + \
               [(n, C.c_uint64) for n in ("sequences", "sequences_short", "sequences_long", "sequences_device_plain", "sequences_host_forced",
                                          "sequences_host_memory", "sequences_host_long", "windows", "dust_windows", "long_min", "segment")]


class Scoring(C.Structure):
    """vsx_scoring: the 14 post-fixup values in search16_init order + n_mismatch."""
    _fields_ = [(n, C.c_int64) for n in (
        "match", "mismatch", "gap_open_query_left", "gap_open_target_left", "gap_open_query_interior",
        "gap_open_target_interior", "gap_open_query_right", "gap_open_target_right",
        "gap_ext_query_left", "gap_ext_target_left", "gap_ext_query_interior", "gap_ext_target_interior",
        "gap_ext_query_right", "gap_ext_target_right")] + [("n_mismatch", C.c_int32)]


class Results(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("score", C.POINTER(C.c_int16)), ("aligned", C.POINTER(C.c_uint16)),
                ("matches", C.POINTER(C.c_uint16)), ("mismatches", C.POINTER(C.c_uint16)),
                ("gaps", C.POINTER(C.c_uint16)), ("cigar_off", C.POINTER(C.c_uint64)),
                ("cigar_blob", C.POINTER(C.c_char)), ("cigar_bytes", C.c_uint64), ("verdict", C.POINTER(C.c_uint8))]


class Ranked(C.Structure):
    """vsx_ranked (include/vsx.h)"""
    _fields_ = [("n_pairs", C.c_uint64), ("n_hits", C.c_uint64), ("pair", C.POINTER(C.c_uint32)), ("score", C.POINTER(C.c_int16)),
                ("aligned", C.POINTER(C.c_uint16)), ("matches", C.POINTER(C.c_uint16)), ("mismatches", C.POINTER(C.c_uint16)),
                ("gaps", C.POINTER(C.c_uint16)), ("verdict", C.POINTER(C.c_uint8)), ("id", C.POINTER(C.c_double)),
                ("cigar_off", C.POINTER(C.c_uint64)), ("cigar_blob", C.POINTER(C.c_char)), ("cigar_bytes", C.c_uint64),
                ("n_undecided", C.c_uint64), ("undecided", C.POINTER(C.c_uint32))]


class Filter(C.Structure):
    """vsx_filter (include/vsx.h): device-side align_trim + search_acceptable_aligned"""
    _fields_ = [("iddef", C.c_int32), ("leftjust", C.c_int32), ("rightjust", C.c_int32), ("pad", C.c_int32),
                ("id", C.c_double), ("weak_id", C.c_double), ("maxid", C.c_double), ("mid", C.c_double),
                ("query_cov", C.c_double), ("target_cov", C.c_double),
                ("maxsubs", C.c_int64), ("maxgaps", C.c_int64), ("mincols", C.c_int64), ("maxdiffs", C.c_int64)]


class PlanInfo(C.Structure):
    """vsx_plan_info (include/vsx.h)"""
    _fields_ = [("tasks", C.c_uint64), ("tasks_tilted", C.c_uint64), ("tasks_tracked", C.c_uint64),
                ("rows_dominant", C.c_uint32), ("chunks", C.c_uint32), ("tasks_max3", C.c_uint64),
                ("tasks_sparse", C.c_uint64), ("waves", C.c_uint64), ("tasks_pair", C.c_uint64),
                ("tasks_split", C.c_uint64)]


class Timing(C.Structure):
    _fields_ = [("forward_ms", C.c_float), ("traceback_ms", C.c_float), ("total_ms", C.c_float),
                ("forward_launches", C.c_uint32), ("traceback_launches", C.c_uint32),
                ("cells", C.c_uint64), ("dir_bytes", C.c_uint64), ("steps_skipped", C.c_uint64)]


class ClusterOut(C.Structure):
    _fields_ = [("n", C.c_uint64), ("n_clusters", C.c_uint64), ("clusterno", C.POINTER(C.c_uint32)), ("hits", Hits)]


class MsaOut(C.Structure):
    _fields_ = [("alnlen", C.c_uint64), ("n_rows", C.c_uint64), ("conslen", C.c_uint64), ("rows", C.POINTER(C.c_char)),
                ("consensus", C.POINTER(C.c_char)), ("profile", C.POINTER(C.c_uint64))]


_lib = None


def load():
    """dlopen libvsx.so and declare the prototypes.  Raises if the extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; "
            "g.build()' or make -C vsearch_amd/csrc). vsearch_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    lib.vsx_version_string.restype = C.c_char_p
    lib.vsx_last_error.restype = C.c_char_p
    lib.vsx_device_count.restype = C.c_int
    lib.vsx_create.argtypes = [C.POINTER(vp), C.POINTER(Scoring), C.c_int]
    lib.vsx_destroy.argtypes = [vp]
    lib.vsx_destroy.restype = None
    lib.vsx_seqset_create.argtypes = [vp, C.POINTER(vp), C.c_uint64, vp, C.c_uint64, vp, vp]
    lib.vsx_seqset_create_both_strands.argtypes = [vp, C.POINTER(vp), C.c_uint64, vp, C.c_uint64, vp, vp]
    lib.vsx_seqset_create_from_device.argtypes = [vp, C.POINTER(vp), C.c_uint64, vp, C.c_uint64, vp, vp]
    lib.vsx_seqset_destroy.argtypes = [vp]
    lib.vsx_seqset_destroy.restype = None
    lib.vsx_seqset_count.argtypes = [vp]
    lib.vsx_seqset_count.restype = C.c_uint64
    lib.vsx_plan_create.argtypes = [vp, C.POINTER(vp), vp, vp, C.c_uint64, vp, vp, C.c_uint64]
    lib.vsx_plan_run.argtypes = [vp]
    lib.vsx_plan_sync.argtypes = [vp, C.POINTER(Timing)]
    lib.vsx_plan_fetch.argtypes = [vp, C.POINTER(Results)]
    lib.vsx_plan_export_hits.argtypes = [vp, vp, C.c_uint64]
    lib.vsx_plan_export_runs.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.vsx_cigar_from_runs.argtypes = [vp, C.c_uint32, vp, C.c_uint64]
    lib.vsx_cigar_from_runs.restype = C.c_int64
    lib.vsx_plan_destroy.argtypes = [vp]
    lib.vsx_plan_destroy.restype = None
    lib.vsx_plan_describe.argtypes = [vp, C.POINTER(PlanInfo)]
    lib.vsx_internal_settle_counts.argtypes = [vp, C.POINTER(C.c_uint64 * 2)]
    lib.vsx_internal_poison_byte.restype = C.c_int                   # VSX_POISON: -1 off, else the fill byte (tests)
    lib.vsx_internal_msa_row_tile.restype = C.c_uint32               # rows of one profile tile of the device MSA (tests)
    lib.vsx_internal_ckpt_bytes_estimate.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32]
    lib.vsx_internal_ckpt_bytes_estimate.restype = C.c_uint64
    lib.vsx_internal_export_host.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.vsx_align_pairs.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, C.POINTER(Results)]
    lib.vsx_align_pairs_filtered.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, C.POINTER(Filter), C.POINTER(Results)]
    lib.vsx_align_pairs_ranked.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, C.POINTER(Filter), C.c_int, C.POINTER(Ranked)]
    lib.vsx_ranked_free.argtypes = [C.POINTER(Ranked)]
    lib.vsx_ranked_free.restype = None
    lib.vsx_plan_set_filter.argtypes = [vp, C.POINTER(Filter)]
    lib.vsx_results_free.argtypes = [C.POINTER(Results)]
    lib.vsx_results_free.restype = None
    lib.vsx_search_opts_default.argtypes = [C.POINTER(SearchOpts)]
    lib.vsx_search_opts_default.restype = None
    lib.vsx_searcher_create.argtypes = [vp, C.POINTER(vp), C.POINTER(SearchOpts), C.c_uint64, vp, C.c_uint64, vp, vp]
    lib.vsx_searcher_destroy.argtypes = [vp]
    lib.vsx_searcher_destroy.restype = None
    lib.vsx_search_batch.argtypes = [vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.POINTER(Hits)]
    lib.vsx_search_batch_meta.argtypes = [vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.POINTER(SeqMeta), C.POINTER(Hits)]
    lib.vsx_searcher_set_meta.argtypes = [vp, C.POINTER(SeqMeta)]
    lib.vsx_hits_free.argtypes = [C.POINTER(Hits)]
    lib.vsx_hits_free.restype = None
    lib.vsx_search_candidates.argtypes = [vp, C.c_char_p, C.c_uint32, vp, vp, C.c_uint64]
    lib.vsx_search_candidates.restype = C.c_int64
    lib.vsx_search_candidates_batch.argtypes = [vp, C.c_int32, C.c_uint64, vp, C.c_uint64, vp, vp, C.POINTER(Candidates)]
    lib.vsx_candidates_free.argtypes = [C.POINTER(Candidates)]
    lib.vsx_candidates_free.restype = None
    lib.vsx_allpairs_block.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, C.POINTER(Hits)]
    lib.vsx_allpairs_rows.argtypes = [vp, C.c_int32, vp, C.c_uint64, C.POINTER(Hits)]
    lib.vsx_allpairs_stream.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, vp, vp]     # (sink: a CFUNCTYPE object, passed as a pointer)
    lib.vsx_dust_mask.argtypes = [vp, C.c_uint64, vp, vp, C.c_int32]
    lib.vsx_multi_searcher_create.argtypes = [C.POINTER(vp), vp, vp, C.c_int32, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp]
    lib.vsx_multi_searcher_destroy.argtypes = [vp]
    lib.vsx_multi_searcher_destroy.restype = None
    lib.vsx_multi_searcher_devices.argtypes = [vp]
    lib.vsx_multi_searcher_devices.restype = C.c_int32
    lib.vsx_multi_searcher_replica.argtypes = [vp, C.c_int32]
    lib.vsx_multi_searcher_replica.restype = vp
    lib.vsx_multi_search_batch.argtypes = [vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, C.POINTER(Hits)]
    lib.vsx_multi_allpairs.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, C.POINTER(Hits)]
    lib.vsx_abundance_ratio_cmp.argtypes = [C.c_int64, C.c_double, C.c_int64]
    lib.vsx_abundance_ratio_cmp.restype = C.c_int
    lib.vsx_cluster_fast.argtypes = [vp, C.c_uint64, C.POINTER(ClusterOut)]
    lib.vsx_cluster_out_free.argtypes = [C.POINTER(ClusterOut)]
    lib.vsx_cluster_out_free.restype = None
    lib.vsx_msa.argtypes = [C.c_uint32, vp, vp, vp, vp, C.POINTER(MsaOut)]
    lib.vsx_msa_device.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, C.POINTER(MsaOut)]
    lib.vsx_msa_device_batch.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, C.POINTER(MsaOut)]
    lib.vsx_msa_out_free.argtypes = [C.POINTER(MsaOut)]
    lib.vsx_msa_out_free.restype = None
    lib.vsx_lma_align.argtypes = [C.POINTER(Scoring), C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64] + \
        [C.POINTER(C.c_int64)] * 5 + [C.POINTER(vp)]
    lib.vsx_merge_opts_default.argtypes = [C.POINTER(MergeOpts)]
    lib.vsx_merge_opts_default.restype = None
    lib.vsx_merge_pairs.argtypes = [vp, C.POINTER(MergeOpts), C.c_uint64, vp, vp, C.c_uint64, vp, vp, vp, vp, C.c_uint64, vp, vp,
                                    C.POINTER(MergeOut)]
    lib.vsx_merge_out_free.argtypes = [C.POINTER(MergeOut)]
    lib.vsx_merge_out_free.restype = None
    lib.vsx_merge_last_stats.argtypes = [C.POINTER(MergeStats)]
    lib.vsx_merge_last_stats.restype = None
    lib.vsx_fastx_filter_opts_default.argtypes = [C.POINTER(FilterOpts)]
    lib.vsx_fastx_filter_opts_default.restype = None
    lib.vsx_fastx_filter.argtypes = [vp, C.POINTER(FilterOpts), C.c_uint64, C.POINTER(FilterReads), C.POINTER(FilterReads),
                                     C.POINTER(FilterOut)]
    lib.vsx_fastx_filter_out_free.argtypes = [C.POINTER(FilterOut)]
    lib.vsx_fastx_filter_out_free.restype = None
    lib.vsx_fastx_filter_last_stats.argtypes = [C.POINTER(FilterStats)]
    lib.vsx_fastx_filter_last_stats.restype = None
    lib.vsx_fastq_eestats_opts_default.argtypes = [C.POINTER(EEStatsOpts)]
    lib.vsx_fastq_eestats_opts_default.restype = None
    lib.vsx_fastq_eestats.argtypes = [vp, C.POINTER(EEStatsOpts), C.c_uint64, C.POINTER(FilterReads), C.POINTER(EEStatsOut)]
    lib.vsx_fastq_eestats_out_free.argtypes = [C.POINTER(EEStatsOut)]
    lib.vsx_fastq_eestats_out_free.restype = None
    lib.vsx_fastq_eestats_last_stats.argtypes = [C.POINTER(EEStatsStats)]
    lib.vsx_fastq_eestats_last_stats.restype = None
    lib.vsx_fastq_stats_opts_default.argtypes = [C.POINTER(FastqStatsOpts)]
    lib.vsx_fastq_stats_opts_default.restype = None
    lib.vsx_fastq_stats.argtypes = [vp, C.POINTER(FastqStatsOpts), C.c_uint64, C.POINTER(FilterReads), C.POINTER(FastqStatsOut)]
    lib.vsx_fastq_stats_out_free.argtypes = [C.POINTER(FastqStatsOut)]
    lib.vsx_fastq_stats_out_free.restype = None
    lib.vsx_fastq_stats_last_stats.argtypes = [C.POINTER(FastqStatsStats)]
    lib.vsx_fastq_stats_last_stats.restype = None
    lib.vsx_fastq_chars_opts_default.argtypes = [C.POINTER(FastqCharsOpts)]
    lib.vsx_fastq_chars_opts_default.restype = None
    lib.vsx_fastq_chars.argtypes = [vp, C.POINTER(FastqCharsOpts), C.c_uint64, C.POINTER(FilterReads), C.POINTER(FastqCharsOut)]
    lib.vsx_fastq_chars_out_free.argtypes = [C.POINTER(FastqCharsOut)]
    lib.vsx_fastq_chars_out_free.restype = None
    lib.vsx_fastq_chars_last_stats.argtypes = [C.POINTER(FastqCharsStats)]
    lib.vsx_fastq_chars_last_stats.restype = None
    lib.vsx_search_exact.argtypes = [vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.POINTER(SeqMeta), C.POINTER(Hits)]
    lib.vsx_search_exact_last_stats.argtypes = [C.POINTER(ExactStats)]
    lib.vsx_search_exact_last_stats.restype = None
    lib.vsx_internal_search_exact_host.argtypes = [C.POINTER(Scoring), C.POINTER(SearchOpts), C.c_uint64, vp, C.c_uint64, vp, vp,
                                                   C.POINTER(SeqMeta), C.c_uint64, vp, C.c_uint64, vp, vp, C.POINTER(SeqMeta),
                                                   C.POINTER(Hits)]
    lib.vsx_derep_opts_default.argtypes = [C.POINTER(DerepOpts)]
    lib.vsx_derep_opts_default.restype = None
    lib.vsx_derep.argtypes = [vp, C.POINTER(DerepOpts), C.c_uint64, C.POINTER(FilterReads), vp, vp, C.POINTER(DerepOut)]
    lib.vsx_derep_out_free.argtypes = [C.POINTER(DerepOut)]
    lib.vsx_derep_out_free.restype = None
    lib.vsx_derep_last_stats.argtypes = [C.POINTER(DerepStats)]
    lib.vsx_derep_last_stats.restype = None
    lib.vsx_internal_derep_thresholds.argtypes = [C.POINTER(C.c_double)]
    lib.vsx_internal_derep_thresholds.restype = None
    lib.vsx_derep_prefix_opts_default.argtypes = [C.POINTER(DerepPrefixOpts)]
    lib.vsx_derep_prefix_opts_default.restype = None
    lib.vsx_derep_prefix.argtypes = [vp, C.POINTER(DerepPrefixOpts), C.c_uint64, C.POINTER(FilterReads), vp, vp, C.POINTER(DerepPrefixOut)]
    lib.vsx_derep_prefix_out_free.argtypes = [C.POINTER(DerepPrefixOut)]
    lib.vsx_derep_prefix_out_free.restype = None
    lib.vsx_derep_prefix_last_stats.argtypes = [C.POINTER(DerepPrefixStats)]
    lib.vsx_derep_prefix_last_stats.restype = None
    lib.vsx_sintax_opts_default.argtypes = [C.POINTER(SintaxOpts)]
    lib.vsx_sintax_opts_default.restype = None
    lib.vsx_sintax.argtypes = [vp, C.POINTER(SintaxOpts), C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint64, vp, C.POINTER(SintaxResult)]
    lib.vsx_sintax_result_free.argtypes = [C.POINTER(SintaxResult)]
    lib.vsx_sintax_result_free.restype = None
    lib.vsx_sintax_last_stats.argtypes = [C.POINTER(SintaxStats)]
    lib.vsx_sintax_last_stats.restype = None
    lib.vsx_internal_sintax_host.argtypes = [C.POINTER(SearchOpts), C.POINTER(SintaxOpts), C.c_uint64, vp, C.c_uint64, vp, vp,
                                             C.POINTER(C.c_char_p), C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint64, vp,
                                             C.POINTER(SintaxResult)]
    lib.vsx_internal_sintax_intern.argtypes = [C.c_uint64, C.POINTER(C.c_char_p), vp, vp, vp]
    lib.vsx_orient_opts_default.argtypes = [C.POINTER(OrientOpts)]
    lib.vsx_orient_opts_default.restype = None
    lib.vsx_orient.argtypes = [vp, C.POINTER(OrientOpts), C.c_uint64, vp, C.c_uint64, vp, vp, vp, C.POINTER(OrientResult)]
    lib.vsx_orient_result_free.argtypes = [C.POINTER(OrientResult)]
    lib.vsx_orient_result_free.restype = None
    lib.vsx_orient_last_stats.argtypes = [C.POINTER(OrientStats)]
    lib.vsx_orient_last_stats.restype = None
    lib.vsx_internal_orient_host.argtypes = [C.POINTER(SearchOpts), C.POINTER(OrientOpts), C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint64, vp,
                                             C.c_uint64, vp, vp, vp, C.POINTER(OrientResult)]
    lib.vsx_internal_orient_matchcounts.argtypes = [vp, vp, C.c_uint64, vp]
    lib.vsx_otutab_opts_default.argtypes = [C.POINTER(OtutabOpts)]
    lib.vsx_otutab_opts_default.restype = None
    lib.vsx_otutab.argtypes = [vp, C.POINTER(OtutabOpts), C.POINTER(Labels), vp, vp, C.POINTER(Labels), vp, C.POINTER(OtutabResult)]
    lib.vsx_otutab_result_free.argtypes = [C.POINTER(OtutabResult)]
    lib.vsx_otutab_result_free.restype = None
    lib.vsx_otutab_last_stats.argtypes = [C.POINTER(OtutabStats)]
    lib.vsx_otutab_last_stats.restype = None
    lib.vsx_internal_otutab_host.argtypes = [C.POINTER(OtutabOpts), C.POINTER(Labels), vp, vp, C.POINTER(Labels), vp, C.POINTER(OtutabResult)]
    lib.vsx_hitout_opts_default.argtypes = [C.POINTER(HitoutOpts)]
    lib.vsx_hitout_opts_default.restype = None
    lib.vsx_hits_render.argtypes = [vp, C.POINTER(HitoutOpts), C.c_uint64, vp, C.c_uint64, vp, vp, C.POINTER(Hits), C.POINTER(HitText)]
    lib.vsx_hit_text_free.argtypes = [C.POINTER(HitText)]
    lib.vsx_hit_text_free.restype = None
    lib.vsx_hits_render_last_stats.argtypes = [C.POINTER(HitoutStats)]
    lib.vsx_hits_render_last_stats.restype = None
    lib.vsx_internal_hits_render_host.argtypes = [C.POINTER(Scoring), C.POINTER(SearchOpts), C.POINTER(HitoutOpts), C.c_uint64, vp, C.c_uint64, vp, vp,
                                                  C.c_uint64, vp, C.c_uint64, vp, vp, C.POINTER(Hits), C.POINTER(HitText)]
    lib.vsx_fastx_mask_opts_default.argtypes = [C.POINTER(MaskOpts)]
    lib.vsx_fastx_mask_opts_default.restype = None
    lib.vsx_fastx_mask.argtypes = [vp, C.POINTER(MaskOpts), C.c_uint64, vp, C.c_uint64, vp, vp, C.POINTER(MaskOut)]
    lib.vsx_fastx_mask_out_free.argtypes = [C.POINTER(MaskOut)]
    lib.vsx_fastx_mask_out_free.restype = None
    lib.vsx_fastx_mask_last_stats.argtypes = [C.POINTER(MaskStats)]
    lib.vsx_fastx_mask_last_stats.restype = None
    lib.vsx_getseqs_opts_default.argtypes = [C.POINTER(GetseqsOpts)]
    lib.vsx_getseqs_opts_default.restype = None
    lib.vsx_getseqs.argtypes = [vp, C.POINTER(GetseqsOpts), C.POINTER(Labels), vp, C.POINTER(Labels), C.POINTER(GetseqsOut)]
    lib.vsx_getseqs_out_free.argtypes = [C.POINTER(GetseqsOut)]
    lib.vsx_getseqs_out_free.restype = None
    lib.vsx_getseqs_last_stats.argtypes = [C.POINTER(GetseqsStats)]
    lib.vsx_getseqs_last_stats.restype = None
    lib.vsx_cut_opts_default.argtypes = [C.POINTER(CutOpts)]
    lib.vsx_cut_opts_default.restype = None
    lib.vsx_cut_pattern_check.argtypes = [C.c_char_p, C.c_uint64, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.vsx_cut.argtypes = [vp, C.POINTER(CutOpts), C.c_uint64, vp, C.c_uint64, vp, vp, C.POINTER(CutOut)]
    lib.vsx_cut_out_free.argtypes = [C.POINTER(CutOut)]
    lib.vsx_cut_out_free.restype = None
    lib.vsx_cut_last_stats.argtypes = [C.POINTER(CutStats)]
    lib.vsx_cut_last_stats.restype = None
    lib.vsx_chimalns_opts_default.argtypes = [C.POINTER(ChimalnsOpts)]
    lib.vsx_chimalns_opts_default.restype = None
    lib.vsx_chimera_alns.argtypes = [vp, C.POINTER(ChimalnsOpts), C.c_uint64, vp, C.c_uint64, vp, vp, vp, C.POINTER(ChimalnsOut)]
    lib.vsx_chimalns_out_free.argtypes = [C.POINTER(ChimalnsOut)]
    lib.vsx_chimalns_out_free.restype = None
    lib.vsx_chimalns_last_stats.argtypes = [C.POINTER(ChimalnsStats)]
    lib.vsx_chimalns_last_stats.restype = None
    lib.vsx_internal_chimalns_host.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p,
                                               C.POINTER(ChimalnsOpts), C.POINTER(ChimalnsOut)]
    lib.vsx_internal_chimalns_device.argtypes = [vp, C.c_uint64] + [C.POINTER(C.c_char_p), vp] * 3 + [C.POINTER(C.c_char_p)] * 2 + \
        [C.POINTER(ChimalnsOpts), C.POINTER(ChimalnsOut)]
    lib.vsx_sortby_opts_default.argtypes = [C.POINTER(SortbyOpts)]
    lib.vsx_sortby_opts_default.restype = None
    lib.vsx_sortby.argtypes = [vp, C.POINTER(SortbyOpts), C.c_uint64, vp, C.c_uint64, vp, vp, vp, vp, C.POINTER(SortbyOut)]
    lib.vsx_sortby_out_free.argtypes = [C.POINTER(SortbyOut)]
    lib.vsx_sortby_out_free.restype = None
    lib.vsx_sortby_last_stats.argtypes = [C.POINTER(SortbyStats)]
    lib.vsx_sortby_last_stats.restype = None
    lib.vsx_lca_opts_default.argtypes = [C.POINTER(LcaOpts)]
    lib.vsx_lca_opts_default.restype = None
    lib.vsx_lca_index_create.argtypes = [vp, C.POINTER(Labels), C.POINTER(vp)]
    lib.vsx_lca_index_destroy.argtypes = [vp]
    lib.vsx_lca_index_destroy.restype = None
    lib.vsx_lca.argtypes = [vp, C.POINTER(LcaOpts), C.POINTER(Hits), C.POINTER(LcaResult)]
    lib.vsx_lca_result_free.argtypes = [C.POINTER(LcaResult)]
    lib.vsx_lca_result_free.restype = None
    lib.vsx_lca_last_stats.argtypes = [C.POINTER(LcaStats)]
    lib.vsx_lca_last_stats.restype = None
    lib.vsx_internal_lca_host.argtypes = [C.POINTER(LcaOpts), C.POINTER(Labels), C.POINTER(Hits), C.POINTER(LcaResult)]
    lib.vsx_internal_lca_index_split.argtypes = [vp, C.c_uint64, vp, vp]
    _lib = lib
    return lib


class VsxError(RuntimeError):
    def __init__(self, code, where):
        msg = load().vsx_last_error().decode(errors="replace")
        super().__init__(f"{where}: error {code}: {msg}")
        self.code = code


def check(code, where):
    if code != VSX_OK:
        raise VsxError(code, where)
