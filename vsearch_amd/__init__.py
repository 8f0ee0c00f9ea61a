"""vsearch_amd -- MI355X-native (gfx950) global pairwise alignment for vsearch workloads.

The package is a thin host-side mirror of the reference's aligner interface over libvsx's C-ABI
(include/vsx.h); all arithmetic runs in hand-written HIP kernels (vsearch_amd/csrc).
"""
from .aligner import (Aligner, SequenceSet, Plan, AlignmentResults, RawResults, DEFAULT_SCORING,  # noqa: F401
                      scoring_from_tuple, cigar_from_runs)
from .search import SearchSession, msa, msa_batch, dust_mask, exact_summary, search_exact_host  # noqa: F401
from .chimera import ChimeraSession, ChimerasDenovoSession, DenovoChimeraSession  # noqa: F401
from .merge import merge_pairs, MergeResult, MERGE_REASONS  # noqa: F401
from .filter import filter_reads, FilterResult  # noqa: F401
from .eestats import read_stats, EEStatsResult  # noqa: F401
from .fastq_stats import fastq_stats, fastq_chars, FastqStatsResult, FastqCharsResult  # noqa: F401
from .derep import dereplicate, derep_fulllength, fastx_uniques, derep_id, DerepResult  # noqa: F401
from .derep_prefix import derep_prefix, derep_prefix_host, DerepPrefixResult  # noqa: F401
from .sintax import sintax, sintax_host, tabbed_lines, log_lines, SintaxResult  # noqa: F401
from .orient import orient, orient_host, orient_session, OrientResult  # noqa: F401
from .otutab import otutab, otutab_host, OtuTable, LabelBlob  # noqa: F401
from .hitout import (render as render_hits, render_host as render_hits_host, RenderedHits, alnout_text, sam_lines, sam_header_lines,  # noqa: F401
                     blast6_lines, fastapairs_lines, qsegout_lines, tsegout_lines, userout_lines)
from .mask import fastx_mask, fastx_mask_host, maskfasta_lines, MaskResult  # noqa: F401
from .getseqs import getseqs, getseq, getsubseq, getseqs_host, read_labels, GetseqsResult  # noqa: F401
from .cut import cut, cut_host, parse_pattern, CutResult  # noqa: F401
# (vsearch_amd.sortby stays the module: its sortby() is not exported under the same name)
from .sortby import sortbysize, sortbylength, sortby_host, SortbyResult  # noqa: F401
# (vsearch_amd.lca stays the module too: call vsearch_amd.lca.lca())
from .lca import LcaIndex, LcaResult, lca_host, lcaout_lines  # noqa: F401
from ._lib import SENTINEL, VsxError, load as load_library  # noqa: F401

__all__ = ["Aligner", "SequenceSet", "Plan", "AlignmentResults", "RawResults", "cigar_from_runs", "DEFAULT_SCORING", "scoring_from_tuple",
           "SearchSession", "exact_summary", "search_exact_host", "ChimeraSession", "DenovoChimeraSession", "ChimerasDenovoSession", "merge_pairs", "MergeResult", "MERGE_REASONS", "filter_reads", "FilterResult", "read_stats", "EEStatsResult", "fastq_stats", "fastq_chars", "FastqStatsResult", "FastqCharsResult", "dereplicate", "derep_fulllength", "fastx_uniques", "derep_id", "DerepResult", "derep_prefix", "derep_prefix_host", "DerepPrefixResult", "sintax", "sintax_host", "tabbed_lines", "log_lines", "SintaxResult", "orient", "orient_host", "orient_session", "OrientResult", "otutab", "otutab_host", "OtuTable", "LabelBlob", "render_hits", "render_hits_host", "RenderedHits", "alnout_text", "sam_lines", "sam_header_lines", "blast6_lines", "fastapairs_lines", "qsegout_lines", "tsegout_lines", "userout_lines", "fastx_mask", "fastx_mask_host", "maskfasta_lines", "MaskResult", "SENTINEL", "VsxError", "load_library"]
__all__ += ["getseqs", "getseq", "getsubseq", "getseqs_host", "read_labels", "GetseqsResult"]
__all__ += ["cut", "cut_host", "parse_pattern", "CutResult"]
__all__ += ["sortbysize", "sortbylength", "sortby_host", "SortbyResult"]
__all__ += ["LcaIndex", "LcaResult", "lca_host", "lcaout_lines"]
