"""Read quality statistics (the reference's --fastq_eestats and --fastq_eestats2) over vsx_fastq_eestats
(include/vsx_eestats.h).

read_stats() takes the quality strings as they stand in the input file and returns an EEStatsResult: the tables both
commands print from, as numpy arrays, and two formatters that reproduce the reference CLI's --output text line for line.
FASTQ parsing and file writing stay with the caller.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import EEStatsOpts, EEStatsOut, EEStatsStats, FilterReads, check
from .merge import _blob

INT_MAX = 2 ** 31 - 1
WANT = {"eestats": _lib.EESTATS_WANT_EESTATS, "eestats2": _lib.EESTATS_WANT_EESTATS2,
        "both": _lib.EESTATS_WANT_EESTATS | _lib.EESTATS_WANT_EESTATS2}
EESTATS_HEADER = "Pos\tRecs\tPctRecs\tMin_Q\tLow_Q\tMed_Q\tMean_Q\tHi_Q\tMax_Q\tMin_Pe\tLow_Pe\tMed_Pe\tMean_Pe\tHi_Pe\tMax_Pe\t" \
                 "Min_EE\tLow_EE\tMed_EE\tMean_EE\tHi_EE\tMax_EE"


def default_opts(ascii=33, qmin=0, qmax=41, length_cutoffs=(50, None, 50), ee_cutoffs=(0.5, 1.0, 2.0), want="both", window=0,
                 hist_budget=0):
    """-> (vsx_fastq_eestats_opts, the array its ee_cutoffs points to).  length_cutoffs: (shortest, longest, increment) with
    longest None for the '*' of --length_cutoffs; ee_cutoffs: used in the given order; want: 'eestats', 'eestats2', 'both'."""
    o = EEStatsOpts()
    _lib.load().vsx_fastq_eestats_opts_default(C.byref(o))
    shortest, longest, increment = length_cutoffs
    o.ascii, o.qmin, o.qmax = ascii, qmin, qmax
    o.len_shortest, o.len_longest, o.len_increment = shortest, INT_MAX if longest is None else longest, increment
    cut = np.ascontiguousarray(ee_cutoffs, np.float64)
    o.ee_cutoffs = cut.ctypes.data_as(C.POINTER(C.c_double))
    o.n_ee_cutoffs = len(cut)
    o.want = WANT[want]
    o.window, o.hist_budget = window, hist_budget
    return o, cut


def last_stats():
    s = EEStatsStats()
    _lib.load().vsx_fastq_eestats_last_stats(C.byref(s))
    return {n: getattr(s, n) for n, _ in EEStatsStats._fields_}


def _pe(q):
    return math.pow(10.0, -q / 10.0)


def _quartiles(values, counts, reads):
    """the reference's scan over (value, count) in the given order -> (min, low, med, hi, max, sum of value * count), -1.0 where
    nothing is found"""
    lo = [-1.0] * 5
    total, n = 0.0, 0.0
    for v, x in zip(values, counts):
        if x > 0:
            total += v * float(x)
            n += float(x)
            if lo[0] < 0:
                lo[0] = v
            for k, share in ((1, 0.25), (2, 0.50), (3, 0.75)):
                if lo[k] < 0 and n >= share * float(reads):
                    lo[k] = v
            lo[4] = v
    return lo, total


class EEStatsResult:
    """n, symbols, len_min, len_max; for eestats: reads_at [len_max], qual_counts [len_max][qmax + 2], sum_ee [len_max],
    ee_bins [len_max][5] (Min, Low, Med, Hi, Max bin of the 1/1000 histogram); for eestats2: cutoff_counts [len_steps][cutoffs].
    Tables a call did not ask for are None."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def eestats_lines(self):
        """the lines of --fastq_eestats --output: the header and one 21-column row per position"""
        if self.reads_at is None:
            raise ValueError("the call did not ask for the eestats tables")
        out = [EESTATS_HEADER]
        cols = self.qual_counts.shape[1] if self.len_max else 0
        for i in range(self.len_max):
            reads = int(self.reads_at[i])
            counts = [int(x) for x in self.qual_counts[i]]
            q, qsum = _quartiles([float(v) for v in range(cols)], counts, reads)
            pe, pesum = _quartiles([_pe(v) for v in range(cols - 1, -1, -1)], counts[::-1], reads)
            ee = [(float(b) + 0.5) / 1000 for b in self.ee_bins[i]]
            mean_q, mean_pe, mean_ee = 1.0 * qsum / reads, 1.0 * pesum / reads, float(self.sum_ee[i]) / reads
            row = "%d\t%d\t%.1f" % (i + 1, reads, 100.0 * reads / self.n)
            row += "\t%.1f\t%.1f\t%.1f\t%.1f\t%.1f\t%.1f" % (q[0], q[1], q[2], mean_q, q[3], q[4])
            row += "\t%.2g\t%.2g\t%.2g\t%.2g\t%.2g\t%.2g" % (pe[0], pe[1], pe[2], mean_pe, pe[3], pe[4])
            row += "\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f" % (ee[0], ee[1], ee[2], mean_ee, ee[3], ee[4])
            out.append(row)
        return out

    def eestats2_lines(self):
        """the lines of --fastq_eestats2 --output"""
        if self.cutoff_counts is None:
            raise ValueError("the call did not ask for the eestats2 table")
        first = "%d reads" % self.n
        if self.n > 0:
            first += ", max len %d, avg %.1f" % (self.len_max, 1.0 * self.symbols / self.n)
        out = [first, "", "Length" + "".join("         MaxEE %.2f" % c for c in self.ee_cutoffs),
               "------" + "   ----------------" * len(self.ee_cutoffs)]
        shortest, longest, increment = self.length_cutoffs
        for x in range(self.cutoff_counts.shape[0]):
            length = shortest + x * increment
            if length > longest:
                break
            out.append("%6d" % length + "".join("   %8d(%5.1f%%)" % (int(c), 100.0 * int(c) / self.n) for c in self.cutoff_counts[x]))
        return out


def _array(ptr, shape, dtype):
    count = int(np.prod(shape))
    if not count or not ptr:
        return np.zeros(shape, dtype)
    return np.ctypeslib.as_array(ptr, shape=(count,)).reshape(shape).astype(dtype, copy=True)


def stats_of_blob(aligner, blob, off, lens, **opts):
    """read_stats() for reads given as a quality blob with offsets (uint64) and lengths (uint32), in any layout"""
    lib = _lib.load()
    o, cut = default_opts(**opts)
    off, lens = np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(lens, np.uint32)
    reads = FilterReads(None, C.cast(C.c_char_p(blob), C.c_void_p), len(blob), off.ctypes.data, lens.ctypes.data, None)
    out = EEStatsOut()
    check(lib.vsx_fastq_eestats(aligner.h if aligner is not None else None, C.byref(o), C.c_uint64(len(lens)), C.byref(reads),
                                C.byref(out)), "vsx_fastq_eestats")
    try:
        n, len_max = int(out.n), int(out.len_max)
        tables = bool(o.want & _lib.EESTATS_WANT_EESTATS)
        cutoffs = bool(o.want & _lib.EESTATS_WANT_EESTATS2)
        cols = int(out.qual_cols)
        return EEStatsResult(
            n=n, symbols=int(out.symbols), len_min=int(out.len_min), len_max=len_max,
            reads_at=_array(out.reads_at, (len_max,), np.uint64) if tables else None,
            qual_counts=_array(out.qual_counts, (len_max, cols), np.uint64) if tables else None,
            sum_ee=_array(out.sum_ee, (len_max,), np.float64) if tables else None,
            ee_bins=_array(out.ee_bins, (len_max, 5), np.int64) if tables else None,
            cutoff_counts=_array(out.cutoff_counts, (int(out.len_steps), int(out.n_ee_cutoffs)), np.uint64) if cutoffs else None,
            ee_cutoffs=[float(c) for c in cut], length_cutoffs=(int(o.len_shortest), int(o.len_longest), int(o.len_increment)),
            stats=last_stats())
    finally:
        lib.vsx_fastq_eestats_out_free(C.byref(out))


def read_stats(aligner, quals, **opts):
    """Accumulate the tables of --fastq_eestats and --fastq_eestats2 over `quals`, a sequence of str or bytes, one quality string
    per read.  aligner: an Aligner (its device runs the kernels), or None under VSX_EESTATS=host.  Options: default_opts().  An
    option value the reference refuses, or a quality outside [qmin, qmax] anywhere, raises VsxError (VSX_EINVAL)."""
    blob, off, lens = _blob(quals)
    return stats_of_blob(aligner, blob, off, lens, **opts)
