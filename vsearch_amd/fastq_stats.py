"""Read summary statistics (the reference's --fastq_stats and --fastq_chars) over vsx_fastq_stats and vsx_fastq_chars
(include/vsx_fastq_stats.h).

fastq_stats() takes the quality strings as they stand in the input file, fastq_chars() the sequences and the quality strings.
Each returns a result with the tables as numpy arrays and log_lines(), which reproduces what the reference CLI writes to its
--log between the `Started` line and the blank line in front of `Finished`, line for line.  FASTQ parsing and file writing
stay with the caller.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import FastqCharsOpts, FastqCharsOut, FastqCharsStats, FastqStatsOpts, FastqStatsOut, FastqStatsStats, FilterReads, check
from .eestats import _array
from .merge import _blob

SYMBOLS, FIRST_SYMBOL = 94, 33


def _last(lib_call, struct):
    s = struct()
    lib_call(C.byref(s))
    return {n: getattr(s, n) for n, _ in struct._fields_}


def _reads(seq_blob, qual_blob, off, lens):
    off, lens = np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(lens, np.uint32)
    cast = lambda b: C.cast(C.c_char_p(b), C.c_void_p) if b is not None else None      # noqa: E731
    return FilterReads(cast(seq_blob), cast(qual_blob), len(qual_blob if qual_blob is not None else seq_blob or b""), off.ctypes.data,
                       lens.ctypes.data, None), (off, lens, seq_blob, qual_blob)


class FastqStatsResult:
    """n, symbols, len_min, len_max, ascii; length_counts [len_max + 1], symbol_counts [len_max][94] (by quality character
    33 ... 126), sum_ee [len_max], ee_counts [len_max][4] (<= 1.0, 0.5, 0.25, 0.1), q_counts [len_max][4] (> 5, 10, 15, 20); stats:
    vsx_fastq_stats_last_stats of the call"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def log_lines(self):
        """the five tables and the closing section of --fastq_stats --log"""
        n, reads, symbols, len_max = self.n, float(self.n), float(self.symbols), self.len_max
        counts = [int(x) for x in self.length_counts]
        upto, total = [], 0                                   # reads of length <= L
        for x in counts:
            total += x
            upto.append(total)
        score = lambda c: c - self.ascii if c >= self.ascii else 0      # noqa: E731
        pe = lambda c: math.pow(10.0, -float(score(c)) / 10.0)          # noqa: E731
        out = ["", "Read length distribution", "      L           N      Pct   AccPct", "-------  ----------  -------  -------"]
        for length in range(len_max, self.len_min - 1, -1):
            if counts[length]:
                before = float(upto[length - 1]) if length else 0.0
                out.append("%2s%5d  %10d   %5.1f%%   %5.1f%%" % (">=" if length == len_max else "  ", length, counts[length],
                                                               float(counts[length]) * 100.0 / reads, 100.0 * (reads - before) / reads))
        out += ["", "Q score distribution", "ASCII    Q       Pe           N      Pct   AccPct",
                "-----  ---  -------  ----------  -------  -------"]
        dist = [int(x) for x in self.symbol_counts.sum(axis=0)] if len_max else [0] * SYMBOLS
        accum = 0
        for k in range(SYMBOLS - 1, -1, -1):
            if dist[k]:
                accum += dist[k]
                c = FIRST_SYMBOL + k
                out.append("    %c  %3d  %7.5f  %10d  %6.1f%%  %6.1f%%" % (chr(c), score(c), pe(c), dist[k], 100.0 * float(dist[k]) / symbols,
                                                                          100.0 * float(accum) / symbols))
        out += ["", "    L  PctRecs  AvgQ  P(AvgQ)      AvgP  AvgEE       Rate   RatePct",
                "-----  -------  ----  -------  --------  -----  ---------  --------"]
        for length in range(2, len_max + 1):
            row = [int(x) for x in self.symbol_counts[length - 1]]
            here = float(sum(row))
            sum_q = sum(x * score(FIRST_SYMBOL + k) for k, x in enumerate(row))
            sum_p = 0.0
            for k, x in enumerate(row):                       # symbols ascending, as the reference adds them
                sum_p += float(x) * pe(FIRST_SYMBOL + k)
            avg_q, avg_p, avg_ee = float(sum_q) / here, sum_p / here, float(self.sum_ee[length - 1]) / here
            rate = avg_ee / float(length)
            out.append("%5d  %6.1f%%  %4.1f  %7.5f  %8.6f  %5.2f  %9.6f  %7.3f%%" % (
                length, 100.0 * (reads - float(upto[length - 1])) / reads, avg_q, math.pow(10.0, -avg_q / 10.0), avg_p, avg_ee, rate, 100.0 * rate))
        out += ["", "    L   1.0000   0.5000   0.2500   0.1000   1.0000   0.5000   0.2500   0.1000",
                "-----  -------  -------  -------  -------  -------  -------  -------  -------"]
        first_empty = len_max
        for i in range(len_max):
            if self.ee_counts[i][0] == 0:
                first_empty = i
                break
        for length in range(first_empty, 0, -1):
            c = [int(x) for x in self.ee_counts[length - 1]]
            out.append("%5d  %7d  %7d  %7d  %7d  " % (length, *c) + "  ".join("%6.2f%%" % (100.0 * float(x) / reads) for x in c))
        out += ["", "Truncate at first Q", "  Len     Q=5    Q=10    Q=15    Q=20", "-----  ------  ------  ------  ------"]
        for length in range(len_max, max(1, len_max // 2) - 1, -1):
            out.append("%5d  " % length + "  ".join("%5.1f%%" % (100.0 * float(int(x)) / reads) for x in self.q_counts[length - 1]))
        out += ["", "%10d  Recs (%.1fM), 0 too long" % (n, reads / 1000000.0)]
        if n:
            out.append("%10.1f  Avg length" % (1.0 * symbols / reads))
        out.append("%9.1fM  Bases" % (symbols / 1000000.0))
        return out


class FastqCharsResult:
    """n, total_chars; seq_counts, qual_counts, tail_counts [256] (by character), maxrun [256] (the longest run minus one), qmin_n,
    qmax_n (the quality characters seen under N; 255 and 0 without one); stats: vsx_fastq_chars_last_stats of the call"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def guess(self):
        """-> (lowest quality character, highest, guessed fastq_qmin, fastq_qmax, fastq_ascii); the characters are 0 when no read has a symbol"""
        seen = np.flatnonzero(self.qual_counts)
        qmin, qmax = (int(seen[0]), int(seen[-1])) if len(seen) else (0, 0)
        ascii = 33 if qmin < ord(";") or qmax < ord("K") else 64
        return qmin, qmax, qmin - ascii, qmax - ascii, ascii

    def log_lines(self):
        """what --fastq_chars --log holds"""
        out = ["Read %d sequences." % self.n]
        if self.n == 0:
            return out
        qmin, qmax, guess_qmin, guess_qmax, ascii = self.guess()
        out.append("Qmin %d, Qmax %d, Range %d" % (qmin, qmax, qmax - qmin + 1))
        out.append("Guess: -fastq_qmin %d -fastq_qmax %d -fastq_ascii %d" % (guess_qmin, guess_qmax, ascii))
        if ascii == 64:
            name = "Solexa format (phred+64)" if qmin < 64 else "Illumina 1.3+ format (phred+64)" if qmin < ord("B") else "Illumina 1.5+ format (phred+64)"
        else:
            name = "Illumina 1.8+ format (phred+33)" if qmax > ord("I") else "Original Sanger format (phred+33)"
        out += ["Guess: " + name, "", "Letter          N   Freq MaxRun", "------ ---------- ------ ------"]
        factor = 100.0 / float(self.total_chars) if self.total_chars else math.inf
        for c in range(256):
            x = int(self.seq_counts[c])
            if not x:
                continue
            line = "     %c %10d %5.1f%% %6d" % (chr(c), x, float(x) * factor, int(self.maxrun[c]))
            if c == ord("N"):
                line += "  Q=%c..%c" % (chr(self.qmin_n), chr(self.qmax_n)) if self.qmin_n < self.qmax_n else "  Q=%c" % chr(self.qmin_n)
            out.append(line)
        out += ["", "Char  ASCII    Freq       Tails", "----  -----  ------  ----------"]
        for c in range(qmin, qmax + 1):
            x = int(self.qual_counts[c])
            if x:
                out.append(" '%c'  %5d  %5.1f%%  %10d" % (chr(c), c, float(x) * factor, int(self.tail_counts[c])))
        return out


def stats_of_blob(aligner, blob, off, lens, ascii=33, qmin=0, qmax=41, window=0):
    """fastq_stats() for reads given as a quality blob with offsets (uint64) and lengths (uint32), in any layout"""
    lib = _lib.load()
    o = FastqStatsOpts()
    lib.vsx_fastq_stats_opts_default(C.byref(o))
    o.ascii, o.qmin, o.qmax, o.window = ascii, qmin, qmax, window
    reads, keep = _reads(None, blob, off, lens)
    out = FastqStatsOut()
    check(lib.vsx_fastq_stats(aligner.h if aligner is not None else None, C.byref(o), C.c_uint64(len(keep[1])), C.byref(reads),
                              C.byref(out)), "vsx_fastq_stats")
    try:
        len_max = int(out.len_max)
        return FastqStatsResult(
            n=int(out.n), symbols=int(out.symbols), len_min=int(out.len_min), len_max=len_max, ascii=int(o.ascii),
            length_counts=_array(out.length_counts, (len_max + 1,), np.uint64),
            symbol_counts=_array(out.symbol_counts, (len_max, SYMBOLS), np.uint64),
            sum_ee=_array(out.sum_ee, (len_max,), np.float64),
            ee_counts=_array(out.ee_counts, (len_max, 4), np.uint64),
            q_counts=_array(out.q_counts, (len_max, 4), np.uint64),
            stats=_last(lib.vsx_fastq_stats_last_stats, FastqStatsStats))
    finally:
        lib.vsx_fastq_stats_out_free(C.byref(out))


def fastq_stats(aligner, quals, **opts):
    """Accumulate the tables of --fastq_stats over `quals`, a sequence of str or bytes, one quality string per read.  aligner: an
    Aligner (its device runs the kernels), or None under VSX_FASTQ_STATS=host.  Options: ascii, qmin, qmax, window.  An option
    value the reference refuses, or a read whose lowest or highest score is out of range, raises VsxError (VSX_EINVAL)."""
    blob, off, lens = _blob(quals)
    return stats_of_blob(aligner, blob, off, lens, **opts)


def chars_of_blob(aligner, seq_blob, qual_blob, off, lens, tail=4, window=0):
    """fastq_chars() for reads given as a sequence blob and a quality blob with shared offsets and lengths, in any layout"""
    lib = _lib.load()
    o = FastqCharsOpts()
    lib.vsx_fastq_chars_opts_default(C.byref(o))
    o.tail, o.window = tail, window
    reads, keep = _reads(seq_blob, qual_blob, off, lens)
    out = FastqCharsOut()
    check(lib.vsx_fastq_chars(aligner.h if aligner is not None else None, C.byref(o), C.c_uint64(len(keep[1])), C.byref(reads),
                              C.byref(out)), "vsx_fastq_chars")
    try:
        return FastqCharsResult(
            n=int(out.n), total_chars=int(out.total_chars), tail=int(o.tail),
            seq_counts=np.array(out.seq_counts, np.uint64), qual_counts=np.array(out.qual_counts, np.uint64),
            tail_counts=np.array(out.tail_counts, np.uint64), maxrun=np.array(out.maxrun, np.int32),
            qmin_n=int(out.qmin_n), qmax_n=int(out.qmax_n), stats=_last(lib.vsx_fastq_chars_last_stats, FastqCharsStats))
    finally:
        lib.vsx_fastq_chars_out_free(C.byref(out))


def fastq_chars(aligner, seqs, quals, **opts):
    """Accumulate the inventory of --fastq_chars over `seqs` and `quals`, two sequences of str or bytes of pairwise equal lengths.
    aligner: an Aligner, or None under VSX_FASTQ_STATS=host.  Options: tail (--fastq_tail), window."""
    sb, off, lens = _blob(seqs)
    qb, _, qlens = _blob(quals)
    if len(lens) != len(qlens) or (lens != qlens).any():
        raise ValueError("fastq_chars: sequence and quality strings differ in length")
    return chars_of_blob(aligner, sb, qb, off, lens, **opts)
