"""Read quality filtering (the analysis core of the reference's --fastq_filter / --fastx_filter) over vsx_fastx_filter
(include/vsx_filter.h).

filter_reads() takes the reads as they stand in the input file(s) and returns a FilterResult with one record per read --
(start, length) of what the command would print, its expected error, the verdict -- and formatters that reproduce the
reference CLI's text: --fastqout, --fastqout_discarded, --fastqout_rev, --fastaout and their siblings, with or without
--fastq_eeout.  FASTQ / FASTA parsing and writing, relabelling, --sizeout, --xsize, --lengthout and --sample stay with the
caller, who also resolves the abundances (--sizein).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FilterOpts, FilterOut, FilterReads, FilterRecord, FilterStats, check
from .merge import _blob, format_ee

RECORD_DTYPE = np.dtype([(n, np.dtype(t)) if n != "pad" else (n, np.uint8, (6,)) for n, t in FilterRecord._fields_])


def default_opts(**kw):
    """vsx_fastx_filter_opts with the reference's defaults; keywords are the field names (maxee=1.0, truncqual=2, ...)"""
    o = FilterOpts()
    _lib.load().vsx_fastx_filter_opts_default(C.byref(o))
    names = {n for n, _ in FilterOpts._fields_}
    for k, v in kw.items():
        if k not in names:
            raise TypeError(f"filter_reads: unknown option {k!r}")
        setattr(o, k, v)
    return o


def last_stats():
    s = FilterStats()
    _lib.load().vsx_fastx_filter_last_stats(C.byref(s))
    return {n: getattr(s, n) for n, _ in FilterStats._fields_}


class FilterResult:
    """`records` / `rev_records` (None without reverse reads): numpy structured arrays (start, length, ee, discarded,
    truncated); `pair_discarded`: the verdict of the read, or of the pair if either of its reads is discarded."""

    def __init__(self, records, rev_records, pair_discarded, totals, seqs, quals, rev_seqs, rev_quals, stats):
        self.records = records
        self.rev_records = rev_records
        self.pair_discarded = pair_discarded
        self._totals = totals
        self._text = {"fwd": (seqs, quals), "rev": (rev_seqs, rev_quals)}
        self.stats = stats

    def __len__(self):
        return len(self.records)

    def kept_indices(self):
        return np.flatnonzero(self.pair_discarded == 0)

    def discarded_indices(self):
        return np.flatnonzero(self.pair_discarded)

    def counts(self):
        """the totals the command prints: kept, of which truncated, discarded"""
        return dict(zip(("kept", "truncated", "discarded"), self._totals))

    def _rows(self, labels, which, side, eeout):
        if which not in ("kept", "discarded") or side not in ("fwd", "rev"):
            raise ValueError("which: 'kept' or 'discarded'; side: 'fwd' or 'rev'")
        recs = self.records if side == "fwd" else self.rev_records
        seqs, quals = self._text[side]
        if recs is None:
            raise ValueError("no reverse reads were given")
        for k in (self.kept_indices() if which == "kept" else self.discarded_indices()):
            r = recs[k]
            a, b = int(r["start"]), int(r["start"]) + int(r["length"])
            label = labels[k]
            if eeout and r["ee"] >= 0.0:
                label += ("" if label.endswith(";") else ";") + "ee=" + format_ee(float(r["ee"]))
            yield label, _text(seqs[k])[a:b], _text(quals[k])[a:b] if quals is not None else None

    def fastq_lines(self, labels, which="kept", side="fwd", eeout=False):
        """--fastqout / --fastqout_discarded / --fastqout_rev / --fastqout_discarded_rev: four lines per read"""
        if self._text[side][1] is None:
            raise ValueError("FASTQ output needs qualities")
        out = []
        for label, seq, qual in self._rows(labels, which, side, eeout):
            out += ["@" + label, seq, "+", qual]
        return out

    def fasta_lines(self, labels, which="kept", side="fwd", width=80, eeout=False):
        """--fastaout and its siblings: the header, then the sequence folded at `width` (below 1: on one line)"""
        out = []
        for label, seq, _ in self._rows(labels, which, side, eeout):
            out.append(">" + label)
            out += [seq] if width < 1 else [seq[i:i + width] for i in range(0, len(seq), width)]
        return out


def _text(s):
    return s if isinstance(s, str) else bytes(s).decode("latin-1")


def _side(seqs, quals, sizes, keep):
    sb, off, lens = _blob(seqs)
    qb = None
    if quals is not None:
        qb, _, qlens = _blob(quals)
        if not np.array_equal(lens, qlens):
            raise ValueError("filter_reads: a quality string differs in length from its sequence")
    ab = None
    if sizes is not None:
        ab = np.ascontiguousarray(sizes, np.uint64)
        if len(ab) != len(seqs):
            raise ValueError("filter_reads: one abundance per read")
    raw = lambda b: C.cast(C.c_char_p(b), C.c_void_p)  # noqa: E731
    keep += [sb, qb, off, lens, ab]
    return FilterReads(raw(sb), raw(qb) if qb is not None else None, len(sb), off.ctypes.data, lens.ctypes.data,
                       ab.ctypes.data if ab is not None else None)


def _records(ptr, n):
    if not n:
        return np.zeros(0, RECORD_DTYPE)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * RECORD_DTYPE.itemsize,)).view(RECORD_DTYPE).copy()


def filter_reads(aligner, seqs, quals=None, rev_seqs=None, rev_quals=None, sizes=None, rev_sizes=None, **opts):
    """Analyse reads (rev_seqs=None) or read pairs.  seqs / quals: sequences of str or bytes, one entry per read; quals=None
    is FASTA input (no quality walk, ee = -1).  sizes: abundances (default 1 each).  aligner: an Aligner (its device runs
    the kernel), or None under VSX_FILTER=host.  Options: default_opts().  An option value the reference refuses, or an
    out-of-range quality where the reference reads it, raises VsxError (VSX_EINVAL)."""
    if rev_seqs is not None and len(rev_seqs) != len(seqs):
        raise ValueError("filter_reads: one reverse read per forward read")
    if rev_seqs is not None and (quals is None) != (rev_quals is None):
        raise ValueError("filter_reads: both sides with qualities, or neither")
    lib = _lib.load()
    o = opts.pop("opts", None) or default_opts(**opts)
    keep = []
    fwd = _side(seqs, quals, sizes, keep)
    rev = _side(rev_seqs, rev_quals, rev_sizes, keep) if rev_seqs is not None else None
    out = FilterOut()
    n = len(seqs)
    check(lib.vsx_fastx_filter(aligner.h if aligner is not None else None, C.byref(o), C.c_uint64(n), C.byref(fwd),
                               C.byref(rev) if rev is not None else None, C.byref(out)), "vsx_fastx_filter")
    try:
        records = _records(out.fwd, n)
        rev_records = _records(out.rev, n) if rev is not None else None
        verdict = np.ctypeslib.as_array(out.pair_discarded, shape=(n,)).copy() if n else np.zeros(0, np.uint8)
        totals = (int(out.kept), int(out.kept_truncated), int(out.discarded))
    finally:
        lib.vsx_fastx_filter_out_free(C.byref(out))
    return FilterResult(records, rev_records, verdict, totals, seqs, quals, rev_seqs, rev_quals, last_stats())
