"""Prefix dereplication (the reference's --derep_prefix) over vsx_derep_prefix (include/vsx_derep_prefix.h).

derep_prefix() takes the reads as they stand in the input file and returns a DerepPrefixResult: the clusters in the command's
output order (size descending, label, the representative's place in the sorted order) with their members in the order of the
--uc file, and every read's rank in the command's sort.  fasta_lines(), uc_lines() and log_lines() reproduce the reference
CLI's text: --output, --uc and the log.  derep_prefix_host() is the same call through the library's host restatement.  FASTA
parsing, --notrunclabels and the abundance annotations stay with the caller: `sizes` are the headers' ;size= annotations, which
the command's sort always reads; sizein says whether they are summed as well.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import DerepPrefixOpts, DerepPrefixOut, DerepPrefixStats, FilterReads, check
from .derep import DerepResult, _text
from .merge import _blob

UNRANKED = (1 << 64) - 1


def default_opts(**kw):
    """vsx_derep_prefix_opts with the reference's defaults; keywords are the field names (sizein=1, minseqlength=1, ...)"""
    o = DerepPrefixOpts()
    _lib.load().vsx_derep_prefix_opts_default(C.byref(o))
    names = {n for n, _ in DerepPrefixOpts._fields_}
    for k, v in kw.items():
        if k not in names:
            raise TypeError(f"derep_prefix: unknown option {k!r}")
        setattr(o, k, v)
    return o


def last_stats():
    s = DerepPrefixStats()
    _lib.load().vsx_derep_prefix_last_stats(C.byref(s))
    return {n: getattr(s, n) for n, _ in DerepPrefixStats._fields_}


class DerepPrefixResult(DerepResult):
    """rep / size / count: one entry per cluster, output order.  members(c): the cluster's input indices in the order of the --uc
    file (the representative first).  rank: per read its place in the command's sorted order, UNRANKED for a discarded read.
    counts: the figures of the log lines.  The FASTA printing and the log lines are DerepResult's."""

    def __init__(self, rep, size, count, member_start, member, rank, counts, seqs, labels, opts, stats):
        super().__init__(rep, size, count, member_start, member, np.zeros(len(member), np.uint8), None, counts, seqs, labels, opts, stats)
        self.rank = rank

    def uc_lines(self):
        """--uc: per cluster its S record and an H record per further member with the member's own length, then the C records;
        every cluster is listed"""
        out = []
        for c in range(len(self)):
            head = self.label(c)
            out.append(f"S\t{c}\t{len(self._seqs[int(self.rep[c])])}\t*\t*\t*\t*\t*\t{head}\t*")
            for m in self.members(c)[1:]:
                out.append(f"H\t{c}\t{len(self._seqs[int(m)])}\t100.0\t+\t0\t0\t*\t{_text(self._labels[int(m)])}\t{head}")
        for c in range(len(self)):
            out.append(f"C\t{c}\t{int(self.size[c])}\t*\t*\t*\t*\t*\t{self.label(c)}\t*")
        return out


def fasta_lines(res, sizeout=False, relabel=None, xsize=False, fasta_width=80):
    """--output: the clusters within minuniquesize / maxuniquesize, up to topn"""
    return res.fasta_lines(sizeout=sizeout, relabel=relabel, xsize=xsize, fasta_width=fasta_width)


def uc_lines(res):
    return res.uc_lines()


def log_lines(res):
    return res.log_lines()


def derep_prefix(aligner, seqs, labels, sizes=None, strand_both=False, **opts):
    """Dereplicate reads by prefix.  seqs / labels: sequences of str or bytes, one entry per read.  sizes: the headers' abundance
    annotations (default 1 each): always a key of the sort, summed only with sizein=1.  aligner: an Aligner (its device runs the
    kernels), or None for the host restatement (as under VSX_DEREP_PREFIX=host).  Options: default_opts().  A value the library
    refuses raises VsxError (VSX_EINVAL); strand_both raises ValueError, as the command is fatal there."""
    if strand_both:
        raise ValueError("Option '--strand both' not supported with --derep_prefix")
    if len(labels) != len(seqs):
        raise ValueError("derep_prefix: one label per read")
    lib = _lib.load()
    o = opts.pop("opts", None) or default_opts(**opts)
    sb, off, lens = _blob(seqs)
    ab = None
    if sizes is not None:
        ab = np.ascontiguousarray(sizes, np.uint64)
        if len(ab) != len(seqs):
            raise ValueError("derep_prefix: one abundance per read")
    raw = [l.encode("latin-1") if isinstance(l, str) else bytes(l) for l in labels]
    lb = b"".join(raw)
    loff = np.zeros(len(raw) + 1, np.uint64)
    if raw:
        np.cumsum([len(l) for l in raw], out=loff[1:])
    ptr = lambda b: C.cast(C.c_char_p(b), C.c_void_p)  # noqa: E731
    reads = FilterReads(ptr(sb), None, len(sb), off.ctypes.data, lens.ctypes.data, ab.ctypes.data if ab is not None else None)
    out = DerepPrefixOut()
    n = len(seqs)
    check(lib.vsx_derep_prefix(aligner.h if aligner is not None else None, C.byref(o), C.c_uint64(n), C.byref(reads), ptr(lb),
                               loff.ctypes.data, C.byref(out)), "vsx_derep_prefix")
    try:
        nc, kept = int(out.n_clusters), int(out.kept)
        arr = lambda p, m: np.ctypeslib.as_array(p, shape=(m,)).copy() if m else np.zeros(0, np.uint64)  # noqa: E731
        rep, size, count = (arr(p, nc) for p in (out.rep, out.size, out.count))
        member_start = np.ctypeslib.as_array(out.member_start, shape=(nc + 1,)).copy()
        member, rank = arr(out.member, kept), arr(out.rank, n)
        counts = {k: int(getattr(out, k)) for k in ("kept", "nucleotides", "shortest", "longest", "discarded_short", "discarded_long",
                                                    "sumsize", "maxsize", "selected")}
        counts["median"] = float(out.median)
    finally:
        lib.vsx_derep_prefix_out_free(C.byref(out))
    used = {k: int(getattr(o, k)) for k in ("minseqlength", "maxseqlength", "minuniquesize", "maxuniquesize", "topn")}
    return DerepPrefixResult(rep, size, count, member_start, member, rank, counts, seqs, labels, used, last_stats())


def derep_prefix_host(seqs, labels, sizes=None, **opts):
    """derep_prefix() through the library's host restatement"""
    return derep_prefix(None, seqs, labels, sizes=sizes, **opts)
