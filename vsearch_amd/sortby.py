"""Abundance and length sorting (--sortbysize, --sortbylength, and the database orders of the clustering and chimera commands) over
include/vsx_sortby.h.

    sortby(aligner, labels, lengths, sizes, order, ...)   sort on the aligner's device: the permutation, n_kept, the median
    sortby_host(labels, lengths, sizes, order, ...)       the library's host restatement: no device
    sortbysize / sortbylength                             the two commands (minsize / maxsize apply to sortbysize only)
    db_order(aligner, labels, lengths, sizes, order)      the plain permutation, for callers that need their input in a database order
    fasta_lines / log_lines                               --output and the median line of --log

Labels are the headers as the reference's parser hands them on (str is encoded as latin-1; bytes are taken as they are); sizes are
the abundances the caller parsed from them.  An order is "size", "length", "length_asc" or the VSX_SORTBY_* number.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import SORTBY_LENGTH, SORTBY_LENGTH_ASC, SORTBY_SIZE, SortbyOpts, check
from .derep import _text
from .orient import _fasta, _header, _size

ORDERS = {"size": SORTBY_SIZE, "length": SORTBY_LENGTH, "length_asc": SORTBY_LENGTH_ASC}
INT64_MAX = (1 << 63) - 1
HOST_ROUTES = ("host_no_context", "host_environment", "host_count", "host_memory", "host_long_prefix")


def last_stats():
    st = _lib.SortbyStats()
    _lib.load().vsx_sortby_last_stats(C.byref(st))
    return {k: (list(getattr(st, k)) if k == "active" else getattr(st, k)) for k, _ in _lib.SortbyStats._fields_}


class SortbyResult:
    """order = the input numbers in output order (uint64; ordinal = index + 1); n_kept = the deck before topn; n_out = len(order);
    median = the command's median as a float; sort_order = the VSX_SORTBY_* number; stats = the call's vsx_sortby_stats"""

    def __init__(self, res, sort_order):
        self.n, self.n_kept, self.n_out = int(res.n), int(res.n_kept), int(res.n_out)
        self.median = float(res.median)
        self.sort_order = sort_order
        if self.n_out:
            self.order = np.ctypeslib.as_array(C.cast(res.order, C.POINTER(C.c_uint64)), shape=(self.n_out,)).copy()
        else:
            self.order = np.zeros(0, np.uint64)
        self.stats = last_stats()

    def tobytes(self):
        """everything two results must share to be the same answer (the median by its bit pattern)"""
        return np.array([self.n, self.n_kept, self.n_out], np.uint64).tobytes() + np.float64(self.median).tobytes() + self.order.tobytes()


def _labels(labels):
    """labels as (blob, offsets, lengths): a list of str / bytes, or the triple itself with the headers anywhere in the blob"""
    if isinstance(labels, tuple):
        return bytes(labels[0]), np.ascontiguousarray(labels[1], np.uint64), np.ascontiguousarray(labels[2], np.uint32)
    raw = [l.encode("latin-1") if isinstance(l, str) else bytes(l) for l in labels]
    lens = np.fromiter((len(r) for r in raw), np.uint32, len(raw))
    off = np.zeros(len(raw), np.uint64)
    if len(raw) > 1:
        np.cumsum(lens[:-1], dtype=np.uint64, out=off[1:])
    return b"".join(raw), off, lens


def _u32(values, what):
    """the reference holds lengths and abundances as unsigned int: a value outside is refused, not wrapped"""
    if isinstance(values, np.ndarray) and values.dtype == np.uint32:
        return np.ascontiguousarray(values)
    wide = [int(v) for v in values]
    if wide and (min(wide) < 0 or max(wide) > 0xFFFFFFFF):
        raise ValueError(f"sortby: {what} outside 0 .. 2^32 - 1")
    return np.array(wide, np.uint32)


def _order(order):
    return ORDERS[order] if isinstance(order, str) else int(order)


def _call(handle, labels, lengths, sizes, order, minsize, maxsize, topn, threads):
    lib = _lib.load()
    blob, off, lens = _labels(labels)
    n = len(lens)
    seqlen, size = _u32(lengths, "length"), _u32(sizes, "abundance")
    if len(seqlen) != n or len(size) != n:
        raise ValueError("sortby: one length and one abundance per label")
    o = SortbyOpts()
    lib.vsx_sortby_opts_default(C.byref(o))
    o.order, o.threads = _order(order), int(threads)
    o.minsize, o.maxsize, o.topn = int(minsize), int(maxsize), int(topn)
    res = _lib.SortbyOut()
    check(lib.vsx_sortby(handle, C.byref(o), n, C.cast(C.c_char_p(blob), C.c_void_p), len(blob), off.ctypes.data_as(C.c_void_p),
                         lens.ctypes.data_as(C.c_void_p), seqlen.ctypes.data_as(C.c_void_p), size.ctypes.data_as(C.c_void_p), C.byref(res)),
          "vsx_sortby")
    try:
        return SortbyResult(res, o.order)
    finally:
        lib.vsx_sortby_out_free(C.byref(res))


def sortby(aligner, labels, lengths, sizes, order, minsize=0, maxsize=INT64_MAX, topn=INT64_MAX, threads=0):
    """Sort records (label, sequence length, abundance) into one of the reference's orders on the aligner's device (vsx_sortby)."""
    return _call(aligner.h, labels, lengths, sizes, order, minsize, maxsize, topn, threads)


def sortby_host(labels, lengths, sizes, order, minsize=0, maxsize=INT64_MAX, topn=INT64_MAX, threads=0):
    """The host restatement: the same call without a context -- what the device is compared to, and its host route."""
    old = os.environ.get("VSX_SORTBY")
    os.environ["VSX_SORTBY"] = "host"
    try:
        return _call(None, labels, lengths, sizes, order, minsize, maxsize, topn, threads)
    finally:
        if old is None:
            del os.environ["VSX_SORTBY"]
        else:
            os.environ["VSX_SORTBY"] = old


def sortbysize(aligner, labels, lengths, sizes, minsize=0, maxsize=INT64_MAX, topn=INT64_MAX):
    """--sortbysize: abundance descending, then label, then input order"""
    return sortby(aligner, labels, lengths, sizes, SORTBY_SIZE, minsize, maxsize, topn)


def sortbylength(aligner, labels, lengths, sizes, topn=INT64_MAX):
    """--sortbylength: length descending, abundance descending, then label, then input order (the command ignores minsize / maxsize)"""
    return sortby(aligner, labels, lengths, sizes, SORTBY_LENGTH, topn=topn)


def db_order(aligner, labels, lengths, sizes, order):
    """the permutation alone, as a list of input numbers: Database::sortbyabundance / sortbylength / sortbylength_shortest_first"""
    return [int(k) for k in sortby(aligner, labels, lengths, sizes, order).order]


# ---- the writers ---------------------------------------------------------------------------------------------------------------
def fasta_lines(result, labels, seqs, sizes=None, sizeout=False, xsize=False, relabel=None, fasta_width=80):
    """--output: the records in sorted order, numbered from 1"""
    out = []
    for x, k in enumerate(result.order):
        k = int(k)
        out += _fasta(_header(_text(labels[k]), _size(sizes, k), x + 1, sizeout, relabel, xsize), _text(seqs[k]), fasta_width)
    return out


def log_lines(result):
    """the median line of --sortbysize / --sortbylength (%.0f: a half rounds to even)"""
    what = "abundance" if result.sort_order == SORTBY_SIZE else "length"
    return ["Median %s: %.0f" % (what, result.median)]
