"""SINTAX taxonomy classification (--sintax) over include/vsx_sintax.h.

    sintax(session, queries, randseed=..., strand_both=...)   on a SearchSession whose labels carry the taxonomy (tax=d:...,p:...)
    sintax_host(db, db_labels, queries, ...)                  the library's host restatement: no device, no session
    tabbed_lines(result, qlabels, dblabels, cutoff)           the --tabbedout lines
    log_lines(result)                                         the closing "Classified ..." line

The C result carries database sequence numbers and counts; the names are cut from the database labels here, at format time.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import SearchOpts, SintaxOpts, check
from .search import _blob

RANKS = "dkpcofgst"
NONE = _lib.SINTAX_NONE


class SintaxResult:
    """per query: strand, classified, boot_count[2], best_count[2], rank_seq[9], rank_count[9]; candidates (n x 2 x 100, NONE =
    unused) when asked for; stats = the call's vsx_sintax_stats"""

    def __init__(self, res, want_candidates):
        n = int(res.n_queries)
        self.n = n
        self.n_classified = int(res.n_classified)
        rec = np.ctypeslib.as_array(C.cast(res.rec, C.POINTER(C.c_uint32)), shape=(max(n, 1), 24))[:n].copy()
        self.strand = rec[:, 0].astype(np.int32)
        self.classified = rec[:, 1].astype(np.int32)
        self.boot_count = rec[:, 2:4].copy()
        self.best_count = rec[:, 4:6].copy()
        self.rank_seq = rec[:, 6:15].copy()
        self.rank_count = rec[:, 15:24].copy()
        self.candidates = None
        if want_candidates:
            self.candidates = np.ctypeslib.as_array(res.candidates, shape=(max(n, 1), 2, _lib.SINTAX_ROUNDS))[:n].copy()
        st = _lib.SintaxStats()
        _lib.load().vsx_sintax_last_stats(C.byref(st))
        self.stats = {k: getattr(st, k) for k, _ in _lib.SintaxStats._fields_}

    def fields(self):
        """everything two results must share to be the same answer"""
        d = dict(strand=self.strand, classified=self.classified, boot_count=self.boot_count, best_count=self.best_count,
                 rank_seq=self.rank_seq, rank_count=self.rank_count)
        if self.candidates is not None:
            d["candidates"] = self.candidates
        return d

    def tobytes(self):
        return b"".join(np.ascontiguousarray(v).tobytes() for _, v in sorted(self.fields().items()))

    def record(self, q):
        """query q as a plain dict (candidates: the two strands' lists)"""
        d = dict(strand=int(self.strand[q]), classified=int(self.classified[q]), boot_count=[int(x) for x in self.boot_count[q]],
                 best_count=[int(x) for x in self.best_count[q]],
                 ranks=[(int(s), int(c)) for s, c in zip(self.rank_seq[q], self.rank_count[q])])
        if self.candidates is not None:
            d["candidates"] = [[int(x) for x in self.candidates[q, s, :int(self.boot_count[q, s])]] for s in range(2)]
        return d


def _opts(randseed, strand_both, sintax_random, want_candidates, window):
    o = SintaxOpts()
    _lib.load().vsx_sintax_opts_default(C.byref(o))
    o.randseed = int(randseed)
    o.strand_both = int(bool(strand_both))
    o.sintax_random = int(bool(sintax_random))
    o.want_candidates = int(bool(want_candidates))
    o.window = int(window)
    return o


def _numbers(query_numbers, n):
    if query_numbers is None:
        return None, None
    a = np.ascontiguousarray(query_numbers, np.uint64)
    if a.size != n:
        raise ValueError("query_numbers: one number per query")
    return a, a.ctypes.data_as(C.c_void_p)


def sintax(session, queries, randseed, strand_both=False, sintax_random=False, want_candidates=False, first_query_no=0,
           query_numbers=None, window=0):
    """Classify `queries` against the session's database (vsx_sintax).  The session's labels carry the taxonomy.  Query k has the
    number first_query_no + k (the reference numbers a file's queries from 0) or query_numbers[k]: the number seeds the query's
    random stream, so the result of a query does not depend on which call, window or position it is classified in.
    `queries`: a list of sequences, or (blob, offsets, lengths) with the sequences anywhere in the blob."""
    lib = _lib.load()
    if isinstance(queries, tuple):
        blob, off, lens = bytes(queries[0]), np.ascontiguousarray(queries[1], np.uint64), np.ascontiguousarray(queries[2], np.uint32)
    else:
        blob, off, lens = _blob(queries)
    o = _opts(randseed, strand_both, sintax_random, want_candidates, window)
    keep, qno = _numbers(query_numbers, len(lens))
    res = _lib.SintaxResult()
    check(lib.vsx_sintax(session.h, C.byref(o), len(lens), C.cast(C.c_char_p(blob), C.c_void_p), len(blob), off.ctypes.data_as(C.c_void_p),
                         lens.ctypes.data_as(C.c_void_p), int(first_query_no), qno, C.byref(res)), "vsx_sintax")
    try:
        return SintaxResult(res, want_candidates)
    finally:
        lib.vsx_sintax_result_free(C.byref(res))


def sintax_host(db, db_labels, queries, randseed, strand_both=False, sintax_random=False, want_candidates=False, first_query_no=0,
                query_numbers=None, wordlength=8, soft_mask=1, hardmask=0, threads=0):
    """The host restatement (vsx_internal_sintax_host) on a database given as text: what the device path is compared to, and
    the route of --sintax_random.  soft_mask: 0 none, 1 soft, 2 dust.  The reference's --sintax never runs DUST: its --dbmask
    dust (the default) leaves out the words over lower-case input symbols only, which is soft_mask 1 here."""
    lib = _lib.load()
    so = SearchOpts()
    lib.vsx_search_opts_default(C.byref(so))
    so.wordlength, so.soft_mask, so.hardmask, so.threads = int(wordlength), int(soft_mask), int(hardmask), int(threads)
    dblob, doff, dlens = _blob(db)
    qblob, qoff, qlens = _blob(queries)
    labels = None
    if db_labels is not None:
        if len(db_labels) != len(dlens):
            raise ValueError("db_labels: one header per sequence")
        labels = (C.c_char_p * max(len(dlens), 1))(*[l.encode() if isinstance(l, str) else bytes(l) for l in db_labels])
    o = _opts(randseed, strand_both, sintax_random, want_candidates, 0)
    keep, qno = _numbers(query_numbers, len(qlens))
    res = _lib.SintaxResult()
    check(lib.vsx_internal_sintax_host(C.byref(so), C.byref(o), len(dlens), C.cast(C.c_char_p(dblob), C.c_void_p), len(dblob),
                                       doff.ctypes.data_as(C.c_void_p), dlens.ctypes.data_as(C.c_void_p), labels, len(qlens),
                                       C.cast(C.c_char_p(qblob), C.c_void_p), len(qblob), qoff.ctypes.data_as(C.c_void_p),
                                       qlens.ctypes.data_as(C.c_void_p), int(first_query_no), qno, C.byref(res)),
          "vsx_internal_sintax_host")
    try:
        return SintaxResult(res, want_candidates)
    finally:
        lib.vsx_sintax_result_free(C.byref(res))


def intern_labels(labels):
    """(ids, start, len), each n x 9: the per-rank name ids the vote compares (vsx_internal_sintax_intern) and where each name
    lies in its label"""
    lib = _lib.load()
    n = len(labels)
    arr = (C.c_char_p * max(n, 1))(*[l.encode() if isinstance(l, str) else bytes(l) for l in labels])
    ids = np.zeros((max(n, 1), 9), np.uint32)
    start = np.zeros((max(n, 1), 9), np.int32)
    ln = np.zeros((max(n, 1), 9), np.int32)
    check(lib.vsx_internal_sintax_intern(n, arr, ids.ctypes.data_as(C.c_void_p), start.ctypes.data_as(C.c_void_p),
                                         ln.ctypes.data_as(C.c_void_p)), "vsx_internal_sintax_intern")
    return ids[:n], start[:n], ln[:n]


def tabbed_lines(result, qlabels, dblabels, cutoff=0.0):
    """The --tabbedout lines (sintax_analyse, commands/sintax.cpp): label, d:Name(0.97),..., strand, and with a cutoff above 0 a
    fourth column of the ranks whose score reaches it.  An unclassified query has empty columns."""
    _, start, ln = intern_labels(dblabels)
    raw = [l.encode() if isinstance(l, str) else bytes(l) for l in dblabels]
    lines = []
    for q in range(result.n):
        label = qlabels[q]
        if not result.classified[q]:
            lines.append(label + ("\t\t\t" if cutoff > 0.0 else "\t\t"))
            continue
        count = int(result.boot_count[q, int(result.strand[q])])
        full, cut = [], []
        for k in range(9):
            seq, votes = int(result.rank_seq[q, k]), int(result.rank_count[q, k])
            if ln[seq, k] > 0:
                name = raw[seq][start[seq, k]:start[seq, k] + ln[seq, k]].decode("latin-1")
                score = 1.0 * votes / count
                full.append("%s:%s(%.2f)" % (RANKS[k], name, score))
                if score >= cutoff:
                    cut.append("%s:%s" % (RANKS[k], name))
        line = label + "\t" + ",".join(full) + "\t" + ("-" if result.strand[q] else "+")
        if cutoff > 0.0:
            line += "\t" + ",".join(cut)
        lines.append(line)
    return lines


def log_lines(result):
    """the closing line of the reference's log"""
    line = "Classified %d of %d sequences" % (result.n_classified, result.n)
    if result.n > 0:
        line += " (%.2f%%)" % (100.0 * result.n_classified / result.n)
    return [line]
