"""The last common ancestor of a query's hits (the reference's --lcaout with --lca_cutoff) over vsx_lca (include/vsx_lca.h).

    index = LcaIndex(tlabels, ctx=aligner)      the database labels, split into their nine rank names and numbered once
    res = lca(index, raw_hits, lca_cutoff=0.8)  -> LcaResult: per query n_top and depth, per level matches and the name to print
    lcaout_lines(res, qlabels, tlabels)         the --lcaout file, one line per query, as the reference CLI writes it (--threads 1)
    lca_host(tlabels, raw_hits, ...)            the same from the library's host restatement; no device

`raw_hits` is what SearchSession.search_batch_raw / search_exact_raw and MultiSearchSession.search_batch_raw return:
(first, hits, cigar blob); the blob is not needed and may be left out.  Reading and writing files stays with the caller.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import LcaOpts, LcaResult as _CResult, LcaStats, check
from .otutab import LabelBlob

LEVELS, NONE = _lib.LCA_LEVELS, _lib.LCA_NONE
RANKS = b"dkpcofgst"


def last_stats():
    s = LcaStats()
    _lib.load().vsx_lca_last_stats(C.byref(s))
    return {n: getattr(s, n) for n, _ in LcaStats._fields_}


def _hits_struct(raw_hits):
    """a vsx_hits over the caller's arrays (+ what must stay alive)"""
    first, hits = raw_hits[0], raw_hits[1]
    first = np.ascontiguousarray(first, np.uint64)
    hits = np.ascontiguousarray(hits)
    if hits.dtype.itemsize != C.sizeof(_lib.Hit):
        raise ValueError("hits: not an array of vsx_hit")
    if len(first) < 1:
        raise ValueError("first: n_queries + 1 values")
    H = _lib.Hits()
    H.n_queries, H.n_hits = len(first) - 1, len(hits)
    H.first = first.ctypes.data_as(C.POINTER(C.c_uint64))
    H.hit = C.cast(hits.ctypes.data, C.POINTER(_lib.Hit)) if len(hits) else None
    return H, (first, hits)


def _opts(lca_cutoff, maxhits, top_hits_only, threads, window):
    o = LcaOpts()
    _lib.load().vsx_lca_opts_default(C.byref(o))
    o.lca_cutoff, o.maxhits, o.top_hits_only = float(lca_cutoff), int(maxhits), int(bool(top_hits_only))
    o.threads, o.window = int(threads), int(window)
    return o


class LcaResult:
    """n_top, depth: per query.  matches, target, start, len: (n_queries, 9); at levels >= depth they are 0 / NONE.
    stats: vsx_lca_last_stats of the call."""

    def __init__(self, res, stats):
        n = int(res.n_queries)
        arr = lambda p, m: np.ctypeslib.as_array(p, shape=(m,)).copy() if m else np.zeros(0, np.uint32)  # noqa: E731
        self.n_top, self.depth = arr(res.n_top, n), arr(res.depth, n)
        self.matches, self.target = arr(res.matches, n * LEVELS).reshape(n, LEVELS), arr(res.target, n * LEVELS).reshape(n, LEVELS)
        self.start, self.len = arr(res.start, n * LEVELS).reshape(n, LEVELS), arr(res.len, n * LEVELS).reshape(n, LEVELS)
        self.stats = stats

    def arrays(self):
        """every result array as bytes: what two routes must agree on"""
        return tuple(a.tobytes() for a in (self.n_top, self.depth, self.matches, self.target, self.start, self.len))


class LcaIndex:
    """vsx_lca_index over `labels` (list of str / bytes, or LabelBlob).  ctx: an Aligner (its device runs the kernels), or None for
    a host index.  stats: vsx_lca_last_stats of the creation."""

    def __init__(self, labels, ctx=None):
        lib = _lib.load()
        T = labels if isinstance(labels, LabelBlob) else LabelBlob(labels)
        self.n, self.h = len(T), C.c_void_p()
        ts = T.struct()
        check(lib.vsx_lca_index_create(ctx.h if ctx is not None else None, C.byref(ts), C.byref(self.h)), "vsx_lca_index_create")
        self.stats = last_stats()

    def split(self):
        """(start, len) as the index holds them, (n, 9) int32 each"""
        st, ln = np.zeros((self.n, LEVELS), np.int32), np.zeros((self.n, LEVELS), np.int32)
        check(_lib.load().vsx_internal_lca_index_split(self.h, self.n, st.ctypes.data, ln.ctypes.data), "vsx_internal_lca_index_split")
        return st, ln

    def close(self):
        if self.h:
            _lib.load().vsx_lca_index_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lca(index, hits, lca_cutoff=1.0, maxhits=0, top_hits_only=False, threads=0, window=0):
    """vsx_lca.  A value the library refuses raises VsxError (VSX_EINVAL): lca_cutoff outside (0.5, 1.0], a hit whose target the
    index does not have, a `first` that does not ascend."""
    lib = _lib.load()
    H, keep = _hits_struct(hits)
    o = _opts(lca_cutoff, maxhits, top_hits_only, threads, window)
    out = _CResult()
    check(lib.vsx_lca(index.h, C.byref(o), C.byref(H), C.byref(out)), "vsx_lca")
    try:
        return LcaResult(out, last_stats())
    finally:
        lib.vsx_lca_result_free(C.byref(out))
        del keep


def lca_host(labels, hits, lca_cutoff=1.0, maxhits=0, top_hits_only=False, threads=0):
    """vsx_internal_lca_host: the reference's loops over the labels' bytes, on `threads` host threads"""
    lib = _lib.load()
    T = labels if isinstance(labels, LabelBlob) else LabelBlob(labels)
    H, keep = _hits_struct(hits)
    o = _opts(lca_cutoff, maxhits, top_hits_only, threads, 0)
    ts = T.struct()
    out = _CResult()
    check(lib.vsx_internal_lca_host(C.byref(o), C.byref(ts), C.byref(H), C.byref(out)), "vsx_internal_lca_host")
    try:
        return LcaResult(out, last_stats())
    finally:
        lib.vsx_lca_result_free(C.byref(out))
        del keep


def lcaout_lines(result, qlabels, tlabels):
    """--lcaout: one line per query in input order (bytes, WITH the newline): the label, a tab, then r:name of every level below
    the query's depth that names something, joined by commas"""
    T = tlabels if isinstance(tlabels, LabelBlob) else LabelBlob(tlabels)
    lines = []
    for q, ql in enumerate(qlabels):
        ql = ql.encode("latin-1") if isinstance(ql, str) else bytes(ql)
        parts = []
        for j in range(int(result.depth[q])):
            n = int(result.len[q, j])
            if n > 0:
                at = int(T.offsets[int(result.target[q, j])]) + int(result.start[q, j])
                parts.append(RANKS[j:j + 1] + b":" + T.blob[at:at + n])
        lines.append(ql + b"\t" + b",".join(parts) + b"\n")
    return lines
