"""Reference-based chimera detection (--uchime_ref, default UCHIME algorithm) over include/vsx_search.h vsx_uchime_ref.

    ChimeraSession(aligner, db, labels=None, **opts)     ~ chimera() with --uchime_ref --db (core/chimera.cpp)
    .uchime_ref(queries) -> per-query dicts (the fields of chimera_result_s, parents as database indices or None)
    .uchimeout(queries, qnames, tnames) -> the --uchimeout lines, byte for byte

Options: minh, mindiv, mindiffs, xn, dn (the UCHIME parameters) and the searcher's soft_mask (--dbmask: 0 none, 1 soft, 2 dust =
default), qmask (--qmask when it differs: 1 + mode), hardmask, wordlength, threads, window (queries per chimera window) and
search_window (queries per window of the part search)."""
import ctypes as C

from . import _lib
from ._lib import ChimeraOpts, ChimeraResult, ChimeraStats, check
from .search import _blob

NONE = 0xFFFFFFFF
STATUS = {0: "no_parents", 1: "no_alignment", 2: "scored"}
_SEARCH_KEYS = ("soft_mask", "qmask", "hardmask", "wordlength", "minwordmatches", "threads")


def format_uchimeout(rec, qname, tnames):
    """one --uchimeout line (without the newline): a scored query as eval_parents prints it (chimera.cpp:1810-1875), any other as the
    "no parents" line of :2320-2340"""
    if rec["status"] != "scored":
        return "%.4f\t%s\t*\t*\t*\t*\t*\t*\t*\t*\t0\t0\t0\t0\t0\t0\t*\tN" % (0.0, qname)
    return "%.4f\t%s\t%s\t%s\t%s\t%.1f\t%.1f\t%.1f\t%.1f\t%.1f\t%d\t%d\t%d\t%d\t%d\t%d\t%.1f\t%s" % (
        rec["score"], qname, tnames[rec["parent_a"]], tnames[rec["parent_b"]], tnames[rec["closest"]],
        rec["id_query_model"], rec["id_query_a"], rec["id_query_b"], rec["id_a_b"], rec["id_query_top"],
        rec["left_yes"], rec["left_no"], rec["left_abstain"], rec["right_yes"], rec["right_no"], rec["right_abstain"],
        rec["divergence"], rec["flag"])


def default_opts():
    """vsx_chimera_opts_default as a ChimeraOpts structure"""
    o = ChimeraOpts()
    _lib.load().vsx_chimera_opts_default(C.byref(o))
    return o


class ChimeraSession:
    def __init__(self, aligner, db, labels=None, **opts):
        lib = _lib.load()
        self.aligner = aligner
        aligner._children.add(self)
        o = default_opts()
        for k, v in opts.items():
            if k in _SEARCH_KEYS:
                setattr(o.search, k, v)
            elif k == "search_window":
                o.search.window = v
            elif k in ("minh", "mindiv", "mindiffs", "xn", "dn", "window"):
                setattr(o, k, v)
            else:
                raise TypeError(f"unknown chimera option {k}")
        self.opts = o
        self.db = list(db)
        self.labels = list(labels) if labels is not None else None
        blob, off, lens = _blob(self.db)
        self._keep = (blob, off, lens)
        self.h = C.c_void_p()
        check(lib.vsx_searcher_create(aligner.h, C.byref(self.h), C.byref(o.search), len(lens),
                                      C.cast(C.c_char_p(blob), C.c_void_p), len(blob),
                                      off.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p)),
              "vsx_searcher_create")
        self.stats = {}

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            _lib.load().vsx_searcher_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def uchime_ref(self, queries):
        """one dict per query: score, parent_a / parent_b / closest (database index or None), status ('scored', 'no_parents',
        'no_alignment'), id_query_model .. id_query_top, left/right yes/no/abstain, divergence, flag"""
        lib = _lib.load()
        blob, off, lens = _blob(queries)
        n = len(lens)
        out = (ChimeraResult * max(n, 1))()
        check(lib.vsx_uchime_ref(self.h, C.byref(self.opts), C.c_uint64(n), C.cast(C.c_char_p(blob), C.c_void_p), C.c_uint64(len(blob)),
                                 off.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), out), "vsx_uchime_ref")
        st = ChimeraStats()
        lib.vsx_chimera_last_stats(C.byref(st))
        self.stats = {k: getattr(st, k) for k, _ in ChimeraStats._fields_}
        recs = []
        for k in range(n):
            r = out[k]
            d = {nm: getattr(r, nm) for nm, _ in ChimeraResult._fields_ if nm != "pad"}
            for p in ("parent_a", "parent_b", "closest"):
                d[p] = None if d[p] == NONE else int(d[p])
            d["status"] = STATUS[d["status"]]
            d["flag"] = d["flag"].decode()
            recs.append(d)
        return recs

    def uchimeout(self, queries, qnames=None, tnames=None, records=None):
        """--uchimeout lines in query order (what the reference CLI writes with --threads 1)"""
        if records is None:
            records = self.uchime_ref(queries)
        qnames = qnames or [f"q{i}" for i in range(len(queries))]
        tnames = tnames or self.labels or [f"t{i}" for i in range(len(self.db))]
        return [format_uchimeout(r, qn, tnames) for r, qn in zip(records, qnames)]
