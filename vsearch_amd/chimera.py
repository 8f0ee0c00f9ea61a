"""Chimera detection (UCHIME) over include/vsx_search.h: reference-based (vsx_uchime_ref) and de novo (vsx_uchime_denovo).

    ChimeraSession(aligner, db, labels=None, **opts)     ~ chimera() with --uchime_ref --db (core/chimera.cpp)
    .uchime_ref(queries) -> per-query dicts (the fields of chimera_result_s, parents as database indices or None)
    .uchimeout(queries, qnames, tnames) -> the --uchimeout lines, byte for byte

    DenovoChimeraSession(aligner, seqs, labels, variant="uchime", **opts)   ~ --uchime_denovo / --uchime2_denovo / --uchime3_denovo
    .uchime_denovo() -> per-sequence dicts in processing order (abundance-sorted); .order[k] = input index of record k
    .uchimeout() -> the --uchimeout lines in processing order;  .nonchimeras() -> input indices of the non-chimeras

    ChimerasDenovoSession(aligner, seqs, labels, **opts)   ~ --chimeras_denovo (long, high-quality reads; vsx_chimeras_denovo)
    .chimeras_denovo() -> per-sequence dicts in processing order;  .tabbedout() -> the --tabbedout lines (chimeras only)
    .chimeras / .nonchimeras -> the labels of --chimeras / --nonchimeras in output order

Options: minh, mindiv, mindiffs, xn, dn (the UCHIME parameters) and the searcher's soft_mask (--dbmask: 0 none, 1 soft, 2 dust =
default), qmask (--qmask when it differs: 1 + mode), hardmask, wordlength, threads, window (queries per chimera window) and
search_window (queries per window of the part search)."""
import ctypes as C

from . import _lib
from ._lib import (ChimeraDenovoOpts, ChimeraDenovoStats, ChimeraOpts, ChimeraResult, ChimerasLongOpts, ChimerasLongResult, ChimeraStats,
                   check)
from .search import _blob, _meta

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


def _records(out, n):
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


VARIANTS = {"uchime": 1, "uchime2": 2, "uchime3": 3}
MASK_MODES = {"none": 0, "soft": 1, "dust": 2}


def header_size(label):
    """the abundance of a FASTA header as header_get_size reads it (core/attributes.cpp:98-188): the first (^|;)size=DIGITS(;|$),
    found with the reference's own scan; 1 when there is none (Database::read)"""
    h = label.encode() if isinstance(label, str) else bytes(label)
    att, n, off = b"size=", len(h), 0
    while off < n - len(att):
        i = h.find(att, off)
        if i < 0:
            break
        off = i
        if off > 0 and h[off - 1:off] != b";":
            off += len(att) + 1
            continue
        d = 0
        while off + len(att) + d < n and h[off + len(att) + d] in b"0123456789":
            d += 1
        if d == 0:
            off += len(att) + 1
            continue
        if off + len(att) + d < n and h[off + len(att) + d:off + len(att) + d + 1] != b";":
            off += len(att) + d + 2
            continue
        v = int(h[off + len(att):off + len(att) + d])
        if v == 0:
            raise ValueError(f"invalid (zero) abundance annotation in header {label!r}")
        return v
    return 1


def sort_by_abundance(sizes, labels):
    """Database::sortbyabundance (core/db.cpp:471-485): abundance descending, then the header (strcmp: bytes), then input order"""
    keys = [l.encode() if isinstance(l, str) else bytes(l) for l in labels]
    return sorted(range(len(labels)), key=lambda i: (-sizes[i], keys[i], i))


def denovo_default_opts(variant="uchime"):
    """vsx_chimera_denovo_opts_default as a ChimeraDenovoOpts structure"""
    o = ChimeraDenovoOpts()
    _lib.load().vsx_chimera_denovo_opts_default(C.byref(o), VARIANTS[variant])
    return o


class DenovoChimeraSession:
    """--uchime_denovo / --uchime2_denovo / --uchime3_denovo of one set of sequences.  Sequences shorter than minseqlength (1) or
    longer than maxseqlength (50 000) are dropped as Database::read drops them; the rest are sorted like sortbyabundance.
    Options as ChimeraSession: minh, mindiv, mindiffs, xn, dn, window (sequences per speculative window), soft_mask (the --qmask
    mode of the de novo input: 0 none, 1 soft, 2 dust = default, or its name), hardmask (1: --hardmask), wordlength (3..8),
    minwordmatches, threads, search_window; plus abskew (default 2, uchime3 16)."""

    def __init__(self, aligner, seqs, labels, variant="uchime", minseqlength=1, maxseqlength=50000, **opts):
        lib = _lib.load()
        if variant not in VARIANTS:
            raise ValueError(f"variant must be one of {sorted(VARIANTS)}")
        if len(labels) != len(seqs):
            raise ValueError("labels: one header per sequence")
        self.aligner = aligner
        aligner._children.add(self)
        o = denovo_default_opts(variant)
        for k, v in opts.items():
            if k == "soft_mask" and isinstance(v, str):
                v = MASK_MODES[v]
            if k in _SEARCH_KEYS:
                setattr(o.base.search, k, v)
            elif k == "search_window":
                o.base.search.window = v
            elif k in ("minh", "mindiv", "mindiffs", "xn", "dn", "window"):
                setattr(o.base, k, v)
            elif k == "abskew":
                o.abskew = v
                o.base.search.maxsizeratio = 1.0 / v
            else:
                raise TypeError(f"unknown chimera option {k}")
        self.opts = o
        keep = [i for i, s in enumerate(seqs) if minseqlength <= len(s) <= maxseqlength]
        sizes = {i: header_size(labels[i]) for i in keep}
        kl = [labels[i] for i in keep]
        self.order = [keep[j] for j in sort_by_abundance([sizes[i] for i in keep], kl)]
        self.seqs = [seqs[i] for i in self.order]
        self.labels = [labels[i] for i in self.order]
        self.sizes = [sizes[i] for i in self.order]
        blob, off, lens = _blob(self.seqs)
        self._keep = (blob, off, lens)
        self.h = C.c_void_p()
        check(lib.vsx_searcher_create(aligner.h, C.byref(self.h), C.byref(o.base.search), len(lens),
                                      C.cast(C.c_char_p(blob), C.c_void_p), len(blob),
                                      off.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p)),
              "vsx_searcher_create")
        m, self._meta_keep = _meta(self.sizes, self.labels, len(lens))
        check(lib.vsx_searcher_set_meta(self.h, C.byref(m)), "vsx_searcher_set_meta")
        self.stats = {}
        self._records = None

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            _lib.load().vsx_searcher_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def uchime_denovo(self):
        """one dict per sequence in processing order (the fields of uchime_ref's records; parents as processing-order indices)"""
        lib = _lib.load()
        n = len(self.seqs)
        out = (ChimeraResult * max(n, 1))()
        check(lib.vsx_uchime_denovo(self.h, C.byref(self.opts), out), "vsx_uchime_denovo")
        st = ChimeraDenovoStats()
        lib.vsx_chimera_denovo_last_stats(C.byref(st))
        self.stats = {k: getattr(st, k) for k, _ in ChimeraDenovoStats._fields_}
        self._records = _records(out, n)
        return self._records

    def uchimeout(self, records=None):
        """--uchimeout lines in processing order (what the reference CLI writes)"""
        if records is None:
            records = self._records if self._records is not None else self.uchime_denovo()
        return [format_uchimeout(r, qn, self.labels) for r, qn in zip(records, self.labels)]

    def nonchimeras(self, records=None):
        """input indices of the sequences whose status is below suspicious (neither 'Y' nor '?'), in processing order"""
        if records is None:
            records = self._records if self._records is not None else self.uchime_denovo()
        return [self.order[k] for k, r in enumerate(records) if r["flag"] == "N"]


LONG_STATUS = {0: "no_parents", 3: "chimeric"}


def chimeras_long_default_opts():
    """vsx_chimeras_long_opts_default as a ChimerasLongOpts structure"""
    o = ChimerasLongOpts()
    _lib.load().vsx_chimeras_long_opts_default(C.byref(o))
    return o


def long_record(r):
    """a ChimerasLongResult as a dict: the per-parent arrays cut to n_parents"""
    n = r.n_parents
    return dict(status=LONG_STATUS[r.status], flag=r.flag.decode(), n_parents=n, alnlen=r.alnlen, parent=[int(x) for x in r.parent[:n]],
                start=list(r.start[:n]), len=list(r.len[:n]), id_query_parent=list(r.id_query_parent[:n]),
                id_query_top=r.id_query_top, divergence=r.divergence)


def format_tabbedout(rec, qname, tnames):
    """one --tabbedout line of --chimeras_denovo (eval_parents_long, chimera.cpp:1183-1239); chimeric records only"""
    ids = rec["id_query_parent"]
    third = tnames[rec["parent"][2]] if rec["n_parents"] > 2 else "*"
    return "%.4f\t%s\t%s\t%s\t%s\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\t0\t0\t0\t0\t0\t0\t%.2f\tY" % (
        99.9999, qname, tnames[rec["parent"][0]], tnames[rec["parent"][1]], third, 100.0, ids[0], ids[1],
        ids[2] if rec["n_parents"] > 2 else 0.0, rec["id_query_top"], 0.0)


class ChimerasDenovoSession:
    """--chimeras_denovo of one set of sequences: the long-read detector.  Constructor conventions as DenovoChimeraSession (length
    filter, ;size= parsing, sortbyabundance order, soft_mask = the --qmask mode, hardmask).  Options: parts (0 = by length),
    parents_max (3), length_min (10), diff_pct (0.0), abskew (1.0), window, wordlength (3..8), minwordmatches, threads,
    search_window."""

    def __init__(self, aligner, seqs, labels, minseqlength=1, maxseqlength=50000, **opts):
        lib = _lib.load()
        if len(labels) != len(seqs):
            raise ValueError("labels: one header per sequence")
        self.aligner = aligner
        aligner._children.add(self)
        o = chimeras_long_default_opts()
        for k, v in opts.items():
            if k == "soft_mask" and isinstance(v, str):
                v = MASK_MODES[v]
            if k in _SEARCH_KEYS:
                setattr(o.search, k, v)
            elif k == "search_window":
                o.search.window = v
            elif k in ("parts", "parents_max", "length_min", "diff_pct", "window"):
                setattr(o, k, v)
            elif k == "abskew":
                o.abskew = v
                o.search.maxsizeratio = 1.0 / v
            else:
                raise TypeError(f"unknown chimera option {k}")
        self.opts = o
        keep = [i for i, s in enumerate(seqs) if minseqlength <= len(s) <= maxseqlength]
        sizes = {i: header_size(labels[i]) for i in keep}
        kl = [labels[i] for i in keep]
        self.order = [keep[j] for j in sort_by_abundance([sizes[i] for i in keep], kl)]
        self.seqs = [seqs[i] for i in self.order]
        self.labels = [labels[i] for i in self.order]
        self.sizes = [sizes[i] for i in self.order]
        blob, off, lens = _blob(self.seqs)
        self._keep = (blob, off, lens)
        self.h = C.c_void_p()
        check(lib.vsx_searcher_create(aligner.h, C.byref(self.h), C.byref(o.search), len(lens),
                                      C.cast(C.c_char_p(blob), C.c_void_p), len(blob),
                                      off.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p)),
              "vsx_searcher_create")
        m, self._meta_keep = _meta(self.sizes, self.labels, len(lens))
        check(lib.vsx_searcher_set_meta(self.h, C.byref(m)), "vsx_searcher_set_meta")
        self.stats = {}
        self._records = None

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            _lib.load().vsx_searcher_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def chimeras_denovo(self):
        """one dict per sequence in processing order: status ('chimeric' / 'no_parents'), flag, n_parents, parent (processing-order
        indices), start, len, id_query_parent, id_query_top, divergence, alnlen"""
        lib = _lib.load()
        n = len(self.seqs)
        out = (ChimerasLongResult * max(n, 1))()
        check(lib.vsx_chimeras_denovo(self.h, C.byref(self.opts), out), "vsx_chimeras_denovo")
        st = ChimeraDenovoStats()
        lib.vsx_chimeras_denovo_last_stats(C.byref(st))
        self.stats = {k: getattr(st, k) for k, _ in ChimeraDenovoStats._fields_}
        self._records = [long_record(out[k]) for k in range(n)]
        return self._records

    def _recs(self):
        return self._records if self._records is not None else self.chimeras_denovo()

    def tabbedout(self, records=None):
        """--tabbedout lines in processing order (what the reference CLI writes with one thread): one per chimeric query"""
        records = records if records is not None else self._recs()
        return [format_tabbedout(r, qn, self.labels) for r, qn in zip(records, self.labels) if r["flag"] == "Y"]

    @property
    def chimeras(self):
        """labels of the --chimeras file, in output order"""
        return [qn for r, qn in zip(self._recs(), self.labels) if r["flag"] == "Y"]

    @property
    def nonchimeras(self):
        """labels of the --nonchimeras file, in output order"""
        return [qn for r, qn in zip(self._recs(), self.labels) if r["flag"] != "Y"]
