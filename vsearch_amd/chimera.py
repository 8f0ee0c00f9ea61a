"""Chimera detection (UCHIME) over include/vsx_search.h: reference-based (vsx_uchime_ref) and de novo (vsx_uchime_denovo).

    ChimeraSession(aligner, db, labels=None, **opts)     ~ chimera() with --uchime_ref --db (core/chimera.cpp)
    .uchime_ref(queries) -> per-query dicts (the fields of chimera_result_s, parents as database indices or None)
    .uchimeout(queries, qnames, tnames) -> the --uchimeout lines, byte for byte

    DenovoChimeraSession(aligner, seqs, labels, variant="uchime", **opts)   ~ --uchime_denovo / --uchime2_denovo / --uchime3_denovo
    .uchime_denovo() -> per-sequence dicts in processing order (abundance-sorted); .order[k] = input index of record k
    .uchimeout() -> the --uchimeout lines in processing order;  .nonchimeras() -> input indices of the non-chimeras

    Both sessions (include/vsx_chimalns.h, vsx_chimera_alns):
    .uchimealns(...) -> the --uchimealns file as text, byte for byte;  .alns_raw(...) -> the rows, line ends and recomputed scores
    .chimeras_fasta / .nonchimeras_fasta / .borderline_fasta(..., fasta_score, sizeout, xsize, relabel, fasta_width) -> FASTA lines
    .summary(...) -> counts and abundances of the three verdicts
    (ChimeraSession takes the queries and their names first, as uchimeout does; DenovoChimeraSession holds its own)

    ChimerasDenovoSession(aligner, seqs, labels, **opts)   ~ --chimeras_denovo (long, high-quality reads; vsx_chimeras_denovo)
    .chimeras_denovo() -> per-sequence dicts in processing order;  .tabbedout() -> the --tabbedout lines (chimeras only)
    .chimeras / .nonchimeras -> the labels of --chimeras / --nonchimeras in output order

Options: minh, mindiv, mindiffs, xn, dn (the UCHIME parameters) and the searcher's soft_mask (--dbmask: 0 none, 1 soft, 2 dust =
default), qmask (--qmask when it differs: 1 + mode), hardmask, wordlength, threads, window (queries per chimera window) and
search_window (queries per window of the part search)."""
import ctypes as C

import numpy as np

from . import _lib
from . import sortby as _sortby
from ._lib import (ChimeraDenovoOpts, ChimeraDenovoStats, ChimeraOpts, ChimeraResult, ChimerasLongOpts, ChimerasLongResult, ChimeraStats,
                   check)
from .derep import strip_size
from .orient import _fasta, _header
from .search import _blob, _meta

NONE = 0xFFFFFFFF
STATUS = {0: "no_parents", 1: "no_alignment", 2: "scored"}
_SEARCH_KEYS = ("soft_mask", "qmask", "hardmask", "wordlength", "minwordmatches", "threads")


def format_uchimeout(rec, qname, tnames, xsize=False):
    """one --uchimeout line (without the newline): a scored query as eval_parents prints it (chimera.cpp:1810-1875), any other as the
    "no parents" line of :2320-2340.  xsize: --xsize, which strips the ;size= annotation from all four labels (header_fprint_strip)"""
    if rec["status"] != "scored":
        return "%.4f\t%s\t*\t*\t*\t*\t*\t*\t*\t*\t0\t0\t0\t0\t0\t0\t*\tN" % (0.0, _strip(qname, xsize))
    return "%.4f\t%s\t%s\t%s\t%s\t%.1f\t%.1f\t%.1f\t%.1f\t%.1f\t%d\t%d\t%d\t%d\t%d\t%d\t%.1f\t%s" % (
        rec["score"], _strip(qname, xsize), _strip(tnames[rec["parent_a"]], xsize), _strip(tnames[rec["parent_b"]], xsize),
        _strip(tnames[rec["closest"]], xsize),
        rec["id_query_model"], rec["id_query_a"], rec["id_query_b"], rec["id_a_b"], rec["id_query_top"],
        rec["left_yes"], rec["left_no"], rec["left_abstain"], rec["right_yes"], rec["right_no"], rec["right_abstain"],
        rec["divergence"], rec["flag"])


SELECT = {"Y": _lib.CHIMALNS_Y, "?": _lib.CHIMALNS_BORDERLINE, "N": _lib.CHIMALNS_N}
_STATUS_CODE = {v: k for k, v in STATUS.items()}


def _structs(records):
    """record dicts (uchime_ref / uchime_denovo) back into a ChimeraResult array"""
    out = (ChimeraResult * max(len(records), 1))()
    for k, d in enumerate(records):
        r = out[k]
        for nm, _ in ChimeraResult._fields_:
            if nm in ("pad", "status", "flag", "parent_a", "parent_b", "closest"):
                continue
            setattr(r, nm, d[nm])
        for p in ("parent_a", "parent_b", "closest"):
            setattr(r, p, NONE if d[p] is None else d[p])
        r.status = _STATUS_CODE[d["status"]]
        r.flag = d["flag"].encode()
    return out


class ChimeraAlns:
    """vsx_chimalns_out copied to the host: per rendered record j its index record[j] in the records, alnlen[j], the six rows
    rows(j) = (A, Q, B, Diffs, Votes, Model) as bytes, lines(j) = an array of (end of A, end of Q, end of B) per output line, and
    the recomputed best_i[j], h[j], counts[j] = (left_yes, left_no, left_abstain, right_yes, right_no, right_abstain)"""

    def __init__(self, out, alignwidth):
        n = int(out.n)
        self.n, self.alignwidth = n, alignwidth

        def arr(ptr, count, dtype):
            return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dtype, copy=True) if count else np.zeros(0, dtype)

        self.record = arr(out.record, n, np.uint64)
        self.alnlen = arr(out.alnlen, n, np.uint32)
        self.text_off = arr(out.text_off, n, np.uint64)
        self.text = C.string_at(out.text, int(out.text_bytes)) if out.text_bytes else b""
        self.line_first = arr(out.line_first, n + 1, np.uint64)
        self.line_end = arr(out.line_end, 3 * int(out.n_lines), np.uint32).reshape(-1, 3)
        self.best_i = arr(out.best_i, n, np.int32)
        self.h = arr(out.h, n, np.float64)
        self.counts = arr(out.counts, 6 * n, np.int32).reshape(-1, 6)
        st = _lib.ChimalnsStats()
        _lib.load().vsx_chimalns_last_stats(C.byref(st))
        self.stats = {k: getattr(st, k) for k, _ in _lib.ChimalnsStats._fields_}

    def rows(self, j):
        o, a = int(self.text_off[j]), int(self.alnlen[j])
        return tuple(self.text[o + r * a:o + (r + 1) * a] for r in range(6))

    def lines(self, j):
        return self.line_end[int(self.line_first[j]):int(self.line_first[j + 1])]

    def arrays(self):
        """everything two routes must agree on"""
        return (self.record.tobytes(), self.alnlen.tobytes(), self.text_off.tobytes(), self.text, self.line_first.tobytes(),
                self.line_end.tobytes(), self.best_i.tobytes(), self.h.tobytes(), self.counts.tobytes())


def _alns_opts(xn, dn, alignwidth, select, window, threads):
    o = _lib.ChimalnsOpts()
    _lib.load().vsx_chimalns_opts_default(C.byref(o))
    o.xn, o.dn, o.alignwidth, o.window, o.threads = xn, dn, alignwidth, window, threads
    o.select = 0
    for f in select:
        o.select |= SELECT[f]
    return o


def alns_host(q, a, b, cigar_a, cigar_b, xn=8.0, dn=1.4, alignwidth=80):
    """vsx_internal_chimalns_host: the host restatement on one (query, parent A, parent B) triple with the two alignments as CIGAR
    text (query against parent); no device"""
    lib = _lib.load()
    o = _alns_opts(xn, dn, alignwidth, "Y", 0, 0)
    enc = [s.encode() if isinstance(s, str) else bytes(s) for s in (q, a, b, cigar_a, cigar_b)]
    res = _lib.ChimalnsOut()
    check(lib.vsx_internal_chimalns_host(enc[0], len(enc[0]), enc[1], len(enc[1]), enc[2], len(enc[2]), enc[3], enc[4], C.byref(o),
                                         C.byref(res)), "vsx_internal_chimalns_host")
    try:
        return ChimeraAlns(res, alignwidth)
    finally:
        lib.vsx_chimalns_out_free(C.byref(res))


def _strip(label, xsize):
    return strip_size(label)[0] if xsize else label


def format_uchimealns(alns, j, rec, qname, qlen, tnames, tlens, xsize=False):
    """the --uchimealns block of rendered record j, as eval_parents prints it (chimera.cpp:1703-1807)"""
    a, b = rec["parent_a"], rec["parent_b"]
    out = ["\n", "-" * 72 + "\n",
           "Query   (%5d nt) %s\n" % (qlen, _strip(qname, xsize)),
           "ParentA (%5d nt) %s\n" % (tlens[a], _strip(tnames[a], xsize)),
           "ParentB (%5d nt) %s\n\n" % (tlens[b], _strip(tnames[b], xsize))]
    rows = [r.decode("latin-1") for r in alns.rows(j)]
    alnlen = int(alns.alnlen[j])
    width = alns.alignwidth if alns.alignwidth > 0 else alnlen
    pa = pq = pb = 0
    for l, (ea, eq, eb) in enumerate(alns.lines(j)):
        i = l * width
        w = min(alnlen - i, width)
        out.append("A %5d %s %d\nQ %5d %s %d\nB %5d %s %d\n" % (pa + 1, rows[0][i:i + w], ea, pq + 1, rows[1][i:i + w], eq,
                                                              pb + 1, rows[2][i:i + w], eb))
        out.append("Diffs   %s\nVotes   %s\nModel   %s\n\n" % (rows[3][i:i + w], rows[4][i:i + w], rows[5][i:i + w]))
        pa, pq, pb = int(ea), int(eq), int(eb)
    divfrac = 100.0 * rec["divergence"] / rec["id_query_top"]
    out.append("Ids.  QA %.1f%%, QB %.1f%%, AB %.1f%%, QModel %.1f%%, Div. %+.1f%%\n" % (
        rec["id_query_a"], rec["id_query_b"], rec["id_a_b"], rec["id_query_model"], divfrac))
    ly, ln, la, ry, rn, ra = (rec[k] for k in ("left_yes", "left_no", "left_abstain", "right_yes", "right_no", "right_abstain"))
    sl, sr = ln + la + ly, rn + ra + ry
    out.append("Diffs Left %d: N %d, A %d, Y %d (%.1f%%); Right %d: N %d, A %d, Y %d (%.1f%%), Score %.4f\n" % (
        sl, ln, la, ly, 100.0 * ly / sl, sr, rn, ra, ry, 100.0 * ry / sr, rec["score"]))
    return "".join(out)


def chimera_fasta(records, labels, seqs, sizes, flags, score_name=None, sizeout=False, xsize=False, relabel=None, fasta_width=80):
    """the lines of --chimeras / --borderline / --nonchimeras (fasta_print_general as chimera.cpp:2258-2363 calls it): the records
    whose flag is in `flags`, numbered per file; score_name ('uchime_ref' / 'uchime_denovo', --fasta_score) appends best_h = max(h, 0)"""
    out, ordinal = [], 0
    for k, r in enumerate(records):
        if r["flag"] not in flags:
            continue
        ordinal += 1
        head = _header(labels[k], sizes[k], ordinal, sizeout, relabel, xsize)
        if score_name:
            merged = relabel is None and not sizeout and head.endswith(";")
            head += ("" if merged else ";") + "%s=%.4f" % (score_name, max(r["score"], 0.0))
        out += _fasta(head, seqs[k], fasta_width)
    return out


def chimera_summary(records, sizes):
    """counts and abundances of the chimeric ('Y'), borderline ('?') and non-chimeric records"""
    s = dict(chimeras=0, borderline=0, nonchimeras=0, chimera_abundance=0, borderline_abundance=0, nonchimera_abundance=0)
    for r, z in zip(records, sizes):
        key = {"Y": ("chimeras", "chimera_abundance"), "?": ("borderline", "borderline_abundance")}.get(r["flag"], ("nonchimeras", "nonchimera_abundance"))
        s[key[0]] += 1
        s[key[1]] += z
    s["total"], s["total_abundance"] = len(records), sum(sizes[:len(records)])
    return s


class _Writers:
    """the FASTA writers and the summary both sessions share.  The leading arguments are the session's: (queries, qnames=None) for
    ChimeraSession, none for DenovoChimeraSession; _source(...) turns them into (records, labels, sequences as printed, abundances)"""

    def _fasta_file(self, flags, src, records, fasta_score, kw):
        recs, labels, seqs, sizes = self._source(*src, records=records)
        return chimera_fasta(recs, labels, seqs, sizes, flags, self.SCORE_NAME if fasta_score else None, **kw)

    def chimeras_fasta(self, *src, records=None, fasta_score=False, **kw):
        """--chimeras lines; fasta_score, sizeout, xsize, relabel, fasta_width as the CLI's options"""
        return self._fasta_file("Y", src, records, fasta_score, kw)

    def borderline_fasta(self, *src, records=None, fasta_score=False, **kw):
        """--borderline lines"""
        return self._fasta_file("?", src, records, fasta_score, kw)

    def nonchimeras_fasta(self, *src, records=None, fasta_score=False, **kw):
        """--nonchimeras lines"""
        return self._fasta_file("N", src, records, fasta_score, kw)

    def summary(self, *src, records=None):
        """counts and abundances of chimeras, borderline sequences and non-chimeras"""
        recs, _, _, sizes = self._source(*src, records=records)
        return chimera_summary(recs, sizes)

    def _alns(self, n, blob, off, lens, records, alignwidth, select, window, threads):
        lib = _lib.load()
        o = _alns_opts(self._base_opts.xn, self._base_opts.dn, alignwidth, select, window, threads)
        res = _lib.ChimalnsOut()
        recs = _structs(records)
        if blob is None:
            rc = lib.vsx_chimera_alns(self.h, C.byref(o), C.c_uint64(n), None, C.c_uint64(0), None, None, recs, C.byref(res))
        else:
            rc = lib.vsx_chimera_alns(self.h, C.byref(o), C.c_uint64(n), C.cast(C.c_char_p(blob), C.c_void_p), C.c_uint64(len(blob)),
                                      off.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), recs, C.byref(res))
        check(rc, "vsx_chimera_alns")
        try:
            return ChimeraAlns(res, alignwidth)
        finally:
            lib.vsx_chimalns_out_free(C.byref(res))


def default_opts():
    """vsx_chimera_opts_default as a ChimeraOpts structure"""
    o = ChimeraOpts()
    _lib.load().vsx_chimera_opts_default(C.byref(o))
    return o


class ChimeraSession(_Writers):
    SCORE_NAME = "uchime_ref"

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
        self._base_opts = o
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

    def uchimeout(self, queries, qnames=None, tnames=None, records=None, xsize=False):
        """--uchimeout lines in query order (what the reference CLI writes with --threads 1); xsize as --xsize"""
        if records is None:
            records = self.uchime_ref(queries)
        qnames = qnames or [f"q{i}" for i in range(len(queries))]
        tnames = tnames or self.labels or [f"t{i}" for i in range(len(self.db))]
        return [format_uchimeout(r, qn, tnames, xsize) for r, qn in zip(records, qnames)]

    def _source(self, queries, qnames=None, records=None):
        qnames = qnames or [f"q{i}" for i in range(len(queries))]
        records = records if records is not None else self.uchime_ref(queries)
        return records, qnames, queries, [header_size(q) for q in qnames]

    def alns_raw(self, queries, records=None, alignwidth=80, select="Y", window=0, threads=0):
        """the alignment blocks of the selected records (flags in `select`: 'Y', '?', scored 'N') as a ChimeraAlns"""
        records = records if records is not None else self.uchime_ref(queries)
        blob, off, lens = _blob(queries)
        return self._alns(len(lens), blob, off, lens, records, alignwidth, select, window, threads)

    def uchimealns(self, queries, qnames=None, tnames=None, records=None, alignwidth=80, xsize=False):
        """the --uchimealns file as text, byte for byte: one block per chimeric query, in query order"""
        records = records if records is not None else self.uchime_ref(queries)
        qnames = qnames or [f"q{i}" for i in range(len(queries))]
        tnames = tnames or self.labels or [f"t{i}" for i in range(len(self.db))]
        alns = self.alns_raw(queries, records, alignwidth)
        tlens = [len(t) for t in self.db]
        return "".join(format_uchimealns(alns, j, records[k], qnames[k], len(queries[k]), tnames, tlens, xsize)
                       for j, k in enumerate(int(x) for x in alns.record))


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


def _abundance_order(aligner, sizes, labels, lengths):
    """sort_by_abundance's list from the aligner's device (vsx_sortby, vsearch_amd/sortby.py).  What that call refuses -- an abundance
    the reference's unsigned int cannot hold, a header with a NUL byte -- is sorted here, by the same rule."""
    keys = [l.encode() if isinstance(l, str) else bytes(l) for l in labels]
    if any(v > 0xFFFFFFFF for v in sizes) or any(b"\0" in k for k in keys):
        return sort_by_abundance(sizes, labels)
    return _sortby.db_order(aligner, keys, lengths, sizes, _lib.SORTBY_SIZE)


def denovo_default_opts(variant="uchime"):
    """vsx_chimera_denovo_opts_default as a ChimeraDenovoOpts structure"""
    o = ChimeraDenovoOpts()
    _lib.load().vsx_chimera_denovo_opts_default(C.byref(o), VARIANTS[variant])
    return o


class DenovoChimeraSession(_Writers):
    """--uchime_denovo / --uchime2_denovo / --uchime3_denovo of one set of sequences.  Sequences shorter than minseqlength (1) or
    longer than maxseqlength (50 000) are dropped as Database::read drops them; the rest are sorted like sortbyabundance.
    Options as ChimeraSession: minh, mindiv, mindiffs, xn, dn, window (sequences per speculative window), soft_mask (the --qmask
    mode of the de novo input: 0 none, 1 soft, 2 dust = default, or its name), hardmask (1: --hardmask), wordlength (3..8),
    minwordmatches, threads, search_window; plus abskew (default 2, uchime3 16)."""

    SCORE_NAME = "uchime_denovo"

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
        self._base_opts = o.base
        keep = [i for i, s in enumerate(seqs) if minseqlength <= len(s) <= maxseqlength]
        sizes = {i: header_size(labels[i]) for i in keep}
        kl = [labels[i] for i in keep]
        self.order = [keep[j] for j in _abundance_order(aligner, [sizes[i] for i in keep], kl, [len(seqs[i]) for i in keep])]
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
        self._masked = None

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

    def uchimeout(self, records=None, xsize=False):
        """--uchimeout lines in processing order (what the reference CLI writes); xsize as --xsize"""
        if records is None:
            records = self._records if self._records is not None else self.uchime_denovo()
        return [format_uchimeout(r, qn, self.labels, xsize) for r, qn in zip(records, self.labels)]

    def nonchimeras(self, records=None):
        """input indices of the sequences whose status is below suspicious (neither 'Y' nor '?'), in processing order"""
        if records is None:
            records = self._records if self._records is not None else self.uchime_denovo()
        return [self.order[k] for k, r in enumerate(records) if r["flag"] == "N"]

    def _recs(self, records=None):
        if records is not None:
            return records
        return self._records if self._records is not None else self.uchime_denovo()

    def masked_text(self):
        """the sequences in processing order as the reference holds and prints them (chimera.cpp:2546-2555): DUST-masked for qmask
        dust (upper case, masked symbols lower case or, with hardmask, 'N'), hard-masked for soft + hardmask, as given otherwise.
        (The searcher's own text keeps masked ambiguity codes in upper case, so the device masker writes this one.)"""
        if self._masked is None:
            so = self.opts.base.search
            mode, hard = int(so.soft_mask), bool(so.hardmask & 1)
            if mode == 0 or (mode == 1 and not hard):
                self._masked = list(self.seqs)
            else:
                from .mask import fastx_mask
                res = fastx_mask(self.aligner, self.seqs, qmask=mode, hardmask=hard, want_bits=False)
                self._masked = [t.decode("latin-1") for t in res.text()]
        return self._masked

    def _source(self, records=None):
        return self._recs(records), self.labels, self.masked_text(), self.sizes

    def alns_raw(self, records=None, alignwidth=80, select="Y", window=0, threads=0):
        """the alignment blocks of the selected records (flags in `select`: 'Y', '?', scored 'N') as a ChimeraAlns"""
        return self._alns(len(self.seqs), None, None, None, self._recs(records), alignwidth, select, window, threads)

    def uchimealns(self, records=None, alignwidth=80, xsize=False):
        """the --uchimealns file as text, byte for byte: one block per chimeric sequence, in processing order"""
        records = self._recs(records)
        alns = self.alns_raw(records, alignwidth)
        tlens = [len(t) for t in self.seqs]
        return "".join(format_uchimealns(alns, j, records[k], self.labels[k], tlens[k], self.labels, tlens, xsize)
                       for j, k in enumerate(int(x) for x in alns.record))


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
        self.order = [keep[j] for j in _abundance_order(aligner, [sizes[i] for i in keep], kl, [len(seqs[i]) for i in keep])]
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
