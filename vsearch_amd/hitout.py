"""The search writers over include/vsx_hitout.h: --alnout, --samout, --blast6out, --fastapairs, --qsegout, --tsegout and all 43
--userout fields of the reference's search commands (core/results.cpp, core/showalign.cpp, commands/usearch_global.cpp:150-326).

    render(session, queries, raw_hits, want=...)   -> RenderedHits: the gapped rows, symbol rows and MD strings, made on the GPU
    render_host(db_text, queries, raw_hits, ...)   -> the same from the library's host restatement; no device
    alnout_text / sam_lines / sam_header_lines / blast6_lines / fastapairs_lines / qsegout_lines / tsegout_lines / userout_lines

`raw_hits` is what SearchSession.search_batch_raw / search_exact_raw return: (first, hits, cigar blob).  The formatters are plain
Python over the rendered bytes and the fields of vsx_hit; each gives the text of the reference CLI run with --threads 1.  A `*_lines`
result is the file's lines without their newlines.  Only fasta_width is honoured of the FASTA options; relabelling and the size
options are out of scope.
"""
import ctypes as C
import hashlib

import numpy as np

from . import _lib
from ._lib import check
from .search import _blob

ROWS, SYMBOLS, SAM = _lib.HITOUT_ROWS, _lib.HITOUT_SYMBOLS_ROW, _lib.HITOUT_SAM
ALL = ROWS | SYMBOLS | SAM

# utils/userfields.cpp, in the reference's order
USERFIELDS = ("query", "target", "evalue", "id", "pctpv", "pctgaps", "pairs", "gaps", "qlo", "qhi", "tlo", "thi", "pv", "ql", "tl", "qs",
              "ts", "alnlen", "opens", "exts", "raw", "bits", "aln", "caln", "qstrand", "tstrand", "qrow", "trow", "qframe", "tframe",
              "mism", "ids", "qcov", "tcov", "id0", "id1", "id2", "id3", "id4", "qilo", "qihi", "tilo", "tihi")


def _hits_struct(raw_hits, n_queries):
    """a vsx_hits over the caller's arrays (+ what must stay alive)"""
    first, hits, cig = raw_hits
    first = np.ascontiguousarray(first, np.uint64)
    hits = np.ascontiguousarray(hits)
    if hits.dtype.itemsize != C.sizeof(_lib.Hit):
        raise ValueError("hits: not an array of vsx_hit")
    cig = bytes(cig)
    cbuf = C.create_string_buffer(cig, max(len(cig), 1))
    H = _lib.Hits()
    H.n_queries, H.n_hits = n_queries, len(hits)
    H.first = first.ctypes.data_as(C.POINTER(C.c_uint64))
    H.hit = C.cast(hits.ctypes.data, C.POINTER(_lib.Hit))
    H.cigar_blob = C.cast(cbuf, C.POINTER(C.c_char))
    H.cigar_bytes = len(cig)
    return H, (first, hits, cbuf)


class RenderedHits:
    """The copies of a vsx_hit_text plus what the formatters read beside it: the hits, the query lengths, the database text."""

    def __init__(self, res, raw_hits, qlens, targets):
        n, nh = int(res.n_queries), int(res.n_hits)
        self.want, self.both = int(res.want), bool(res.both)
        self.first, self.hits, self.cigar_blob = np.asarray(raw_hits[0]), np.asarray(raw_hits[1]), bytes(raw_hits[2])
        self.qlens, self.targets = [int(x) for x in qlens], targets
        arr = lambda p, k, dt: np.ctypeslib.as_array(p, shape=(max(k, 1),))[:k].astype(dt, copy=True) if p else None
        self.row_blob = C.string_at(res.row_blob, int(res.row_bytes)) if res.row_blob else b""
        self.md_blob = C.string_at(res.md_blob, int(res.md_bytes)) if res.md_blob else b""
        self.qtext = C.string_at(res.qtext, int(res.qtext_bytes)) if res.qtext else b""
        self.row_len = arr(res.row_len, nh, np.uint32)
        self.qrow_off, self.trow_off = arr(res.qrow_off, nh, np.uint64), arr(res.trow_off, nh, np.uint64)
        self.sym_off, self.aln_off = arr(res.sym_off, nh, np.uint64), arr(res.aln_off, nh, np.uint64)
        self.md_off, self.md_len = arr(res.md_off, nh, np.uint64), arr(res.md_len, nh, np.uint32)
        self.qplus_off, self.qminus_off = arr(res.qplus_off, n, np.uint64), arr(res.qminus_off, n, np.uint64)
        self.stats = last_stats()

    ARRAYS = ("row_len", "qrow_off", "trow_off", "sym_off", "aln_off", "md_off", "md_len", "qplus_off", "qminus_off")
    BLOBS = ("row_blob", "md_blob", "qtext")

    def same_as(self, other):
        """the first array or blob that differs from `other`'s, or None"""
        for n in self.ARRAYS:
            a, b = getattr(self, n), getattr(other, n)
            if (a is None) != (b is None) or (a is not None and not np.array_equal(a, b)):
                return n
        for n in self.BLOBS:
            if getattr(self, n) != getattr(other, n):
                return n
        return None

    def _row(self, off, h):
        if off is None:
            raise ValueError("this row was not asked for (want)")
        o = int(off[h])
        return self.row_blob[o:o + int(self.row_len[h])].decode("latin-1")

    def qrow(self, h):
        return self._row(self.qrow_off, h)

    def trow(self, h):
        return self._row(self.trow_off, h)

    def symbols(self, h):
        return self._row(self.sym_off, h)

    def alnrow(self, h):
        """the query row --alnout shows (a minus-strand hit: the plus strand's masked text backwards, complemented)"""
        return self._row(self.aln_off, h)

    def md(self, h):
        if self.md_off is None:
            raise ValueError("the MD strings were not asked for (want)")
        o = int(self.md_off[h])
        return self.md_blob[o:o + int(self.md_len[h])].decode("latin-1")

    def qstrand(self, q, minus=False):
        """the masked text of a query strand"""
        o = int((self.qminus_off if minus else self.qplus_off)[q])
        return self.qtext[o:o + self.qlens[q]].decode("latin-1")

    def cigar(self, h):
        o = int(self.hits[h]["cigar_off"])
        return self.cigar_blob[o:self.cigar_blob.index(b"\0", o)].decode()


def last_stats():
    st = _lib.HitoutStats()
    _lib.load().vsx_hits_render_last_stats(C.byref(st))
    return {n: getattr(st, n) for n, _ in _lib.HitoutStats._fields_}


def _opts(want, threads, window):
    o = _lib.HitoutOpts()
    _lib.load().vsx_hitout_opts_default(C.byref(o))
    o.want, o.threads, o.window = int(want), int(threads), int(window)
    return o


def _queries(queries):
    """list of sequences, or an explicit (blob, offsets, lengths) as the C call takes it"""
    if isinstance(queries, tuple):
        blob, off, lens = queries
        return bytes(blob), np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(lens, np.uint32)
    return _blob(queries)


def render(session, queries, raw_hits, want=ALL, threads=0, window=0):
    """vsx_hits_render: rows, symbols and MD strings of the hits of `queries` (as handed to the search) on the session's device.
    A MultiSearchSession renders with its replica 0."""
    lib = _lib.load()
    handle = session.h
    if hasattr(session, "n_devices"):
        lib.vsx_multi_searcher_replica.restype = C.c_void_p
        lib.vsx_multi_searcher_replica.argtypes = [C.c_void_p, C.c_int32]
        handle = C.c_void_p(lib.vsx_multi_searcher_replica(session.h, 0))
    blob, off, lens = _queries(queries)
    H, keep = _hits_struct(raw_hits, len(lens))
    o = _opts(want, threads, window)
    res = _lib.HitText()
    check(lib.vsx_hits_render(handle, C.byref(o), len(lens), C.cast(C.c_char_p(blob), C.c_void_p), len(blob), off.ctypes.data_as(C.c_void_p),
                              lens.ctypes.data_as(C.c_void_p), C.byref(H), C.byref(res)), "vsx_hits_render")
    try:
        targets = session.masked_db_text() if hasattr(session, "masked_db_text") else _masked_text(lib, handle, session.db)
        return RenderedHits(res, raw_hits, lens, targets)
    finally:
        lib.vsx_hit_text_free(C.byref(res))


def _masked_text(lib, handle, db):
    blob, off, lens = _blob(db)
    lib.vsx_searcher_db_text.restype = C.c_uint64
    buf = C.create_string_buffer(max(1, len(blob)))
    n = lib.vsx_searcher_db_text(handle, buf, C.c_uint64(len(blob)))
    raw = buf.raw[:int(n)]
    return [raw[int(o):int(o) + int(l)].decode("latin-1") for o, l in zip(off, lens)]


def render_host(db_text, queries, raw_hits, want=ALL, threads=0, scoring=None, n_mismatch=False, **search_opts):
    """vsx_internal_hits_render_host: the host restatement on a database given as text AS INDEXED (it is not masked again).
    search_opts: the searcher's soft_mask / qmask / hardmask / strand_both."""
    from .aligner import DEFAULT_SCORING
    lib = _lib.load()
    so = _lib.SearchOpts()
    lib.vsx_search_opts_default(C.byref(so))
    for k, v in search_opts.items():
        if not hasattr(so, k):
            raise TypeError(f"unknown search option {k}")
        setattr(so, k, v)
    sc = scoring
    if sc is None:
        sc = _lib.Scoring()
        for k, v in DEFAULT_SCORING.items():
            setattr(sc, k, int(v))
        sc.n_mismatch = 1 if n_mismatch else 0
    db_text = [t.decode("latin-1") if isinstance(t, bytes) else t for t in db_text]
    dblob, doff, dlens = _blob([t.encode("latin-1") for t in db_text])
    blob, off, lens = _queries(queries)
    H, keep = _hits_struct(raw_hits, len(lens))
    o = _opts(want, threads, 0)
    res = _lib.HitText()
    check(lib.vsx_internal_hits_render_host(C.byref(sc), C.byref(so), C.byref(o), len(dlens), C.cast(C.c_char_p(dblob), C.c_void_p), len(dblob),
                                            doff.ctypes.data_as(C.c_void_p), dlens.ctypes.data_as(C.c_void_p), len(lens),
                                            C.cast(C.c_char_p(blob), C.c_void_p), len(blob), off.ctypes.data_as(C.c_void_p),
                                            lens.ctypes.data_as(C.c_void_p), C.byref(H), C.byref(res)), "vsx_internal_hits_render_host")
    try:
        return RenderedHits(res, raw_hits, lens, db_text)
    finally:
        lib.vsx_hit_text_free(C.byref(res))


# ---- which hits a writer sees (search_output_results, commands/usearch_global.cpp:150-326) -------------------------------------------
def reported(text, q, maxhits=0, top_hits_only=False):
    """the hit numbers of query q the writers print: the first maxhits (0: all), cut at the first one below the top identity"""
    a, b = int(text.first[q]), int(text.first[q + 1])
    if maxhits and maxhits > 0:
        b = min(b, a + int(maxhits))
    out = []
    for h in range(a, b):
        if top_hits_only and text.hits[h]["id"] < text.hits[a]["id"]:
            break
        out.append(h)
    return out


def _runs(cigar):
    out, n = [], 0
    digits = False
    for ch in cigar:
        if ch.isdigit():
            n, digits = n * 10 + int(ch), True
        else:
            out.append((n if digits else 1, ch))
            n, digits = 0, False
    return out


def _fold(seq, width):
    """fasta_print_sequence (core/fasta.cpp:423-450)"""
    if width < 1:
        return [seq]
    return [seq[i:i + width] for i in range(0, len(seq), width)]


# ---- --alnout (results_show_alnout, results.cpp:690-788; align_show, showalign.cpp:193-367) ------------------------------------------
def alnout_text(text, qlabels, tlabels, rowlen=64, maxhits=0, top_hits_only=False, output_no_hits=False, head=None):
    """head: the two lines the CLI opens the file with (its command line and its banner), or None for the records alone"""
    out = [l + "\n" for l in (head or ())]
    for q in range(len(text.first) - 1):
        a, b = int(text.first[q]), int(text.first[q + 1])
        toreport = min(b - a, int(maxhits)) if maxhits and maxhits > 0 else b - a
        if toreport == 0:
            if output_no_hits:
                out.append(f"\nQuery >{qlabels[q]}\nNo hits\n")
            continue
        hs = reported(text, q, maxhits, top_hits_only)
        qlen = text.qlens[q]
        out.append(f"\nQuery >{qlabels[q]}\n %Id   TLen  Target\n")
        for h in hs:
            x = text.hits[h]
            t = int(x["target"])
            out.append("%3.0f%% %6d  %s\n" % (x["id"], len(text.targets[t]), tlabels[t]))
        for h in hs:
            x = text.hits[h]
            t, minus = int(x["target"]), bool(x["strand"])
            tlen = len(text.targets[t])
            nw = max(len(str(qlen)), len(str(tlen)))
            out.append("\n Query %*dnt >%s\nTarget %*dnt >%s\n" % (nw, qlen, qlabels[q], nw, tlen, tlabels[t]))
            width = rowlen if rowlen else qlen + tlen
            c0, ilen = int(x["trim_q_left"]) + int(x["trim_t_left"]), int(x["internal_alignmentlength"])
            ops = "".join(op * n for n, op in _runs(text.cigar(h)))[c0:c0 + ilen]
            qr, sy, tr = text.alnrow(h), text.symbols(h), text.trow(h)
            qpos = qlen - 1 - int(x["trim_q_left"]) if minus else int(x["trim_q_left"])
            tpos = int(x["trim_t_left"])
            for i in range(0, ilen, max(width, 1)):
                chunk = ops[i:i + width]
                qstart, tstart = qpos, tpos
                nq = chunk.count("M") + chunk.count("D")
                qpos += -nq if minus else nq
                tpos += chunk.count("M") + chunk.count("I")
                out.append("\n%*s %*d %c %s %d\n" % (3, "Qry", nw, min(qstart + 1, qlen), "-" if minus else "+", qr[i:i + width],
                                                    qpos + 2 if minus else qpos))
                out.append("%*s %*s   %s\n" % (3, "", nw, "", sy[i:i + width]))
                out.append("%*s %*d %c %s %d\n" % (3, "Tgt", nw, min(tstart + 1, tlen), "+", tr[i:i + width], tpos))
            out.append("\n%d cols, %d ids (%3.1f%%), %d gaps (%3.1f%%)\n" % (
                ilen, x["matches"], x["id"], x["internal_indels"], 100.0 * int(x["internal_indels"]) / ilen if ilen > 0 else 0.0))
    return "".join(out)


# ---- --samout (results_show_samout / results_show_samheader, results.cpp:922-1071) ---------------------------------------------------
def sam_header_lines(db, tlabels, dbname, prog_version, command_line, prog_name="vsearch"):
    """`db`: the database sequences AS READ -- the reference writes the header before it masks the database
    (commands/usearch_global.cpp:568-583); M5 is over what get_hex_seq_digest_md5 hashes: the upper case with U as T"""
    lines = ["@HD\tVN:1.0\tSO:unsorted\tGO:query"]
    for t, seq in enumerate(db):
        m5 = hashlib.md5(seq.upper().replace("U", "T").encode("latin-1")).hexdigest()
        lines.append(f"@SQ\tSN:{tlabels[t]}\tLN:{len(seq)}\tM5:{m5}\tUR:file:{dbname}")
    lines.append(f"@PG\tID:{prog_name}\tVN:{prog_version}\tCL:{command_line}")
    return lines


def sam_lines(text, qlabels, tlabels, maxhits=0, top_hits_only=False, output_no_hits=False):
    lines = []
    for q in range(len(text.first) - 1):
        a, b = int(text.first[q]), int(text.first[q + 1])
        toreport = min(b - a, int(maxhits)) if maxhits and maxhits > 0 else b - a
        if toreport == 0:
            if output_no_hits:
                lines.append(f"{qlabels[q]}\t4\t*\t0\t255\t*\t*\t0\t0\t{text.qstrand(q)}\t*")
            continue
        for k, h in enumerate(reported(text, q, maxhits, top_hits_only)):
            x = text.hits[h]
            minus = int(x["strand"])
            cigar = "".join(f"{n}{'D' if op == 'I' else 'I' if op == 'D' else op}" for n, op in _runs(text.cigar(h)))
            lines.append("%s\t%d\t%s\t1\t255\t%s\t*\t0\t0\t%s\t*\tAS:i:%.0f\tXN:i:0\tXM:i:%d\tXO:i:%d\tXG:i:%d\tNM:i:%d\tMD:Z:%s\tYT:Z:UU" % (
                qlabels[q], (0x10 * minus) | (0x100 if k > 0 else 0), tlabels[int(x["target"])], cigar, text.qstrand(q, bool(minus)),
                x["id"], x["mismatches"], x["internal_gaps"], x["internal_indels"], int(x["mismatches"]) + int(x["internal_indels"]),
                text.md(h)))
    return lines


# ---- the per-hit writers ---------------------------------------------------------------------------------------------------------------
def _per_hit(text, maxhits, top_hits_only):
    """(q, h) of every hit the per-hit writers print, and (q, None) for a query without a reported hit"""
    for q in range(len(text.first) - 1):
        hs = reported(text, q, maxhits, top_hits_only)
        if hs:
            for h in hs:
                yield q, h
        else:
            yield q, None


def blast6_lines(text, qlabels, tlabels, maxhits=0, top_hits_only=False, output_no_hits=False):
    lines = []
    for q, h in _per_hit(text, maxhits, top_hits_only):
        if h is None:
            if output_no_hits:
                lines.append(f"{qlabels[q]}\t*\t0.0\t0\t0\t0\t0\t0\t0\t0\t-1\t0")
            continue
        x = text.hits[h]
        t, qlen = int(x["target"]), text.qlens[q]
        lines.append("%s\t%s\t%.1f\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d" % (
            qlabels[q], tlabels[t], x["id"], x["internal_alignmentlength"], x["mismatches"], x["internal_gaps"],
            qlen if x["strand"] else 1, 1 if x["strand"] else qlen, 1, len(text.targets[t]), -1, 0))
    return lines


def fastapairs_lines(text, qlabels, tlabels, fasta_width=80, maxhits=0, top_hits_only=False):
    lines = []
    for q, h in _per_hit(text, maxhits, top_hits_only):
        if h is None:
            continue
        lines += [">" + qlabels[q]] + _fold(text.qrow(h), fasta_width)
        lines += [">" + tlabels[int(text.hits[h]["target"])]] + _fold(text.trow(h), fasta_width) + [""]
    return lines


def qsegout_lines(text, qlabels, fasta_width=80, maxhits=0, top_hits_only=False):
    lines = []
    for q, h in _per_hit(text, maxhits, top_hits_only):
        if h is None:
            continue
        x = text.hits[h]
        seg = text.qstrand(q, bool(x["strand"]))[int(x["trim_q_left"]):text.qlens[q] - int(x["trim_q_right"])]
        lines += [">" + qlabels[q]] + _fold(seg, fasta_width)
    return lines


def tsegout_lines(text, tlabels, fasta_width=80, maxhits=0, top_hits_only=False):
    lines = []
    for q, h in _per_hit(text, maxhits, top_hits_only):
        if h is None:
            continue
        x = text.hits[h]
        t = int(x["target"])
        seg = text.targets[t][int(x["trim_t_left"]):len(text.targets[t]) - int(x["trim_t_right"])]
        lines += [">" + tlabels[t]] + _fold(seg, fasta_width)
    return lines


def _userfield(text, f, q, h, qlabels, tlabels):
    """one field of results_show_userout_one (results.cpp:330-542); h None: the no-hit form"""
    qlen = text.qlens[q]
    x = text.hits[h] if h is not None else None
    t = int(x["target"]) if x is not None else None
    tlen = len(text.targets[t]) if x is not None else 0
    ilen = int(x["internal_alignmentlength"]) if x is not None else 0
    pairs = int(x["matches"]) + int(x["mismatches"]) if x is not None else 0
    if f == "query":
        return qlabels[q]
    if f == "target":
        return tlabels[t] if x is not None else "*"
    if f == "evalue":
        return "-1"
    if f in ("id", "id0", "id1", "id2", "id3", "id4"):
        return "%.1f" % (x[f] if x is not None else 0.0)
    if f == "pctpv":
        return "%.1f" % (100.0 * int(x["matches"]) / ilen if ilen > 0 else 0.0)
    if f == "pctgaps":
        return "%.1f" % (100.0 * int(x["internal_indels"]) / ilen if ilen > 0 else 0.0)
    if f == "pairs":
        return "%d" % pairs
    if f == "gaps":
        return "%d" % (x["internal_indels"] if x is not None else 0)
    if f == "qlo":
        return "%d" % ((qlen if x["strand"] else 1) if x is not None else 0)
    if f == "qhi":
        return "%d" % ((1 if x["strand"] else qlen) if x is not None else 0)
    if f == "tlo":
        return "1" if x is not None else "0"
    if f in ("thi", "tl", "ts"):
        return "%d" % tlen
    if f in ("ql", "qs"):
        return "%d" % qlen
    if f in ("pv", "ids"):
        return "%d" % (x["matches"] if x is not None else 0)
    if f == "alnlen":
        return "%d" % ilen
    if f == "opens":
        return "%d" % (x["internal_gaps"] if x is not None else 0)
    if f == "exts":
        return "%d" % (int(x["internal_indels"]) - int(x["internal_gaps"]) if x is not None else 0)
    if f == "raw":
        return "%d" % (x["nwscore"] if x is not None else 0)
    if f == "bits":
        return "0"
    if f == "aln":
        return "".join(op * n for n, op in _runs(text.cigar(h))) if x is not None else ""
    if f == "caln":
        return text.cigar(h) if x is not None else ""
    if f == "qstrand":
        return ("-" if x["strand"] else "+") if x is not None else ""
    if f == "tstrand":
        return "+" if x is not None else ""
    if f == "qrow":
        return text.qrow(h) if x is not None else ""
    if f == "trow":
        return text.trow(h) if x is not None else ""
    if f in ("qframe", "tframe"):
        return "+0"
    if f == "mism":
        return "%d" % (x["mismatches"] if x is not None else 0)
    if f == "qcov":
        return "%.1f" % (100.0 * pairs / float(qlen) if x is not None else 0.0)
    if f == "tcov":
        return "%.1f" % (100.0 * pairs / float(tlen) if x is not None else 0.0)
    if f == "qilo":
        return "%d" % (int(x["trim_q_left"]) + 1 if x is not None else 0)
    if f == "qihi":
        return "%d" % (qlen - int(x["trim_q_right"]) if x is not None else 0)
    if f == "tilo":
        return "%d" % (int(x["trim_t_left"]) + 1 if x is not None else 0)
    if f == "tihi":
        return "%d" % (tlen - int(x["trim_t_right"]) if x is not None else 0)
    raise ValueError(f"unknown userfield {f}")


def userout_lines(text, qlabels, tlabels, fields=USERFIELDS, maxhits=0, top_hits_only=False, output_no_hits=False):
    """--userout with any of the 43 fields of utils/userfields.cpp, in any order"""
    lines = []
    for q, h in _per_hit(text, maxhits, top_hits_only):
        if h is None and not output_no_hits:
            continue
        lines.append("\t".join(_userfield(text, f, q, h, qlabels, tlabels) for f in fields))
    return lines
