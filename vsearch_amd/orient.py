"""Sequence orientation (--orient) over include/vsx_orient.h.

    orient_session(aligner, db, ...)                  a SearchSession with this command's default word length (12)
    orient(session, seqs, quals=None, qmask="dust")   count the words of each read that speak for either strand; + / - / ?
    orient_host(db, seqs, ...)                        the library's host restatement: no device, no session
    tabbed_lines / fasta_lines / fastq_lines / notmatched_lines / log_lines    the reference CLI's text

The query is taken as given: the reference neither DUST-masks nor hard-masks the reads of this command, so qmask "dust" (its
default) and "soft" both only leave out the words over lower-case symbols.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import OrientOpts, SearchOpts, check
from .derep import _text, strip_size
from .search import SearchSession, _blob

QMASK = {"none": 0, "soft": 1, "dust": 2}
STRANDS = "+-?"
DEFAULT_WORDLENGTH = 12


def orient_session(aligner, db, sizes=None, labels=None, wordlength=DEFAULT_WORDLENGTH, **opts):
    """the database of an orient run: soft_mask 0 none / 1 soft / 2 dust (--dbmask), hardmask 1 (--hardmask)"""
    opts.setdefault("id", 0.97)                       # (the searcher wants one; this command aligns nothing)
    return SearchSession(aligner, db, sizes=sizes, labels=labels, wordlength=wordlength, **opts)


def last_stats():
    st = _lib.OrientStats()
    _lib.load().vsx_orient_last_stats(C.byref(st))
    d = {k: getattr(st, k) for k, _ in _lib.OrientStats._fields_ if k != "queries_class"}
    d["queries_class"] = [int(x) for x in st.queries_class]
    return d


class OrientResult:
    """per read: count_fwd, count_rev, strand (0 +, 1 -, 2 ?); n_fwd / n_rev / n_none; with want_text, text[k] (and qual[k] when
    qualities were given) = the read as the command writes it: - reads reverse-complemented, their qualities reversed.
    stats = the call's vsx_orient_stats"""

    def __init__(self, res, off, lens, want_text, has_qual):
        n = int(res.n_queries)
        self.n = n
        self.n_fwd, self.n_rev, self.n_none = int(res.n_fwd), int(res.n_rev), int(res.n_none)
        rec = np.ctypeslib.as_array(C.cast(res.rec, C.POINTER(C.c_uint32)), shape=(max(n, 1), 3))[:n].copy()
        self.count_fwd = rec[:, 0].copy()
        self.count_rev = rec[:, 1].copy()
        self.strand = rec[:, 2].astype(np.int32)
        # the oriented text stays one blob at the caller's offsets; the per-read lists are cut on first use
        nbytes = int((off + lens).max()) if n else 0
        self._off, self._lens, self._cut = off, lens, {}
        self.text_blob = (C.string_at(res.text, nbytes) if nbytes else b"") if want_text else None
        self.qual_blob = (C.string_at(res.qual, nbytes) if nbytes else b"") if want_text and has_qual else None
        self.stats = last_stats()

    def _reads(self, name, blob):
        if blob is None:
            return None
        if name not in self._cut:
            self._cut[name] = [blob[int(o):int(o) + int(l)] for o, l in zip(self._off, self._lens)]
        return self._cut[name]

    @property
    def text(self):
        return self._reads("text", self.text_blob)

    @property
    def qual(self):
        return self._reads("qual", self.qual_blob)

    def fields(self):
        """everything two results must share to be the same answer"""
        return dict(count_fwd=self.count_fwd, count_rev=self.count_rev, strand=self.strand)

    def tobytes(self):
        b = b"".join(np.ascontiguousarray(v).tobytes() for _, v in sorted(self.fields().items()))
        for part in (self.text, self.qual):
            if part is not None:
                b += b"\0".join(part)
        return b

    def record(self, k):
        return dict(count_fwd=int(self.count_fwd[k]), count_rev=int(self.count_rev[k]), strand=STRANDS[int(self.strand[k])])


def _opts(qmask, want_text, window):
    o = OrientOpts()
    _lib.load().vsx_orient_opts_default(C.byref(o))
    o.qmask = QMASK[qmask] if isinstance(qmask, str) else int(qmask)
    o.want_text = int(bool(want_text))
    o.window = int(window)
    return o


def _queries(seqs, quals):
    """(blob, offsets, lengths, quality blob or None): a list of reads, or (blob, offsets, lengths) with the reads anywhere in the
    blob (quals then is a blob with the qualities at the same offsets)"""
    if isinstance(seqs, tuple):
        blob, off, lens = bytes(seqs[0]), np.ascontiguousarray(seqs[1], np.uint64), np.ascontiguousarray(seqs[2], np.uint32)
        qblob = None if quals is None else bytes(quals)
    else:
        blob, off, lens = _blob(seqs)
        qblob = None
        if quals is not None:
            qblob, _, qlens = _blob(quals)
            if len(qlens) != len(lens) or np.any(qlens != lens):
                raise ValueError("quals: one quality string per read, as long as the read")
    if qblob is not None and len(qblob) != len(blob):
        raise ValueError("quals: the quality blob must be as long as the sequence blob")
    return blob, off, lens, qblob


def orient(session, seqs, quals=None, qmask="dust", want_text=True, window=0):
    """Orient `seqs` against the session's database (vsx_orient).  The first call builds the session's match-count table."""
    lib = _lib.load()
    blob, off, lens, qblob = _queries(seqs, quals)
    o = _opts(qmask, want_text, window)
    res = _lib.OrientResult()
    check(lib.vsx_orient(session.h, C.byref(o), len(lens), C.cast(C.c_char_p(blob), C.c_void_p), len(blob), off.ctypes.data_as(C.c_void_p),
                         lens.ctypes.data_as(C.c_void_p), None if qblob is None else C.cast(C.c_char_p(qblob), C.c_void_p), C.byref(res)),
          "vsx_orient")
    try:
        return OrientResult(res, off, lens, want_text, qblob is not None)
    finally:
        lib.vsx_orient_result_free(C.byref(res))


def orient_host(db, seqs, quals=None, qmask="dust", want_text=True, wordlength=DEFAULT_WORDLENGTH, soft_mask=2, hardmask=0, threads=0):
    """The host restatement (vsx_internal_orient_host) on a database given as text: what the device path is compared to, and its
    host route.  soft_mask: 0 none, 1 soft, 2 dust (--dbmask; the default of the reference is dust)."""
    lib = _lib.load()
    so = SearchOpts()
    lib.vsx_search_opts_default(C.byref(so))
    so.wordlength, so.soft_mask, so.hardmask, so.threads = int(wordlength), int(soft_mask), int(hardmask), int(threads)
    dblob, doff, dlens = _blob(db)
    blob, off, lens, qblob = _queries(seqs, quals)
    o = _opts(qmask, want_text, 0)
    res = _lib.OrientResult()
    check(lib.vsx_internal_orient_host(C.byref(so), C.byref(o), len(dlens), C.cast(C.c_char_p(dblob), C.c_void_p), len(dblob),
                                       doff.ctypes.data_as(C.c_void_p), dlens.ctypes.data_as(C.c_void_p), len(lens),
                                       C.cast(C.c_char_p(blob), C.c_void_p), len(blob), off.ctypes.data_as(C.c_void_p),
                                       lens.ctypes.data_as(C.c_void_p), None if qblob is None else C.cast(C.c_char_p(qblob), C.c_void_p),
                                       C.byref(res)), "vsx_internal_orient_host")
    try:
        return OrientResult(res, off, lens, want_text, qblob is not None)
    finally:
        lib.vsx_orient_result_free(C.byref(res))


def matchcounts(session, words):
    """the device table's entries for `words` (vsx_internal_orient_matchcounts; builds the table if no call has)"""
    w = np.ascontiguousarray(words, np.uint32)
    out = np.zeros(max(len(w), 1), np.uint32)
    check(_lib.load().vsx_internal_orient_matchcounts(session.h, w.ctypes.data_as(C.c_void_p), len(w), out.ctypes.data_as(C.c_void_p)),
          "vsx_internal_orient_matchcounts")
    return out[:len(w)]


# ---- the writers ---------------------------------------------------------------------------------------------------------------
def _header(label, size, ordinal, sizeout, relabel, xsize):
    if relabel is not None and ordinal > 0:
        head, trailing = f"{relabel}{ordinal}", False
    elif xsize or sizeout:
        head, trailing = strip_size(label)
    else:
        head, trailing = label, False
    if sizeout:
        head += ("" if trailing else ";") + f"size={int(size)}"
    return head


def _fasta(head, seq, fasta_width):
    if fasta_width < 1:
        return [">" + head, seq]
    return [">" + head] + [seq[i:i + fasta_width] for i in range(0, len(seq), fasta_width)]


def _selected(result, strands):
    """(read, ordinal) of the reads whose verdict is in `strands`, in input order, numbered from 1"""
    ordinal = 0
    for k in range(result.n):
        if int(result.strand[k]) in strands:
            ordinal += 1
            yield k, ordinal


def _size(sizes, k):
    return 1 if sizes is None else int(sizes[k])


def tabbed_lines(result, labels):
    """--tabbedout: label, + | - | ?, count_fwd, count_rev"""
    return [f"{_text(labels[k])}\t{STRANDS[int(result.strand[k])]}\t{int(result.count_fwd[k])}\t{int(result.count_rev[k])}"
            for k in range(result.n)]


def fasta_lines(result, labels, sizes=None, sizeout=False, xsize=False, relabel=None, fasta_width=80):
    """--fastaout: the oriented reads (+ as given, - reverse-complemented), numbered over both"""
    out = []
    for k, ordinal in _selected(result, (0, 1)):
        out += _fasta(_header(_text(labels[k]), _size(sizes, k), ordinal, sizeout, relabel, xsize), _text(result.text[k]), fasta_width)
    return out


def fastq_lines(result, labels, sizes=None, sizeout=False, xsize=False, relabel=None, fasta_width=80):
    """--fastqout: the oriented reads with their qualities (reversed for - reads); fasta_width does not apply"""
    if result.qual is None:
        raise ValueError("no qualities: the input was FASTA")
    out = []
    for k, ordinal in _selected(result, (0, 1)):
        out += ["@" + _header(_text(labels[k]), _size(sizes, k), ordinal, sizeout, relabel, xsize), _text(result.text[k]), "+",
                _text(result.qual[k])]
    return out


def notmatched_lines(result, labels, sizes=None, sizeout=False, xsize=False, relabel=None, fasta_width=80):
    """--notmatched: the ? reads as given, numbered on their own; FASTQ if the input was FASTQ, else FASTA"""
    out = []
    for k, ordinal in _selected(result, (2,)):
        head = _header(_text(labels[k]), _size(sizes, k), ordinal, sizeout, relabel, xsize)
        if result.qual is not None:
            out += ["@" + head, _text(result.text[k]), "+", _text(result.qual[k])]
        else:
            out += _fasta(head, _text(result.text[k]), fasta_width)
    return out


def log_lines(result):
    """the five closing lines of the reference's log; the percentages are left out when there are no reads"""
    def line(name, count):
        return name + str(count) + (" (%.2f%%)" % (100.0 * count / result.n) if result.n > 0 else "")
    return [line("Forward oriented sequences: ", result.n_fwd), line("Reverse oriented sequences: ", result.n_rev),
            line("All oriented sequences:     ", result.n_fwd + result.n_rev), line("Not oriented sequences:     ", result.n_none),
            "Total number of sequences:  %d" % result.n]
