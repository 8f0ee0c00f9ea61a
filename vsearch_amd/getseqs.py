"""Sequence extraction by label (--fastx_getseqs, --fastx_getseq, --fastx_getsubseq) over include/vsx_getseqs.h.

    getseqs(aligner, headers, seqs, mode, needles, substr=False, field=None, ...)   decide every header on the device
    getseq(aligner, headers, seqs, label, substr=False)                              --fastx_getseq: one label
    getsubseq(aligner, headers, seqs, label, subseq_start, subseq_end, substr=False) --fastx_getsubseq: one label, a piece of the matched
    getseqs_host(headers, seqs, mode, needles, ...)                                  the library's host restatement: no device
    read_labels(path)                                                                the reference's reader of --labels / --label_words
    fasta_lines / fastq_lines / log_lines                                            --fastaout / --notmatched, --fastqout / --notmatchedfq, the log

A header is what the reference's parser hands on: cut at the first blank unless --notrunclabels.  FASTA / FASTQ parsing stays with
the caller; nothing is copied: the writers cut the caller's sequences and qualities with the record's (start, length).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import GetseqsOpts, GetseqsOut, GetseqsStats, check
from .derep import _text
from .orient import _fasta, _header, _size
from .otutab import LabelBlob, _bytes

LABEL, LABELS, WORD, WORDS = 0, 1, 2, 3
MODES = {"label": LABEL, "labels": LABELS, "label_word": WORD, "word": WORD, "label_words": WORDS, "words": WORDS}
LINE_PIECE = 1023          # what the reference's fgets buffer of 1024 bytes holds


def last_stats():
    s = GetseqsStats()
    _lib.load().vsx_getseqs_last_stats(C.byref(s))
    return {n: getattr(s, n) for n, _ in GetseqsStats._fields_}


class GetseqsResult:
    """per sequence in input order: matched (0 / 1), ordinal (1-based among the sequences of the same verdict), start and length of
    the piece to print; kept / discarded; stats = the call's vsx_getseqs_stats"""

    def __init__(self, out):
        n = int(out.n)
        self.n = n
        if n:
            rec = np.ctypeslib.as_array(C.cast(out.rec, C.POINTER(C.c_uint32)), shape=(n, 4)).copy()
        else:
            rec = np.zeros((0, 4), np.uint32)
        self.matched, self.ordinal, self.start, self.length = (np.ascontiguousarray(rec[:, k]) for k in range(4))
        self.kept, self.discarded = int(out.kept), int(out.discarded)
        self.stats = last_stats()

    def arrays(self):
        """everything two routes must agree on"""
        return (self.matched.tobytes(), self.ordinal.tobytes(), self.start.tobytes(), self.length.tobytes(), self.kept, self.discarded)

    def record(self, k):
        return (int(self.matched[k]), int(self.ordinal[k]), int(self.start[k]), int(self.length[k]))


def _lengths(seqs, n):
    if isinstance(seqs, np.ndarray):
        lens = np.ascontiguousarray(seqs, np.uint32)
    else:
        lens = np.array([s if isinstance(s, (int, np.integer)) else len(s) for s in seqs], np.uint32)
    if len(lens) != n:
        raise ValueError("getseqs: one sequence (or sequence length) per header")
    return lens


def getseqs(aligner, headers, seqs, mode, needles, substr=False, field=None, subseq_start=0, subseq_end=0, window=0, threads=0):
    """Decide every header.  headers: a list of str / bytes or a LabelBlob.  seqs: the sequences (only their lengths are read) or
    an array of lengths.  mode: "label", "labels", "label_word", "label_words" (or the VSX_GETSEQS_* number).  needles: one str /
    bytes for the single-needle modes, a list or a LabelBlob for the list modes.  field: --label_field (word modes), None without.
    aligner: an Aligner (its device runs the kernels), or None for the host restatement.  What the library refuses raises
    VsxError (VSX_EINVAL)."""
    lib = _lib.load()
    H = headers if isinstance(headers, LabelBlob) else LabelBlob(headers)
    if isinstance(needles, (str, bytes, bytearray)):
        needles = [needles]
    N = needles if isinstance(needles, LabelBlob) else LabelBlob(needles)
    lens = _lengths(seqs, len(H))
    o = GetseqsOpts()
    lib.vsx_getseqs_opts_default(C.byref(o))
    o.mode = MODES[mode] if isinstance(mode, str) else int(mode)
    o.substr = int(substr)
    fb = None if field is None else _bytes(field)
    if fb is not None:
        o.field = C.cast(C.c_char_p(fb), C.c_void_p)
        o.field_len = len(fb)
    o.subseq_start, o.subseq_end = int(subseq_start), int(subseq_end)
    o.window, o.threads = int(window), int(threads)
    hs, ns = H.struct(), N.struct()
    out = GetseqsOut()
    check(lib.vsx_getseqs(aligner.h if aligner is not None else None, C.byref(o), C.byref(hs), lens.ctypes.data if len(lens) else None,
                          C.byref(ns), C.byref(out)), "vsx_getseqs")
    try:
        return GetseqsResult(out)
    finally:
        lib.vsx_getseqs_out_free(C.byref(out))


def getseqs_host(headers, seqs, mode, needles, **kw):
    """getseqs() without a context: the library's host restatement, the same hashed rule on `threads` host threads"""
    return getseqs(None, headers, seqs, mode, needles, **kw)


def getseq(aligner, headers, seqs, label, substr=False, **kw):
    """--fastx_getseq: the sequences whose header equals (or, with substr, contains) `label`, case folded"""
    return getseqs(aligner, headers, seqs, LABEL, label, substr=substr, **kw)


def getsubseq(aligner, headers, seqs, label, subseq_start, subseq_end, substr=False, **kw):
    """--fastx_getsubseq: as getseq(), and of a matched sequence only [subseq_start, subseq_end] (1-based, inclusive)"""
    return getseqs(aligner, headers, seqs, LABEL, label, substr=substr, subseq_start=subseq_start, subseq_end=subseq_end, **kw)


def read_labels(path):
    """The reference's reader of --labels / --label_words -> (labels as bytes, warn).  It reads pieces of at most 1 023 bytes, so a
    longer line becomes several labels; a piece ends at a NUL byte (strlen); one trailing newline is dropped, a carriage return
    kept; empty pieces are skipped.  warn: the "Labels longer than 1023 characters are not supported" warning applies, which is
    when the longest piece has 1 023 bytes."""
    with open(path, "rb") as f:
        data = f.read()
    labels, longest, at = [], 0, 0
    while at < len(data):
        nl = data.find(b"\n", at, at + LINE_PIECE)
        end = nl + 1 if nl >= 0 else min(at + LINE_PIECE, len(data))
        piece = data[at:end].split(b"\0")[0]
        at = end
        if piece.endswith(b"\n"):
            piece = piece[:-1]
        if not piece:
            continue
        longest = max(longest, len(piece))
        labels.append(piece)
    return labels, longest >= LINE_PIECE


# ---- the writers ---------------------------------------------------------------------------------------------------------------
def _side(result, matched):
    want = 1 if matched else 0
    for k in range(result.n):
        if int(result.matched[k]) == want:
            yield k, int(result.ordinal[k]), int(result.start[k]), int(result.length[k])


def fasta_lines(result, labels, seqs, matched=True, sizes=None, sizeout=False, xsize=False, relabel=None, fasta_width=80):
    """--fastaout (matched=True) or --notmatched (matched=False)"""
    out = []
    for k, ordinal, a, n in _side(result, matched):
        out += _fasta(_header(_text(labels[k]), _size(sizes, k), ordinal, sizeout, relabel, xsize), _text(seqs[k])[a:a + n], fasta_width)
    return out


def fastq_lines(result, labels, seqs, quals, matched=True, sizes=None, sizeout=False, xsize=False, relabel=None, fasta_width=80):
    """--fastqout (matched=True) or --notmatchedfq (matched=False): the qualities cut as the sequence; fasta_width does not apply"""
    if quals is None:
        raise ValueError("no qualities: the input was FASTA")
    out = []
    for k, ordinal, a, n in _side(result, matched):
        out += ["@" + _header(_text(labels[k]), _size(sizes, k), ordinal, sizeout, relabel, xsize), _text(seqs[k])[a:a + n], "+",
                _text(quals[k])[a:a + n]]
    return out


def log_lines(result):
    """the closing line of all three commands"""
    total = result.kept + result.discarded
    line = "%d of %d sequences extracted" % (result.kept, total)
    if total:
        line += " (%.1f%%)" % (100.0 * result.kept / total)
    return [line]
