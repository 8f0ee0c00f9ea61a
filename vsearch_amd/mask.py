"""Sequence masking (--fastx_mask, --maskfasta) over include/vsx_mask.h.

    fastx_mask(aligner, seqs, quals=None, qmask="dust", hardmask=False, ...)   mask on the device: text, bitmap, unmasked counts, verdicts
    fastx_mask_host(seqs, ...)                                                  the library's host restatement: no device
    fasta_lines / fastq_lines / log_lines                                       --fastx_mask's --fastaout, --fastqout and closing log lines
    maskfasta_lines                                                             --maskfasta's --output

Sequences are taken as the reference's reader delivers them (case preserved).  The qualities only travel through to fastq_lines.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import MaskOpts, check
from .derep import _text
from .orient import _fasta, _header, _queries, _size

QMASK = {"none": 0, "soft": 1, "dust": 2}
VERDICTS = ("kept", "discarded_less", "discarded_more")


def last_stats():
    st = _lib.MaskStats()
    _lib.load().vsx_fastx_mask_last_stats(C.byref(st))
    return {k: getattr(st, k) for k, _ in _lib.MaskStats._fields_}


class MaskResult:
    """per sequence: unmasked, verdict (0 kept, 1 discarded for less than min_unmasked_pct, 2 for more than max_unmasked_pct); kept /
    discarded_less / discarded_more; text_blob = the masked text packed at the input's lengths (None without want_text); bits_blob = the
    bitmap over it, bit i % 8 of byte i // 8 set where packed symbol i does not count as unmasked (None without want_bits);
    stats = the call's vsx_fastx_mask_stats"""

    def __init__(self, res, lens, quals, want_text, want_bits):
        n = int(res.n)
        self.n = n
        self.kept, self.discarded_less, self.discarded_more = int(res.kept), int(res.discarded_less), int(res.discarded_more)
        rec = np.ctypeslib.as_array(C.cast(res.rec, C.POINTER(C.c_uint32)), shape=(max(n, 1), 2))[:n].copy()
        self.unmasked = rec[:, 0].copy()
        self.verdict = rec[:, 1].astype(np.int32)
        self.lengths = np.asarray(lens, np.uint32).copy()
        self.offsets = np.zeros(n + 1, np.uint64)
        np.cumsum(self.lengths, dtype=np.uint64, out=self.offsets[1:])
        nbytes = int(res.text_bytes)
        self.text_blob = (C.string_at(res.text, nbytes) if nbytes else b"") if want_text else None
        self.bits_blob = (C.string_at(res.bits, (nbytes + 7) // 8) if nbytes else b"") if want_bits else None
        self.quals = quals
        self.stats = last_stats()
        self._cut = None

    def text(self):
        """the masked sequences, one bytes object each (None without want_text)"""
        if self.text_blob is None:
            return None
        if self._cut is None:
            o = self.offsets
            self._cut = [self.text_blob[int(o[k]):int(o[k + 1])] for k in range(self.n)]
        return self._cut

    def bits(self):
        """the bitmap as one bool per packed symbol (None without want_bits)"""
        if self.bits_blob is None:
            return None
        return np.unpackbits(np.frombuffer(self.bits_blob, np.uint8), bitorder="little")[:int(self.offsets[-1])].astype(bool)

    def fields(self):
        """everything two results must share to be the same answer"""
        return dict(unmasked=self.unmasked, verdict=self.verdict, lengths=self.lengths,
                    totals=np.array([self.kept, self.discarded_less, self.discarded_more], np.uint64))

    def tobytes(self):
        b = b"".join(np.ascontiguousarray(v).tobytes() for _, v in sorted(self.fields().items()))
        for part in (self.text_blob, self.bits_blob):
            if part is not None:
                b += b"\0" + part
        return b

    def record(self, k):
        return dict(unmasked=int(self.unmasked[k]), length=int(self.lengths[k]), verdict=VERDICTS[int(self.verdict[k])])


def _opts(qmask, hardmask, min_unmasked_pct, max_unmasked_pct, want_text, want_bits, window):
    o = MaskOpts()
    _lib.load().vsx_fastx_mask_opts_default(C.byref(o))
    o.qmask = QMASK[qmask] if isinstance(qmask, str) else int(qmask)
    o.hardmask = int(hardmask)
    o.min_unmasked_pct, o.max_unmasked_pct = float(min_unmasked_pct), float(max_unmasked_pct)
    o.want = (_lib.MASK_WANT_TEXT if want_text else 0) | (_lib.MASK_WANT_BITS if want_bits else 0)
    o.window = int(window)
    return o


def _call(handle, seqs, quals, o):
    lib = _lib.load()
    blob, off, lens, qblob = _queries(seqs, quals)
    if qblob is not None and not isinstance(seqs, tuple):
        quals = [q.encode() if isinstance(q, str) else bytes(q) for q in quals]
    elif qblob is not None:
        quals = [qblob[int(a):int(a) + int(l)] for a, l in zip(off, lens)]
    res = _lib.MaskOut()
    check(lib.vsx_fastx_mask(handle, C.byref(o), len(lens), C.cast(C.c_char_p(blob), C.c_void_p), len(blob), off.ctypes.data_as(C.c_void_p),
                             lens.ctypes.data_as(C.c_void_p), C.byref(res)), "vsx_fastx_mask")
    try:
        return MaskResult(res, lens, quals, bool(o.want & _lib.MASK_WANT_TEXT), bool(o.want & _lib.MASK_WANT_BITS))
    finally:
        lib.vsx_fastx_mask_out_free(C.byref(res))


def fastx_mask(aligner, seqs, quals=None, qmask="dust", hardmask=False, min_unmasked_pct=0.0, max_unmasked_pct=100.0, want_text=True,
               window=0, want_bits=True):
    """Mask `seqs` (a list, or (blob, offsets, lengths)) on the aligner's device (vsx_fastx_mask)."""
    return _call(aligner.h, seqs, quals, _opts(qmask, hardmask, min_unmasked_pct, max_unmasked_pct, want_text, want_bits, window))


def fastx_mask_host(seqs, quals=None, qmask="dust", hardmask=False, min_unmasked_pct=0.0, max_unmasked_pct=100.0, want_text=True,
                    window=0, want_bits=True):
    """The host restatement: the same call without a context under VSX_MASK=host -- what the device is compared to, and its host route."""
    old = os.environ.get("VSX_MASK")
    os.environ["VSX_MASK"] = "host"
    try:
        return _call(None, seqs, quals, _opts(qmask, hardmask, min_unmasked_pct, max_unmasked_pct, want_text, want_bits, window))
    finally:
        if old is None:
            del os.environ["VSX_MASK"]
        else:
            os.environ["VSX_MASK"] = old


# ---- the writers ---------------------------------------------------------------------------------------------------------------
def _kept(result):
    """(sequence, ordinal) of the kept sequences in input order: the ordinal is the running `kept` of the reference's loop"""
    ordinal = 0
    for k in range(result.n):
        if int(result.verdict[k]) == 0:
            ordinal += 1
            yield k, ordinal


def fasta_lines(result, labels, sizes=None, sizeout=False, xsize=False, relabel=None, fasta_width=80):
    """--fastx_mask --fastaout: the kept sequences, masked"""
    text, out = result.text(), []
    for k, ordinal in _kept(result):
        out += _fasta(_header(_text(labels[k]), _size(sizes, k), ordinal, sizeout, relabel, xsize), _text(text[k]), fasta_width)
    return out


def fastq_lines(result, labels, sizes=None, sizeout=False, xsize=False, relabel=None, fasta_width=80):
    """--fastx_mask --fastqout: the kept sequences, masked, with their qualities as given; fasta_width does not apply"""
    if result.quals is None:
        raise ValueError("no qualities: the input was FASTA")
    text, out = result.text(), []
    for k, ordinal in _kept(result):
        out += ["@" + _header(_text(labels[k]), _size(sizes, k), ordinal, sizeout, relabel, xsize), _text(text[k]), "+", _text(result.quals[k])]
    return out


def maskfasta_lines(result, labels, sizes=None, sizeout=False, xsize=False, relabel=None, fasta_width=80):
    """--maskfasta --output: EVERY sequence, masked, numbered i + 1 (the command does not read the percentage options)"""
    text, out = result.text(), []
    for k in range(result.n):
        out += _fasta(_header(_text(labels[k]), _size(sizes, k), k + 1, sizeout, relabel, xsize), _text(text[k]), fasta_width)
    return out


def log_lines(result, min_unmasked_pct=0.0, max_unmasked_pct=100.0):
    """the closing lines of --fastx_mask: the "less than" line only with a minimum, the "more than" line only with a maximum"""
    out = []
    if min_unmasked_pct > 0.0:
        out.append("%d sequences with less than %.1f%% unmasked residues discarded" % (result.discarded_less, min_unmasked_pct))
    if max_unmasked_pct < 100.0:
        out.append("%d sequences with more than %.1f%% unmasked residues discarded" % (result.discarded_more, max_unmasked_pct))
    out.append("%d sequences kept" % result.kept)
    return out
