"""Restriction-site cutting (--cut) over include/vsx_cut.h.

    cut(aligner, seqs, pattern, ...)     cut on the aligner's device: matches per sequence, the two fragment lists, the uncut list, the
                                         reverse-complemented text
    cut_host(seqs, pattern, ...)         the library's host restatement: no device
    parse_pattern(pattern)               (pattern without its marks, cut_fwd, cut_rev), or ValueError with the reference's message
    fasta_lines / log_lines              --fastaout, --fastaout_rev, --fastaout_discarded, --fastaout_discarded_rev and the closing line

Sequences are taken as the reference's reader delivers them (case preserved, illegal bytes already stripped).
The package exports the function under the module's name: `vsearch_amd.cut` is cut(); reach the writers with
`from vsearch_amd.cut import fasta_lines, log_lines` or importlib.import_module("vsearch_amd.cut").
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import CutOpts, check
from .derep import _text
from .orient import _fasta, _header, _queries, _size

PATTERN_MESSAGES = (None, "No forward sequence cut site (^) found in pattern", "No reverse sequence cut site (_) found in pattern",
                    "Multiple cut sites not supported", "Empty cut pattern string", "Illegal character in cut pattern")
WHICH = ("fastaout", "fastaout_rev", "fastaout_discarded", "fastaout_discarded_rev")


def last_stats():
    st = _lib.CutStats()
    _lib.load().vsx_cut_last_stats(C.byref(st))
    return {k: getattr(st, k) for k, _ in _lib.CutStats._fields_}


def parse_pattern(pattern):
    """-> (the pattern without '^' and '_', cut_fwd, cut_rev); ValueError with the reference's fatal message for a pattern it refuses"""
    raw = pattern.encode("latin-1") if isinstance(pattern, str) else bytes(pattern)
    stripped = C.create_string_buffer(max(len(raw), 1))
    plen, fwd, rev = C.c_uint64(0), C.c_int32(0), C.c_int32(0)
    cause = _lib.load().vsx_cut_pattern_check(raw, len(raw), stripped, C.byref(plen), C.byref(fwd), C.byref(rev))
    if cause != 0:
        raise ValueError(PATTERN_MESSAGES[cause])
    return stripped.raw[:plen.value].decode("latin-1"), int(fwd.value), int(rev.value)


def _records(ptr, count):
    """count records of (uint64 seq, uint32 start, uint32 length) -> (seq, start, length) arrays, or None for a NULL list"""
    if not ptr:
        return None
    raw = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint32)), shape=(max(count, 1), 4))[:count].copy()
    seq = raw[:, 0].astype(np.uint64) | (raw[:, 1].astype(np.uint64) << np.uint64(32))
    return seq, raw[:, 2].copy(), raw[:, 3].copy()


def _array(ptr, count, ctype, dtype):
    if not ptr:
        return None
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(max(count, 1),))[:count].astype(dtype)


class CutResult:
    """matches = matches per sequence; fwd / rev = (seq, start, length) arrays of the forward / reverse fragments in output order, in
    forward coordinates, ordinal = index + 1 (None when not wanted); n_fwd / n_rev = their counts, wanted or not; uncut = the numbers of
    the sequences without a match; text_blob = the reverse-complemented pieces, rev_off / discarded_off = the offsets of the reverse
    fragments / of the uncut sequences into it (None without their bit); cut / uncut_total / total_matches = the command's totals;
    stats = the call's vsx_cut_stats"""

    def __init__(self, res):
        self.n = int(res.n)
        self.n_fwd, self.n_rev, self.n_uncut = int(res.n_fwd), int(res.n_rev), int(res.n_uncut)
        self.cut, self.uncut_total, self.total_matches = int(res.cut), int(res.uncut_total), int(res.total_matches)
        self.matches = _array(res.matches, self.n, C.c_uint32, np.uint32)
        self.fwd = _records(res.fwd, self.n_fwd)
        self.rev = _records(res.rev, self.n_rev)
        self.uncut = _array(res.uncut, self.n_uncut, C.c_uint64, np.uint64)
        self.rev_off = _array(res.rev_off, self.n_rev + 1, C.c_uint64, np.uint64)
        self.discarded_off = _array(res.discarded_off, self.n_uncut + 1, C.c_uint64, np.uint64)
        nbytes = int(res.text_bytes)
        self.text_blob = (C.string_at(res.text, nbytes) if nbytes else b"") if res.text else None
        self.stats = last_stats()

    def fields(self):
        """everything two results must share to be the same answer"""
        out = dict(matches=self.matches, uncut=self.uncut,
                   totals=np.array([self.cut, self.uncut_total, self.total_matches, self.n_fwd, self.n_rev, self.n_uncut], np.uint64))
        for name, rec in (("fwd", self.fwd), ("rev", self.rev)):
            if rec is not None:
                out[name + "_seq"], out[name + "_start"], out[name + "_length"] = rec
        for name in ("rev_off", "discarded_off"):
            if getattr(self, name) is not None:
                out[name] = getattr(self, name)
        return out

    def tobytes(self):
        b = b"".join(k.encode() + np.ascontiguousarray(v).tobytes() for k, v in sorted(self.fields().items()))
        return b if self.text_blob is None else b + b"\0" + self.text_blob

    def rev_text(self, k):
        """the text of reverse fragment k"""
        if self.rev_off is None:
            raise ValueError("no reverse text: the call did not ask for it")
        return self.text_blob[int(self.rev_off[k]):int(self.rev_off[k + 1])]

    def discarded_rev_text(self, k):
        """uncut sequence k of the uncut list, reverse-complemented"""
        if self.discarded_off is None:
            raise ValueError("no discarded reverse text: the call did not ask for it")
        return self.text_blob[int(self.discarded_off[k]):int(self.discarded_off[k + 1])]


def _opts(pattern, want_fwd, want_rev, want_rev_text, want_discarded_rev_text, window, threads):
    raw = pattern.encode("latin-1") if isinstance(pattern, str) else bytes(pattern)
    o = CutOpts()
    _lib.load().vsx_cut_opts_default(C.byref(o))
    o.pattern, o.pattern_len = raw, len(raw)
    o.want = ((_lib.CUT_WANT_FWD if want_fwd else 0) | (_lib.CUT_WANT_REV if want_rev else 0) | (_lib.CUT_WANT_REV_TEXT if want_rev_text else 0)
              | (_lib.CUT_WANT_DISCARDED_REV_TEXT if want_discarded_rev_text else 0))
    o.window, o.threads = int(window), int(threads)
    return o


def _call(handle, seqs, pattern, o):
    parse_pattern(pattern)                                   # the reference's message for a pattern it refuses
    lib = _lib.load()
    blob, off, lens, _ = _queries(seqs, None)
    res = _lib.CutOut()
    check(lib.vsx_cut(handle, C.byref(o), len(lens), C.cast(C.c_char_p(blob), C.c_void_p), len(blob), off.ctypes.data_as(C.c_void_p),
                      lens.ctypes.data_as(C.c_void_p), C.byref(res)), "vsx_cut")
    try:
        return CutResult(res)
    finally:
        lib.vsx_cut_out_free(C.byref(res))


def cut(aligner, seqs, pattern, want_fwd=True, want_rev=True, want_rev_text=True, want_discarded_rev_text=True, window=0, threads=0):
    """Cut `seqs` (a list, or (blob, offsets, lengths)) at `pattern` (e.g. "G^AATT_C") on the aligner's device (vsx_cut)."""
    return _call(aligner.h, seqs, pattern, _opts(pattern, want_fwd, want_rev, want_rev_text, want_discarded_rev_text, window, threads))


def cut_host(seqs, pattern, want_fwd=True, want_rev=True, want_rev_text=True, want_discarded_rev_text=True, window=0, threads=0):
    """The host restatement: the same call without a context -- what the device is compared to, and its host route."""
    old = os.environ.get("VSX_CUT")
    os.environ["VSX_CUT"] = "host"
    try:
        return _call(None, seqs, pattern, _opts(pattern, want_fwd, want_rev, want_rev_text, want_discarded_rev_text, window, threads))
    finally:
        if old is None:
            del os.environ["VSX_CUT"]
        else:
            os.environ["VSX_CUT"] = old


# ---- the writers ---------------------------------------------------------------------------------------------------------------
def fasta_lines(result, labels, seqs, which, sizes=None, sizeout=False, xsize=False, relabel=None, fasta_width=80):
    """one of --cut's four files: `fastaout` (forward fragments), `fastaout_rev` (reverse fragments, reverse-complemented),
    `fastaout_discarded` (the uncut sequences), `fastaout_discarded_rev` (the same, reverse-complemented); each numbered on its own"""
    if which not in WHICH:
        raise ValueError(f"which must be one of {WHICH}")
    out = []

    def put(k, ordinal, text):
        out.extend(_fasta(_header(_text(labels[k]), _size(sizes, k), ordinal, sizeout, relabel, xsize), _text(text), fasta_width))

    if which == "fastaout":
        if result.fwd is None:
            raise ValueError("no forward fragments: the call did not ask for them")
        for x, (k, start, length) in enumerate(zip(*result.fwd)):
            put(int(k), x + 1, seqs[int(k)][int(start):int(start) + int(length)])
    elif which == "fastaout_rev":
        if result.rev is None:
            raise ValueError("no reverse fragments: the call did not ask for them")
        for x, k in enumerate(result.rev[0]):
            put(int(k), x + 1, result.rev_text(x))
    elif which == "fastaout_discarded":
        for x, k in enumerate(result.uncut):
            put(int(k), x + 1, seqs[int(k)])
    else:
        for x, k in enumerate(result.uncut):
            put(int(k), x + 1, result.discarded_rev_text(x))
    return out


def log_lines(result):
    """the closing line of --cut"""
    return ["%d sequence(s) cut %d times, %d sequence(s) never cut." % (result.cut, result.total_matches, result.uncut_total)]
