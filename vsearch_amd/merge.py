"""Paired-end read merging (the reference's --fastq_mergepairs core) over vsx_merge_pairs (include/vsx_merge.h).

merge_pairs() takes the reads as they stand in the two FASTQ files (the reverse read NOT reverse-complemented) and returns
a MergeResult with the per-pair records and formatters that reproduce the reference CLI's text: --fastqout (with or
without --fastq_eeout) and --eetabbedout.  FASTQ parsing and writing and the command's file-level statistics stay with
the caller.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import MergeOpts, MergeOut, MergeRecord, MergeStats, check

# VSX_MERGE_* (include/vsx_merge.h), by value
MERGE_REASONS = ["ok", "minlen", "maxlen", "maxns", "minovlen", "maxdiffs", "maxdiffpct", "staggered", "repeat",
                 "minmergelen", "maxmergelen", "maxee", "minscore", "nokmers"]

RECORD_DTYPE = np.dtype([(n, np.dtype(t)) for n, t in MergeRecord._fields_])


def _blob(items):
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in items]
    lens = np.array([len(b) for b in bs], np.uint32)
    off = np.zeros(len(bs), np.uint64)
    if len(bs) > 1:
        off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return b"".join(bs), off, lens


def default_opts(**kw):
    """vsx_merge_opts with the reference's defaults; keywords are the field names without the fastq_ prefix
    (minovlen=5, maxee=1.0, ...) plus window."""
    o = MergeOpts()
    _lib.load().vsx_merge_opts_default(C.byref(o))
    names = {n for n, _ in MergeOpts._fields_}
    for k, v in kw.items():
        f = k if k in names else "fastq_" + k
        if f not in names or f == "pad":
            raise TypeError(f"merge_pairs: unknown option {k!r}")
        setattr(o, f, v)
    return o


def format_ee(ee):
    """fastq_print_general's variable-precision expected-error format (also --eetabbedout's)"""
    digits = 4
    for d, bound in ((13, 1e-9), (12, 1e-8), (11, 1e-7), (10, 1e-6), (9, 1e-5), (8, 1e-4), (7, 1e-3), (6, 1e-2), (5, 1e-1)):
        if ee < bound:
            digits = d
            break
    return "%.*f" % (digits, ee)


class MergeResult:
    """Per-pair records (numpy structured array `records`: merged, reason, fwd_trunc, rev_trunc, merged_length,
    overlap_length, fwd_errors, rev_errors, ee_merged, ee_fwd, ee_rev, blob_off) + the merged reads."""

    def __init__(self, records, seq_blob, qual_blob, stats):
        self.records = records
        self.seq_blob = seq_blob
        self.qual_blob = qual_blob
        self.stats = stats

    def __len__(self):
        return len(self.records)

    def __getattr__(self, name):
        if name != "records" and name in RECORD_DTYPE.names:
            return self.records[name]
        raise AttributeError(name)

    def sequence(self, k):
        r = self.records[k]
        return self.seq_blob[int(r["blob_off"]):int(r["blob_off"]) + int(r["merged_length"])].decode() if r["merged"] else None

    def quality(self, k):
        r = self.records[k]
        return self.qual_blob[int(r["blob_off"]):int(r["blob_off"]) + int(r["merged_length"])].decode() if r["merged"] else None

    def merged_indices(self):
        return np.flatnonzero(self.records["merged"])

    def not_merged_indices(self):
        return np.flatnonzero(self.records["merged"] == 0)

    def fastq_lines(self, labels, eeout=False):
        """--fastqout: four lines per merged pair, the forward read's label (plus ;ee= with --fastq_eeout)"""
        out = []
        for k in self.merged_indices():
            label = labels[k]
            if eeout:
                label += ("" if label.endswith(";") else ";") + "ee=" + format_ee(float(self.records["ee_merged"][k]))
            out += ["@" + label, self.sequence(k), "+", self.quality(k)]
        return out

    def eetabbed_lines(self):
        """--eetabbedout: ee_fwd, ee_rev, fwd_errors, rev_errors per merged pair"""
        r = self.records
        return ["%s\t%s\t%d\t%d" % (format_ee(float(r["ee_fwd"][k])), format_ee(float(r["ee_rev"][k])),
                                    r["fwd_errors"][k], r["rev_errors"][k]) for k in self.merged_indices()]

    def reason_counts(self):
        """{reason name: pairs}, the not-merged reasons that occur (the statistics block of the reference's log)"""
        cnt = np.bincount(self.records["reason"][self.records["merged"] == 0], minlength=len(MERGE_REASONS))
        return {MERGE_REASONS[i]: int(c) for i, c in enumerate(cnt) if c}


def last_stats():
    s = MergeStats()
    _lib.load().vsx_merge_last_stats(C.byref(s))
    return {n: getattr(s, n) for n, _ in MergeStats._fields_}


def merge_pairs(aligner, fwd, fqual, rev, rqual, **opts):
    """Merge read pairs.  fwd / fqual / rev / rqual: sequences of str or bytes, one entry per pair, as read from the
    forward and the reverse FASTQ file.  aligner: an Aligner (its device runs the kernel), or None under VSX_MERGE=host.
    Options: default_opts().  An out-of-range quality raises VsxError (VSX_EINVAL) naming the value and the bound."""
    if not (len(fwd) == len(fqual) == len(rev) == len(rqual)):
        raise ValueError("merge_pairs: fwd, fqual, rev, rqual must have one entry per pair")
    lib = _lib.load()
    o = opts.pop("opts", None) or default_opts(**opts)
    fs, foff, flen = _blob(fwd)
    fq, foff2, flen2 = _blob(fqual)
    rs, roff, rlen = _blob(rev)
    rq, roff2, rlen2 = _blob(rqual)
    if not (np.array_equal(flen, flen2) and np.array_equal(rlen, rlen2)):
        raise ValueError("merge_pairs: a quality string differs in length from its sequence")
    out = MergeOut()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)       # noqa: E731
    raw = lambda b: C.cast(C.c_char_p(b), C.c_void_p)  # noqa: E731
    check(lib.vsx_merge_pairs(aligner.h if aligner is not None else None, C.byref(o), C.c_uint64(len(fwd)),
                              raw(fs), raw(fq), C.c_uint64(len(fs)), ptr(foff), ptr(flen),
                              raw(rs), raw(rq), C.c_uint64(len(rs)), ptr(roff), ptr(rlen), C.byref(out)), "vsx_merge_pairs")
    try:
        n = int(out.n)
        records = np.ctypeslib.as_array(C.cast(out.rec, C.POINTER(C.c_uint8)), shape=(n * RECORD_DTYPE.itemsize,)).view(RECORD_DTYPE).copy() \
            if n else np.zeros(0, RECORD_DTYPE)
        nb = int(out.blob_bytes)
        seq_blob = C.string_at(out.seq_blob, nb) if nb else b""
        qual_blob = C.string_at(out.qual_blob, nb) if nb else b""
    finally:
        lib.vsx_merge_out_free(C.byref(out))
    return MergeResult(records, seq_blob, qual_blob, last_stats())
