"""Full-length dereplication (the reference's --derep_fulllength, --fastx_uniques and --derep_id) over vsx_derep
(include/vsx_derep.h).

dereplicate() takes the reads as they stand in the input file and returns a DerepResult: the clusters in the command's output
order (size descending, label, input index) with their members, strands and -- for FASTQ input -- the merged quality strings,
and formatters that reproduce the reference CLI's text: --output / --fastaout, --fastqout, --uc, --tabbedout and the log lines.
derep_fulllength(), fastx_uniques() and derep_id() are the three commands with the CLI's own defaults.  FASTA / FASTQ parsing,
--notrunclabels and the abundance annotations (--sizein) stay with the caller.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import DerepOpts, DerepOut, DerepStats, FilterReads, check
from .merge import _blob

INT64_MAX = (1 << 63) - 1


def default_opts(**kw):
    """vsx_derep_opts with the reference's defaults; keywords are the field names (strand_both=1, minseqlength=1, ...)"""
    o = DerepOpts()
    _lib.load().vsx_derep_opts_default(C.byref(o))
    names = {n for n, _ in DerepOpts._fields_}
    for k, v in kw.items():
        if k not in names:
            raise TypeError(f"dereplicate: unknown option {k!r}")
        setattr(o, k, v)
    return o


def last_stats():
    s = DerepStats()
    _lib.load().vsx_derep_last_stats(C.byref(s))
    return {n: getattr(s, n) for n, _ in DerepStats._fields_}


def thresholds():
    """T[v], v = 0 .. 128: the largest double p with trunc(-10 log10 p) >= v, as the quality kernel compares them"""
    t = (C.c_double * _lib.DEREP_THRESHOLDS)()
    _lib.load().vsx_internal_derep_thresholds(t)
    return list(t)


def _text(s):
    return s if isinstance(s, str) else bytes(s).decode("latin-1")


def _find_size(h):
    """the first (^|;)size=[0-9]+(;|$) of a header -> (start, end) or None"""
    off, n = 0, len(h)
    while off < n - 5:
        off = h.find("size=", off)
        if off < 0:
            break
        if off > 0 and h[off - 1] != ";":
            off += 6
            continue
        digits = 0
        while off + 5 + digits < n and h[off + 5 + digits] in "0123456789":
            digits += 1
        if digits == 0:
            off += 6
            continue
        if off + 5 + digits < n and h[off + 5 + digits] != ";":
            off += 5 + digits + 2
            continue
        return off, off + 5 + digits
    return None


def strip_size(h):
    """a header without its size annotation, as the reference prints it before a new one -> (text, ends with the separator)"""
    found = _find_size(h)
    if found is None:
        return h, h.endswith(";")
    start, end = found
    out, last = "", -1
    if start > 1:
        out, last = h[:start - 1], start - 2
    if len(h) > end + 1:
        out, last = out + h[end:], len(h) - 1
    return out, last >= 0 and h[last] == ";"


class DerepResult:
    """rep / size / count: one entry per cluster, output order.  members(c) / strands(c): the cluster's input indices (the
    representative first, then input order) and 0 '+' / 1 '-' per member.  quality(c): the merged quality string (FASTQ input).
    counts: the figures of the log lines."""

    def __init__(self, rep, size, count, member_start, member, strand, quals, counts, seqs, labels, opts, stats):
        self.rep, self.size, self.count = rep, size, count
        self.member_start, self.member, self.strand = member_start, member, strand
        self.quals = quals
        self.counts = counts
        self._seqs, self._labels = seqs, labels
        self.opts = opts
        self.stats = stats

    def __len__(self):
        return len(self.rep)

    def members(self, c):
        return self.member[self.member_start[c]:self.member_start[c + 1]]

    def strands(self, c):
        return self.strand[self.member_start[c]:self.member_start[c + 1]]

    def quality(self, c):
        if self.quals is None:
            raise ValueError("no merged qualities: the input was FASTA, or want_quality was off")
        return self.quals[c]

    def label(self, c):
        return _text(self._labels[int(self.rep[c])])

    def sequence(self, c):
        """the representative's own text: its case and its U are kept"""
        return _text(self._seqs[int(self.rep[c])])

    # ---- the writers: minuniquesize, maxuniquesize and topn apply to FASTA and FASTQ only ----------------------------------
    def _written(self):
        o, ordinal = self.opts, 0
        for c in range(len(self)):
            if o["minuniquesize"] <= int(self.size[c]) <= o["maxuniquesize"]:
                ordinal += 1
                yield c, ordinal
                if ordinal == o["topn"]:
                    break

    def _header(self, c, ordinal, sizeout, relabel, xsize):
        if relabel is not None and ordinal > 0:
            head, trailing = f"{relabel}{ordinal}", False
        elif xsize or sizeout:
            head, trailing = strip_size(self.label(c))
        else:
            head, trailing = self.label(c), False
        if sizeout:
            head += ("" if trailing else ";") + f"size={int(self.size[c])}"
        return head

    def fasta_lines(self, sizeout=False, relabel=None, xsize=False, fasta_width=80):
        """--output / --fastaout: the header, then the sequence folded at fasta_width (below 1: on one line)"""
        out = []
        for c, ordinal in self._written():
            seq = self.sequence(c)
            out.append(">" + self._header(c, ordinal, sizeout, relabel, xsize))
            if fasta_width < 1:
                out.append(seq)
            else:
                out += [seq[i:i + fasta_width] for i in range(0, len(seq), fasta_width)]
        return out

    def fastq_lines(self, sizeout=False, relabel=None, xsize=False):
        """--fastqout: four lines per unique sequence, the quality line merged over the members"""
        out = []
        for c, ordinal in self._written():
            out += ["@" + self._header(c, ordinal, sizeout, relabel, xsize), self.sequence(c), "+", self.quality(c)]
        return out

    def uc_lines(self):
        """--uc: per cluster its S record and an H record per further member, then the C records; every cluster is listed"""
        out = []
        for c in range(len(self)):
            head, length = self.label(c), len(self._seqs[int(self.rep[c])])
            out.append(f"S\t{c}\t{length}\t*\t*\t*\t*\t*\t{head}\t*")
            for m, s in zip(self.members(c)[1:], self.strands(c)[1:]):
                out.append(f"H\t{c}\t{length}\t100.0\t{'-' if s else '+'}\t0\t0\t*\t{_text(self._labels[int(m)])}\t{head}")
        for c in range(len(self)):
            out.append(f"C\t{c}\t{int(self.size[c])}\t*\t*\t*\t*\t*\t{self.label(c)}\t*")
        return out

    def tabbed_lines(self, relabel=None):
        """--tabbedout: a line per member -- its label, the cluster's (new) label, cluster number, member number, count, label"""
        out = []
        for c in range(len(self)):
            head = self.label(c)
            name = f"{relabel}{c + 1}" if relabel is not None else head
            for j, m in enumerate(self.members(c)):
                out.append(f"{_text(self._labels[int(m)])}\t{name}\t{c}\t{j}\t{int(self.count[c])}\t{head}")
        return out

    def log_lines(self):
        """the lines the command writes to its log"""
        k, o, out = self.counts, self.opts, []
        if k["kept"] > 0:
            out.append(f"{k['nucleotides']} nt in {k['kept']} seqs, min {k['shortest']}, max {k['longest']}, "
                       f"avg {k['nucleotides'] / k['kept']:.0f}")
        else:
            out.append(f"{k['nucleotides']} nt in {k['kept']} seqs")
        for name, n in (("minseqlength", k["discarded_short"]), ("maxseqlength", k["discarded_long"])):
            if n:
                out.append(f"{name} {o[name]}: {n} {'sequence' if n == 1 else 'sequences'} discarded.")
        clusters = len(self)
        if clusters < 1:
            out.append("0 unique sequences")
        else:
            out.append(f"{clusters} unique sequences, avg cluster {k['sumsize'] / clusters:.1f}, median {k['median']:.0f}, "
                       f"max {k['maxsize']}")
        if k["selected"] < clusters:
            gone = clusters - k["selected"]
            out.append(f"{k['selected']} uniques written, {gone} clusters discarded ({100.0 * gone / clusters:.1f}%)")
        return out


def dereplicate(aligner, seqs, labels, quals=None, sizes=None, **opts):
    """Dereplicate reads.  seqs / labels / quals: sequences of str or bytes, one entry per read; quals=None is FASTA input.
    sizes: abundances (--sizein; default 1 each).  aligner: an Aligner (its device runs the kernels), or None for the host
    restatement (as under VSX_DEREP=host).  Options: default_opts(); want_quality defaults to "the input has qualities".
    A value the library refuses raises VsxError (VSX_EINVAL)."""
    if len(labels) != len(seqs):
        raise ValueError("dereplicate: one label per read")
    lib = _lib.load()
    if quals is not None:
        opts.setdefault("want_quality", 1)
    o = opts.pop("opts", None) or default_opts(**opts)
    sb, off, lens = _blob(seqs)
    qb = None
    if quals is not None:
        qb, _, qlens = _blob(quals)
        if not np.array_equal(lens, qlens):
            raise ValueError("dereplicate: a quality string differs in length from its sequence")
    ab = None
    if sizes is not None:
        ab = np.ascontiguousarray(sizes, np.uint64)
        if len(ab) != len(seqs):
            raise ValueError("dereplicate: one abundance per read")
    raw = [l.encode("latin-1") if isinstance(l, str) else bytes(l) for l in labels]
    lb = b"".join(raw)
    loff = np.zeros(len(raw) + 1, np.uint64)
    if raw:
        np.cumsum([len(l) for l in raw], out=loff[1:])
    ptr = lambda b: C.cast(C.c_char_p(b), C.c_void_p)  # noqa: E731
    reads = FilterReads(ptr(sb), ptr(qb) if qb is not None else None, len(sb), off.ctypes.data, lens.ctypes.data,
                        ab.ctypes.data if ab is not None else None)
    out = DerepOut()
    n = len(seqs)
    check(lib.vsx_derep(aligner.h if aligner is not None else None, C.byref(o), C.c_uint64(n), C.byref(reads), ptr(lb), loff.ctypes.data,
                        C.byref(out)), "vsx_derep")
    try:
        nc, kept = int(out.n_clusters), int(out.kept)
        arr = lambda p, m, dt: np.ctypeslib.as_array(p, shape=(m,)).copy() if m else np.zeros(0, dt)  # noqa: E731
        rep, size, count = (arr(p, nc, np.uint64) for p in (out.rep, out.size, out.count))
        member_start = np.ctypeslib.as_array(out.member_start, shape=(nc + 1,)).copy()
        member, strand = arr(out.member, kept, np.uint64), arr(out.strand, kept, np.uint8)
        merged = None
        if o.want_quality:
            qoff = np.ctypeslib.as_array(out.qual_off, shape=(nc + 1,)).copy()
            blob = C.string_at(out.qual_blob, int(out.qual_bytes)).decode("latin-1")
            merged = [blob[int(qoff[c]):int(qoff[c + 1])] for c in range(nc)]
        counts = {k: int(getattr(out, k)) for k in ("kept", "nucleotides", "shortest", "longest", "discarded_short", "discarded_long",
                                                    "sumsize", "maxsize", "selected")}
        counts["median"] = float(out.median)
    finally:
        lib.vsx_derep_out_free(C.byref(out))
    used = {k: int(getattr(o, k)) for k in ("minseqlength", "maxseqlength", "minuniquesize", "maxuniquesize", "topn")}
    return DerepResult(rep, size, count, member_start, member, strand, merged, counts, seqs, labels, used, last_stats())


def _command(name, default_minseqlength, by_label, fastq_ok):
    def run(aligner, seqs, labels, quals=None, sizes=None, fastqout=False, tabbedout=False, **opts):
        if quals is not None and not fastq_ok:
            raise ValueError("FASTQ input is only allowed with the fastx_uniques command")
        if quals is None and fastqout:
            raise ValueError("Cannot write FASTQ output when input file is not in FASTQ format")
        if quals is None and tabbedout:
            raise ValueError("Cannot write tab separated output file when input file is not in FASTQ format")
        opts.setdefault("minseqlength", default_minseqlength)
        opts["by_label"] = by_label
        opts["want_quality"] = 1 if (quals is not None and fastqout) else 0
        return dereplicate(aligner, seqs, labels, quals=quals, sizes=sizes, **opts)
    run.__name__ = name
    run.__doc__ = (f"--{name} with the CLI's defaults (minseqlength {default_minseqlength}); fastqout / tabbedout name the outputs the "
                   "caller will write, and raise where the CLI is fatal.  Other keywords: default_opts().")
    return run


derep_fulllength = _command("derep_fulllength", 32, 0, False)
fastx_uniques = _command("fastx_uniques", 1, 0, True)
derep_id = _command("derep_id", 32, 1, False)
