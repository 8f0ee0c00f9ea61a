"""OTU / ASV tables (the reference's --otutabout, --biomout and --mothur_shared_out) over vsx_otutab (include/vsx_otutab.h).

otutab() takes the labels of the queries and of the targets, the first hit per query and, for a search, which targets were matched
at all, and returns an OtuTable: the sorted sample and OTU names, the taxonomy per OTU, the non-zero cells in the writers' order
and a rank per label.  from_search() and from_clusters() fold what SearchSession returns into that call.  otutabout_lines(),
mothur_shared_lines() and biom_text() reproduce the reference CLI's three files byte for byte; reading and writing files stays
with the caller, and so do --sizein (`sizes`), --notrunclabels and the relabelling modes other than a plain prefix.
otutab_host() is the same call through the library's host restatement.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Labels, OtutabOpts, OtutabResult, OtutabStats, check

NONE = 0xFFFFFFFF


def last_stats():
    s = OtutabStats()
    _lib.load().vsx_otutab_last_stats(C.byref(s))
    return {n: getattr(s, n) for n, _ in OtutabStats._fields_}


def _bytes(l):
    return l.encode("latin-1") if isinstance(l, str) else bytes(l)


class LabelBlob:
    """labels as vsx_labels wants them.  LabelBlob(list of str / bytes) packs them one after the other; LabelBlob.of(blob, offsets,
    lengths) takes spans as they are (they may overlap, repeat and come in any order)."""

    def __init__(self, labels):
        raw = [_bytes(l) for l in labels]
        self.blob = b"".join(raw)
        self.lengths = np.array([len(l) for l in raw], np.uint32)
        self.offsets = np.zeros(len(raw), np.uint64)
        if len(raw) > 1:
            np.cumsum(self.lengths[:-1], dtype=np.uint64, out=self.offsets[1:])

    @classmethod
    def of(cls, blob, offsets, lengths):
        self = cls.__new__(cls)
        self.blob = bytes(blob)
        self.offsets = np.ascontiguousarray(offsets, np.uint64)
        self.lengths = np.ascontiguousarray(lengths, np.uint32)
        if len(self.offsets) != len(self.lengths):
            raise ValueError("otutab: one offset and one length per label")
        return self

    def __len__(self):
        return len(self.lengths)

    def struct(self):
        return Labels(len(self), C.cast(C.c_char_p(self.blob), C.c_void_p), len(self.blob), self.offsets.ctypes.data, self.lengths.ctypes.data)


class OtuTable:
    """samples / otus: the sorted names (bytes).  tax: per OTU its taxonomy (bytes) or None.  has_tax: some add carried tax=.
    nz_otu / nz_sample / nz_count: the non-zero cells ordered by (OTU, sample).  q_sample: the sample rank of every query.
    t_otu: the OTU rank of every target that took part in an add, else NONE.  stats: vsx_otutab_last_stats of the call."""

    def __init__(self, samples, otus, tax, has_tax, nz_otu, nz_sample, nz_count, q_sample, t_otu, stats):
        self.samples, self.otus, self.tax, self.has_tax = samples, otus, tax, has_tax
        self.nz_otu, self.nz_sample, self.nz_count = nz_otu, nz_sample, nz_count
        self.q_sample, self.t_otu, self.stats = q_sample, t_otu, stats

    def arrays(self):
        """every result array in one tuple of plain Python / bytes values: what two routes must agree on"""
        return (self.samples, self.otus, self.tax, self.has_tax, self.nz_otu.tobytes(), self.nz_sample.tobytes(), self.nz_count.tobytes(),
                self.q_sample.tobytes(), self.t_otu.tobytes())

    def dense(self):
        """counts[otu][sample] as a uint64 matrix (for small tables)"""
        m = np.zeros((len(self.otus), len(self.samples)), np.uint64)
        m[self.nz_otu, self.nz_sample] = self.nz_count
        return m


def _names(blob, nbytes, off, lens, n, none_ok=False):
    raw = C.string_at(blob, int(nbytes)) if nbytes else b""
    out = []
    for r in range(n):
        o, l = int(off[r]), int(lens[r])
        out.append(None if (none_ok and l == NONE) else raw[o:o + l])
    return out


def otutab(qlabels, tlabels, q_target, sizes=None, matched=None, aligner=None, threads=0, _host=False):
    """Build the table.  qlabels / tlabels: lists of str or bytes, or LabelBlob.  q_target: per query the number of its first hit's
    target, NONE without a hit.  sizes: the queries' abundances (default 1 each; the reference's search commands pass the header's
    ;size= annotation with or without --sizein, its clustering commands only with --sizein).  matched: per target whether any hit
    reached it (a search: the others enter the table with no counts), or None (a clustering: no such pass).  aligner: an Aligner
    (its device runs the kernels), or None for the host restatement.  A value the library refuses raises VsxError (VSX_EINVAL)."""
    lib = _lib.load()
    Q = qlabels if isinstance(qlabels, LabelBlob) else LabelBlob(qlabels)
    T = tlabels if isinstance(tlabels, LabelBlob) else LabelBlob(tlabels)
    qt = np.ascontiguousarray(q_target, np.uint32)
    if len(qt) != len(Q):
        raise ValueError("otutab: one target per query")
    ab = None
    if sizes is not None:
        ab = np.ascontiguousarray(sizes, np.uint64)
        if len(ab) != len(Q):
            raise ValueError("otutab: one abundance per query")
    tm = None
    if matched is not None:
        tm = np.ascontiguousarray(np.asarray(matched) != 0, np.uint8)
        if len(tm) != len(T):
            raise ValueError("otutab: one matched flag per target")
    o = OtutabOpts()
    lib.vsx_otutab_opts_default(C.byref(o))
    o.threads = int(threads)
    qs, ts = Q.struct(), T.struct()
    out = OtutabResult()
    ptr = lambda a: a.ctypes.data if a is not None and len(a) else None  # noqa: E731
    if _host:
        check(lib.vsx_internal_otutab_host(C.byref(o), C.byref(qs), ptr(ab), ptr(qt), C.byref(ts), tm.ctypes.data if tm is not None else None,
                                           C.byref(out)), "vsx_internal_otutab_host")
    else:
        check(lib.vsx_otutab(aligner.h if aligner is not None else None, C.byref(o), C.byref(qs), ptr(ab), ptr(qt), C.byref(ts),
                             tm.ctypes.data if tm is not None else None, C.byref(out)), "vsx_otutab")
    try:
        ns, no, nc = int(out.n_samples), int(out.n_otus), int(out.n_cells)
        arr = lambda p, m, dt: np.ctypeslib.as_array(p, shape=(m,)).copy() if m else np.zeros(0, dt)  # noqa: E731
        samples = _names(out.sample_blob, out.sample_bytes, out.sample_off, out.sample_len, ns)
        otus = _names(out.otu_blob, out.otu_bytes, out.otu_off, out.otu_len, no)
        tax = _names(out.tax_blob, out.tax_bytes, out.tax_off, out.tax_len, no, none_ok=True)
        return OtuTable(samples, otus, tax, bool(out.has_tax), arr(out.nz_otu, nc, np.uint32), arr(out.nz_sample, nc, np.uint32),
                        arr(out.nz_count, nc, np.uint64), arr(out.q_sample, len(Q), np.uint32), arr(out.t_otu, len(T), np.uint32), last_stats())
    finally:
        lib.vsx_otutab_result_free(C.byref(out))


def otutab_host(qlabels, tlabels, q_target, sizes=None, matched=None, threads=0):
    """otutab() through vsx_internal_otutab_host, the library's host restatement"""
    return otutab(qlabels, tlabels, q_target, sizes=sizes, matched=matched, threads=threads, _host=True)


def from_search(qlabels, tlabels, first, hits, sizes=None, aligner=None, host=False):
    """The table of a search.  first, hits: what SearchSession.search_batch_raw / search_exact_raw return (the cigar blob is not
    needed).  A query's target is that of its first returned hit; a target counts as matched when any returned hit with `accepted`
    or `weak` names it -- so a target that was only ever a second hit is in neither pass and has no row, as in the reference."""
    first = np.asarray(first, np.uint64)
    n = len(first) - 1
    q_target = np.full(n, NONE, np.uint32)
    has = first[1:] > first[:-1]
    if len(hits):
        q_target[has] = hits["target"][first[:-1][has].astype(np.int64)]
    matched = np.zeros(len(tlabels), np.uint8)
    if len(hits):
        took = (hits["accepted"] != 0) | (hits["weak"] != 0)
        matched[hits["target"][took]] = 1
    if host:
        return otutab_host(qlabels, tlabels, q_target, sizes=sizes, matched=matched)
    return otutab(qlabels, tlabels, q_target, sizes=sizes, matched=matched, aligner=aligner)


def from_clusters(labels, clusterno, per, sizes=None, relabel=None, aligner=None, host=False):
    """The table of a clustering.  clusterno, per: what SearchSession.cluster_fast returns (per[s] is None for a centroid), labels:
    the sequences' labels in the same order.  Every sequence is a query whose target is its cluster's centroid; with
    relabel="P" the target's label is P followed by the 1-based cluster number in creation order, and goes through the same OTU
    scan as any label.  There is no unmatched pass."""
    n = len(clusterno)
    if len(labels) != n or len(per) != n:
        raise ValueError("from_clusters: one label and one hit entry per sequence")
    ncl = (max(clusterno) + 1) if n else 0
    centroid = [None] * ncl
    for s in range(n):
        if per[s] is None:
            centroid[clusterno[s]] = s
    if relabel is not None:
        prefix = _bytes(relabel)
        tlabels = [prefix + str(c + 1).encode() for c in range(ncl)]
    else:
        tlabels = [_bytes(labels[centroid[c]]) for c in range(ncl)]
    q_target = np.asarray(clusterno, np.uint32)
    if host:
        return otutab_host(labels, tlabels, q_target, sizes=sizes)
    return otutab(labels, tlabels, q_target, sizes=sizes, aligner=aligner)


def _rows(t):
    """per OTU the (sample, count) pairs of its cells, from the sorted cell list"""
    cut = np.searchsorted(t.nz_otu, np.arange(len(t.otus) + 1))
    return [(t.nz_sample[cut[r]:cut[r + 1]], t.nz_count[cut[r]:cut[r + 1]]) for r in range(len(t.otus))]


def otutabout_lines(t):
    """--otutabout: the header, then a line per OTU (bytes, without the newline)"""
    head = b"#OTU ID" + b"".join(b"\t" + s for s in t.samples)
    if t.has_tax:
        head += b"\ttaxonomy"
    lines = [head]
    ns = len(t.samples)
    for r, (cols, counts) in enumerate(_rows(t)):
        row = np.zeros(ns, np.uint64)
        row[cols] = counts
        line = t.otus[r] + b"".join(b"\t%d" % int(v) for v in row)
        if t.has_tax:
            line += b"\t" + (t.tax[r] or b"")
        lines.append(line)
    return lines


def mothur_shared_lines(t):
    """--mothur_shared_out: the header, then a line per sample (bytes, without the newline)"""
    lines = [b"label\tGroup\tnumOtus" + b"".join(b"\t" + o for o in t.otus)]
    no = len(t.otus)
    order = np.lexsort((t.nz_otu, t.nz_sample))
    cut = np.searchsorted(t.nz_sample[order], np.arange(len(t.samples) + 1))
    for s, name in enumerate(t.samples):
        row = np.zeros(no, np.uint64)
        sel = order[cut[s]:cut[s + 1]]
        row[t.nz_otu[sel]] = t.nz_count[sel]
        lines.append(b"vsearch\t" + name + b"\t%d" % no + b"".join(b"\t%d" % int(v) for v in row))
    return lines


def biom_text(t, table_id, generated_by, date):
    """--biomout (BIOM 1.0, sparse), the whole file as bytes.  The reference prints the --biomout file name as id, "vsearch <version>"
    as generated_by and a local ISO 8601 timestamp as date."""
    out = [b"{\n\t\"id\":\"" + _bytes(table_id) + b"\",\n"
           b"\t\"format\": \"Biological Observation Matrix 1.0\",\n"
           b"\t\"format_url\": \"http://biom-format.org/documentation/format_versions/biom-1.0.html\",\n"
           b"\t\"type\": \"OTU table\",\n"
           b"\t\"generated_by\": \"" + _bytes(generated_by) + b"\",\n"
           b"\t\"date\": \"" + _bytes(date) + b"\",\n"
           b"\t\"matrix_type\": \"sparse\",\n"
           b"\t\"matrix_element_type\": \"int\",\n"
           b"\t\"shape\": [%d,%d],\n" % (len(t.otus), len(t.samples))]
    rows = []
    for r, name in enumerate(t.otus):
        meta = (b"{\"taxonomy\":\"" + (t.tax[r] or b"") + b"\"}") if t.has_tax else b"null"
        rows.append(b"\n\t\t{\"id\":\"" + name + b"\", \"metadata\":" + meta + b"}")
    out.append(b"\t\"rows\":[" + b",".join(rows) + b"\n\t],\n")
    cols = [b"\n\t\t{\"id\":\"" + name + b"\", \"metadata\":null}" for name in t.samples]
    out.append(b"\t\"columns\":[" + b",".join(cols) + b"\n\t],\n")
    data = [b"\n\t\t[%d,%d,%d]" % (int(a), int(b), int(c)) for a, b, c in zip(t.nz_otu, t.nz_sample, t.nz_count)]
    out.append(b"\t\"data\": [" + b",".join(data) + b"\n\t]\n}\n")
    return b"".join(out)
