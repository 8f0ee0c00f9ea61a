"""Seeded generator of read pairs for the merge tests and bench_merge.py, and a runner of the reference CLI's
--fastq_mergepairs (oracle/_ref/vsearch_ref) that returns its outputs as lists of lines.

Pairs are simulated amplicon reads: a random fragment, the forward read from its 5' end and the reverse read from the
other strand's 5' end, qualities that decay toward the 3' end, substitutions drawn from the qualities.  Fragment lengths
run from far below the read length (staggered pairs, with read-through into random adapter) to beyond twice the read
length (no overlap).  A share of the pairs is built to land in particular verdicts of the merge core: tandem repeats
(several good diagonals), spaced substitutions in a long overlap (too many differences), short high-quality overlaps
(overlap too short), N's, and reads of unequal length.
"""
import os
import subprocess
import tempfile

import numpy as np

BASES = np.frombuffer(b"ACGT", np.uint8)
_COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGTNacgtn", b"TGCANtgcan"):
    _COMP[_a] = _b

# the lines of the reference's statistics block (--log), by reason name
LOG_REASONS = {
    "reads too short (after truncation)": "minlen", "reads too long (after truncation)": "maxlen", "too many N's": "maxns",
    "too few kmers found on same diagonal": "nokmers", "multiple potential alignments": "repeat",
    "too many differences": "maxdiffs", "too high percentage of differences": "maxdiffpct",
    "alignment score too low, or score drop too high": "minscore", "overlap too short": "minovlen",
    "expected error too high": "maxee", "merged fragment too short": "minmergelen", "merged fragment too long": "maxmergelen",
    "staggered read pairs": "staggered",
}

CLI_FLAGS = {"minovlen": "--fastq_minovlen", "maxdiffs": "--fastq_maxdiffs", "maxdiffpct": "--fastq_maxdiffpct",
             "truncqual": "--fastq_truncqual", "maxns": "--fastq_maxns", "maxee": "--fastq_maxee",
             "minmergelen": "--fastq_minmergelen", "maxmergelen": "--fastq_maxmergelen", "qmaxout": "--fastq_qmaxout",
             "qminout": "--fastq_qminout", "qmax": "--fastq_qmax", "qmin": "--fastq_qmin", "minlen": "--fastq_minlen",
             "maxlen": "--fastq_maxlen", "ascii": "--fastq_ascii"}


def revcomp(a):
    return _COMP[a[::-1]]


def _qualities(rng, n, flat=False, qrange=(2, 41)):
    """qualities drawn on the scale 2..41 and stretched linearly onto qrange (the identity for the default range)"""
    if n == 0:
        return np.zeros(0, np.int64)
    if flat:
        q = np.full(n, 38, np.int64) + rng.integers(-2, 3, n)
    else:
        start, drop = rng.integers(32, 41), rng.integers(5, 36)
        q = start - drop * (np.arange(n) / max(n, 1)) ** 2 + rng.normal(0, 2.5, n)
        q = np.clip(np.rint(q), 2, 41).astype(np.int64)
    lo, hi = qrange
    return lo + ((q - 2) * (hi - lo) + 19) // 39


def _with_errors(rng, seq, q):
    seq = seq.copy()
    hit = rng.random(len(seq)) < 10.0 ** (-np.maximum(q, 2) / 10.0)
    for p in np.flatnonzero(hit):
        seq[p] = BASES[(np.searchsorted(BASES, seq[p]) + rng.integers(1, 4)) % 4]
    return seq


def generate(seed, n, read_len=250, ascii=33, qrange=(2, 41)):
    """-> labels, fwd, fqual, rev, rqual: lists of str, n pairs.  ascii: the quality offset of the strings; qrange: the lowest and
    the highest quality value that occurs (the defaults give the pairs this function has always given)"""
    rng = np.random.default_rng(seed)
    labels, fwd, fqual, rev, rqual = [], [], [], [], []
    for k in range(n):
        kind = rng.random()
        flen = rlen = read_len
        flat = False
        if kind < 0.06:                                   # tandem repeat
            unit = BASES[rng.integers(0, 4, rng.integers(5, 13))]
            L = int(rng.integers(read_len, 2 * read_len - 20))
            frag = np.tile(unit, L // len(unit) + 1)[:L]
        else:
            if kind < 0.12:                               # a short, clean overlap
                L = int(2 * read_len - rng.integers(5, 16))
                flat = True
            elif kind < 0.22:                             # no overlap, or next to none
                L = int(rng.integers(2 * read_len - 6, 2 * read_len + 60))
            elif kind < 0.30:                             # reads of unequal length (the shorter forward read gives staggered pairs)
                lo = min(40, read_len - 1)
                flen, rlen = int(rng.integers(lo, read_len)), int(rng.integers(lo, read_len + 1))
                L = int(rng.integers(30, flen + rlen))
            elif 0.42 <= kind < 0.50:                     # a fragment shorter than the reads: staggered, read-through
                L = int(rng.integers(int(0.3 * read_len), read_len))
            else:
                L = int(rng.integers(int(0.85 * read_len), 2 * read_len))
            frag = BASES[rng.integers(0, 4, L)]
        # reads run through the fragment's end into adapter
        ftrue = np.concatenate([frag, BASES[rng.integers(0, 4, max(0, flen - L))]])[:flen]
        rtrue = np.concatenate([revcomp(frag), BASES[rng.integers(0, 4, max(0, rlen - L))]])[:rlen]
        fq, rq = _qualities(rng, len(ftrue), flat, qrange), _qualities(rng, len(rtrue), flat, qrange)
        f, r = _with_errors(rng, ftrue, fq), _with_errors(rng, rtrue, rq)
        if 0.30 <= kind < 0.38 and len(r) > 60:           # spaced substitutions at high quality: many differences, no big drop
            for p in range(int(rng.integers(0, 12)), len(r), int(rng.integers(9, 16))):
                r[p] = BASES[(np.searchsorted(BASES, r[p]) + 1) % 4]
                rq[p] = min(max(rq[p], 30), qrange[1])
        if 0.38 <= kind < 0.42:                           # N's
            for read in (f, r):
                read[rng.integers(0, len(read), rng.integers(1, 6))] = ord("N")
        labels.append(f"pair{k}")
        fwd.append(f.tobytes().decode()); fqual.append((fq + ascii).astype(np.uint8).tobytes().decode())
        rev.append(r.tobytes().decode()); rqual.append((rq + ascii).astype(np.uint8).tobytes().decode())
    return labels, fwd, fqual, rev, rqual


def edge_pairs():
    """-> labels, fwd, fqual, rev, rqual: lower-case and ambiguous symbols, reads shorter than 5, identical reads,
    low-complexity repeats (every symbol is one the reference's FASTQ reader accepts)"""
    rng = np.random.default_rng(77)
    frag = BASES[rng.integers(0, 4, 180)].tobytes().decode()
    rc = revcomp(np.frombuffer(frag.encode(), np.uint8)).tobytes().decode()
    hi = lambda s: "I" * len(s)          # noqa: E731
    pairs = [
        ("lower", frag[:120].lower(), rc[:120]),
        ("mixedcase", "".join(c.lower() if i % 3 else c for i, c in enumerate(frag[:130])), rc[:130].lower()),
        ("ambig", frag[:60] + "RYKMSWBDHVN" + frag[71:140], rc[:50] + "nryk" + rc[54:140]),
        ("uracil", frag[:140].replace("T", "U"), rc[:140]),
        ("short4", "ACGT", "ACGT"), ("short1", "A", "T"), ("short5", "ACGTA", "TACGT"), ("short_vs_long", "ACG", rc[:100]),
        ("identical", frag[:100], frag[:100]),
        ("palindrome", "ACGT" * 30, "ACGT" * 30),
        ("homopolymer", "A" * 120, "T" * 120),
        ("dinucleotide", "AC" * 70, "GT" * 70),
        ("unit7", "ACGGTCA" * 25, revcomp(np.frombuffer(("ACGGTCA" * 25).encode(), np.uint8)).tobytes().decode()),
        ("full_overlap", frag, rc),
        ("all_n", "N" * 50, "N" * 50),
    ]
    labels = [p[0] for p in pairs]
    fwd = [p[1] for p in pairs]
    rev = [p[2] for p in pairs]
    return labels, fwd, [hi(s) for s in fwd], rev, [hi(s) for s in rev]


def _rc(s):
    return revcomp(np.frombuffer(s.encode(), np.uint8)).tobytes().decode()


def _rnd(rng, n):
    return BASES[rng.integers(0, 4, n)].tobytes().decode()


def _reads(rng, frag, F, R):
    """the forward and the reverse read of a fragment, read through into random adapter where the fragment is shorter"""
    return (frag + _rnd(rng, max(0, F - len(frag))))[:F], (_rc(frag) + _rnd(rng, max(0, R - len(frag))))[:R]


def _put(q, pos, ch):
    return q[:pos] + ch + q[pos + 1:]


BOUNDARY_LENGTHS = [(5, 5), (5, 9), (6, 6), (8, 8), (8, 64), (9, 9), (9, 10), (10, 10), (10, 5), (10, 65), (63, 63), (63, 64), (64, 63),
                    (64, 64), (64, 65), (65, 65), (65, 127), (127, 127), (127, 128), (128, 64), (128, 128), (128, 129), (129, 129),
                    (129, 63), (255, 255), (255, 256), (256, 256), (256, 257), (257, 257), (257, 128), (511, 511), (511, 512),
                    (512, 511), (512, 512), (512, 9), (9, 512), (512, 257), (65, 512), (256, 6), (6, 129)]
# what the truncation and the N groups of boundary_pairs() need; every other pair reads the same with or without them
BOUNDARY_OPTS = {"truncqual": 2, "maxns": 4}
TRUNCATION_POINTS = (0, 1, 63, 64, 65, 127, 128, 191, 192, 249)


def n_pairs(ascii=33, q=40, maxns=4):
    """-> labels, fwd, fqual, rev, rqual: exactly maxns and maxns + 1 N's in one read, no two in the same lane of a 64-lane stride
    (p mod 64 distinct); N's at 63 / 64; N's inside the overlap facing a base and facing an N, and in the overhang.  250-symbol reads
    of a 300-symbol fragment: forward position p and reverse position 299 - p read the same fragment position."""
    rng = np.random.default_rng(909)
    spread = [3, 70, 140, 200, 249, 17, 90][:maxns + 1]
    assert len({p % 64 for p in spread}) == len(spread) == maxns + 1
    cases = [("at_maxns_fwd", spread[:maxns], []), ("over_maxns_fwd", spread, []), ("at_maxns_rev", [], spread[:maxns]),
             ("over_maxns_rev", [], spread), ("at_63_64", [63, 64], [63, 64]), ("faces_base", [150], []), ("faces_n", [150], [149]),
             ("faces_n_63", [236], [63]), ("overhang", [10], [20]), ("overlap_edges", [50, 249], [50, 249])]
    out = [[], [], [], [], []]
    for name, fn, rn in cases:
        f, r = _reads(rng, _rnd(rng, 300), 250, 250)
        for p in fn:
            f = _put(f, p, "N")
        for p in rn:
            r = _put(r, p, "N")
        for col, v in zip(out, ("n_" + name, f, chr(ascii + q) * 250, r, chr(ascii + q) * 250)):
            col.append(v)
    return out


def boundary_pairs():
    """-> labels, fwd, fqual, rev, rqual: a fixed list of pairs at the boundaries of the merge kernel (one wave per pair, 64 lanes
    striding over positions and diagonals).  To be merged with BOUNDARY_OPTS (plus whatever a test adds).

    len_*    (F, R) of BOUNDARY_LENGTHS; per combination a full overlap, overlaps of exactly 10, 9 and 5, a stagger of 1 and a
             stagger of min(F, R) - 6 (where the lengths allow), flat Q40
    trunc_*  250-symbol reads of a 260-symbol fragment (shorter where both reads are cut, so they still overlap); the first quality at truncqual 2 ('#') at TRUNCATION_POINTS on the forward
             read, the reverse read and both, then a second '#' and a Q42 symbol behind it that no reader may look at
    cap_*    homopolymer, dinucleotide, unit-5 and unit-7 pairs at 512 x 512 and 512 x 511 (every diagonal passes the census), two
             exact tandem copies, and two pairs whose two best diagonals tie below minscore: the first is not staggered, the second
             is, so the verdict (minscore, not staggered) shows which one won
    n_*      n_pairs()"""
    rng = np.random.default_rng(4242)
    out = [[], [], [], [], []]

    def add(label, f, r, fq=None, rq=None):
        for col, v in zip(out, (label, f, fq or "I" * len(f), r, rq or "I" * len(r))):
            col.append(v)

    for F, R in BOUNDARY_LENGTHS:
        m = min(F, R)
        frags = [("full", max(F, R))] + [(f"ov{k}", F + R - k) for k in (10, 9, 5) if k <= m] + [("stagger1", R - 1)]
        if m - 6 >= 2:
            frags.append(("staggermax", R - (m - 6)))
        for name, L in frags:
            if L >= 1:
                add(f"len_{F}_{R}_{name}", *_reads(rng, _rnd(rng, L), F, R))
    for side in ("fwd", "rev", "both"):
        for p in TRUNCATION_POINTS:
            f, r = _reads(rng, _rnd(rng, 260 if side != "both" else min(260, max(30, 2 * p - 20))), 250, 250)
            q = "I" * 250
            for at, ch in ((p, "#"), (p + 2, "#"), (p + 3, "K")):
                if at < 250:
                    q = _put(q, at, ch)
            add(f"trunc_{side}_{p}", f, r, q if side != "rev" else None, q if side != "fwd" else None)
    for name, unit in (("homopolymer", "A"), ("dinucleotide", "AC"), ("unit5", "ACGGT"), ("unit7", "ACGGTCA")):
        for R in (512, 511):
            frag = (unit * 512)[:512]
            add(f"cap_{name}_{R}", frag, _rc(frag)[:R])
    u = _rnd(rng, 100)
    add("cap_tandem2", u + u, _rc(u + u))
    add("cap_tandem2_short_rev", u + u, _rc(u))
    for F, R in ((40, 40), (100, 70)):
        x = "GATTACAG"                                # 8 matches at Q40 score 15.998 < minscore 16
        f = x + "".join("AC"[k % 2] for k in range(F - 16)) + x
        rcr = x + "".join("GT"[k % 2] for k in range(R - 16)) + x
        add(f"cap_tie_{F}_{R}", f, _rc(rcr))
    for col, extra in zip(out, n_pairs()):
        col.extend(extra)
    return out


def quality_order_pairs(swapped=False):
    """300 pairs for a run with window 64: pair 40 is longer than the kernel's 512 (host route) and holds Q43, pair 130 is a device
    pair and holds Q42; swapped: pair 40 the device pair with Q42, pair 130 the long one with Q43.  The reference stops at the
    first bad value in input order."""
    rng = np.random.default_rng(31)
    data = [list(c) for c in generate(20269, 300, read_len=100)]
    lf, lr = _reads(rng, _rnd(rng, 900), 600, 600)
    sf, sr = _reads(rng, _rnd(rng, 150), 100, 100)
    long_ = (lf, _put("I" * 600, 300, "L"), lr, "I" * 600)
    short = (sf, "I" * 100, sr, _put("I" * 100, 70, "K"))
    for k, pair in ((130, long_), (40, short)) if swapped else ((40, long_), (130, short)):
        for col, v in zip(data[1:], pair):
            col[k] = v
    return data


def truncated(q, ascii=33, truncqual=None):
    if truncqual is None:
        return len(q)
    return next((p for p, c in enumerate(q) if ord(c) - ascii <= truncqual), len(q))


def disagreement_sides(f, fq, r, rq, merged_len, ascii=33, truncqual=None):
    """-> (columns of the overlap where the reads disagree and the forward quality is the higher, ... the reverse quality is the
    higher), from the inputs and the merged length alone; (0, 0) for a staggered pair"""
    ftr, rtr = truncated(fq, ascii, truncqual), truncated(rq, ascii, truncqual)
    ov = ftr + rtr - merged_len
    if not 0 < ov <= min(ftr, rtr):
        return 0, 0
    rc, rcq = _rc(r[:rtr].upper().replace("U", "T")), rq[:rtr][::-1]
    nf = nr = 0
    for t in range(ov):
        a, b = f[ftr - ov + t].upper().replace("U", "T"), rc[t]
        if a != b and a in "ACGT" and b in "ACGT":
            qa, qb = fq[ftr - ov + t], rcq[t]
            nf += qa > qb
            nr += qb > qa
    return nf, nr


def write_fastq(path, labels, seqs, quals):
    with open(path, "w") as fh:
        for lab, s, q in zip(labels, seqs, quals):
            fh.write(f"@{lab}\n{s}\n+\n{q}\n")


def ref_binary():
    here = os.path.dirname(os.path.abspath(__file__))
    return os.path.join(os.path.dirname(here), "oracle", "_ref", "vsearch_ref")


def parse_log_reasons(text):
    """reason counts of the statistics block the reference writes to --log (or stderr)"""
    out = {}
    for line in text.splitlines():
        parts = line.strip().split("  ", 1)
        if len(parts) == 2 and parts[1].strip() in LOG_REASONS and parts[0].strip().isdigit():
            out[LOG_REASONS[parts[1].strip()]] = int(parts[0])
    return out


def run_reference(labels, fwd, fqual, rev, rqual, threads=1, allowmergestagger=False, **opts):
    """Run the reference CLI on the pairs.  -> dict(returncode, stderr, fastq (lines of --fastqout with --fastq_eeout),
    eetabbed (lines), notmerged (forward labels), reasons (counts from --log), seconds)"""
    import time
    with tempfile.TemporaryDirectory() as d:
        p = lambda n: os.path.join(d, n)       # noqa: E731
        write_fastq(p("f.fq"), labels, fwd, fqual)
        write_fastq(p("r.fq"), labels, rev, rqual)
        args = [ref_binary(), "--fastq_mergepairs", p("f.fq"), "--reverse", p("r.fq"), "--fastqout", p("m.fq"), "--fastq_eeout",
                "--eetabbedout", p("ee.tsv"), "--fastqout_notmerged_fwd", p("nf.fq"), "--log", p("log.txt"),
                "--threads", str(threads), "--quiet"]
        if allowmergestagger:
            args.append("--fastq_allowmergestagger")
        for k, v in opts.items():
            args += [CLI_FLAGS[k], str(v)]
        t0 = time.perf_counter()
        r = subprocess.run(args, capture_output=True, text=True)
        dt = time.perf_counter() - t0
        read = lambda n: open(p(n)).read().splitlines() if os.path.exists(p(n)) else []      # noqa: E731
        log = open(p("log.txt")).read() if os.path.exists(p("log.txt")) else ""
        return {"returncode": r.returncode, "stderr": r.stderr, "fastq": read("m.fq"), "eetabbed": read("ee.tsv"),
                "notmerged": [ln[1:] for ln in read("nf.fq")[0::4]], "reasons": parse_log_reasons(log), "seconds": dt}


# the option sets of tests/golden/merge_golden.json (keywords of vsearch_amd.merge.merge_pairs / run_reference)
GOLDEN_OPTION_SETS = [
    {},
    {"minovlen": 5, "maxdiffs": 1, "truncqual": 8, "maxns": 1, "maxee": 0.05, "minmergelen": 48, "maxmergelen": 80,
     "qmaxout": 50, "allowmergestagger": True},
    {"minovlen": 7, "maxdiffpct": 3.0, "truncqual": 15, "maxns": 0, "maxee": 0.5, "minlen": 24, "maxlen": 48,
     "qmaxout": 30, "qminout": 5},
]


def parse_fastq(path):
    lines = open(path).read().splitlines()
    return [ln[1:] for ln in lines[0::4]], lines[1::4], lines[3::4]


def pack_golden(node):
    """lists of strings are stored as one newline-joined string (one line of the file per field)"""
    if isinstance(node, dict):
        return {k: pack_golden(v) for k, v in node.items()}
    if isinstance(node, list) and all(isinstance(x, str) for x in node):
        return {"lines": "\n".join(node), "n": len(node)}
    if isinstance(node, list):
        return [pack_golden(x) for x in node]
    return node


def unpack_golden(node):
    if isinstance(node, dict):
        if set(node) == {"lines", "n"}:
            return node["lines"].split("\n") if node["n"] else []
        return {k: unpack_golden(v) for k, v in node.items()}
    if isinstance(node, list):
        return [unpack_golden(x) for x in node]
    return node


def load_golden(path):
    import json
    with open(path) as fh:
        return unpack_golden(json.load(fh))


def write_golden(path, example_dir):
    """Record the reference CLI's answers: generate(11, 200, read_len=48) + edge_pairs() under GOLDEN_OPTION_SETS, and
    the reference's own api_examples merge pair (example_dir) at default options."""
    import json
    g, e = generate(11, 200, read_len=48), edge_pairs()
    data = [a + b for a, b in zip(g, e)]
    keys = ("labels", "fwd", "fqual", "rev", "rqual")
    doc = {"inputs": dict(zip(keys, data)), "cases": []}
    for opts in GOLDEN_OPTION_SETS:
        ref = run_reference(*data, **opts)
        assert ref["returncode"] == 0, ref["stderr"]
        doc["cases"].append({"opts": opts, **{k: ref[k] for k in ("fastq", "eetabbed", "notmerged", "reasons")}})
    lab, fs, fq = parse_fastq(os.path.join(example_dir, "merge_fwd.fastq"))
    _, rs, rq = parse_fastq(os.path.join(example_dir, "merge_rev.fastq"))
    ref = run_reference(lab, fs, fq, rs, rq)
    doc["example"] = {"inputs": dict(zip(keys, (lab, fs, fq, rs, rq))),
                      "expected_fasta": open(os.path.join(example_dir, "expected_merge.fasta")).read(),
                      **{k: ref[k] for k in ("fastq", "eetabbed", "notmerged", "reasons")}}
    with open(path, "w") as fh:
        json.dump(pack_golden(doc), fh, indent=0)


if __name__ == "__main__":
    import sys
    write_golden(sys.argv[1], sys.argv[2])
