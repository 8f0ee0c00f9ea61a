"""Inputs, a plain-Python restatement and the reference-CLI runner for the dereplication tests (--derep_fulllength,
--fastx_uniques, --derep_id).

    py_derep()        the reference's loop (core/derep.cpp: derep()) over a dictionary of normalised strings: both strands, sizes,
                      the quality merge with math.log10, the order of the clusters, the counts of the log lines
    *_set()           input builders: the worked examples, the alphabet, palindromes, ties, discards, options, FASTQ in both
                      quality modes; and the device sets (lengths around the kernels' chunk sizes, cluster sizes, quality blocks,
                      table steps, seeded reads)
    run_reference()   the reference CLI (oracle/_ref/vsearch_ref) on one set: --output / --fastaout, --fastqout, --uc,
                      --tabbedout, --log
    __main__          writes tests/golden/derep_golden.json: the sets' inputs and the reference's recorded lines, nothing else
"""
import json
import math
import os
import random
import re
import subprocess
import tempfile

from tests.search_exact_data import IUPAC, norm, random_seq, revcomp, substitute

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "derep_golden.json")
INT64_MAX = (1 << 63) - 1

COMMAND_MINSEQLENGTH = {"derep_fulllength": 32, "fastx_uniques": 1, "derep_id": 32}
DEFAULT_OPTS = dict(strand_both=0, sizein=0, maxseqlength=50000, minuniquesize=1, maxuniquesize=INT64_MAX, topn=INT64_MAX, qout_max=0,
                    ascii=33, asciiout=33, qminout=0, qmaxout=41)
DEFAULT_FMT = dict(sizeout=False, relabel=None, xsize=False, fasta_width=80)


def full_opts(s):
    o = dict(DEFAULT_OPTS, minseqlength=COMMAND_MINSEQLENGTH[s["cmd"]])
    o.update(s.get("opts") or {})
    return o


def full_fmt(s):
    f = dict(DEFAULT_FMT)
    f.update(s.get("fmt") or {})
    return f


def abundances(labels):
    """--sizein as the caller resolves it: the first ;size=N annotation of a label, 1 without one"""
    out = []
    for l in labels:
        m = re.search(r"(?:^|;)size=(\d+)(?:;|$)", l)
        out.append(int(m.group(1)) if m else 1)
    return out


def sizes_of(s):
    return abundances(s["labels"]) if full_opts(s)["sizein"] else None


# ---- the plain-Python restatement ---------------------------------------------------------------------------------------------
def _prob(sym, ascii_):
    q = ord(sym) - ascii_
    return 0.75 if q < 2 else math.pow(10.0, -q / 10.0)


def merge_symbol(q1, q2, s1, s2, o):
    p1, p2 = _prob(q1, o["ascii"]), _prob(q2, o["ascii"])
    p3 = min(p1, p2) if o["qout_max"] else (p1 * float(s1) + p2 * float(s2)) / float(s1 + s2)
    v = int(math.trunc(-10.0 * math.log10(p3)))
    return chr(max(min(v, o["qmaxout"]), o["qminout"]) + o["asciiout"])


def py_derep(s, want_quality=None):
    """-> dict(clusters=[dict(rep, size, count, members, strands, qual)] in output order, counts=the log lines' figures)"""
    o = full_opts(s)
    seqs, labels, quals = s["seqs"], s["labels"], s.get("quals")
    if want_quality is None:
        want_quality = quals is not None
    sizes = sizes_of(s) or [1] * len(seqs)
    by_label = s["cmd"] == "derep_id"
    table, clusters = {}, []
    counts = dict(kept=0, nucleotides=0, shortest=0, longest=0, discarded_short=0, discarded_long=0, sumsize=0, maxsize=0)
    shortest = None
    for k, seq in enumerate(seqs):
        if len(seq) < o["minseqlength"]:
            counts["discarded_short"] += 1
            continue
        if len(seq) > o["maxseqlength"]:
            counts["discarded_long"] += 1
            continue
        counts["kept"] += 1
        counts["nucleotides"] += len(seq)
        counts["longest"] = max(counts["longest"], len(seq))
        shortest = len(seq) if shortest is None else min(shortest, len(seq))
        extra = labels[k] if by_label else None
        c, strand = table.get((norm(seq), extra)), 0
        if c is None and o["strand_both"]:
            c, strand = table.get((norm(revcomp(seq)), extra)), 1
        counts["sumsize"] += sizes[k]
        if c is None:
            table[(norm(seq), extra)] = len(clusters)
            clusters.append(dict(rep=k, size=sizes[k], count=1, members=[k], strands=[0], qual=quals[k] if want_quality else None))
            continue
        cl = clusters[c]
        if want_quality:
            cl["qual"] = "".join(merge_symbol(a, b, cl["size"], sizes[k], o) for a, b in zip(cl["qual"], quals[k]))
        cl["size"] += sizes[k]
        cl["count"] += 1
        cl["members"].append(k)
        cl["strands"].append(strand)
    counts["shortest"] = shortest or 0
    # strcmp: bytes compare as unsigned characters
    clusters.sort(key=lambda cl: (-cl["size"], labels[cl["rep"]].encode("latin-1"), cl["rep"]))
    n = len(clusters)
    counts["maxsize"] = max((cl["size"] for cl in clusters), default=0)
    if n == 0:
        counts["median"] = 0.0
    elif n % 2:
        counts["median"] = float(clusters[n // 2]["size"])
    else:
        counts["median"] = clusters[n // 2]["size"] + (clusters[n // 2 - 1]["size"] - clusters[n // 2]["size"]) * 0.5
    in_range = sum(1 for cl in clusters if o["minuniquesize"] <= cl["size"] <= o["maxuniquesize"])
    counts["selected"] = min(in_range, o["topn"])
    return dict(clusters=clusters, counts=counts)


def result_fields(res):
    """a DerepResult in py_derep's shape"""
    clusters = []
    for c in range(len(res)):
        clusters.append(dict(rep=int(res.rep[c]), size=int(res.size[c]), count=int(res.count[c]), members=[int(m) for m in res.members(c)],
                             strands=[int(x) for x in res.strands(c)], qual=res.quals[c] if res.quals is not None else None))
    return dict(clusters=clusters, counts=dict(res.counts))


def call(aligner, s, want_quality=None, **extra):
    """the set through the package's entry point of its command"""
    from vsearch_amd import derep
    o = full_opts(s)
    fastq = s.get("quals") is not None
    kw = {k: o[k] for k in ("strand_both", "minseqlength", "maxseqlength", "minuniquesize", "maxuniquesize", "topn", "qout_max", "ascii",
                            "asciiout", "qminout", "qmaxout")}
    kw.update(extra)
    want = fastq if want_quality is None else want_quality
    return getattr(derep, s["cmd"])(aligner, s["seqs"], s["labels"], quals=s.get("quals"), sizes=sizes_of(s), fastqout=want,
                                    tabbedout=fastq, **kw)


def formatted(res, s):
    """the formatters' text in the shape run_reference records"""
    f = full_fmt(s)
    out = dict(fasta=res.fasta_lines(sizeout=f["sizeout"], relabel=f["relabel"], xsize=f["xsize"], fasta_width=f["fasta_width"]),
               uc=res.uc_lines(), log=res.log_lines())
    if s.get("quals") is not None:
        out["fastq"] = res.fastq_lines(sizeout=f["sizeout"], relabel=f["relabel"], xsize=f["xsize"])
        out["tabbed"] = res.tabbed_lines(relabel=f["relabel"])
    return out


# ---- input builders --------------------------------------------------------------------------------------------------------------
def _set(name, cmd, seqs, labels=None, quals=None, opts=None, fmt=None):
    return dict(name=name, cmd=cmd, seqs=list(seqs), labels=list(labels) if labels else [f"r{k}" for k in range(len(seqs))],
                quals=list(quals) if quals is not None else None, opts=opts or {}, fmt=fmt or {})


def worked_examples():
    """TTTT then AAAA: one cluster, the second on minus; ACGT / acgu: plus, the first one's text printed"""
    seqs = ["TTTT", "ACGT", "CCCA", "acgu", "CCCA", "AAAA", "TGGG"]
    labels = ["a1", "b2", "c3", "d4", "e5", "s6", "g7"]
    return _set("worked_examples", "fastx_uniques", seqs, labels, opts=dict(strand_both=1))


def alphabet_set():
    frame = "GATTACA{}CATTAGGC"
    seqs = []
    for c in IUPAC:
        seqs += [frame.format(c), frame.format(c.lower())]
    seqs += [frame.format("T").replace("T", "U"), frame.format("u").lower(), frame.format("A"), frame.format("N")]
    return _set("alphabet", "fastx_uniques", seqs)


def palindromes_set():
    pal = "ACGTTGCATGCAACGT"
    assert revcomp(pal) == pal
    seqs = [pal, "AATT", pal.lower(), "GGATCC", "AATT", "ACGTTGCATGCAACGA", "GGATCC"]
    return _set("palindromes", "fastx_uniques", seqs, opts=dict(strand_both=1))


def rc_first_set():
    rng = random.Random(31)
    a, b = random_seq(rng, 40), random_seq(rng, 40)
    seqs = [revcomp(a), b, a, revcomp(b), a, revcomp(a)]
    return [_set("rc_first", "derep_fulllength", seqs, opts=dict(strand_both=1)),
            _set("rc_first_plus_only", "derep_fulllength", seqs)]


def ties_set():
    rng = random.Random(37)
    a, b, c, d = (random_seq(rng, 35) for _ in range(4))
    seqs = [a, b, c, d, a, b, c, d, d]
    labels = ["zeta", "alpha", "Alpha", "beta", "x1", "x2", "x3", "x4", "x5"]
    same = _set("ties_same_label", "derep_fulllength", [a, b, c, a, b, c], ["same"] * 6)
    return [_set("ties_label", "derep_fulllength", seqs, labels), same]


def sizein_sets():
    rng = random.Random(41)
    a, b, c = (random_seq(rng, 36) for _ in range(3))
    seqs = [a, b, a, c, b, revcomp(c), a]
    labels = ["r0;size=3", "r1", "r2;size=10;", "r3;size=2", "r4;size=1", "r5", "tag;size=7;extra=1"]
    return [_set("sizein", "derep_fulllength", seqs, labels, opts=dict(sizein=1, strand_both=1), fmt=dict(sizeout=True)),
            _set("sizein_ignored", "derep_fulllength", seqs, labels, opts=dict(strand_both=1), fmt=dict(sizeout=True)),
            _set("sizein_xsize", "derep_fulllength", seqs, labels, opts=dict(sizein=1, strand_both=1), fmt=dict(xsize=True))]


def selection_set():
    rng = random.Random(43)
    base = [random_seq(rng, 33) for _ in range(7)]
    seqs = []
    for k, b in enumerate(base):
        seqs += [b] * (k + 1)
    rng.shuffle(seqs)
    return _set("selection", "derep_fulllength", seqs, opts=dict(minuniquesize=2, maxuniquesize=6, topn=3))


def discards_set():
    rng = random.Random(47)
    seqs = [random_seq(rng, n) for n in (31, 32, 33, 60, 61, 5, 40, 32)]
    seqs += [seqs[1], seqs[3]]
    return _set("discards", "derep_fulllength", seqs, opts=dict(maxseqlength=60))


def empty_sequences_set():
    return _set("empty_sequences", "fastx_uniques", ["", "ACGT", "", "A", "ACGT", ""], opts=dict(minseqlength=0))


def format_sets():
    rng = random.Random(53)
    a, b = random_seq(rng, 81), random_seq(rng, 80)
    c = random_seq(rng, 170)
    seqs = [a, b, c, a, c, c]
    labels = ["one;size=4", "two", "three;", "four", "five", "six"]
    out = [_set("format_relabel_sizeout", "derep_fulllength", seqs, labels, fmt=dict(relabel="Uniq", sizeout=True)),
           _set("format_sizeout", "derep_fulllength", seqs, labels, fmt=dict(sizeout=True)),
           _set("format_xsize", "derep_fulllength", seqs, labels, fmt=dict(xsize=True)),
           _set("format_width0", "derep_fulllength", seqs, labels, fmt=dict(fasta_width=0)),
           _set("format_width80", "derep_fulllength", seqs, labels),
           _set("format_width60", "derep_fulllength", seqs, labels, fmt=dict(fasta_width=60))]
    return out


def derep_id_set():
    rng = random.Random(59)
    a, b = random_seq(rng, 34), random_seq(rng, 34)
    seqs = [a, a, b, a, revcomp(b), b, revcomp(a)]
    labels = ["x", "y", "x", "x", "x", "y", "y"]
    return [_set("derep_id", "derep_id", seqs, labels, opts=dict(strand_both=1)),
            _set("derep_id_plus", "derep_id", seqs, labels)]


def _qual(rng, n, lo=33, hi=73):
    return "".join(chr(rng.randint(lo, hi)) for _ in range(n))


def fastq_sets():
    """the worked quality example, random qualities in both modes, minus-strand members (their strings are applied unreversed),
    the 0.75 branch ('!' and '"'), another offset with clamped output"""
    rng = random.Random(61)
    w = "ACGTACGTAC"
    worked = dict(seqs=[w, w, w, "GGGGGGGGGG"], labels=["w0", "w1", "w2", "w3"], quals=["IIIII#####", "5555555555", "!!!!!IIIII", "ABCDEFGHIJ"])
    a, b = random_seq(rng, 30), random_seq(rng, 45)
    seqs = [a, b, revcomp(a), a, revcomp(b), b, revcomp(a), random_seq(rng, 30)]
    labels = [f"q{k};size={rng.randint(1, 20)}" for k in range(len(seqs))]
    quals = [_qual(rng, len(x)) for x in seqs]
    low = ["!\"#$%&!\"!\"" * 3, "\"!\"!!!\"\"#I" * 3, "!!!!!!!!!!" * 3]
    out = []
    for mode in (0, 1):
        tag = "max" if mode else "avg"
        out.append(_set(f"fastq_worked_{tag}", "fastx_uniques", worked["seqs"], worked["labels"], worked["quals"], opts=dict(qout_max=mode)))
        out.append(_set(f"fastq_minus_{tag}", "fastx_uniques", seqs, labels, quals, opts=dict(qout_max=mode, strand_both=1, sizein=1),
                        fmt=dict(sizeout=True)))
        out.append(_set(f"fastq_low_{tag}", "fastx_uniques", [a, a, a], None, low, opts=dict(qout_max=mode)))
        q64 = [_qual(rng, len(x), 64, 64 + 41) for x in seqs]
        out.append(_set(f"fastq_ascii64_{tag}", "fastx_uniques", seqs, labels, q64,
                        opts=dict(qout_max=mode, strand_both=1, ascii=64, asciiout=64, qminout=10, qmaxout=30), fmt=dict(relabel="U")))
    return out


def empty_set():
    return _set("empty", "derep_fulllength", [])


def golden_sets():
    return ([worked_examples(), alphabet_set(), palindromes_set()] + rc_first_set() + ties_set() + sizein_sets()
            + [selection_set(), discards_set(), empty_sequences_set()] + format_sets() + derep_id_set() + fastq_sets() + [empty_set()])


# ---- the device sets -------------------------------------------------------------------------------------------------------------
LENGTHS_DEVICE = (0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 2047, 2048, 2049, 20000)


def lengths_set(seed=67):
    """per length: a sequence twice, its reverse complement, and a pair of duplicates that differ from it only in the last symbol"""
    rng = random.Random(seed)
    seqs = []
    for L in LENGTHS_DEVICE:
        if L == 0:
            seqs += ["", ""]
            continue
        s = random_seq(rng, L)
        other = substitute(s, L - 1)
        seqs += [s, other, revcomp(s), s, other]
    rng.shuffle(seqs)
    return _set("lengths", "fastx_uniques", seqs, opts=dict(strand_both=1, minseqlength=0))


def cluster_sizes_set(seed=71):
    rng = random.Random(seed)
    seqs, quals = [], []
    for members in (1, 2, 63, 64, 65, 1000):
        s = random_seq(rng, 40)
        for _ in range(members):
            seqs.append(s if rng.random() < 0.7 else revcomp(s))
            quals.append(_qual(rng, 40))
    order = list(range(len(seqs)))
    rng.shuffle(order)
    seqs, quals = [seqs[k] for k in order], [quals[k] for k in order]
    labels = [f"m{k};size={rng.randint(1, 50)}" for k in range(len(seqs))]
    return _set("cluster_sizes", "fastx_uniques", seqs, labels, quals, opts=dict(strand_both=1, sizein=1))


def quality_blocks_set(qout_max=0, seed=73):
    rng = random.Random(seed + qout_max)
    seqs, quals = [], []
    for L in (63, 64, 65, 129):
        s = random_seq(rng, L)
        for _ in range(5):
            seqs.append(s)
            quals.append(_qual(rng, L, 33, 126))
    return _set(f"quality_blocks_{qout_max}", "fastx_uniques", seqs, None, quals, opts=dict(qout_max=qout_max, qmaxout=93))


def table_step_set(n, seed=79):
    """n reads, about a third of them duplicates: read counts on both sides of a table-size step (3n > 2 * size)"""
    rng = random.Random(seed * 1009 + n)
    base = [random_seq(rng, rng.randint(20, 44)) for _ in range(max(1, (2 * n) // 3))]
    seqs = [base[k] if k < len(base) else rng.choice(base) for k in range(n)]
    rng.shuffle(seqs)
    return _set(f"table_{n}", "fastx_uniques", seqs, opts=dict(strand_both=1))


def random_set(n=2000, seed=83, fastq=False, qout_max=0):
    """60 % duplicates, 30 % of those reverse-complemented, abundances 1 .. 50"""
    rng = random.Random(seed)
    seqs, quals = [], []
    for _ in range(n):
        if seqs and rng.random() < 0.6:
            s = rng.choice(seqs)
            if rng.random() < 0.3:
                s = revcomp(s)
        else:
            s = random_seq(rng, rng.randint(32, 120))
        seqs.append(s)
        quals.append(_qual(rng, len(s)))
    labels = [f"read{k};size={rng.randint(1, 50)}" for k in range(n)]
    if fastq:
        return _set(f"random_fastq_{qout_max}", "fastx_uniques", seqs, labels, quals, opts=dict(strand_both=1, sizein=1, qout_max=qout_max))
    return _set("random_fasta", "derep_fulllength", seqs, labels, opts=dict(strand_both=1, sizein=1))


def reversed_set(s):
    out = dict(s, name=s["name"] + "_reversed", seqs=s["seqs"][::-1], labels=s["labels"][::-1])
    out["quals"] = s["quals"][::-1] if s.get("quals") is not None else None
    return out


# ---- the reference CLI -----------------------------------------------------------------------------------------------------------
def ref_binary():
    return os.path.join(ROOT, "oracle", "_ref", "vsearch_ref")


LOG_LINE = re.compile(r" nt in \d+ seqs|seqlength -?\d+: |unique sequences|uniques written")


def run_reference(s):
    """-> dict(fasta, uc, log[, fastq, tabbed]) of the reference CLI with one thread"""
    o, f = full_opts(s), full_fmt(s)
    fastq = s.get("quals") is not None
    with tempfile.TemporaryDirectory(prefix="vsx_derep_") as tmp:
        p = lambda n: os.path.join(tmp, n)  # noqa: E731
        with open(p("in"), "w") as fh:
            for k, seq in enumerate(s["seqs"]):
                fh.write(f"@{s['labels'][k]}\n{seq}\n+\n{s['quals'][k]}\n" if fastq else f">{s['labels'][k]}\n{seq}\n")
        args = [ref_binary(), "--" + s["cmd"], p("in"), "--uc", p("o.uc"), "--log", p("log.txt"), "--quiet", "--threads", "1",
                "--fasta_width", str(f["fasta_width"]), "--strand", "both" if o["strand_both"] else "plus",
                "--minseqlength", str(o["minseqlength"]), "--maxseqlength", str(o["maxseqlength"]),
                "--minuniquesize", str(o["minuniquesize"])]
        args += ["--fastaout" if s["cmd"] == "fastx_uniques" else "--output", p("o.fa")]
        if o["maxuniquesize"] != INT64_MAX:
            args += ["--maxuniquesize", str(o["maxuniquesize"])]
        if o["topn"] != INT64_MAX:
            args += ["--topn", str(o["topn"])]
        if o["sizein"]:
            args.append("--sizein")
        if f["sizeout"]:
            args.append("--sizeout")
        if f["xsize"]:
            args.append("--xsize")
        if f["relabel"] is not None:
            args += ["--relabel", f["relabel"]]
        if fastq:
            args += ["--fastqout", p("o.fq"), "--tabbedout", p("o.tsv"), "--fastq_ascii", str(o["ascii"]), "--fastq_asciiout", str(o["asciiout"]),
                     "--fastq_qminout", str(o["qminout"]), "--fastq_qmaxout", str(o["qmaxout"]), "--fastq_qmax", str(126 - o["ascii"])]
            if o["qout_max"]:
                args.append("--fastq_qout_max")
        r = subprocess.run(args, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{s['name']}: reference CLI failed: {r.stderr[-2000:]}")
        read = lambda n: open(p(n)).read().splitlines()  # noqa: E731
        out = dict(fasta=read("o.fa"), uc=read("o.uc"), log=[l for l in read("log.txt") if LOG_LINE.search(l)])
        if fastq:
            out["fastq"], out["tabbed"] = read("o.fq"), read("o.tsv")
        return out


INPUT_KEYS = ("name", "cmd", "seqs", "labels", "quals", "opts", "fmt")


def write_golden(path=GOLDEN):
    sets = []
    for s in golden_sets():
        rec = {k: s[k] for k in INPUT_KEYS}
        rec["ref"] = run_reference(s)
        sets.append(rec)
    with open(path, "w") as f:
        json.dump(dict(sets=sets), f, indent=0, separators=(",", ":"))
        f.write("\n")
    return sets


def load_golden(path=GOLDEN):
    with open(path) as f:
        return json.load(f)["sets"]


if __name__ == "__main__":
    for rec in write_golden():
        print(f"{rec['name']}: {len(rec['seqs'])} reads, {len(rec['ref']['uc'])} uc lines, log {rec['ref']['log']}")
