"""Inputs, a plain-Python restatement and the reference-CLI runner for the prefix-dereplication tests (--derep_prefix).

    py_derep_prefix() the reference's LITERAL loop (commands/derep_prefix.cpp): sort (length, annotation, label, input order), walk
                      with a dictionary of live buckets -- exact match, else the longest live proper prefix, which is deleted and
                      whose members follow the newcomer, else a new bucket -- then the qsort order.  Not the one-pass rule.
    *_set()           input builders, one per case the command can reach; and the device sets (table steps, seeded reads)
    run_reference()   the reference CLI (oracle/_ref/vsearch_ref) on one set: --output, --uc, --log
    __main__          writes tests/golden/derep_prefix_golden.json: the sets' inputs and the reference's recorded lines
"""
import json
import os
import random
import re
import subprocess
import tempfile

from tests.derep_data import abundances
from tests.search_exact_data import IUPAC, norm, random_seq, substitute

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "derep_prefix_golden.json")
INT64_MAX = (1 << 63) - 1

DEFAULT_OPTS = dict(sizein=0, minseqlength=32, maxseqlength=50000, minuniquesize=1, maxuniquesize=INT64_MAX, topn=INT64_MAX)
DEFAULT_FMT = dict(sizeout=False, relabel=None, xsize=False, fasta_width=80)


def full_opts(s):
    return dict(DEFAULT_OPTS, **(s.get("opts") or {}))


def full_fmt(s):
    return dict(DEFAULT_FMT, **(s.get("fmt") or {}))


# ---- the plain-Python restatement: the loop ---------------------------------------------------------------------------------------
def py_derep_prefix(s):
    """-> dict(clusters=[dict(rep, size, count, members)] in output order, counts=the log lines' figures, rank=per read or None)"""
    o = full_opts(s)
    seqs, labels = s["seqs"], s["labels"]
    annotation = abundances(labels)
    counts = dict(kept=0, nucleotides=0, shortest=0, longest=0, discarded_short=0, discarded_long=0, sumsize=0, maxsize=0)
    kept = []
    for k, seq in enumerate(seqs):
        if len(seq) < o["minseqlength"]:
            counts["discarded_short"] += 1
        elif len(seq) > o["maxseqlength"]:
            counts["discarded_long"] += 1
        else:
            kept.append(k)
    counts["kept"] = len(kept)
    counts["nucleotides"] = sum(len(seqs[k]) for k in kept)
    counts["shortest"] = min((len(seqs[k]) for k in kept), default=0)
    counts["longest"] = max((len(seqs[k]) for k in kept), default=0)
    # strcmp: bytes compare as unsigned characters
    kept.sort(key=lambda k: (len(seqs[k]), -annotation[k], labels[k].encode("latin-1"), k))
    rank = [None] * len(seqs)
    for r, k in enumerate(kept):
        rank[k] = r
    live, shortest = {}, counts["shortest"]
    for k in kept:
        text = norm(seqs[k])
        ab = annotation[k] if o["sizein"] else 1
        counts["sumsize"] += ab
        b = live.get(text)
        if b is not None:                                                    # exact match
            b["size"] += ab
            b["members"].append(k)
            continue
        found = None
        for plen in range(len(text) - 1, shortest - 1, -1):                  # the longest live proper prefix
            found = live.get(text[:plen])
            if found is not None:
                del live[text[:plen]]                                        # marked deleted
                break
        if found is not None:
            live[text] = dict(first=k, size=found["size"] + ab, members=[k] + found["members"])
        else:
            live[text] = dict(first=k, size=ab, members=[k])
    clusters = sorted(live.values(), key=lambda b: (-b["size"], labels[b["first"]].encode("latin-1"), rank[b["first"]]))
    clusters = [dict(rep=b["first"], size=b["size"], count=len(b["members"]), members=b["members"]) for b in clusters]
    n = len(clusters)
    counts["maxsize"] = max((c["size"] for c in clusters), default=0)
    if n == 0:
        counts["median"] = 0.0
    elif n % 2:
        counts["median"] = float(clusters[(n - 1) // 2]["size"])
    else:
        counts["median"] = (clusters[n // 2 - 1]["size"] + clusters[n // 2]["size"]) / 2.0
    in_range = sum(1 for c in clusters if o["minuniquesize"] <= c["size"] <= o["maxuniquesize"])
    counts["selected"] = min(in_range, o["topn"])
    return dict(clusters=clusters, counts=counts, rank=rank)


def result_fields(res):
    """a DerepPrefixResult in py_derep_prefix's shape"""
    from vsearch_amd.derep_prefix import UNRANKED
    clusters = [dict(rep=int(res.rep[c]), size=int(res.size[c]), count=int(res.count[c]), members=[int(m) for m in res.members(c)])
                for c in range(len(res))]
    return dict(clusters=clusters, counts=dict(res.counts), rank=[None if int(r) == UNRANKED else int(r) for r in res.rank])


def call(aligner, s, **extra):
    """the set through the package's entry point"""
    from vsearch_amd import derep_prefix
    kw = full_opts(s)
    kw.update(extra)
    return derep_prefix(aligner, s["seqs"], s["labels"], sizes=abundances(s["labels"]), **kw)


def formatted(res, s):
    """the formatters' text in the shape run_reference records"""
    import importlib
    dp = importlib.import_module("vsearch_amd.derep_prefix")
    return dict(fasta=dp.fasta_lines(res, **full_fmt(s)), uc=dp.uc_lines(res), log=dp.log_lines(res))


# ---- input builders --------------------------------------------------------------------------------------------------------------
def _set(name, seqs, labels=None, opts=None, fmt=None):
    return dict(name=name, seqs=list(seqs), labels=list(labels) if labels else [f"r{k}" for k in range(len(seqs))], opts=opts or {},
                fmt=fmt or {})


def _other(c):
    return "ACGT"["ACGT".index(c) ^ 1] if c in "ACGT" else "A"


def ladder_set():
    """every prefix of one 300-symbol sequence, duplicates at several levels, shuffled: one cluster"""
    rng = random.Random(101)
    base = random_seq(rng, 300)
    seqs = [base[:n] for n in range(1, 301)]
    for n, copies in ((1, 2), (16, 1), (17, 3), (150, 2), (299, 1), (300, 2)):
        seqs += [base[:n]] * copies
    rng.shuffle(seqs)
    return _set("ladder", seqs, opts=dict(minseqlength=1))


def winners_set():
    """an item with two extenders, four times: the winner decided by length, by abundance, by label, by input position"""
    rng = random.Random(103)
    p = [random_seq(rng, 40) for _ in range(4)]
    seqs = [p[0] + "CC", p[0], p[0] + "A",
            p[1] + "A", p[1] + "C", p[1],
            p[2] + "A", p[2], p[2] + "C",
            p[3] + "G", p[3] + "T", p[3]]
    labels = ["len_long", "len_item", "len_short",
              "ab_a;size=2", "ab_c;size=5", "ab_item",
              "lab_zz", "lab_item", "lab_aa",
              "pos", "pos", "pos_item"]
    return _set("winners", seqs, labels)


def thousand_extenders_set():
    """an item with 1 000 extenders of one length and abundance: the smallest label wins, 999 found clusters of their own"""
    rng = random.Random(107)
    item = random_seq(rng, 12)
    tails = rng.sample(range(1024), 1000)
    seqs = [item] + [item + "".join("ACGT"[(t >> (2 * i)) & 3] for i in range(5)) for t in tails]
    names = [f"e{k:04d}" for k in range(1000)]
    rng.shuffle(names)
    return _set("thousand_extenders", seqs, ["item"] + names, opts=dict(minseqlength=1, topn=3))


def absorbed_set():
    """P, X = P + A absorbs P; Y = P + CG extends only the absorbed P and must not join; Z = X + T joins the chain"""
    rng = random.Random(109)
    p = random_seq(rng, 36)
    return _set("absorbed", [p + "CG", p + "AT", p, p + "A"], ["y", "z", "p", "x"])


def boundary_lengths_set():
    """chains (l - 1, l, l + 1) for l = 16, 32, 1 024: lengths 15 / 16 / 17, 31 / 32 / 33 and 1 023 / 1 024 / 1 025 each as the prefix and
    as the extender by one symbol; beside every chain a read that differs from its longest in the last symbol only"""
    rng = random.Random(113)
    seqs = []
    for l in (16, 32, 1024):
        base = random_seq(rng, l + 1)
        seqs += [base[:l + 1], base[:l - 1], base[:l], substitute(base, l)]
        other = random_seq(rng, l + 1)
        seqs += [other[:l], substitute(other[:l + 1], l - 1)]               # differs in the prefix's last symbol: no join
    return _set("boundary_lengths", seqs, opts=dict(minseqlength=1))


def near_misses_set():
    """per prefix length 32, 33, 40: a candidate that differs from the true prefix only in the prefix's last symbol, and two that
    differ only in the symbol after the prefix's end (both extend it: the lower rank takes it)"""
    rng = random.Random(127)
    seqs, labels = [], []
    for l in (32, 33, 40):
        p, tail = random_seq(rng, l), random_seq(rng, 9)
        seqs += [p[:-1] + _other(p[-1]) + tail, p + "G" + tail, p, p + "T" + tail]
        labels += [f"miss{l}", f"after_g{l}", f"item{l}", f"after_t{l}"]
    return _set("near_misses", seqs, labels)


def candidate_lengths_set():
    """63, 64 and 65 distinct candidate lengths below one node"""
    rng = random.Random(131)
    seqs = []
    for n in (63, 64, 65):
        base = random_seq(rng, 32 + n)
        seqs += [base[:32 + k] for k in range(n + 1)]
    rng.shuffle(seqs)
    return _set("candidate_lengths", seqs)


def alphabet_set():
    """U = T, lower case, every ambiguity code against itself, N against A"""
    frame = "GATTACA{}CATTAGGCGATTACATTGACCAGTAGGCA"
    seqs = []
    for c in IUPAC:
        seqs += [frame.format(c), frame.format(c.lower()).lower() + "acgu", frame.format(c) + "ACGTA"]
    seqs += [frame.format("N") + "GG", frame.format("A") + "GGC", frame.format("T") + "CC", frame.format("U").replace("T", "u") + "CCA"]
    return _set("alphabet", seqs)


def sizein_sets():
    """the annotation is a key of the sort with and without --sizein (the extender of size 9 wins); without annotations the label
    decides and another extender wins; the sums follow --sizein alone"""
    rng = random.Random(137)
    p = random_seq(rng, 34)
    seqs = [p + "A", p, p + "C", p, p + "C"]
    labels = ["a_ext;size=2", "item;size=3", "c_ext;size=9", "item2", "c_dup;size=4;"]
    plain = ["a_ext", "item", "c_ext", "item2", "c_dup"]
    return [_set("sizein", seqs, labels, opts=dict(sizein=1), fmt=dict(sizeout=True)),
            _set("sizein_ignored", seqs, labels, fmt=dict(sizeout=True)),
            _set("sizein_no_annotations", seqs, plain, opts=dict(sizein=1), fmt=dict(sizeout=True))]


def cluster_order_set():
    """two clusters of one size and label: the shorter representative comes first in the sorted order and last in the input"""
    rng = random.Random(139)
    return _set("cluster_order", [random_seq(rng, 50), random_seq(rng, 40)], ["same", "same"])


def selection_set():
    """minuniquesize, maxuniquesize and topn over clusters of 1 .. 7 members (truncated copies among them); eight clusters of sizes
    1 .. 8: the median is 4.5"""
    rng = random.Random(149)
    seqs = []
    for k in range(8):
        b = random_seq(rng, 45)
        seqs += [b] + [b[:45 - m] for m in range(1, k + 1)]
    rng.shuffle(seqs)
    return _set("selection", seqs, opts=dict(minuniquesize=2, maxuniquesize=6, topn=3))


def one_symbol_set():
    return _set("one_symbol", ["A", "a", "C", "AC", "ACG", "G", "N", "u", "T", "GN"], opts=dict(minseqlength=1))


def discards_set():
    rng = random.Random(157)
    b = random_seq(rng, 61)
    return _set("discards", [b[:31], b[:32], b[:60], b, random_seq(rng, 5), b[:33]], opts=dict(maxseqlength=60))


def all_discarded_set():
    return _set("all_discarded", ["ACGT", "ACGTACGT"])


def empty_set():
    return _set("empty", [])


def sum_limit_set():
    """a total abundance of 2^32 - 1 is served"""
    rng = random.Random(163)
    a = random_seq(rng, 33)
    return _set("sum_limit", [a, a[:32]], ["big;size=4294967294", "one;size=1"], opts=dict(sizein=1), fmt=dict(sizeout=True))


def format_sets():
    rng = random.Random(167)
    a, c = random_seq(rng, 81), random_seq(rng, 170)
    seqs = [a, c[:100], c, a[:80], c, c[:161]]
    labels = ["one;size=4", "two", "three;", "four", "five", "six"]
    return [_set("format_relabel_sizeout", seqs, labels, fmt=dict(relabel="Uniq", sizeout=True)),
            _set("format_xsize", seqs, labels, fmt=dict(xsize=True)),
            _set("format_width0", seqs, labels, fmt=dict(fasta_width=0)),
            _set("format_width60", seqs, labels, fmt=dict(fasta_width=60))]


def golden_sets():
    return ([ladder_set(), winners_set(), thousand_extenders_set(), absorbed_set(), boundary_lengths_set(), near_misses_set(),
             candidate_lengths_set(), alphabet_set()] + sizein_sets()
            + [cluster_order_set(), selection_set(), one_symbol_set(), discards_set(), all_discarded_set(), empty_set(),
               sum_limit_set()] + format_sets())


# ---- the device sets and the seeded sets ---------------------------------------------------------------------------------------------
def nested_random_set(seed):
    """a small set over a two-letter alphabet with heavy nesting: 1 .. 14 reads of 1 .. 7 symbols, labels and annotations that tie"""
    rng = random.Random(seed)
    n = rng.randint(1, 14)
    seqs = ["".join(rng.choice("AC") for _ in range(rng.randint(1, 7))) for _ in range(n)]
    labels = [rng.choice("abc") + (f";size={rng.randint(1, 3)}" if rng.random() < 0.5 else "") for _ in range(n)]
    return _set(f"nested_{seed}", seqs, labels, opts=dict(minseqlength=1, sizein=seed & 1))


def large_nested_set(n=40000, seed=181):
    """40 000 reads of 1 .. 14 symbols over two letters, three labels, annotations 1 .. 3: every key of the sort ties thousands of
    times, and the input is large enough for the library to sort it in slices"""
    rng = random.Random(seed)
    seqs = ["".join(rng.choice("AC") for _ in range(rng.randint(1, 14))) for _ in range(n)]
    labels = [rng.choice("abc") + f";size={rng.randint(1, 3)}" for _ in range(n)]
    return _set("large_nested", seqs, labels, opts=dict(minseqlength=1, sizein=1))


def table_step_set(n, seed=173):
    """n reads, half of them truncated copies of others: read counts on both sides of a table-size step (3 n > 2 * size)"""
    rng = random.Random(seed * 1009 + n)
    base = [random_seq(rng, rng.randint(36, 60)) for _ in range(max(1, n // 2))]
    seqs = []
    for k in range(n):
        b = base[k] if k < len(base) else rng.choice(base)
        seqs.append(b if k < len(base) else b[:rng.randint(32, len(b))])
    rng.shuffle(seqs)
    return _set(f"table_{n}", seqs)


def random_set(n=2000, seed=179):
    """2 000 reads of 32 .. 120 symbols: 60 % are copies of earlier reads, two thirds of those cut at a random length; annotations
    1 .. 50, summed"""
    rng = random.Random(seed)
    seqs = []
    for _ in range(n):
        if seqs and rng.random() < 0.6:
            s = rng.choice(seqs)
            if rng.random() < 0.67:
                s = s[:rng.randint(32, len(s))]
        else:
            s = random_seq(rng, rng.randint(32, 120))
        seqs.append(s)
    labels = [f"read{k};size={rng.randint(1, 50)}" for k in range(n)]
    return _set("random", seqs, labels, opts=dict(sizein=1), fmt=dict(sizeout=True))


def reversed_set(s):
    return dict(s, name=s["name"] + "_reversed", seqs=s["seqs"][::-1], labels=s["labels"][::-1])


# ---- the reference CLI -----------------------------------------------------------------------------------------------------------
def ref_binary():
    return os.path.join(ROOT, "oracle", "_ref", "vsearch_ref")


LOG_LINE = re.compile(r" nt in \d+ seqs|seqlength -?\d+: |unique sequences|uniques written")


def run_reference(s):
    """-> dict(fasta, uc, log) of the reference CLI with one thread"""
    o, f = full_opts(s), full_fmt(s)
    with tempfile.TemporaryDirectory(prefix="vsx_derep_prefix_") as tmp:
        p = lambda n: os.path.join(tmp, n)  # noqa: E731
        with open(p("in"), "w") as fh:
            for k, seq in enumerate(s["seqs"]):
                fh.write(f">{s['labels'][k]}\n{seq}\n")
        args = [ref_binary(), "--derep_prefix", p("in"), "--output", p("o.fa"), "--uc", p("o.uc"), "--log", p("log.txt"), "--quiet",
                "--threads", "1", "--fasta_width", str(f["fasta_width"]), "--minseqlength", str(o["minseqlength"]),
                "--maxseqlength", str(o["maxseqlength"]), "--minuniquesize", str(o["minuniquesize"])]
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
        r = subprocess.run(args, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{s['name']}: reference CLI failed: {r.stderr[-2000:]}")
        read = lambda n: open(p(n)).read().splitlines()  # noqa: E731
        return dict(fasta=read("o.fa"), uc=read("o.uc"), log=[l for l in read("log.txt") if LOG_LINE.search(l)])


INPUT_KEYS = ("name", "seqs", "labels", "opts", "fmt")


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
