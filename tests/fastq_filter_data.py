"""Inputs for the read-filter tests and bench_filter.py, a plain-Python restatement of the reference's `analyse`
(py_analyse: a second checker beside the library's host restatement, which also names the cause of every discard and of
every truncation), and a runner of the reference CLI's --fastq_filter / --fastx_filter (oracle/_ref/vsearch_ref) that
returns its outputs as lists of lines.

A "set" is one run of the command: {"name", "opts", "labels", "seqs", "quals" (None: FASTA input), optionally "sizes",
"rev_seqs", "rev_quals", "rev_sizes"}.  Labels of reads with an abundance carry it as ;size=N (the runner passes --sizein).
"""
import math
import os
import re
import subprocess
import tempfile

import numpy as np

LONG_MIN = -2 ** 63
INT64_MAX = 2 ** 63 - 1
DBL_MAX = float.fromhex("0x1.fffffffffffffp+1023")

# the reference's defaults (src/vsearch.h)
DEFAULTS = {"ascii": 33, "qmin": 0, "qmax": 41, "stripleft": 0, "stripright": 0, "trunclen": -1, "trunclen_keep": -1,
            "truncqual": LONG_MIN, "minqual": 0, "minlen": 1, "maxlen": INT64_MAX, "maxns": INT64_MAX, "minsize": 0,
            "maxsize": INT64_MAX, "maxee": DBL_MAX, "maxee_rate": DBL_MAX, "truncee": DBL_MAX, "truncee_rate": DBL_MAX}

CLI_FLAGS = {"ascii": "--fastq_ascii", "qmin": "--fastq_qmin", "qmax": "--fastq_qmax", "stripleft": "--fastq_stripleft",
             "stripright": "--fastq_stripright", "trunclen": "--fastq_trunclen", "trunclen_keep": "--fastq_trunclen_keep",
             "truncqual": "--fastq_truncqual", "minqual": "--fastq_minqual", "minlen": "--fastq_minlen", "maxlen": "--fastq_maxlen",
             "maxns": "--fastq_maxns", "minsize": "--minsize", "maxsize": "--maxsize", "maxee": "--fastq_maxee",
             "maxee_rate": "--fastq_maxee_rate", "truncee": "--fastq_truncee", "truncee_rate": "--fastq_truncee_rate"}

DISCARD_CAUSES = ("maxee", "maxee_rate", "minqual", "shorter_than_trunclen", "minlen", "maxlen", "maxns", "minsize", "maxsize",
                  "reverse_only")
TRUNCATION_CAUSES = ("stripleft", "stripright", "trunclen", "trunclen_keep", "truncqual", "truncee", "truncee_rate")


class QualityError(Exception):
    """what the reference exits with: kind 'below qmin' / 'above qmax', the value, the bound"""

    def __init__(self, kind, value, bound):
        super().__init__(f"FASTQ quality value ({value}) {kind} ({bound})")
        self.kind, self.value, self.bound = kind, value, bound


def py_analyse(seq, qual, opts=None, size=1):
    """Steps 1-7 of the command's per-read analysis.  qual None: FASTA input.  -> dict(start, length, ee, discarded, truncated,
    discard_causes, truncation_causes); raises QualityError where the reference exits."""
    o = dict(DEFAULTS, **(opts or {}))
    full = len(seq)
    start, length = 0, full
    cut, why = set(), set()
    if o["stripleft"] < length:
        start += o["stripleft"]
        length -= o["stripleft"]
        if o["stripleft"] > 0:
            cut.add("stripleft")
    else:
        if length > 0:
            cut.add("stripleft")
        start, length = length, 0
    if o["stripright"] < length:
        length -= o["stripright"]
        if o["stripright"] > 0:
            cut.add("stripright")
    else:
        if length > 0:
            cut.add("stripright")
        length = 0
    if 0 <= o["trunclen"] < length:
        length = o["trunclen"]
        cut.add("trunclen")
    if 0 <= o["trunclen_keep"] < length:
        length = o["trunclen_keep"]
        cut.add("trunclen_keep")
    ee = -1.0
    if qual is not None:
        ee = 0.0
        for i in range(length):
            c = ord(qual[start + i]) if isinstance(qual, str) else qual[start + i]
            q = (c - 256 if c > 127 else c) - o["ascii"]
            if q < o["qmin"]:
                raise QualityError("below qmin", q, o["qmin"])
            if q > o["qmax"]:
                raise QualityError("above qmax", q, o["qmax"])
            e = math.pow(10.0, -q / 10.0)
            ee += e
            stops = {name for name, hit in (("truncqual", q <= o["truncqual"]), ("truncee", ee > o["truncee"]),
                                            ("truncee_rate", ee > o["truncee_rate"] * (i + 1))) if hit}
            if stops:
                ee -= e
                length = i
                cut |= stops
                break
            if q < o["minqual"]:
                why.add("minqual")
        if ee > o["maxee"]:
            why.add("maxee")
        if length > 0 and ee / length > o["maxee_rate"]:
            why.add("maxee_rate")
    if o["trunclen"] >= 0 and length < o["trunclen"]:
        why.add("shorter_than_trunclen")
    if length < o["minlen"]:
        why.add("minlen")
    if length > o["maxlen"]:
        why.add("maxlen")
    text = seq if isinstance(seq, str) else bytes(seq).decode("latin-1")
    if sum(c in "Nn" for c in text[start:start + length]) > o["maxns"]:
        why.add("maxns")
    if size < o["minsize"]:
        why.add("minsize")
    if size > o["maxsize"]:
        why.add("maxsize")
    return {"start": start, "length": length, "ee": ee, "discarded": bool(why), "truncated": length < full,
            "discard_causes": why, "truncation_causes": cut}


def py_filter(s):
    """py_analyse over a set -> dict(fwd, rev (or None): lists of py_analyse results, pair_discarded, counts, discard_causes,
    truncation_causes: the causes that occur in the set ('reverse_only': a pair whose forward read alone would be kept))"""
    n = len(s["seqs"])
    sizes, rsizes = s.get("sizes") or [1] * n, s.get("rev_sizes") or [1] * n
    quals = s["quals"] or [None] * n
    paired = s.get("rev_seqs") is not None
    rquals = (s["rev_quals"] or [None] * n) if paired else None
    fwd, rev = [], [] if paired else None
    for k in range(n):                                   # the reference's order: read k forward, read k reverse
        fwd.append(py_analyse(s["seqs"][k], quals[k], s["opts"], sizes[k]))
        if paired:
            rev.append(py_analyse(s["rev_seqs"][k], rquals[k], s["opts"], rsizes[k]))
    verdict = [fwd[k]["discarded"] or bool(rev and rev[k]["discarded"]) for k in range(n)]
    trunc = [fwd[k]["truncated"] or bool(rev and rev[k]["truncated"]) for k in range(n)]
    why, cut = set(), set()
    for side in (fwd, rev or []):
        for r in side:
            why |= r["discard_causes"]
            cut |= r["truncation_causes"]
    if rev and any(rev[k]["discarded"] and not fwd[k]["discarded"] for k in range(n)):
        why.add("reverse_only")
    counts = {"kept": verdict.count(False), "truncated": sum(t and not v for t, v in zip(trunc, verdict)),
              "discarded": verdict.count(True)}
    return {"fwd": fwd, "rev": rev, "pair_discarded": verdict, "counts": counts, "discard_causes": why, "truncation_causes": cut}


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _qual(rng, n, lo=20, hi=41, ascii=33):
    return "".join(chr(ascii + int(q)) for q in rng.integers(lo, hi + 1, n))


def _put(s, pos, ch):
    return s[:pos] + ch + s[pos + 1:]


def _set(name, opts, reads, **more):
    """reads: (label, seq, qual) or (label, seq, qual, size)"""
    s = {"name": name, "opts": opts, "labels": [r[0] for r in reads], "seqs": [r[1] for r in reads], "quals": [r[2] for r in reads]}
    if any(len(r) > 3 for r in reads):
        s["sizes"] = [r[3] if len(r) > 3 else 1 for r in reads]
        s["labels"] = [f"{lab};size={n}" for lab, n in zip(s["labels"], s["sizes"])]
    s.update(more)
    return s


EDGE_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 300)
STOP_POINTS = (0, 63, 64, 65)        # and the last position of each read


def edge_reads():
    """-> list of sets at the edges of the analysis and of the kernel's 64-position chunks (the docstring of each group below says
    what it holds; tests/test_fastq_filter_host.py asserts the properties with py_analyse)"""
    rng = np.random.default_rng(606)
    sets = []
    Q = lambda n: _qual(rng, n)          # noqa: E731
    S = lambda n: _seq(rng, n)           # noqa: E731

    # every length at the defaults (the empty read is discarded by minlen 1), and with expected-error filters on
    reads = [(f"len{n}", S(n), Q(n)) for n in EDGE_LENGTHS]
    sets.append(_set("lengths", {}, reads))
    sets.append(_set("lengths_maxee", {"maxee": 0.25, "maxee_rate": 0.002}, reads))

    # a stop by truncqual at 0, 63, 64, 65 and at the last position, a second low quality and an out-of-range symbol behind it
    reads = []
    for n in (66, 128, 129, 300):
        for p in STOP_POINTS + (n - 1,):
            q = _put(Q(n), p, "#")
            for at, ch in ((p + 2, "#"), (p + 3, "K")):
                if at < n:
                    q = _put(q, at, ch)
            reads.append((f"tq{n}_{p}", S(n), q))
    sets.append(_set("truncqual", {"truncqual": 2}, reads))

    # truncee 0.645 over Q20 (0.01 each) stops at 64; an early Q17 moves the stop to 63 and before, an early Q30 to 65 and behind
    reads = [("te_q20", S(200), "5" * 200)]
    for k, sym in enumerate("2222????"):
        reads.append((f"te_{k}", S(200), _put("5" * 200, 3 + k, sym) if k % 2 else _put(_put("5" * 200, 3, sym), 9 + k, sym)))
    reads += [("te_short", S(40), "5" * 40), ("te_none", S(120), "I" * 120), ("te_first", S(10), "!" + "I" * 9)]
    sets.append(_set("truncee", {"truncee": 0.645}, reads))

    # truncee_rate 0.004: k symbols of Q30 (0.001), then Q10 (0.1) until the mean passes the rate, k around the chunk edge
    reads = [(f"tr_{k}", S(140), "?" * k + "+" * (140 - k)) for k in (30, 59, 60, 61, 62, 63, 64, 65, 66, 67, 95, 126, 127, 128)]
    reads += [(f"tr20_{k}", S(140), "?" * k + "5" + "+" * (139 - k)) for k in (62, 63)]       # (one Q20 between: stops at 64 and 65)
    reads += [("tr_first", S(30), "+" * 30), ("tr_none", S(130), "I" * 130)]
    sets.append(_set("truncee_rate", {"truncee_rate": 0.004}, reads))

    # strip / truncate by 20: reads of 19, 20, 21 (the option is len + 1, len, len - 1), 0, 1 and 100
    reads = [(f"n{n}", S(n), Q(n)) for n in (0, 1, 19, 20, 21, 100)]
    for opt in ("stripleft", "stripright", "trunclen", "trunclen_keep"):
        sets.append(_set(opt, {opt: 20}, reads))
    sets.append(_set("strip_both", {"stripleft": 20, "stripright": 20, "minlen": 2}, reads + [(f"m{n}", S(n), Q(n)) for n in (39, 40, 41, 42)]))

    # N / n counts at maxns - 1, maxns, maxns + 1 inside [5, 35), with more Ns in the stripped-off and the truncated-off parts
    reads = []
    for count in (1, 2, 3):
        for tag, outside in (("in", ()), ("out", (0, 2, 4, 35, 36, 59))):
            s = S(60)
            for j in range(count):
                s = _put(s, (5, 19, 34)[j], "Nn"[j % 2])
            for p in outside:
                s = _put(s, p, "Nn"[p % 2])
            reads.append((f"ns{count}_{tag}", s, Q(60)))
    reads.append(("ns_edges", _put(_put(_put(_put(S(60), 4, "N"), 5, "N"), 34, "n"), 35, "N"), Q(60)))
    sets.append(_set("maxns", {"maxns": 2, "stripleft": 5, "trunclen_keep": 30}, reads))

    # minqual 10 with truncqual 2: a Q5 before the stop discards; at the stop (the Q2 itself) and behind it, it does not
    base = "I" * 100
    reads = [("mq_before", S(100), _put(_put(base, 70, "#"), 20, "&")), ("mq_at", S(100), _put(base, 70, "#")),
             ("mq_after", S(100), _put(_put(base, 70, "#"), 80, "&")), ("mq_none", S(100), base),
             ("mq_no_stop", S(100), _put(base, 64, "&")), ("mq_63", S(100), _put(_put(base, 64, "#"), 63, "&")),
             ("mq_chunk2", S(200), _put(_put("I" * 200, 190, "#"), 130, "&"))]
    sets.append(_set("minqual", {"minqual": 10, "truncqual": 2}, reads))

    # length filters and abundances at the bounds and one beyond
    sets.append(_set("minlen_maxlen", {"minlen": 10, "maxlen": 100}, [(f"l{n}", S(n), Q(n)) for n in (9, 10, 100, 101)]))
    sets.append(_set("sizes", {"minsize": 2, "maxsize": 10}, [(f"s{n}", S(30), Q(30), n) for n in (1, 2, 10, 11)]))

    # pairs: each verdict combination, truncation on either side, a pair discarded by its reverse read only
    f = [("p_keep", S(80), "I" * 80), ("p_fwd_bad", S(80), "+" * 80), ("p_rev_bad", S(80), "I" * 80), ("p_both_bad", S(80), "+" * 80),
         ("p_fwd_cut", S(80), _put("I" * 80, 64, "#")), ("p_rev_cut", S(80), "I" * 80), ("p_rev_short", S(80), "I" * 80)]
    r = [(S(80), "I" * 80), (S(80), "I" * 80), (S(80), "+" * 80), (S(80), "+" * 80), (S(80), "I" * 80), (S(70), _put("I" * 70, 63, "#")),
         (S(12), "I" * 12)]
    sets.append(_set("pairs", {"maxee": 1.0, "truncqual": 2, "minlen": 20}, f, rev_seqs=[x[0] for x in r], rev_quals=[x[1] for x in r]))
    return sets


def rounding_reads(want=8):
    """-> list of one-read sets where (s + e) - e != s at a truncqual stop (s: the sum before the stop, e: the error of Q2), with
    maxee the smaller of the two sums, so the verdict depends on keeping the reference's two operations: `want` reads where the
    reference discards and a kept-old-sum rule would keep (label up_*), `want` of the reverse (label down_*)."""
    rng = np.random.default_rng(8128)
    e = math.pow(10.0, -2 / 10.0)
    up, down = [], []
    while len(up) < want or len(down) < want:
        n = int(rng.integers(8, 41))
        qual = _qual(rng, n) + "#" + _qual(rng, 5)
        s = 0.0
        for c in qual[:n]:
            s += math.pow(10.0, -(ord(c) - 33) / 10.0)
        t = (s + e) - e
        if t == s:
            continue
        side, tag = (up, "up") if t > s else (down, "down")
        if len(side) < want:
            side.append(_set(f"{tag}_{len(side)}", {"truncqual": 2, "maxee": min(s, t)}, [(f"{tag}_{len(side)}", _seq(rng, n + 6), qual)]))
    return up + down


def quality_cases():
    """-> list of (set, fatal): an out-of-range symbol before the stop and at the stop is the reference's fatal error
    (fatal = (kind, value, bound)); behind the stop or beyond trunclen the run is normal (fatal None).  Offsets 33 and 64."""
    rng = np.random.default_rng(5)
    cases = []
    for ascii in (33, 64):
        hi, lo2, bad_hi = chr(ascii + 40), chr(ascii + 2), chr(ascii + 42)
        base = hi * 100
        common = {"ascii": ascii} if ascii != 33 else {}
        one = lambda name, opts, qual: _set(f"{name}_{ascii}", dict(common, **opts), [("ok", _seq(rng, 100), base), ("probe", _seq(rng, 100), qual)])  # noqa: E731
        cases += [
            (one("above_before_stop", {"truncqual": 2}, _put(_put(base, 70, lo2), 30, bad_hi)), ("above qmax", 42, 41)),
            (one("above_no_stop", {}, _put(base, 99, bad_hi)), ("above qmax", 42, 41)),
            (one("below_at_stop", {"truncqual": 8, "qmin": 5}, _put(base, 64, chr(ascii + 3))), ("below qmin", 3, 5)),
            (one("above_after_stop", {"truncqual": 2}, _put(_put(base, 63, lo2), 64, bad_hi)), None),
            (one("above_beyond_trunclen", {"trunclen": 64}, _put(base, 64, bad_hi)), None),
            (one("above_in_stripped", {"stripleft": 10, "stripright": 10}, _put(_put(base, 9, bad_hi), 90, bad_hi)), None),
            (one("above_after_truncee", {"truncee": 0.5}, _put(_put(base, 10, chr(ascii + 0)), 12, bad_hi)), None),
        ]
    # the first failure in the reference's order: read 0 forward, read 0 reverse, read 1 forward ...
    base = "I" * 80
    pair = _set("pair_order", {}, [("p0", _seq(rng, 80), base), ("p1", _seq(rng, 80), _put(base, 5, "L"))],
                rev_seqs=[_seq(rng, 80), _seq(rng, 80)], rev_quals=[_put(base, 70, "K"), base])
    cases.append((pair, ("above qmax", 42, 41)))
    return cases


def fasta_set():
    """FASTA input through --fastx_filter: no quality walk; a read stripped to length 0, Ns, lengths around the line width"""
    rng = np.random.default_rng(99)
    reads = [(f"fa{n}", _seq(rng, n), None) for n in (5, 6, 7, 85, 86, 165, 166, 200)]
    reads.append(("fa_ns", "ACGTNNnnACGTNACGTACGTACGTACGT", None))
    reads.append(("fa_lower", "acgtacgtacgtnacgtacgtacgtacgtacgt", None))
    s = _set("fasta", {"stripleft": 5, "stripright": 1, "maxns": 2, "maxlen": 159, "trunclen_keep": 190}, reads)
    s["quals"] = None
    return s


def draw_opts(rng, read_len):
    """an option set check_parameters accepts, in ranges where every filter and every truncation has an effect on reads of generate()"""
    o = {}
    pick = lambda p: rng.random() < p      # noqa: E731
    if pick(0.3): o["stripleft"] = int(rng.integers(0, read_len // 4))
    if pick(0.3): o["stripright"] = int(rng.integers(0, read_len // 4))
    if pick(0.3): o["trunclen"] = int(rng.integers(max(1, read_len // 3), read_len + 10))
    if pick(0.2): o["trunclen_keep"] = int(rng.integers(max(1, read_len // 3), read_len + 10))
    if pick(0.5): o["truncqual"] = int(rng.integers(0, 16))
    if pick(0.25): o["minqual"] = int(rng.integers(0, 12))
    if pick(0.4): o["minlen"] = int(rng.integers(1, read_len // 2 + 2))
    if pick(0.3): o["maxlen"] = int(rng.integers(read_len // 2, read_len + 5))
    if pick(0.4): o["maxns"] = int(rng.integers(0, 4))
    if pick(0.5): o["maxee"] = float(np.round(rng.uniform(0.05, 3.0), 3))
    if pick(0.3): o["maxee_rate"] = float(np.round(rng.uniform(0.0005, 0.03), 5))
    if pick(0.3): o["truncee"] = float(np.round(rng.uniform(0.05, 3.0), 3))
    if pick(0.3): o["truncee_rate"] = float(np.round(rng.uniform(0.0005, 0.03), 5))
    if pick(0.25): o["minsize"] = int(rng.integers(1, 4))
    if pick(0.25): o["maxsize"] = int(rng.integers(3, 40))
    return o


def generate(seed, n, read_len=150, paired=False, opts=None, ascii=33, qrange=(0, 41)):
    """-> a set of n seeded random reads (lengths 0 .. read_len, qualities decaying toward the 3' end with dips, Ns, lower case,
    abundances 1 .. 50) with drawn options (draw_opts) unless `opts` is given; qualities inside qrange, written at offset `ascii`
    (the defaults leave every seeded set as it was: the clip to (0, 41) changes nothing and no random number is drawn for it)"""
    rng = np.random.default_rng(seed)

    def side(tag):
        reads = []
        for k in range(n):
            L = int(rng.integers(0, read_len + 1)) if rng.random() < 0.3 else read_len
            start, drop = rng.integers(30, 42), rng.integers(0, 38)
            q = np.clip(np.rint(start - drop * (np.arange(L) / max(L, 1)) ** 2 + rng.normal(0, 3.0, L)), 0, 41).astype(int)
            if L and rng.random() < 0.3:
                q[rng.integers(0, L, rng.integers(1, 4))] = rng.integers(0, 12)
            q = np.clip(q, qrange[0], qrange[1])
            s = _seq(rng, L)
            if L and rng.random() < 0.3:
                for p in rng.integers(0, L, rng.integers(1, 5)):
                    s = _put(s, int(p), "Nn"[int(p) % 2])
            if rng.random() < 0.1:
                s = s.lower()
            reads.append((f"{tag}{k}", s, "".join(chr(ascii + int(v)) for v in q), int(rng.integers(1, 51)) if rng.random() < 0.5 else 1))
        return reads

    o = draw_opts(rng, read_len) if opts is None else opts
    f = side("r")
    more = {}
    if paired:
        r = side("r")
        more = {"rev_seqs": [x[1] for x in r], "rev_quals": [x[2] for x in r], "rev_sizes": [x[3] for x in r]}
    s = _set(f"generate_{seed}", o, f, **more)
    if paired:
        s["rev_labels"] = [f"{lab.split(';')[0]};size={n}" for lab, n in zip(s["labels"], s["rev_sizes"])]
    return s


# ---- the reference CLI ---------------------------------------------------------------------------------------------------------
def ref_binary():
    here = os.path.dirname(os.path.abspath(__file__))
    return os.path.join(os.path.dirname(here), "oracle", "_ref", "vsearch_ref")


def _write(path, labels, seqs, quals):
    with open(path, "w") as fh:
        for k, (lab, s) in enumerate(zip(labels, seqs)):
            fh.write(f"@{lab}\n{s}\n+\n{quals[k]}\n" if quals is not None else f">{lab}\n{s}\n")


def run_reference(s, eeout=True):
    """Run the reference CLI on a set (--fastq_filter, or --fastx_filter for FASTA input; --threads 1, --sizein where the set has
    abundances).  -> dict(returncode, stderr, kept / discarded / kept_rev / discarded_rev: the lines of --fastqout (with
    --fastq_eeout) and its siblings, or of --fastaout and its siblings for FASTA input, counts, seconds)"""
    import time
    fastq = s["quals"] is not None
    paired = s.get("rev_seqs") is not None
    with tempfile.TemporaryDirectory() as d:
        p = lambda n: os.path.join(d, n)       # noqa: E731
        _write(p("f.in"), s["labels"], s["seqs"], s["quals"])
        kind = "fastq" if fastq else "fasta"
        args = [ref_binary(), "--fastq_filter" if fastq else "--fastx_filter", p("f.in"), f"--{kind}out", p("kept"),
                f"--{kind}out_discarded", p("discarded"), "--log", p("log"), "--threads", "1", "--quiet"]
        if paired:
            _write(p("r.in"), s.get("rev_labels") or s["labels"], s["rev_seqs"], s["rev_quals"])
            args += ["--reverse", p("r.in"), f"--{kind}out_rev", p("kept_rev"), f"--{kind}out_discarded_rev", p("discarded_rev")]
        if fastq and eeout:
            args.append("--fastq_eeout")
        if s.get("sizes") or s.get("rev_sizes"):
            args.append("--sizein")
        for k, v in s["opts"].items():
            args += [CLI_FLAGS[k], repr(v) if isinstance(v, float) else str(v)]
        t0 = time.perf_counter()
        r = subprocess.run(args, capture_output=True, text=True)
        dt = time.perf_counter() - t0
        read = lambda n: open(p(n)).read().splitlines() if os.path.exists(p(n)) else []      # noqa: E731
        log = open(p("log")).read() if os.path.exists(p("log")) else ""
        m = re.search(r"(\d+) sequences kept \(of which (\d+) truncated\), (\d+) sequences discarded", log)
        counts = dict(zip(("kept", "truncated", "discarded"), map(int, m.groups()))) if m else None
        return {"returncode": r.returncode, "stderr": r.stderr, "kept": read("kept"), "discarded": read("discarded"),
                "kept_rev": read("kept_rev"), "discarded_rev": read("discarded_rev"), "counts": counts, "seconds": dt}


def library_lines(res, s, eeout=True):
    """the same four outputs from a vsearch_amd.filter.FilterResult"""
    fastq = s["quals"] is not None
    fmt = (lambda lab, which, side: res.fastq_lines(lab, which, side, eeout=eeout)) if fastq else \
        (lambda lab, which, side: res.fasta_lines(lab, which, side))
    out = {"kept": fmt(s["labels"], "kept", "fwd"), "discarded": fmt(s["labels"], "discarded", "fwd"), "kept_rev": [], "discarded_rev": []}
    if s.get("rev_seqs") is not None:
        rl = s.get("rev_labels") or s["labels"]
        out.update({"kept_rev": fmt(rl, "kept", "rev"), "discarded_rev": fmt(rl, "discarded", "rev")})
    out["counts"] = res.counts()
    return out


def call_args(s):
    """positional and keyword arguments of vsearch_amd.filter.filter_reads (behind the aligner) for a set"""
    return (s["seqs"], s["quals"]), dict(s["opts"], rev_seqs=s.get("rev_seqs"), rev_quals=s.get("rev_quals"), sizes=s.get("sizes"),
                                         rev_sizes=s.get("rev_sizes"))


def scattered_call(aligner, s, seed, **extra):
    """The set through vsx_fastx_filter with its reads laid out in the blobs in shuffled order, junk between them and equal reads
    sharing their bytes (non-monotone, overlapping offsets).  -> (records, rev_records or None, pair_discarded, counts)"""
    import ctypes as C
    from vsearch_amd import _lib
    from vsearch_amd.filter import _records, default_opts
    rng = np.random.default_rng(seed)
    lib = _lib.load()
    n = len(s["seqs"])
    keep = []

    def side(seqs, quals, sizes):
        order = rng.permutation(n)
        off, sb, qb, seen = np.zeros(n, np.uint64), bytearray(), bytearray(), {}
        for k in order:
            key = (seqs[k], quals[k] if quals is not None else None)
            if key not in seen:
                gap = int(rng.integers(0, 9))
                sb += b"N" * gap
                qb += b"\x7f" * gap                       # out of range under every offset: nobody may read between the reads
                seen[key] = len(sb)
                sb += seqs[k].encode()
                qb += (quals[k] if quals is not None else "").encode()
            off[k] = seen[key]
        lens = np.array([len(x) for x in seqs], np.uint32)
        ab = np.ascontiguousarray(sizes, np.uint64) if sizes is not None else None
        sb, qb = bytes(sb), bytes(qb)
        keep.extend([sb, qb, off, lens, ab])
        raw = lambda b: C.cast(C.c_char_p(b), C.c_void_p)  # noqa: E731
        return _lib.FilterReads(raw(sb), raw(qb) if quals is not None else None, len(sb), off.ctypes.data, lens.ctypes.data,
                                ab.ctypes.data if ab is not None else None)

    fwd = side(s["seqs"], s["quals"], s.get("sizes"))
    rev = side(s["rev_seqs"], s["rev_quals"], s.get("rev_sizes")) if s.get("rev_seqs") is not None else None
    out = _lib.FilterOut()
    o = default_opts(**dict(s["opts"], **extra))
    _lib.check(lib.vsx_fastx_filter(aligner.h if aligner is not None else None, C.byref(o), C.c_uint64(n), C.byref(fwd),
                                    C.byref(rev) if rev is not None else None, C.byref(out)), "vsx_fastx_filter")
    try:
        return (_records(out.fwd, n), _records(out.rev, n) if rev is not None else None,
                np.ctypeslib.as_array(out.pair_discarded, shape=(n,)).copy(),
                {"kept": int(out.kept), "truncated": int(out.kept_truncated), "discarded": int(out.discarded)})
    finally:
        lib.vsx_fastx_filter_out_free(C.byref(out))


# ---- tests/golden/fastq_filter_golden.json -----------------------------------------------------------------------------------------
GOLDEN_SEEDS = ((21, False), (22, True), (23, False))     # generate(seed, 40, read_len=100, paired)


def golden_sets():
    return edge_reads() + [generate(seed, 40, read_len=100, paired=p) for seed, p in GOLDEN_SEEDS] + [fasta_set()]


def write_golden(path):
    """Record the reference CLI's answers (--threads 1): golden_sets() and rounding_reads() with their four outputs and totals, and
    for quality_cases() whether the run was fatal, with the value and the bound of its message."""
    import json
    from tests.merge_data import pack_golden
    doc = {"sets": [], "rounding": [], "quality": []}
    for key, sets in (("sets", golden_sets()), ("rounding", rounding_reads())):
        for s in sets:
            ref = run_reference(s)
            assert ref["returncode"] == 0, (s["name"], ref["stderr"])
            doc[key].append({"input": s, "expected": {k: ref[k] for k in ("kept", "discarded", "kept_rev", "discarded_rev", "counts")}})
    for s, _ in quality_cases():
        ref = run_reference(s)
        m = re.search(r"FASTQ quality value \((-?\d+)\) (below qmin|above qmax) \((-?\d+)\)", ref["stderr"])
        fatal = [m.group(2), int(m.group(1)), int(m.group(3))] if m else None
        assert (ref["returncode"] != 0) == (fatal is not None), (s["name"], ref["stderr"])
        doc["quality"].append({"input": s, "fatal": fatal,
                               "expected": None if fatal else {k: ref[k] for k in ("kept", "discarded", "kept_rev", "discarded_rev", "counts")}})
    with open(path, "w") as fh:
        json.dump(pack_golden(doc), fh, indent=0)


def load_golden(path):
    from tests.merge_data import load_golden as load
    return load(path)


if __name__ == "__main__":
    import sys
    write_golden(sys.argv[1])
