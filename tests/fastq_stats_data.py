"""Inputs for the read-summary tests and bench_fastq_stats.py, plain-Python restatements of the reference's --fastq_stats and
--fastq_chars (py_fastq_stats, py_fastq_chars: a second checker beside the library's host restatement; they return the tables
and the text), and a runner of the reference CLI (oracle/_ref/vsearch_ref) that returns the comparable log lines -- the lines of
--log after the `Started` line, up to but excluding the blank line in front of `Finished` -- or the value and the range of the
fatal message.

A "set" is one input with its options: {"name", "opts", "tail", "seqs", "quals", "commands"}.  opts: ascii, qmin, qmax of
--fastq_stats; tail: --fastq_tail of --fastq_chars; commands: which of "stats" / "chars" the golden file records for the set.
"""
import math
import os
import re
import subprocess
import tempfile

import numpy as np

from tests import eestats_data

DEFAULTS = {"ascii": 33, "qmin": 0, "qmax": 41}
BOTH = ["stats", "chars"]
EE_THRESHOLDS = (1.0, 0.5, 0.25, 0.1)
Q_THRESHOLDS = (5, 10, 15, 20)
U32 = 2 ** 32

# the tiles of the kernels (vsearch_amd/csrc/vsx_fastq_stats_internal.h): 64 positions at a time, waves of 64 reads (256 reads per workgroup)
WALK_POSITIONS, WAVE = 64, 64
EDGE_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 300)
EDGE_READ_COUNTS = (63, 64, 65, 255, 256, 257)
IUPAC = "ACGTURYSWKMDBHVN"


class RangeError(Exception):
    """what the reference exits with: the value and the range"""

    def __init__(self, value, qmin, qmax):
        super().__init__(f"FASTQ quality value ({value}) out of range ({qmin}-{qmax})")
        self.value, self.qmin, self.qmax = value, qmin, qmax


def _score(c, ascii):
    return c - ascii if c >= ascii else 0


def _pe(q):
    return math.pow(10.0, -float(q) / 10.0)


def py_fastq_stats(quals, opts=None):
    """--fastq_stats, read by read as the reference does it -> dict(n, symbols, len_min, len_max, length_counts, symbol_counts
    [len_max][94], sum_ee, ee_counts, q_counts, lines)"""
    o = dict(DEFAULTS, **(opts or {}))
    ascii = o["ascii"]
    len_max = max([len(q) for q in quals], default=0)
    length_counts = [0] * (len_max + 1)
    symbol_counts = [[0] * 94 for _ in range(len_max)]
    sum_ee = [0.0] * len_max
    ee_counts = [[0] * 4 for _ in range(len_max)]
    q_counts = [[0] * 4 for _ in range(len_max)]
    for qual in quals:
        chars = [ord(c) if isinstance(c, str) else c for c in qual]
        length_counts[len(chars)] += 1
        if chars:
            # the lowest, then the highest: as unsigned against (unsigned) qmin and (unsigned) qmax
            for c in (min(chars), max(chars)):
                if not o["qmin"] % U32 <= _score(c, ascii) <= o["qmax"] % U32:
                    raise RangeError(_score(c, ascii), o["qmin"], o["qmax"])
        ee, lowest = 0.0, None
        for i, c in enumerate(chars):
            symbol_counts[i][c - 33] += 1
            q = _score(c, ascii)
            lowest = q if lowest is None else min(lowest, q)
            for k, t in enumerate(Q_THRESHOLDS):
                q_counts[i][k] += lowest > t
            ee += _pe(q)
            sum_ee[i] += ee
            for k, t in enumerate(EE_THRESHOLDS):
                ee_counts[i][k] += ee <= t
    n, symbols = len(quals), sum(len(q) for q in quals)
    t = {"n": n, "symbols": symbols, "len_min": min([len(q) for q in quals], default=0), "len_max": len_max, "length_counts": length_counts,
         "symbol_counts": symbol_counts, "sum_ee": sum_ee, "ee_counts": ee_counts, "q_counts": q_counts}
    t["lines"] = _stats_text(t, ascii)
    return t


def _stats_text(t, ascii):
    n, len_max, lc = float(t["n"]), t["len_max"], t["length_counts"]
    symbols = float(t["symbols"])
    cumulative = list(np.cumsum(lc))
    lines = ["", "Read length distribution", "      L           N      Pct   AccPct", "-------  ----------  -------  -------"]
    for L in range(len_max, t["len_min"] - 1, -1):
        if lc[L] != 0:
            previous = float(cumulative[L - 1]) if L != 0 else 0.0
            lines.append("%2s%5d  %10d   %5.1f%%   %5.1f%%" % (">=" if L == len_max else "  ", L, lc[L], lc[L] * 100.0 / n, 100.0 * (n - previous) / n))
    lines += ["", "Q score distribution", "ASCII    Q       Pe           N      Pct   AccPct", "-----  ---  -------  ----------  -------  -------"]
    dist = [sum(row[k] for row in t["symbol_counts"]) for k in range(94)]
    acc = 0
    for k in reversed(range(94)):
        if dist[k] == 0:
            continue
        acc += dist[k]
        q = _score(33 + k, ascii)
        lines.append("    %c  %3d  %7.5f  %10d  %6.1f%%  %6.1f%%" % (chr(33 + k), q, _pe(q), dist[k], 100.0 * dist[k] / symbols, 100.0 * acc / symbols))
    lines += ["", "    L  PctRecs  AvgQ  P(AvgQ)      AvgP  AvgEE       Rate   RatePct", "-----  -------  ----  -------  --------  -----  ---------  --------"]
    for L in range(2, len_max + 1):
        row = t["symbol_counts"][L - 1]
        count = float(sum(row))
        sum_q = sum(row[k] * _score(33 + k, ascii) for k in range(94))
        sum_p = 0.0
        for k in range(94):
            sum_p = sum_p + float(row[k]) * _pe(_score(33 + k, ascii))
        avgq, avgp, avgee = float(sum_q) / count, sum_p / count, t["sum_ee"][L - 1] / count
        rate = avgee / float(L)
        lines.append("%5d  %6.1f%%  %4.1f  %7.5f  %8.6f  %5.2f  %9.6f  %7.3f%%" % (L, 100.0 * (n - float(cumulative[L - 1])) / n, avgq, _pe(avgq), avgp, avgee, rate,
                                                                            100.0 * rate))
    lines += ["", "    L   1.0000   0.5000   0.2500   0.1000   1.0000   0.5000   0.2500   0.1000",
              "-----  -------  -------  -------  -------  -------  -------  -------  -------"]
    table = t["ee_counts"] + [[0] * 4]
    top = next(i for i, row in enumerate(table) if row[0] == 0)
    for L in range(top, 0, -1):
        c = table[L - 1]
        lines.append("%5d  %7d  %7d  %7d  %7d  %6.2f%%  %6.2f%%  %6.2f%%  %6.2f%%" % ((L,) + tuple(c) + tuple(100.0 * float(x) / n for x in c)))
    lines += ["", "Truncate at first Q", "  Len     Q=5    Q=10    Q=15    Q=20", "-----  ------  ------  ------  ------"]
    L = len_max
    while L >= max(1, len_max // 2):
        lines.append("%5d  %5.1f%%  %5.1f%%  %5.1f%%  %5.1f%%" % ((L,) + tuple(100.0 * float(x) / n for x in t["q_counts"][L - 1])))
        L -= 1
    lines += ["", "%10d  Recs (%.1fM), 0 too long" % (t["n"], n / 1000000.0)]
    if t["n"] != 0:
        lines.append("%10.1f  Avg length" % (1.0 * symbols / n))
    lines.append("%9.1fM  Bases" % (symbols / 1000000.0))
    return lines


def map_symbol(c):
    c = ord(c) if isinstance(c, str) else c
    return c & 0xDF if chr(c).isascii() and chr(c).isalpha() else ord("N")


def py_fastq_chars(seqs, quals, tail=4):
    """--fastq_chars, read by read as the reference does it -> dict(n, total_chars, seq_counts, qual_counts, tail_counts, maxrun
    [256 each], qmin_n, qmax_n, lines)"""
    seq_counts, qual_counts, tail_counts, maxrun = [0] * 256, [0] * 256, [0] * 256, [0] * 256
    qmin_n, qmax_n, total = 255, 0, 0
    for seq, qual in zip(seqs, quals):
        assert len(seq) == len(qual)
        total += len(seq)
        q = [ord(c) if isinstance(c, str) else c for c in qual]
        run_char, run = -1, 0
        for i, raw in enumerate(seq):
            s = map_symbol(raw)
            seq_counts[s] += 1
            qual_counts[q[i]] += 1
            if s == ord("N"):
                qmin_n, qmax_n = min(qmin_n, q[i]), max(qmax_n, q[i])
            if s == run_char:
                run += 1
                maxrun[s] = max(maxrun[s], run)
            else:
                run_char, run = s, 0
        if len(q) >= tail and all(c == q[-1] for c in q[len(q) - tail:]):
            tail_counts[q[-1]] += 1
    t = {"n": len(seqs), "total_chars": total, "seq_counts": seq_counts, "qual_counts": qual_counts, "tail_counts": tail_counts,
         "maxrun": maxrun, "qmin_n": qmin_n, "qmax_n": qmax_n}
    t["lines"] = _chars_text(t)
    return t


FORMATS = ("Solexa format (phred+64)", "Illumina 1.3+ format (phred+64)", "Illumina 1.5+ format (phred+64)",
           "Illumina 1.8+ format (phred+33)", "Original Sanger format (phred+33)")


def _chars_text(t):
    lines = ["Read %d sequences." % t["n"]]
    if t["n"] == 0:
        return lines
    seen = [c for c in range(256) if t["qual_counts"][c]]
    qmin, qmax = (seen[0], seen[-1]) if seen else (0, 0)
    offset = 33 if qmin < 59 or qmax < 75 else 64
    lines.append("Qmin %d, Qmax %d, Range %d" % (qmin, qmax, qmax - qmin + 1))
    lines.append("Guess: -fastq_qmin %d -fastq_qmax %d -fastq_ascii %d" % (qmin - offset, qmax - offset, offset))
    if offset == 64:
        lines.append("Guess: " + (FORMATS[0] if qmin < 64 else FORMATS[1] if qmin < 66 else FORMATS[2]))
    else:
        lines.append("Guess: " + (FORMATS[3] if qmax > 73 else FORMATS[4]))
    lines += ["", "Letter          N   Freq MaxRun", "------ ---------- ------ ------"]
    for c in range(256):
        if t["seq_counts"][c]:
            line = "     %c %10d %5.1f%% %6d" % (chr(c), t["seq_counts"][c], t["seq_counts"][c] * (100.0 / t["total_chars"]), t["maxrun"][c])
            if c == ord("N"):
                line += "  Q=%c..%c" % (chr(t["qmin_n"]), chr(t["qmax_n"])) if t["qmin_n"] < t["qmax_n"] else "  Q=%c" % chr(t["qmin_n"])
            lines.append(line)
    lines += ["", "Char  ASCII    Freq       Tails", "----  -----  ------  ----------"]
    for c in seen:
        lines.append(" '%c'  %5d  %5.1f%%  %10d" % (chr(c), c, t["qual_counts"][c] * (100.0 / t["total_chars"]), t["tail_counts"][c]))
    return lines


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _set(name, quals, seqs=None, opts=None, tail=4, commands=None):
    quals = list(quals)
    return {"name": name, "opts": dict(opts or {}), "tail": tail, "seqs": list(seqs) if seqs is not None else ["A" * len(q) for q in quals],
            "quals": quals, "commands": list(commands or BOTH)}


def _seq(rng, n):
    """n symbols: mostly ACGT with homopolymer stretches, some N, IUPAC codes and lower case"""
    out = []
    while len(out) < n:
        r = rng.random()
        c = "ACGT"[int(rng.integers(0, 4))] if r < 0.9 else "N" if r < 0.94 else IUPAC[int(rng.integers(0, len(IUPAC)))]
        if rng.random() < 0.05:
            c = c.lower()
        out += [c] * (int(rng.integers(2, 9)) if rng.random() < 0.1 else 1)
    return "".join(out[:n])


def _q(values, ascii=33):
    return "".join(chr(ascii + v) for v in values)


def generate(seed, n, read_len=150, opts=None, tail=4, ascii=33, qrange=(0, 41)):
    """n reads of lengths 0 .. read_len with declining qualities (eestats_data.declining); every fifth read ends in a quality tail"""
    rng = np.random.default_rng(seed)
    quals = eestats_data.declining(rng, n, read_len, ascii=ascii, qrange=qrange)
    for k in range(0, n, 5):
        t = int(rng.integers(1, 9))
        if len(quals[k]) >= t:
            quals[k] = quals[k][:len(quals[k]) - t] + quals[k][-1] * t
    return _set(f"generate_{seed}", quals, [_seq(rng, len(q)) for q in quals], opts, tail)


# per format guess of --fastq_chars: the lowest and the highest quality character of the set
FORMAT_RANGES = {"solexa": (";", "h"), "illumina13": ("@", "h"), "illumina15": ("B", "i"), "illumina18": ("#", "J"), "sanger": ("!", "I")}
# reads whose running expected error lands exactly on, or one ulp beside, a threshold (values: tests/test_fastq_stats_host.py)
EE_LANDINGS = ("+II", "+++++", "!I", "5" * 25, "5" * 10)
Q_EDGES = (5, 6, 10, 11, 15, 16, 20, 21)
Q_FALLS_AT_64 = "I" * 64 + "&I"


def edge_reads():
    """-> the sets at the edges of the two commands and of the kernels' tiles (tests/test_fastq_stats_host.py asserts what each holds)"""
    rng = np.random.default_rng(2020)
    qual = lambda n, lo=2, hi=41: eestats_data._qual(rng, n, lo=lo, hi=hi)      # noqa: E731
    few = lambda n: eestats_data._qual(rng, n, values=(3, 12, 25, 38))          # noqa: E731  (few rows in the recorded tables)
    sets = []
    # every edge length in one call, and a read whose lowest score falls at position 64 (0-based), the first of the second tile
    lengths = [few(n) for n in EDGE_LENGTHS] + [few(n) for n in (70, 64, 2)] + [Q_FALLS_AT_64]
    sets.append(_set("lengths", lengths, [_seq(rng, len(q)) for q in lengths]))
    # reads per call at the edges of a wave and of a workgroup; short reads (the golden file records every set's text)
    for count in EDGE_READ_COUNTS:
        quals = [few((k * 7 + k // 11) % 5) for k in range(count)]
        sets.append(_set(f"reads_{count}", quals, ["ACGTT"[:len(q)] for q in quals]))
    # the longest read in the last lane of a wave only
    last = [few(int(rng.integers(0, 11))) for _ in range(WAVE - 1)] + [few(20)]
    sets.append(_set("last_lane", last, [_seq(rng, len(q)) for q in last]))
    # exact landings of the running expected error, and lowest scores on both sides of every Q threshold
    sets.append(_set("ee_landings", EE_LANDINGS, commands=["stats"]))
    q_edges = ["IIII" + chr(33 + m) + "II" for m in Q_EDGES]
    sets.append(_set("q_edges", q_edges, commands=["stats"]))
    # offset 64: a ';' is below the offset, counts as Q 0 with Pe 1.0 and passes qmin 0
    sets.append(_set("ascii64_low", ["hhh;hhhh", "@ABCDefgh", "hhhhh", ";;"], opts={"ascii": 64}, commands=["stats"]))
    sets.append(_set("qmax93", [qual(n, lo=0, hi=93) for n in (12, 9, 3)] + ["~" * 5], opts={"qmax": 93}, commands=["stats"]))
    # no reads at all, and reads without a symbol
    sets.append(_set("empty", []))
    sets.append(_set("only_empty_reads", ["", "", ""]))
    # runs of 1, 2, 64, 65 and a whole read; a run that would continue across two reads; lower case and IUPAC; no N
    runs = ["ACGT" + "C" * 2 + "A" + "G" * 64 + "A" + "T" * 65 + "A", "W" * 70, "KKKKK", "KKKKKKK", "acgtRYSWKMDBHVuUaA", "rrRRr"]
    sets.append(_set("runs", [qual(len(s), lo=30) for s in runs], runs, commands=["chars"]))
    # N with one quality character, and with two
    sets.append(_set("n_one_q", ["IIII#II", "II#"], ["ACGTNAC", "AAn"], commands=["chars"]))
    sets.append(_set("n_two_q", ["IIII#II", "II5"], ["ACGTNAC", "AAn"], commands=["chars"]))
    # tails: the same reads under tail = 1, 4, the read length and the read length + 1; "IIII5555" + "I5555": the character that
    # breaks the tail sits at exactly len - tail under tail = 5 and 8
    tails = ["IIII5555", "I5555", "55555555", "I", "", "IIIIIII5", "+++I+++"]
    for tail in (1, 4, 5, 8, 9):
        sets.append(_set(f"tail_{tail}", tails, [_seq(rng, len(q)) for q in tails], tail=tail, commands=["chars"]))
    # quality ranges that land on each of the five format guesses
    for name, (lo, hi) in FORMAT_RANGES.items():
        quals = [lo + hi * 5, _q(rng.integers(ord(lo) - 33, ord(hi) - 32, 40)), hi * 4]
        sets.append(_set("format_" + name, quals, [_seq(rng, len(q)) for q in quals], commands=["chars"]))
    return sets


ORDER_VALUES = (2, 3, 13, 23, 33, 37)
_ORDER = {}


def order_reads(want=4, tries=20000):
    """-> sets of a few reads in which summing the running expected errors of some position over the reads in reversed order gives
    other bits than in input order, found by search.  Each set carries "position", the first such position."""
    if (want, tries) in _ORDER:
        return [dict(s) for s in _ORDER[(want, tries)]]
    rng = np.random.default_rng(1234)
    sets = []
    for _ in range(tries):
        quals = [eestats_data._qual(rng, int(rng.integers(3, 8)), values=ORDER_VALUES) for _ in range(int(rng.integers(3, 6)))]
        forward, backward = py_fastq_stats(quals)["sum_ee"], py_fastq_stats(quals[::-1])["sum_ee"]
        differ = [i for i, (a, b) in enumerate(zip(forward, backward)) if a != b]
        if differ:
            s = _set(f"order_{len(sets)}", quals, commands=["stats"])
            s["position"] = differ[0]
            sets.append(s)
        if len(sets) == want:
            break
    _ORDER[(want, tries)] = sets
    return [dict(s) for s in sets]


def quality_cases():
    """-> list of (set, (value, qmin, qmax)): reads the range check refuses, none of them the first read; a later read would be
    refused with another value, so the value named tells the first read in input order"""
    rng = np.random.default_rng(17)
    good = lambda n, ascii=33: eestats_data._qual(rng, n, lo=10, hi=40, ascii=ascii)      # noqa: E731
    put = eestats_data._put
    cases = []
    # offset 64 with qmin -5: (unsigned) -5 refuses every non-empty read, the empty first one passes
    cases.append((_set("negative_qmin", ["", "h", "hhi"], opts={"ascii": 64, "qmin": -5}, commands=["stats"]), (40, -5, 41)))
    above = [good(80), put(good(80), 50, "K"), put(good(80), 0, "L"), good(80)]
    cases.append((_set("above", above, commands=["stats"]), (42, 0, 41)))
    below = [good(70), good(70), put(good(70), 69, "$"), put(good(70), 2, "#")]
    cases.append((_set("below", below, opts={"qmin": 5}, commands=["stats"]), (3, 5, 41)))
    # a read with both: the lowest is named; the highest of the read before it is in range
    both = [good(30), put(put(good(30), 3, "L"), 20, "%"), put(good(30), 0, "M")]
    cases.append((_set("both", both, opts={"qmin": 5}, commands=["stats"]), (4, 5, 41)))
    # many reads: the first refused read sits in the second workgroup of the walk, a later one is the last read
    many = [good(4) for _ in range(260)]
    many[257] = put(many[257], 3, "J")
    many[259] = put(many[259], 0, "K")
    cases.append((_set("above_late", many, opts={"qmax": 40}, commands=["stats"]), (41, 0, 40)))
    return cases


# ---- the reference CLI ---------------------------------------------------------------------------------------------------------
def ref_binary():
    return eestats_data.ref_binary()


def comparable(log_text):
    """the lines of a --log after the `Started` line, up to but excluding the blank line in front of `Finished`"""
    lines = log_text.split("\n")
    start = next(k for k, line in enumerate(lines) if line.startswith("Started"))
    end = next(k for k, line in enumerate(lines) if line.startswith("Finished"))
    assert lines[end - 1] == ""
    return lines[start + 1:end - 1]


def run_reference(s, commands=BOTH):
    """Write the set as FASTQ and run the reference CLI's --fastq_stats / --fastq_chars --log on it (one thread: both commands are
    single-threaded) -> dict(returncode, stderr, stats, chars: lists of lines or None, fatal: (value, qmin, qmax) or None,
    seconds: per command)"""
    import time
    out = {"returncode": 0, "stderr": "", "seconds": {}, "fatal": None}
    o = dict(DEFAULTS, **s["opts"])
    with tempfile.TemporaryDirectory() as d:
        fastq = os.path.join(d, "in.fastq")
        with open(fastq, "w") as fh:
            for k, (seq, q) in enumerate(zip(s["seqs"], s["quals"])):
                fh.write(f"@r{k}\n{seq}\n+\n{q}\n")
        for command in commands:
            path = os.path.join(d, command + ".log")
            args = [ref_binary(), "--fastq_" + command, fastq, "--log", path, "--quiet", "--threads", "1"]
            if command == "stats":
                args += ["--fastq_ascii", str(o["ascii"]), "--fastq_qmin", str(o["qmin"]), "--fastq_qmax", str(o["qmax"])]
            else:
                args += ["--fastq_tail", str(s["tail"])]
            t0 = time.perf_counter()
            r = subprocess.run(args, capture_output=True, text=True)
            out["seconds"][command] = time.perf_counter() - t0
            out["returncode"] = out["returncode"] or r.returncode
            out["stderr"] += r.stderr
            out[command] = comparable(open(path).read()) if r.returncode == 0 else None
            m = re.search(r"FASTQ quality value \((-?\d+)\) out of range \((-?\d+)-(-?\d+)\)", r.stderr)
            if r.returncode != 0 and m:
                out["fatal"] = tuple(int(x) for x in m.groups())
    return out


# ---- calls and comparisons -----------------------------------------------------------------------------------------------------
def call_stats(aligner, s, **extra):
    from vsearch_amd.fastq_stats import fastq_stats
    return fastq_stats(aligner, s["quals"], **dict(s["opts"], **extra))


def call_chars(aligner, s, **extra):
    from vsearch_amd.fastq_stats import fastq_chars
    return fastq_chars(aligner, s["seqs"], s["quals"], **dict({"tail": s["tail"]}, **extra))


def call(aligner, s, command, **extra):
    return (call_stats if command == "stats" else call_chars)(aligner, s, **extra)


def scattered(s, seed):
    """the set's reads laid out in larger blobs in shuffled order, junk between them (a quality byte out of range under every
    offset, a non-letter in the sequence) and equal reads sharing their bytes -> seq blob, qual blob, offsets, lengths"""
    rng = np.random.default_rng(seed)
    n = len(s["quals"])
    off, sblob, qblob, seen = np.zeros(n, np.uint64), bytearray(), bytearray(), {}
    for k in rng.permutation(n):
        key = (s["seqs"][k], s["quals"][k])
        if key not in seen:
            junk = int(rng.integers(0, 9))
            sblob += b"*" * junk
            qblob += b"\x7f" * junk
            seen[key] = len(qblob)
            sblob += key[0].encode()
            qblob += key[1].encode()
        off[k] = seen[key]
    return bytes(sblob), bytes(qblob), off, np.array([len(q) for q in s["quals"]], np.uint32)


def scattered_call(aligner, s, command, seed, **extra):
    from vsearch_amd.fastq_stats import chars_of_blob, stats_of_blob
    sblob, qblob, off, lens = scattered(s, seed)
    if command == "stats":
        return stats_of_blob(aligner, qblob, off, lens, **dict(s["opts"], **extra))
    return chars_of_blob(aligner, sblob, qblob, off, lens, **dict({"tail": s["tail"]}, **extra))


STATS_FIELDS = ("n", "symbols", "len_min", "len_max")
STATS_TABLES = ("length_counts", "symbol_counts", "sum_ee", "ee_counts", "q_counts")
CHARS_FIELDS = ("n", "total_chars", "qmin_n", "qmax_n")
CHARS_TABLES = ("seq_counts", "qual_counts", "tail_counts", "maxrun")


def assert_same_tables(a, b, name=""):
    """two results of one command field for field, sum_ee by bit pattern"""
    stats = hasattr(a, "sum_ee")
    for f in STATS_FIELDS if stats else CHARS_FIELDS:
        assert getattr(a, f) == getattr(b, f), (name, f, getattr(a, f), getattr(b, f))
    for f in STATS_TABLES if stats else CHARS_TABLES:
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape and x.dtype == y.dtype, (name, f, x.shape, y.shape)
        if x.dtype.kind == "f":
            x, y = x.view(np.uint64), y.view(np.uint64)
        bad = np.argwhere(x != y)
        assert bad.size == 0, f"{name} {f}: {len(bad)} entries differ, first at {bad[:3].tolist()}"


def assert_equals_py(res, s, command):
    """a result against py_fastq_stats / py_fastq_chars, table for table (sum_ee by bit pattern) and line for line"""
    if command == "stats":
        py = py_fastq_stats(s["quals"], s["opts"])
        for f in STATS_FIELDS:
            assert getattr(res, f) == py[f], (s["name"], f)
        for f in STATS_TABLES:
            mine = getattr(res, f)
            if f == "sum_ee":
                assert mine.view(np.uint64).tolist() == np.array(py[f], np.float64).view(np.uint64).tolist(), (s["name"], f)
            else:
                assert mine.tolist() == py[f], (s["name"], f)
    else:
        py = py_fastq_chars(s["seqs"], s["quals"], s["tail"])
        for f in CHARS_FIELDS + CHARS_TABLES:
            mine = getattr(res, f)
            assert (mine.tolist() if hasattr(mine, "tolist") else mine) == py[f], (s["name"], f)
    assert res.log_lines() == py["lines"], s["name"]
    return py


# ---- tests/golden/fastq_stats_golden.json --------------------------------------------------------------------------------------
GOLDEN_SEED = 61


def golden_sets():
    return edge_reads() + [generate(GOLDEN_SEED, 12, read_len=20, tail=3)]


def write_golden(path):
    """Record the reference CLI's texts: golden_sets() and order_reads() with the comparable log lines of the commands each set names,
    and for quality_cases() the value and the range of the fatal message of --fastq_stats."""
    import json
    from tests.merge_data import pack_golden
    doc = {"sets": [], "order": [], "quality": []}
    for key, sets in (("sets", golden_sets()), ("order", order_reads())):
        for s in sets:
            ref = run_reference(s, s["commands"])
            assert ref["returncode"] == 0, (s["name"], ref["stderr"])
            doc[key].append({"input": s, "expected": {c: ref[c] for c in s["commands"]}})
    for s, _ in quality_cases():
        ref = run_reference(s, ["stats"])
        assert ref["returncode"] != 0 and ref["fatal"], (s["name"], ref["stderr"])
        doc["quality"].append({"input": s, "fatal": list(ref["fatal"])})
    with open(path, "w") as fh:
        json.dump(pack_golden(doc), fh, indent=0)


def load_golden(path):
    from tests.merge_data import load_golden as load
    return load(path)


if __name__ == "__main__":
    import sys
    write_golden(sys.argv[1])
