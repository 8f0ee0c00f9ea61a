"""Inputs for the read-statistics tests and bench_eestats.py, plain-Python restatements of the reference's --fastq_eestats and
--fastq_eestats2 (py_eestats, py_eestats2: a second checker beside the library's host restatement; they return the tables and
the text), and a runner of the reference CLI (oracle/_ref/vsearch_ref) that returns the two --output texts as lists of lines.

A "set" is one input with one set of options: {"name", "opts", "quals", "commands"}.  opts: a dict of the keywords of
vsearch_amd.eestats.default_opts (ascii, qmin, qmax, length_cutoffs [shortest, longest or None, increment], ee_cutoffs);
commands: which of "eestats" / "eestats2" the golden file records for the set.
"""
import math
import os
import re
import subprocess
import tempfile

import numpy as np

DEFAULTS = {"ascii": 33, "qmin": 0, "qmax": 41, "length_cutoffs": [50, None, 50], "ee_cutoffs": [0.5, 1.0, 2.0]}
INT_MAX = 2 ** 31 - 1
RESOLUTION = 1000
BOTH = ["eestats", "eestats2"]
HEADER = "Pos\tRecs\tPctRecs\tMin_Q\tLow_Q\tMed_Q\tMean_Q\tHi_Q\tMax_Q\tMin_Pe\tLow_Pe\tMed_Pe\tMean_Pe\tHi_Pe\tMax_Pe\t" \
         "Min_EE\tLow_EE\tMed_EE\tMean_EE\tHi_EE\tMax_EE"

# the tiles of the kernels (vsearch_amd/csrc/vsx_eestats_internal.h): the walk takes 256 reads x 64 positions, the ordered sum
# 16 positions x 256 reads
WALK_READS, WALK_POSITIONS, SUM_POSITIONS = 256, 64, 16
EDGE_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129)
TILE_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65)


class QualityError(Exception):
    """what the reference exits with: kind 'below qmin' / 'above qmax', the value, the bound"""

    def __init__(self, kind, value, bound):
        super().__init__(f"FASTQ quality value ({value}) {kind} ({bound})")
        self.kind, self.value, self.bound = kind, value, bound


def _quality(c, o):
    c = ord(c) if isinstance(c, str) else c
    q = (c - 256 if c > 127 else c) - o["ascii"]
    if q < o["qmin"]:
        raise QualityError("below qmin", q, o["qmin"])
    if q > o["qmax"]:
        raise QualityError("above qmax", q, o["qmax"])
    return max(q, 0)


def _pe(q):
    return math.pow(10.0, -q / 10.0)


def _scan(pairs, reads):
    """the reference's quartile scan over (value, count) pairs in the given order -> [min, low, med, hi, max], -1 where none"""
    found = [-1] * 5
    n = 0.0
    for v, x in pairs:
        if x > 0:
            n += float(x)
            if found[0] < 0:
                found[0] = v
            for k, share in ((1, 0.25), (2, 0.50), (3, 0.75)):
                if found[k] < 0 and n >= share * float(reads):
                    found[k] = v
            found[4] = v
    return found


def py_eestats(quals, opts=None):
    """--fastq_eestats, read by read as the reference does it -> dict(n, len_max, reads_at, qual_counts, sum_ee, ee_bins, hist:
    per position {bin: count}, lines)"""
    o = dict(DEFAULTS, **(opts or {}))
    cols = o["qmax"] + 2
    len_max = max([len(q) for q in quals], default=0)
    reads_at = [0] * len_max
    qual_counts = [[0] * cols for _ in range(len_max)]
    hist = [{} for _ in range(len_max)]
    sum_ee = [0.0] * len_max
    for qual in quals:
        ee = 0.0
        for i, c in enumerate(qual):
            reads_at[i] += 1
            q = _quality(c, o)
            qual_counts[i][q] += 1
            ee += _pe(q)
            b = min(RESOLUTION * (i + 1), int(RESOLUTION * ee))
            hist[i][b] = hist[i].get(b, 0) + 1
            sum_ee[i] += ee
    lines, ee_bins = [HEADER], []
    n = len(quals)
    for i in range(len_max):
        reads = reads_at[i]
        qs = _scan([(float(q), qual_counts[i][q]) for q in range(cols)], reads)
        qsum = 0.0
        for q in range(cols):
            if qual_counts[i][q] > 0:
                qsum += q * float(qual_counts[i][q])
        pes = _scan([(_pe(q), qual_counts[i][q]) for q in range(cols - 1, -1, -1)], reads)
        pesum = 0.0
        for q in range(cols - 1, -1, -1):
            if qual_counts[i][q] > 0:
                pesum += _pe(q) * float(qual_counts[i][q])
        bins = _scan(sorted(hist[i].items()), reads)
        ee_bins.append(bins)
        ees = [(float(b) + 0.5) / RESOLUTION for b in bins]
        row = "%d\t%d\t%.1f" % (i + 1, reads, 100.0 * reads / n)
        row += "\t%.1f\t%.1f\t%.1f\t%.1f\t%.1f\t%.1f" % (qs[0], qs[1], qs[2], 1.0 * qsum / reads, qs[3], qs[4])
        row += "\t%.2g\t%.2g\t%.2g\t%.2g\t%.2g\t%.2g" % (pes[0], pes[1], pes[2], 1.0 * pesum / reads, pes[3], pes[4])
        row += "\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f" % (ees[0], ees[1], ees[2], sum_ee[i] / reads, ees[3], ees[4])
        lines.append(row)
    return {"n": n, "len_max": len_max, "reads_at": reads_at, "qual_counts": qual_counts, "sum_ee": sum_ee, "ee_bins": ee_bins,
            "hist": hist, "lines": lines}


def _c_div(a, b):
    """C integer division: toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def py_eestats2(quals, opts=None):
    """--fastq_eestats2 as the reference does it, the table growing with the longest read so far -> dict(n, symbols, len_max,
    len_steps, cutoff_counts, lines)"""
    o = dict(DEFAULTS, **(opts or {}))
    shortest, longest, increment = o["length_cutoffs"]
    longest = INT_MAX if longest is None else longest
    cutoffs = o["ee_cutoffs"]
    n = symbols = seen_longest = len_steps = 0
    table = []
    for qual in quals:
        n += 1
        if len(qual) > seen_longest:
            seen_longest = len(qual)
            high = min(seen_longest, longest)
            new_steps = 1 + max(0, _c_div(high - shortest, increment))
            if new_steps > len_steps:
                table += [[0] * len(cutoffs) for _ in range(new_steps - len_steps)]
                len_steps = new_steps
        symbols += len(qual)
        ee = 0.0
        for i, c in enumerate(qual):
            ee += _pe(_quality(c, o))
            for x in range(len_steps):
                if i + 1 == shortest + x * increment:
                    for y, cut in enumerate(cutoffs):
                        if ee <= cut:
                            table[x][y] += 1
    first = "%d reads" % n
    if n > 0:
        first += ", max len %d, avg %.1f" % (seen_longest, 1.0 * symbols / n)
    lines = [first, "", "Length" + "".join("         MaxEE %.2f" % c for c in cutoffs), "------" + "   ----------------" * len(cutoffs)]
    for x in range(len_steps):
        length = shortest + x * increment
        if length > longest:
            break
        lines.append("%6d" % length + "".join("   %8d(%5.1f%%)" % (c, 100.0 * c / n) for c in table[x]))
    return {"n": n, "symbols": symbols, "len_max": seen_longest, "len_steps": len_steps, "cutoff_counts": table, "lines": lines}


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _qual(rng, n, values=None, lo=2, hi=41, ascii=33):
    if values is not None:
        return "".join(chr(ascii + int(values[k])) for k in rng.integers(0, len(values), n))
    return "".join(chr(ascii + int(q)) for q in rng.integers(lo, hi + 1, n))


def _put(s, pos, ch):
    return s[:pos] + ch + s[pos + 1:]


def _set(name, opts, quals, commands=None):
    return {"name": name, "opts": opts, "quals": list(quals), "commands": list(commands or BOTH)}


def declining(rng, n, read_len, ascii=33, qrange=(0, 41)):
    """n reads of lengths 0 .. read_len (most of them full length) whose qualities decay toward the 3' end, with dips, clipped to
    qrange (the default changes nothing)"""
    quals = []
    for _ in range(n):
        L = int(rng.integers(0, read_len + 1)) if rng.random() < 0.3 else read_len
        start, drop = rng.integers(30, 42), rng.integers(0, 38)
        q = np.clip(np.rint(start - drop * (np.arange(L) / max(L, 1)) ** 2 + rng.normal(0, 3.0, L)), 0, 41).astype(int)
        if L and rng.random() < 0.3:
            q[rng.integers(0, L, rng.integers(1, 4))] = rng.integers(0, 12)
        q = np.clip(q, qrange[0], qrange[1])
        quals.append("".join(chr(ascii + int(v)) for v in q))
    return quals


def generate(seed, n, read_len=150, opts=None, ascii=33, qrange=(0, 41)):
    return _set(f"generate_{seed}", opts or {}, declining(np.random.default_rng(seed), n, read_len, ascii=ascii, qrange=qrange))


UNSORTED_CUTOFFS = [3.0, 0.25, 1.0, 0.05, 10.0, 0.5, 2.0, 0.001]


def edge_reads():
    """-> the sets at the edges of the two commands and of the kernels' tiles (tests/test_eestats_host.py asserts what each holds)"""
    rng = np.random.default_rng(1010)
    sets = []
    # every edge length in one call
    mixed = [_qual(rng, n) for n in EDGE_LENGTHS] + [_qual(rng, n, lo=20) for n in (129, 70, 64)]
    sets.append(_set("lengths", {}, mixed))
    # more reads than one workgroup of the walk and one step of the ordered sum take, lengths at the position tiles' edges
    tiles = [_qual(rng, TILE_LENGTHS[(k * 7 + k // 11) % len(TILE_LENGTHS)]) for k in range(WALK_READS + 4)]
    for k in (0, WALK_READS - 1, WALK_READS, WALK_READS + 3):
        tiles[k] = _qual(rng, 65, lo=0, hi=5)            # the first and last read of a tile reach the first and last position of one
    sets.append(_set("tiles", {"length_cutoffs": [16, None, 16]}, tiles))
    # positions reached by 5, 4, 3, 2, 1 reads whose running sums fall into different bins: the running count of the quartile scan
    # lands exactly on 0.25, 0.50 and 0.75 of the reads
    quartiles = ["".join(chr(33 + q) for q in row) for row in ([40, 40, 40, 40, 40], [30, 30, 30, 30], [20, 20, 20], [10, 10], [3])]
    sets.append(_set("quartiles", {"length_cutoffs": [1, None, 1]}, quartiles))
    # q = 0 everywhere: ee = i + 1, the last bin of every row, and cutoffs (1.0, 2.0) equal to the running sum
    sets.append(_set("all_q0", {"length_cutoffs": [1, None, 1]}, ["!" * n for n in (1, 2, 3, 64, 65, 0)]))
    # the forms of --length_cutoffs and --ee_cutoffs
    reads = [_qual(rng, n, lo=15) for n in (129, 128, 127, 100, 66, 65, 64, 63, 59, 30, 1, 0)]
    sets.append(_set("lc_1_star_1", {"length_cutoffs": [1, None, 1]}, reads, ["eestats2"]))
    sets.append(_set("lc_60_120_7", {"length_cutoffs": [60, 120, 7]}, reads, ["eestats2"]))
    sets.append(_set("lc_longest_below", {"length_cutoffs": [10, 40, 10]}, reads, ["eestats2"]))
    sets.append(_set("lc_shortest_above", {"length_cutoffs": [500, None, 50]}, reads, ["eestats2"]))
    sets.append(_set("one_cutoff", {"ee_cutoffs": [1.0]}, reads, ["eestats2"]))
    sets.append(_set("eight_cutoffs", {"ee_cutoffs": UNSORTED_CUTOFFS, "length_cutoffs": [20, None, 20]}, reads, ["eestats2"]))
    # offset 64 with qmin -5: symbols below the offset count as q = 0 and add 1.0
    low = [_qual(rng, n, lo=-5, hi=40, ascii=64) for n in (40, 33, 20, 7)] + [";<=>?@" * 5]
    sets.append(_set("ascii64_qmin-5", {"ascii": 64, "qmin": -5, "qmax": 41, "length_cutoffs": [10, None, 10]}, low))
    sets.append(_set("qmax93", {"qmax": 93, "length_cutoffs": [10, None, 10]}, [_qual(rng, n, lo=0, hi=93) for n in (40, 35, 20, 3)] + ["~" * 30]))
    # no reads at all, and reads without a symbol
    sets.append(_set("empty", {}, []))
    sets.append(_set("only_empty_reads", {}, ["", ""]))
    return sets


ROUNDING_VALUES = (2, 3, 10, 13, 20, 23, 30, 33, 37, 40)


def _tree_sum(v, lo, hi, memo):
    """pairwise sum of v[lo:hi], split in the middle; memo: the sums of the ranges already formed for this v"""
    if hi - lo == 1:
        return v[lo]
    if (lo, hi) not in memo:
        mid = lo + (hi - lo) // 2
        memo[(lo, hi)] = _tree_sum(v, lo, mid, memo) + _tree_sum(v, mid, hi, memo)
    return memo[(lo, hi)]


_ROUNDING = {}


def rounding_reads(want=8, tries=20000):
    """-> one-read sets where, at some position, the sum in position order and a pairwise tree sum of the same errors fall into
    different bins of the histogram; the set's only cutoff is the smaller of the two sums at the first such position and its only
    length is that position, so the eestats2 count depends on the order too.  Each set carries "position", "in_order", "tree"."""
    if (want, tries) in _ROUNDING:
        return [dict(s) for s in _ROUNDING[(want, tries)]]
    rng = np.random.default_rng(4711)
    sets = []
    for _ in range(tries):
        n = int(rng.integers(2, 151))
        qual = _qual(rng, n, values=ROUNDING_VALUES)
        pe = [_pe(ord(c) - 33) for c in qual]
        ee, memo = 0.0, {}
        for i in range(n):
            ee += pe[i]
            tree = _tree_sum(pe, 0, i + 1, memo)
            if int(RESOLUTION * ee) != int(RESOLUTION * tree):
                s = _set(f"rounding_{len(sets)}", {"length_cutoffs": [i + 1, i + 1, 1], "ee_cutoffs": [min(ee, tree)]}, [qual], ["eestats2"])
                s.update({"position": i, "in_order": ee, "tree": tree})
                sets.append(s)
                break
        if len(sets) == want:
            break
    _ROUNDING[(want, tries)] = sets
    return [dict(s) for s in sets]


def quality_cases():
    """-> list of (set, (kind, value, bound)): out-of-range values, none of them in the first read; a later read holds another one
    at an earlier position, so the value named tells read order from position order"""
    rng = np.random.default_rng(17)
    good = lambda n, ascii=33: _qual(rng, n, lo=10, hi=40, ascii=ascii)      # noqa: E731
    cases = []
    above = [good(80), _put(good(80), 50, "K"), _put(good(80), 0, "L"), good(80)]
    cases.append((_set("above", {}, above), ("above qmax", 42, 41)))
    below = [good(70), good(70), _put(good(70), 69, "$"), _put(good(70), 2, "#")]
    cases.append((_set("below", {"qmin": 5}, below), ("below qmin", 3, 5)))
    below64 = [good(30, 64), _put(good(30, 64), 10, ":"), _put(good(30, 64), 0, "5")]
    cases.append((_set("below_64", {"ascii": 64, "qmin": -5}, below64), ("below qmin", -6, -5)))
    # many reads: the first bad value sits in the second workgroup of the walk, a later one in the first position of the last read
    many = [good(40) for _ in range(300)]
    many[290] = _put(many[290], 39, "J")
    many[299] = _put(many[299], 0, "K")
    cases.append((_set("above_late", {"qmax": 40}, many), ("above qmax", 41, 40)))
    return cases


# ---- the reference CLI ---------------------------------------------------------------------------------------------------------
def ref_binary():
    here = os.path.dirname(os.path.abspath(__file__))
    return os.path.join(os.path.dirname(here), "oracle", "_ref", "vsearch_ref")


def cli_options(opts):
    o = dict(DEFAULTS, **opts)
    shortest, longest, increment = o["length_cutoffs"]
    return ["--fastq_ascii", str(o["ascii"]), "--fastq_qmin", str(o["qmin"]), "--fastq_qmax", str(o["qmax"]),
            "--length_cutoffs", f"{shortest},{'*' if longest is None else longest},{increment}",
            "--ee_cutoffs", ",".join(repr(float(c)) for c in o["ee_cutoffs"])]


def run_reference(s, commands=BOTH):
    """Write the set as FASTQ and run the reference CLI's --fastq_eestats / --fastq_eestats2 --output on it (one thread: both
    commands are single-threaded) -> dict(returncode, stderr, eestats, eestats2: lists of lines, seconds: per command)"""
    import time
    out = {"returncode": 0, "stderr": "", "seconds": {}}
    with tempfile.TemporaryDirectory() as d:
        fastq = os.path.join(d, "in.fastq")
        with open(fastq, "w") as fh:
            for k, q in enumerate(s["quals"]):
                fh.write(f"@r{k}\n{'A' * len(q)}\n+\n{q}\n")
        for command in commands:
            path = os.path.join(d, command)
            args = [ref_binary(), "--fastq_" + command, fastq, "--output", path, "--quiet", "--threads", "1"]
            # (--length_cutoffs and --ee_cutoffs, the last four entries, belong to eestats2)
            args += cli_options(s["opts"])[:None if command == "eestats2" else -4]
            t0 = time.perf_counter()
            r = subprocess.run(args, capture_output=True, text=True)
            out["seconds"][command] = time.perf_counter() - t0
            out["returncode"] = out["returncode"] or r.returncode
            out["stderr"] += r.stderr
            out[command] = open(path).read().split("\n")[:-1] if os.path.exists(path) and r.returncode == 0 else None
    return out


def call(aligner, s, **extra):
    """the set through vsearch_amd.eestats.read_stats"""
    from vsearch_amd.eestats import read_stats
    return read_stats(aligner, s["quals"], **dict(s["opts"], **extra))


def scattered_call(aligner, s, seed, **extra):
    """the set with its reads laid out in the blob in shuffled order, out-of-range junk between them and equal reads sharing their
    bytes: non-monotonic, overlapping offsets"""
    from vsearch_amd.eestats import stats_of_blob
    rng = np.random.default_rng(seed)
    n = len(s["quals"])
    off, blob, seen = np.zeros(n, np.uint64), bytearray(), {}
    for k in rng.permutation(n):
        q = s["quals"][k]
        if q not in seen:
            blob += b"\x7f" * int(rng.integers(0, 9))          # out of range under every offset: nobody may read between the reads
            seen[q] = len(blob)
            blob += q.encode()
        off[k] = seen[q]
    lens = np.array([len(q) for q in s["quals"]], np.uint32)
    return stats_of_blob(aligner, bytes(blob), off, lens, **dict(s["opts"], **extra))


TABLES = ("reads_at", "qual_counts", "sum_ee", "ee_bins", "cutoff_counts")


def assert_same_tables(a, b, name=""):
    """two EEStatsResults field for field, sum_ee by bit pattern"""
    for f in ("n", "symbols", "len_min", "len_max", "ee_cutoffs", "length_cutoffs"):
        assert getattr(a, f) == getattr(b, f), (name, f)
    for f in TABLES:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), (name, f)
        if x is None:
            continue
        assert x.shape == y.shape and x.dtype == y.dtype, (name, f, x.shape, y.shape)
        if x.dtype.kind == "f":
            x, y = x.view(np.uint64), y.view(np.uint64)
        bad = np.argwhere(x != y)
        assert bad.size == 0, f"{name} {f}: {len(bad)} entries differ, first at {bad[:3].tolist()}"


def assert_equals_py(res, s):
    """an EEStatsResult against py_eestats / py_eestats2, table for table (sum_ee by bit pattern) and line for line"""
    py, py2 = py_eestats(s["quals"], s["opts"]), py_eestats2(s["quals"], s["opts"])
    assert (res.n, res.symbols, res.len_max) == (py2["n"], py2["symbols"], py2["len_max"]), s["name"]
    assert res.len_min == min([len(q) for q in s["quals"]], default=0)
    assert res.reads_at.tolist() == py["reads_at"], s["name"]
    assert res.qual_counts.tolist() == py["qual_counts"], s["name"]
    assert res.sum_ee.view(np.uint64).tolist() == np.array(py["sum_ee"], np.float64).view(np.uint64).tolist(), s["name"]
    assert res.ee_bins.tolist() == py["ee_bins"], s["name"]
    assert res.cutoff_counts.tolist() == py2["cutoff_counts"], s["name"]
    assert res.eestats_lines() == py["lines"] and res.eestats2_lines() == py2["lines"], s["name"]
    return py, py2


# ---- tests/golden/fastq_eestats_golden.json ------------------------------------------------------------------------------------
GOLDEN_SEEDS = (51, 52)            # generate(seed, 40, read_len=100)


def golden_sets():
    return edge_reads() + [generate(seed, 40, read_len=100) for seed in GOLDEN_SEEDS]


def write_golden(path):
    """Record the reference CLI's texts: golden_sets() and rounding_reads() with the --output of the commands each set names, and for
    quality_cases() the value and the bound of the fatal message of both commands."""
    import json
    from tests.merge_data import pack_golden
    doc = {"sets": [], "rounding": [], "quality": []}
    for key, sets in (("sets", golden_sets()), ("rounding", rounding_reads())):
        for s in sets:
            ref = run_reference(s, s["commands"])
            assert ref["returncode"] == 0, (s["name"], ref["stderr"])
            doc[key].append({"input": s, "expected": {c: ref[c] for c in s["commands"]}})
    for s, _ in quality_cases():
        fatal = []
        for command in BOTH:
            ref = run_reference(s, [command])
            m = re.search(r"FASTQ quality value \((-?\d+)\) (below qmin|above qmax) \((-?\d+)\)", ref["stderr"])
            assert ref["returncode"] != 0 and m, (s["name"], ref["stderr"])
            fatal.append([m.group(2), int(m.group(1)), int(m.group(3))])
        assert fatal[0] == fatal[1]
        doc["quality"].append({"input": s, "fatal": fatal[0]})
    with open(path, "w") as fh:
        json.dump(pack_golden(doc), fh, indent=0)


def load_golden(path):
    from tests.merge_data import load_golden as load
    return load(path)


if __name__ == "__main__":
    import sys
    write_golden(sys.argv[1])
