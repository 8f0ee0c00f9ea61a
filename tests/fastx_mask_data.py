"""Inputs, a plain-Python restatement and the reference-CLI runner for the masking tests (--fastx_mask, --maskfasta).

    py_fastx_mask()   the reference's literal loops: wo (core/mask.cpp:79-134), the window loop (139-188), hardmask (248-262), the
                      counts and verdicts of commands/fastx_mask.cpp:92-146.  It does NOT restate the chain rule of the long route.
    py_windows()      W(i) at one position / the windows the reference's loop visits, for the assertions that a set reaches its case
    golden_sets()     named input sets, each the smallest that reaches the edges it is named after
    run_reference()   the reference CLI (oracle/_ref/vsearch_ref) on one set: --fastaout, --fastqout, --maskfasta --output, the log lines
    __main__          writes tests/golden/fastx_mask_golden.json: the sets' inputs and the reference's recorded text, nothing else
                      --digest / --long S,S,...: child-process drivers of tests/test_gpu_fastx_mask.py

How the sets steer the chain: FILLER is text without a repeated 3-mer in any 64 symbols (a de Bruijn cycle), so a window over it
scores 0; an ISLAND of eight equal symbols scores 10 * 15 / 7 = 21 at (a, b) = (0, 7) when a window starts on it, which is the
smallest masked interval and gives the largest step, 32 + 32 - 7 = 57.
"""
import hashlib
import json
import os
import random
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(HERE, "golden", "fastx_mask_golden.json")

QMASKS = ("none", "soft", "dust")
MODES = (("none", 0), ("soft", 0), ("soft", 1), ("dust", 0), ("dust", 1))     # the rows of the mode table
DEFAULT_OPTS = dict(qmask="dust", hardmask=0, min_unmasked_pct=0.0, max_unmasked_pct=100.0, sizeout=0, xsize=0, relabel=None, fasta_width=80)
WINDOW, HALF, LEVEL = 64, 32, 20
MAX_STEP = 57                          # 32 + 32 - 7: no masked window has b < 7 (asserted over the sets in the host tests)


def full_opts(opts):
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    return o


# ---- the plain-Python restatement ---------------------------------------------------------------------------------------------
def map_2bit(c):
    """utils/maps.cpp: A 0, C 1, G 2, T 3, U 3 in either case, everything else 0"""
    return {"C": 1, "G": 2, "T": 3, "U": 3}.get(c.upper(), 0)


def wo(s):
    """core/mask.cpp:79-134 on the window s (at most 64 symbols) -> (bestv, beg, end)"""
    n = len(s)
    l1 = n - 3 + 1 - 5
    if l1 < 0:
        return 0, 0, 0
    bestv = besti = bestj = 0
    words, word = [], 0
    for j in range(n):
        word = ((word << 2) | map_2bit(s[j])) & 0xFFFFFFFF
        words.append(word & 63)
    for i in range(l1):
        counts = [0] * 64
        total = 0
        for j in range(2, n - i):
            w = words[i + j]
            c = counts[w]
            if c != 0:
                total += c
                v = 10 * total // j
                if v > bestv:
                    bestv, besti, bestj = v, i, j
            counts[w] += 1
    return bestv, besti, besti + bestj


def py_window(seq, i):
    """W(i) = (v, a, b) of the window at position i"""
    return wo(seq[i:i + WINDOW])


def py_windows(seq):
    """the windows the reference's loop visits: [(i, v, a, b)]"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, a, b = py_window(seq, i)
        out.append((i, v, a, b))
        if v > LEVEL and b < HALF:
            i += HALF - b
        i += HALF
    return out


def py_dust(seq, hardmask):
    """dust_core, core/mask.cpp:139-188"""
    out = list(seq) if hardmask else [c.upper() if "a" <= c <= "z" else c for c in seq]
    for i, v, a, b in py_windows(seq):
        if v > LEVEL:
            for j in range(i + a, i + b + 1):
                out[j] = "N" if hardmask else chr(ord(seq[j]) | 0x20)
    return "".join(out)


def py_mask_one(seq, qmask, hardmask):
    """-> (masked text, unmasked count, [symbol does not count])"""
    if qmask == "dust":
        text = py_dust(seq, hardmask)
    elif qmask == "soft" and hardmask:
        text = "".join("N" if ord(c) & 0x20 else c for c in seq)
    else:
        text = seq
    if qmask == "none":
        counts = [True] * len(text)
    elif hardmask:
        counts = [c != "N" for c in text]
    else:
        counts = ["A" <= c <= "Z" for c in text]
    return text, sum(counts), [not c for c in counts]


def py_fastx_mask(seqs, qmask="dust", hardmask=0, min_unmasked_pct=0.0, max_unmasked_pct=100.0):
    """-> dict(text, unmasked, verdict, bits (one flag per packed symbol), kept, discarded_less, discarded_more)"""
    res = dict(text=[], unmasked=[], verdict=[], bits=[], kept=0, discarded_less=0, discarded_more=0)
    for seq in seqs:
        text, unmasked, flags = py_mask_one(seq, qmask, hardmask)
        pct = 100.0 * unmasked / len(seq) if len(seq) else float("nan")
        verdict = 1 if pct < min_unmasked_pct else 2 if pct > max_unmasked_pct else 0
        res[("kept", "discarded_less", "discarded_more")[verdict]] += 1
        res["text"].append(text)
        res["unmasked"].append(unmasked)
        res["verdict"].append(verdict)
        res["bits"] += flags
    return res


# ---- builders ------------------------------------------------------------------------------------------------------------------
def de_bruijn():
    """a cycle of 64 symbols that holds every 3-mer once"""
    k, n, a, out = 4, 3, [0] * 12, []

    def db(t, p):
        if t > n:
            if n % p == 0:
                out.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return "".join("ACGT"[x] for x in out)


CYCLE = de_bruijn()


def filler(n, phase=0):
    return "".join(CYCLE[(phase + k) % 64] for k in range(n))


def island_train(n_islands, period=57, sym="A", tail=0):
    """islands of eight `sym` every `period` symbols, filler between them (from the phases 37 .. 63 of the cycle, at which the filler
    neither starts nor ends on an A and a window that starts on the island scores exactly (21, 0, 7))"""
    out = []
    for k in range(n_islands):
        out.append(sym * 8 + filler(period - 8, phase=37 + (5 * k) % 27))
    return "".join(out) + filler(tail, phase=5)


def low_complexity(rng, n):
    p = rng.choice([1, 2, 3, 4])
    u = "".join(rng.choice("ACGT") for _ in range(p))
    return (u * (n // p + 1))[:n]


def island_seq(rng, n, alphabet="ACGT", lower=0.0, p_island=0.35):
    """n symbols of random text with low-complexity islands; `lower`: the chance of a stretch in lower case"""
    parts, left = [], n
    while left > 0:
        seg = low_complexity(rng, rng.randint(6, 70)) if rng.random() < p_island else "".join(rng.choice(alphabet) for _ in range(rng.randint(5, 90)))
        if rng.random() < lower:
            seg = seg.lower()
        parts.append(seg)
        left -= len(seg)
    return "".join(parts)[:n]


def seeded_sequences(seed, count, lo, hi, **kw):
    rng = random.Random(seed)
    return [island_seq(rng, rng.randint(lo, hi), **kw) for _ in range(count)]


def quality(rng, n):
    return "".join(chr(33 + rng.randint(2, 40)) for _ in range(n))


def _set(name, seqs, opts=None, labels=None, quals=None):
    return dict(name=name, seqs=list(seqs), labels=labels or [f"s{k}" for k in range(len(seqs))], quals=quals, opts=dict(opts or {}))


LENGTHS = (1, 7, 8, 9, 63, 64, 65, 95, 96, 97)
SEGMENT_LENGTHS = (191, 192, 193, 255, 256, 257)


def length_seqs():
    """every length at which the window loop changes shape, as poly-A (masked from 8 on) and as an island train"""
    return ["A" * n for n in LENGTHS] + [island_train(2, tail=40)[:n] for n in LENGTHS]


def window_seqs():
    """b = 7 (step 57), b = 31 (shift 1), b = 32 (no shift), a final window shorter than 8"""
    return [island_train(1, tail=60),                                  # W(0) = (21, 0, 7)
            filler(24) + "A" * 8 + filler(70, phase=9),                # the island ends at 31
            filler(25) + "A" * 8 + filler(70, phase=9),                # ... and at 32
            filler(64, phase=2) + "ACG",                               # the window at 64 has 3 symbols
            "C" * 67]                                                  # ... and here, behind a masked one


def phase_seq():
    """65 islands 57 apart: the chain is 0, 57, 114, ... and walks through every offset of a 64-grid, 0, 1, 56 and 63 among them"""
    return island_train(65, tail=30)


def segment_seqs():
    return [island_train(5)[:n] for n in SEGMENT_LENGTHS] + [phase_seq()]


MODE_SEQS = ["ACGTNNNNacgtnnnnRYKMrykmUUUUuuuu" + "T" * 20 + filler(30) + "acacacacacacacacacac" + filler(12, 3).lower() + "N" + "n",
             "n" * 5 + filler(40, 11) + "N" * 5 + "GGGGGGGGGGGG" + "u" * 12 + "BDHVbdhvSWsw",
             filler(20).lower() + "AAAAAAAAAAAAAAAA" + filler(30, 7)]


def percent_seqs():
    """soft masking, 8 symbols: 25 % (= min, kept), 75 % (= max, kept), 12.5 % (less), 87.5 % (more), 50 %; one third against 33.3 / 33.4"""
    return ["ACgtacgt", "ACGTACgt", "Acgtacgt", "ACGTACGt", "ACGTacgt", "Acg"]


def golden_sets():
    rng = random.Random(1901)
    sets = [_set("lengths", length_seqs()), _set("lengths_hard", length_seqs(), dict(hardmask=1)),
            _set("windows", window_seqs()), _set("segments", segment_seqs())]
    for qmask, hard in MODES:
        sets.append(_set(f"modes_{qmask}_{hard}", MODE_SEQS, dict(qmask=qmask, hardmask=hard)))
    sets.append(_set("percent", percent_seqs(), dict(qmask="soft", min_unmasked_pct=25.0, max_unmasked_pct=75.0)))
    sets.append(_set("percent_third", percent_seqs(), dict(qmask="soft", min_unmasked_pct=33.4, max_unmasked_pct=100.0)))
    sets.append(_set("percent_hard", MODE_SEQS + ["N" * 30 + "ACGT"], dict(qmask="dust", hardmask=1, min_unmasked_pct=50.0, max_unmasked_pct=90.0)))
    mixed = seeded_sequences(1902, 24, 30, 400, alphabet="ACGTacgtNRYU", lower=0.2)
    sets.append(_set("fastq", mixed, dict(min_unmasked_pct=40.0), quals=[quality(rng, len(s)) for s in mixed]))
    sets.append(_set("fastq_soft_hard", mixed, dict(qmask="soft", hardmask=1, max_unmasked_pct=95.0), quals=sets[-1]["quals"]))
    sized = [f"r{k};size={k + 2}" for k in range(len(mixed))]
    sets.append(_set("relabel_sizeout", mixed, dict(relabel="M", sizeout=1, fasta_width=0), labels=sized))
    sets.append(_set("xsize_width", mixed, dict(xsize=1, fasta_width=33, hardmask=1), labels=sized))
    return sets


def empty_set():
    """a sequence of length 0 (NaN per cent: kept) between others; the CLI never delivers one, so this set has no golden"""
    return _set("empty", ["", "ACGTACGTAAAAAAAAAAAAAAAA", "", "acgt", ""], dict(min_unmasked_pct=10.0, max_unmasked_pct=90.0))


def sizes_of(s):
    out = []
    for lab in s["labels"]:
        m = re.search(r"(?:^|;)size=(\d+)(?:;|$)", lab)
        out.append(int(m.group(1)) if m else 1)
    return out


def mask_kw(s):
    o = full_opts(s["opts"])
    return dict(qmask=o["qmask"], hardmask=o["hardmask"], min_unmasked_pct=o["min_unmasked_pct"], max_unmasked_pct=o["max_unmasked_pct"])


def writer_kw(s):
    o = full_opts(s["opts"])
    return dict(sizes=sizes_of(s), sizeout=bool(o["sizeout"]), xsize=bool(o["xsize"]), relabel=o["relabel"], fasta_width=o["fasta_width"])


# ---- the reference CLI -----------------------------------------------------------------------------------------------------------
def ref_binary():
    return os.path.join(ROOT, "oracle", "_ref", "vsearch_ref")


def write_fasta(path, names, seqs):
    with open(path, "w") as f:
        for n, s in zip(names, seqs):
            f.write(f">{n}\n{s}\n")


def write_fastq(path, names, seqs, quals):
    with open(path, "w") as f:
        for n, s, q in zip(names, seqs, quals):
            f.write(f"@{n}\n{s}\n+\n{q}\n")


def cli_args(opts, percentages=True):
    o = full_opts(opts)
    a = ["--qmask", o["qmask"], "--fasta_width", str(o["fasta_width"]), "--threads", "1", "--quiet"]
    if percentages:
        a += ["--min_unmasked_pct", repr(o["min_unmasked_pct"]), "--max_unmasked_pct", repr(o["max_unmasked_pct"])]
    for flag in ("hardmask", "sizeout", "xsize"):
        if o[flag]:
            a.append("--" + flag)
    if o["relabel"] is not None:
        a += ["--relabel", o["relabel"]]
    return a


def _run(args, name):
    r = subprocess.run(args, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{name}: reference CLI failed: {r.stderr[-2000:]}")


def run_reference(s, outputs=("fasta", "fastq", "maskfasta", "log")):
    """-> dict(fasta, fastq (None for FASTA input), maskfasta, log): the lines of each output"""
    fastq = s.get("quals") is not None
    with tempfile.TemporaryDirectory(prefix="vsx_mask_") as tmp:
        p = lambda n: os.path.join(tmp, n)
        read = lambda n: open(p(n)).read().split("\n")[:-1]
        write_fasta(p("in.fa"), s["labels"], s["seqs"])
        if fastq:
            write_fastq(p("in.fq"), s["labels"], s["seqs"], s["quals"])
        out = {}
        if set(outputs) & {"fasta", "fastq", "log"}:
            args = [ref_binary(), "--fastx_mask", p("in.fq") if fastq else p("in.fa"), "--fastaout", p("fasta"), "--log", p("log.txt")]
            if fastq:
                args += ["--fastqout", p("fastq")]
            _run(args + cli_args(s["opts"]), s["name"])
            out["fasta"] = read("fasta")
            out["fastq"] = read("fastq") if fastq else None
            out["log"] = [l for l in open(p("log.txt")).read().splitlines() if re.search(r"sequences (kept|with (less|more) than)", l)]
        if "maskfasta" in outputs:
            _run([ref_binary(), "--maskfasta", p("in.fa"), "--output", p("masked")] + cli_args(s["opts"], percentages=False), s["name"])
            out["maskfasta"] = read("masked")
        return out


def assert_text_equals_golden(res, s):
    """every writer of vsearch_amd.mask on a result of set `s` against the reference's recorded text, byte for byte"""
    from vsearch_amd.mask import fasta_lines, fastq_lines, log_lines, maskfasta_lines
    ref, kw, o = s["ref"], writer_kw(s), full_opts(s["opts"])
    assert fasta_lines(res, s["labels"], **kw) == ref["fasta"], s["name"]
    if s["quals"] is not None:
        assert fastq_lines(res, s["labels"], **kw) == ref["fastq"], s["name"]
    else:
        assert ref["fastq"] is None
    assert maskfasta_lines(res, s["labels"], **kw) == ref["maskfasta"], s["name"]
    assert log_lines(res, o["min_unmasked_pct"], o["max_unmasked_pct"]) == ref["log"], s["name"]


INPUT_KEYS = ("name", "seqs", "labels", "quals", "opts")
SHARED_KEYS = ("seqs", "labels", "quals")


def write_golden(path=GOLDEN):
    """a set whose inputs equal an earlier set's (other options on the same input) is stored as a reference to it"""
    sets, stored = [], []
    for s in golden_sets():
        rec = {k: s[k] for k in INPUT_KEYS}
        rec["ref"] = run_reference(s)
        sets.append(rec)
        same = next((t["name"] for t in sets[:-1] if all(t[k] == rec[k] for k in SHARED_KEYS)), None)
        stored.append(dict(name=rec["name"], opts=rec["opts"], same_inputs_as=same, ref=rec["ref"]) if same else rec)
    with open(path, "w") as f:
        json.dump(dict(sets=stored), f, indent=0, separators=(",", ":"))
        f.write("\n")
    return sets


def load_golden(path=GOLDEN):
    with open(path) as f:
        stored = json.load(f)["sets"]
    by_name, sets = {}, []
    for rec in stored:
        if "same_inputs_as" in rec:
            base = by_name[rec["same_inputs_as"]]
            rec = dict({k: base[k] for k in SHARED_KEYS}, name=rec["name"], opts=rec["opts"], ref=rec["ref"])
        by_name[rec["name"]] = rec
        sets.append(rec)
    return sets


def all_sets():
    return load_golden() + [empty_set()]


# ---- calls and comparisons -------------------------------------------------------------------------------------------------------
def call(aligner, s, **extra):
    """the set through vsearch_amd.mask: the device with an aligner, the host restatement without"""
    from vsearch_amd.mask import fastx_mask, fastx_mask_host
    kw = dict(mask_kw(s), **extra)
    if aligner is None:
        return fastx_mask_host(s["seqs"], quals=s["quals"], **kw)
    return fastx_mask(aligner, s["seqs"], quals=s["quals"], **kw)


def assert_same(a, b, what):
    """two MaskResults field for field, text and bits included where both have them"""
    import numpy as np
    fa, fb = a.fields(), b.fields()
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), (what, k, fa[k][:16], fb[k][:16])
    if a.text_blob is not None and b.text_blob is not None:
        assert a.text_blob == b.text_blob, (what, "text")
    if a.bits_blob is not None and b.bits_blob is not None:
        assert a.bits_blob == b.bits_blob, (what, "bits")


def assert_equals_py(res, s):
    """a MaskResult against py_fastx_mask() field for field"""
    import numpy as np
    exp = py_fastx_mask(s["seqs"], **mask_kw(s))
    name = s["name"]
    assert [int(x) for x in res.unmasked] == exp["unmasked"], name
    assert [int(x) for x in res.verdict] == exp["verdict"], name
    assert (res.kept, res.discarded_less, res.discarded_more) == (exp["kept"], exp["discarded_less"], exp["discarded_more"]), name
    assert [t.decode("latin-1") for t in res.text()] == exp["text"], name
    assert np.array_equal(res.bits(), np.array(exp["bits"], bool)), name


def device_digest(aligner, sets=None):
    """SHA-256 over every set's device result; asserts that no sequence took a host route"""
    h = hashlib.sha256()
    for s in sets or all_sets():
        res = call(aligner, s)
        st = res.stats
        assert st["sequences_host_forced"] + st["sequences_host_memory"] + st["sequences_host_long"] == 0, (s["name"], st)
        h.update(s["name"].encode() + b"\0" + res.tobytes())
    return h.hexdigest()


def _child_digest():
    from vsearch_amd import Aligner, _lib
    with Aligner(device=0) as al:
        print(f"digest {device_digest(al)} poison {_lib.load().vsx_internal_poison_byte()}")


def _child_long(segments):
    """every set on the long route (the parent set VSX_MASK_LONG_MIN=1) under each segment length: one line per (segment, set)"""
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        for seg in segments:
            os.environ["VSX_MASK_SEGMENT"] = str(seg)
            for s in all_sets():
                res = call(al, s)
                st = res.stats
                dust = full_opts(s["opts"])["qmask"] == "dust"
                assert st["segment"] == seg and st["long_min"] == 1, st
                filled = sum(1 for x in s["seqs"] if len(x) >= 1)          # (an empty sequence is below any threshold)
                assert (st["sequences_long"], st["sequences_short"]) == ((filled, len(s["seqs"]) - filled) if dust else (0, 0)), (s["name"], st)
                print(f"long {seg} {s['name']} {hashlib.sha256(res.tobytes()).hexdigest()}")


if __name__ == "__main__":
    if "--digest" in sys.argv:
        _child_digest()
    elif "--long" in sys.argv:
        _child_long([int(x) for x in sys.argv[sys.argv.index("--long") + 1].split(",")])
    else:
        for rec in write_golden():
            exp = py_fastx_mask(rec["seqs"], **mask_kw(rec))
            kept = [t for t, v in zip(exp["text"], exp["verdict"]) if v == 0]
            got = [l for l in rec["ref"]["fasta"] if not l.startswith(">")] if full_opts(rec["opts"])["fasta_width"] == 0 else None
            print(f"{rec['name']}: {len(rec['seqs'])} sequences; {' | '.join(rec['ref']['log'])}" + ("" if got is None or got == kept else "   PY DIFFERS"))
