"""Restriction-site cutting: vsx_cut on three shapes of input, each with a six-cutter and with a degenerate pattern.

    python bench_cut.py [--shapes reads,amplicons,chromosomes] [--scale F] [--steps K] [--warmup W] [--no-host] [--no-cli] [--out FILE]

Shapes: 1 000 000 simulated reads of 250 bp; 100 000 sequences of 1 400 bp; 8 sequences of 5 Mbp (uniform random ACGT, one packed
blob).  Patterns: G^AATT_C and GCCNNNN^N_GGC.  Every call asks for both fragment lists and both reverse-complemented texts.
Prints one JSON line (and writes it to --out).  Per shape and pattern: the device call end to end (median of the steps after the
warm-up, all of them listed) with the split and the counters of vsx_cut_last_stats for the median call; the library's host
restatement with 16 threads on the same input with every array and the text compared; where oracle/_ref/vsearch_ref exists, the
reference CLI (one thread, it has no more) on a sample (reading and writing FASTA included) and the SHA-256 of its four files against
ours.  The call starts from spans in memory and the CLI from a file: the times stand side by side, no ratio.  --scale shrinks the
sequence counts for a trial run.  Not measured: hardware counters, scattered input (which is packed on the host first).
"""
import argparse
import hashlib
import importlib
import json
import os
import sys
import time

import numpy as np

from tests import cut_data as cd
from vsearch_amd import Aligner

ct = importlib.import_module("vsearch_amd.cut")
SPLIT = ("seconds_stage", "seconds_h2d", "seconds_match", "seconds_rank", "seconds_fragments", "seconds_emit", "seconds_output", "seconds_total")
COUNTS = ("sequences", "symbols", "blocks", "items", "tile") + cd.HOST_ROUTES
SHAPES = dict(reads=(1000000, 250, 20000), amplicons=(100000, 1400, 5000), chromosomes=(8, 5000000, 1))     # count, length, CLI sample
PATTERNS = ("G^AATT_C", "GCCNNNN^N_GGC")


def simulate(count, length, seed):
    rng = np.random.default_rng(seed)
    blob = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, count * length, dtype=np.uint8)].tobytes()
    return blob, np.arange(count, dtype=np.uint64) * np.uint64(length), np.full(count, length, np.uint32)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        t = time.perf_counter()
        res = fn()
        out.append((time.perf_counter() - t, res))
    out.sort(key=lambda x: x[0])
    return [round(t, 6) for t, _ in out], out[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="reads,amplicons,chromosomes")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    record = dict(bench="cut", steps=a.steps, warmup=a.warmup, scale=a.scale, shapes={})
    with Aligner(device=0) as al:
        for seed, shape in enumerate(a.shapes.split(",")):
            count, length, sample = SHAPES[shape]
            count = max(1, int(count * a.scale))
            seqs = simulate(count, length, 2100 + seed)
            rec = dict(sequences=count, length=length, patterns={})
            for pattern in PATTERNS:
                times, (t_med, res) = timed(lambda: ct.cut(al, seqs, pattern), a.steps, a.warmup)
                st = res.stats
                r = dict(device=dict(seconds=round(t_med, 6), all=times, cut=res.cut, matches=res.total_matches, fragments=[res.n_fwd, res.n_rev],
                                     text_bytes=len(res.text_blob), split={k: round(st[k], 6) for k in SPLIT}, counts={k: st[k] for k in COUNTS}))
                if not a.no_host:
                    htimes, (h_med, hres) = timed(lambda: ct.cut_host(seqs, pattern, threads=16), 3, 0)
                    r["host"] = dict(seconds=round(h_med, 6), all=htimes, threads=16, equal=hres.tobytes() == res.tobytes())
                if os.path.exists(cd.ref_binary()) and not a.no_cli:
                    S = min(sample, count)
                    part = [seqs[0][k * length:(k + 1) * length].decode() for k in range(S)]
                    s = cd._set("bench", part, pattern, labels=[f"q{k}" for k in range(S)])
                    t = time.perf_counter()
                    ref = cd.run_cli(s)
                    t_cli = time.perf_counter() - t
                    ours = ct.cut(al, part, pattern)
                    same = all(hashlib.sha256(ref[w].encode("latin-1")).hexdigest() == cd.sha(cd.lib_text(ours, s, w)) for w in cd.WHICH)
                    r["cli"] = dict(sample=S, seconds=round(t_cli, 4), threads=1, matches=ours.total_matches, parity_sample_match=same,
                                    log_match=ct.log_lines(ours) == [ref["log"]])
                rec["patterns"][pattern] = r
                print(f"{shape} {pattern}: device {r['device']['seconds']} s", file=sys.stderr, flush=True)
            record["shapes"][shape] = rec
    line = json.dumps(record, separators=(",", ":"))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
