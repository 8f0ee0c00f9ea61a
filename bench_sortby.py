"""Abundance and length sorting: vsx_sortby on simulated dereplicated amplicon headers and on shallow random labels.

    python bench_sortby.py [--inputs illumina,random16] [--n 1000000] [--steps K] [--warmup W] [--no-host] [--no-python] [--no-cli] [--out FILE]

Inputs: `illumina` -- n Illumina-style headers with ;size= and about 70 % singletons (the deep case: the names share 25 to 40 leading
bytes), sorted by VSX_SORTBY_SIZE and by VSX_SORTBY_LENGTH; `random16` -- n random 16-byte labels, all singletons (the shallow case),
by VSX_SORTBY_SIZE.  Prints one JSON line (and writes it to --out).  Per input and order: the device call end to end from arrays in
memory (median of the steps after the warm-up, all of them listed) with the seconds per stage, the rounds and the active items per
round of vsx_sortby_last_stats for the median call; the library's host restatement with 16 threads on the same input, every array
compared; sort_by_abundance (the Python sort the chimera sessions used) on the same input with the order compared; where
oracle/_ref/vsearch_ref exists, the reference CLI's --sortbysize (one thread) on a 100 000-header sample, FASTA reading and writing
included, with the SHA-256 of its --output against ours.  The call starts from arrays in memory and the CLI from a file: the times
stand side by side, no ratio.  Last, the sort step of a DenovoChimeraSession on bench_uchime_denovo.py's input: sort_by_abundance
(what the session called before) beside the device call it makes now.  Not measured: hardware counters, labels of kilobytes, 10^7
items.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

from tests import sortby_data as sd
from vsearch_amd import Aligner
from vsearch_amd import sortby as sb
from vsearch_amd.chimera import _abundance_order, header_size, sort_by_abundance

SPLIT = ("seconds_stage", "seconds_h2d", "seconds_numeric", "seconds_refine", "seconds_host_finish", "seconds_output", "seconds_total")
COUNTS = ("items", "kept", "label_bytes", "rounds", "active_numeric", "active", "capped_items") + sd.HOST_ROUTES
CLI_SAMPLE = 100000


def illumina(n, seed):
    """headers like M01234:56:000000000-ABCDE:1:1101:15589:1332;size=3 -- about 70 % singletons, the rest 2 .. 1 000 (Zipf-like)"""
    rng = np.random.default_rng(seed)
    lane, tile = rng.integers(1, 3, n), rng.choice((1101, 1102, 1103, 2101, 2102), n)
    x, y = rng.integers(1000, 30000, n), rng.integers(1000, 30000, n)
    sizes = np.where(rng.random(n) < 0.7, 1, np.minimum(1000, 1 + rng.zipf(1.5, n))).astype(np.uint32)
    labels = [f"M01234:56:000000000-ABCDE:{lane[k]}:{tile[k]}:{x[k]}:{y[k]}" + ("" if sizes[k] == 1 else f";size={sizes[k]}") for k in range(n)]
    return labels, sizes, rng.integers(240, 254, n).astype(np.uint32)


def random16(n, seed):
    rng = np.random.default_rng(seed)
    raw = rng.integers(ord("a"), ord("z") + 1, (n, 16), dtype=np.uint8)
    return [bytes(r).decode() for r in raw], np.ones(n, np.uint32), np.full(n, 250, np.uint32)


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
    ap.add_argument("--inputs", default="illumina,random16")
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-python", action="store_true")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    record = dict(bench="sortby", n=a.n, steps=a.steps, warmup=a.warmup, inputs={})
    with Aligner(device=0) as al:
        for seed, name in enumerate(a.inputs.split(",")):
            labels, sizes, lengths = dict(illumina=illumina, random16=random16)[name](a.n, 3400 + seed)
            triple = sb._labels(labels)                                  # the blob / offsets / lengths the C call takes, built once
            rec = dict(label_bytes=len(triple[0]), singletons=round(float(np.mean(sizes == 1)), 3), orders={})
            for order in (("size", "length") if name == "illumina" else ("size",)):
                times, (t_med, res) = timed(lambda: sb.sortby(al, triple, lengths, sizes, order), a.steps, a.warmup)
                st = res.stats
                r = dict(device=dict(seconds=round(t_med, 6), all=times, median=res.median, split={k: round(st[k], 6) for k in SPLIT},
                                     counts={k: st[k] for k in COUNTS}))
                if not a.no_host:
                    htimes, (h_med, hres) = timed(lambda: sb.sortby_host(triple, lengths, sizes, order, threads=16), 3, 0)
                    r["host"] = dict(seconds=round(h_med, 6), all=htimes, threads=16, equal=hres.tobytes() == res.tobytes())
                if not a.no_python and order == "size":
                    plain = [int(v) for v in sizes]
                    t = time.perf_counter()
                    py = sort_by_abundance(plain, labels)
                    r["sort_by_abundance"] = dict(seconds=round(time.perf_counter() - t, 4), equal=py == [int(k) for k in res.order])
                if os.path.exists(sd.ref_binary()) and not a.no_cli and order == "size":
                    S = min(CLI_SAMPLE, a.n)
                    s = sd._set("bench", labels[:S], "size", seqs=["ACGT"] * S)
                    t = time.perf_counter()
                    ref = sd.run_cli(s)
                    t_cli = time.perf_counter() - t
                    ours = sd.call(al, s)
                    r["cli"] = dict(sample=S, seconds=round(t_cli, 4), threads=1, parity_sample_match=sd.sha(ref["output"]) == sd.sha(sd.lib_text(ours, s)),
                                    log_match=sb.log_lines(ours) == [ref["log"]])
                rec["orders"][order] = r
                print(f"{name} {order}: device {r['device']['seconds']} s, rounds {st['rounds']}", file=sys.stderr, flush=True)
            record["inputs"][name] = rec
        # the sort step of DenovoChimeraSession on bench_uchime_denovo.py's input
        import bench_uchime_denovo
        labels, seqs = bench_uchime_denovo.workload(20000)
        sizes, lengths = [header_size(l) for l in labels], [len(x) for x in seqs]
        before, (b_med, b_res) = timed(lambda: sort_by_abundance(sizes, labels), a.steps, a.warmup)
        after, (a_med, a_res) = timed(lambda: _abundance_order(al, sizes, labels, lengths), a.steps, a.warmup)
        record["denovo_sort_step"] = dict(sequences=len(labels), sort_by_abundance=round(b_med, 6), device=round(a_med, 6), equal=b_res == a_res)
    line = json.dumps(record, separators=(",", ":"))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
