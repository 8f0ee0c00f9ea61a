"""Extraction by label: vsx_getseqs on one million simulated headers, four runs of the pipeline's kind and a sweep over the number
of distinct label lengths.

    python bench_getseqs.py [--reads N] [--cli-sample S] [--steps K] [--warmup W] [--no-host] [--out FILE]

Input: N headers of the pipeline's form, read<k>;sample=S<0..95>;size=<1..50>, of which a tenth are OTU_<0..19999> instead.
Runs: LABELS exact with 10 000 names; LABELS + substr with 10 000 names; WORDS + field with 96 sample names; WORD + field with one
name; and LABELS + substr with lists of D = 1, 10, 100, 1 000 distinct lengths (one label per length, none of which occurs).
Prints one JSON line (and writes it to --out).  Per run: the device call end to end (median of the steps, all of them listed) with
the split and the counters of vsx_getseqs_last_stats for the median call; the library's host restatement on the same input with
every array compared; where oracle/_ref/vsearch_ref exists, the reference CLI with one thread on the first S reads (reading and
writing FASTA included) and the sha256 of its --fastaout and --notmatched against ours.  The call starts from spans in memory and
the CLI from a file: the times stand side by side, no ratio.  Not measured: hardware counters, headers of kilobytes.
"""
import argparse
import hashlib
import importlib
import json
import os
import statistics
import time

import numpy as np

from tests import getseqs_data as gd
from vsearch_amd import Aligner

gs = importlib.import_module("vsearch_amd.getseqs")
SPLIT = ("seconds_stage", "seconds_table", "seconds_match", "seconds_ordinals", "seconds_output")
COUNTS = ("labels_in_table", "distinct_lengths", "table_slots", "probes", "verifications", "headers_device", "headers_host")


def simulate(n, seed=20):
    rng = np.random.default_rng(seed)
    sample, size, otu, kind = rng.integers(0, 96, n), rng.integers(1, 51, n), rng.integers(0, 20000, n), rng.integers(0, 10, n)
    return [(b"OTU_%d" % otu[k]) if kind[k] == 0 else (b"read%d;sample=S%d;size=%d" % (k, sample[k], size[k])) for k in range(n)]


def runs():
    names = [b"OTU_%d" % k for k in range(0, 20000, 2)]
    yield "labels_exact_10000", "labels", names, {}
    yield "labels_substr_10000", "labels", names, dict(substr=True)
    yield "words_field_96", "label_words", [b"S%d" % k for k in range(0, 192, 2)], dict(field="sample")
    yield "word_field_1", "label_word", b"S17", dict(field="sample")
    for d in (1, 10, 100, 1000):
        yield "lengths_sweep_%d" % d, "labels", [b"Q" + b"w" * k for k in range(1, d + 1)], dict(substr=True)


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


def sha(lines):
    return hashlib.sha256("".join(l + "\n" for l in lines).encode("latin-1")).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--cli-sample", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    heads = gs.LabelBlob(simulate(a.reads))
    lens = np.full(a.reads, 250, np.uint32)
    record = dict(bench="getseqs", reads=a.reads, steps=a.steps, warmup=a.warmup, header_bytes=len(heads.blob), runs={})
    with Aligner(device=0) as al:
        for name, mode, needles, kw in runs():
            N = gs.LabelBlob(needles) if isinstance(needles, list) else needles
            times, (t_med, res) = timed(lambda: gs.getseqs(al, heads, lens, mode, N, **kw), a.steps, a.warmup)
            st = res.stats
            r = dict(device=dict(seconds=t_med, all=times, kept=res.kept, split={k: round(st[k], 6) for k in SPLIT}, counts={k: st[k] for k in COUNTS}))
            if not a.no_host:
                htimes, (h_med, hres) = timed(lambda: gs.getseqs_host(heads, lens, mode, N, threads=16, **kw), 3, 0)
                r["host"] = dict(seconds=h_med, all=htimes, threads=16, equal=hres.arrays() == res.arrays(), split={k: round(hres.stats[k], 6) for k in SPLIT})
            if os.path.exists(gd.ref_binary()) and a.cli_sample:
                S = min(a.cli_sample, a.reads)
                raw = heads.blob
                hs = [raw[int(o):int(o) + int(l)] for o, l in zip(heads.offsets[:S], heads.lengths[:S])]
                seqs, quals = ["ACGT" * 5] * S, ["I" * 20] * S
                single = mode in gd.SINGLE
                t = time.perf_counter()
                ref = gd.run_cli(hs, seqs, quals, mode, [needles] if single else needles, None, kw.get("substr", False), kw.get("field"), None,
                                 gd.WRITER_DEFAULTS)
                t_cli = time.perf_counter() - t
                ours = gs.getseqs(al, hs, [20] * S, mode, N, **kw)
                same = all(hashlib.sha256(ref[f]).hexdigest() == sha(gs.fasta_lines(ours, hs, seqs, f == "fastaout")) for f in ("fastaout", "notmatched"))
                r["cli"] = dict(sample=S, seconds=round(t_cli, 4), threads=1, kept=ours.kept, parity_sample_match=same)
            record["runs"][name] = r
    line = json.dumps(record, separators=(",", ":"))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
