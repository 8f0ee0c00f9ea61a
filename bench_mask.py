"""Masking throughput: vsx_fastx_mask (DUST, soft text out) on three inputs, and the two device routes against each other.

    python bench_mask.py [--reads N] [--refs D] [--genome L] [--cli-sample S] [--steps K] [--warmup W] [--no-host] [--out FILE]

Inputs: N simulated reads of 250 bp and D reference-like sequences of 1 400 bp, random text in which every tenth sequence carries a
low-complexity island (a repeat of a 1 .. 4-mer over 20 .. 60 symbols); one sequence of L symbols with an island about every 2 000.
Prints one JSON line (and writes it to --out).  Per input: the device call end to end (median of the steps, all of them listed,
the masked text and the bitmap returned) with the split of vsx_fastx_mask_last_stats for the median call; the library's host
restatement (VSX_MASK=host, all usable CPUs) on the same input with every array compared; where oracle/_ref/vsearch_ref exists, the
reference CLI's --maskfasta with one thread on the first S sequences (reading and writing FASTA included; --fastx_mask takes no
--maxseqlength, so it could not read the long sequence) and the sha256 of its --output against ours.  The call starts from a blob in memory and the CLI from a file: the times stand side by side, no ratio.
`routes`: one sequence of 10 k .. L symbols on the long route (a window at every position, the chain by segments) and on the short
route (one wavefront walks the sequence), VSX_MASK_LONG_MIN set for the call, results compared; and a batch of 1 000 sequences of
20 000 symbols both ways, where the short route has a wave per sequence and the long route launches per sequence.
"""
import argparse
import hashlib
import json
import os
import subprocess
import tempfile
import time

import numpy as np

from oracle import refcli
from tests import fastx_mask_data as md
from vsearch_amd import Aligner
from vsearch_amd.mask import fastx_mask, fastx_mask_host, maskfasta_lines

LETTERS = np.frombuffer(b"ACGT", np.uint8)
SPLIT = ("seconds_stage", "seconds_h2d", "seconds_mask", "seconds_apply", "seconds_d2h_output")
COUNTS = ("sequences_short", "sequences_long", "windows", "dust_windows", "long_min", "segment")
NEVER = 1 << 32                       # a route threshold no sequence reaches


def island(rng, n):
    unit = LETTERS[rng.integers(0, 4, int(rng.integers(1, 5)))]
    return np.resize(unit, n)


def simulate(seed, count, length, every=10):
    """count rows of `length` random symbols; every `every`-th row carries one island"""
    rng = np.random.default_rng(seed)
    rows = LETTERS[rng.integers(0, 4, (count, length), dtype=np.uint8)]
    for k in range(0, count, every):
        n = int(rng.integers(20, 61))
        at = int(rng.integers(0, length - n))
        rows[k, at:at + n] = island(rng, n)
    return rows


def genome(seed, length):
    rng = np.random.default_rng(seed)
    row = LETTERS[rng.integers(0, 4, length, dtype=np.uint8)]
    at = 0
    while True:
        at += int(rng.integers(1000, 3000))
        n = int(rng.integers(20, 200))
        if at + n >= length:
            return row
        row[at:at + n] = island(rng, n)


def as_input(rows):
    rows = np.atleast_2d(rows)
    n, length = rows.shape
    return rows.tobytes(), np.arange(n, dtype=np.uint64) * np.uint64(length), np.full(n, length, np.uint32)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        res = fn()
        out.append((time.perf_counter() - t0, res))
    out.sort(key=lambda x: x[0])
    return [round(t, 6) for t, _ in out], out[len(out) // 2]


def with_env(name, value, fn):
    old = os.environ.get(name)
    os.environ[name] = str(value)
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def device_record(al, inp, steps, warmup, long_min=None):
    call = lambda: fastx_mask(al, inp)
    fn = call if long_min is None else (lambda: with_env("VSX_MASK_LONG_MIN", long_min, call))
    all_s, (median, res) = timed(fn, steps, warmup)
    st = res.stats
    assert st["sequences_host_forced"] + st["sequences_host_memory"] + st["sequences_host_long"] == 0, st
    rec = dict(seconds=round(median, 6), seconds_all=all_s, symbols_per_second=round(len(inp[0]) / median))
    rec.update({k: round(st[k], 6) for k in SPLIT})
    rec.update({k: int(st[k]) for k in COUNTS})
    return rec, res


def cli_record(rows, sample, device_sample):
    names = [f"s{k}" for k in range(sample)]
    with tempfile.TemporaryDirectory(prefix="vsx_bench_mask_") as tmp:
        src, dst = os.path.join(tmp, "in.fa"), os.path.join(tmp, "out.fa")
        with open(src, "wb") as f:
            for name, row in zip(names, rows[:sample]):
                f.write(b">" + name.encode() + b"\n" + row.tobytes() + b"\n")
        t0 = time.perf_counter()
        r = subprocess.run([md.ref_binary(), "--maskfasta", src, "--output", dst, "--qmask", "dust", "--threads", "1", "--fasta_width", "0",
                            "--maxseqlength", str(max(50000, rows.shape[1])), "--quiet"], capture_output=True, text=True)
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        theirs = hashlib.sha256(open(dst, "rb").read()).hexdigest()
    ours = hashlib.sha256(("\n".join(maskfasta_lines(device_sample, names, fasta_width=0)) + "\n").encode()).hexdigest()
    return dict(sample=sample, threads=1, seconds=round(dt, 4), parity_sample_match=ours == theirs)


def bench_input(al, name, rows, args):
    inp = as_input(rows)
    rec = dict(sequences=len(inp[2]), symbols=len(inp[0]))
    rec["device"], res = device_record(al, inp, args.steps, args.warmup)
    rec["masked_symbols"] = int(res.bits().sum())
    if not args.no_host:
        t0 = time.perf_counter()
        ref = fastx_mask_host(inp)
        rec["host"] = dict(seconds=round(time.perf_counter() - t0, 6), threads=refcli.usable_cpus(), equal=ref.tobytes() == res.tobytes())
        assert rec["host"]["equal"], name
    if os.path.exists(md.ref_binary()) and args.cli_sample:
        sample = min(args.cli_sample, len(inp[2]))
        rec["cli"] = cli_record(np.atleast_2d(rows), sample, fastx_mask(al, as_input(np.atleast_2d(rows)[:sample])))
    return rec


def bench_routes(al, row, args):
    out = []
    lengths = [n for n in (10000, 30000, 100000, 300000, 1000000) if n < len(row)] + [len(row)]
    for n in lengths:
        inp = as_input(row[:n])
        long_rec, a = device_record(al, inp, 3, 1, long_min=1)
        short_rec, b = device_record(al, inp, 3, 1, long_min=NEVER)
        assert long_rec["sequences_long"] == 1 and short_rec["sequences_short"] == 1 and a.tobytes() == b.tobytes(), n
        out.append(dict(length=n, long=long_rec, short=short_rec))
    rows = simulate(args.seed + 3, 1000, 20000)
    inp = as_input(rows)
    long_rec, a = device_record(al, inp, 3, 1, long_min=1)
    short_rec, b = device_record(al, inp, 3, 1, long_min=NEVER)
    assert a.tobytes() == b.tobytes()
    return dict(single=out, batch_1000x20000=dict(long=long_rec, short=short_rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--refs", type=int, default=100000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--cli-sample", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rec = dict(bench="mask", qmask="dust", hardmask=0)
    row = genome(args.seed + 2, args.genome)
    with Aligner(device=0) as al:
        rec["reads_250"] = bench_input(al, "reads", simulate(args.seed, args.reads, 250), args)
        rec["refs_1400"] = bench_input(al, "refs", simulate(args.seed + 1, args.refs, 1400), args)
        rec["genome"] = bench_input(al, "genome", row, args)
        rec["routes"] = bench_routes(al, row, args)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
