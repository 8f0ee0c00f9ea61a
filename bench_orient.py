"""Orientation throughput: vsx_orient on simulated 250 bp reads, half of them reverse-complemented, against a simulated 16S-like
reference set, at the command's default word length 12, with the oriented text returned.

    python bench_orient.py [--db D] [--reads N] [--cli-sample S] [--steps K] [--warmup W] [--no-host] [--out FILE]

Workload: bench_sintax.py's (D reference sequences of about 1 400 bp in genera, N reads of 250 bp cut from them with 1 %
substitutions, half reverse-complemented).  Prints one JSON line (and writes it to --out): the session, the match-count table
build once (first call), then per call the seconds end to end (median of the steps, all of them listed), reads/s and the split of
vsx_orient_last_stats for the median call: staging (packing and uploads), the count kernel and the emit kernel (from events) and
output (downloads and the copies to the caller's offsets).  Next to it the library's own host restatement
(vsx_internal_orient_host, all usable CPUs) on the same input, table build and per-read work apart.  Where oracle/_ref/vsearch_ref
exists: the reference CLI's --orient with one thread on the first S reads (reading both FASTA files and building its index
included, as the command does them) and a parity digest: sha256 of the sorted --tabbedout lines of that sample, ours against the
CLI's.  The call starts from blobs in memory and the CLI from files: the two times are printed side by side, not as a ratio.
"""
import argparse
import json
import os
import subprocess
import tempfile
import time

import numpy as np

from bench_sintax import LETTERS, READ_LENGTH, REF_LENGTH, digest, fasta, mutated, simulate
from tests import orient_data as od
from vsearch_amd import Aligner
from vsearch_amd.orient import orient, orient_host, orient_session, tabbed_lines

SPLIT = ("seconds_stage", "seconds_count", "seconds_emit", "seconds_output")


def simulate_reads(seed, db_rows, n_reads, step=100000):
    """bench_sintax.py's reads (1 % substitutions, half reverse-complemented), drawn in blocks so that a million fit in memory"""
    rng = np.random.default_rng(seed + 1)
    codes = np.searchsorted(LETTERS, db_rows).astype(np.uint8)
    out = np.empty((n_reads, READ_LENGTH), np.uint8)
    for k0 in range(0, n_reads, step):
        n = min(step, n_reads - k0)
        src = rng.integers(0, len(db_rows), n)
        at = rng.integers(0, REF_LENGTH - READ_LENGTH, n)
        reads = mutated(rng, codes[src[:, None], at[:, None] + np.arange(READ_LENGTH)[None, :]], 0.01)
        minus = rng.random(n) < 0.5
        reads[minus] = 3 - reads[minus][:, ::-1]
        out[k0:k0 + n] = LETTERS[reads]
    return out


def same_answer(a, b):
    return bool(all(np.array_equal(a.fields()[k], b.fields()[k]) for k in a.fields()) and a.text_blob == b.text_blob)


def run_cli(db_path, q_path, out_path, threads):
    args = [od.ref_binary(), "--orient", q_path, "--db", db_path, "--tabbedout", out_path, "--threads", str(threads), "--quiet"]
    t0 = time.perf_counter()
    r = subprocess.run(args, capture_output=True, text=True)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    return dt, open(out_path).read().split("\n")[:-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db", type=int, default=100000)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--cli-sample", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    db_rows, labels, _ = simulate(a.seed, a.db, 0)
    read_rows = simulate_reads(a.seed, db_rows, a.reads)
    db = [r.tobytes() for r in db_rows]
    blob = read_rows.tobytes()
    off = np.arange(a.reads, dtype=np.uint64) * READ_LENGTH
    lens = np.full(a.reads, READ_LENGTH, np.uint32)
    rec = dict(bench="orient", db=a.db, db_length=REF_LENGTH, reads=a.reads, read_length=READ_LENGTH, wordlength=12, want_text=1,
               dbmask="dust", qmask="dust", steps=a.steps, warmup=a.warmup)
    with Aligner(device=0) as al:
        t0 = time.perf_counter()
        sess = orient_session(al, db, soft_mask=2)
        rec["seconds_session"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        first = orient(sess, (blob[:READ_LENGTH * 64], off[:64], lens[:64]))
        rec["seconds_first_call_with_build"] = time.perf_counter() - t0
        rec["build"] = {k: first.stats[k] for k in ("seconds_build", "build_chunks", "build_keys")}
        calls = []
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            res = orient(sess, (blob, off, lens))
            dt = time.perf_counter() - t0
            if step >= a.warmup:
                calls.append((dt, res.stats))
        order = sorted(range(len(calls)), key=lambda k: calls[k][0])
        med_dt, med = calls[order[len(order) // 2]]
        rec["seconds_all"] = [round(c[0], 4) for c in calls]
        rec["seconds"] = med_dt
        rec["reads_per_second"] = a.reads / med_dt
        rec["split"] = {k: med[k] for k in SPLIT + ("seconds_total",)}
        rec["counters"] = {k: med[k] for k in ("queries_device", "queries_class", "windows", "words_distinct")}
        rec["verdicts"] = dict(fwd=res.n_fwd, rev=res.n_rev, none=res.n_none)
        rec["sets_the_time"] = max(SPLIT, key=lambda k: med[k])
        # the count kernel gathers two table entries per distinct word: the rate at which the 64 MB table answers random 4-byte reads
        rec["table_gathers_per_second"] = 2 * med["words_distinct"] / med["seconds_count"] if med["seconds_count"] > 0 else None
        if not a.no_host:
            t0 = time.perf_counter()
            host = orient_host(db, (blob, off, lens), soft_mask=2)
            rec["host_restatement"] = dict(seconds=time.perf_counter() - t0, seconds_build=host.stats["seconds_build"],
                                           seconds_reads=host.stats["seconds_count"], seconds_total=host.stats["seconds_total"],
                                           equal=same_answer(host, res),
                                           note="seconds_total also holds the DUST masking of the database text, which the session did for the device")
        if a.cli_sample and os.path.exists(od.ref_binary()):
            n = min(a.cli_sample, a.reads)
            qnames = [f"read{k}" for k in range(n)]
            ours = orient(sess, (blob[:READ_LENGTH * n], off[:n], lens[:n]))
            ours_digest = digest(tabbed_lines(ours, qnames))
            with tempfile.TemporaryDirectory(prefix="vsx_bench_orient_") as tmp:
                p = lambda x: os.path.join(tmp, x)
                fasta(p("db.fa"), labels, db_rows)
                fasta(p("q.fa"), qnames, read_rows[:n])
                dt, lines = run_cli(p("db.fa"), p("q.fa"), p("out.tsv"), 1)
            rec["reference_cli"] = dict(sample=n, seconds_threads_1=dt, digest_threads_1=digest(lines), digest_ours=ours_digest,
                                        parity=digest(lines) == ours_digest,
                                        note="the CLI reads two FASTA files and builds its index inside the time; no ratio is claimed")
        sess.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
