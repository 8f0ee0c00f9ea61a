"""SINTAX throughput: vsx_sintax on simulated 250 bp reads against a simulated 16S-like reference set, both strands.

    python bench_sintax.py [--db D] [--reads N] [--cli-sample S] [--steps K] [--warmup W] [--out FILE]

Workload: D reference sequences of about 1 400 bp with a nine-rank taxonomy -- D / 20 genera, each 12 % from a common ancestor,
twenty members per genus 2 % from their genus (four species of five strains) -- and N reads of 250 bp cut from them with 1 %
substitutions, half reverse-complemented; --strand both, word length 8.  Prints one JSON line (and writes it to --out): the
session and index build on their own, then per call the seconds end to end (median of the steps, all of them listed), reads/s and
the split of vsx_sintax_last_stats for the median call: staging (host word lists and uploads), sample, count/select, vote
(kernel times from events) and output.  Where oracle/_ref/vsearch_ref exists: the reference CLI's --sintax on the first S reads
against the same database with 1 thread and with 16 threads (reading both FASTA files and building its index included, as the
command does them), and a parity digest: sha256 of the sorted --tabbedout lines of that sample, ours against the CLI's.  The call
starts from blobs in memory and the CLI from files: the two times are printed side by side, not as a ratio.
"""
import argparse
import hashlib
import json
import os
import subprocess
import tempfile
import time

import numpy as np

from tests import sintax_data as sd
from vsearch_amd import Aligner, SearchSession, sintax, tabbed_lines

READ_LENGTH, REF_LENGTH, GENUS_SIZE = 250, 1400, 20
LETTERS = np.frombuffer(b"ACGT", np.uint8)


def mutated(rng, rows, rate):
    out = rows.copy()
    hit = rng.random(rows.shape) < rate
    out[hit] = (out[hit] + rng.integers(1, 4, int(hit.sum()), dtype=np.uint8)) & 3
    return out


def simulate(seed, n_db, n_reads):
    """-> (database rows, their labels, read rows) -- rows as uint8 arrays of ASCII symbols"""
    rng = np.random.default_rng(seed)
    n_genera = max(1, n_db // GENUS_SIZE)
    ancestor = rng.integers(0, 4, (1, REF_LENGTH), dtype=np.uint8)
    genera = mutated(rng, np.repeat(ancestor, n_genera, axis=0), 0.12)
    genus_of = np.arange(n_db) % n_genera
    db = mutated(rng, genera[genus_of], 0.02)
    labels = []
    for i in range(n_db):
        g, m = int(genus_of[i]), i // n_genera
        labels.append(f"r{i};tax=d:Bacteria,k:K{g % 3},p:P{g % 40},c:C{g % 160},o:O{g % 640},f:F{g // 4},g:G{g},s:S{g}_{m // 5},t:T{i};")
    src = rng.integers(0, n_db, n_reads)
    at = rng.integers(0, REF_LENGTH - READ_LENGTH, n_reads)
    reads = mutated(rng, db[src[:, None], at[:, None] + np.arange(READ_LENGTH)[None, :]], 0.01)
    minus = rng.random(n_reads) < 0.5
    reads[minus] = 3 - reads[minus][:, ::-1]
    return LETTERS[db], labels, LETTERS[reads]


def digest(lines):
    h = hashlib.sha256()
    for line in sorted(lines):
        h.update(line.encode() + b"\n")
    return h.hexdigest()


def fasta(path, names, rows):
    with open(path, "wb") as f:
        for name, row in zip(names, rows):
            f.write(b">" + name.encode() + b"\n" + row.tobytes() + b"\n")


def run_cli(db_path, q_path, out_path, seed, threads):
    args = [sd.ref_binary(), "--sintax", q_path, "--db", db_path, "--tabbedout", out_path, "--strand", "both", "--randseed", str(seed),
            "--sintax_cutoff", "0.8", "--threads", str(threads), "--quiet"]
    t0 = time.perf_counter()
    r = subprocess.run(args, capture_output=True, text=True)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    return dt, open(out_path).read().split("\n")[:-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db", type=int, default=100000)
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--cli-sample", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    db_rows, labels, read_rows = simulate(a.seed, a.db, a.reads)
    db = [r.tobytes() for r in db_rows]
    blob = read_rows.tobytes()
    off = np.arange(a.reads, dtype=np.uint64) * READ_LENGTH
    lens = np.full(a.reads, READ_LENGTH, np.uint32)
    qnames = [f"read{k}" for k in range(a.reads)]
    rec = dict(bench="sintax", db=a.db, db_length=REF_LENGTH, reads=a.reads, read_length=READ_LENGTH, strand="both", wordlength=8,
               randseed=a.seed, steps=a.steps, warmup=a.warmup)
    with Aligner(device=0) as al:
        t0 = time.perf_counter()
        sess = SearchSession(al, db, labels=labels, id=0.97, soft_mask=1)
        rec["seconds_session"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        first = sintax(sess, (blob[:READ_LENGTH * 64], off[:64], lens[:64]), randseed=a.seed, strand_both=True)
        rec["seconds_first_call_with_index"] = time.perf_counter() - t0
        rec["seconds_index"] = first.stats["seconds_index"]
        calls = []
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            res = sintax(sess, (blob, off, lens), randseed=a.seed, strand_both=True)
            dt = time.perf_counter() - t0
            if step >= a.warmup:
                calls.append((dt, res.stats))
        order = sorted(range(len(calls)), key=lambda k: calls[k][0])
        med_dt, med = calls[order[len(order) // 2]]
        rec["seconds_all"] = [round(c[0], 4) for c in calls]
        rec["seconds"] = med_dt
        rec["reads_per_second"] = a.reads / med_dt
        rec["split"] = {k: med[k] for k in ("seconds_stage", "seconds_sample", "seconds_count", "seconds_vote", "seconds_output", "seconds_total")}
        rec["counters"] = {k: med[k] for k in ("queries_device", "windows", "strands_sampled", "rounds_counted", "tiles")}
        rec["classified"] = res.n_classified
        rec["sets_the_time"] = max(("seconds_stage", "seconds_sample", "seconds_count", "seconds_vote", "seconds_output"), key=lambda k: med[k])
        if a.cli_sample and os.path.exists(sd.ref_binary()):
            n = min(a.cli_sample, a.reads)
            ours = sintax(sess, (blob[:READ_LENGTH * n], off[:n], lens[:n]), randseed=a.seed, strand_both=True)
            ours_lines = tabbed_lines(ours, qnames[:n], labels, 0.8)
            with tempfile.TemporaryDirectory(prefix="vsx_bench_sintax_") as tmp:
                p = lambda x: os.path.join(tmp, x)
                fasta(p("db.fa"), labels, db_rows)
                fasta(p("q.fa"), qnames[:n], read_rows[:n])
                cli = {}
                for threads in (1, 16):
                    dt, lines = run_cli(p("db.fa"), p("q.fa"), p(f"out{threads}.tsv"), a.seed, threads)
                    cli[f"seconds_threads_{threads}"] = dt
                    cli[f"digest_threads_{threads}"] = digest(lines)
                cli.update(sample=n, digest_ours=digest(ours_lines), parity=all(cli[f"digest_threads_{t}"] == digest(ours_lines) for t in (1, 16)),
                           note="the CLI reads two FASTA files and builds its index inside the time; no ratio is claimed")
                rec["reference_cli"] = cli
        sess.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
