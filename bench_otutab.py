"""OTU table throughput: vsx_otutab on the labels and first hits of a finished search.

    python bench_otutab.py [--queries N] [--targets T] [--samples S] [--cli-sample C] [--steps K] [--warmup W] [--out FILE]

Workload: N query labels (default 4 000 000) over S samples (96), half of the samples named by ;sample= and half by the label's
first word, every label with a ;size= annotation (--sizein); T targets (20 000), a part of them with otu= and a part with tax=;
hits drawn with a long tail (Pareto), so a few cells are hot; 5 % of the queries without a hit; the targets no query hit enter
through the unmatched pass.  Prints one JSON line (and writes it to --out): per call the seconds end to end (median of the steps,
all of them listed), labels/s, the seconds split and counters of vsx_otutab_last_stats for the median call -- the scan kernel is
`seconds_scan` -- the table's size; the library's host restatement on the same input with 16 threads, with the equality of every
result array asserted, and which route is faster end to end; and, where oracle/_ref/vsearch_ref exists, the reference CLI's
--search_exact --otutabout with one thread on the first C queries (each an exact copy of its target's sequence; FASTA parsing and the
search included) with a parity digest: sha256 of the --otutabout text, ours against the CLI's.  The call starts from labels and hits
in memory and the CLI from files: no ratio is claimed.
"""
import argparse
import hashlib
import importlib
import json
import os
import tempfile
import time

import numpy as np

from oracle import refcli
from vsearch_amd import Aligner

ot = importlib.import_module("vsearch_amd.otutab")
NONE = ot.NONE


def simulate(seed, nq, nt, ns):
    rng = np.random.default_rng(seed)
    t = []
    for j in range(nt):
        l = "otu%d" % j
        if j % 3 == 0:
            l = "ref%d;otu=OTU_%d" % (j, j // 2 if j % 30 == 0 else j)
        if j % 4 == 0:
            l += ";tax=d:Bacteria,p:P%d,g:G%d" % (j % 40, j)
        t.append((l + (";" if j % 2 else "")).encode())
    sample = rng.integers(0, ns, nq)
    size = rng.choice(np.array([1, 1, 1, 2, 3, 8, 120], np.uint64), nq)
    q_target = np.minimum(rng.pareto(0.6, nq), nt - 1).astype(np.uint32)
    q_target[rng.random(nq) < 0.05] = NONE
    q = [(b"S%d.%d;size=%d" % (s, k, a)) if s % 2 else (b"read%d;sample=S%d;size=%d" % (k, s, a)) for k, (s, a) in enumerate(zip(sample.tolist(), size.tolist()))]
    matched = np.zeros(nt, np.uint8)
    matched[q_target[q_target != NONE]] = 1
    return ot.LabelBlob(q), ot.LabelBlob(t), q_target, size, matched, q, t


def cli_sample(q, t, q_target, size, n, seed):
    """the reference CLI on the first n queries -> (seconds, sha256 of its --otutabout, sha256 of ours, labels/s)"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    db = [bytes(r) for r in letters[rng.integers(0, 4, (len(t), 100))]]
    miss = [bytes(r) for r in letters[rng.integers(0, 4, (n, 100))]]
    qs = [db[int(x)] if x != NONE else miss[k] for k, x in enumerate(q_target[:n].tolist())]
    matched = np.zeros(len(t), np.uint8)
    matched[q_target[:n][q_target[:n] != NONE]] = 1
    with tempfile.TemporaryDirectory(prefix="vsx_otutab_bench_") as tmp:
        refcli.write_fasta(os.path.join(tmp, "db.fa"), [l.decode() for l in t], db)
        refcli.write_fasta(os.path.join(tmp, "q.fa"), [l.decode() for l in q[:n]], qs)
        secs = refcli.run(["--search_exact", os.path.join(tmp, "q.fa"), "--db", os.path.join(tmp, "db.fa"), "--otutabout", os.path.join(tmp, "t.tsv"),
                           "--sizein", "--threads", "1", "--quiet"])
        theirs = open(os.path.join(tmp, "t.tsv"), "rb").read()
    ours = b"".join(l + b"\n" for l in ot.otutabout_lines(ot.otutab_host(q[:n], t, q_target[:n], sizes=size[:n], matched=matched)))
    return secs, hashlib.sha256(theirs).hexdigest(), hashlib.sha256(ours).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=4000000)
    ap.add_argument("--targets", type=int, default=20000)
    ap.add_argument("--samples", type=int, default=96)
    ap.add_argument("--cli-sample", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Q, T, q_target, size, matched, q, t = simulate(a.seed, a.queries, a.targets, a.samples)
    out = dict(bench="otutab", queries=a.queries, targets=a.targets, samples=a.samples, label_bytes=len(Q.blob) + len(T.blob))
    with Aligner(device=0) as al:
        calls = []
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            res = ot.otutab(Q, T, q_target, sizes=size, matched=matched, aligner=al)
            wall = time.perf_counter() - t0
            if res.stats["labels_host"] or not res.stats["labels_device"]:
                raise RuntimeError("the device route did not answer")
            if step >= a.warmup:
                calls.append((res.stats["seconds_total"], wall, res.stats))
        calls.sort(key=lambda c: c[0])
        med = calls[len(calls) // 2]
        out.update(seconds=med[0], seconds_all=[round(c[0], 6) for c in calls], seconds_with_python=med[1], labels_per_second=(a.queries + a.targets) / med[0],
                   stats=med[2], scan_kernel_seconds=med[2]["seconds_scan"], n_samples=len(res.samples), n_otus=len(res.otus), n_cells=len(res.nz_count),
                   has_tax=res.has_tax)
        host = ot.otutab_host(Q, T, q_target, sizes=size, matched=matched, threads=16)
        if host.arrays() != res.arrays():
            raise RuntimeError("device and host restatement differ")
        hs = sorted(ot.otutab_host(Q, T, q_target, sizes=size, matched=matched, threads=16).stats["seconds_total"] for _ in range(3))[1]
        out.update(host_threads=16, host_seconds=hs, host_stats=host.stats, host_equal=True, faster_route="device" if med[0] < hs else "host",
                   faster_by=max(hs, med[0]) / min(hs, med[0]))
    if refcli.available() and a.cli_sample:
        n = min(a.cli_sample, a.queries)
        secs, theirs, ours = cli_sample(q, t, q_target, size, n, a.seed + 1)
        out.update(cli_sample=n, cli_seconds=secs, cli_digest=theirs, our_digest=ours, parity_sample_match=theirs == ours)
        if theirs != ours:
            raise RuntimeError("the --otutabout text of the sample differs from the reference CLI's")
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
