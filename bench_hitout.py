"""Search hit writers: vsx_hits_render on the hits of a finished search.

    python bench_hitout.py [--reads N] [--targets T] [--cli-sample C] [--steps K] [--warmup W] [--out FILE]

Workload: N simulated 250 bp reads (default 1 000 000; windows of the database sequences with 2 % substitutions, half of them reverse
complemented) against T random sequences of 400 bp (200 000), both strands, default DUST masking, through search_batch_raw.  Then
render() with each `want`: the median of K calls after W, split as vsx_hits_render_last_stats splits it -- masking, CIGAR parse and
staging, H2D, the three kernels, D2H.  The same input goes through the library's host restatement with 16 threads, with the
equality of every array and blob asserted.  The formatters are Python and not the measured path: they are timed on the CLI sample
only.  Where oracle/_ref/vsearch_ref exists, the reference CLI runs with one thread on the first C reads (100 000) writing the same
seven files, and the sha256 of each file is compared with ours.  Prints one JSON line (and writes it to --out).  The call starts
from hits in memory and the CLI from FASTA files and includes its search: no ratio is claimed.
"""
import argparse
import hashlib
import json
import os
import tempfile
import time

import numpy as np

from tests import hitout_data as hd
from vsearch_amd import Aligner, SearchSession
from vsearch_amd import hitout as ho

LETTERS = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")


def simulate(seed, n_reads, n_targets, read_len=250, target_len=400):
    rng = np.random.default_rng(seed)
    db = LETTERS[rng.integers(0, 4, (n_targets, target_len))]
    src = rng.integers(0, n_targets, n_reads)
    start = rng.integers(0, target_len - read_len + 1, n_reads)
    reads = db[src[:, None], start[:, None] + np.arange(read_len)[None, :]]
    sub = rng.random(reads.shape) < 0.02
    reads[sub] = LETTERS[rng.integers(0, 4, int(sub.sum()))]
    minus = rng.random(n_reads) < 0.5
    reads[minus] = COMP[reads[minus][:, ::-1]]
    return [bytes(r) for r in db], [bytes(r) for r in reads]


def median_call(fn, steps, warmup):
    calls = []
    for step in range(warmup + steps):
        t0 = time.perf_counter()
        res = fn()
        wall = time.perf_counter() - t0
        if step >= warmup:
            calls.append((res.stats["seconds_total"], wall, res.stats))
    calls.sort(key=lambda c: c[0])
    return res, calls[len(calls) // 2], [round(c[0], 6) for c in calls]


def cli_sample(sess, db, reads, n):
    """the reference CLI on the first n reads -> seconds per run, and per file (sha256 of the CLI's, sha256 of ours)"""
    s = hd._cli("bench", opts=dict(qmask="dust", dbmask="dust"), fmt=dict(maxhits=3, output_no_hits=1), search_args=("--id", "0.9", "--maxaccepts", "4"),
                inputs=([d.decode() for d in db], [r.decode() for r in reads[:n]]))
    with tempfile.TemporaryDirectory(prefix="vsx_hitout_bench_") as tmp:
        t0 = time.perf_counter()
        ref = hd.run_reference(s, tmp=tmp)
        secs = (time.perf_counter() - t0) / 3                      # run_reference starts the CLI three times on the same input
    raw = sess.search_batch_raw(reads[:n])
    t0 = time.perf_counter()
    text = ho.render(sess, reads[:n], raw)
    t_render = time.perf_counter() - t0
    t0 = time.perf_counter()
    ours = hd.format_all(text, s)
    t_format = time.perf_counter() - t0
    sha = lambda x: hashlib.sha256(x.encode("latin-1")).hexdigest()
    return secs, t_render, t_format, {w: (sha(ref[w]), sha(ours[w])) for w in hd.WRITERS}, len(raw[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--targets", type=int, default=200000)
    ap.add_argument("--cli-sample", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=19)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    db, reads = simulate(a.seed, a.reads, a.targets)
    out = dict(bench="hitout", reads=a.reads, targets=a.targets)
    with Aligner(device=0) as al:
        sess = SearchSession(al, db, id=0.9, maxaccepts=4, strand_both=1, soft_mask=2)
        t0 = time.perf_counter()
        raw = sess.search_batch_raw(reads)
        out.update(search_seconds=time.perf_counter() - t0, hits=int(len(raw[1])), minus_hits=int((raw[1]["strand"] == 1).sum()),
                   columns=int(raw[1]["internal_alignmentlength"].sum()))
        full = None
        for name, want in (("rows", ho.ROWS), ("symbols", ho.SYMBOLS), ("sam", ho.SAM), ("all", ho.ALL)):
            res, med, every = median_call(lambda: ho.render(sess, reads, raw, want=want), a.steps, a.warmup)
            if res.stats["hits_host"] or res.stats["hits_device"] != len(raw[1]):
                raise RuntimeError("the device route did not answer")
            st = med[2]
            out["device_" + name] = dict(seconds=med[0], seconds_all=every, seconds_with_python=med[1], hits_per_second=len(raw[1]) / med[0],
                                         kernels_seconds=st["seconds_rows"] + st["seconds_md_count"] + st["seconds_md_fill"],
                                         transfers_seconds=st["seconds_h2d"] + st["seconds_d2h"], row_bytes=len(res.row_blob), md_bytes=len(res.md_blob),
                                         stats=st)
            full = res
        targets = sess.masked_db_text()
        kw = dict(strand_both=1, soft_mask=2)
        host = ho.render_host(targets, reads, raw, threads=16, **kw)
        if host.same_as(full) is not None:
            raise RuntimeError(f"device and host restatement differ in {host.same_as(full)}")
        hs = sorted((ho.render_host(targets, reads, raw, threads=16, **kw).stats for _ in range(3)), key=lambda s: s["seconds_total"])[1]
        dev = out["device_all"]
        out.update(host_threads=16, host_seconds=hs["seconds_total"], host_stats=hs, host_equal=True,
                   faster_route="device" if dev["seconds"] < hs["seconds_total"] else "host",
                   faster_by=max(hs["seconds_total"], dev["seconds"]) / min(hs["seconds_total"], dev["seconds"]),
                   transfers_set_the_time=dev["transfers_seconds"] > dev["kernels_seconds"])
        if os.path.exists(hd.ref_binary()) and a.cli_sample:
            n = min(a.cli_sample, a.reads)
            secs, t_render, t_format, digests, nh = cli_sample(sess, db, reads, n)
            out.update(cli_sample=n, cli_sample_hits=nh, cli_seconds_per_run=secs, sample_render_seconds=t_render, sample_format_seconds_python=t_format,
                       digests={w: d[0] for w, d in digests.items()}, parity_sample_match={w: d[0] == d[1] for w, d in digests.items()})
            if not all(d[0] == d[1] for d in digests.values()):
                raise RuntimeError("a file of the sample differs from the reference CLI's: " + json.dumps(out["parity_sample_match"]))
        sess.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
