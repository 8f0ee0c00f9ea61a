"""Read statistics throughput: vsx_fastq_eestats (both tables in one call) on simulated 250 bp reads with a declining quality
profile (the forward reads of tests/merge_data.generate: qualities decaying toward the 3' end).

    python bench_eestats.py [--reads N] [--unique U] [--cli-sample S] [--steps K] [--warmup W] [--want both|eestats|eestats2] [--out FILE]

Prints one JSON line (and writes it to --out): reads/s of the C call end to end (median of the steps, all of them listed),
the seconds split of vsx_fastq_eestats_last_stats for the median call with the ordered-sum kernel's share of the device time,
and -- where oracle/_ref/vsearch_ref exists -- the reference CLI's --fastq_eestats and --fastq_eestats2 times on the first S
reads (one thread: both commands are single-threaded; file reading and writing included, as the commands do them), plus a parity
digest: sha256 of the two output texts of that sample, ours against the CLI's.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import time

from tests import eestats_data as ed
from tests import merge_data as md
from vsearch_amd import Aligner, _lib
from vsearch_amd.eestats import _blob, default_opts, last_stats, read_stats


def digest(*texts):
    h = hashlib.sha256()
    for lines in texts:
        for line in lines:
            h.update(line.encode() + b"\n")
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--unique", type=int, default=50000, help="distinct generated reads; repeated up to --reads")
    ap.add_argument("--cli-sample", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--want", default="both", choices=["both", "eestats", "eestats2"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    unique = min(a.unique, a.reads)
    _, _, fqual, _, _ = md.generate(a.seed, unique)
    reps = -(-a.reads // unique)
    quals = (fqual * reps)[:a.reads]
    qb, off, lens = _blob(quals)
    lib = _lib.load()
    opts, keep = default_opts(want=a.want)
    reads = _lib.FilterReads(None, C.cast(C.c_char_p(qb), C.c_void_p), len(qb), off.ctypes.data, lens.ctypes.data, None)
    out = {"bench": "eestats", "reads": a.reads, "unique_reads": unique, "read_length": 250, "input_bytes": len(qb), "want": a.want,
           "library": os.path.basename(_lib.LIB_PATH)}
    with Aligner(device=0) as al:
        calls = []
        for step in range(a.warmup + a.steps):
            res = _lib.EEStatsOut()
            t0 = time.perf_counter()
            _lib.check(lib.vsx_fastq_eestats(al.h, C.byref(opts), C.c_uint64(a.reads), C.byref(reads), C.byref(res)), "vsx_fastq_eestats")
            dt = time.perf_counter() - t0
            lib.vsx_fastq_eestats_out_free(C.byref(res))
            if step >= a.warmup:
                calls.append((dt, last_stats()))
        dt, split = sorted(calls, key=lambda c: c[0])[len(calls) // 2]
        device = split["seconds_walk"] + split["seconds_sum"] + split["seconds_quantile"]
        out.update({"seconds": dt, "reads_per_s": a.reads / dt, "seconds_all": [c[0] for c in calls]})
        out.update({k: split[k] for k in ("seconds_stage", "seconds_h2d", "seconds_walk", "seconds_sum", "seconds_quantile",
                                          "seconds_d2h_output", "seconds_total", "windows", "reads_host")})
        out["sum_share_of_kernels"] = split["seconds_sum"] / device if device else None
        if os.path.exists(ed.ref_binary()) and a.cli_sample > 0:
            n = min(a.cli_sample, a.reads)
            sample = {"name": "bench", "opts": {}, "quals": quals[:n]}
            ref = ed.run_reference(sample)
            t0 = time.perf_counter()
            ours = read_stats(al, sample["quals"])
            t_ours = time.perf_counter() - t0
            d_ref, d_ours = digest(ref["eestats"], ref["eestats2"]), digest(ours.eestats_lines(), ours.eestats2_lines())
            out.update({"cli_sample_reads": n, "cli_seconds_eestats_1_thread": ref["seconds"]["eestats"],
                        "cli_seconds_eestats2_1_thread": ref["seconds"]["eestats2"],
                        "cli_reads_per_s_eestats": n / ref["seconds"]["eestats"], "cli_reads_per_s_eestats2": n / ref["seconds"]["eestats2"],
                        "cli_reads_per_s_both": n / (ref["seconds"]["eestats"] + ref["seconds"]["eestats2"]),
                        "sample_seconds_python_call": t_ours, "parity_digest_reference": d_ref, "parity_digest": d_ours,
                        "parity": d_ref == d_ours})
    del keep
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
