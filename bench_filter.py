"""Read filtering throughput: vsx_fastx_filter on simulated 250 bp reads (the forward reads of tests/merge_data.generate:
qualities decaying toward the 3' end, errors drawn from the qualities, a share with Ns) with maxee 1.0, truncqual 2, maxns 0.

    python bench_filter.py [--reads N] [--unique U] [--cli-sample S] [--steps K] [--warmup W] [--out FILE]

Prints one JSON line (and writes it to --out): reads/s of the C call end to end (median of the steps, all of them listed),
the seconds split of vsx_fastx_filter_last_stats for the median call, and -- where oracle/_ref/vsearch_ref exists -- the
reference CLI's --fastq_filter time on the first S reads (one thread; file reading and writing included, as the command does
them), plus a parity digest: sha256 of the kept and the discarded FASTQ with --fastq_eeout of that sample, ours against the CLI's.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import time

from tests import fastq_filter_data as fd
from tests import merge_data as md
from vsearch_amd import Aligner, _lib
from vsearch_amd.filter import _blob, default_opts, filter_reads, last_stats

OPTS = {"maxee": 1.0, "truncqual": 2, "maxns": 0}


def digest(kept, discarded):
    h = hashlib.sha256()
    for line in list(kept) + list(discarded):
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    unique = min(a.unique, a.reads)
    _, fwd, fqual, _, _ = md.generate(a.seed, unique)
    reps = -(-a.reads // unique)
    seqs, quals = (fwd * reps)[:a.reads], (fqual * reps)[:a.reads]
    sb, off, lens = _blob(seqs)
    qb = _blob(quals)[0]
    lib = _lib.load()
    opts = default_opts(**OPTS)
    raw = lambda b: C.cast(C.c_char_p(b), C.c_void_p)  # noqa: E731
    reads = _lib.FilterReads(raw(sb), raw(qb), len(sb), off.ctypes.data, lens.ctypes.data, None)
    out = {"bench": "filter", "reads": a.reads, "unique_reads": unique, "read_length": 250, "input_bytes": 2 * len(sb), "opts": OPTS}
    with Aligner(device=0) as al:
        calls = []
        for step in range(a.warmup + a.steps):
            res = _lib.FilterOut()
            t0 = time.perf_counter()
            _lib.check(lib.vsx_fastx_filter(al.h, C.byref(opts), C.c_uint64(a.reads), C.byref(reads), None, C.byref(res)), "vsx_fastx_filter")
            dt = time.perf_counter() - t0
            totals = (int(res.kept), int(res.kept_truncated), int(res.discarded))
            lib.vsx_fastx_filter_out_free(C.byref(res))
            if step >= a.warmup:
                calls.append((dt, last_stats()))
        dt, split = sorted(calls, key=lambda c: c[0])[len(calls) // 2]
        out.update({"seconds": dt, "reads_per_s": a.reads / dt, "seconds_all": [c[0] for c in calls],
                    "kept": totals[0], "kept_truncated": totals[1], "discarded": totals[2],
                    "seconds_stage": split["seconds_stage"], "seconds_h2d": split["seconds_h2d"], "seconds_kernel": split["seconds_kernel"],
                    "seconds_d2h_output": split["seconds_d2h_output"], "seconds_total": split["seconds_total"],
                    "windows": split["windows"], "reads_host": split["reads_host"],
                    "kernel_over_h2d": split["seconds_kernel"] / split["seconds_h2d"] if split["seconds_h2d"] else None})
        if os.path.exists(fd.ref_binary()) and a.cli_sample > 0:
            n = min(a.cli_sample, a.reads)
            sample = {"name": "bench", "opts": OPTS, "labels": [f"read{k}" for k in range(n)], "seqs": seqs[:n], "quals": quals[:n]}
            ref = fd.run_reference(sample)
            t0 = time.perf_counter()
            ours = filter_reads(al, sample["seqs"], sample["quals"], **OPTS)
            t_ours = time.perf_counter() - t0
            mine = fd.library_lines(ours, sample)
            d_ref, d_ours = digest(ref["kept"], ref["discarded"]), digest(mine["kept"], mine["discarded"])
            out.update({"cli_sample_reads": n, "cli_seconds_1_thread": ref["seconds"], "cli_reads_per_s_1_thread": n / ref["seconds"],
                        "sample_seconds_python_call": t_ours, "parity_digest_reference": d_ref, "parity_digest": d_ours,
                        "parity": d_ref == d_ours and ref["counts"] == mine["counts"]})
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
