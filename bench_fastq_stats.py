"""Read summary throughput: vsx_fastq_stats and vsx_fastq_chars on simulated 250 bp reads with a declining quality profile (the
forward reads of tests/merge_data.generate: qualities decaying toward the 3' end).

    python bench_fastq_stats.py [--reads N] [--unique U] [--cli-sample S] [--steps K] [--warmup W] [--out FILE]

Prints one JSON line (and writes it to --out).  Per call: reads/s of the C call end to end (median of the steps, all of them
listed) and the seconds split of its *_last_stats for the median call.  vsx_fastq_eestats with want = eestats runs on the same
reads in the same process, alternating with vsx_fastq_stats step by step: the two share the ordered-sum kernel.  Where
oracle/_ref/vsearch_ref exists: the reference CLI's --fastq_stats and --fastq_chars times on the first S reads (one thread;
file reading and log writing included, as the commands do them), and a parity digest: sha256 of the comparable log text of
that sample, ours against the CLI's.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import time

from tests import fastq_stats_data as fd
from tests import merge_data as md
from vsearch_amd import Aligner, _lib, eestats
from vsearch_amd.fastq_stats import _blob, _last, fastq_chars, fastq_stats


def digest(lines):
    h = hashlib.sha256()
    for line in lines:
        h.update(line.encode() + b"\n")
    return h.hexdigest()


def median(calls):
    return sorted(calls, key=lambda c: c[0])[len(calls) // 2]


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
    qb, _, _ = _blob(quals)
    lib = _lib.load()
    cast = lambda b: C.cast(C.c_char_p(b), C.c_void_p)      # noqa: E731
    reads = _lib.FilterReads(cast(sb), cast(qb), len(qb), off.ctypes.data, lens.ctypes.data, None)
    n = C.c_uint64(a.reads)
    so, co = _lib.FastqStatsOpts(), _lib.FastqCharsOpts()
    lib.vsx_fastq_stats_opts_default(C.byref(so))
    lib.vsx_fastq_chars_opts_default(C.byref(co))
    eo, keep = eestats.default_opts(want="eestats")
    out = {"bench": "fastq_stats", "reads": a.reads, "unique_reads": unique, "read_length": 250, "input_bytes_per_blob": len(qb),
           "library": os.path.basename(_lib.LIB_PATH)}

    def timed(call, res, free, stats):
        t0 = time.perf_counter()
        _lib.check(call(res), "bench")
        dt = time.perf_counter() - t0
        free(C.byref(res))
        return dt, stats()

    with Aligner(device=0) as al:
        runs = {
            "stats": lambda: timed(lambda r: lib.vsx_fastq_stats(al.h, C.byref(so), n, C.byref(reads), C.byref(r)), _lib.FastqStatsOut(),
                                   lib.vsx_fastq_stats_out_free, lambda: _last(lib.vsx_fastq_stats_last_stats, _lib.FastqStatsStats)),
            "eestats": lambda: timed(lambda r: lib.vsx_fastq_eestats(al.h, C.byref(eo), n, C.byref(reads), C.byref(r)), _lib.EEStatsOut(),
                                     lib.vsx_fastq_eestats_out_free, eestats.last_stats),
            "chars": lambda: timed(lambda r: lib.vsx_fastq_chars(al.h, C.byref(co), n, C.byref(reads), C.byref(r)), _lib.FastqCharsOut(),
                                   lib.vsx_fastq_chars_out_free, lambda: _last(lib.vsx_fastq_chars_last_stats, _lib.FastqCharsStats)),
        }
        calls = {name: [] for name in runs}
        for step in range(a.warmup + a.steps):
            for name, run in runs.items():              # alternating: the calls see the same machine
                result = run()
                if step >= a.warmup:
                    calls[name].append(result)
        for name in runs:
            dt, split = median(calls[name])
            out[name] = {"seconds": dt, "reads_per_s": a.reads / dt, "seconds_all": [c[0] for c in calls[name]],
                         **{k: v for k, v in split.items() if k != "reads"}}
        out["stats_over_eestats"] = out["stats"]["seconds"] / out["eestats"]["seconds"]
        if os.path.exists(fd.ref_binary()) and a.cli_sample > 0:
            m = min(a.cli_sample, a.reads)
            sample = fd._set("bench", quals[:m], seqs[:m])
            ref = fd.run_reference(sample)
            t0 = time.perf_counter()
            ours = {"stats": fastq_stats(al, sample["quals"]).log_lines(), "chars": fastq_chars(al, sample["seqs"], sample["quals"]).log_lines()}
            t_ours = time.perf_counter() - t0
            out["cli"] = {"sample_reads": m, "sample_seconds_python_calls_and_text": t_ours}
            for name in ("stats", "chars"):
                d_ref, d_ours = digest(ref[name]), digest(ours[name])
                out["cli"][name] = {"seconds_1_thread": ref["seconds"][name], "reads_per_s": m / ref["seconds"][name],
                                    "parity_digest_reference": d_ref, "parity_digest": d_ours, "parity": d_ref == d_ours}
    del keep
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
