"""Paired-end merging throughput: vsx_merge_pairs on simulated 2 x 250 amplicon pairs (tests/merge_data.generate: fragment
lengths from staggered to no overlap, qualities decaying toward the 3' end, errors drawn from the qualities).

    python bench_merge.py [--pairs N] [--unique U] [--cli-sample S] [--steps K] [--warmup W]

Prints one JSON line: pairs/s of the C call end to end (best of the steps), the seconds split of vsx_merge_last_stats,
scored diagonals per pair, and -- where oracle/_ref/vsearch_ref exists -- the reference CLI's --fastq_mergepairs time on
the first S pairs with 16 threads and with one thread (file reading and writing included, as the command does them), plus
a parity digest: sha256 of the merged FASTQ + eetabbed lines of that sample, ours against the one-thread CLI run.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import time

import numpy as np

from tests import merge_data as md
from vsearch_amd import Aligner, _lib
from vsearch_amd.merge import RECORD_DTYPE, _blob, default_opts, last_stats, merge_pairs


def digest(fastq, eetabbed):
    h = hashlib.sha256()
    for line in list(fastq) + list(eetabbed):
        h.update(line.encode() + b"\n")
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=400000)
    ap.add_argument("--unique", type=int, default=50000, help="distinct generated pairs; repeated up to --pairs")
    ap.add_argument("--cli-sample", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()

    unique = min(a.unique, a.pairs)
    labels, fwd, fqual, rev, rqual = md.generate(a.seed, unique)
    reps = -(-a.pairs // unique)
    big = [(x * reps)[:a.pairs] for x in (fwd, fqual, rev, rqual)]
    fs, foff, flen = _blob(big[0]); fq = _blob(big[1])[0]
    rs, roff, rlen = _blob(big[2]); rq = _blob(big[3])[0]
    lib = _lib.load()
    opts = default_opts()
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)       # noqa: E731
    raw = lambda b: C.cast(C.c_char_p(b), C.c_void_p)  # noqa: E731
    out = {"bench": "merge", "pairs": a.pairs, "unique_pairs": unique, "read_length": 250, "input_bytes": 2 * (len(fs) + len(rs))}
    with Aligner(device=0) as al:
        best, split = None, None
        for step in range(a.warmup + a.steps):
            res = _lib.MergeOut()
            t0 = time.perf_counter()
            _lib.check(lib.vsx_merge_pairs(al.h, C.byref(opts), C.c_uint64(a.pairs), raw(fs), raw(fq), C.c_uint64(len(fs)), ptr(foff), ptr(flen),
                                           raw(rs), raw(rq), C.c_uint64(len(rs)), ptr(roff), ptr(rlen), C.byref(res)), "vsx_merge_pairs")
            dt = time.perf_counter() - t0
            merged = int(np.ctypeslib.as_array(C.cast(res.rec, C.POINTER(C.c_uint8)), shape=(a.pairs * RECORD_DTYPE.itemsize,))
                         .view(RECORD_DTYPE)["merged"].sum())
            lib.vsx_merge_out_free(C.byref(res))
            if step >= a.warmup and (best is None or dt < best):
                best, split = dt, last_stats()
        out.update({"seconds": best, "pairs_per_s": a.pairs / best, "merged_share": merged / a.pairs,
                    "seconds_stage_h2d": split["seconds_stage"], "seconds_kernel": split["seconds_kernel"],
                    "seconds_d2h_unpack": split["seconds_unpack"], "windows": split["windows"],
                    "diagonals_per_pair": split["diagonals_scored"] / a.pairs, "pairs_host": split["pairs_host"],
                    "share_stage_unpack": (split["seconds_stage"] + split["seconds_unpack"]) / split["seconds_total"]})
        if os.path.exists(md.ref_binary()) and a.cli_sample > 0:
            s = min(a.cli_sample, unique)
            sample = [x[:s] for x in (labels, fwd, fqual, rev, rqual)]
            ref1 = md.run_reference(*sample, threads=1)
            ref16 = md.run_reference(*sample, threads=16)
            t0 = time.perf_counter()
            ours = merge_pairs(al, *sample[1:])
            t_ours = time.perf_counter() - t0
            d_ref, d_ours = digest(ref1["fastq"], ref1["eetabbed"]), digest(ours.fastq_lines(sample[0], eeout=True), ours.eetabbed_lines())
            out.update({"cli_sample_pairs": s, "cli_seconds_1_thread": ref1["seconds"], "cli_seconds_16_threads": ref16["seconds"],
                        "cli_pairs_per_s_1_thread": s / ref1["seconds"], "cli_pairs_per_s_16_threads": s / ref16["seconds"],
                        "sample_seconds_python_call": t_ours, "parity_digest_reference": d_ref, "parity_digest": d_ours,
                        "parity": d_ref == d_ours})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
