"""Dereplication throughput: vsx_derep on simulated 250 bp amplicon reads, both strands.

    python bench_derep.py [--reads N] [--templates T] [--cli-sample S] [--steps K] [--warmup W] [--out FILE]

Workload: T distinct random templates of 250 bp with abundances falling off as 1 / rank; N reads drawn from them, 70 % exact
copies and 30 % with one substitution at a random position (mostly singletons, as sequencing errors are), 30 % of all reads
reverse-complemented; --strand both, no abundances, no qualities.  Prints one JSON line (and writes it to --out): per call the
seconds end to end (median of the steps, all of them listed), reads/s, the clusters found and the seconds split and counters of
vsx_derep_last_stats for the median call.  Where oracle/_ref/vsearch_ref exists: the reference CLI's --derep_fulllength
--strand both --uc with one thread on the first S reads (reading the FASTA file and writing the --uc file included, as the
command does them), and a parity digest: sha256 of the sorted --uc lines of that sample, ours against the CLI's.  The call
starts from blobs in memory and the CLI from a file: no ratio is claimed.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import tempfile
import time

import numpy as np

from tests import derep_data as dd
from vsearch_amd import Aligner, _lib
from vsearch_amd.derep import default_opts, dereplicate, last_stats

READ_LENGTH = 250


def simulate(seed, n_templates, n_reads):
    """-> read rows as a uint8 array of ASCII symbols"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    templates = letters[rng.integers(0, 4, (n_templates, READ_LENGTH))]
    weight = 1.0 / np.arange(1, n_templates + 1)
    reads = templates[rng.choice(n_templates, n_reads, p=weight / weight.sum())].copy()
    sub = np.flatnonzero(rng.random(n_reads) < 0.3)
    pos = rng.integers(0, READ_LENGTH, sub.size)
    nxt = np.zeros(256, np.uint8)
    nxt[letters] = np.frombuffer(b"CGTA", np.uint8)
    reads[sub, pos] = nxt[reads[sub, pos]]
    comp = np.zeros(256, np.uint8)
    comp[letters] = np.frombuffer(b"TGCA", np.uint8)
    minus = rng.random(n_reads) < 0.3
    reads[minus] = comp[reads[minus][:, ::-1]]
    return reads


def digest(lines):
    h = hashlib.sha256()
    for line in sorted(lines):
        h.update(line.encode() + b"\n")
    return h.hexdigest()


def reference(sample):
    with tempfile.TemporaryDirectory(prefix="vsx_derep_bench_") as tmp:
        fa, uc = os.path.join(tmp, "r.fa"), os.path.join(tmp, "o.uc")
        with open(fa, "wb") as f:
            for k0 in range(0, len(sample), 65536):
                f.write(b"".join(b">r%d\n%s\n" % (k0 + k, r.tobytes()) for k, r in enumerate(sample[k0:k0 + 65536])))
        args = [dd.ref_binary(), "--derep_fulllength", fa, "--strand", "both", "--uc", uc, "--threads", "1", "--quiet"]
        t0 = time.perf_counter()
        r = subprocess.run(args, capture_output=True, text=True)
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        return dt, open(uc).read().splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--templates", type=int, default=20000)
    ap.add_argument("--cli-sample", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    reads = simulate(a.seed, a.templates, a.reads)
    blob = reads.tobytes()
    off = np.arange(a.reads, dtype=np.uint64) * READ_LENGTH
    lens = np.full(a.reads, READ_LENGTH, np.uint32)
    labels = [b"r%d" % k for k in range(a.reads)]
    label_blob = b"".join(labels)
    label_off = np.zeros(a.reads + 1, np.uint64)
    np.cumsum([len(l) for l in labels], out=label_off[1:])
    lib = _lib.load()
    opts = default_opts(strand_both=1)
    fr = _lib.FilterReads(C.cast(C.c_char_p(blob), C.c_void_p), None, len(blob), off.ctypes.data, lens.ctypes.data, None)
    out = {"bench": "derep", "reads": a.reads, "templates": a.templates, "read_length": READ_LENGTH, "strand": "both",
           "input_bytes": len(blob), "library": os.path.basename(_lib.LIB_PATH)}

    with Aligner(device=0) as al:
        calls = []
        for step in range(a.warmup + a.steps):
            res = _lib.DerepOut()
            t0 = time.perf_counter()
            _lib.check(lib.vsx_derep(al.h, C.byref(opts), a.reads, C.byref(fr), C.cast(C.c_char_p(label_blob), C.c_void_p),
                                     label_off.ctypes.data, C.byref(res)), "vsx_derep")
            dt = time.perf_counter() - t0
            clusters, maxsize = int(res.n_clusters), int(res.maxsize)
            lib.vsx_derep_out_free(C.byref(res))
            if step == 0:
                out["first_call_seconds"] = dt
            if step >= a.warmup:
                calls.append((dt, last_stats()))
        dt, st = sorted(calls, key=lambda c: c[0])[len(calls) // 2]
        if st["reads_host"]:
            raise RuntimeError("the call ran on the host")
        out["call"] = {"seconds": dt, "reads_per_s": a.reads / dt, "seconds_all": [c[0] for c in calls], "clusters": clusters,
                       "largest_cluster": maxsize, **st}
        if os.path.exists(dd.ref_binary()) and a.cli_sample > 0:
            m = min(a.cli_sample, a.reads)
            seqs, names = [r.tobytes() for r in reads[:m]], ["r%d" % k for k in range(m)]
            t0 = time.perf_counter()
            ours = dereplicate(al, seqs, names, strand_both=1)
            t_ours = time.perf_counter() - t0
            secs, lines = reference(reads[:m])
            mine = ours.uc_lines()
            out["cli"] = {"sample_reads": m, "sample_call_seconds_with_python_marshalling": t_ours, "sample_call_seconds": ours.stats["seconds_total"],
                          "sample_clusters": len(ours), "threads_1": {"seconds": secs, "reads_per_s": m / secs},
                          "includes": "FASTA parsing, --uc writing", "parity_digest_reference": digest(lines), "parity_digest": digest(mine),
                          "parity": digest(lines) == digest(mine)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
