"""Prefix dereplication throughput: vsx_derep_prefix on simulated 250 bp amplicon reads of which a share is cut short.

    python bench_derep_prefix.py [--reads N] [--templates T] [--cut F] [--cli-sample S] [--steps K] [--warmup W] [--out FILE]

Workload: T distinct random templates of 250 bp with abundances falling off as 1 / rank; N reads drawn from them, 70 % exact
copies and 30 % with one substitution at a random position; a share F (default 0.4) of all reads is cut at a length drawn
uniformly from 100 .. 249, so a template's reads form chains of several levels; no abundances.  Prints one JSON line (and
writes it to --out): per call the seconds end to end (median of the steps, all of them listed), reads/s, the clusters and nodes
found, the seconds split and counters of vsx_derep_prefix_last_stats for the median call and the probes per node; the
library's host restatement on the same input (its worker pool uses the CPUs the process may use) with the equality of its
output arrays; and, where oracle/_ref/vsearch_ref exists, the reference CLI's --derep_prefix --uc with one thread on the first
S reads (reading the FASTA file and writing the --uc file included) with a parity digest: sha256 of the sorted --uc lines of
that sample, ours against the CLI's.  The call starts from blobs in memory and the CLI from a file: no ratio is claimed.
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

from tests import derep_prefix_data as pd
from vsearch_amd import Aligner, _lib, derep_prefix
from vsearch_amd.derep_prefix import default_opts, last_stats

READ_LENGTH, CUT_SHORTEST = 250, 100
ARRAYS = (("rep", "n_clusters"), ("size", "n_clusters"), ("count", "n_clusters"), ("member", "kept"), ("rank", "n"))


def simulate(seed, n_templates, n_reads, cut):
    """-> read rows as a uint8 array of ASCII symbols, and the reads' lengths"""
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
    lens = np.full(n_reads, READ_LENGTH, np.uint32)
    short = rng.random(n_reads) < cut
    lens[short] = rng.integers(CUT_SHORTEST, READ_LENGTH, int(short.sum()))
    return reads, lens


def digest(lines):
    h = hashlib.sha256()
    for line in sorted(lines):
        h.update(line.encode() + b"\n")
    return h.hexdigest()


def reference(sample, lens):
    with tempfile.TemporaryDirectory(prefix="vsx_derep_prefix_bench_") as tmp:
        fa, uc = os.path.join(tmp, "r.fa"), os.path.join(tmp, "o.uc")
        with open(fa, "wb") as f:
            for k0 in range(0, len(sample), 65536):
                f.write(b"".join(b">r%d\n%s\n" % (k0 + k, r.tobytes()[:lens[k0 + k]]) for k, r in enumerate(sample[k0:k0 + 65536])))
        args = [pd.ref_binary(), "--derep_prefix", fa, "--uc", uc, "--threads", "1", "--quiet"]
        t0 = time.perf_counter()
        r = subprocess.run(args, capture_output=True, text=True)
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        return dt, open(uc).read().splitlines()


def arrays_of(res):
    return {name: np.ctypeslib.as_array(getattr(res, name), shape=(max(int(getattr(res, count)), 1),))[:int(getattr(res, count))].copy()
            for name, count in ARRAYS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--templates", type=int, default=20000)
    ap.add_argument("--cut", type=float, default=0.4)
    ap.add_argument("--cli-sample", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=13)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    reads, lens = simulate(a.seed, a.templates, a.reads, a.cut)
    blob = reads.tobytes()
    off = np.arange(a.reads, dtype=np.uint64) * READ_LENGTH
    labels = [b"r%d" % k for k in range(a.reads)]
    label_blob = b"".join(labels)
    label_off = np.zeros(a.reads + 1, np.uint64)
    np.cumsum([len(l) for l in labels], out=label_off[1:])
    lib = _lib.load()
    opts = default_opts()
    fr = _lib.FilterReads(C.cast(C.c_char_p(blob), C.c_void_p), None, len(blob), off.ctypes.data, lens.ctypes.data, None)
    out = {"bench": "derep_prefix", "reads": a.reads, "templates": a.templates, "read_length": READ_LENGTH, "cut_share": a.cut,
           "cut_lengths": [CUT_SHORTEST, READ_LENGTH - 1], "input_bytes": int(lens.sum()), "library": os.path.basename(_lib.LIB_PATH)}

    def one_call(handle):
        res = _lib.DerepPrefixOut()
        t0 = time.perf_counter()
        _lib.check(lib.vsx_derep_prefix(handle, C.byref(opts), a.reads, C.byref(fr), C.cast(C.c_char_p(label_blob), C.c_void_p),
                                        label_off.ctypes.data, C.byref(res)), "vsx_derep_prefix")
        dt = time.perf_counter() - t0
        got = (dt, last_stats(), int(res.n_clusters), int(res.maxsize), arrays_of(res))
        lib.vsx_derep_prefix_out_free(C.byref(res))
        return got

    with Aligner(device=0) as al:
        calls = []
        for step in range(a.warmup + a.steps):
            got = one_call(al.h)
            if step == 0:
                out["first_call_seconds"] = got[0]
            if step >= a.warmup:
                calls.append(got)
        dt, st, clusters, maxsize, device_arrays = sorted(calls, key=lambda c: c[0])[len(calls) // 2]
        if st["reads_host"]:
            raise RuntimeError("the call ran on the host")
        out["call"] = {"seconds": dt, "reads_per_s": a.reads / dt, "seconds_all": [c[0] for c in calls], "clusters": clusters,
                       "largest_cluster": maxsize, "probes_per_node": st["probes"] / max(st["nodes"], 1), **st}
        hosts = [one_call(None) for _ in range(3)]
        hdt, hst, _, _, host_arrays = sorted(hosts, key=lambda c: c[0])[1]
        out["host"] = {"seconds": hdt, "reads_per_s": a.reads / hdt, "seconds_all": [c[0] for c in hosts], "cpus": min(16, lib.vsx_internal_usable_cpus()),
                       "equal_to_device": all(np.array_equal(device_arrays[n], host_arrays[n]) for n, _ in ARRAYS), **hst}
        out["faster_route"] = "device" if dt < hdt else "host"
        if os.path.exists(pd.ref_binary()) and a.cli_sample > 0:
            m = min(a.cli_sample, a.reads)
            seqs, names = [r.tobytes()[:lens[k]] for k, r in enumerate(reads[:m])], ["r%d" % k for k in range(m)]
            t0 = time.perf_counter()
            ours = derep_prefix(al, seqs, names)
            t_ours = time.perf_counter() - t0
            secs, lines = reference(reads[:m], lens)
            mine = ours.uc_lines()
            out["cli"] = {"sample_reads": m, "sample_call_seconds_with_python_marshalling": t_ours, "sample_call_seconds": ours.stats["seconds_total"],
                          "sample_clusters": len(ours), "threads_1": {"seconds": secs, "reads_per_s": m / secs},
                          "includes": "FASTA parsing, --uc writing", "parity_digest_reference": digest(lines), "parity_digest": digest(mine),
                          "parity": digest(lines) == digest(mine)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
