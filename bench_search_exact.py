"""Exact-search throughput: vsx_search_exact on simulated 250 bp reads mapped back onto a set of distinct sequences, both strands.

    python bench_search_exact.py [--reads N] [--db D] [--cli-sample S] [--steps K] [--warmup W] [--out FILE]

Workload: D distinct random sequences of 250 bp; N reads drawn from them, about 60 % exact copies (half of those
reverse-complemented), the rest one substitution away; --strand both, no masking.  Prints one JSON line (and writes it to --out):
the index build of the first call on its own, then per call the seconds end to end (median of the steps, all of them listed),
queries/s and the seconds split and counters of vsx_search_exact_last_stats for the median call.  Where oracle/_ref/vsearch_ref
exists: the reference CLI's --search_exact on the first S reads against the same database with 1 thread and with 16 threads
(reading both FASTA files, building its index and writing --userout included, as the command does them), and a parity digest:
sha256 of the sorted query+target+qstrand+caln lines of that sample, ours against the CLI's.
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

from tests import search_exact_data as sd
from vsearch_amd import Aligner, SearchSession, _lib
from vsearch_amd.search import exact_last_stats

READ_LENGTH = 250
FIELDS = ("query", "target", "qstrand", "caln")


def simulate(seed, n_db, n_reads):
    """-> (db rows, read rows) as uint8 arrays of ASCII symbols"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    db = letters[rng.integers(0, 4, (n_db, READ_LENGTH))]
    reads = db[rng.integers(0, n_db, n_reads)].copy()
    kind = rng.random(n_reads)
    comp = np.zeros(256, np.uint8)
    comp[letters] = np.frombuffer(b"TGCA", np.uint8)
    minus = (kind >= 0.3) & (kind < 0.6)
    reads[minus] = comp[reads[minus][:, ::-1]]
    sub = np.flatnonzero(kind >= 0.6)
    pos = rng.integers(0, READ_LENGTH, sub.size)
    nxt = np.zeros(256, np.uint8)
    nxt[letters] = np.frombuffer(b"CGTA", np.uint8)
    reads[sub, pos] = nxt[reads[sub, pos]]
    return db, reads


def digest(lines):
    h = hashlib.sha256()
    for line in sorted(lines):
        h.update(line.encode() + b"\n")
    return h.hexdigest()


def fasta(path, prefix, rows):
    with open(path, "wb") as f:
        for k0 in range(0, len(rows), 65536):
            f.write(b"".join(b">%s%d\n%s\n" % (prefix, k0 + k, r.tobytes()) for k, r in enumerate(rows[k0:k0 + 65536])))


def reference(db, sample, threads):
    with tempfile.TemporaryDirectory(prefix="vsx_exact_bench_") as tmp:
        p = lambda n: os.path.join(tmp, n)            # noqa: E731
        fasta(p("db.fa"), b"t", db)
        fasta(p("q.fa"), b"q", sample)
        args = [sd.ref_binary(), "--search_exact", p("q.fa"), "--db", p("db.fa"), "--strand", "both", "--qmask", "none", "--dbmask", "none",
                "--threads", str(threads), "--userout", p("u.tsv"), "--userfields", "+".join(FIELDS), "--quiet"]
        t0 = time.perf_counter()
        r = subprocess.run(args, capture_output=True, text=True)
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        return dt, open(p("u.tsv")).read().splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--db", type=int, default=200000)
    ap.add_argument("--cli-sample", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    db, reads = simulate(a.seed, a.db, a.reads)
    blob = reads.tobytes()
    off = np.arange(a.reads, dtype=np.uint64) * READ_LENGTH
    lens = np.full(a.reads, READ_LENGTH, np.uint32)
    lib = _lib.load()
    out = {"bench": "search_exact", "reads": a.reads, "db_sequences": a.db, "read_length": READ_LENGTH, "strand": "both",
           "input_bytes": len(blob), "library": os.path.basename(_lib.LIB_PATH)}

    def call(sess, n):
        res = _lib.Hits()
        t0 = time.perf_counter()
        _lib.check(lib.vsx_search_exact(sess.h, n, C.cast(C.c_char_p(blob), C.c_void_p), n * READ_LENGTH, off.ctypes.data_as(C.c_void_p),
                                        lens.ctypes.data_as(C.c_void_p), None, C.byref(res)), "vsx_search_exact")
        dt = time.perf_counter() - t0
        return dt, exact_last_stats(), res

    with Aligner(device=0) as al:
        sess = SearchSession(al, [r.tobytes() for r in db], id=1.0, strand_both=1)
        calls = []
        for step in range(a.warmup + a.steps):
            dt, st, res = call(sess, a.reads)
            lib.vsx_hits_free(C.byref(res))
            if step == 0:
                out["index_build_seconds"] = st["seconds_index"]
                out["first_call_seconds"] = dt
            if step >= a.warmup:
                calls.append((dt, st))
        dt, st = sorted(calls, key=lambda c: c[0])[len(calls) // 2]
        out["call"] = {"seconds": dt, "queries_per_s": a.reads / dt, "seconds_all": [c[0] for c in calls], **st}
        if os.path.exists(sd.ref_binary()) and a.cli_sample > 0:
            m = min(a.cli_sample, a.reads)
            t0 = time.perf_counter()
            _, _, res = call(sess, m)
            t_ours = time.perf_counter() - t0
            first, hits, cig = SearchSession._raw_hits(res)
            ours = []
            for q in range(m):
                for k in range(int(first[q]), int(first[q + 1])):
                    o = int(hits["cigar_off"][k])
                    ours.append("q%d\tt%d\t%s\t%s" % (q, hits["target"][k], "-" if hits["strand"][k] else "+", cig[o:cig.index(b"\0", o)].decode()))
            out["cli"] = {"sample_reads": m, "sample_call_seconds": t_ours, "sample_queries_per_s": m / t_ours, "hits": len(ours),
                          "includes": "FASTA parsing of queries and database, index build, --userout writing"}
            for threads in (1, 16):
                secs, lines = reference(db, reads[:m], threads)
                out["cli"]["threads_%d" % threads] = {"seconds": secs, "queries_per_s": m / secs, "parity_digest_reference": digest(lines),
                                                      "parity_digest": digest(ours), "parity": digest(lines) == digest(ours)}
        sess.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
