"""Last common ancestor output (--lcaout): vsx_lca on simulated search hits over SILVA-style labels.

    python bench_lca.py [--queries 1000000] [--hits 8] [--labels 200000] [--genera 5000] [--steps 5] [--no-host] [--no-cli] [--out FILE]

The shape: `queries` queries of `hits` hits each over `labels` database labels of about 120 bytes in `genera` genera; a query's hits
fall into its genus mostly, with strays into a sister genus and anywhere.  Prints one JSON line (and writes it to --out): the index
build once (split, numbering); vsx_lca end to end from the hit records in memory -- a first call, then the median of `steps` calls,
all of them listed, with the seconds per stage of vsx_lca_last_stats for the median call -- under the plain cutoff and under
--top_hits_only; the library's host restatement (vsx_internal_lca_host, the reference's loops over the labels' bytes) on 16
threads on the same input with every array compared; where oracle/_ref/vsearch_ref exists, the reference CLI's --usearch_global
--lcaout (one thread) on a sample of 2 000 queries against 2 000 labelled sequences, with the SHA-256 of its file against
lcaout_lines of a search through the library.  The CLI reads files and searches: its time stands beside ours, no ratio.  Not
measured: hardware counters, queries with thousands of hits, labels of kilobytes.
"""
import argparse
import hashlib
import json
import os
import random
import sys
import tempfile
import time

import numpy as np

from tests import lca_data as ld
from vsearch_amd import Aligner, SearchSession
from vsearch_amd import lca as lc

SPLIT = ("seconds_stage", "seconds_h2d", "seconds_vote", "seconds_d2h", "seconds_output", "seconds_total")
INDEX = ("seconds_index_stage", "seconds_index_split", "seconds_index_number", "seconds_index_total")
COUNTS = ("labels_device", "labels_host", "windows", "queries_device", "queries_host", "hits_device", "hits_host", "host_no_context",
          "host_environment", "host_count", "host_memory", "host_collision")


def silva_labels(n, genera, seed):
    """labels like AB123456.1.1503;tax=d:Bacteria,p:Proteobacteria,c:Gammaproteobacteria,o:...,f:...,g:...,s:...; and each one's genus"""
    rng = random.Random(seed)
    syl = ("bac", "ter", "ia", "pro", "teo", "mona", "coc", "cus", "lacto", "strepto", "entero", "vibrio", "spira", "myces", "thermo", "halo")
    word = lambda k: "".join(rng.choice(syl) for _ in range(k)).capitalize()  # noqa: E731
    phyla = [word(3) for _ in range(40)]
    lineage = []
    for g in range(genera):
        p = phyla[g % len(phyla)]
        lineage.append(("Bacteria" if g % 9 else "Archaea", p, p[:6] + "ia_c%d" % (g % 120), word(2) + "ales_o%d" % (g % 400), word(2) + "aceae_f%d" % (g % 1200),
                        word(2) + "_g%d" % g))
    labels, genus = [], np.zeros(n, np.uint32)
    for i in range(n):
        g = rng.randrange(genera)
        genus[i] = g
        d, p, c, o, f, gn = lineage[g]
        tax = "d:%s,p:%s,c:%s,o:%s,f:%s,g:%s" % (d, p, c, o, f, gn)
        if rng.random() < 0.7:
            tax += ",s:%s_sp%d" % (gn, rng.randrange(6))
        labels.append("%s%06d.1.%d;tax=%s;" % (rng.choice(("AB", "CP", "JX", "KF")), rng.randrange(10 ** 6), rng.randint(1200, 1600), tax))
    return labels, genus


def simulated_hits(nq, per, genus, genera, seed):
    """(first, hits): a query's hits lie in its genus, one in five in the sister genus, one in twenty anywhere; ids fall along the list"""
    rng = np.random.default_rng(seed)
    order = np.argsort(genus, kind="stable").astype(np.uint32)
    start = np.searchsorted(genus[order], np.arange(genera + 1))
    filled = np.nonzero(np.diff(start) > 0)[0]
    qg = filled[rng.integers(0, len(filled), nq)]
    g = np.repeat(qg, per)
    r = rng.random(nq * per)
    sister = filled[(np.searchsorted(filled, g) + 1) % len(filled)]
    g = np.where(r < 0.2, sister, g)
    pick = order[start[g] + (rng.random(nq * per) * (start[g + 1] - start[g])).astype(np.int64)]
    pick = np.where(r < 0.05, rng.integers(0, len(genus), nq * per), pick).astype(np.uint32)
    hits = np.zeros(nq * per, ld.hit_dtype())
    hits["target"] = pick
    hits["query"] = np.repeat(np.arange(nq, dtype=np.uint32), per)
    hits["id"] = 100.0 - np.tile(np.arange(per) // 3, nq) * 0.5
    return np.arange(nq + 1, dtype=np.uint64) * per, hits


def timed(fn, steps):
    t = time.perf_counter()
    fn()
    first = time.perf_counter() - t
    out = []
    for _ in range(steps):
        t = time.perf_counter()
        res = fn()
        out.append((time.perf_counter() - t, res))
    out.sort(key=lambda x: x[0])
    return round(first, 6), [round(t, 6) for t, _ in out], out[len(out) // 2]


def cli_sample(al):
    rng = random.Random(457)
    db, dbl = ld.live_db(rng)
    qs, ql = ld.live_queries(rng, db)
    search = ["--id", "0.9", "--maxaccepts", "8", "--maxrejects", "32"]
    with tempfile.TemporaryDirectory(prefix="bench_lca_") as tmp:
        ld.write_fasta(os.path.join(tmp, "db.fa"), zip(dbl, db))
        ld.write_fasta(os.path.join(tmp, "q.fa"), zip(ql, qs))
        t = time.perf_counter()
        ref, _ = ld.cli_lcaout(tmp, "usearch_global", search, "0.8")
        t_cli = time.perf_counter() - t
    sess = SearchSession(al, db, labels=dbl, id=0.9, maxaccepts=8, maxrejects=32)
    raw = sess.search_batch_raw(qs, labels=ql)
    sess.close()
    with lc.LcaIndex(dbl, ctx=al) as index:
        res = lc.lca(index, raw, lca_cutoff=0.8)
    ours = b"".join(lc.lcaout_lines(res, ql, dbl))
    return dict(queries=len(qs), targets=len(db), hits=int(raw[0][-1]), seconds=round(t_cli, 4), threads=1, lca_seconds=round(res.stats["seconds_total"], 6),
                parity_sample_match=hashlib.sha256(ours).hexdigest() == hashlib.sha256(ref.encode("latin-1")).hexdigest())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1000000)
    ap.add_argument("--hits", type=int, default=8)
    ap.add_argument("--labels", type=int, default=200000)
    ap.add_argument("--genera", type=int, default=5000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--cutoff", type=float, default=0.8)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    labels, genus = silva_labels(a.labels, a.genera, 449)
    T = lc.LabelBlob(labels)
    raw = simulated_hits(a.queries, a.hits, genus, a.genera, 451)
    record = dict(bench="lca", queries=a.queries, hits=int(raw[0][-1]), labels=a.labels, genera=a.genera, label_bytes=len(T.blob), cutoff=a.cutoff,
                  steps=a.steps, modes={})
    with Aligner(device=0) as al:
        t = time.perf_counter()
        index = lc.LcaIndex(T, ctx=al)
        record["index"] = dict(seconds=round(time.perf_counter() - t, 6), split={k: round(index.stats[k], 6) for k in INDEX},
                               counts={k: index.stats[k] for k in COUNTS})
        t = time.perf_counter()
        again = lc.LcaIndex(T, ctx=al)
        record["index"]["second_build_seconds"] = round(time.perf_counter() - t, 6)
        again.close()
        t = time.perf_counter()
        host_index = lc.LcaIndex(T)
        record["index"]["host_seconds"] = round(time.perf_counter() - t, 6)
        record["index"]["host_split_equal"] = all(np.array_equal(x, y) for x, y in zip(index.split(), host_index.split()))
        for mode, top in (("plain", False), ("top_hits_only", True)):
            first, times, (t_med, res) = timed(lambda: lc.lca(index, raw, lca_cutoff=a.cutoff, top_hits_only=top), a.steps)
            st = res.stats
            r = dict(device=dict(first_call=first, seconds=round(t_med, 6), all=times, split={k: round(st[k], 6) for k in SPLIT},
                                 counts={k: st[k] for k in COUNTS}),
                     depth_histogram=np.bincount(res.depth, minlength=10).tolist(), mean_n_top=round(float(res.n_top.mean()), 3))
            if not a.no_host:
                _, htimes, (h_med, hres) = timed(lambda: lc.lca_host(T, raw, lca_cutoff=a.cutoff, top_hits_only=top, threads=16), 3)
                r["host_restatement"] = dict(seconds=round(h_med, 6), all=htimes, threads=16, equal=hres.arrays() == res.arrays())
                assert r["host_restatement"]["equal"], "the device and the host restatement differ"
                _, itimes, (i_med, ires) = timed(lambda: lc.lca(host_index, raw, lca_cutoff=a.cutoff, top_hits_only=top, threads=16), 3)
                r["host_index_route"] = dict(seconds=round(i_med, 6), all=itimes, threads=16, equal=ires.arrays() == res.arrays())
                assert r["host_index_route"]["equal"], "the device and the host index route differ"
            record["modes"][mode] = r
            print(f"{mode}: device {r['device']['seconds']} s (vote {st['seconds_vote']:.4f} s)", file=sys.stderr, flush=True)
        index.close()
        host_index.close()
        if os.path.exists(ld.ref_binary()) and not a.no_cli:
            record["cli"] = cli_sample(al)
            assert record["cli"]["parity_sample_match"], "the --lcaout text differs from the reference CLI's on the sample"
    line = json.dumps(record, separators=(",", ":"))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
