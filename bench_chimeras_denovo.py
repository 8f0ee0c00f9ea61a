#!/usr/bin/env python3
"""Secondary bench: long-read de novo chimera detection (--chimeras_denovo) through vsearch_amd.ChimerasDenovoSession
(vsx_chimeras_denovo).  Simulated full-length amplicons: families of 1 400-1 600 bp (a few variants per family at ~2 % divergence),
Zipf-like abundances, and about 20 % two- and three-parent chimeras of the variants joined at exact breakpoints, at lower abundance.
Reports sequences/s of the median of --repeats calls (every wall is listed), that call's seconds split, the speculative passes, the kernel / host counts and -- when oracle/_ref/vsearch_ref exists --
the reference CLI's one-thread wall time and a parity digest on a PREFIX of the abundance-sorted input (a prefix of a sorted input is
a self-contained de novo run).  Prints ONE JSON line.

  python bench_chimeras_denovo.py [--seqs 4000 --prefix 1000]
"""
import argparse
import hashlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

ALPHA = np.frombuffer(b"ACGT", np.uint8)


def _mut(rng, a, rate):
    a = a.copy()
    m = rng.random(a.size) < rate
    a[m] = ALPHA[rng.integers(0, 4, int(m.sum()))]
    return a


def workload(n, seed=2029, chimera_frac=0.2):
    """(labels, sequences) in a shuffled input order; labels carry ;size="""
    rng = np.random.default_rng(seed)
    n_chim = int(n * chimera_frac)
    n_good = n - n_chim
    good = []
    while len(good) < n_good:
        anc = ALPHA[rng.integers(0, 4, int(rng.integers(1400, 1601)))]
        for _ in range(min(int(rng.integers(3, 12)), n_good - len(good))):
            good.append(_mut(rng, anc, 0.02))
    ranks = rng.permutation(n_good) + 1
    gsize = np.maximum(1, (20000.0 / ranks ** 1.1).astype(np.int64))
    seqs, sizes = list(good), [int(x) for x in gsize]
    for i in range(n_chim):
        k = 2 if i % 3 else 3
        ps = [int(x) for x in rng.choice(n_good, k, replace=False)]
        m = min(good[p].size for p in ps)
        cuts = sorted(int(x) for x in rng.choice(np.arange(m // 6, m - m // 6), k - 1, replace=False))
        edges = [0] + cuts + [None]
        seqs.append(np.concatenate([good[p][edges[j]:edges[j + 1]] for j, p in enumerate(ps)]))
        sizes.append(int(rng.integers(1, max(1, min(sizes[p] for p in ps)) + 1)))
    order = rng.permutation(len(seqs))
    labels = [f"s{j};size={sizes[j]}" for j in order]
    return labels, [seqs[j].tobytes() for j in order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=4000)
    ap.add_argument("--prefix", type=int, default=1000, help="sorted sequences run through the reference CLI (0 = none)")
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5, help="timed calls on the same input; the median is reported, all walls are listed")
    args = ap.parse_args()

    from oracle import refcli
    from vsearch_amd import Aligner, ChimerasDenovoSession

    t0 = time.time()
    labels, seqs = workload(args.seqs)
    gen_s = time.time() - t0
    with Aligner(device=0) as al:
        warm = ChimerasDenovoSession(al, seqs[:256], labels[:256], window=args.window)
        warm.chimeras_denovo()                                          # warm-up: kernels, pools
        warm.close()
        runs = []
        for _ in range(max(1, args.repeats)):
            t1 = time.time()
            s = ChimerasDenovoSession(al, seqs, labels, window=args.window)
            setup_s = time.time() - t1
            t2 = time.time()
            recs = s.chimeras_denovo()
            runs.append((time.time() - t2, dict(s.stats), setup_s))
            if len(runs) < max(1, args.repeats):
                s.close()
        wall, st, setup_s = sorted(runs, key=lambda r: r[0])[len(runs) // 2]          # the median call and its own seconds split
        lines = s.tabbedout(recs)
        prefix_lines = s.tabbedout(recs[:args.prefix])                  # the lines of the first --prefix sorted sequences
        sorted_seqs, sorted_labels = s.seqs, s.labels
        s.close()
    r3 = lambda x: round(x, 3)
    res = {"bench": "chimeras_denovo", "seqs": len(seqs), "mean_len": round(sum(map(len, seqs)) / max(1, len(seqs)), 1),
           "wall_s": r3(wall), "seqs_per_s": round(len(seqs) / wall, 1), "walls_s": [r3(r[0]) for r in runs],
           "seconds_rank": r3(st["seconds_rank"]), "seconds_members": r3(st["seconds_members"]), "seconds_search": r3(st["seconds_search"]),
           "seconds_align": r3(st["seconds_align"]), "seconds_eval": r3(st["seconds_eval"]), "seconds_reconcile": r3(st["seconds_reconcile"]),
           "windows": st["windows"], "passes": st["passes"], "passes_max": st["passes_max"], "queries_reevaluated": st["queries_reevaluated"],
           "parts": st["parts"], "pairs_searched": st["pairs_searched"], "pairs_aligned": st["pairs_aligned"],
           "queries_kernel": st["queries_kernel"], "queries_host": st["queries_host"], "chimeras_Y": len(lines),
           "setup_s": r3(setup_s), "workload_gen_s": round(gen_s, 2)}
    if args.prefix and refcli.available():
        k = min(args.prefix, len(seqs))
        with tempfile.TemporaryDirectory(prefix="vsxref_") as tmp:
            f, to = os.path.join(tmp, "in.fa"), os.path.join(tmp, "t.tsv")
            refcli.write_fasta(f, sorted_labels[:k], sorted_seqs[:k])
            secs = refcli.run(["--chimeras_denovo", f, "--tabbedout", to, "--threads", "1", "--quiet"])
            ref = open(to).read().splitlines()
        mine = prefix_lines
        if ref != mine:
            diff = [(a, b) for a, b in zip(mine, ref) if a != b]
            print(f"prefix lines: vsx {len(mine)}, ref {len(ref)}, {len(diff)} differ; first ones (vsx / ref):", file=sys.stderr)
            for a, b in diff[:5]:
                print(f"  vsx {a}\n  ref {b}", file=sys.stderr)
        dig = lambda ls: hashlib.sha256("\n".join(ls).encode()).hexdigest()[:16]
        res.update({"ref_prefix": k, "ref_threads": 1, "ref_prefix_s": r3(secs), "ref_prefix_seqs_per_s": round(k / secs, 1),
                    "ref_prefix_chimeras": len(ref), "parity_digest_ref": dig(ref), "parity_digest_vsx": dig(mine), "parity_match": ref == mine})
    print(json.dumps(res))
    return 0 if res.get("parity_match", True) else 1


if __name__ == "__main__":
    sys.exit(main())
