#!/usr/bin/env python3
"""Secondary bench: de novo chimera detection (--uchime_denovo / --uchime2_denovo / --uchime3_denovo) through
vsearch_amd.DenovoChimeraSession (vsx_uchime_denovo).  An amplicon-like set: families of 300-500 bp (a few variants per family at
~2 % divergence), Zipf-like abundances, and about 20 % two- and three-parent chimeras of the variants at lower abundance, some of
them abundant enough to be candidate parents of later chimeras.  Reports sequences/s, the seconds split, the speculative passes and
-- when oracle/_ref/vsearch_ref exists -- the reference CLI's one-thread wall time and a parity digest on a PREFIX of the
abundance-sorted input: a prefix of a sorted input is a self-contained de novo run, so the first K lines of the full run must equal
the CLI's lines on the first K sequences.  Prints ONE JSON line.

  python bench_uchime_denovo.py [--seqs 20000 --prefix 2000 --variant uchime]
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


def workload(n, seed=2027, chimera_frac=0.2):
    """(labels, sequences) in a shuffled input order; labels carry ;size="""
    rng = np.random.default_rng(seed)
    n_chim = int(n * chimera_frac)
    n_good = n - n_chim
    good = []
    while len(good) < n_good:
        anc = ALPHA[rng.integers(0, 4, int(rng.integers(300, 501)))]
        for _ in range(min(int(rng.integers(3, 12)), n_good - len(good))):
            good.append(_mut(rng, anc, 0.02))
    # Zipf-like abundances over the non-chimeras, in a random rank order
    ranks = rng.permutation(n_good) + 1
    gsize = np.maximum(1, (20000.0 / ranks ** 1.1).astype(np.int64))
    seqs, sizes = list(good), [int(x) for x in gsize]
    for i in range(n_chim):
        k = 2 if i % 3 else 3
        ps = [int(x) for x in rng.choice(n_good, k, replace=False)]
        m = min(good[p].size for p in ps)
        cuts = sorted(int(x) for x in rng.choice(np.arange(m // 6, m - m // 6), k - 1, replace=False))
        edges = [0] + cuts + [None]
        seqs.append(_mut(rng, np.concatenate([good[p][edges[j]:edges[j + 1]] for j, p in enumerate(ps)]), 0.003))
        top = max(1, min(sizes[p] for p in ps) // 4)
        sizes.append(int(rng.integers(1, top + 1)))
    order = rng.permutation(len(seqs))
    labels = [f"s{j};size={sizes[j]}" for j in order]
    return labels, [seqs[j].tobytes() for j in order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=20_000)
    ap.add_argument("--prefix", type=int, default=2000, help="sorted sequences run through the reference CLI (0 = none)")
    ap.add_argument("--variant", default="uchime", choices=["uchime", "uchime2", "uchime3"])
    ap.add_argument("--window", type=int, default=0)
    args = ap.parse_args()

    from oracle import refcli
    from vsearch_amd import Aligner, DenovoChimeraSession

    t0 = time.time()
    labels, seqs = workload(args.seqs)
    gen_s = time.time() - t0
    with Aligner(device=0) as al:
        warm = DenovoChimeraSession(al, seqs[:512], labels[:512], variant=args.variant, window=args.window)
        warm.uchime_denovo()                                            # warm-up: kernels, pools
        warm.close()
        t1 = time.time()
        s = DenovoChimeraSession(al, seqs, labels, variant=args.variant, window=args.window)
        setup_s = time.time() - t1
        t2 = time.time()
        recs = s.uchime_denovo()
        wall = time.time() - t2
        st = dict(s.stats)
        lines = s.uchimeout(recs)
        sorted_seqs, sorted_labels = s.seqs, s.labels
        s.close()
    flags = [r["flag"] for r in recs]
    r3 = lambda x: round(x, 3)
    res = {"bench": "uchime_denovo", "variant": args.variant, "seqs": len(seqs), "wall_s": r3(wall), "seqs_per_s": round(len(seqs) / wall, 1),
           "seconds_rank": r3(st["seconds_rank"]), "seconds_members": r3(st["seconds_members"]), "seconds_search": r3(st["seconds_search"]),
           "seconds_align": r3(st["seconds_align"]), "seconds_eval": r3(st["seconds_eval"]), "seconds_reconcile": r3(st["seconds_reconcile"]),
           "windows": st["windows"], "passes": st["passes"], "passes_max": st["passes_max"], "queries_reevaluated": st["queries_reevaluated"],
           "pairs_searched": st["pairs_searched"], "pairs_aligned": st["pairs_aligned"], "queries_kernel": st["queries_kernel"],
           "queries_host": st["queries_host"], "chimeras_Y": flags.count("Y"), "suspicious": flags.count("?"),
           "setup_s": r3(setup_s), "workload_gen_s": round(gen_s, 2)}
    if args.prefix and refcli.available():
        k = min(args.prefix, len(seqs))
        with tempfile.TemporaryDirectory(prefix="vsxref_") as tmp:
            f, uo = os.path.join(tmp, "in.fa"), os.path.join(tmp, "u.tsv")
            refcli.write_fasta(f, sorted_labels[:k], sorted_seqs[:k])
            secs = refcli.run([f"--{args.variant}_denovo", f, "--uchimeout", uo, "--threads", "1", "--quiet"])
            ref = open(uo).read().splitlines()
        mine = lines[:k]
        if ref != mine:
            diff = [(a, b) for a, b in zip(mine, ref) if a != b]
            print(f"{len(diff)} prefix lines differ; first ones (vsx / ref):", file=sys.stderr)
            for a, b in diff[:5]:
                print(f"  vsx {a}\n  ref {b}", file=sys.stderr)
        dig = lambda ls: hashlib.sha256("\n".join(ls).encode()).hexdigest()[:16]
        res.update({"ref_prefix": k, "ref_threads": 1, "ref_prefix_s": r3(secs), "ref_prefix_seqs_per_s": round(k / secs, 1),
                    "parity_digest_ref": dig(ref), "parity_digest_vsx": dig(mine), "parity_match": ref == mine})
    print(json.dumps(res))
    return 0 if res.get("parity_match", True) else 1


if __name__ == "__main__":
    sys.exit(main())
