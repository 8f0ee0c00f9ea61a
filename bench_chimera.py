#!/usr/bin/env python3
"""Secondary bench: --uchime_ref through vsearch_amd.ChimeraSession (vsx_uchime_ref).  A family reference database (N sequences of
300-600 bp, families of 50 at 3 % divergence) and Q queries: one third two-parent chimeras, one third three-parent chimeras, the rest
mutated members.  Reports queries/s and the seconds split into part search, whole-query alignment and evaluation, and -- when
oracle/_ref/vsearch_ref exists -- the reference CLI at 16 threads on a sample of the queries with a parity digest of the sample's
--uchimeout lines.  Prints ONE JSON line.

  python bench_chimera.py [--db 50000 --queries 20000 --sample 1000]
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


def workload(n_db, n_q, seed=2026):
    rng = np.random.default_rng(seed)
    db = []
    while len(db) < n_db:
        anc = ALPHA[rng.integers(0, 4, int(rng.integers(300, 601)))]
        for _ in range(min(50, n_db - len(db))):
            m = _mut(rng, anc, 0.03)
            cut = int(rng.integers(0, 4))                       # small length variation inside a family
            db.append(m[cut:m.size - int(rng.integers(0, 4))])
    qs = []
    for i in range(n_q):
        kind = i % 3
        if kind == 2:
            qs.append(_mut(rng, db[int(rng.integers(0, n_db))], 0.01))
            continue
        ps = [int(x) for x in rng.choice(n_db, kind + 2, replace=False)]
        n = min(db[p].size for p in ps)
        cuts = sorted(int(x) for x in rng.choice(np.arange(n // 6, n - n // 6), kind + 1, replace=False))
        edges = [0] + cuts + [None]
        qs.append(_mut(rng, np.concatenate([db[p][edges[j]:edges[j + 1]] for j, p in enumerate(ps)]), 0.01))
    return [d.tobytes() for d in db], [q.tobytes() for q in qs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db", type=int, default=50_000)
    ap.add_argument("--queries", type=int, default=20_000)
    ap.add_argument("--sample", type=int, default=1000, help="queries run through the reference CLI for the parity digest (0 = none)")
    ap.add_argument("--window", type=int, default=0)
    args = ap.parse_args()

    from oracle import refcli
    from vsearch_amd import Aligner, ChimeraSession

    t0 = time.time()
    db, qs = workload(args.db, args.queries)
    tn = [f"r{i}" for i in range(len(db))]
    qn = [f"q{i}" for i in range(len(qs))]
    gen_s = time.time() - t0
    with Aligner(device=0) as al:
        t1 = time.time()
        s = ChimeraSession(al, db, labels=tn, window=args.window)
        setup_s = time.time() - t1
        s.uchime_ref(qs[:min(len(qs), 256)])                    # warm-up: k-mer index, pools
        t2 = time.time()
        recs = s.uchime_ref(qs)
        wall = time.time() - t2
        st = dict(s.stats)
        lines = s.uchimeout(qs, qn, records=recs)
    flags = [r["flag"] if r["status"] == "scored" else "N" for r in recs]
    res = {"bench": "uchime_ref", "db": len(db), "queries": len(qs), "wall_s": round(wall, 3), "queries_per_s": round(len(qs) / wall, 1),
           "seconds_search": round(st["seconds_search"], 3), "seconds_align": round(st["seconds_align"], 3),
           "seconds_eval": round(st["seconds_eval"], 3), "windows": st["windows"], "pairs_aligned": st["pairs_aligned"],
           "sentinel_pairs": st["sentinel_pairs"], "queries_kernel": st["queries_kernel"], "queries_host": st["queries_host"],
           "chimeras_Y": flags.count("Y"), "suspicious": flags.count("?"), "setup_s": round(setup_s, 3), "workload_gen_s": round(gen_s, 2)}
    if args.sample and refcli.available():
        k = min(args.sample, len(qs))
        idx = np.linspace(0, len(qs) - 1, k).astype(int).tolist()
        with tempfile.TemporaryDirectory(prefix="vsxref_") as tmp:
            qf, df, uo = os.path.join(tmp, "q.fa"), os.path.join(tmp, "db.fa"), os.path.join(tmp, "u.tsv")
            refcli.write_fasta(qf, [qn[i] for i in idx], [qs[i] for i in idx])
            refcli.write_fasta(df, tn, db)
            thr = min(16, refcli.usable_cpus())
            secs = refcli.run(["--uchime_ref", qf, "--db", df, "--uchimeout", uo, "--threads", str(thr), "--quiet"])
            ref = sorted(open(uo).read().splitlines())           # (line order follows the reference's worker threads)
        mine = sorted(lines[i] for i in idx)
        if ref != mine:
            by = {ln.split("\t")[1]: ln for ln in ref}
            diff = [(ln, by.get(ln.split("\t")[1])) for ln in mine if by.get(ln.split("\t")[1]) != ln]
            print(f"{len(diff)} sample lines differ; first ones (vsx / ref):", file=sys.stderr)
            for a, b in diff[:5]:
                print(f"  vsx {a}\n  ref {b}", file=sys.stderr)
        dig = lambda ls: hashlib.sha256("\n".join(ls).encode()).hexdigest()[:16]
        res.update({"ref_sample": k, "ref_threads": thr, "ref_sample_s": round(secs, 3),
                    "ref_sample_queries_per_s": round(k / secs, 1), "parity_digest_ref": dig(ref), "parity_digest_vsx": dig(mine),
                    "parity_match": ref == mine})
    print(json.dumps(res))
    return 0 if res.get("parity_match", True) else 1


if __name__ == "__main__":
    sys.exit(main())
