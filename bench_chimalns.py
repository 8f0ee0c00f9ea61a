#!/usr/bin/env python3
"""Secondary bench: the --uchimealns blocks of the chimeric records of bench_chimera.py's set (vsearch_amd.ChimeraSession.alns_raw ->
vsx_chimera_alns -> vsx_chimalns.hip).  The detection runs once (not timed here); the rendering of its 'Y' records is timed on the
kernel route and on the library's host restatement (VSX_CHIMALNS=host, 16 threads), each the median of --runs calls after a warm-up.
Reports records/s and the seconds split (re-alignment, kernel, download, host) of both, and -- when oracle/_ref/vsearch_ref exists --
a parity digest of the formatted text against the reference CLI (--threads 1: the file's order is the input's) on a sample of the
queries.  Prints ONE JSON line.

  python bench_chimalns.py [--db 50000 --queries 20000 --sample 1000 --runs 5]
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

from bench_chimera import workload  # noqa: E402

SPLIT = ("seconds_align", "seconds_kernel", "seconds_download", "seconds_host")


def timed(call, runs):
    """the median call of `runs` by wall time: (wall, its stats)"""
    out = []
    for _ in range(runs):
        t = time.perf_counter()
        r = call()
        out.append((time.perf_counter() - t, r.stats))
    out.sort(key=lambda x: x[0])
    return out[len(out) // 2], [round(w, 4) for w, _ in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db", type=int, default=50_000)
    ap.add_argument("--queries", type=int, default=20_000)
    ap.add_argument("--sample", type=int, default=1000, help="queries run through the reference CLI for the parity digest (0 = none)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--alignwidth", type=int, default=80)
    args = ap.parse_args()

    from oracle import refcli
    from vsearch_amd import Aligner, ChimeraSession

    db, qs = workload(args.db, args.queries)
    tn = [f"r{i}" for i in range(len(db))]
    qn = [f"q{i}" for i in range(len(qs))]
    threads = min(16, refcli.usable_cpus())
    with Aligner(device=0) as al:
        s = ChimeraSession(al, db, labels=tn)
        recs = s.uchime_ref(qs)
        n_y = sum(r["flag"] == "Y" for r in recs)
        dev_call = lambda: s.alns_raw(qs, recs, alignwidth=args.alignwidth)
        dev_call()                                              # warm-up: texts, pools
        (dev_wall, dev_st), dev_all = timed(dev_call, args.runs)
        os.environ["VSX_CHIMALNS"] = "host"
        try:
            host_call = lambda: s.alns_raw(qs, recs, alignwidth=args.alignwidth, threads=threads)
            host_call()
            (host_wall, host_st), host_all = timed(host_call, args.runs)
            host_arrays = host_call().arrays()
        finally:
            del os.environ["VSX_CHIMALNS"]
        same = host_arrays == dev_call().arrays()
        res = {"bench": "uchimealns", "db": len(db), "queries": len(qs), "records": n_y, "alignwidth": args.alignwidth, "runs": args.runs,
               "device_wall_s": round(dev_wall, 4), "device_records_per_s": round(n_y / dev_wall, 1), "device_walls": dev_all,
               "host_threads": threads, "host_wall_s": round(host_wall, 4), "host_records_per_s": round(n_y / host_wall, 1), "host_walls": host_all,
               "device_over_host": round(host_wall / dev_wall, 3), "routes_agree": bool(same),
               "records_kernel": dev_st["records_kernel"], "records_host_on_device_route": dev_st["records_host"]}
        for k in SPLIT:
            res["device_" + k] = round(dev_st[k], 4)
            res["host_" + k] = round(host_st[k], 4)
        if args.sample and refcli.available():
            k = min(args.sample, len(qs))
            sq, sn = qs[:k], qn[:k]
            t = time.perf_counter()
            mine = s.uchimealns(sq, sn, records=recs[:k], alignwidth=args.alignwidth)
            fmt_s = time.perf_counter() - t
            with tempfile.TemporaryDirectory(prefix="vsxref_") as tmp:
                qf, df, uo = os.path.join(tmp, "q.fa"), os.path.join(tmp, "db.fa"), os.path.join(tmp, "alns.txt")
                refcli.write_fasta(qf, sn, sq)
                refcli.write_fasta(df, tn, db)
                secs = refcli.run(["--uchime_ref", qf, "--db", df, "--uchimealns", uo, "--alignwidth", str(args.alignwidth), "--threads", "1", "--quiet"])
                ref = open(uo).read()
            dig = lambda t: hashlib.sha256(t.encode()).hexdigest()[:16]
            res.update({"ref_sample": k, "ref_sample_blocks": ref.count("\nQuery   ("), "ref_sample_s_whole_command_1_thread": round(secs, 3),
                        "sample_render_and_format_s": round(fmt_s, 3), "parity_digest_ref": dig(ref), "parity_digest_vsx": dig(mine),
                        "parity_match": ref == mine})
    print(json.dumps(res))
    return 0 if res.get("parity_match", True) and res["routes_agree"] else 1


if __name__ == "__main__":
    sys.exit(main())
