#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY: randomized soak of vsx_merge_pairs (vsx_merge.hip and the host route) against the REFERENCE CLI
(vsearch_ref --fastq_mergepairs), byte for byte, and of the device against the host path (VSX_MERGE=host), field for field.

A round: 100-300 pairs of tests/merge_data.generate() at a random read length in 20 .. 512, a random quality encoding (--fastq_ascii
33 or 64, qmin / qmax / qminout / qmaxout inside what both programs accept: ascii + qmin >= 33, ascii + qmax <= 126, ascii + qmaxout
<= 126), 0-5 pairs longer than the kernel's 512 (host route), a random window, and each of the 13 merge options with probability
0.3.  Compared: the merged FASTQ with --fastq_eeout, the --eetabbedout lines, the labels of the pairs not merged, the reason counts.
A round the reference refuses counts as failing.  --reference-only counts the reference's lines without a device.

    python oracle/soak_merge.py --seconds 120 --seed 1 --out soak_merge.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from tests import merge_data as md  # noqa: E402


def draw(rng):
    """-> (options of merge_pairs / run_reference, generate()'s encoding keywords, read length, pairs, long pairs, window)"""
    read_len = int(rng.integers(20, 513))
    ascii = int(rng.choice([33, 64]))
    qmin = int(rng.integers(-5 if ascii == 64 else 0, 11))
    qmax = int(rng.integers(qmin + 20, 126 - ascii + 1))
    o = {}
    if ascii != 33:
        o["ascii"] = ascii
    if qmin != 0:
        o["qmin"] = qmin
    if qmax != 41:
        o["qmax"] = qmax
    qminout = int(rng.integers(0, 21))
    choices = {
        "minovlen": lambda: int(rng.integers(5, 21)), "maxdiffs": lambda: int(rng.integers(0, 9)),
        "maxdiffpct": lambda: float(rng.choice([2.0, 5.0, 10.0])), "truncqual": lambda: int(rng.integers(qmin, qmin + 16)),
        "maxns": lambda: int(rng.integers(0, 4)), "maxee": lambda: float(rng.choice([0.5, 1.0, 2.0])),
        "minmergelen": lambda: int(rng.integers(read_len // 2, read_len + 1)), "maxmergelen": lambda: int(rng.integers(read_len, 2 * read_len)),
        "qminout": lambda: qminout, "qmaxout": lambda: int(rng.integers(max(qminout, 20), 126 - ascii + 1)),
        "minlen": lambda: int(rng.integers(5, read_len // 2 + 1)), "maxlen": lambda: int(rng.integers(read_len - 5, read_len + 50)),
        "allowmergestagger": lambda: True,
    }
    for key, pick in choices.items():
        v = pick()                       # (always drawn: the stream of random numbers does not depend on which options are set)
        if rng.random() < 0.3:
            o[key] = v
    if o.get("qminout", 0) > o.get("qmaxout", 41):
        o["qmaxout"] = int(min(126 - ascii, o["qminout"] + 20))
    enc = dict(ascii=ascii, qrange=(qmin if rng.random() < 0.3 else max(qmin, 2), qmax))
    return o, enc, read_len, int(rng.integers(100, 301)), int(rng.integers(0, 6)), int(rng.choice([0, 1, 7, 64, 1000]))


def data(rng, enc, read_len, n, n_long):
    d = [list(c) for c in md.generate(int(rng.integers(1, 2 ** 31)), n, read_len=read_len, **enc)]
    lg = md.generate(int(rng.integers(1, 2 ** 31)), n_long, read_len=int(rng.integers(513, 700)), **enc)
    for k in range(n_long):
        at = int(rng.integers(0, len(d[0]) + 1))
        for col, src in zip(d, lg):
            col.insert(at, src[k])
    d[0] = [f"p{k}" for k in range(len(d[0]))]
    return d


def compare(res, labels, ref):
    """the first difference as a dict, or None"""
    pairs = (("fastq", res.fastq_lines(labels, eeout=True), ref["fastq"]), ("eetabbed", res.eetabbed_lines(), ref["eetabbed"]),
             ("notmerged", [labels[k] for k in res.not_merged_indices()], ref["notmerged"]))
    for what, got, exp in pairs:
        if got != exp:
            first = next((i for i, (x, y) in enumerate(zip(got, exp)) if x != y), min(len(got), len(exp)))
            return {"what": what, "lines": [len(got), len(exp)], "first_diff": first, "got": got[first] if first < len(got) else None,
                    "exp": exp[first] if first < len(exp) else None}
    if res.reason_counts() != ref["reasons"]:
        return {"what": "reasons", "got": res.reason_counts(), "exp": ref["reasons"]}
    return None


def same_records(a, b):
    return all((a.records[n].view(np.uint64) if a.records[n].dtype.kind == "f" else a.records[n]).tolist() ==
               (b.records[n].view(np.uint64) if b.records[n].dtype.kind == "f" else b.records[n]).tolist() for n in a.records.dtype.names) \
        and a.seq_blob == b.seq_blob and a.qual_blob == b.qual_blob


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    ap.add_argument("--max-rounds", type=int, default=0, help="stop after this many rounds (0: run for --seconds): a deterministic set of rounds for a given seed")
    ap.add_argument("--reference-only", action="store_true", help="run the reference alone and count its lines (no device)")
    a = ap.parse_args()
    if not os.path.exists(md.ref_binary()):
        raise SystemExit("oracle/_ref/vsearch_ref missing: make -C oracle ref_full")
    al = None
    if not a.reference_only:
        from vsearch_amd import Aligner
        from vsearch_amd.merge import merge_pairs
        al = Aligner()
    rng = np.random.default_rng(a.seed)
    t_end = time.time() + a.seconds
    rounds = lines = bad = 0
    ref_seconds = 0.0
    failing = []
    while time.time() < t_end and (a.max_rounds <= 0 or rounds < a.max_rounds):
        o, enc, read_len, n, n_long, window = draw(rng)
        d = data(rng, enc, read_len, n, n_long)
        ref = md.run_reference(*d, **o)
        ref_seconds += ref["seconds"]
        rounds += 1
        cli = {**o, "read_len": read_len, "pairs": len(d[0]), "long": n_long, "window": window, "qrange": list(enc["qrange"])}
        if ref["returncode"] != 0:
            bad += 1
            if len(failing) < 10:
                failing.append({"cli": cli, "round": rounds - 1, "error": ref["stderr"][-300:]})
            continue
        lines += len(ref["fastq"]) + len(ref["eetabbed"]) + len(ref["notmerged"])
        if a.reference_only:
            continue
        res = merge_pairs(al, *d[1:], window=window, **o)
        diff = compare(res, d[0], ref)
        if diff is None and res.stats["pairs_host"] != sum(len(f) > 512 or len(r) > 512 for f, r in zip(d[1], d[3])):
            diff = {"what": "pairs_host", "got": res.stats["pairs_host"]}
        if diff is None:
            os.environ["VSX_MERGE"] = "host"
            try:
                host = merge_pairs(None, *d[1:], **o)
            finally:
                del os.environ["VSX_MERGE"]
            if not same_records(res, host):
                diff = {"what": "device and host records differ"}
        if diff is not None:
            bad += 1
            if len(failing) < 10:
                failing.append({"cli": cli, "round": rounds - 1, **diff})
    if al is not None:
        al.close()
    out = {"rounds": rounds, "lines": lines, "failing_rounds": bad, "failures": failing, "seed": a.seed, "seconds": a.seconds,
           "reference_seconds": round(ref_seconds, 3),
           "what": "vsx_merge_pairs (device, host route for long reads, VSX_MERGE=host) vs vsearch_ref --fastq_mergepairs with the same randomly drawn options and encoding"}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
