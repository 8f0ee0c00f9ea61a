#!/usr/bin/env python3
"""profiles/early_stop/skipped.py [qlen dlen db] -- the share of DP steps the early stop skips on the benchmark's workload, measured:
Timing.steps_skipped of one plan run over the steps its tasks were planned with (longest padded target + 16 per task)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from vsearch_amd import Aligner, SequenceSet, workload      # noqa: E402


def main():
    qlen = int(sys.argv[1]) if len(sys.argv) > 1 else 250
    dlen = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    dbn = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
    nq, cands = 100_000, 8
    dev = torch.device("cuda", 0)
    db_ascii, db_off, db_len, fam = workload.make_family_db(dbn, dlen, seed=17, device=dev)
    q_ascii, q_off, q_len, src = workload.make_queries(db_ascii, db_off, db_len, nq, qlen, seed=11, device=dev)
    qidx, tidx = workload.family_candidates(src, fam, per_query=cands, seed=5)
    with Aligner(device=0) as al:
        T = SequenceSet(al, blob=db_ascii.numel(), offsets=db_off, lengths=db_len, device_ptr=db_ascii.data_ptr())
        Q = SequenceSet(al, blob=q_ascii.numel(), offsets=q_off, lengths=q_len, device_ptr=q_ascii.data_ptr())
        plan = al.plan(Q, T, qidx, tidx)
        info = plan.describe()
        plan.run()
        tm = plan.sync()
        plan.close()
    dmax = db_len[tidx].reshape(nq, cands).max(axis=1).astype(np.int64)
    steps = int((((dmax + 3) & ~3) + 16).sum())
    print(f"{qlen} x {dlen}: tasks {info['tasks']} (split {info['tasks_split']}, max3 {info['tasks_max3']}), steps {steps}, "
          f"skipped {int(tm.steps_skipped)} = {100.0 * tm.steps_skipped / steps:.2f} %, forward {tm.forward_ms:.3f} ms")


if __name__ == "__main__":
    main()
