#!/usr/bin/env python3
"""profiles/early_stop/predict.py [queries] [qlen] [tlen] -- the share of DP steps the early stop of the DP kernel should skip on the
benchmark's workload, from the plain-integer model of tests/test_early_stop_math.py (no GPU: workload.* with device="cpu").

A task is one query against its 8 family candidates.  The kernel looks between 16-step blocks of phase A, from t >= Q on, while
t + 32 <= t_switch = (shortest target - 1) & ~1; it ends the task at the first such t at which every target satisfies the criterion
after step t - 1, and skips steps - t with steps = longest padded target + 16.  (The model looks at every block; the kernel may look
a block or more later where it schedules its next look from the top border cell's shortfall, so this is an upper bound.)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import test_early_stop_math as M      # noqa: E402
from vsearch_amd import workload                 # noqa: E402


def main():
    nq = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    qlen = int(sys.argv[2]) if len(sys.argv) > 2 else 250
    tlen = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    R = 16 if qlen > 160 else 10
    db, off, ln, fam = workload.make_family_db(2000, tlen, device="cpu")
    qa, qoff, qln, src = workload.make_queries(db, off, ln, nq, qlen, device="cpu")
    qi, ti = workload.family_candidates(src, fam)
    db, qa = bytes(db.numpy()).decode(), bytes(qa.numpy()).decode()
    s = M.DEFAULT
    total = skipped = fired = 0
    scores = []
    for k in range(nq):
        q = qa[int(qoff[k]):int(qoff[k]) + int(qln[k])]
        ts = [db[int(off[x]):int(off[x]) + int(ln[x])] for x in ti[qi == k]]
        Q = len(q)
        sch = M.Schedule(Q, R)
        dmin, dmax = min(map(len, ts)), max(map(len, ts))
        steps = ((dmax + 3) & ~3) + 16
        t_switch = (dmin - 1) & ~1
        per = []
        for t in ts:
            H, En, htop, score, leave, margin, lv1s = M._dp(q, t, s)
            scores.append(score)
            per.append((M._plain_tables(sch, H, htop, s), H, En, htop, len(t)))
        t_exit = None
        t_ = (Q + 15) & ~15
        while t_ + 32 <= t_switch:
            if all(M._plain_criterion(sch, tabs, H, En, htop, D, s, t_ - 1)[0] for tabs, H, En, htop, D in per):
                t_exit = t_
                break
            t_ += 16
        total += steps
        if t_exit is not None:
            skipped += steps - t_exit
            fired += 1
        print(f"task {k}: Q {Q} D {dmin}..{dmax} steps {steps} exit {t_exit}", flush=True)
    print(f"tasks {nq}, exits {fired}, steps {total}, skipped {skipped} = {100.0 * skipped / total:.1f} %, "
          f"scores min/median/max {min(scores)}/{int(np.median(scores))}/{max(scores)}")


if __name__ == "__main__":
    main()
