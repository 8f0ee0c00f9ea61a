"""-m gpu: ONE plan that passes through every stage of vsx_plan_create (vsx_plan.cpp) at once, pinned as a whole.

The kernel classes are asserted piecemeal elsewhere (test_gpu_parity, test_gpu_split_profile, test_gpu_tb_fused_text,
test_gpu_walk_batch, test_gpu_early_stop); here one fixed pair list holds every situation the planner distinguishes, and what
Plan.describe() and the Timing of one run report for it is compared with tests/golden/plan_shape.json.  Those numbers are RECORDED
(from the planner as it was before its stages were split into functions), not derived: a change of any of them is a change of what
the planner decides, and has to be meant.  The results themselves must equal those of a single-chunk plan of the same pairs."""
import json
import os
import random

import pytest

from tests import common, poison_cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_shape.json")
CHUNK_BUDGET = 1 << 20       # bytes of checkpoints per chunk: below the tracked and the multi-strip task, about four sparse waves
WHOLE_BUDGET = 1 << 30       # one chunk
TIMING_FIELDS = ("forward_launches", "traceback_launches", "cells", "dir_bytes")


def _target(rng, q, length, impure=False):
    """a mutated copy of q, cut or padded to `length` symbols; impure: one N in the middle"""
    t = common.mutate(rng, q, 0.08)[:length]
    t += common.rnd_seq(rng, length - len(t))
    if impure:
        t = t[:length // 2] + "N" + t[length // 2 + 1:]
    return t


def plan_shape_pairs():
    """-> (queries, targets, qidx, tidx).  Default scoring: every task below 7 966 symbols of query + target is of the MAX3 class."""
    rng = random.Random(20261021)
    qs, ts, pairs = [], [], []

    def query(qlen, tlens, impure_at=()):
        q = common.rnd_seq(rng, qlen)
        qs.append(q)
        for k, tl in enumerate(tlens):
            ts.append(_target(rng, q, tl, k in impure_at))
            pairs.append((len(qs) - 1, len(ts) - 1))

    # 14 rows per lane, 116 targets of one length, one of them with an N: fourteen full tasks, thirteen of them eligible -> three PAIR
    # groups of four and a whole-wave remainder; the last four targets are a sparse task (nq = 2).  Three groups exceed the budget.
    query(200, [220] * 116, impure_at=(43,))
    # 20 rows, one or two targets each: the large sparse class (nq = 4), seventeen waves -> several chunks
    for k in range(70):
        query(300, [300 - k, 290][:1 + k % 2])
    # 18 rows, two tasks beside seventy with 20 rows: merge_thin_row_classes moves them
    query(280, [280])
    query(286, [270, 260])
    # three and four targets: nq = 2
    for k in range(6):
        query(150, [160, 150, 140, 130][:3 + k % 2])
    # nine targets: a full task and a one-target task
    query(150, [150 + 3 * k for k in range(9)])
    # 16 and 10 rows, whole-wave, every target pure: the split class; the same with an N among the targets: not
    query(250, [260] * 8)
    query(250, [240 + k for k in range(6)])
    query(150, [170] * 7)
    query(250, [260] * 8, impure_at=(5,))
    # 4 rows, shorter than one pipeline position of the large class: stays where it is
    query(20, [20, 25])
    # longer than 16 x 32 rows: two strips
    query(600, [580])
    # no_overflow_possible refuses 100 + 8 000 symbols: the tracked class
    query(100, [8000])
    # closed forms: empty query, empty target, beyond search16_fits (600 x 42 000 > 25 000 000)
    query(0, [50])
    query(120, [0])
    query(600, [42000])
    # the planner sorts by query itself: hand the pairs over in a fixed scattered order
    n = len(pairs)
    order = sorted(range(n), key=lambda k: ((k * 7919) % n, k))
    return qs, ts, [pairs[k][0] for k in order], [pairs[k][1] for k in order]


def test_plan_shape(gpu_required):
    """describe() and the launch / cell / checkpoint figures of one run equal the recorded ones; rows equal a single-chunk plan's"""
    from vsearch_amd import Aligner
    qs, ts, qi, ti = plan_shape_pairs()
    assert 200 <= len(qi) <= 500
    with Aligner() as al:
        rows, _, info, tm = poison_cases.plan_rows(al, qs, ts, qi, ti, dir_budget_bytes=CHUNK_BUDGET)
        whole_rows, _, whole_info, _ = poison_cases.plan_rows(al, qs, ts, qi, ti, dir_budget_bytes=WHOLE_BUDGET)
    seen = {"pairs": len(qi), "describe": info, "timing": {k: int(getattr(tm, k)) for k in TIMING_FIELDS}, "describe_whole": whole_info}
    print("plan_shape: " + json.dumps(seen, sort_keys=True))
    # the input holds what it is meant to hold (a recorded zero would pin nothing)
    for k in ("tasks_sparse", "tasks_pair", "tasks_split", "tasks_tracked", "tasks_max3"):
        assert info[k] > 0, (k, info)
    assert info["chunks"] >= 3 and whole_info["chunks"] == 1, (info, whole_info)
    with open(GOLDEN) as f:
        want = json.load(f)
    assert seen == want
    assert rows == whole_rows
