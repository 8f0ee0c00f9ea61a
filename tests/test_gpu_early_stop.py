"""The early stop of the DP kernel (vsx_forward_kernel EARLY): a whole-wave single-strip MAX3 task ends once the rest of
every target is a proven right-terminal gap, and forms score and leave column from the closed form (tests/test_early_stop_math.py holds
the proof's model).  Every field of every pair, CIGAR included, against the oracle; Timing.steps_skipped tells whether the exit was taken.
The shapes are small and sit where the exit can go wrong: no / most dummy rows, both row classes that have the split-profile kernel and the
byte-profile kernel beside them, a phase A too short to look, targets of very different lengths, empty slots, Q + D near the MAX3 bound,
a scoring and a query outside the class."""
import random

import numpy as np
import pytest

from tests import common

IU = common.IUPAC + "ACGT" * 6


def _target(rng, q, n, off, div, alpha="ACGT"):
    """n symbols: a mutated copy of q from column off on, between random flanks"""
    t = common.rnd_seq(rng, off) + common.mutate(rng, q, div)
    t = (t + common.rnd_seq(rng, n))[:n]
    return "".join(c if c in alpha else rng.choice("ACGT") for c in t)


def _run(oracle, qs, ts, qi, ti, scoring="default"):
    """one plan -> (steps skipped, plan description); asserts parity of every pair"""
    from vsearch_amd import Aligner
    sc = common.load_golden()["scorings"][scoring]
    P, nmm = tuple(sc["P"]), bool(sc["n_mismatch"])
    qi, ti = np.array(qi, np.uint32), np.array(ti, np.uint32)
    with Aligner(scoring=P, n_mismatch=nmm) as al:
        p = al.plan(al.sequences(qs), al.sequences(ts), qi, ti)
        info = p.describe()
        p.run()
        skipped = int(p.sync().steps_skipped)
        res = p.fetch()
        p.close()
    for k in range(len(qi)):
        assert res.row(k) == tuple(oracle.align(qs[qi[k]], ts[ti[k]], P, nmm)), (k, len(qs[qi[k]]), len(ts[ti[k]]))
    print(scoring, [len(q) for q in qs], info, "skipped", skipped)
    return skipped, info


def _tasks_of_eight(rng, q, centres, off, div, impure=False, per_task=8):
    """targets of a query in groups whose lengths lie within +-12 of a centre each (the planner sorts a query's targets by falling
    length and cuts eight to a task: the groups stay together); impure: one IUPAC symbol in one target of every group"""
    ts = []
    for ctr in centres:
        for x in range(per_task):
            t = _target(rng, q, ctr + rng.randint(-12, 12), off + rng.randint(0, 3), div)
            if impure and x == 2:
                p = rng.randrange(len(t))
                t = t[:p] + "N" + t[p + 1:]
            ts.append(t)
    return ts


@pytest.mark.gpu
@pytest.mark.parametrize("Q", [250, 256, 241])
def test_exit_taken_rows16(gpu_required, oracle, Q):
    # R = 16: the split-profile class; 256 = no dummy rows, 241 = 15 of them; a copy at a common offset, long overhangs
    rng = random.Random(100 + Q)
    q = common.rnd_seq(rng, Q)
    ts = _tasks_of_eight(rng, q, (600, 1000, 1480), 40, 0.06)
    skipped, info = _run(oracle, [q], ts, [0] * len(ts), range(len(ts)))
    assert info["tasks_split"] == 3 and info["rows_dominant"] == 16
    assert skipped > 0


@pytest.mark.gpu
@pytest.mark.parametrize("Q", [145, 160])
def test_exit_taken_rows10_byte_profile(gpu_required, oracle, Q):
    # R = 10 with IUPAC symbols on both sides: the byte-profile single-strip class (an impure target keeps a task out of SPLIT)
    rng = random.Random(200 + Q)
    q = common.rnd_seq(rng, Q, IU)
    ts = _tasks_of_eight(rng, q, (600, 1000, 1480), 25, 0.04, impure=True)
    skipped, info = _run(oracle, [q], ts, [0] * len(ts), range(len(ts)))
    assert info["tasks_split"] == 0 and info["tasks_max3"] == 3 and info["rows_dominant"] == 10
    assert skipped > 0


@pytest.mark.gpu
def test_targets_that_end_on_the_query_never_exit(gpu_required, oracle):
    rng = random.Random(3)
    q = common.rnd_seq(rng, 250)
    ts = [common.rnd_seq(rng, 700 + rng.randint(0, 8)) + q for _ in range(8)]
    skipped, _ = _run(oracle, [q], ts, [0] * 8, range(8))
    assert skipped == 0


@pytest.mark.gpu
def test_parity_where_the_exit_is_hard(gpu_required, oracle):
    rng = random.Random(4)
    qs, ts, qi, ti = [], [], [], []

    def add(q, targets):
        qs.append(q)
        for t in targets:
            qi.append(len(qs) - 1); ti.append(len(ts)); ts.append(t)

    # one unrelated target among seven related
    q = common.rnd_seq(rng, 250)
    add(q, _tasks_of_eight(rng, q, (900,), 30, 0.08, per_task=7) + [common.rnd_seq(rng, 905)])
    # a weak copy followed by an exact copy
    q = common.rnd_seq(rng, 241)
    add(q, [(common.rnd_seq(rng, 20 + x) + common.mutate(rng, q, 0.25) + common.rnd_seq(rng, 60) + q + common.rnd_seq(rng, 400))[:1000 + x]
            for x in range(8)])
    # targets of very different lengths: a long phase B
    q = common.rnd_seq(rng, 250)
    add(q, [_target(rng, q, n, 10, 0.05) for n in (252, 300, 420, 640, 900, 1200, 1400, 1500)])
    # a task of five targets: empty slots
    q = common.rnd_seq(rng, 256)
    add(q, _tasks_of_eight(rng, q, (800,), 50, 0.05, per_task=5))
    # Q + D near the MAX3 bound
    q = common.rnd_seq(rng, 250)
    add(q, [_target(rng, q, 1578 - x, 100, 0.05) for x in range(8)])
    # D - Q in 1 .. 40
    q = common.rnd_seq(rng, 250)
    add(q, [_target(rng, q, 250 + d, d // 2, 0.03) for d in (1, 2, 5, 16, 17, 31, 33, 40)])
    q = common.rnd_seq(rng, 145, IU)
    add(q, [_target(rng, q, 145 + d, 0, 0.03, alpha=IU) for d in (1, 3, 8, 15, 24, 32, 39, 40)])
    _run(oracle, qs, ts, qi, ti)


@pytest.mark.gpu
def test_outside_the_class_nothing_is_skipped(gpu_required, oracle):
    rng = random.Random(5)
    # zero terminal penalties: no MAX3 class (the right-end gap open is 0)
    q = common.rnd_seq(rng, 250)
    ts = _tasks_of_eight(rng, q, (900,), 40, 0.05)
    skipped, info = _run(oracle, [q], ts, [0] * 8, range(8), scoring="zero_terminal")
    assert skipped == 0 and info["tasks_max3"] == 0
    # a multi-strip query
    q = common.rnd_seq(rng, 530)
    ts = _tasks_of_eight(rng, q, (1100,), 20, 0.05)
    skipped, _ = _run(oracle, [q], ts, [0] * 8, range(8))
    assert skipped == 0
