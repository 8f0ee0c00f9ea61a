"""The split-profile classes of the DP kernel (vsx_forward_kernel SPLIT): whole-wave single-strip MAX3 tasks whose targets
are all plain A / C / G / T read their scores from two dword tables and add both to the diagonal in one v_add3_u32.  The class can only go
wrong at its edges, so the shapes are small: every row class around the two that have the kernel (R = 10, 16), no / most dummy rows,
targets of length 1, targets much shorter and much longer than the query (a long phase B), Q + D near the MAX3 bound, IUPAC queries
(eligible) and IUPAC targets (the task leaves the class), PAIR groups and sparse tasks beside it, chunk boundaries between its tasks.
Every field of every pair, CIGAR included, against the oracle; the switch is read once per process, so each mode is a child process."""
import os
import subprocess
import sys

import pytest

from tests import common

_SNIPPET = r"""
import os, random, sys
import numpy as np
sys.path.insert(0, %r)
from tests import common
from oracle import pyoracle
from vsearch_amd import Aligner
P = %r
nmm = %r
rng = random.Random(4711)
orc = pyoracle.Oracle()
IU = common.IUPAC + "ACGT" * 4
qs, ts, qi, ti = [], [], [], []

def related(q, lo, hi):
    # a target of exactly n symbols, n drawn from lo .. hi: a mutated copy of the query between random flanks, cut or padded
    n = rng.randint(lo, hi)
    t = common.rnd_seq(rng, rng.randint(0, max(0, n - len(q)))) + common.mutate(rng, q, 0.12)
    t = (t + common.rnd_seq(rng, n))[:n]
    return "".join(c if c in "ACGT" else rng.choice("ACGT") for c in t)        # (an IUPAC query must not make its targets leave the class)

def add(Q, alpha, lens, impure_at=()):
    # one query of Q symbols over `alpha`; a target per entry of lens = (lo, hi); targets listed in impure_at get one IUPAC symbol
    k = len(qs)
    qs.append(common.rnd_seq(rng, Q, alpha))
    for x, (lo, hi) in enumerate(lens):
        t = related(qs[k], lo, hi)
        if x in impure_at:
            p = rng.randrange(len(t))
            t = t[:p] + "N" + t[p + 1:]
        qi.append(k); ti.append(len(ts)); ts.append(t)

# (rows per lane of the query's class in brackets; the classes with the kernel are R = 10 and R = 16)
add(17, "ACGT", [(10, 60)] * 6)                                            # [4]  one task, not in the class
add(100, "ACGT", [(50, 300)] * 7)                                          # [8]  one task, not in the class
add(145, "ACGT", [(1, 1), (7, 7), (90, 144), (145, 145), (301, 303), (410, 700), (701, 703), (998, 999)])     # [10] one task of 8
add(160, IU, [(300, 640)] * 8 + [(20, 150)] * 4)                           # [10] IUPAC query: 8 -> the class, 4 -> a sparse task
add(250, "ACGT", [(260, 520)] * 40)                                        # [16] five tasks: a PAIR group of four and one left over
add(256, IU, [(600, 900)] * 8 + [(100, 500)] * 8, impure_at=(3,))          # [16] no dummy rows; the task of the long targets leaves
add(241, "ACGT", [(400, 800)] * 8 + [(1, 240)] * 5, impure_at=(10,))       # [16] 15 dummy rows; 8 + 5: the task of five leaves
add(300, "ACGT", [(200, 400)] * 5)                                         # [20] not in the class
add(250, "ACGT", [(1577, 1579), (1298, 1303), (897, 903), (597, 603), (297, 303), (49, 51), (7, 7), (1, 1)])  # [16] Q + D near the MAX3 bound
add(145, "ACGT", [(300, 500)] * 8 + [(10, 100)], impure_at=(2,))           # [10] 8 + 1: the task of eight leaves, the single is sparse
add(250, "ACGT", [(255, 262)] * 5)                                         # [16] a task of five
add(200, "ACGT", [(100, 700)] * 6)                                         # [14] not in the class
qi = np.array(qi, np.uint32); ti = np.array(ti, np.uint32)

# the planner's grouping, restated: a query's targets by falling length (stable), eight to a task
expect = 0
for k in range(len(qs)):
    mine = sorted([x for x in range(len(qi)) if qi[x] == k], key=lambda x: -len(ts[ti[x]]))
    tasks = [mine[b:b + 8] for b in range(0, len(mine), 8)]
    whole = [tk for tk in tasks if len(tk) > 4]                            # (<= 4 targets: a sparse task under the suite's VSX_SPARSE_MIN=1)
    pure = [tk for tk in whole if all(set(ts[ti[x]]) <= set("ACGT") for x in tk)]
    in_pair = len(pure) // 4 * 4 if (len(tasks) >= 4 and set(qs[k]) <= set("ACGT") and os.environ.get("VSX_PAIRPROF", "1") != "0") else 0
    if len(qs[k]) in (145, 160, 250, 256, 241):
        expect += len(pure) - in_pair
with Aligner(scoring=P, n_mismatch=nmm) as al:
    Qs, Ts = al.sequences(qs), al.sequences(ts)
    p = al.plan(Qs, Ts, qi, ti, dir_budget_bytes=int(os.environ.get("VSX_TEST_DIR_BUDGET", "0")))
    info = p.describe()
    p.run()
    res = p.fetch()
    p.close()
bad = 0
for k in range(len(qi)):
    if res.row(k) != tuple(orc.align(qs[qi[k]], ts[ti[k]], P, nmm)):
        bad += 1
print("INFO", info["tasks"], info["tasks_split"], info["tasks_max3"], info["tasks_pair"], info["tasks_sparse"], bad, info["chunks"], expect, len(qi))
"""

# tasks of the snippet's plan that meet every condition of the class when the scoring admits the MAX3 sub-class for all of them:
# 145: 1, 160: 1, 250 x 40: 1 (four go to the PAIR group), 256: 1 of 2, 241: 1 of 2, 250 (long): 1, 145 (8 + 1): 0, 250 x 5: 1
_DESIGNED = 7
_TASKS = 20
# default / nmismatch: reach = 4 * 18 + 2 * (Q + Dp + 64) * 4 < 15800 holds up to Q + Dp = 1901 (the snippet's largest: 250 + 1580);
# uniform10_1 has smaller penalties still.  zero_terminal has no MAX3 (right-end gap open 0), distinct12 cannot be tilted (the two
# interior gap extensions differ): no task may enter the class there.
_MAX3_SETS = ("default", "nmismatch", "uniform10_1")


def _run(name, env_extra):
    sc = common.load_golden()["scorings"][name]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ, **env_extra)
    p = subprocess.run([sys.executable, "-c", _SNIPPET % (root, tuple(sc["P"]), bool(sc["n_mismatch"]))], env=e, capture_output=True, text=True,
                       timeout=600, cwd=root)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    keys = ("tasks", "split", "max3", "pair", "sparse", "bad", "chunks", "expect", "pairs")
    out = dict(zip(keys, (int(x) for x in [ln for ln in p.stdout.splitlines() if ln.startswith("INFO")][-1].split()[1:])))
    print(name, env_extra, out)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "nmismatch", "zero_terminal", "uniform10_1", "distinct12"])
def test_split_profile_class(gpu_required, name):
    """Every field of every pair against the oracle with the class on and off; tasks_split is exactly the designed count under the scoring
    sets that admit MAX3 and 0 under the others and with VSX_SPLITPROF=0; PAIR groups and sparse tasks keep their tasks."""
    on = _run(name, {"VSX_SPLITPROF": "1"})
    off = _run(name, {"VSX_SPLITPROF": "0"})
    assert on["bad"] == 0 and off["bad"] == 0, (name, on, off)
    assert on["tasks"] == off["tasks"] == _TASKS and on["expect"] == _DESIGNED, (name, on, off)
    assert off["split"] == 0, (name, off)
    assert on["split"] == (_DESIGNED if name in _MAX3_SETS else 0), (name, on)
    assert (on["pair"], on["sparse"], on["max3"]) == (off["pair"], off["sparse"], off["max3"]), (name, on, off)
    if name in _MAX3_SETS:
        assert on["sparse"] == 2, (name, on)                              # the tasks of 4 and of 1 target
        assert on["pair"] == 4 and on["max3"] == _TASKS, (name, on)      # the PAIR group keeps precedence; every task is a MAX3 task


@pytest.mark.gpu
def test_split_profile_chunks_and_pair_off(gpu_required):
    """The same plan cut into several chunks by a small checkpoint budget -- chunk and launch boundaries fall between tasks of the class --
    and with the PAIR classes off, where the four tasks of the group join the class as well."""
    cut = _run("default", {"VSX_SPLITPROF": "1", "VSX_TEST_DIR_BUDGET": str(2 << 20)})
    assert cut["bad"] == 0 and cut["chunks"] >= 3 and cut["split"] == _DESIGNED, cut
    nopair = _run("default", {"VSX_SPLITPROF": "1", "VSX_PAIRPROF": "0"})
    assert nopair["bad"] == 0 and nopair["pair"] == 0 and nopair["split"] == nopair["expect"] == _DESIGNED + 4, nopair
