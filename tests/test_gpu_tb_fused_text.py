"""-m gpu: the traceback epilogues format the CIGAR text and write the output arrays themselves (VSX_TB_FUSED_TEXT: vsx_marshal_pair of
vsearch_amd/csrc/vsx_tbtext.h, called by vsx_traceback_tilt_kernel and vsx_traceback_ck_kernel).  Plans of hand-made sequences, every
field and the CIGAR of every pair against the scalar oracle (oracle.pyoracle.Oracle), and the device text's layout: dword-aligned
strings that tile [0, text used) without a hole, zero padding.

The pairs of a class share one traceback launch in pair order (each query here is a sequence of its own, or its pairs are
neighbours), so a case's pair count is its launch's lane count: 1, 63, 64, 65 and 130 leave invalid lanes in the last wave, whose
lane 0 still makes the wave's one allocation.  Which kernel a plan's pairs went to is asserted through Plan.describe(): the tilted
kernel needs a tilted task of R >= 4 rows (vsx_launch_traceback_ck); a query under four symbols has R = 1, and a target long enough
for the planner's no_overflow_possible() to fail makes the task a tracked one: both keep vsx_traceback_ck_kernel."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import common
from tests import marshal_data as md

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = md.DEFAULT
CORE = "CGTCGTCGTCGTCGTCGTCG"                                    # 20 symbols, no A: inside A flanks it aligns as <left>I 20M <right>I
FLANKS = ((9, 1001), (10, 1000), (99, 911), (100, 910), (999, 11), (1000, 10))      # targets of 1 030 symbols
WAVE_COUNTS = (1, 63, 64, 65, 130)
IUPAC = "NRYWSKMBDHV"


def _case(pairs):
    """[(query, target)] -> a case; equal queries share an index (and so a task, as far as they are neighbours)"""
    qs, ts, qidx, tidx = {}, {}, [], []
    for q, t in pairs:
        qidx.append(qs.setdefault(q, len(qs)))
        tidx.append(ts.setdefault(t, len(ts)))
    return dict(P=P, queries=list(qs), targets=list(ts), qidx=np.array(qidx, np.uint32), tidx=np.array(tidx, np.uint32))


def _kind(rng, k):
    if k % 4 == 0:                                                # identical: one run
        s = common.rnd_seq(rng, rng.randint(17, 64))
        return s, s
    if k % 4 == 1:                                                # terminal gaps across 9 | 10, 99 | 100, 999 | 1000
        a, b = FLANKS[(k // 4) % len(FLANKS)]
        return CORE, "A" * a + CORE + "A" * b
    s = common.rnd_seq(rng, 64)
    if k % 4 == 2:                                                # interior gaps of 1 and 2: their counts 1 are omitted
        return s, s[:20] + s[21:42] + common.rnd_seq(rng, 2) + s[42:]
    q = list(s[:48])                                              # N and IUPAC symbols on both sides
    for x in rng.sample(range(48), 6):
        q[x] = rng.choice(IUPAC)
    t = list(common.mutate(rng, s[:48], 0.05))
    t[rng.randrange(len(t))] = "N"
    return "".join(q), "".join(t)


def wave_pairs(n):
    """n pairs of one class (queries of 17 .. 64 symbols: R = 4, tilted), kinds in turn"""
    rng = random.Random(4242 + n)
    return [_kind(rng, k if n > 1 else 1) for k in range(n)]


def short_pairs(n):
    """queries of 1 .. 3 symbols: R = 1, the first traceback kernel whatever the scoring class"""
    rng = random.Random(77)
    return [(common.rnd_seq(rng, 1 + k % 3), common.rnd_seq(rng, rng.randint(1, 40))) for k in range(n)]


def tracked_pairs(n, refused_at):
    """20-symbol queries inside targets of 8 000: Q + D is past what no_overflow_possible() admits under the default scoring, so the
    tasks are tracked ones (R = 4) on vsx_traceback_ck_kernel; pair `refused_at` has 40 000 A for a target: its score leaves int16, the
    DP kernel flags it (VsxSlotOut::overflow) and the lane in the middle of the wave gets the sentinel row and the empty string"""
    rng = random.Random(8000)
    out = []
    for k in range(n):
        q = common.rnd_seq(rng, 20, "CGT")
        a = rng.randint(1, 7000)
        out.append((q, "A" * 40000) if k == refused_at else (q, "A" * a + q + "A" * (7980 - a)))
    return out


def mixed_pairs():
    rng = random.Random(11)
    s = common.rnd_seq(rng, 250)
    long_t = common.rnd_seq(rng, 2400) + s + common.rnd_seq(rng, 2350)      # 250 x 5 000: no overflow possible, but not tilted
    return wave_pairs(65) + [(s, s), (s, long_t)] + short_pairs(5) + tracked_pairs(9, 4)


CASES = {f"wave{n}": (lambda n=n: wave_pairs(n)) for n in WAVE_COUNTS}
CASES.update(identical=lambda: [(s, s) for s in (common.rnd_seq(random.Random(250), 250),)], short=lambda: short_pairs(65),
             tracked=lambda: tracked_pairs(70, 30), mixed=mixed_pairs)


def expected(case, orc):
    memo = {}
    return [memo.setdefault((q, t), tuple(orc.align(case["queries"][q], case["targets"][t], case["P"])))
            for q, t in zip(case["qidx"].tolist(), case["tidx"].tolist())]


@pytest.fixture(scope="module")
def want(oracle):
    """name -> (case, oracle rows), computed once and never changed"""
    memo = {}

    def get(name):
        if name not in memo:
            case = _case(CASES[name]())
            memo[name] = (case, expected(case, oracle))
        return memo[name]
    return get


def fetch_raw(plan):
    from vsearch_amd import _lib
    from vsearch_amd.aligner import AlignmentResults
    lib, res = _lib.load(), _lib.Results()
    _lib.check(lib.vsx_plan_fetch(plan.h, C.byref(res)), "vsx_plan_fetch")
    try:
        n = int(res.n_pairs)
        off = np.ctypeslib.as_array(res.cigar_off, shape=(n,)).astype(np.uint64, copy=True)
        blob = C.string_at(res.cigar_blob, int(res.cigar_bytes)) if res.cigar_bytes else b""
        return AlignmentResults(res), off, blob
    finally:
        lib.vsx_results_free(C.byref(res))


def check(res, off, blob, rows, what):
    """every row, then the layout of the text (no pair of these cases is answered by the host: all of it is device text)"""
    assert len(res) == len(rows)
    bad = [(k, res.row(k), rows[k]) for k in range(len(rows)) if res.row(k) != rows[k]]
    assert not bad, f"{what}: {len(bad)} of {len(rows)} rows differ from the oracle, first: {bad[:2]}"
    at = 0
    for o, k in sorted((int(off[k]), k) for k in range(len(rows))):
        size, s = md.padded(rows[k][5]), rows[k][5].encode()
        assert o % 4 == 0 and o == at, f"{what}: pair {k}: string at {o}, the one before ends at {at}"
        assert blob[o:o + size] == s + b"\0" * (size - len(s)), (what, k, blob[o:o + size], s)
        at = o + size
    assert at == len(blob) == sum(md.padded(r[5]) for r in rows), what


class Loaded:
    def __init__(self, case):
        from vsearch_amd import Aligner
        self.case = case
        self.al = Aligner(scoring=case["P"])
        self.Q, self.T = self.al.sequences(case["queries"]), self.al.sequences(case["targets"])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.al.close()

    def plan(self):
        return self.al.plan(self.Q, self.T, self.case["qidx"], self.case["tidx"])


def run_case(case, rows, what):
    """a fresh plan: run, fetch, check -> its description"""
    with Loaded(case) as L:
        p = L.plan()
        info = p.describe()
        p.run()
        res, off, blob = fetch_raw(p)
        p.close()
        assert L.al.settle_counts() == (0, 0), what
    check(res, off, blob, rows, what)
    return info


def _run_lengths(rows):
    return {n for r in rows for n, _ in md.runs_of(r[5])}


@pytest.mark.parametrize("n", WAVE_COUNTS)
def test_tilted_kernel_pair_counts(gpu_required, want, n):
    case, rows = want(f"wave{n}")
    info = run_case(case, rows, f"wave{n}")
    assert info["tasks_tilted"] == info["tasks"] and info["tasks_tracked"] == 0 and info["rows_dominant"] == 4, info
    if n >= 63:                                                   # the inputs reach the edges they were made for
        assert {9, 10, 99, 100, 999, 1000, 1001} <= _run_lengths(rows)
        cig = [r[5] for r in rows]
        assert any(re.search(r"M[ID]\d+M", c) for c in cig) and any(re.search(r"M2[ID]\d+M", c) for c in cig), "gaps of 1 and of 2"
        assert any(re.fullmatch(r"\d+M", c) for c in cig)
        assert len({len(c) % 4 for c in cig}) >= 3                 # (tests/test_tbtext_format_host.py has every residue)
    else:
        assert rows[0][5] == "9I20M1001I"


def test_identical_sequences(gpu_required, want):
    case, rows = want("identical")
    assert rows[0][5] == "250M"
    info = run_case(case, rows, "identical")
    assert info["tasks_tilted"] == 1 and info["rows_dominant"] == 16, info


def test_first_kernel_short_queries(gpu_required, want):
    case, rows = want("short")
    info = run_case(case, rows, "short")
    assert info["rows_dominant"] == 1 and info["tasks"] >= 3, info               # R = 1: never the tilted kernel


def test_first_kernel_tracked_with_a_refused_pair_inside_a_wave(gpu_required, want):
    case, rows = want("tracked")
    assert rows[30] == md.SENTINEL_ROW and all(r != md.SENTINEL_ROW for k, r in enumerate(rows) if k != 30)
    info = run_case(case, rows, "tracked")
    assert info["tasks_tracked"] == info["tasks"] == 70 and info["tasks_tilted"] == 0, info


def test_plan_mixing_the_classes(gpu_required, want):
    case, rows = want("mixed")
    info = run_case(case, rows, "mixed")
    assert 0 < info["tasks_tilted"] < info["tasks"] and 0 < info["tasks_tracked"] < info["tasks"], info
    assert md.SENTINEL_ROW in rows and "250M" in [r[5] for r in rows]


def test_run_twice_and_short_buffers(gpu_required, want, monkeypatch):
    """the same plan run twice; then fresh plans whose first run buffer / text buffer hold half of what they need: a pair whose runs
    did not fit gets the lone NUL and the plan runs again (settle_runs), a string that does not fit is skipped while the cursor still
    counts it, and the text alone is made again by vsx_cigar_text_kernel from the records and the dense run words (settle)"""
    case, rows = want("mixed")
    used, text_used = md.used_words(rows), sum(md.padded(r[5]) for r in rows)
    with Loaded(case) as L:
        p = L.plan()
        for turn in (1, 2):
            p.run()
            check(*fetch_raw(p), rows, f"run {turn}")
        p.close()
        assert L.al.settle_counts() == (0, 0)
        counts = [0, 0]
        for var, cap, which in (("VSX_TEST_RUNS_CAP", used // 2, 0), ("VSX_TEST_TEXT_CAP", text_used // 2, 1), ("VSX_TEST_TEXT_CAP", 4, 1)):
            monkeypatch.setenv(var, str(cap))
            p = L.plan()
            p.run()
            check(*fetch_raw(p), rows, f"{var}={cap}")
            counts[which] += 1
            assert L.al.settle_counts() == tuple(counts), (var, cap)
            p.run()                                               # settled: its buffers are exact now
            check(*fetch_raw(p), rows, f"{var}={cap}, second run")
            assert L.al.settle_counts() == tuple(counts), (var, cap)
            p.close()
            monkeypatch.delenv(var)


_POISON_SNIPPET = r"""
import sys
sys.path.insert(0, %r)
from oracle import pyoracle
from tests import test_gpu_tb_fused_text as F
from vsearch_amd import _lib
assert _lib.load().vsx_internal_poison_byte() == 0xA5
orc = pyoracle.Oracle()
for name in ("wave130", "mixed"):
    case = F._case(F.CASES[name]())
    rows = F.expected(case, orc)
    with F.Loaded(case) as L:
        p = L.plan()
        p.run()
        F.check(*F.fetch_raw(p), rows, name)
        p.close()
print("POISON OK")
"""


def test_poisoned_memory(gpu_required):
    """every block the library hands out filled with 0xA5 first (VSX_POISON is read once per process: a child): no string byte, padding
    byte or array element may come from memory nobody wrote"""
    env = dict(os.environ, VSX_POISON="1")
    for k in ("VSX_POISON_BYTE", "VSX_TEST_RUNS_CAP", "VSX_TEST_TEXT_CAP"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-c", _POISON_SNIPPET % ROOT], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0 and "POISON OK" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
