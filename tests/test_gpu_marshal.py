"""-m gpu: the stage between the traceback and the caller -- the dense run buffer, vsx_cigar_text_kernel (vsx_tbtext.hip), settle() /
fetch_core() / fetch_ranked_lists() and the device-to-device exports (vsx_fetch.cpp) -- on the inputs of tests/marshal_data.py.

Expected values are the scalar oracle's rows, field for field and CIGAR included (a pair the filter rejects keeps its numbers and loses
its CIGAR; tests/test_marshal_host.py asserts without a device that the inputs reach their edges).  The overflow recovery is reached
through the size hooks VSX_TEST_RUNS_CAP / VSX_TEST_TEXT_CAP (read by vsx_plan_create: a smaller FIRST capacity, nothing else) and
observed through Aligner.settle_counts(): every forced test asserts on the counters, so none can pass by never overflowing.  An
overflow is a bounds-checked skip on the device followed by the designed resize and re-run; nothing here provokes a fault."""
import ctypes as C
import json
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import marshal_data as md

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT_CASES = [c["name"] for c in md.digit_edges() + md.wave_edges()]


def _case(name):
    if name.startswith("mixed"):
        return md.dense_mixed(int(name[5:]))
    return {c["name"]: c for c in md.digit_edges() + md.wave_edges() + (md.dense_runs(),)}[name]


@pytest.fixture(scope="module")
def want(oracle):
    """name, filter -> (rows, verdicts) by the oracle; computed once per case and filter, never changed"""
    memo = {}

    def get(name, flt=None):
        key = (name, json.dumps(flt, sort_keys=True))
        if key not in memo:
            if (name, "null") not in memo:
                memo[(name, "null")] = (md.oracle_rows(_case(name), oracle), None)
            rows = memo[(name, "null")][0]
            memo[key] = (rows, None) if flt is None else md.filtered_rows(_case(name), rows, md.full_filter(**flt))
        return memo[key]
    return get


class _Loaded:
    """an Aligner with a case's sequences on the device"""

    def __init__(self, case):
        from vsearch_amd import Aligner
        self.case = case
        self.al = Aligner(scoring=case["P"])
        self.Q, self.T = self.al.sequences(case["queries"]), self.al.sequences(case["targets"])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.al.close()

    def plan(self, flt=None, budget=0):
        p = self.al.plan(self.Q, self.T, self.case["qidx"], self.case["tidx"], dir_budget_bytes=budget)
        if flt is not None:
            p.set_filter(**flt)
        return p

    def fetch(self, flt=None, budget=0):
        """a fresh plan: run, fetch -> (AlignmentResults, cigar_off, blob)"""
        p = self.plan(flt, budget)
        try:
            p.run()
            return _fetch_raw(p)
        finally:
            p.close()


def _fetch_raw(plan):
    from vsearch_amd import _lib
    from vsearch_amd.aligner import AlignmentResults
    lib, res = _lib.load(), _lib.Results()
    _lib.check(lib.vsx_plan_fetch(plan.h, C.byref(res)), "vsx_plan_fetch")
    try:
        n = int(res.n_pairs)
        off = np.ctypeslib.as_array(res.cigar_off, shape=(n,)).astype(np.uint64, copy=True) if n else np.zeros(0, np.uint64)
        blob = C.string_at(res.cigar_blob, int(res.cigar_bytes)) if res.cigar_bytes else b""
        assert all(blob.find(b"\0", int(o)) >= 0 for o in off), "a CIGAR string is not terminated inside the blob"
        return AlignmentResults(res), off, blob
    finally:
        lib.vsx_results_free(C.byref(res))


def _assert_rows(res, rows, verdicts=None, what=""):
    assert len(res) == len(rows)
    bad = [(k, res.row(k), rows[k]) for k in range(len(rows)) if res.row(k) != rows[k]]
    assert not bad, f"{what}: {len(bad)} of {len(rows)} rows differ from the oracle, first: {bad[:2]}"
    if verdicts is not None:
        assert res.verdict is not None and res.verdict.tolist() == verdicts, what


def _device_used(case, rows):
    """(run words, text bytes) the device pairs of these rows occupy, by the oracle"""
    dev = [rows[k] for k in range(len(rows)) if k not in set(case["host"])]
    return md.used_words(dev), sum(md.padded(r[5]) for r in dev)


def _assert_layout(case, rows, off, blob):
    """the device text: dword-aligned strings that tile [0, text_used) without overlap, zero padding; behind it the strings of the
    pairs the host answered, in pair order, unpadded (their offsets are therefore not aligned)"""
    host = set(case["host"])
    dev = [k for k in range(len(rows)) if k not in host]
    spans = sorted((int(off[k]), md.padded(rows[k][5]), k) for k in dev)
    at = 0
    for o, size, k in spans:
        assert o % 4 == 0, (k, o)
        assert o == at, f"pair {k}: string at {o}, the previous one ends at {at}"
        s = rows[k][5].encode()
        assert blob[o:o + size] == s + b"\0" * (size - len(s)), (k, blob[o:o + size], s)
        at = o + size
    assert at == _device_used(case, rows)[1]
    for k in case["host"]:
        s = rows[k][5].encode() + b"\0"
        assert int(off[k]) == at and blob[at:at + len(s)] == s, k
        at += len(s)
    assert at == len(blob)


def _export_cigars(plan, n):
    """the plan's records and run words through vsx_plan_export_hits / vsx_plan_export_runs, device-to-device in the order a rank of
    the multi-GPU gather makes the calls, copied to the host (Plan.export_host: a process can initialise only one HIP runtime, and
    torch's own copy finds no device once libvsx has started, so the torch buffers of sharding.export_records are covered in a child
    process, test_export_records_settles_an_overflowed_plan); every CIGAR is rebuilt with vsx_cigar_from_runs
    -> (records dict, cigars, number of run words)"""
    from vsearch_amd import sharding
    rec, runs = plan.export_host()
    assert rec.shape == (n, sharding.HIT_RECORD_BYTES)
    d = sharding.decode_records(rec)
    assert int((d["run_off"] + d["nruns"])[d["nruns"] > 0].max(initial=0)) <= len(runs), "a record points past the exported run words"
    return d, sharding.cigars_from_gather(rec, runs), len(runs)


def _host_words(case, rows):
    return sum(1 for k in case["host"] if rows[k][5])


# ---- 1. the text kernel's edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TEXT_CASES)
def test_text_edges(gpu_required, want, name):
    """digit counts 1 | 2 ... 9999 | 10000 up to the longest run, every string length mod 4, pair counts around one wave and one block,
    invalid lanes in the last wave, zero-run pairs between pairs with many, host-answered strings behind the device text; and the
    kernel's formatter against the host's (vsx_cigar_from_runs) on the same exported run words"""
    case = _case(name)
    flt = md.FILTER if name.startswith("wave") else None
    rows, verdicts = want(name, flt)
    with _Loaded(case) as L:
        before = L.al.settle_counts()
        p = L.plan(flt)
        p.run()
        res, off, blob = _fetch_raw(p)
        rec, cigars, n_words = _export_cigars(p, len(rows))
        p.close()
        assert L.al.settle_counts() == before
    _assert_rows(res, rows, verdicts, name)
    _assert_layout(case, rows, off, blob)
    assert cigars == res.cigar == [r[5] for r in rows]
    assert n_words == _device_used(case, rows)[0] + _host_words(case, rows)
    assert rec["score"].tolist() == [r[0] for r in rows] and rec["aligned"].tolist() == [r[1] for r in rows]


# ---- 2. / 3. forced overflow of the run buffer and of the text buffer ---------------------------------------------------------------
@pytest.mark.parametrize("name,flt", [("wave257", None), ("wave257", md.FILTER), ("squares", None), ("overhangs", None)],
                         ids=["wave257", "wave257-filtered", "squares", "overhangs"])
def test_forced_overflows(gpu_required, want, monkeypatch, name, flt):
    """fresh plans under VSX_TEST_RUNS_CAP in {1, used / 2, used - 1, used}: the plan runs again exactly when the capacity is below
    `used` (the <= of the traceback epilogue, the > of the settling); under VSX_TEST_TEXT_CAP in {4, text / 2, text - 4, text}: only the
    text kernel runs again; both together: a plan re-run followed by a text re-run.  Every row equals the oracle every time."""
    case = _case(name)
    rows, verdicts = want(name, flt)
    used, text_used = _device_used(case, rows)
    with _Loaded(case) as L:
        p = L.plan(flt)
        p.run()
        assert p.export_runs() == used + _host_words(case, rows)          # the size query: what the device used = what the oracle says
        res, off, blob = _fetch_raw(p)
        p.close()
        assert len(blob) - sum(len(rows[k][5]) + 1 for k in case["host"]) == text_used
        _assert_rows(res, rows, verdicts, "unforced")
        assert L.al.settle_counts() == (0, 0)
        plans = texts = 0
        for cap, step in ((1, 1), (used // 2, 1), (used - 1, 1), (used, 0)):
            monkeypatch.setenv("VSX_TEST_RUNS_CAP", str(cap))
            res, off, blob = L.fetch(flt)
            plans += step
            print(f"{name}: run cap {cap} of {used}: counters {L.al.settle_counts()}")
            assert L.al.settle_counts() == (plans, texts), (cap, used)
            _assert_rows(res, rows, verdicts, f"run cap {cap}")
            _assert_layout(case, rows, off, blob)
        monkeypatch.delenv("VSX_TEST_RUNS_CAP")
        for cap, step in ((4, 1), (text_used // 2, 1), (text_used - 4, 1), (text_used, 0)):
            monkeypatch.setenv("VSX_TEST_TEXT_CAP", str(cap))
            res, off, blob = L.fetch(flt)
            texts += step
            print(f"{name}: text cap {cap} of {text_used}: counters {L.al.settle_counts()}")
            assert L.al.settle_counts() == (plans, texts), (cap, text_used)
            _assert_rows(res, rows, verdicts, f"text cap {cap}")
            _assert_layout(case, rows, off, blob)
        monkeypatch.setenv("VSX_TEST_RUNS_CAP", str(used // 2))
        monkeypatch.setenv("VSX_TEST_TEXT_CAP", str(text_used // 2))
        res, off, blob = L.fetch(flt)
        assert L.al.settle_counts() == (plans + 1, texts + 1)
        _assert_rows(res, rows, verdicts, "both caps")
        _assert_layout(case, rows, off, blob)


def test_forced_overflows_ranked(gpu_required, want, monkeypatch):
    """vsx_align_pairs_ranked on the 257-pair case under the same capacities: the kept list equals the unforced one and the one derived
    from the oracle (each pair is a query of its own: kept pairs in pair order), the refused pair is listed once, kept <= n"""
    case = _case("wave257")
    rows, verdicts = want("wave257", md.RANKED_FILTER)
    used, text_used = _device_used(case, rows)
    kept = [k for k, v in enumerate(verdicts) if v == 1]
    keys = ("pair", "score", "aligned", "matches", "mismatches", "gaps", "verdict", "id")

    def check(got, first, what):
        assert got["pair"].tolist() == kept and len(kept) <= len(rows), what
        assert [(int(got["score"][x]), int(got["aligned"][x]), int(got["matches"][x]), int(got["mismatches"][x]), int(got["gaps"][x]),
                 got["cigar"][x]) for x in range(len(kept))] == [rows[k] for k in kept], what
        assert sorted(got["undecided"].tolist()) == sorted(case["host"] + case["refused"]), what          # (each once: not doubled by the second run)
        assert got["verdict"].tolist() == [1] * len(kept)
        if first is not None:
            assert all(np.array_equal(got[key], first[key]) for key in keys) and got["cigar"] == first["cigar"], what

    with _Loaded(case) as L:
        first = L.al.align_pairs_ranked(L.Q, L.T, case["qidx"], case["tidx"], md.RANKED_FILTER)
        check(first, None, "unforced")
        assert L.al.settle_counts() == (0, 0)
        plans = texts = 0
        for var, caps in (("VSX_TEST_RUNS_CAP", ((1, 1), (used // 2, 1), (used - 1, 1), (used, 0))),
                          ("VSX_TEST_TEXT_CAP", ((4, 1), (text_used // 2, 1), (text_used - 4, 1), (text_used, 0)))):
            for cap, step in caps:
                monkeypatch.setenv(var, str(cap))
                got = L.al.align_pairs_ranked(L.Q, L.T, case["qidx"], case["tidx"], md.RANKED_FILTER)
                plans, texts = plans + (step if "RUNS" in var else 0), texts + (step if "TEXT" in var else 0)
                assert L.al.settle_counts() == (plans, texts), (var, cap)
                check(got, first, f"{var}={cap}")
            monkeypatch.delenv(var)


# ---- 4. chunks and the pipeline ------------------------------------------------------------------------------------------------
def test_forced_overflows_in_a_chunked_plan(gpu_required, want, monkeypatch):
    """a plan cut into several chunks that share one checkpoint block: with half the run words and half the text bytes it needs, the
    early chunks fit and the later ones do not; the plan and then its text kernel run again, and a further run of the settled plan
    (its buffers now exact) does not"""
    name = "mixed720"
    case = _case(name)
    rows, _ = want(name)
    used, text_used = _device_used(case, rows)
    monkeypatch.setenv("VSX_TEST_RUNS_CAP", str(used // 2))
    monkeypatch.setenv("VSX_TEST_TEXT_CAP", str(text_used // 2))
    with _Loaded(case) as L:
        p = L.plan(budget=1 << 20)
        assert p.describe()["chunks"] >= 3, p.describe()
        p.run()
        res, off, blob = _fetch_raw(p)
        assert L.al.settle_counts() == (1, 1)
        p.run()
        again, off2, blob2 = _fetch_raw(p)
        p.close()
        assert L.al.settle_counts() == (1, 1)
    _assert_rows(res, rows, None, "chunked")
    _assert_rows(again, rows, None, "chunked, second run")
    _assert_layout(case, rows, off, blob)
    _assert_layout(case, rows, off2, blob2)


_PIPE_SNIPPET = r"""
import json, sys
import numpy as np
sys.path.insert(0, %r)
from oracle import pyoracle
from tests import marshal_data as md
from vsearch_amd import Aligner
case = md.dense_mixed(md.PIPE_PAIRS)
rows = md.oracle_rows(case, pyoracle.Oracle())
dev = [k for k in range(len(rows)) if k not in set(case["host"])]
out = {}
with Aligner(scoring=case["P"]) as al:
    Q, T = al.sequences(case["queries"]), al.sequences(case["targets"])
    res = al.align_pairs_oneshot(Q, T, case["qidx"], case["tidx"])
    out["plain"] = al.settle_counts()
    bad = [k for k in range(len(rows)) if res.row(k) != rows[k]]
    assert not bad, ("plain", len(bad), bad[:3], res.row(bad[0]), rows[bad[0]])
    rk = al.align_pairs_ranked(Q, T, case["qidx"], case["tidx"], {})
    out["ranked"] = al.settle_counts()
    assert rk["pair"].tolist() == dev and sorted(rk["undecided"].tolist()) == case["host"], "ranked lists"
    got = [(int(rk["score"][x]), int(rk["aligned"][x]), int(rk["matches"][x]), int(rk["mismatches"][x]), int(rk["gaps"][x]), rk["cigar"][x])
           for x in range(len(dev))]
    assert got == [rows[k] for k in dev], "ranked rows"
print("COUNTS", json.dumps(out))
"""


def test_forced_overflows_in_a_pipeline(gpu_required, want):
    """vsx_align_pairs / vsx_align_pairs_ranked over 4 200 pairs in nine pipelined slices (VSX_PIPELINE_SLICE is read once per process:
    a child process), capacities that the two quarter slices meet and the seven larger ones do not: a slice is run again while later
    slices are queued on the shared checkpoint blocks.  Every row equals the oracle (asserted in the child); each call re-runs exactly
    the seven overflowing slices' plans and text kernels."""
    case = _case(f"mixed{md.PIPE_PAIRS}")
    rows, _ = want(case["name"])
    cuts = md.pipeline_cuts(md.PIPE_PAIRS, md.PIPE_SLICE)
    over_runs, over_text = md.slice_overflows(case, rows, cuts, md.PIPE_RUNS_CAP, md.PIPE_TEXT_CAP)
    n_slices = len(cuts) - 1
    assert 1 <= sum(over_runs) < n_slices and 1 <= sum(over_text) < n_slices
    e = dict(os.environ)
    e.update({"VSX_PIPELINE_SLICE": str(md.PIPE_SLICE), "VSX_TEST_RUNS_CAP": str(md.PIPE_RUNS_CAP), "VSX_TEST_TEXT_CAP": str(md.PIPE_TEXT_CAP)})
    e.pop("VSX_PIPELINE", None)
    p = subprocess.run([sys.executable, "-c", _PIPE_SNIPPET % ROOT], env=e, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    counts = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("COUNTS")][0][7:])
    print("pipeline counters:", counts, "slices overflowing:", sum(over_runs), sum(over_text), "of", n_slices)
    assert 1 <= counts["plain"][0] <= n_slices and 1 <= counts["plain"][1] <= n_slices
    assert counts["plain"] == [sum(over_runs), sum(over_text)]
    assert counts["ranked"] == [2 * sum(over_runs), 2 * sum(over_text)]


# ---- 5. the exports ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wave257", "mixed720"])
def test_exports_settle_an_overflowed_plan(gpu_required, want, monkeypatch, name):
    """run, then export the records and the run words without any fetch (what sharding.export_records does for a rank of the
    multi-GPU gather) under half the run words the plan needs: the exports run the plan again themselves; (n_cigar_runs,
    cigar_run_offset) with the exported words rebuild every CIGAR, host-answered pairs included"""
    case = _case(name)
    rows, _ = want(name)
    used, _ = _device_used(case, rows)
    monkeypatch.setenv("VSX_TEST_RUNS_CAP", str(used // 2))
    with _Loaded(case) as L:
        p = L.plan()
        p.run()
        rec, cigars, n_words = _export_cigars(p, len(rows))
        assert L.al.settle_counts() == (1, 0)
        res, off, blob = _fetch_raw(p)                     # a fetch after the exports finds the plan settled
        p.close()
        assert L.al.settle_counts() == (1, 0)
    assert n_words == used + _host_words(case, rows)
    assert cigars == [r[5] for r in rows]
    for x, key in enumerate(("score", "aligned", "matches", "mismatches", "gaps")):
        assert rec[key].tolist() == [r[x] for r in rows], key
    _assert_rows(res, rows, None, "fetch after export")


_EXPORT_SNIPPET = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, %r)
torch.cuda.set_device(0)
from oracle import pyoracle
from tests import marshal_data as md
from vsearch_amd import Aligner, sharding
case = md.wave_case(257)
rows = md.oracle_rows(case, pyoracle.Oracle())
with Aligner(scoring=case["P"]) as al:
    Q, T = al.sequences(case["queries"]), al.sequences(case["targets"])
    plan = al.plan(Q, T, case["qidx"], case["tidx"])
    plan.run()
    rec, runs = sharding.export_records(plan, len(rows))
    counts = al.settle_counts()
    assert rec.is_cuda and runs.is_cuda
    d = sharding.decode_records(rec)
    assert int((d["run_off"] + d["nruns"]).max()) <= runs.numel(), "a record points past the exported run words"
    cig = sharding.cigars_from_gather(rec, runs)
    got = [(int(d["score"][k]), int(d["aligned"][k]), int(d["matches"][k]), int(d["mismatches"][k]), int(d["gaps"][k]), cig[k])
           for k in range(len(rows))]
    bad = [k for k in range(len(rows)) if got[k] != rows[k]]
    assert not bad, (len(bad), bad[:3], got[bad[0]], rows[bad[0]])
    plan.close()
print("COUNTS", json.dumps(counts))
"""


def test_export_records_settles_an_overflowed_plan(gpu_required, want):
    """the same through sharding.export_records itself, into torch buffers (a child process: torch has to start the HIP runtime
    before libvsx does): run, export, no fetch, under half the run words the 257-pair case needs"""
    case = _case("wave257")
    used, _ = _device_used(case, want("wave257")[0])
    e = dict(os.environ, VSX_TEST_RUNS_CAP=str(used // 2))
    e.pop("VSX_TEST_TEXT_CAP", None)
    p = subprocess.run([sys.executable, "-c", _EXPORT_SNIPPET % ROOT], env=e, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("COUNTS")][0][7:]) == [1, 0]


# ---- 6. a search command under both capacities -----------------------------------------------------------------------------------
def test_search_userout_under_both_caps(gpu_required, tmp_path, monkeypatch):
    """SearchSession.userout on a small family database with both hooks at tiny values: line for line the unforced output and the
    reference CLI's --userout"""
    from tests import test_gpu_mask as M
    from vsearch_amd import Aligner, SearchSession
    M._need_ref()
    rng = random.Random(6262)
    db = M._masked_families(rng, 40, 5, 420, 0.05, False)
    qs = M._queries(rng, db, 150, 200, 0.03, False)
    exp = M._reference_userout(str(tmp_path), db, qs, [], ["--id", "0.8", "--maxaccepts", "2", "--maxrejects", "4"])
    outs = []
    for caps in (None, ("16", "64")):
        if caps:
            monkeypatch.setenv("VSX_TEST_RUNS_CAP", caps[0])
            monkeypatch.setenv("VSX_TEST_TEXT_CAP", caps[1])
        with Aligner() as al:
            ss = SearchSession(al, db, id=0.8, maxaccepts=2, maxrejects=4, strand_both=0, soft_mask=2)
            outs.append(ss.userout(qs, fields=M.FIELDS))
            counts = al.settle_counts()
        assert (counts[0] >= 1 and counts[1] >= 1) if caps else counts == (0, 0), counts
    assert len(exp) > 100
    assert outs[1] == outs[0], M._first_diff(outs[1], outs[0])
    assert outs[1] == exp, M._first_diff(outs[1], exp)


# ---- 7. the natural capacities ---------------------------------------------------------------------------------------------------
def test_natural_capacities_overflow_without_a_hook(gpu_required, want, monkeypatch):
    """131 072 pairs over the 24 of dense_runs() in one plan, no hook: about 24.6 M run words against the first 16 Mi + 1 and about
    38.8 MB of text against 32 MiB + 16 (tests/test_marshal_host.py proves both from the oracle): the plan and then its text kernel run
    again, every row equals its oracle row"""
    monkeypatch.delenv("VSX_TEST_RUNS_CAP", raising=False)
    monkeypatch.delenv("VSX_TEST_TEXT_CAP", raising=False)
    case = _case("dense")
    rows, _ = want("dense")
    idx = md.dense_index(md.NATURAL_PAIRS)
    with _Loaded(case) as L:
        t0 = time.time()
        p = L.al.plan(L.Q, L.T, idx, idx)
        p.run()
        res = p.fetch()
        wall = time.time() - t0
        tm = p.sync()                                   # the events of the plan's LAST run, the second one
        p.close()
        # the plan really holds every index pair: its DP cells are the sum of Q x D over all 131 072 pairs (about 10.8 G per run)
        cells = int(sum(len(case["queries"][k]) * len(case["targets"][k]) for k in range(24)) * (md.NATURAL_PAIRS // 24)
                    + sum(len(case["queries"][k]) * len(case["targets"][k]) for k in range(md.NATURAL_PAIRS % 24)))
        print(f"natural capacities: {md.NATURAL_PAIRS} pairs = {tm.cells / 1e9:.2f} G cells per run; planned, run twice and fetched in "
              f"{wall:.3f} s; second run on the device {tm.total_ms:.2f} ms (DP {tm.forward_ms:.2f}, traceback {tm.traceback_ms:.2f}) = "
              f"{tm.cells / tm.total_ms / 1e6:.0f} GCUPS")
        assert int(tm.cells) == cells and cells > 10 * 10 ** 9
        assert L.al.settle_counts() == (1, 1)
    for x, arr in enumerate((res.score, res.aligned, res.matches, res.mismatches, res.gaps)):
        assert np.array_equal(arr.astype(np.int64), np.array([r[x] for r in rows], np.int64)[idx]), x
    cig = [r[5] for r in rows]
    bad = [k for k in range(len(idx)) if res.cigar[k] != cig[idx[k]]]
    assert not bad, (len(bad), bad[:3])
