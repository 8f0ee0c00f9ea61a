"""Read statistics on the device (vsx_fastq_eestats, vsearch_amd.eestats) against the library's host restatement
(VSX_EESTATS=host) field for field with sum_ee compared by bit pattern, against the recorded texts of the reference CLI
(tests/golden/fastq_eestats_golden.json, see tests/test_eestats_host.py for how it was recorded), and once against the live
reference binary build() leaves in oracle/_ref (skipped only where that binary is absent).

No call has more than 2 000 reads and no read more than 300 positions.
"""
import contextlib
import os

import numpy as np
import pytest

from tests import eestats_data as ed

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
needs_cli = pytest.mark.skipif(not os.path.exists(ed.ref_binary()), reason="oracle/_ref/vsearch_ref not built")


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


@pytest.fixture(scope="module")
def golden():
    return ed.load_golden(os.path.join(HERE, "golden", "fastq_eestats_golden.json"))


@contextlib.contextmanager
def host_path():
    old = os.environ.get("VSX_EESTATS")
    os.environ["VSX_EESTATS"] = "host"
    try:
        yield
    finally:
        if old is None:
            del os.environ["VSX_EESTATS"]
        else:
            os.environ["VSX_EESTATS"] = old


def on_device(aligner, s, **extra):
    res = ed.call(aligner, s, **extra)
    assert res.stats["reads_host"] == 0 and res.stats["reads"] == len(s["quals"])
    assert res.stats["windows"] >= 1 or res.symbols == 0
    return res


def on_host(s, **extra):
    with host_path():
        res = ed.call(None, s, **extra)
    assert res.stats["reads_host"] == res.stats["reads"]
    return res


def all_sets():
    return ed.golden_sets() + ed.rounding_reads()


def test_golden_on_device(aligner, golden):
    for d in golden["sets"] + golden["rounding"]:
        s = d["input"]
        res = on_device(aligner, s)
        for command in s["commands"]:
            mine = res.eestats_lines() if command == "eestats" else res.eestats2_lines()
            assert mine == d["expected"][command], (s["name"], command)


@pytest.mark.parametrize("window", [0, 1, 7])
def test_every_set_equals_host(aligner, window):
    for s in all_sets():
        ed.assert_same_tables(on_device(aligner, s, window=window), on_host(s), f"{s['name']} window {window}")


def test_window_counts(aligner):
    s = ed.generate(77, 100, read_len=90)
    assert on_device(aligner, s).stats["windows"] == 1
    assert on_device(aligner, s, window=1).stats["windows"] == 100 and on_device(aligner, s, window=7).stats["windows"] == 15


def test_scattered_offsets(aligner):
    """shuffled, non-monotonic offsets with shared bytes and out-of-range junk between the reads"""
    for s in (ed.generate(77, 100, read_len=90), [x for x in ed.edge_reads() if x["name"] == "tiles"][0]):
        base = on_host(s)
        for window in (0, 7):
            res = ed.scattered_call(aligner, s, seed=5, window=window)
            assert res.stats["reads_host"] == 0
            ed.assert_same_tables(res, base, f"{s['name']} scattered, window {window}")


@pytest.mark.parametrize("seed", [31, 32])
def test_generated_reads_equal_host(aligner, seed):
    """reads up to 300 positions, several workgroups of the walk, several steps of the ordered sum, windows that split both"""
    opts = {"length_cutoffs": [1, None, 1], "ee_cutoffs": ed.UNSORTED_CUTOFFS} if seed % 2 else {"length_cutoffs": [33, 290, 17]}
    s = ed.generate(seed, 1500, read_len=300, opts=opts)
    base = on_host(s)
    for window in (0, 700):
        ed.assert_same_tables(on_device(aligner, s, window=window), base, f"{s['name']} window {window}")
    for want in ("eestats", "eestats2"):
        ed.assert_same_tables(on_device(aligner, s, want=want), on_host(s, want=want), f"{s['name']} {want}")


def test_read_order_shows_and_is_kept(aligner):
    """sum_ee of the reversed input differs in bits from the forward one, and the device matches the host on both"""
    s = ed.generate(78, 2000, read_len=80)
    r = dict(s, quals=s["quals"][::-1])
    forward, backward = on_device(aligner, s), on_device(aligner, r, window=300)
    assert (forward.sum_ee.view(np.uint64) != backward.sum_ee.view(np.uint64)).any()
    ed.assert_same_tables(forward, on_host(s), "forward")
    ed.assert_same_tables(backward, on_host(r), "backward")


def test_histogram_budget_routes_the_whole_call_to_the_host(aligner):
    s = ed.generate(79, 50, read_len=100)
    # row i has 1000 * (i + 1) + 1 counters of 4 bytes: 100 rows are 20 200 400 bytes
    need = 4 * sum(1000 * (i + 1) + 1 for i in range(100))
    over = ed.call(aligner, s, hist_budget=need - 1)
    assert over.stats["reads_host"] == 50 and over.stats["windows"] == 0
    within = ed.call(aligner, s, hist_budget=need)
    assert within.stats["reads_host"] == 0 and within.stats["windows"] == 1
    ed.assert_same_tables(over, within)
    # eestats2 alone needs no histogram
    alone = ed.call(aligner, s, hist_budget=1, want="eestats2")
    assert alone.stats["reads_host"] == 0 and alone.cutoff_counts.tolist() == within.cutoff_counts.tolist()


def test_quality_cases_on_device(aligner, golden):
    from vsearch_amd import VsxError
    for d in golden["quality"]:
        s, fatal = d["input"], d["fatal"]
        for extra in ({}, {"window": 7}, {"want": "eestats2", "window": 1}):
            with pytest.raises(VsxError, match=rf"FASTQ quality value \({fatal[1]}\) {fatal[0]} \({fatal[2]}\)") as ei:
                ed.call(aligner, s, **extra)
            assert ei.value.code == -1, s["name"]


@needs_cli
@pytest.mark.parametrize("opts", [{}, {"qmax": 45, "length_cutoffs": [25, 240, 15], "ee_cutoffs": [4.0, 0.25, 1.5, 0.01]}],
                         ids=["default", "non-default"])
def test_live_reference_on_device(aligner, opts):
    s = ed.generate(2024, 2000, read_len=250, opts=opts)
    ref = ed.run_reference(s)
    assert ref["returncode"] == 0, ref["stderr"]
    res = on_device(aligner, s)
    assert res.eestats_lines() == ref["eestats"]
    assert res.eestats2_lines() == ref["eestats2"]
