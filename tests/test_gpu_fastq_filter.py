"""Read filtering on the device (vsx_fastx_filter, vsearch_amd.filter) against the recorded answers of the reference CLI
(tests/golden/fastq_filter_golden.json, see tests/test_fastq_filter_host.py for how it was recorded), against the library's
host restatement (VSX_FILTER=host) field for field with doubles compared by bit pattern, and once against the live reference
binary build() leaves in oracle/_ref (skipped only where that binary is absent).
"""
import contextlib
import os

import numpy as np
import pytest

from tests import fastq_filter_data as fd

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("kept", "discarded", "kept_rev", "discarded_rev", "counts")
needs_cli = pytest.mark.skipif(not os.path.exists(fd.ref_binary()), reason="oracle/_ref/vsearch_ref not built")


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


@pytest.fixture(scope="module")
def golden():
    return fd.load_golden(os.path.join(HERE, "golden", "fastq_filter_golden.json"))


@contextlib.contextmanager
def host_path():
    old = os.environ.get("VSX_FILTER")
    os.environ["VSX_FILTER"] = "host"
    try:
        yield
    finally:
        if old is None:
            del os.environ["VSX_FILTER"]
        else:
            os.environ["VSX_FILTER"] = old


def run(aligner, s, **extra):
    from vsearch_amd.filter import filter_reads
    a, k = fd.call_args(s)
    return filter_reads(aligner, *a, **dict(k, **extra))


def on_device(aligner, s, **extra):
    res = run(aligner, s, **extra)
    assert res.stats["reads_host"] == 0 and res.stats["windows"] >= 1
    return res


def on_host(s):
    with host_path():
        res = run(None, s)
    assert res.stats["reads_host"] == res.stats["reads"]
    return res


def assert_same_records(a, b, name=""):
    """field for field, doubles by bit pattern"""
    for x, y in ((a.records, b.records), (a.rev_records, b.rev_records)):
        assert (x is None) == (y is None)
        if x is None:
            continue
        assert x.dtype == y.dtype and len(x) == len(y)
        for field in ("start", "length", "ee", "discarded", "truncated"):
            u, v = x[field], y[field]
            if u.dtype.kind == "f":
                u, v = u.view(np.uint64), v.view(np.uint64)
            bad = np.flatnonzero(u != v)
            assert bad.size == 0, f"{name} {field}: {bad.size} reads differ, first {bad[:5]}: {x[bad[:3]]} != {y[bad[:3]]}"
    assert a.pair_discarded.tolist() == b.pair_discarded.tolist() and a.counts() == b.counts()


def test_golden_on_device(aligner, golden):
    for d in golden["sets"] + golden["rounding"]:
        s = d["input"]
        res = on_device(aligner, s)
        mine = fd.library_lines(res, s)
        for key in KEYS:
            assert mine[key] == d["expected"][key], (s["name"], key)


def test_edge_and_rounding_reads_equal_host(aligner):
    for s in fd.edge_reads() + fd.rounding_reads():
        assert_same_records(on_device(aligner, s), on_host(s), s["name"])


@pytest.mark.parametrize("seed", [31, 32])
def test_generated_reads_equal_host(aligner, seed):
    """two seeds, eight drawn option sets each, single and paired, reads up to 300"""
    for j in range(8):
        s = fd.generate(seed * 100 + j, 150, read_len=(70, 200, 300)[j % 3], paired=j % 2 == 1)
        assert_same_records(on_device(aligner, s), on_host(s), f"{s['name']} {s['opts']}")


def test_quality_cases_on_device(aligner, golden):
    from vsearch_amd import VsxError
    for d in golden["quality"]:
        s, fatal = d["input"], d["fatal"]
        if fatal is None:
            mine = fd.library_lines(on_device(aligner, s), s)
            for key in KEYS:
                assert mine[key] == d["expected"][key], (s["name"], key)
        else:
            with pytest.raises(VsxError, match=rf"FASTQ quality value \({fatal[1]}\) {fatal[0]} \({fatal[2]}\)") as ei:
                run(aligner, s)
            assert ei.value.code == -1, s["name"]


def test_first_quality_failure_across_windows(aligner):
    """the first bad value in the reference's order is the one named, whichever window meets it"""
    from vsearch_amd import VsxError
    rng = np.random.default_rng(41)
    n, good = 30, "I" * 80
    quals, rquals = [good] * n, [good] * n
    rquals[17] = fd._put(good, 3, "K")                    # Q42: read 17 reverse comes before read 18 forward
    quals[18], quals[29] = fd._put(good, 0, "L"), fd._put(good, 79, "L")
    s = fd._set("order", {}, [(f"r{k}", fd._seq(rng, 80), quals[k]) for k in range(n)],
                rev_seqs=[fd._seq(rng, 80) for _ in range(n)], rev_quals=rquals)
    for window in (0, 1, 7):
        with pytest.raises(VsxError, match=r"FASTQ quality value \(42\) above qmax \(41\)"):
            run(aligner, s, window=window)


def test_paired_input(aligner):
    s = [x for x in fd.edge_reads() if x["name"] == "pairs"][0]
    res = on_device(aligner, s)
    assert res.stats["reads"] == 2 * len(s["seqs"])
    assert res.pair_discarded.tolist() == [0, 1, 1, 1, 0, 0, 1]
    assert res.records["discarded"].tolist() == [0, 1, 0, 1, 0, 0, 0] and res.rev_records["discarded"].tolist() == [0, 0, 1, 1, 0, 0, 1]
    assert res.counts() == {"kept": 3, "truncated": 2, "discarded": 4}
    assert_same_records(res, on_host(s))


def test_fasta_input(aligner, golden):
    d = golden["sets"][-1]
    s = d["input"]
    assert s["quals"] is None
    res = on_device(aligner, s)
    assert (res.records["ee"] == -1.0).all()
    assert res.fasta_lines(s["labels"], "kept") == d["expected"]["kept"]
    assert res.fasta_lines(s["labels"], "discarded") == d["expected"]["discarded"]
    assert_same_records(res, on_host(s))


def test_windows_and_scattered_offsets(aligner):
    s = fd.generate(77, 100, read_len=90, paired=True)
    base = on_device(aligner, s)
    assert base.stats["windows"] == 1
    assert_same_records(base, on_host(s))
    for window, windows in ((1, 100), (7, 15)):
        res = on_device(aligner, s, window=window)
        assert res.stats["windows"] == windows
        assert_same_records(res, base, f"window {window}")
    for window in (0, 7):
        recs, rrecs, verdict, counts = fd.scattered_call(aligner, s, seed=5, window=window)
        assert recs.tobytes() == base.records.tobytes() and rrecs.tobytes() == base.rev_records.tobytes()
        assert verdict.tolist() == base.pair_discarded.tolist() and counts == base.counts()


@needs_cli
def test_live_reference_on_device(aligner):
    s = fd.generate(2024, 2000, read_len=250, opts={"maxee": 1.0, "truncqual": 7, "trunclen": 180, "maxns": 0})
    ref = fd.run_reference(s)
    assert ref["returncode"] == 0, ref["stderr"]
    assert min(ref["counts"]["kept"], ref["counts"]["discarded"], ref["counts"]["truncated"]) > 100
    mine = fd.library_lines(on_device(aligner, s), s)
    for key in KEYS:
        assert mine[key] == ref[key], key
