"""Paired-end merging on the device (vsx_merge_pairs, vsearch_amd.merge) against the reference CLI's --fastq_mergepairs.

Every comparison is exact: the merged FASTQ with --fastq_eeout, the --eetabbedout lines, the labels of the pairs that did
not merge and the counts of the log's statistics block, over ALL pairs of the input.  The live comparisons run the
reference binary build() leaves in oracle/_ref (--threads 1 keeps its output in input order) and are skipped only where
that binary is absent.

Reason classes.  At the reference's default options only these verdicts can occur: ok, nokmers, repeat, maxdiffs,
minscore, minovlen, staggered (maxlen / maxns / maxee / min- and maxmergelen are unbounded by default, minlen 1 needs an
empty read, and a difference percentage above 100 does not exist).  The default-option test asserts each of those on the
REFERENCE's counts; the drawn option sets assert the remaining ones the same way.
"""
import contextlib
import json
import os

import numpy as np
import pytest

from tests import merge_data as md

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
needs_cli = pytest.mark.skipif(not os.path.exists(md.ref_binary()), reason="oracle/_ref/vsearch_ref not built")

MAX_LEN = 512          # VSX_MERGE_MAX_LEN (include/vsx_merge.h)


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


@contextlib.contextmanager
def host_path():
    old = os.environ.get("VSX_MERGE")
    os.environ["VSX_MERGE"] = "host"
    try:
        yield
    finally:
        if old is None:
            del os.environ["VSX_MERGE"]
        else:
            os.environ["VSX_MERGE"] = old


def assert_matches(res, labels, ref):
    from vsearch_amd.merge import MERGE_REASONS
    assert len(res) == len(labels)
    mine = res.fastq_lines(labels, eeout=True)
    assert len(mine) == len(ref["fastq"]), (len(mine) // 4, len(ref["fastq"]) // 4)
    for i, (a, b) in enumerate(zip(mine, ref["fastq"])):
        assert a == b, f"merged FASTQ line {i}: {a[:100]!r} != {b[:100]!r}"
    assert res.eetabbed_lines() == ref["eetabbed"]
    assert [labels[k] for k in res.not_merged_indices()] == ref["notmerged"]
    assert res.reason_counts() == ref["reasons"]
    assert set(res.reason_counts()) <= set(MERGE_REASONS)


def assert_same_records(a, b):
    """field for field, doubles by bit pattern"""
    assert a.records.dtype == b.records.dtype and len(a) == len(b)
    for name in a.records.dtype.names:
        x, y = a.records[name], b.records[name]
        if x.dtype.kind == "f":
            x, y = x.view(np.uint64), y.view(np.uint64)
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, f"{name}: {bad.size} pairs differ, first {bad[:5]}"
    assert a.seq_blob == b.seq_blob and a.qual_blob == b.qual_blob


def test_golden_on_device(aligner):
    """tests/golden/merge_golden.json (see tests/test_merge_host.py for how it was recorded), through the kernel"""
    from vsearch_amd.merge import merge_pairs, last_stats
    doc = md.load_golden(os.path.join(HERE, "golden", "merge_golden.json"))
    i = doc["inputs"]
    for case in doc["cases"]:
        res = merge_pairs(aligner, i["fwd"], i["fqual"], i["rev"], i["rqual"], **case["opts"])
        assert_matches(res, i["labels"], case)
        assert last_stats()["pairs_host"] == 0
    e = doc["example"]
    i = e["inputs"]
    res = merge_pairs(aligner, i["fwd"], i["fqual"], i["rev"], i["rqual"])
    assert_matches(res, i["labels"], e)
    fasta = e["expected_fasta"].split("\n", 1)[1].replace("\n", "")
    assert res.sequence(0) == fasta


@needs_cli
def test_live_default_options(aligner):
    from vsearch_amd.merge import merge_pairs, last_stats
    data = md.generate(20261, 20000)
    ref = md.run_reference(*data)
    assert ref["returncode"] == 0, ref["stderr"]
    for reason in ("nokmers", "repeat", "maxdiffs", "minscore", "minovlen", "staggered"):
        assert ref["reasons"].get(reason, 0) > 0, f"the input has no pair the reference rejects as {reason}: {ref['reasons']}"
    assert len(ref["eetabbed"]) > 0
    res = merge_pairs(aligner, *data[1:])
    assert_matches(res, data[0], ref)
    st = last_stats()
    assert st["pairs"] == 20000 and st["pairs_host"] == 0 and st["diagonals_scored"] > 0


@needs_cli
@pytest.mark.parametrize("opts,expect", [
    (dict(minovlen=5, maxdiffs=4, truncqual=7, maxns=1, maxee=1.0, minmergelen=200, maxmergelen=420, qmaxout=50,
          allowmergestagger=True), ("maxns", "maxee", "minmergelen", "maxmergelen", "maxdiffs")),
    (dict(minovlen=6, maxdiffpct=4.0, truncqual=12, maxns=0, maxee=2.0, minlen=100, qmaxout=35), ("minlen", "maxdiffpct", "maxns")),
    (dict(minovlen=7, maxdiffs=30, maxlen=249, qmaxout=45, qminout=3), ("maxlen",)),
    (dict(minovlen=8, maxdiffs=2, maxdiffpct=1.5, truncqual=3, maxee=0.25, qmaxout=60, allowmergestagger=True), ("maxee", "maxdiffs")),
])
def test_live_drawn_options(aligner, opts, expect):
    from vsearch_amd.merge import merge_pairs
    data = md.generate(20262, 20000)
    ref = md.run_reference(*data, **opts)
    assert ref["returncode"] == 0, ref["stderr"]
    for reason in expect:
        assert ref["reasons"].get(reason, 0) > 0, f"no pair the reference rejects as {reason}: {ref['reasons']}"
    res = merge_pairs(aligner, *data[1:], **opts)
    assert_matches(res, data[0], ref)


def test_kernel_equals_host_path(aligner):
    from vsearch_amd.merge import merge_pairs
    g, e = md.generate(20263, 6000), md.edge_pairs()
    data = [a + b for a, b in zip(g, e)]
    # letters that are no nucleotide code (the reference's FASTQ reader refuses them; the merge core reads them as unknown)
    data[0].append("letters"); data[1].append("ACGTTGCATT" * 5 + "EFIJLOPQXZ" + "GATTACAGGC" * 5)
    data[2].append("I" * 110); data[3].append("GCCTGTAATC" * 5 + "ACGTAC" + "AATGCAACGT" * 5); data[4].append("I" * 106)
    for opts in ({}, dict(minovlen=5, truncqual=9, maxns=2, maxee=1.5, qmaxout=55, allowmergestagger=True, minmergelen=150)):
        dev = merge_pairs(aligner, *data[1:], **opts)
        with host_path():
            host = merge_pairs(None, *data[1:], **opts)
        assert host.stats["pairs_host"] == len(data[0]) and dev.stats["pairs_host"] == 0
        assert_same_records(dev, host)


def test_window_size_does_not_change_results(aligner):
    from vsearch_amd.merge import merge_pairs
    data = md.generate(20264, 5000)
    base = merge_pairs(aligner, *data[1:])
    assert base.stats["windows"] == 1
    for window in (1, 7, 1000, 4999):
        n = 300 if window == 1 else 5000
        part = [d[:n] for d in data]
        res = merge_pairs(aligner, *part[1:], window=window)
        assert res.stats["windows"] == -(-n // window)
        if n == 5000:
            assert_same_records(res, base)
        else:
            assert_same_records(res, merge_pairs(aligner, *part[1:]))


@needs_cli
def test_long_reads_take_the_host_path(aligner):
    from vsearch_amd.merge import merge_pairs, last_stats
    short = md.generate(20265, 400)
    long_ = md.generate(20266, 40, read_len=MAX_LEN + 88)
    edge = md.generate(20267, 20, read_len=MAX_LEN)               # exactly at the limit: still the kernel's
    order = np.random.default_rng(5).permutation(460)
    data = [[(a + b + c)[k] for k in order] for a, b, c in zip(short, long_, edge)]
    data[0] = [f"p{k}" for k in range(460)]
    n_long = sum(1 for f, r in zip(data[1], data[3]) if len(f) > MAX_LEN or len(r) > MAX_LEN)
    assert n_long >= 30
    ref = md.run_reference(*data)
    assert ref["returncode"] == 0, ref["stderr"]
    res = merge_pairs(aligner, *data[1:], window=64)
    assert_matches(res, data[0], ref)
    assert last_stats()["pairs_host"] == n_long


@needs_cli
def test_edge_inputs(aligner):
    from vsearch_amd.merge import merge_pairs
    data = md.edge_pairs()
    for opts in ({}, dict(minovlen=5), dict(allowmergestagger=True, maxns=0)):
        ref = md.run_reference(*data, **opts)
        assert ref["returncode"] == 0, ref["stderr"]
        res = merge_pairs(aligner, *data[1:], **opts)
        assert_matches(res, data[0], ref)
    assert ref["reasons"].get("repeat", 0) > 0


def test_quality_out_of_range_on_device(aligner):
    from vsearch_amd import VsxError
    from vsearch_amd.merge import merge_pairs
    labels, fwd, fqual, rev, rqual = md.generate(20268, 200, read_len=100)
    bad = list(rqual)
    k = next(k for k in range(100, 200) if len(rqual[k]) == 100 and len(fqual[k]) == 100)
    bad[k] = bad[k][:40] + "K" + bad[k][41:]                      # Q42 > qmax 41
    with pytest.raises(VsxError, match=r"quality value \(42\) above qmax \(41\)") as ei:
        merge_pairs(aligner, fwd, fqual, rev, bad, window=64)
    assert ei.value.code == -1
    assert len(merge_pairs(aligner, fwd, fqual, rev, bad, qmax=42)) == 200
    # beyond the truncation point the reference never reads it
    bad[k] = bad[k][:20] + "#" + bad[k][21:]
    assert len(merge_pairs(aligner, fwd, fqual, rev, bad, truncqual=2)) == 200
