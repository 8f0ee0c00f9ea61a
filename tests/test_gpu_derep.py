"""Dereplication on the device (vsx_derep, vsearch_amd.derep) against the library's host restatement field for field -- cluster
order, members, strands, sizes, merged qualities -- over the recorded sets (tests/golden/derep_golden.json) and over the sizes
at which the kernels change path: the chunk and pass sizes of the reused hash and compare loops, cluster sizes around a
wavefront, quality blocks around 64 positions, table-size steps, staging windows.  Once against the live reference binary
build() leaves in oracle/_ref (skipped only where that binary is absent).
"""
import os
import random

import numpy as np
import pytest

from tests import derep_data as dd

pytestmark = pytest.mark.gpu

needs_cli = pytest.mark.skipif(not os.path.exists(dd.ref_binary()), reason="oracle/_ref/vsearch_ref not built")

_HOST = {}


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


@pytest.fixture(scope="module")
def golden():
    return dd.load_golden()


def on_host(s):
    """the host restatement's answer, computed once per set"""
    if s["name"] not in _HOST:
        res = dd.call(None, s)
        assert res.stats["reads_host"] == res.counts["kept"]
        _HOST[s["name"]] = (dd.result_fields(res), dd.formatted(res, s))
    return _HOST[s["name"]]


def on_device(aligner, s, **extra):
    res = dd.call(aligner, s, **extra)
    assert res.stats["reads_host"] == 0
    if res.counts["kept"]:
        assert res.stats["windows"] >= 1 and res.stats["slots_visited"] >= res.counts["kept"]
    return res


def assert_device_is_host(aligner, s, **extra):
    res = on_device(aligner, s, **extra)
    fields, text = on_host(s)
    got = dd.result_fields(res)
    assert got["counts"] == fields["counts"], s["name"]
    assert len(got["clusters"]) == len(fields["clusters"]), s["name"]
    for c, (a, b) in enumerate(zip(got["clusters"], fields["clusters"])):
        assert a == b, (s["name"], c)
    assert dd.formatted(res, s) == text, s["name"]
    return res


def test_golden_sets(aligner, golden):
    for s in golden:
        res = assert_device_is_host(aligner, s)
        text = dd.formatted(res, s)
        for key in text:
            assert text[key] == s["ref"][key], (s["name"], key)


def test_lengths(aligner):
    """0, 1, the chunk (16) and pair (32) sizes, the hash pass (1 024) and compare pass (2 048), 20 000: duplicates, reverse
    complements and pairs that differ only in the last symbol"""
    s = dd.lengths_set()
    res = assert_device_is_host(aligner, s)
    # per length: {s, rc(s)} and {other}; the two empty reads form one cluster
    assert len(res) == 2 * (len(dd.LENGTHS_DEVICE) - 1) + 1


def test_cluster_sizes(aligner):
    """clusters of 1, 2, 63, 64, 65 and 1 000 members, both strands, abundances, merged qualities"""
    res = assert_device_is_host(aligner, dd.cluster_sizes_set())
    assert sorted(int(c) for c in res.count) == [1, 2, 63, 64, 65, 1000]


@pytest.mark.parametrize("qout_max", [0, 1])
def test_quality_blocks(aligner, qout_max):
    """strings of 63, 64, 65 and 129 positions, every quality symbol 33 .. 126"""
    assert_device_is_host(aligner, dd.quality_blocks_set(qout_max))


def test_three_hash_bits(aligner, monkeypatch):
    """VSX_DEREP_HASH_BITS=3: eight hash values for everything, so the comparison of the code words alone decides"""
    monkeypatch.setenv("VSX_DEREP_HASH_BITS", "3")
    for s in (dd.lengths_set(), dd.cluster_sizes_set(), dd.derep_id_set()[0], dd.table_step_set(86)):
        res = assert_device_is_host(aligner, s)
        assert res.stats["candidates_compared"] >= res.counts["kept"] - len(res)


@pytest.mark.parametrize("n", [1, 2, 42, 43, 85, 86])
def test_table_steps(aligner, n):
    """the table doubles where 3 n exceeds twice its size: 42 | 43 reads (64 | 128 slots), 85 | 86 (128 | 256)"""
    assert_device_is_host(aligner, dd.table_step_set(n))


@pytest.mark.parametrize("window", [1, 7])
def test_windows(aligner, window):
    s = dd.lengths_set()
    res = assert_device_is_host(aligner, s, window=window)
    assert res.stats["windows"] == -(-res.counts["kept"] // window)
    assert_device_is_host(aligner, dd.fastq_sets()[1], window=window)


def test_scattered_offsets(aligner, monkeypatch):
    """the reads laid out in the blob in another order, with gaps between them"""
    from vsearch_amd import derep

    def scattered(items):
        bs = [x.encode() if isinstance(x, str) else bytes(x) for x in items]
        rng = random.Random(89)
        order = list(range(len(bs)))
        rng.shuffle(order)
        off = np.zeros(len(bs), np.uint64)
        parts, at = [], 0
        for k in order:
            gap = rng.randint(0, 37)
            parts.append(b"#" * gap)
            off[k] = at + gap
            parts.append(bs[k])
            at += gap + len(bs[k])
        return b"".join(parts) + b"#" * 5, off, np.array([len(b) for b in bs], np.uint32)

    monkeypatch.setattr(derep, "_blob", scattered)
    for s in (dd.lengths_set(), dd.cluster_sizes_set()):
        assert_device_is_host(aligner, s)


def test_reversed_input(aligner):
    """the representatives change with the order of the input; the host restatement follows"""
    for s in (dd.cluster_sizes_set(), dd.rc_first_set()[0]):
        r = dd.reversed_set(s)
        res = assert_device_is_host(aligner, r)
        assert dd.result_fields(res) == dd.py_derep(r)


def test_two_runs_are_identical(aligner):
    s = dd.cluster_sizes_set()
    a, b = on_device(aligner, s), on_device(aligner, s)
    assert dd.result_fields(a) == dd.result_fields(b) and dd.formatted(a, s) == dd.formatted(b, s)
    for x, y in ((a.rep, b.rep), (a.size, b.size), (a.count, b.count), (a.member_start, b.member_start), (a.member, b.member), (a.strand, b.strand)):
        assert x.tobytes() == y.tobytes()


def test_the_wrap_is_refused(aligner):
    from vsearch_amd import VsxError
    from vsearch_amd.derep import dereplicate
    with pytest.raises(VsxError) as e:
        dereplicate(aligner, ["ACGT", "ACGT"], ["a", "b"], sizes=[4294967295, 2], minseqlength=1)
    assert e.value.code == -1 and "2^32" in str(e.value)
    res = dereplicate(aligner, ["ACGT", "ACGT"], ["a", "b"], sizes=[4294967294, 1], minseqlength=1)
    assert int(res.size[0]) == 4294967295 and res.stats["reads_host"] == 0


@needs_cli
@pytest.mark.parametrize("which", ["fasta", "fastq_avg", "fastq_max"])
def test_random_reads_against_the_live_cli(aligner, which):
    """2 000 reads, 60 % duplicates, 30 % of those reverse-complemented, abundances 1 .. 50"""
    s = dd.random_set() if which == "fasta" else dd.random_set(fastq=True, qout_max=int(which == "fastq_max"))
    res = assert_device_is_host(aligner, s)
    ref, text = dd.run_reference(s), dd.formatted(res, s)
    assert set(ref) == set(text)
    for key in text:
        assert text[key] == ref[key], (which, key)
