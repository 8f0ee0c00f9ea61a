"""Prefix dereplication on the device (vsx_derep_prefix, vsearch_amd.derep_prefix) against the library's host restatement on
every output array -- cluster order, sizes, counts, member lists, ranks -- over the recorded sets
(tests/golden/derep_prefix_golden.json) and over what changes the kernels' path: three hash bits, table-size steps, staging
windows, scattered offsets, reversed input.  Every route to the host with its counter, two calls byte for byte, and once
against the live reference binary build() leaves in oracle/_ref (skipped only where that binary is absent).
"""
import importlib
import os
import random

import numpy as np
import pytest

from tests import derep_prefix_data as pd

pytestmark = pytest.mark.gpu

needs_cli = pytest.mark.skipif(not os.path.exists(pd.ref_binary()), reason="oracle/_ref/vsearch_ref not built")

ARRAYS = ("rep", "size", "count", "member_start", "member", "rank")
ROUTES = ("host_no_context", "host_environment", "host_read_count", "host_memory")
_HOST = {}


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


@pytest.fixture(scope="module")
def golden():
    return pd.load_golden()


def on_host(s):
    """the host restatement's answer, computed once per set"""
    if s["name"] not in _HOST:
        res = pd.call(None, s)
        assert res.stats["reads_host"] == res.counts["kept"] and res.stats["host_no_context"] == 1
        _HOST[s["name"]] = (res, pd.formatted(res, s))
    return _HOST[s["name"]]


def on_device(aligner, s, **extra):
    res = pd.call(aligner, s, **extra)
    st = res.stats
    assert st["reads_host"] == 0 and sum(st[r] for r in ROUTES) == 0
    if res.counts["kept"]:
        assert st["windows"] >= 1 and 1 <= st["nodes"] <= res.counts["kept"] and st["distinct_lengths"] >= 1
    return res


def assert_device_is_host(aligner, s, **extra):
    res = on_device(aligner, s, **extra)
    ref, text = on_host(s)
    assert res.counts == ref.counts, s["name"]
    for name in ARRAYS:
        assert np.array_equal(getattr(res, name), getattr(ref, name)), (s["name"], name)
    assert res.stats["nodes"] == ref.stats["nodes"] and res.stats["distinct_lengths"] == ref.stats["distinct_lengths"]
    assert pd.formatted(res, s) == text, s["name"]
    return res


def test_golden_sets(aligner, golden):
    for s in golden:
        res = assert_device_is_host(aligner, s)
        text = pd.formatted(res, s)
        for key in text:
            assert text[key] == s["ref"][key], (s["name"], key)


def test_large_nested_set(aligner):
    """40 000 reads in 10 000 workgroups: a few thousand nodes, every one with thousands of duplicates and up to 13 prefixes"""
    res = assert_device_is_host(aligner, pd.large_nested_set())
    assert res.stats["nodes"] < 40000 and res.stats["probes"] > res.stats["nodes"]


def test_three_hash_bits(aligner, golden, monkeypatch):
    """VSX_DEREP_PREFIX_HASH_BITS=3: eight hash values for everything, so the comparison of the code words alone decides"""
    monkeypatch.setenv("VSX_DEREP_PREFIX_HASH_BITS", "3")
    by_name = {s["name"]: s for s in golden}
    for name in ("ladder", "boundary_lengths", "near_misses", "candidate_lengths", "alphabet", "one_symbol", "winners"):
        res = assert_device_is_host(aligner, by_name[name])
        assert res.stats["candidates_compared"] >= res.stats["nodes"] - len(res)      # at least the links that were made
    res = assert_device_is_host(aligner, pd.table_step_set(86))
    assert res.stats["candidates_compared"] > 0


@pytest.mark.parametrize("n", [1, 2, 42, 43, 85, 86])
def test_table_steps(aligner, n):
    """the table doubles where 3 n exceeds twice its size: 42 | 43 reads (64 | 128 slots), 85 | 86 (128 | 256)"""
    assert_device_is_host(aligner, pd.table_step_set(n))


@pytest.mark.parametrize("window", [1, 7])
def test_windows(aligner, golden, window):
    for s in golden:
        if s["name"] in ("boundary_lengths", "selection", "one_symbol"):
            res = assert_device_is_host(aligner, s, window=window)
            assert res.stats["windows"] == -(-res.counts["kept"] // window)


def test_scattered_offsets(aligner, golden, monkeypatch):
    """the reads laid out in the blob in another order, with gaps between them"""
    dp = importlib.import_module("vsearch_amd.derep_prefix")

    def scattered(items):
        bs = [x.encode() if isinstance(x, str) else bytes(x) for x in items]
        rng = random.Random(191)
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

    monkeypatch.setattr(dp, "_blob", scattered)
    for s in golden:
        if s["name"] in ("boundary_lengths", "candidate_lengths", "alphabet"):
            assert_device_is_host(aligner, s)


def test_reversed_input(aligner, golden):
    """ties of the sort and of the cluster order fall the other way; the host restatement and the loop follow"""
    for s in golden:
        if s["name"] in ("winners", "ladder", "cluster_order", "selection"):
            r = pd.reversed_set(s)
            res = assert_device_is_host(aligner, r)
            assert pd.result_fields(res) == pd.py_derep_prefix(r)


def test_two_runs_are_identical(aligner, golden):
    s = next(g for g in golden if g["name"] == "thousand_extenders")
    a, b = on_device(aligner, s), on_device(aligner, s)
    assert pd.formatted(a, s) == pd.formatted(b, s)
    for name in ARRAYS:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name


def test_host_routes_and_their_counters(aligner, golden, monkeypatch):
    s = next(g for g in golden if g["name"] == "selection")
    ref, _ = on_host(s)

    def routed(counter, **extra):
        res = pd.call(aligner, s, **extra)
        assert res.stats["reads_host"] == res.counts["kept"] and res.stats["windows"] == 0
        assert {r: res.stats[r] for r in ROUTES} == {r: int(r == counter) for r in ROUTES}
        for name in ARRAYS:
            assert np.array_equal(getattr(res, name), getattr(ref, name)), (counter, name)

    with monkeypatch.context() as m:
        m.setenv("VSX_DEREP_PREFIX", "host")
        routed("host_environment")
    with monkeypatch.context() as m:
        m.setenv("VSX_DEREP_PREFIX_DEVICE_READS", str(ref.counts["kept"] - 1))
        routed("host_read_count")
    with monkeypatch.context() as m:
        m.setenv("VSX_DEREP_PREFIX_DEVICE_READS", str(ref.counts["kept"]))
        on_device(aligner, s)                                                # at the limit the device still answers
    with monkeypatch.context() as m:
        m.setenv("VSX_DEREP_PREFIX_PRETEND_BYTES", str(1 << 50))
        routed("host_memory")
    on_device(aligner, s)


def test_the_wrap_is_refused(aligner):
    from vsearch_amd import VsxError, derep_prefix
    with pytest.raises(VsxError) as e:
        derep_prefix(aligner, ["ACGT", "ACG"], ["a", "b"], sizes=[4294967295, 1], sizein=1, minseqlength=1)
    assert e.value.code == -1 and "2^32" in str(e.value)
    res = derep_prefix(aligner, ["ACGT", "ACG"], ["a", "b"], sizes=[4294967294, 1], sizein=1, minseqlength=1)
    assert int(res.size[0]) == 4294967295 and res.stats["reads_host"] == 0 and [int(m) for m in res.members(0)] == [0, 1]


@needs_cli
def test_random_reads_against_the_live_cli(aligner):
    """2 000 reads, 60 % copies of earlier reads, two thirds of those cut at a random length, annotations 1 .. 50 summed"""
    s = pd.random_set()
    res = assert_device_is_host(aligner, s)
    assert len(res) < res.stats["nodes"] < res.counts["kept"]                # duplicates and absorbed prefixes both occur
    ref, text = pd.run_reference(s), pd.formatted(res, s)
    assert set(ref) == set(text)
    for key in text:
        assert text[key] == ref[key], key
