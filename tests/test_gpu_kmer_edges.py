"""-m gpu: the k-mer candidate stage (vsearch_amd/csrc/vsx_kmer.hip) on the inputs of tests/kmer_edge_data.py -- counters at the
full byte and on either side of the 255 / 256 class switch, thresholds around 128 and 255 with mm - 1 beside mm in one counter dword,
the selection kernel's clamped bin and ties, buckets of one unit to 34 trips, the gaps, hops and unit edges of the packed index as
the device builds it, tag collisions of the long-word index.  Each case is a three-way equality: the device's candidate lists, the
library's host restatement and the plain-Python py_candidates(); index_postings pins the device build's posting count.
tests/test_kmer_edges_host.py asserts, without a device, that the inputs reach the edges they are named after.

At word length 15 the library's host restatement needs a table of 4^15 entries (17 GB with its scratch copy), so that case compares
the device with py_candidates() alone.

Two cases go through the reference CLI: --usearch_global --minwordmatches 129 on a primer set (the order of the candidates shows in
the hits), and --cluster_fast on the same sequences, whose subset indexes (16-bit postings, eight per unit, a tail loop above 64
units) exist in clustering only."""
import os

import pytest

from tests import kmer_edge_data as ked
from tests.test_gpu_search import FIELDS, REF_BIN, _first_diff, run_reference, run_reference_cluster

pytestmark = pytest.mark.gpu


def three_way(db, queries, opts, expect, monkeypatch, host=True):
    """device == host restatement == py_candidates for every query, under every environment the edges name; on a difference the
    first differing query and the edge it stands for"""
    from vsearch_amd import Aligner, SearchSession
    want = ked.expected(db, queries, opts)
    edge_of = {}
    for e in expect:
        edge_of.setdefault(e["query"], e["edge"])
    envs = []
    for e in expect:
        if e.get("env", {}) not in envs:
            envs.append(e.get("env", {}))
    with Aligner() as al:
        ss = SearchSession(al, db, id=0.5, **opts)
        runs = [("host", ss.candidates_batch(queries, device=False))] if host else []
        for env in envs:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            runs.append((f"device {env}" if env else "device", ss.candidates_batch(queries, device=True)))
            for k in env:
                monkeypatch.delenv(k)
        postings = ss.kmer_stats["index_postings"]
    for name, got in runs:
        assert len(got) == len(want)
        for k, (g, x) in enumerate(zip(got, want)):
            if g != x:
                d = next((i for i, (a, b) in enumerate(zip(g, x)) if a != b), min(len(g), len(x)))
                pytest.fail(f"{name}: query {k} ({edge_of.get(k, 'no named edge')}): {len(g)} candidates, restatement {len(x)}; "
                            f"first difference at {d}: {g[d:d + 3]} != {x[d:d + 3]}")
    assert postings == ked.posting_count(db, opts["wordlength"])


def test_class_switch(gpu_required, monkeypatch):
    three_way(*ked.class_switch(), monkeypatch)


@pytest.mark.parametrize("mm", ked.MM_ALL)
@pytest.mark.parametrize("w", [8, 12])
def test_threshold_edges(gpu_required, monkeypatch, w, mm):
    db, queries, opts, expect = ked.threshold_edges(w)
    mine = [e for e in expect if e["minwordmatches"] == mm]
    assert mine
    three_way(db, queries, dict(opts, minwordmatches=mm), mine, monkeypatch)


def test_selection_edges(gpu_required, monkeypatch):
    three_way(*ked.selection_edges(), monkeypatch)


def test_bucket_trips(gpu_required, monkeypatch):
    three_way(*ked.bucket_trips(), monkeypatch)


def test_primer_buckets(gpu_required, monkeypatch):
    three_way(*ked.primer_set(), monkeypatch)


def test_gap_edges(gpu_required, monkeypatch):
    three_way(*ked.gap_edges(), monkeypatch)


@pytest.mark.parametrize("w", [9, 12, 15])
def test_tag_collisions(gpu_required, monkeypatch, w):
    three_way(*ked.tag_collisions(w), monkeypatch, host=w < 15)


# ---- against the reference CLI ---------------------------------------------------------------------------------------------------
def cli_slice():
    """3 000 primer sequences with bodies of 150, so that a query has 163 words and --minwordmatches 129 is a real threshold"""
    return ked.primer_set(seed=407, n_seq=3000, body=150, per_family=20, rate=0.012, minwordmatches=129, n_queries=40)


def test_usearch_global_minwordmatches_129_matches_reference_cli(gpu_required, tmp_path):
    if not os.path.exists(REF_BIN):
        pytest.fail("oracle/_ref/vsearch_ref missing")
    from vsearch_amd import Aligner, SearchSession
    db, queries, opts, _ = cli_slice()
    assert all(len(ked.words_of(q, 8)) >= 129 for q in queries)
    exp = run_reference(str(tmp_path), db, queries, ["--id", "0.8", "--minwordmatches", "129", "--maxaccepts", "2", "--maxrejects", "4"])
    with Aligner() as al:
        ss = SearchSession(al, db, id=0.8, minwordmatches=129, maxaccepts=2, maxrejects=4)
        got = ss.userout(queries, fields=FIELDS)
        cands = ss.candidates_batch(queries, device=True)
    assert len(exp) > 40
    assert got == exp, _first_diff(got, exp)
    # the restatement's order is the order the hits come out in
    assert cands == ked.expected(db, queries, dict(wordlength=8, minwordmatches=129, maxaccepts=2, maxrejects=4))


def test_cluster_fast_primer_slice_matches_reference_cli(gpu_required, tmp_path):
    if not os.path.exists(REF_BIN):
        pytest.fail("oracle/_ref/vsearch_ref missing")
    from vsearch_amd import Aligner, SearchSession
    seqs = cli_slice()[0]
    names = [f"s{i:04d}" for i in range(len(seqs))]
    assert len(set(map(len, seqs))) == 1                                   # sorted by length already: the labels order them
    exp = run_reference_cluster(str(tmp_path), seqs, names, ["--id", "0.97"])
    assert sum(1 for l in exp if l[0] == "H") > 1000
    for round_size in (32, 1000):
        with Aligner() as al:
            ss = SearchSession(al, seqs, id=0.97, maxrejects=8)
            got = ss.uc_lines(names, round=round_size)
        assert got == exp, (round_size, _first_diff(got, exp))
