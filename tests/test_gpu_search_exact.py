"""Exact sequence search on the device (vsx_search_exact: hash, index build and probe kernels of vsx_exact.hip) against the library's
host restatement field for field, against the plain-Python restatement, and against the recorded lines of the reference CLI
(tests/golden/search_exact_golden.json); once against the live reference binary build() leaves in oracle/_ref.

Every device call must be answered by the kernels (queries_host == 0).  No call has more than 4 000 queries or 4 000 database
sequences.  The kernels' sizes whose edges the length set walks (vsx_exact_internal.h): 16 symbols per lane and 1 024 per wave pass
in the hash kernel, 32 per lane and 2 048 per wave pass in the compare loop; the table sets sit on the 2/3-fill edges of a
power-of-two table and on both sides of the probe's 64-slot round.
"""
import contextlib
import ctypes as C
import os
import random

import numpy as np
import pytest

from tests import search_exact_data as sd

pytestmark = pytest.mark.gpu

needs_cli = pytest.mark.skipif(not os.path.exists(sd.ref_binary()), reason="oracle/_ref/vsearch_ref not built")


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


@pytest.fixture(scope="module")
def golden():
    return sd.load_golden()


@contextlib.contextmanager
def environment(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


@contextlib.contextmanager
def session(aligner, s, **extra):
    from vsearch_amd import SearchSession
    kw = sd.session_opts(s["opts"])
    kw.update(extra)
    sess = SearchSession(aligner, s["db"], sizes=s["db_sizes"], labels=s["db_names"], **kw)
    try:
        yield sess
    finally:
        sess.close()


def on_device(sess, s, raw=False):
    call = sess.search_exact_raw if raw else sess.search_exact
    res = call(s["queries"], sizes=s["sizes"], labels=s["names"])
    st = sess.exact_stats
    assert st["queries_host"] == 0 and st["queries_device"] == len(s["queries"])
    return res


_HOST = {}


def on_host(s, raw=False):
    """the host restatement's answer, computed once per set"""
    key = (s["name"], raw)
    if key not in _HOST:
        from vsearch_amd.search import search_exact_host
        _HOST[key] = search_exact_host(s["db"], s["queries"], db_sizes=s["db_sizes"], db_labels=s["db_names"], sizes=s["sizes"],
                                       labels=s["names"], raw=raw, **sd.session_opts(s["opts"]))
    return _HOST[key]


def same_raw(a, b):
    return np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def device_equals_host(aligner, s, **extra):
    with session(aligner, s, **extra) as sess:
        hits = on_device(sess, s)
        stats = dict(sess.exact_stats)
    assert hits == on_host(s), s["name"]
    return hits, stats


# ---- the golden sets: the issue's example, alphabet, small lengths, filters, masking, the zero-length query ------------------------
def test_golden_sets(aligner, golden):
    for s in golden:
        hits, _ = device_equals_host(aligner, s)
        assert sd.userout_lines(s, hits) == s["ref"]["userout"], s["name"]
        assert sd.uc_lines(s, hits) == s["ref"]["uc"], s["name"]
        assert sd.uc_lines(s, hits, uc_allhits=True) == s["ref"]["uc_allhits"], s["name"]


def test_filters_and_selfid(aligner, golden):
    for s in [g for g in golden if g["name"].startswith("filter_")] + [sd.selfid_set()]:
        hits, _ = device_equals_host(aligner, s)
        sd.assert_hits_equal_py(hits, s)
    assert all(hs == [] for hs in device_equals_host(aligner, sd.selfid_set())[0])


def test_masking_combinations(aligner, golden):
    got = {}
    for s in [g for g in golden if g["name"].startswith("masking_")]:
        got[s["name"]] = [len(hs) for hs in device_equals_host(aligner, s)[0]]
    assert got["masking_dust_none_hard"] == [0, 1, 0]
    assert got["masking_dust_none"] == got["masking_dust_dust_hard"] == got["masking_none_none_hard"] == [1, 1, 1]


# ---- lengths and alphabet, with the full hash and with three bits of it ------------------------------------------------------------
@pytest.fixture(scope="module")
def lengths():
    return sd.lengths_set(sd.LENGTHS_DEVICE, name="lengths_device")


def check_lengths(s, hits):
    # every query: itself on the plus strand, its reverse complement on the minus strand, none of the near copies
    # (a query of one or two symbols also equals the shortened copy of the next length's query, wherever that happens)
    for q, hs in enumerate(hits):
        seq = s["queries"][q]
        want = sorted([(t, 0) for t, d in enumerate(s["db"]) if d == seq] + [(t, 1) for t, d in enumerate(s["db"]) if d == sd.revcomp(seq)])
        assert len(want) == 2 or len(seq) <= 2
        assert [(h["target"], h["strand"]) for h in hs] == want, len(seq)


def test_lengths(aligner, lengths):
    assert len(lengths["db"]) <= 4000
    hits, _ = device_equals_host(aligner, lengths)
    check_lengths(lengths, hits)
    sd.assert_hits_equal_py(hits, lengths)


def test_alphabet(aligner):
    s = sd.alphabet_set()
    hits, _ = device_equals_host(aligner, s)
    sd.assert_hits_equal_py(hits, s)


def collision_set():
    """1 500 database sequences of ONE length: with three hash bits an eighth of them share a query's hash and length"""
    rng = random.Random(37)
    db = sorted({sd.random_seq(rng, 50) for _ in range(1500)})
    rng.shuffle(db)
    qs = [db[k] for k in range(0, 200, 2)] + [sd.revcomp(db[k]) for k in range(1, 100, 2)] + [sd.substitute(db[k], 49) for k in range(50)]
    return sd._set("collisions", db, qs)


def test_collisions_three_hash_bits(aligner, lengths):
    """VSX_EXACT_HASH_BITS=3 (read when the index is built): almost every probe walks a chain of false candidates and the
    comparison alone decides.  The results are those of the 64-bit hash."""
    for s in (lengths, sd.alphabet_set(), collision_set()):
        with environment("VSX_EXACT_HASH_BITS", "3"):
            hits, stats = device_equals_host(aligner, s)
        sd.assert_hits_equal_py(hits, s)
        assert stats["candidates_compared"] > stats["hits"], s["name"]
        if s is lengths:
            check_lengths(lengths, hits)
        if s["name"] == "collisions":
            # 400 strands, each against about 1 500 / 8 candidates of its own length: far above the 150 hits
            assert stats["hits"] == 150 and stats["candidates_compared"] > 100 * stats["hits"]
            assert stats["slots_visited"] > stats["candidates_compared"]


# ---- the table -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 42, 43, 1365, 1366, 2730, 2731])
def test_table_sizes(aligner, n):
    """2/3-fill edges of a power-of-two table (3 -> 4 | 8 slots at 5 | 6, 2 048 | 4 096 at 1 365 | 1 366, 4 096 | 8 192 at 2 730 | 2 731)
    and of the 64-slot round (42 | 43 sequences: 64 | 128 slots)"""
    s = sd.table_set(n)
    hits, stats = device_equals_host(aligner, s)
    sd.assert_hits_equal_py(hits, s)
    assert stats["strands_probed"] == 2 * len(s["queries"]) and stats["windows"] == 1


def test_duplicates_and_palindromes(aligner):
    s = sd.duplicates_set(300)
    hits, stats = device_equals_host(aligner, s)
    sd.assert_hits_equal_py(hits, s)
    assert [len(hs) for hs in hits] == [300, 300, 600, 0]
    # the palindrome hits each of its targets on both strands, plus first
    assert [(h["target"], h["strand"]) for h in hits[2][:4]] == [(hits[2][0]["target"], 0), (hits[2][0]["target"], 1),
                                                                   (hits[2][2]["target"], 0), (hits[2][2]["target"], 1)]


def test_capacity_three_hundred_thousand_hits(aligner):
    """1 000 queries that each hit 300 targets: 300 000 hits in one window, more than the hit buffer's first size -- the probe
    reports the space it needs and is launched again"""
    rng = random.Random(41)
    seq = sd.random_seq(rng, 60)
    s = sd._set("capacity", [seq] * 300 + [sd.random_seq(rng, 60) for _ in range(20)], [seq] * 1000)
    with session(aligner, s) as sess:
        first, hits, cig = got = on_device(sess, s, raw=True)
        assert sess.exact_stats["hits"] == 300000 and sess.exact_stats["windows"] == 1
    assert np.array_equal(first, np.arange(1001, dtype=np.uint64) * 300)
    assert np.array_equal(hits["target"], np.tile(np.arange(300, dtype=np.uint32), 1000)) and not hits["strand"].any()
    assert same_raw(got, on_host(s, raw=True))


# ---- windows -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hundred():
    s = sd.seeded_set(43, 150, 99, name="hundred")
    s["queries"].insert(50, "")                   # a zero-length query in the middle of a window
    s["sizes"].insert(50, 1)
    s["names"].insert(50, "empty;size=1")
    return s


@pytest.mark.parametrize("window", [1, 7, 0])
def test_windows(aligner, hundred, window):
    hits, stats = device_equals_host(aligner, hundred, window=window)
    assert hits[50] == [] and stats["windows"] == (1 if window == 0 else -(-100 // window))
    sd.assert_hits_equal_py(hits, hundred)


def test_scattered_offsets(aligner, hundred):
    """the queries anywhere in the caller's blob: shuffled, unaligned, with other bytes between them"""
    from vsearch_amd import _lib
    from vsearch_amd.search import SearchSession, _meta
    rng = random.Random(47)
    qs = hundred["queries"]
    order = list(range(len(qs)))
    rng.shuffle(order)
    blob, off = bytearray(), np.zeros(len(qs), np.uint64)
    for k in order:
        blob += sd.random_seq(rng, rng.randint(0, 9)).encode()
        off[k] = len(blob)
        blob += qs[k].encode()
    blob = bytes(blob)
    lens = np.array([len(q) for q in qs], np.uint32)
    with session(aligner, hundred, window=7) as sess:
        res = _lib.Hits()
        m, keep = _meta(hundred["sizes"], hundred["names"], len(qs))
        _lib.check(_lib.load().vsx_search_exact(sess.h, len(qs), C.cast(C.c_char_p(blob), C.c_void_p), len(blob), off.ctypes.data_as(C.c_void_p),
                                                lens.ctypes.data_as(C.c_void_p), C.byref(m), C.byref(res)), "vsx_search_exact")
        assert same_raw(SearchSession._raw_hits(res), on_host(hundred, raw=True))


def test_zero_queries(aligner, hundred):
    with session(aligner, hundred) as sess:
        first, hits, cig = sess.search_exact_raw([])
        assert first.tolist() == [0] and len(hits) == 0 and sess.exact_stats["queries_host"] == 0


def test_plus_strand_only(aligner, hundred):
    s = dict(hundred, name="hundred_plus", opts=dict(hundred["opts"], strand_both=0))
    hits, stats = device_equals_host(aligner, s)
    assert stats["strands_probed"] == 100 and not any(h["strand"] for hs in hits for h in hs)
    sd.assert_hits_equal_py(hits, s)


# ---- repeatability ---------------------------------------------------------------------------------------------------------------------
def test_repeatable(aligner):
    """insertion order into the table varies; the returned bytes do not: two calls on one searcher and a second searcher"""
    s = sd.seeded_set(53, 3000, 2000, name="repeat")
    with session(aligner, s) as sess:
        a = on_device(sess, s, raw=True)
        assert sess.exact_stats["seconds_index"] > 0
        b = on_device(sess, s, raw=True)
        assert sess.exact_stats["seconds_index"] == 0          # the index is paid once per searcher
    with session(aligner, s) as sess:
        c = on_device(sess, s, raw=True)
    assert same_raw(a, b) and same_raw(a, c) and same_raw(a, on_host(s, raw=True))


def test_host_switch(aligner, hundred):
    """VSX_EXACT=host answers from the host restatement on the same searcher"""
    with session(aligner, hundred) as sess:
        with environment("VSX_EXACT", "host"):
            hits = sess.search_exact(hundred["queries"], sizes=hundred["sizes"], labels=hundred["names"])
            assert sess.exact_stats["queries_device"] == 0 and sess.exact_stats["queries_host"] == 100
        assert hits == on_device(sess, hundred) == on_host(hundred)


# ---- the live reference --------------------------------------------------------------------------------------------------------------
@needs_cli
def test_live_reference_cli(aligner):
    s = sd.seeded_set(59, 3000, 2000, name="live")
    ref = sd.run_reference(s, threads=1)
    hits, _ = device_equals_host(aligner, s)
    assert sd.userout_lines(s, hits) == ref["userout"]
    assert sd.uc_lines(s, hits) == ref["uc"]
    dbm, unique, total = sd.summary_of(s, hits)
    assert dbm == ref["dbmatched"] and (unique, total) == sd.log_counts(ref["log"])
