"""SINTAX on the device (vsx_sintax: the sample, count-and-select and vote kernels of vsx_sintax.hip) against the library's host
restatement field for field (with the round winners of both strands), against the recorded lines of the reference CLI
(tests/golden/sintax_golden.json), and once against the live reference binary build() leaves in oracle/_ref.

Every device call must be answered by the kernels (queries_device == n).  The tile of the packed index holds 32 630 sequences
(vsx_kmer_pack.h): the tile-edge databases put the winner on both sides of that edge.
"""
import contextlib
import os
import random

import numpy as np
import pytest

from tests import sintax_data as sd

pytestmark = pytest.mark.gpu

TILE = 32630

needs_cli = pytest.mark.skipif(not os.path.exists(sd.ref_binary()), reason="oracle/_ref/vsearch_ref not built")


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


@pytest.fixture(scope="module")
def golden():
    return {s["name"]: s for s in sd.load_golden()}


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
    o = sd.full_opts(s["opts"])
    kw = dict(id=0.97, wordlength=o["wordlength"], soft_mask=sd.MASK_MODES[o["dbmask"]], hardmask=1 if o["hardmask"] else 0)
    kw.update(extra)
    sess = SearchSession(aligner, s["db"], labels=s["db_labels"], **kw)
    try:
        yield sess
    finally:
        sess.close()


def call_kw(s):
    o = sd.full_opts(s["opts"])
    return dict(randseed=o["seed"], strand_both=o["strand_both"], sintax_random=o["random"], want_candidates=True)


def on_device(sess, s, route="queries_device", **extra):
    from vsearch_amd import sintax
    kw = call_kw(s)
    kw.update(extra)
    res = sintax(sess, s["queries"], **kw)
    assert res.stats[route] == len(s["queries"]), res.stats
    assert sum(res.stats[k] for k in res.stats if k.startswith("queries_")) == len(s["queries"])
    return res


def on_host(s, **extra):
    from vsearch_amd import sintax_host
    o = sd.full_opts(s["opts"])
    kw = call_kw(s)
    kw.update(wordlength=o["wordlength"], soft_mask=sd.MASK_MODES[o["dbmask"]], hardmask=1 if o["hardmask"] else 0)
    kw.update(extra)
    return sintax_host(s["db"], s["db_labels"], s["queries"], **kw)


def assert_same(a, b, what):
    fa, fb = a.fields(), b.fields()
    assert set(fa) == set(fb)
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), (what, k, np.argwhere(np.asarray(fa[k]) != np.asarray(fb[k]))[:5])
    assert a.n_classified == b.n_classified


def route_of(s):
    o = sd.full_opts(s["opts"])
    return "queries_host_random" if o["random"] else "queries_host_wordlength" if o["wordlength"] > 8 else "queries_device"


# ---- every set: device = host restatement, and the formatted text = the reference's ---------------------------------------------------
def test_golden_sets(aligner, golden):
    from vsearch_amd import tabbed_lines, log_lines
    for s in golden.values():
        with session(aligner, s) as sess:
            res = on_device(sess, s, route_of(s))
        assert_same(res, on_host(s), s["name"])
        assert tabbed_lines(res, s["qlabels"], s["db_labels"], sd.full_opts(s["opts"])["cutoff"]) == s["ref"]["tabbed"], s["name"]
        assert log_lines(res) == s["ref"]["log"], s["name"]


def test_hardmask_and_dust_masked_databases(aligner):
    for s in sd.hardmask_sets():
        with session(aligner, s) as sess:
            res = on_device(sess, s)
        assert_same(res, on_host(s), s["name"])
        assert [int(x) for x in res.classified] == [0, 1, 1], s["name"]


# ---- tile edges ------------------------------------------------------------------------------------------------------------------
_FILL = {}


def filler(n, length=40):
    if "all" not in _FILL:
        rng = np.random.default_rng(20261019)
        codes = rng.integers(0, 4, size=(2 * TILE + 64, length), dtype=np.uint8)
        text = np.frombuffer(b"ACGT", np.uint8)[codes]
        _FILL["all"] = [row.tobytes().decode() for row in text]
    return list(_FILL["all"][:n])


def edge_set(name, db, queries):
    return sd._set(name, db, [f"s{i};tax=d:D,p:P{i % 7},g:G{i};" for i in range(len(db))], queries, dict(seed=41, strand_both=1, dbmask="none"))


def winners(res):
    return [int(res.rank_seq[q, 6]) for q in range(res.n)]


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1])
def test_tile_edge_last_sequence(aligner, n):
    """the winner is the database's last sequence: inside tile 0, the last of tile 0, the first of tile 1"""
    rng = random.Random(n)
    db = filler(n)
    a = sd.no_repeat_seq(rng, 40)
    db[n - 1], db[n // 2] = a, sd.no_repeat_seq(rng, 40)
    s = edge_set(f"edge_{n}", db, [a, sd.revcomp(a), db[n // 2]])
    with session(aligner, s) as sess:
        res = on_device(sess, s)
        assert res.stats["tiles"] == (n + TILE - 1) // TILE
    assert_same(res, on_host(s), s["name"])
    assert winners(res) == [n - 1, n - 1, n // 2] and list(res.strand) == [0, 1, 0] and all(res.classified)


def test_three_tiles(aligner):
    """one database of three tiles: the winner in each tile in turn; an identical pair across the first edge (the lower number
    wins); a shorter sequence with the same count in a later tile than the longer one (the shorter wins)"""
    rng = random.Random(5)
    n = 2 * TILE + 10
    db = filler(n)
    e, g, h, c, d = (sd.no_repeat_seq(rng, 40) for _ in range(5))
    db[7], db[TILE + 5], db[2 * TILE + 3] = e, g, h
    db[TILE - 1], db[TILE] = c, c
    db[50], db[TILE + 10] = d, d[:39]
    s = edge_set("edge_three_tiles", db, [e, g, h, c, d[:39], sd.revcomp(h)])
    with session(aligner, s) as sess:
        res = on_device(sess, s)
        assert res.stats["tiles"] == 3
    assert_same(res, on_host(s), s["name"])
    assert winners(res) == [7, TILE + 5, 2 * TILE + 3, TILE - 1, TILE + 10, 2 * TILE + 3] and all(res.classified)


# ---- windows, query numbers, repeatability -------------------------------------------------------------------------------------------
def test_windows_offsets_and_query_numbers(aligner, golden):
    from vsearch_amd import sintax
    s = golden["strands"]
    n = len(s["queries"])
    with session(aligner, s) as sess:
        whole = on_device(sess, s)
        for window in (1, 7):
            assert_same(on_device(sess, s, window=window), whole, f"window {window}")
        # the sequences scattered over a blob with gaps, in reversed order, each with its own number
        rng = random.Random(9)
        blob, off, lens = bytearray(), [], []
        for q in reversed(s["queries"]):
            blob += bytes(rng.choice(b"ACGTN") for _ in range(rng.randrange(1, 9)))
            off.append(len(blob))
            lens.append(len(q))
            blob += q.encode()
        rev = sintax(sess, (bytes(blob), off, lens), query_numbers=list(range(n))[::-1], **call_kw(s))
        part = sintax(sess, s["queries"][3:12], first_query_no=3, window=4, **call_kw(s))
        again = on_device(sess, s)
    assert rev.stats["queries_device"] == n
    for q in range(n):
        assert rev.record(n - 1 - q) == whole.record(q), q
    for q in range(3, 12):
        assert part.record(q - 3) == whole.record(q), q
    assert again.tobytes() == whole.tobytes()                      # two calls: identical bytes
    assert_same(whole, on_host(s), "strands")


# ---- host routes: each one forced and counted ------------------------------------------------------------------------------------------
def test_host_routes(aligner, golden):
    s = golden["ties"]
    host = on_host(s)
    with session(aligner, s) as sess:
        assert_same(on_device(sess, s), host, "device")
        with environment("VSX_SINTAX", "host"):
            assert_same(on_device(sess, s, "queries_host_forced"), host, "forced")
        with environment("VSX_SINTAX_MAX_DBLEN", "200"):           # the longest sequence has 240 symbols
            assert_same(on_device(sess, s, "queries_host_dblen"), host, "dblen")
        rnd = on_device(sess, s, "queries_host_random", sintax_random=True)
        assert_same(rnd, on_host(s, sintax_random=True), "random")
    with session(aligner, s, wordlength=12) as sess:
        assert_same(on_device(sess, s, "queries_host_wordlength"), on_host(s, wordlength=12), "wordlength")


def test_refusals(aligner, golden):
    from vsearch_amd import SearchSession, VsxError, sintax
    s = golden["ties"]
    with session(aligner, s) as sess:
        with pytest.raises(VsxError, match="randseed 0"):
            sintax(sess, s["queries"], randseed=0)
    sess = SearchSession(aligner, s["db"], id=0.97)
    try:
        with pytest.raises(VsxError, match="no labels"):
            sintax(sess, s["queries"], randseed=3)
    finally:
        sess.close()


# ---- the live reference CLI --------------------------------------------------------------------------------------------------------
def live_set():
    rng = random.Random(77)
    db, labels = sd.taxonomy_db(rng, families=30, genera=10, species=10, length=300)
    qs = []
    for k in range(2000):
        r = rng.random()
        if r < 0.06:
            q = sd.random_seq(rng, 36)                   # fewer than 32 words: never classified
        elif r < 0.12:
            q = sd.random_seq(rng, 150)
        else:
            src = rng.choice(db)
            a = rng.randrange(0, len(src) - 150)
            q = sd.mutate(rng, src[a:a + 150], 0.02)
            if r < 0.55:
                q = sd.revcomp(q)
        qs.append(q)
    return sd._set("live", db, labels, qs, dict(seed=97, strand_both=1, cutoff=0.8))


@needs_cli
def test_live_reference_cli(aligner):
    from vsearch_amd import tabbed_lines, log_lines
    s = live_set()
    assert len(s["db"]) == 3000 and len(s["queries"]) == 2000
    ref = sd.run_reference(s, threads=4)
    cols = [l.split("\t") for l in ref["tabbed"]]
    assert any(c[1] == "" for c in cols) and {c[2] for c in cols if c[1]} == {"+", "-"}       # unclassified, and both strands win
    with session(aligner, s) as sess:
        res = on_device(sess, s)
    assert sorted(tabbed_lines(res, s["qlabels"], s["db_labels"], 0.8)) == sorted(ref["tabbed"])
    assert log_lines(res) == ref["log"]
