"""Orientation on the device (vsx_orient: the build, count and emit kernels of vsx_orient.hip) against the library's host restatement
field for field (records, oriented text, qualities), against the recorded text of the reference CLI
(tests/golden/orient_golden.json), the device's match-count table against the plain-Python restatement word for word, and once
against the live reference binary build() leaves in oracle/_ref.

Every device call must be answered by the kernels: the stats count each route and the tests assert the counts.
The count kernel's length classes end at 512, 4 096 and 16 384 (VSX_ORIENT_MAX_QLEN) symbols; VSX_ORIENT_BUILD_KEYS is the key
budget of a chunk of the table build (tests lower it so that small databases are cut).
"""
import contextlib
import os
import random

import numpy as np
import pytest

from tests import orient_data as od

pytestmark = pytest.mark.gpu

needs_cli = pytest.mark.skipif(not os.path.exists(od.ref_binary()), reason="oracle/_ref/vsearch_ref not built")


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


@pytest.fixture(scope="module")
def golden():
    return {s["name"]: s for s in od.load_golden()}


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
def session(aligner, db, wordlength=12, dbmask="dust", hardmask=0):
    from vsearch_amd.orient import orient_session
    sess = orient_session(aligner, db, wordlength=wordlength, soft_mask=od.MASK_MODES[dbmask], hardmask=1 if hardmask else 0)
    try:
        yield sess
    finally:
        sess.close()


def set_session(aligner, s):
    o = od.full_opts(s["opts"])
    return session(aligner, s["db"], o["wordlength"], o["dbmask"], o["hardmask"])


def on_device(sess, queries, quals=None, routes=None, **kw):
    """routes: {stat: count} the call must report; default: every query on the device"""
    from vsearch_amd.orient import orient
    res = orient(sess, queries, quals=quals, **kw)
    n = res.n
    want = dict(queries_device=n) if routes is None else routes
    for k in ("queries_device", "queries_host_wordlength", "queries_host_qlen", "queries_host_forced"):
        assert res.stats[k] == want.get(k, 0), (k, res.stats)
    assert sum(res.stats["queries_class"]) == res.stats["queries_device"]
    return res


def on_host(db, queries, quals=None, wordlength=12, dbmask="dust", hardmask=0, **kw):
    from vsearch_amd.orient import orient_host
    return orient_host(db, queries, quals=quals, wordlength=wordlength, soft_mask=od.MASK_MODES[dbmask], hardmask=1 if hardmask else 0, **kw)


def assert_same(a, b, what):
    fa, fb = a.fields(), b.fields()
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), (what, k, np.argwhere(np.asarray(fa[k]) != np.asarray(fb[k]))[:5].ravel())
    assert (a.n_fwd, a.n_rev, a.n_none) == (b.n_fwd, b.n_rev, b.n_none), what
    assert a.text == b.text and a.qual == b.qual, what
    assert a.stats["words_distinct"] == b.stats["words_distinct"], what


def mixed(seed, n_db=30, db_len=300):
    """a database of random sequences (one partly lower case, one low-complexity) and a function that cuts reads from it"""
    rng = random.Random(seed)
    db = [od.random_seq(rng, db_len) for _ in range(n_db)]
    db[1] = db[1][:db_len // 2].lower() + db[1][db_len // 2:]
    db[2] = db[2][:100] + "AT" * 40 + db[2][180:]

    def read(length, k):
        """a read of exactly `length` symbols made of database pieces; every other one reverse-complemented"""
        parts, have = [], 0
        while have < length:
            t = db[rng.randrange(n_db)]
            a = rng.randrange(0, db_len - 20)
            piece = t[a:a + min(rng.randrange(20, db_len), length - have)]
            parts.append(piece)
            have += len(piece)
        r = "".join(parts)[:length]
        return od.revcomp(r) if k % 2 else r
    return rng, db, read


def qualities(rng, reads):
    return ["".join(chr(33 + rng.randrange(41)) for _ in r) for r in reads]


# ---- every set: device = host restatement, and the formatted text = the reference's ---------------------------------------------------
def test_golden_sets(aligner, golden):
    for s in list(golden.values()) + [od.wordlength_15_set()]:
        o = od.full_opts(s["opts"])
        n = len(s["queries"])
        routes = dict(queries_host_wordlength=n) if o["wordlength"] > 12 else None
        with set_session(aligner, s) as sess:
            res = on_device(sess, s["queries"], s["quals"], routes, qmask=o["qmask"])
        assert_same(res, on_host(s["db"], s["queries"], s["quals"], o["wordlength"], o["dbmask"], o["hardmask"], qmask=o["qmask"]), s["name"])
        if "ref" in s:
            od.assert_text_equals_golden(res, s)
    assert od.full_opts(golden["ratio_edges"]["opts"])["wordlength"] == 12                # the command's default runs on the device


# ---- the table: every word of three databases -----------------------------------------------------------------------------------------
def expected_table(db, w, dbmask, hardmask=0):
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    table = np.zeros(4 ** w, np.uint32)
    for word, count in od.match_counts(db, w, dbmask, hardmask).items():
        x = 0
        for c in word:
            x = x * 4 + code[c]
        table[x] = count
    return table


def assert_table(sess, db, w, dbmask, hardmask=0):
    from vsearch_amd.orient import matchcounts
    want = expected_table(db, w, dbmask, hardmask)
    got = matchcounts(sess, np.arange(4 ** w, dtype=np.uint32))
    assert np.array_equal(got, want), (w, dbmask, np.argwhere(got != want)[:5].ravel())
    return want


def test_matchcounts_equal_python_on_every_word(aligner, golden):
    _, db, _ = mixed(301)
    db += ["", "ACG", db[0], db[0][:50] + db[3][50:], "N" * 40, db[4].replace("T", "U")]
    for w, dbmask, hardmask in ((3, "none", 0), (8, "soft", 0), (12, "dust", 0), (12, "soft", 1), (9, "dust", 1)):
        with session(aligner, db, w, dbmask, hardmask) as sess:
            table = assert_table(sess, db, w, dbmask, hardmask)
        assert table.max() >= 2
    s = golden["ratio_edges"]
    with set_session(aligner, s) as sess:
        assert assert_table(sess, s["db"], 12, "none").max() == 17
    from vsearch_amd import VsxError
    from vsearch_amd.orient import matchcounts
    with session(aligner, db, 13) as sess, pytest.raises(VsxError):
        matchcounts(sess, [0])
    with session(aligner, db, 5) as sess, pytest.raises(VsxError):
        matchcounts(sess, [4 ** 5])


def test_build_chunk_boundaries_and_a_repeating_long_sequence(aligner):
    from vsearch_amd.orient import last_stats
    rng = random.Random(307)
    shared = od.markers(rng, 8, 12)
    # eight sequences of 500 symbols; sequences k and k + 1 share marker k, so every chunk boundary has a word on both sides
    db = []
    for k in range(8):
        body = od.random_seq(rng, 500 - 24)
        db.append(shared[k - 1] + body + shared[k] if k else od.random_seq(rng, 12) + body + shared[k])
    for budget, chunks in ((999, 8), (1000, 4), (1001, 4), (1499, 4), (1500, 3), (10 ** 6, 1)):
        with environment("VSX_ORIENT_BUILD_KEYS", str(budget)), session(aligner, db, 12, "none") as sess:
            assert_table(sess, db, 12, "none")
            st = last_stats()
            assert (st["build_chunks"], st["build_keys"]) == (chunks, 4000), (budget, st)
    # one sequence of 20 000 symbols in which every word occurs twice, far over the budget: a chunk of its own between two others
    half = od.random_seq(rng, 10000)
    db2 = [db[0], half + half, db[1]]
    for w in (12, 8):
        with environment("VSX_ORIENT_BUILD_KEYS", "1000"), session(aligner, db2, w, "none") as sess:
            table = assert_table(sess, db2, w, "none")
            assert last_stats()["build_chunks"] == 3
        if w == 12:
            assert table.max() <= 2 and (table > 0).sum() > 10000
    # two builds give the same table (integer atomics)
    from vsearch_amd.orient import matchcounts
    tables = []
    for _ in range(2):
        with session(aligner, db2, 12, "none") as sess:
            tables.append(matchcounts(sess, np.arange(4 ** 12, dtype=np.uint32)).tobytes())
    assert tables[0] == tables[1]


# ---- the count kernel's edges ----------------------------------------------------------------------------------------------------------
def test_query_lengths_around_a_wave_of_positions(aligner):
    rng, db, read = mixed(311)
    for w in (3, 8, 12):
        qs = [read(n + w - 1, k) for k, n in enumerate((1, 2, 63, 63, 64, 64, 65, 65, 127, 128, 129))]
        with session(aligner, db, w, "soft") as sess:
            res = on_device(sess, qs)
        assert_same(res, on_host(db, qs, None, w, "soft"), w)
        assert res.stats["queries_class"] == [len(qs), 0, 0]


def test_length_classes_at_their_capacities(aligner):
    """capacity - 1, capacity and capacity + 1 symbols in each class; the last + 1 is the host route.  Random text: nearly every
    position is a new distinct word at word length 12, so the sets are as full as they get"""
    rng, db, read = mixed(313, n_db=12, db_len=2000)
    lengths = [n + d for n in od.CLASS_QLEN for d in (-1, 0, 1)]
    qs = [read(n, k) for k, n in enumerate(lengths)] + [od.random_seq(rng, n) for n in od.CLASS_QLEN]
    n = len(qs)
    assert max(len(q) for q in qs) == od.MAX_QLEN + 1
    host = on_host(db, qs, None, 12, "none")
    assert min(len(set(q[p:p + 12] for p in range(len(q) - 11))) / (len(q) - 11) for q in qs[-3:]) > 0.99
    with session(aligner, db, 12, "none") as sess:
        res = on_device(sess, qs, routes=dict(queries_device=n - 1, queries_host_qlen=1))
        assert res.stats["queries_class"] == [3, 4, 4]
        assert_same(res, host, "classes")
        # the same with the slot hash cut to three bits: every word starts its probe in one of eight slots
        with environment("VSX_ORIENT_HASH_BITS", "3"):
            assert_same(on_device(sess, qs, routes=dict(queries_device=n - 1, queries_host_qlen=1)), host, "hash bits")
    for w in (3, 8):                                                                       # many repeats: short chains, full dedup
        with session(aligner, db, w, "none") as sess:
            assert_same(on_device(sess, qs, routes=dict(queries_device=n - 1, queries_host_qlen=1)), on_host(db, qs, None, w, "none"), w)
    assert {"+", "-"} <= {host.record(k)["strand"] for k in range(n)}


def test_windows_offsets_order_and_repeat_calls(aligner):
    rng, db, read = mixed(317)
    qs = [read(rng.randrange(0, 400), k) for k in range(40)] + [read(600, 0), read(5000, 1), "", "N" * 30]
    quals = qualities(rng, qs)
    host = on_host(db, qs, quals, 12, "dust")
    with session(aligner, db) as sess:
        first = on_device(sess, qs, quals)
        assert first.stats["windows"] == 1 and first.stats["build_chunks"] == 1
        assert_same(first, host, "one window")
        again = on_device(sess, qs, quals)
        assert again.stats["build_chunks"] == 0 and again.tobytes() == first.tobytes()           # the table is kept; two calls byte-equal
        for window in (1, 7):
            res = on_device(sess, qs, quals, window=window)
            assert res.stats["windows"] == -(-len(qs) // window)
            assert res.tobytes() == first.tobytes(), window
        # reversed order
        rev = on_device(sess, qs[::-1], quals[::-1], window=7)
        assert [rev.record(k) for k in range(rev.n)] == [first.record(k) for k in range(first.n)][::-1]
        assert rev.text == first.text[::-1] and rev.qual == first.qual[::-1]
        # scattered offsets: the reads in shuffled order with gaps between them, the qualities at the same offsets
        order = list(range(len(qs)))
        rng.shuffle(order)
        blob, qblob, off = bytearray(), bytearray(), [0] * len(qs)
        for k in order:
            gap = rng.randrange(0, 9)
            blob += b"#" * gap
            qblob += b"!" * gap
            off[k] = len(blob)
            blob += qs[k].encode()
            qblob += quals[k].encode()
        lens = [len(q) for q in qs]
        for window in (0, 7):
            sc = on_device(sess, (bytes(blob), off, lens), bytes(qblob), window=window)
            assert sc.tobytes() == first.tobytes(), window


def test_emitted_text_and_qualities(aligner):
    """reads of 0, 1, 63, 64 and 65 symbols with every IUPAC code in both cases, oriented +, - and ?"""
    rng = random.Random(331)
    w = 12
    fwd, rev = od.markers(rng, 2, w)
    db = od.marker_db([(fwd, 1, 0), (rev, 0, 1)])
    tail = lambda n: od.random_seq(rng, n, "ACGTURYSWKMDBHVNacgturyswkmdbhvnXx-")
    qs = ["", "R", "a"]
    for n in (63, 64, 65, 200):
        qs += [fwd + "N" + tail(n - w - 1), rev + "n" + tail(n - w - 1), tail(n)]
        assert all(len(q) == n for q in qs[-3:])
    quals = qualities(rng, qs)
    host = on_host(db, qs, quals, w, "none", qmask="none")
    assert "".join(host.record(k)["strand"] for k in range(3, len(qs))) == "+-?" * 4
    with session(aligner, db, w, "none") as sess:
        res = on_device(sess, qs, quals, qmask="none")
        assert_same(res, host, "emit")
        for k, q in enumerate(qs):
            minus = host.record(k)["strand"] == "-"
            assert res.text[k].decode("latin-1") == (od.revcomp(q) if minus else q), k
            assert res.qual[k].decode("latin-1") == (quals[k][::-1] if minus else quals[k]), k
        bare = on_device(sess, qs, qmask="none")                                                 # FASTA input: no qualities come back
        assert bare.qual is None and bare.text == res.text
        none = on_device(sess, qs, quals, qmask="none", want_text=False)
        assert none.text is None and none.qual is None and np.array_equal(none.strand, res.strand)


# ---- host routes: each one forced and counted ------------------------------------------------------------------------------------------
def test_host_routes(aligner, golden):
    s = golden["wordlength_12"]
    n = len(s["queries"])
    long_read = (s["db"][0] * 103)[:od.MAX_QLEN + 1]
    qs = s["queries"] + [long_read]
    host = on_host(s["db"], qs)
    with session(aligner, s["db"]) as sess:
        assert_same(on_device(sess, qs, routes=dict(queries_device=n, queries_host_qlen=1)), host, "qlen")
        assert_same(on_device(sess, s["queries"] + [long_read[:-1]]), on_host(s["db"], s["queries"] + [long_read[:-1]]), "max qlen")
        with environment("VSX_ORIENT", "host"):
            forced = on_device(sess, qs, routes=dict(queries_host_forced=n + 1))
            assert_same(forced, host, "forced")
            assert forced.stats["windows"] == 0
    for w in (13, 14, 15):
        with session(aligner, s["db"], w) as sess:
            assert_same(on_device(sess, qs, routes=dict(queries_host_wordlength=n + 1)), on_host(s["db"], qs, None, w), w)


def test_refusals(aligner, golden):
    from vsearch_amd import VsxError
    from vsearch_amd.orient import orient
    s = golden["wordlength_12"]
    with set_session(aligner, s) as sess:
        with pytest.raises(VsxError, match="qmask"):
            orient(sess, s["queries"], qmask=5)
        with pytest.raises(VsxError, match="overlap"):
            orient(sess, (s["queries"][0].encode(), [0, 4], [20, 20]))
        with pytest.raises(VsxError, match="exceeds"):
            orient(sess, (b"ACGT", [2], [20]))


# ---- the live reference CLI --------------------------------------------------------------------------------------------------------
@needs_cli
def test_live_reference_cli(aligner):
    from vsearch_amd.orient import tabbed_lines, fasta_lines
    db, reads = od.simulated(97, n_db=200, db_len=400, n_reads=2000, read_len=150, flipped=0.5, unrelated=0.1)
    s = od._set("live", db, reads)
    ref = od.run_reference(s, outputs=("tabbed", "fasta"))
    verdicts = [l.split("\t")[1] for l in ref["tabbed"]]
    assert len(verdicts) == 2000 and min(verdicts.count(c) for c in "+-") >= 500 and verdicts.count("?") >= 20
    with set_session(aligner, s) as sess:
        res = on_device(sess, s["queries"])
    assert "\n".join(tabbed_lines(res, s["qlabels"])) == "\n".join(ref["tabbed"])
    assert "\n".join(fasta_lines(res, s["qlabels"])) == "\n".join(ref["fasta"])
