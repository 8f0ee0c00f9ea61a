"""--lcaout on the device (vsx_lca_index_create, vsx_lca; vsearch_amd.lca) against the library's host restatement on every result
array and against the reference CLI's recorded files, over the sets of tests/lca_data.py -- with whole hashes, with three bits and
with one bit of them, so that the verification and the host's numbering decide; the split kernel's start / len against the shared
tax_split on every label of every set and on 20 000 seeded labels with decoys; windows of 1 and 7 queries; labels at scattered,
shared and reversed spans; a call after a larger one and two calls byte for byte; every route to the host with its counter; the
digest of all sets under poisoned device memory; and three searches against the live reference binary build() leaves in
oracle/_ref (skipped only where that binary is absent).
"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import lca_data as ld

pytestmark = pytest.mark.gpu

lc = ld.lca_module()
needs_cli = pytest.mark.skipif(not os.path.exists(ld.ref_binary()), reason="oracle/_ref/vsearch_ref not built")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ("host_no_context", "host_environment", "host_count", "host_memory")
CHILD_TIMEOUT = 120
FATAL_STATUS = (134, 139, -6, -11, 124, 137)


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


@pytest.fixture(scope="module")
def golden():
    return ld.load_golden()


@pytest.fixture(scope="module")
def sets():
    """every named set with the host restatement's answer per option combination, made once"""
    return [dict(s, host={combo: ld.run_set(s, combo, host=True).arrays() for combo in ld.COMBOS}) for s in ld.all_sets()]


def device_index(aligner, labels, collision=False):
    index = lc.LcaIndex(labels, ctx=aligner)
    st = index.stats
    assert sum(st[r] for r in ROUTES) == 0 and st["labels_device"] == len(index.split()[0]) and st["labels_host"] == 0, st
    assert st["host_collision"] == int(collision), st
    return index


def on_device(index, s, combo, window=0):
    res = ld.run_set(s, combo, index=index, window=window)
    st = res.stats
    assert sum(st[r] for r in ROUTES) == 0 and st["queries_host"] == 0 and st["queries_device"] == len(s["hits"]), st
    assert st["hits_device"] == sum(len(h) for h in s["hits"])
    return res


def assert_sets_on_device(aligner, sets, collision=False):
    collided = 0
    for s in sets:
        index = lc.LcaIndex(s["tlabels"], ctx=aligner)
        assert sum(index.stats[r] for r in ROUTES) == 0 and index.stats["labels_device"] == len(s["tlabels"])
        if not collision:
            assert index.stats["host_collision"] == 0
        collided += index.stats["host_collision"]
        with index:
            for combo in ld.COMBOS:
                res = on_device(index, s, combo)
                for k, (a, b) in enumerate(zip(res.arrays(), s["host"][combo])):
                    assert a == b, (s["name"], combo, k)
                assert res.stats["host_collision"] == index.stats["host_collision"]
    return collided


def test_every_set(aligner, sets):
    assert_sets_on_device(aligner, sets)


def test_the_files_are_the_recorded_ones(aligner, golden):
    tl, ql = [l for l, _ in golden["db"]], [l for l, _ in golden["queries"]]
    with device_index(aligner, tl) as index:
        for r in golden["runs"]:
            if r["lcaout"] is None:                                      # --search_exact: the reference writes no --lcaout file
                continue
            raw = ld.make_hits(ld.golden_hitlists(golden, r["command"]))
            res = lc.lca(index, raw, lca_cutoff=float(r["cutoff"]), maxhits=r["maxhits"], top_hits_only=r["top_hits_only"])
            assert res.stats["queries_device"] == len(ql)
            assert b"".join(lc.lcaout_lines(res, ql, tl)).decode("latin-1") == r["lcaout"], r


@pytest.mark.parametrize("bits", [3, 1])
def test_every_set_with_cut_hashes(aligner, sets, monkeypatch, bits):
    """eight hash values, then two: different prefixes share runs, the verification sees it and the host numbers the index"""
    monkeypatch.setenv("VSX_LCA_HASH_BITS", str(bits))
    collided = assert_sets_on_device(aligner, sets, collision=True)
    assert collided >= len(sets) - 2                                      # (a set whose labels all split alike has one prefix per level)
    s = ld.random_set(7)
    with lc.LcaIndex(s["tlabels"], ctx=aligner) as index:
        assert index.stats["host_collision"] == 1
        assert on_device(index, s, s["combo"]).arrays() == ld.run_set(s, s["combo"], host=True).arrays()


def test_the_split_kernel_is_tax_split(aligner, sets):
    for s in sets:
        with device_index(aligner, s["tlabels"]) as index, lc.LcaIndex(s["tlabels"]) as host:
            for a, b in zip(index.split(), host.split()):
                assert np.array_equal(a, b), s["name"]
    labels = ld.random_labels()
    assert len(labels) == 20000 and min(map(len, labels)) == 0 and max(map(len, labels)) == 400
    with device_index(aligner, labels) as index, lc.LcaIndex(labels) as host:
        dev, ref = index.split(), host.split()
        for a, b in zip(dev, ref):
            diff = np.nonzero((a != b).any(axis=1))[0]
            assert len(diff) == 0, (int(diff[0]), labels[int(diff[0])], a[diff[0]], b[diff[0]])
        named = (ref[0] > 0).sum(axis=0)
        assert named.min() > 100 and (ref[1].max(axis=1) > 64).sum() > 20        # every rank is named often; names longer than a step occur
        py = [ld.py_tax_split(l) for l in labels[:2000]]
        assert [list(map(int, x)) for x in ref[0][:2000]] == [p[0] for p in py] and [list(map(int, x)) for x in ref[1][:2000]] == [p[1] for p in py]


def many_queries(seed=409, n=300):
    """one set of many queries over a few labels, so that windows cut it"""
    rng = random.Random(seed)
    base = ld.random_set(seed)
    hits = []
    for _ in range(n):
        k = rng.choice((0, 1, 2, 3, 5, 8, 64, 65, 130)) if rng.random() < 0.3 else rng.randint(1, 10)
        fav = rng.randrange(len(base["tlabels"]))
        hits.append([(fav if rng.random() < 0.7 else rng.randrange(len(base["tlabels"])), rng.choice((100.0, 99.0, 98.5))) for _ in range(k)])
    return dict(base, hits=hits, qlabels=[ld.B("q%d" % i) for i in range(n)])


@pytest.mark.parametrize("window", [1, 7])
def test_windows(aligner, window):
    s = many_queries()
    with device_index(aligner, s["tlabels"]) as index:
        for combo in ((0.51, 0, False), (0.75, 3, True), (1.0, 0, True)):
            whole = on_device(index, s, combo)
            cut = on_device(index, s, combo, window=window)
            assert cut.stats["windows"] == -(-len(s["hits"]) // window) and whole.stats["windows"] == 1
            assert cut.arrays() == whole.arrays() == ld.run_set(s, combo, host=True).arrays()


def scattered(labels, seed):
    """the labels laid out in another order with gaps between them; equal labels share one span"""
    rng = random.Random(seed)
    order = list(range(len(labels)))
    rng.shuffle(order)
    off, parts, at, seen = np.zeros(len(labels), np.uint64), [], 0, {}
    for k in order:
        if labels[k] in seen and rng.random() < 0.5:
            off[k] = seen[labels[k]]
            continue
        gap = rng.randint(0, 5)
        parts.append(b",;tax="[:gap] + labels[k])
        off[k] = seen[labels[k]] = at + gap
        at += gap + len(labels[k])
    return lc.LabelBlob.of(b"".join(parts) + b";tax=d:", off, [len(l) for l in labels])


def test_scattered_shared_and_reversed_spans(aligner, sets):
    for s in sets:
        combo = (0.51, 0, False)
        with device_index(aligner, scattered(s["tlabels"], 419)) as index:
            assert on_device(index, s, combo).arrays() == s["host"][combo], s["name"]
        n = len(s["tlabels"])
        back = dict(s, tlabels=s["tlabels"][::-1], hits=[[(n - 1 - t, i) for t, i in h] for h in s["hits"]])
        with device_index(aligner, back["tlabels"]) as index:
            res = on_device(index, back, combo)
            want = ld.run_set(back, combo, host=True)
            assert res.arrays() == want.arrays() and res.arrays()[:3] == s["host"][combo][:3], s["name"]
            assert lc.lcaout_lines(res, s["qlabels"], back["tlabels"]) == lc.lcaout_lines(ld.run_set(s, combo, host=True), s["qlabels"], s["tlabels"])


def test_repeatable(aligner, sets):
    """two calls, and a call after a larger one on the same context (its scratch blocks come back used)"""
    s = next(x for x in sets if x["name"] == "lengths")
    combo = (0.51, 0, True)
    with device_index(aligner, s["tlabels"]) as index:
        a = on_device(index, s, combo)
        b = on_device(index, s, combo)
        big = many_queries(421, 3000)
        with device_index(aligner, ld.random_labels(5000, 431) + big["tlabels"]) as other:
            shifted = dict(big, hits=[[(t + 5000, i) for t, i in h] for h in big["hits"]])
            assert on_device(other, shifted, combo).arrays()[:3] == ld.run_set(big, combo, host=True).arrays()[:3]
        c = on_device(index, s, combo)
        assert a.arrays() == b.arrays() == c.arrays() == s["host"][combo]
    with device_index(aligner, s["tlabels"]) as again:
        assert [x.tobytes() for x in again.split()] == [x.tobytes() for x in lc.LcaIndex(s["tlabels"]).split()]
        assert on_device(again, s, combo).arrays() == a.arrays()


def test_host_routes_and_their_counters(aligner, sets, monkeypatch):
    s = next(x for x in sets if x["name"] == "ties")
    combo = (0.51, 0, True)
    want = s["host"][combo]
    nq, nh, nl = len(s["hits"]), sum(len(h) for h in s["hits"]), len(s["tlabels"])

    def routed(index, counter):
        res = ld.run_set(s, combo, index=index)
        assert {r: res.stats[r] for r in ROUTES} == {r: int(r == counter) for r in ROUTES}, res.stats
        assert res.stats["queries_device"] == 0 and res.stats["queries_host"] == nq and res.stats["hits_host"] == nh and res.arrays() == want

    def host_index(counter):
        index = lc.LcaIndex(s["tlabels"], ctx=aligner if counter != "host_no_context" else None)
        assert {r: index.stats[r] for r in ROUTES} == {r: int(r == counter) for r in ROUTES}, index.stats
        assert index.stats["labels_device"] == 0 and index.stats["labels_host"] == nl
        return index

    # the index goes to the host: every call on it follows, for the index's reason
    with host_index("host_no_context") as index:
        routed(index, "host_no_context")
    with monkeypatch.context() as m:
        m.setenv("VSX_LCA", "host")
        with host_index("host_environment") as index:
            routed(index, "host_environment")
    with monkeypatch.context() as m:
        m.setenv("VSX_LCA_DEVICE_COUNT", str(9 * nl - 1))
        with host_index("host_count") as index:
            routed(index, "host_count")
    with monkeypatch.context() as m:
        m.setenv("VSX_LCA_PRETEND_BYTES", str(1 << 50))
        with host_index("host_memory") as index:
            routed(index, "host_memory")
    # a device index, the call goes to the host
    with device_index(aligner, s["tlabels"]) as index:
        with monkeypatch.context() as m:
            m.setenv("VSX_LCA", "host")
            routed(index, "host_environment")
        with monkeypatch.context() as m:
            m.setenv("VSX_LCA_DEVICE_COUNT", str(nh - 1))
            routed(index, "host_count")
        with monkeypatch.context() as m:
            m.setenv("VSX_LCA_DEVICE_COUNT", str(max(nh, 9 * nl)))
            assert on_device(index, s, combo).arrays() == want          # at the limit the device still answers
        with monkeypatch.context() as m:
            m.setenv("VSX_LCA_PRETEND_BYTES", str(1 << 50))
            routed(index, "host_memory")
        assert on_device(index, s, combo).arrays() == want


def test_refusals_on_the_device_route(aligner):
    from vsearch_amd import VsxError
    with pytest.raises(VsxError) as e:
        lc.LcaIndex(lc.LabelBlob.of(b"abc", [1], [3]), ctx=aligner)
    assert e.value.code == -1
    with pytest.raises(VsxError) as e:
        lc.LcaIndex([b"a\0"], ctx=aligner)
    assert e.value.code == -1
    with lc.LcaIndex(["a;tax=d:A"], ctx=aligner) as index:
        for bad in (lambda: lc.lca(index, ld.make_hits([[(1, 99.0)]])), lambda: lc.lca(index, ld.make_hits([[(0, 99.0)]]), lca_cutoff=0.5),
                    lambda: lc.lca(index, (np.array([0, 2], np.uint64), ld.make_hits([[(0, 99.0)]])[1]))):
            with pytest.raises(VsxError) as e:
                bad()
            assert e.value.code == -1


def test_digest_under_poisoned_memory(aligner):
    """the digest of every set's device result in a child process per poison byte; a child that fails, faults or runs into its time
    limit ends the sequence"""
    want = ld.device_digest(aligner)
    for byte in ("0x00", "0xA5", "0xFF"):
        env = dict(os.environ, VSX_POISON="1", VSX_POISON_BYTE=byte)
        try:
            p = subprocess.run([sys.executable, "-m", "tests.lca_data", "--digest"], env=env, cwd=ROOT, capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.fail(f"the child under poison byte {byte} ran into its time limit of {CHILD_TIMEOUT} s; no further child was started")
        text = p.stdout + p.stderr
        assert p.returncode == 0 and p.returncode not in FATAL_STATUS and "illegal memory access" not in text, (byte, p.returncode, text[-2000:])
        lines = [l for l in p.stdout.splitlines() if l.startswith("digest ")]
        assert lines == [f"digest {want} poison {int(byte, 16)}"], (byte, text[-2000:])


# ---- against the live CLI -----------------------------------------------------------------------------------------------------------
def cli_text(tmp, command, db, dbl, qs, ql, search, cutoff, top_hits_only=False):
    ld.write_fasta(os.path.join(tmp, "db.fa"), zip(dbl, db))
    ld.write_fasta(os.path.join(tmp, "q.fa"), zip(ql, qs))
    return ld.cli_lcaout(tmp, command, search, cutoff, top_hits_only=top_hits_only)[0]


def live_search(aligner, tmp_path, seed, top_hits_only):
    from vsearch_amd import SearchSession
    rng = random.Random(seed)
    db, dbl = ld.live_db(rng)
    qs, ql = ld.live_queries(rng, db)
    ref = cli_text(str(tmp_path), "usearch_global", db, dbl, qs, ql, ["--id", "0.9", "--maxaccepts", "8", "--maxrejects", "32"], "0.8", top_hits_only)
    sess = SearchSession(aligner, db, labels=dbl, id=0.9, maxaccepts=8, maxrejects=32)
    raw = sess.search_batch_raw(qs, labels=ql)
    sess.close()
    with device_index(aligner, dbl) as index:
        res = lc.lca(index, raw, lca_cutoff=0.8, top_hits_only=top_hits_only)
    assert sum(res.stats[r] for r in ROUTES) == 0 and res.stats["queries_device"] == len(qs)
    depths = set(int(d) for d in res.depth)
    assert np.any(np.diff(raw[0].astype(np.int64)) > 4) and len(depths) >= 4 and 0 in depths, depths
    assert b"".join(lc.lcaout_lines(res, ql, dbl)).decode("latin-1") == ref
    assert lc.lca_host(dbl, raw, lca_cutoff=0.8, top_hits_only=top_hits_only).arrays() == res.arrays()
    return res


@needs_cli
def test_usearch_global_against_the_live_cli(aligner, tmp_path):
    live_search(aligner, tmp_path, 433, False)


@needs_cli
def test_usearch_global_top_hits_only_against_the_live_cli(aligner, tmp_path):
    res = live_search(aligner, tmp_path, 439, True)
    assert np.any(res.n_top > 1)                                          # ties at the top occur


@needs_cli
def test_search_exact_against_the_live_cli(aligner, tmp_path):
    """the reference's --search_exact accepts --lcaout and writes no file: that is what the CLI is held to here; the hits of
    search_exact_raw go through the kernels against the host restatement and the plain-Python loops"""
    from vsearch_amd import SearchSession
    rng = random.Random(443)
    db, dbl = ld.live_db(rng)
    qs, ql = ld.live_queries(rng, db)
    assert cli_text(str(tmp_path), "search_exact", db, dbl, qs, ql, [], "0.8") is None
    sess = SearchSession(aligner, db, labels=dbl, id=1.0)
    raw = sess.search_exact_raw(qs, labels=ql)
    sess.close()
    with device_index(aligner, dbl) as index:
        res = lc.lca(index, raw, lca_cutoff=0.8)
    assert res.stats["queries_device"] == len(qs) and np.any(np.diff(raw[0].astype(np.int64)) > 1)
    assert lc.lca_host(dbl, raw, lca_cutoff=0.8).arrays() == res.arrays()
    hitlists = [[(int(h["target"]), float(h["id"])) for h in raw[1][int(a):int(b)]] for a, b in zip(raw[0][:-1], raw[0][1:])]
    lines, _ = ld.py_lca(dbl, ql, hitlists, 0.8)
    assert lc.lcaout_lines(res, ql, dbl) == lines
