"""The search hit writers on the device (vsx_hits_render, vsearch_amd.hitout) against the library's host restatement on every output
array and blob, over the explicit sets of tests/hitout_data.py and seeded random triples, with every `want` bit alone; windows of 1
and 7 hits; queries at scattered and reversed offsets; a call after a larger call of another shape; two calls byte for byte; every
route to the host with its counter; the digest of all sets under poisoned device memory; and two searches against the live reference
binary build() leaves in oracle/_ref, all seven files byte for byte (skipped only where that binary is absent).
"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import hitout_data as hd
from vsearch_amd import hitout as ho

pytestmark = pytest.mark.gpu

needs_cli = pytest.mark.skipif(not os.path.exists(hd.ref_binary()), reason="oracle/_ref/vsearch_ref not built")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ("host_no_context", "host_environment", "host_hit_count", "host_memory")
CHILD_TIMEOUT = 120
FATAL_STATUS = (134, 139, -6, -11, 124, 137)


@pytest.fixture(scope="module")
def aligners(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as a0, Aligner(device=0, n_mismatch=True) as a1:
        yield {0: a0, 1: a1}


def on_device(aligners, s, want=ho.ALL, window=0):
    res = hd.render_explicit(aligners[hd.full_opts(s["opts"])["n_mismatch"]], s, want=want, window=window)
    st = res.stats
    assert sum(st[r] for r in ROUTES) == 0 and st["hits_host"] == 0 and st["hits_device"] == len(s["hits"]), st
    return res


@pytest.fixture(scope="module")
def random_set():
    return hd.random_triples(461, 3000)


@pytest.mark.parametrize("want", (ho.ALL, ho.ROWS, ho.SYMBOLS, ho.SAM))
def test_device_equals_host_on_every_set(aligners, random_set, want):
    for s in hd.explicit_sets() + [random_set]:
        res = on_device(aligners, s, want=want)
        ref = hd.render_explicit(None, s, want=want, host=True)
        assert res.same_as(ref) is None, (s["name"], want, res.same_as(ref))
        assert res.stats["db_text_uploaded"] == 1 and res.stats["windows"] == 1


@pytest.mark.parametrize("window", (1, 7))
def test_windows(aligners, window):
    for s in (hd.gaps_set(), hd.md_events_set(), hd.random_triples(463, 150)):
        res = on_device(aligners, s, window=window)
        assert res.stats["windows"] == -(-len(s["hits"]) // window)
        assert res.same_as(hd.render_explicit(None, s, host=True)) is None, (s["name"], window)


def test_scattered_and_reversed_query_offsets(aligners):
    from vsearch_amd import SearchSession
    s = hd.random_triples(467, 500)
    raw = hd.raw_hits(len(s["queries"]), hd.explicit_records(s))
    rng = random.Random(479)
    blob, off, lens = bytearray(), [0] * len(s["queries"]), [len(q) for q in s["queries"]]
    for q in reversed(range(len(s["queries"]))):                                      # the last query first, junk between them
        blob += bytes(rng.choice(b"ACGT#") for _ in range(rng.randrange(0, 9)))
        off[q] = len(blob)
        blob += s["queries"][q].encode()
    sess = SearchSession(aligners[0], s["db"], id=0.5, **hd.session_opts(s["opts"]))
    try:
        plain = ho.render(sess, s["queries"], raw)
        moved = ho.render(sess, (bytes(blob), off, lens), raw)
    finally:
        sess.close()
    assert plain.stats["hits_host"] == moved.stats["hits_host"] == 0 and moved.stats["db_text_uploaded"] == 0
    assert moved.same_as(plain) is None and plain.same_as(hd.render_explicit(None, s, host=True)) is None


def test_repeatable_and_after_a_larger_call(aligners, random_set):
    """two calls, and a call after a larger call of another shape on the same searcher (its buffers come back used)"""
    from vsearch_amd import SearchSession
    small, big = hd.gaps_set(), random_set
    db = small["db"] + big["db"]
    shift = lambda s, by: hd.raw_hits(len(s["queries"]), [dict(r, target=r["target"] + by) for r in hd.explicit_records(s)])
    sess = SearchSession(aligners[0], db, id=0.5, **hd.session_opts({}))
    try:
        a = ho.render(sess, small["queries"], shift(small, 0))
        b = ho.render(sess, small["queries"], shift(small, 0))
        big_res = ho.render(sess, big["queries"], shift(big, len(small["db"])))
        c = ho.render(sess, small["queries"], shift(small, 0), want=ho.SAM | ho.SYMBOLS)
        d = ho.render(sess, small["queries"], shift(small, 0))
    finally:
        sess.close()
    assert all(r.stats["hits_host"] == 0 for r in (a, b, big_res, c, d))
    assert (a.stats["db_text_uploaded"], b.stats["db_text_uploaded"]) == (1, 0)
    assert a.same_as(b) is None and a.same_as(d) is None and a.md_blob == c.md_blob
    assert a.same_as(hd.render_explicit(None, small, host=True)) is None


def test_host_routes_and_their_counters(aligners, monkeypatch):
    s = hd.md_events_set()
    ref = hd.render_explicit(None, s, host=True)
    n = len(s["hits"])
    assert {r: ref.stats[r] for r in ROUTES} == {r: int(r == "host_no_context") for r in ROUTES}

    def routed(counter):
        res = hd.render_explicit(aligners[0], s)
        assert {r: res.stats[r] for r in ROUTES} == {r: int(r == counter) for r in ROUTES}
        assert res.stats["hits_device"] == 0 and res.stats["hits_host"] == n and res.same_as(ref) is None

    with monkeypatch.context() as m:
        m.setenv("VSX_HITOUT", "host")
        routed("host_environment")
    with monkeypatch.context() as m:
        m.setenv("VSX_HITOUT_DEVICE_HITS", str(n - 1))
        routed("host_hit_count")
    with monkeypatch.context() as m:
        m.setenv("VSX_HITOUT_DEVICE_HITS", str(n))
        on_device(aligners, s)                                                        # at the limit the device still answers
    with monkeypatch.context() as m:
        m.setenv("VSX_HITOUT_PRETEND_BYTES", str(1 << 50))
        routed("host_memory")
    on_device(aligners, s)


def test_refusal_on_the_device_route(aligners):
    from vsearch_amd import SearchSession, VsxError
    s = hd.lengths_set()
    recs = hd.explicit_records(s)
    recs[3] = dict(recs[3], cigar="63M")
    sess = SearchSession(aligners[0], s["db"], id=0.5, **hd.session_opts(s["opts"]))
    try:
        with pytest.raises(VsxError) as e:
            ho.render(sess, s["queries"], hd.raw_hits(len(s["queries"]), recs))
        assert e.value.code == -1
    finally:
        sess.close()


def test_digest_under_poisoned_memory(aligners):
    """the digest of every set's device result in a child process per poison byte; a child that fails, faults or runs into its time
    limit ends the sequence"""
    want = hd.device_digest(aligners)
    for byte in (None, "0x00", "0xA5", "0xFF"):
        env = {k: v for k, v in os.environ.items() if k not in ("VSX_POISON", "VSX_POISON_BYTE")}
        if byte is not None:
            env.update(VSX_POISON="1", VSX_POISON_BYTE=byte)
        try:
            p = subprocess.run([sys.executable, "-m", "tests.hitout_data", "--digest"], env=env, cwd=ROOT, capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.fail(f"the child under poison byte {byte} ran into its time limit of {CHILD_TIMEOUT} s; no further child was started")
        text = p.stdout + p.stderr
        assert p.returncode == 0 and p.returncode not in FATAL_STATUS and "illegal memory access" not in text, (byte, p.returncode, text[-2000:])
        lines = [l for l in p.stdout.splitlines() if l.startswith("digest ")]
        assert lines == [f"digest {want} poison {-1 if byte is None else int(byte, 16)}"], (byte, text[-2000:])


# ---- against the live CLI -----------------------------------------------------------------------------------------------------------
def live_set(name, command, opts, fmt, search_args, seed):
    db, qs = hd.live_inputs(seed)
    return hd._cli(name, opts=opts, fmt=fmt, search_args=search_args, command=command, inputs=(db, qs))


def assert_live(aligner, s, tmp_path, search, names):
    from vsearch_amd import SearchSession
    ref = hd.run_reference(s, tmp=tmp_path)
    sess = SearchSession(aligner, s["db"], **search, **hd.session_opts(s["opts"]))
    try:
        raw = sess.search_exact_raw(s["queries"]) if s["command"] == "search_exact" else sess.search_batch_raw(s["queries"])
        text = ho.render(sess, s["queries"], raw)
    finally:
        sess.close()
    assert text.stats["hits_host"] == 0 and text.stats["hits_device"] == len(raw[1]) > 1000
    assert np.any(raw[1]["strand"] == 1) and np.any(np.diff(raw[0].astype(np.int64)) == 0) and np.any(np.diff(raw[0].astype(np.int64)) > 1)
    got = hd.format_all(text, s)
    for name in names:
        assert got[name] == ref[name], (s["name"], name)
    assert hd.sam_header_of(text, s, ref["samheader"]) == ref["samheader"]


@needs_cli
@pytest.mark.parametrize("hardmask", (0, 1))
def test_usearch_global_against_the_live_cli(aligners, tmp_path, hardmask):
    """--usearch_global --strand both --maxaccepts 4 --maxhits 3 --output_no_hits with the default DUST masking, and with --hardmask"""
    s = live_set("live_global", "usearch_global", dict(qmask="dust", dbmask="dust", hardmask=hardmask), dict(maxhits=3, output_no_hits=1),
                 ("--id", "0.9", "--maxaccepts", "4"), 487)
    assert_live(aligners[0], s, tmp_path, dict(id=0.9, maxaccepts=4), hd.WRITERS + ("userout_reversed",))


@needs_cli
def test_search_exact_against_the_live_cli(aligners, tmp_path):
    db, qs = hd.live_inputs(491)
    rng = random.Random(499)
    qs = [(hd.revcomp(db[rng.randrange(len(db))]) if k % 3 == 0 else db[rng.randrange(len(db))]) if k % 10 else q for k, q in enumerate(qs)]
    db = db + db[:40]                                                                 # duplicates: second hits
    s = hd._cli("live_exact", opts={}, fmt=dict(output_no_hits=1), search_args=(), command="search_exact", inputs=(db, qs))
    assert_live(aligners[0], s, tmp_path, dict(id=1.0), ("samout", "blast6out"))
