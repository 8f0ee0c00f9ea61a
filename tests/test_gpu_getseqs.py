"""Sequence extraction by label on the device (vsx_getseqs, vsearch_amd.getseqs) against the library's host restatement on every
record and total and against the reference CLI's recorded files, over the sets of tests/getseqs_data.py -- with whole hashes, with
three bits and with one bit of them, so that every probe runs into false neighbours; match launches of 1 and of 7 headers;
scattered, shared and reversed spans; a call after a larger call and two calls byte for byte; every route to the host with its
counter; the digest of all sets under poisoned device memory; and 2 000 reads against the live reference binary build() leaves in
oracle/_ref in each of the eight mode rows and --fastx_getsubseq, on the bytes of all four files (skipped only where that binary is
absent, as in the sibling files).
"""
import importlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import getseqs_data as gd

pytestmark = pytest.mark.gpu

gs = importlib.import_module("vsearch_amd.getseqs")
needs_cli = pytest.mark.skipif(not os.path.exists(gd.ref_binary()), reason="oracle/_ref/vsearch_ref not built")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ("host_no_context", "host_environment", "host_count", "host_memory", "host_needle_length", "host_header_length", "host_lengths")
CHILD_TIMEOUT = 120
FATAL_STATUS = (134, 139, -6, -11, 124, 137)


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


@pytest.fixture(scope="module")
def host_results():
    """the host restatement of every set, computed once and shared"""
    return {s["name"]: gd.call(None, s) for s in gd.sets()}


def on_device(aligner, s, **kw):
    res = gd.call(aligner, s, **kw)
    st = res.stats
    assert sum(st[r] for r in ROUTES) == 0 and st["headers_host"] == 0 and st["headers_device"] == len(res.matched), (s["name"], st)
    return res


def test_every_set(aligner, host_results):
    for s in gd.sets():
        res = on_device(aligner, s)
        assert res.arrays() == host_results[s["name"]].arrays(), s["name"]
        assert res.stats["probes"] == host_results[s["name"]].stats["probes"] or res.kept, s["name"]     # without a match no route leaves early
        if s["cli"]:
            gd.assert_text_equals_golden(res, s)


@pytest.mark.parametrize("bits", [3, 1])
def test_every_set_with_cut_hashes(aligner, host_results, monkeypatch, bits):
    """eight hash values, then two: every probe walks a chain of false neighbours and is decided by the bytes"""
    monkeypatch.setenv("VSX_GETSEQS_HASH_BITS", str(bits))
    more = 0
    for s in gd.sets():
        res = on_device(aligner, s)
        assert res.arrays() == host_results[s["name"]].arrays(), s["name"]
        more += res.stats["verifications"] > host_results[s["name"]].stats["verifications"]
    assert more > 10


@pytest.mark.parametrize("window", [1, 7])
def test_windows(aligner, host_results, window):
    for name in ("ordinals_alternating", "ordinals_all", "ordinals_none", "word_boundaries", "header_lengths_substr", "subseq_3_10", "folding_labels"):
        s = gd.by_name(name)
        assert on_device(aligner, s, window=window).arrays() == host_results[name].arrays(), name


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
        parts.append(b"W" * gap + labels[k])
        off[k] = seen[labels[k]] = at + gap
        at += gap + len(labels[k])
    return gs.LabelBlob.of(b"".join(parts) + b";A1", off, [len(l) for l in labels])


def test_scattered_shared_and_reversed_spans(aligner, host_results):
    for name in ("word_boundaries", "header_lengths_substr", "list_1000_words", "folding_labels", "field_boundaries", "needle_lengths_exact"):
        s = gd.by_name(name)
        want = host_results[name]
        heads = s["headers"] + s["headers"][:5]                      # repeated headers may share a span
        lens = [len(x) for x in s["seqs"]] + [len(x) for x in s["seqs"][:5]]
        plain = gs.getseqs(aligner, heads, lens, s["mode"], gd.needles_arg(s), **gd.call_kw(s))
        assert plain.arrays()[0][:4 * len(s["headers"])] == want.arrays()[0]
        needles = gd.needles_arg(s) if s["mode"] in gd.SINGLE else scattered(s["needles"], 5)
        moved = gs.getseqs(aligner, scattered(heads, 3), lens, s["mode"], needles, **gd.call_kw(s))
        assert moved.arrays() == plain.arrays() and moved.stats["headers_host"] == 0, name
        back = gs.getseqs(aligner, heads[::-1], lens[::-1], s["mode"], gd.needles_arg(s), **gd.call_kw(s))
        assert np.array_equal(back.matched, plain.matched[::-1]) and np.array_equal(back.length, plain.length[::-1]), name
        assert (back.kept, back.discarded) == (plain.kept, plain.discarded)


def large_inputs(n=20000, seed=11):
    rng = random.Random(seed)
    heads = [b"read%d;sample=S%d;size=%d" % (k, rng.randrange(40), rng.randrange(1, 9)) for k in range(n)]
    return heads, np.full(n, 10, np.uint32)


def test_repeatable_and_after_a_larger_call(aligner, host_results):
    s = gd.by_name("lengths_300_substr")
    a = on_device(aligner, s)
    b = on_device(aligner, s)
    heads, lens = large_inputs()
    big = gs.getseqs(aligner, heads, lens, "label_words", [b"S%d" % k for k in range(0, 40, 3)], field="sample")
    assert big.arrays() == gs.getseqs_host(heads, lens, "label_words", [b"S%d" % k for k in range(0, 40, 3)], field="sample").arrays()
    assert big.stats["headers_device"] == len(heads) and 0 < big.kept < len(heads)
    c = on_device(aligner, s)
    assert a.arrays() == b.arrays() == c.arrays() == host_results[s["name"]].arrays()
    assert (a.stats["probes"], a.stats["verifications"]) == (b.stats["probes"], b.stats["verifications"])


def test_host_routes_and_their_counters(aligner, host_results, monkeypatch):
    s = gd.by_name("positions_words")
    ref, n = host_results[s["name"]], len(s["headers"])

    def routed(counter, al=aligner, headers=None, want=ref):
        res = gd.call(al, s, headers=headers)
        assert {r: res.stats[r] for r in ROUTES} == {r: int(r == counter) for r in ROUTES}, (counter, res.stats)
        assert res.stats["headers_device"] == 0 and res.stats["headers_host"] == res.n
        if want is not None:
            assert res.arrays() == want.arrays()
        return res

    routed("host_no_context", al=None)
    with monkeypatch.context() as m:
        m.setenv("VSX_GETSEQS", "host")
        routed("host_environment")
    with monkeypatch.context() as m:
        m.setenv("VSX_GETSEQS_DEVICE_HEADERS", str(n - 1))
        routed("host_count")
    with monkeypatch.context() as m:
        m.setenv("VSX_GETSEQS_DEVICE_HEADERS", str(n))
        on_device(aligner, s)                                       # at the limit the device still answers
    with monkeypatch.context() as m:
        m.setenv("VSX_GETSEQS_PRETEND_BYTES", str(1 << 50))
        routed("host_memory")
    with monkeypatch.context() as m:
        m.setenv("VSX_GETSEQS_MAX_LENGTHS", "1")
        routed("host_lengths")
    with monkeypatch.context() as m:
        m.setenv("VSX_GETSEQS_MAX_LENGTHS", "2")
        on_device(aligner, s)
    # a header beyond the bound of the occurrence modes; the whole-header modes serve any length
    long = [b"x" * 2047 + b";WXYZW"] + s["headers"][1:]
    lens = [len(x) for x in s["seqs"]]
    res = routed("host_header_length", headers=long, want=None)
    assert res.arrays() == gs.getseqs_host(long, lens, s["mode"], s["needles"]).arrays() and res.matched[0] == 1
    at_bound = [b"x" * 2041 + b";WXYZW"] + s["headers"][1:]
    assert len(at_bound[0]) == 2047 and on_device(aligner, s, headers=at_bound).matched[0] == 1
    exact = gs.getseqs(aligner, long, lens, "labels", [long[1].upper(), b"a1"])
    assert exact.stats["headers_host"] == 0 and list(exact.matched[:2]) == [0, 1]
    assert exact.arrays() == gs.getseqs_host(long, lens, "labels", [long[1].upper(), b"a1"]).arrays()
    # a needle beyond the bound
    needle = b"Q" * 2048
    res = gs.getseqs(aligner, [needle.lower(), b"q"], [3, 3], "labels", [needle, b"zz"])
    assert {r: res.stats[r] for r in ROUTES} == {r: int(r == "host_needle_length") for r in ROUTES} and list(res.matched) == [1, 0]
    res = gs.getseqs(aligner, [needle.lower()[1:], b"q"], [3, 3], "labels", [needle[1:], b"zz"])
    assert res.stats["headers_device"] == 2 and list(res.matched) == [1, 0]
    on_device(aligner, s)


def test_refusals_on_the_device_route(aligner):
    from vsearch_amd import VsxError
    for args, kw in (((["a"], [1], "label_word", b""), {}), ((["a"], [1], "labels", gs.LabelBlob.of(b"ab", [0, 1], [1, 0])), {}),
                     ((["a"], [1], "label", b"a"), dict(subseq_start=2, subseq_end=1)), ((gs.LabelBlob.of(b"abc", [1], [3]), [1], "label", b"a"), {})):
        with pytest.raises(VsxError) as e:
            gs.getseqs(aligner, *args, **kw)
        assert e.value.code == -1
    assert gs.getseqs(aligner, [], [], "labels", [b"x"]).arrays()[4:] == (0, 0)
    assert gs.getseqs(aligner, [b"a", b""], [1, 1], "labels", []).arrays()[4:] == (0, 2)


def test_digest_under_poisoned_memory(aligner):
    """the digest of every set's device result in a child process per poison byte; a child that fails, faults or runs into its time
    limit ends the sequence"""
    want = gd.device_digest(aligner)
    for byte in ("0x00", "0xA5", "0xFF"):
        env = dict(os.environ, VSX_POISON="1", VSX_POISON_BYTE=byte)
        try:
            p = subprocess.run([sys.executable, "-m", "tests.getseqs_data", "--digest"], env=env, cwd=ROOT, capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.fail(f"the child under poison byte {byte} ran into its time limit of {CHILD_TIMEOUT} s; no further child was started")
        text = p.stdout + p.stderr
        assert p.returncode == 0 and p.returncode not in FATAL_STATUS and "illegal memory access" not in text, (byte, p.returncode, text[-2000:])
        lines = [l for l in p.stdout.splitlines() if l.startswith("digest ")]
        assert lines == [f"digest {want} poison {int(byte, 16)}"], (byte, text[-2000:])


# ---- against the live CLI -----------------------------------------------------------------------------------------------------------
def live_reads(seed, n=2000):
    rng = random.Random(seed)
    heads, seqs, quals = [], [], []
    for k in range(n):
        name = rng.choice((b"read%d" % k, b"OTU_%d" % rng.randrange(300), b"otu_%d" % rng.randrange(300)))
        tail = rng.choice((b"", b";sample=S%d" % rng.randrange(30), b";xsample=S%d;tax=k:B,g:G_%d" % (rng.randrange(30), rng.randrange(9)),
                           b";sample=S%dx;size=%d" % (rng.randrange(30), rng.randrange(1, 50)), b"_S%d;sample=s%d;" % (rng.randrange(30), rng.randrange(30))))
        heads.append(b"OTU_7" if k % 97 == 0 else name + tail)
        L = rng.randrange(1, 60)
        seqs.append("".join(rng.choice("ACGT") for _ in range(L)))
        quals.append("".join(chr(rng.randrange(48, 74)) for _ in range(L)))
    return heads, seqs, quals


LIVE = [("label", b"otu_7", False, None, None), ("label", b"otu_1", True, None, None),
        ("labels", [b"OTU_%d" % k for k in range(0, 300, 7)] + [b"otu_5;SAMPLE=s3"], False, None, None),
        ("labels", [b"otu_%d;" % k for k in range(0, 300, 11)] + [b"G_3", b"=s1"], True, None, None),
        ("label_word", b"S7", False, None, None), ("label_word", b"S7", False, "sample", None),
        ("label_words", [b"S%d" % k for k in range(0, 30, 4)] + [b"OTU_12", b"k"], False, None, None),
        ("label_words", [b"S%d" % k for k in range(0, 30, 4)] + [b"s3"], False, "sample", None),
        ("label", b"otu_2", True, None, (5, 20))]


@needs_cli
@pytest.mark.parametrize("row", range(len(LIVE)))
def test_two_thousand_reads_against_the_live_cli(aligner, row):
    mode, needles, substr, field, subseq = LIVE[row]
    heads, seqs, quals = live_reads(100 + row)
    single = mode in gd.SINGLE
    writer = dict(gd.WRITER_DEFAULTS, relabel="r" if row % 3 == 0 else None, sizeout=row % 2 == 1, sizein=True)
    ref = gd.run_cli(heads, seqs, quals, mode, [needles] if single else needles, None, substr, field, subseq, writer,
                     command=("fastx_getsubseq" if subseq else ("fastx_getseq" if row < 2 else "fastx_getseqs")))
    s = dict(headers=heads, seqs=seqs, quals=quals, mode=mode, needles=[needles] if single else needles, substr=substr, field=field, subseq=subseq,
             writer=writer, name="live%d" % row)
    res = gd.call(aligner, s)
    assert res.stats["headers_device"] == len(heads) and 0 < res.kept < len(heads), (res.kept, res.stats)
    got = gd.texts(res, s)
    for name in gd.FILES:
        assert "".join(l + "\n" for l in got[name]).encode("latin-1") == ref[name], (row, name)
    assert got["log"] == ref["log"]
    assert res.arrays() == gd.call(None, s).arrays()
