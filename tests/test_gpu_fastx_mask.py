"""Sequence masking on the device (vsx_fastx_mask, vsearch_amd.mask) against the library's host restatement on records, text and
bits over the sets of tests/fastx_mask_data.py, and the writers against the reference's recorded text; each `want` bit alone; windows
of 1 and 7; scattered and reversed offsets; a call after a larger call and two calls byte for byte; the long route forced on every
set and on seeded sequences, with the route counters asserted; both routes in one call; every host route with its counter; the digest
of all sets under poisoned device memory; 2 000 sequences against the live reference binary build() leaves in oracle/_ref (skipped
only where that binary is absent); one sequence of 200 000 symbols on both routes.
"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import fastx_mask_data as md
from vsearch_amd import mask as mk

pytestmark = pytest.mark.gpu

needs_cli = pytest.mark.skipif(not os.path.exists(md.ref_binary()), reason="oracle/_ref/vsearch_ref not built")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_ROUTES = ("sequences_host_forced", "sequences_host_memory", "sequences_host_long")
CHILD_TIMEOUT = 120
FATAL_STATUS = (134, 139, -6, -11, 124, 137)


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


@pytest.fixture(scope="module")
def sets():
    return md.all_sets()


@pytest.fixture(scope="module")
def host(sets):
    """the host restatement of every set, computed once"""
    return {s["name"]: md.call(None, s) for s in sets}


@pytest.fixture(scope="module")
def island_batch():
    """about 200 seeded sequences of 200 .. 3 000 symbols with low-complexity islands, and their host restatement"""
    s = md._set("islands", md.seeded_sequences(1931, 200, 200, 3000, alphabet="ACGTacgtNU", lower=0.1))
    return s, md.call(None, s)


def on_device(aligner, s, **kw):
    res = md.call(aligner, s, **kw)
    st = res.stats
    assert sum(st[r] for r in HOST_ROUTES) == 0 and st["sequences"] == len(s["seqs"]), st
    return res


def routes(monkeypatch, long_min=None, segment=None, device_bytes=None):
    for name, v in (("VSX_MASK_LONG_MIN", long_min), ("VSX_MASK_SEGMENT", segment), ("VSX_MASK_DEVICE_BYTES", device_bytes)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def test_device_equals_host_on_every_set(aligner, sets, host):
    for s in sets:
        res = on_device(aligner, s)
        md.assert_same(res, host[s["name"]], s["name"])
        assert res.tobytes() == host[s["name"]].tobytes(), s["name"]
        dust = md.full_opts(s["opts"])["qmask"] == "dust"
        assert res.stats["sequences_short" if dust else "sequences_device_plain"] == len(s["seqs"]) and res.stats["sequences_long"] == 0, res.stats
        if "ref" in s:
            md.assert_text_equals_golden(res, s)


@pytest.mark.parametrize("want_text,want_bits", ((True, False), (False, True), (False, False)))
def test_each_want_bit_alone(aligner, sets, host, want_text, want_bits):
    for s in sets:
        res = on_device(aligner, s, want_text=want_text, want_bits=want_bits)
        assert (res.text_blob is None) == (not want_text) and (res.bits_blob is None) == (not want_bits)
        md.assert_same(res, host[s["name"]], (s["name"], want_text, want_bits))


@pytest.mark.parametrize("window", (1, 7))
def test_windows(aligner, sets, host, window):
    for s in sets:
        res = on_device(aligner, s, window=window)
        assert res.stats["windows"] == -(-len(s["seqs"]) // window)
        assert res.tobytes() == host[s["name"]].tobytes(), (s["name"], window)


def test_scattered_and_reversed_offsets(aligner, island_batch):
    s, ref = island_batch
    rng = random.Random(1933)
    blob, off = bytearray(), [0] * len(s["seqs"])
    for k in reversed(range(len(s["seqs"]))):                                # the last sequence first, junk between them
        blob += bytes(rng.choice(b"ACGT#") for _ in range(rng.randrange(0, 9)))
        off[k] = len(blob)
        blob += s["seqs"][k].encode()
    lens = np.array([len(x) for x in s["seqs"]], np.uint32)
    res = mk.fastx_mask(aligner, (bytes(blob), np.array(off, np.uint64), lens))
    assert sum(res.stats[r] for r in HOST_ROUTES) == 0
    assert res.tobytes() == ref.tobytes()


def test_call_after_a_larger_call_and_repeatability(aligner, sets, host, island_batch):
    big, ref = island_batch
    first = on_device(aligner, big)
    assert first.tobytes() == ref.tobytes()
    for s in sets:
        assert on_device(aligner, s).tobytes() == host[s["name"]].tobytes(), s["name"]
    assert on_device(aligner, big).tobytes() == first.tobytes()


def test_long_route_on_every_set_in_child_processes(sets, host):
    """VSX_MASK_LONG_MIN=1 with segments of 64 and 128: the child asserts the route counters and prints one digest per (segment, set)"""
    import hashlib
    env = dict(os.environ, VSX_MASK_LONG_MIN="1")
    try:
        p = subprocess.run([sys.executable, "-m", "tests.fastx_mask_data", "--long", "64,128"], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        pytest.fail(f"the child ran into its time limit of {CHILD_TIMEOUT} s")
    text = p.stdout + p.stderr
    assert p.returncode == 0 and "illegal memory access" not in text, (p.returncode, text[-3000:])
    got = [l.split() for l in p.stdout.splitlines() if l.startswith("long ")]
    want = [["long", str(seg), s["name"], hashlib.sha256(host[s["name"]].tobytes()).hexdigest()] for seg in (64, 128) for s in sets]
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:4]


@pytest.mark.parametrize("segment", (64, 128, 4096))
def test_long_route_on_seeded_sequences(aligner, island_batch, monkeypatch, segment):
    s, ref = island_batch
    routes(monkeypatch, long_min=1, segment=segment)
    res = on_device(aligner, s)
    assert (res.stats["sequences_long"], res.stats["sequences_short"], res.stats["segment"]) == (len(s["seqs"]), 0, segment), res.stats
    assert res.stats["dust_windows"] == sum(len(x) for x in s["seqs"])       # a window at every position
    md.assert_same(res, ref, segment)
    routes(monkeypatch)
    short = on_device(aligner, s)
    assert (short.stats["sequences_long"], short.stats["sequences_short"]) == (0, len(s["seqs"])), short.stats
    assert short.stats["dust_windows"] == ref.stats["dust_windows"]          # the walk visits what the host's loop visits
    assert res.tobytes() == short.tobytes() == ref.tobytes()


def test_both_routes_in_one_call(aligner, island_batch, monkeypatch):
    s, ref = island_batch
    routes(monkeypatch, long_min=1500, segment=256)
    res = on_device(aligner, s, window=64)
    n_long = sum(1 for x in s["seqs"] if len(x) >= 1500)
    assert 0 < n_long < len(s["seqs"])
    assert (res.stats["sequences_long"], res.stats["sequences_short"]) == (n_long, len(s["seqs"]) - n_long), res.stats
    assert res.tobytes() == ref.tobytes()


def test_host_routes_and_their_counters(aligner, island_batch, monkeypatch):
    s, ref = island_batch
    n = len(s["seqs"])
    # VSX_MASK=host with a context
    monkeypatch.setenv("VSX_MASK", "host")
    res = md.call(aligner, s)
    assert [res.stats[r] for r in HOST_ROUTES] == [n, 0, 0] and res.tobytes() == ref.tobytes()
    monkeypatch.delenv("VSX_MASK")
    # no window fits
    routes(monkeypatch, device_bytes=1000)
    res = md.call(aligner, s, window=50)
    assert [res.stats[r] for r in HOST_ROUTES] == [0, n, 0] and res.stats["windows"] == 4 and res.tobytes() == ref.tobytes()
    # the windows fit (one sequence each: at most ~3 000 symbols twice, the bitmaps, the tables), the long route's working set does not
    routes(monkeypatch, long_min=2000, segment=64, device_bytes=16384)
    res = md.call(aligner, s, window=1)
    n_long = sum(1 for x in s["seqs"] if len(x) >= 2000)
    assert n_long > 0 and [res.stats[r] for r in HOST_ROUTES] == [0, 0, n_long], res.stats
    assert res.stats["sequences_short"] == n - n_long and res.stats["sequences_long"] == 0
    assert res.tobytes() == ref.tobytes()


def test_digest_under_poisoned_memory(aligner, sets):
    """the digest of every set's device result in a child process per poison byte; a child that fails, faults or runs into its time
    limit ends the sequence"""
    want = md.device_digest(aligner, sets)
    for byte in (None, "0x00", "0xA5", "0xFF"):
        env = {k: v for k, v in os.environ.items() if k not in ("VSX_POISON", "VSX_POISON_BYTE")}
        if byte is not None:
            env.update(VSX_POISON="1", VSX_POISON_BYTE=byte)
        try:
            p = subprocess.run([sys.executable, "-m", "tests.fastx_mask_data", "--digest"], env=env, cwd=ROOT, capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.fail(f"the child under poison byte {byte} ran into its time limit of {CHILD_TIMEOUT} s; no further child was started")
        text = p.stdout + p.stderr
        assert p.returncode == 0 and p.returncode not in FATAL_STATUS and "illegal memory access" not in text, (byte, p.returncode, text[-2000:])
        lines = [l for l in p.stdout.splitlines() if l.startswith("digest ")]
        assert lines == [f"digest {want} poison {-1 if byte is None else int(byte, 16)}"], (byte, text[-2000:])


# ---- against the live CLI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def live_input():
    seqs = md.seeded_sequences(1937, 2000, 300, 500, alphabet="ACGTacgt", lower=0.25)
    return seqs, [f"q{k}" for k in range(len(seqs))]


@needs_cli
@pytest.mark.parametrize("opts", (dict(qmask="dust"), dict(qmask="dust", hardmask=1), dict(qmask="soft", hardmask=1),
                                  dict(qmask="dust", min_unmasked_pct=55.0, max_unmasked_pct=97.5)),
                         ids=("dust", "dust_hard", "soft_hard", "dust_percent"))
def test_against_the_live_cli(aligner, live_input, opts):
    seqs, labels = live_input
    s = md._set("live", seqs, opts, labels=labels)
    ref = md.run_reference(s)
    res = on_device(aligner, s)
    kw = md.writer_kw(s)
    o = md.full_opts(opts)
    assert "\n".join(mk.fasta_lines(res, labels, **kw)) == "\n".join(ref["fasta"])
    assert "\n".join(mk.maskfasta_lines(res, labels, **kw)) == "\n".join(ref["maskfasta"])
    assert mk.log_lines(res, o["min_unmasked_pct"], o["max_unmasked_pct"]) == ref["log"]
    if "min_unmasked_pct" in opts:
        assert min(res.kept, res.discarded_less, res.discarded_more) > 0


def test_one_long_sequence_on_both_routes(aligner, monkeypatch):
    rng = random.Random(1939)
    s = md._set("long", [md.island_seq(rng, 200000, p_island=0.2)])
    ref = md.call(None, s)
    assert 1000 < int(ref.unmasked[0]) < 199000
    routes(monkeypatch)                                                     # the built-in threshold: the long route
    res = on_device(aligner, s)
    assert (res.stats["sequences_long"], res.stats["sequences_short"], res.stats["dust_windows"]) == (1, 0, 200000), res.stats
    routes(monkeypatch, long_min=1 << 32)
    short = on_device(aligner, s)
    assert (short.stats["sequences_long"], short.stats["sequences_short"]) == (0, 1), short.stats
    assert res.tobytes() == short.tobytes() == ref.tobytes()
    routes(monkeypatch, segment=64)                                         # 3 125 segments
    assert on_device(aligner, s).tobytes() == ref.tobytes()
