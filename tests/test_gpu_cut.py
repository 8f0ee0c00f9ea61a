"""Restriction-site cutting on the device (vsx_cut, vsearch_amd.cut) against the library's host restatement on every array and on the
text blob over the sets of tests/cut_data.py, and the writers against the reference's recorded files; VSX_CUT_TILE at its smallest
value and at the default (matches whose window straddles a block edge and a tile edge are in the `edges` set); one sequence of
200 000 symbols with blocks of 0, 1 and 64 matches; 5 000 short sequences with windows of 1 and 7, scattered and reversed offsets; a
call after a larger call and two calls byte for byte; each `want` bit alone; every host route with its counter; the digest of all sets
under poisoned device memory; 2 000 sequences against the live reference binary build() leaves in oracle/_ref (skipped only where
that binary is absent).
"""
import importlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import cut_data as cd

ct = importlib.import_module("vsearch_amd.cut")            # (the package exports the function cut under the module's name)

pytestmark = pytest.mark.gpu

needs_cli = pytest.mark.skipif(not os.path.exists(cd.ref_binary()), reason="oracle/_ref/vsearch_ref not built")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 120
FATAL_STATUS = (134, 139, -6, -11, 124, 137)


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


@pytest.fixture(scope="module")
def sets():
    return cd.all_sets()


@pytest.fixture(scope="module")
def host(sets):
    """the host restatement of every set, computed once"""
    return {s["name"]: cd.call(None, s) for s in sets}


@pytest.fixture(scope="module")
def short_batch():
    """5 000 sequences of 0 .. 300 symbols, about one site per 100 symbols, and their host restatement"""
    s = cd._set("short", cd.seeded_set(2121, 5000, 0, 300, "ACGTNacgt", site_rate=0.01))
    return s, cd.call(None, s)


def device_sets(sets):
    return [s for s in sets if len(cd.py_pattern(s["pattern"])[0]) <= 64]


def on_device(aligner, s, **kw):
    res = cd.call(aligner, s, **kw)
    assert [res.stats[r] for r in cd.HOST_ROUTES] == [0] * 5 and res.stats["sequences"] == len(s["seqs"]), res.stats
    return res


@pytest.mark.parametrize("tile", (64, None), ids=("tile64", "tile_default"))
def test_device_equals_host_on_every_set(aligner, sets, host, monkeypatch, tile):
    if tile is None:
        monkeypatch.delenv("VSX_CUT_TILE", raising=False)
    else:
        monkeypatch.setenv("VSX_CUT_TILE", str(tile))
    for s in device_sets(sets):
        res = on_device(aligner, s)
        assert res.stats["tile"] == (tile or 4096)
        blocks = sum((len(x) + 63) // 64 for x in s["seqs"])
        items = sum(-(-((len(x) + 63) // 64) // (res.stats["tile"] // 64)) for x in s["seqs"])
        assert (res.stats["blocks"], res.stats["items"]) == (blocks, items), (s["name"], res.stats)
        cd.assert_same(res, host[s["name"]], s["name"])
        assert res.tobytes() == host[s["name"]].tobytes(), s["name"]
        cd.assert_equals_py(res, s)
        if "ref" in s:
            cd.assert_text_equals_golden(res, s)


def test_one_long_sequence_with_blocks_of_0_1_and_64_matches(aligner, monkeypatch):
    rng = random.Random(2122)
    kinds = ("A" * 64, "C" * 64, "C" * 63 + "A", "CCAC" * 16)
    seq = "".join(rng.choice(kinds) for _ in range(200000 // 64))
    assert len(seq) == 200000
    s = cd._set("long", [seq], "^A_")
    ref = cd.call(None, s)
    per_block = {seq[b:b + 64].count("A") for b in range(0, len(seq), 64)}
    assert per_block == {0, 1, 16, 64} and int(ref.matches[0]) == seq.count("A")
    for tile in ("64", "4096", None):
        if tile is None:
            monkeypatch.delenv("VSX_CUT_TILE", raising=False)
        else:
            monkeypatch.setenv("VSX_CUT_TILE", tile)
        res = on_device(aligner, s)
        assert res.stats["items"] == -(-3125 // (int(tile or 4096) // 64))
        assert res.tobytes() == ref.tobytes(), tile
    monkeypatch.delenv("VSX_CUT_TILE", raising=False)
    # a six-cutter over the same length: sites over block and tile edges, most blocks empty
    sites = sorted(rng.sample(range(0, 200000 - 6, 7), 400)) + [4096 * k - d for k in range(1, 40) for d in (1, 3, 5)]
    s = cd._set("long_sites", [cd.with_sites(200000, sorted(sites))])
    ref = cd.call(None, s)
    assert int(ref.matches[0]) > 400
    assert on_device(aligner, s).tobytes() == ref.tobytes()


@pytest.mark.parametrize("window", (1, 7))
def test_windows(aligner, short_batch, window):
    s, ref = short_batch
    assert on_device(aligner, s, window=window).tobytes() == ref.tobytes()


def test_scattered_and_reversed_offsets(aligner, short_batch):
    s, ref = short_batch
    rng = random.Random(2123)
    blob, off = bytearray(), [0] * len(s["seqs"])
    for k in reversed(range(len(s["seqs"]))):                                # the last sequence first, junk between them
        blob += b"GAATTC"[:rng.randrange(0, 7)]
        off[k] = len(blob)
        blob += s["seqs"][k].encode()
    lens = np.array([len(x) for x in s["seqs"]], np.uint32)
    res = ct.cut(aligner, (bytes(blob), np.array(off, np.uint64), lens), s["pattern"])
    assert [res.stats[r] for r in cd.HOST_ROUTES] == [0] * 5
    assert res.tobytes() == ref.tobytes()


def test_call_after_a_larger_call_and_repeatability(aligner, sets, host, short_batch):
    big, ref = short_batch
    first = on_device(aligner, big)
    assert first.tobytes() == ref.tobytes()
    for s in device_sets(sets):
        assert on_device(aligner, s).tobytes() == host[s["name"]].tobytes(), s["name"]
    assert on_device(aligner, big).tobytes() == first.tobytes()


@pytest.mark.parametrize("bits", (0, 1, 2, 4, 8, 5, 10))
def test_each_want_bit_alone(aligner, sets, host, bits):
    kw = dict(want_fwd=bool(bits & 1), want_rev=bool(bits & 2), want_rev_text=bool(bits & 4), want_discarded_rev_text=bool(bits & 8))
    for s in device_sets(sets):
        res = on_device(aligner, s, **kw)
        assert (res.fwd is None) == (not bits & 1) and (res.rev is None) == (not bits & 6)
        assert (res.rev_off is None) == (not bits & 4) and (res.discarded_off is None) == (not bits & 8) and (res.text_blob is None) == (not bits & 12)
        cd.assert_same(res, host[s["name"]], (s["name"], bits))
        assert res.tobytes() == cd.call(None, s, **kw).tobytes(), (s["name"], bits)


def test_host_routes_and_their_counters(aligner, sets, host, short_batch, monkeypatch):
    s, ref = short_batch

    def routes(res):
        return [res.stats[r] for r in cd.HOST_ROUTES]
    assert routes(ref) == [1, 0, 0, 0, 0]                                    # no context
    monkeypatch.setenv("VSX_CUT", "host")
    res = cd.call(aligner, s)
    assert routes(res) == [0, 1, 0, 0, 0] and res.tobytes() == ref.tobytes()
    monkeypatch.delenv("VSX_CUT")
    monkeypatch.setenv("VSX_CUT_DEVICE_COUNT", str(len(s["seqs"]) + sum(len(x) for x in s["seqs"]) - 1))
    res = cd.call(aligner, s)
    assert routes(res) == [0, 0, 1, 0, 0] and res.tobytes() == ref.tobytes()
    monkeypatch.setenv("VSX_CUT_DEVICE_COUNT", str(len(s["seqs"]) + sum(len(x) for x in s["seqs"])))
    assert routes(cd.call(aligner, s)) == [0] * 5
    monkeypatch.delenv("VSX_CUT_DEVICE_COUNT")
    monkeypatch.setenv("VSX_CUT_PRETEND_BYTES", str(1 << 50))
    res = cd.call(aligner, s)
    assert routes(res) == [0, 0, 0, 1, 0] and res.stats["blocks"] == 0 and res.tobytes() == ref.tobytes()
    monkeypatch.delenv("VSX_CUT_PRETEND_BYTES")
    long_set = next(x for x in sets if x["name"] == "pattern_65")
    res = cd.call(aligner, long_set)
    assert routes(res) == [0, 0, 0, 0, 1] and res.tobytes() == host["pattern_65"].tobytes()
    cd.assert_text_equals_golden(res, long_set)
    assert routes(cd.call(aligner, next(x for x in sets if x["name"] == "pattern_64"))) == [0] * 5


def test_digest_under_poisoned_memory(aligner, sets):
    """the digest of every set's device result in a child process per poison byte; a child that fails, faults or runs into its time
    limit ends the sequence"""
    want = cd.device_digest(aligner, sets)
    for byte in (None, "0x00", "0xA5", "0xFF"):
        env = {k: v for k, v in os.environ.items() if k not in ("VSX_POISON", "VSX_POISON_BYTE")}
        if byte is not None:
            env.update(VSX_POISON="1", VSX_POISON_BYTE=byte)
        try:
            p = subprocess.run([sys.executable, "-m", "tests.cut_data", "--digest"], env=env, cwd=ROOT, capture_output=True, text=True,
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
    rng = random.Random(2124)
    seqs = cd.seeded_set(2125, 2000, 300, 499, "ACGT", site_rate=0.002)      # a planted site in six of ten
    for k in range(0, len(seqs), 9):                                         # some with N and lower case
        x = list(seqs[k])
        for _ in range(6):
            x[rng.randrange(len(x))] = "N"
        seqs[k] = "".join(x[:len(x) // 2]) + "".join(x[len(x) // 2:]).lower()
    return seqs, [f"q{k};size={k % 7 + 1}" for k in range(len(seqs))]


@needs_cli
@pytest.mark.parametrize("pattern", ("G^AATT_C", "GG^_CC", "GCCNNNN^N_GGC"))
def test_against_the_live_cli(aligner, live_input, pattern):
    seqs, labels = live_input
    s = cd._set("live", seqs, pattern, dict(sizeout=1), labels=labels)
    ref = cd.run_cli(s)
    res = on_device(aligner, s)
    cd.assert_text_equals_cli(res, s, ref)
    assert res.cut > 0 and res.uncut_total > 0
