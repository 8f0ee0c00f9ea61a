"""Abundance and length sorting on the device (vsx_sortby, vsearch_amd.sortby) against the library's host restatement and the
plain-Python restatement on the order, n_kept, n_out and the median's bit pattern over the sets of tests/sortby_data.py, and the
writers against the reference's recorded files; again under round caps of 1 and 2 with the host_long_prefix counter; scattered and
reversed header offsets in a blob with gaps; a call after a larger call of another order and two calls byte for byte; every host
route with its counter; the digest of all sets under poisoned device memory; 20 seeded rounds of random options and data; 2 000
records against the live reference binary build() leaves in oracle/_ref (skipped only where that binary is absent); and a
DenovoChimeraSession whose order is sort_by_abundance's.
"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import sortby_data as sd
from vsearch_amd import sortby as sb

pytestmark = pytest.mark.gpu

needs_cli = pytest.mark.skipif(not os.path.exists(sd.ref_binary()), reason="oracle/_ref/vsearch_ref not built")
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
    return sd.all_sets()


@pytest.fixture(scope="module")
def host(sets):
    """the host restatement of every set, computed once"""
    return {s["name"]: sd.call(None, s) for s in sets}


@pytest.fixture(scope="module")
def big():
    """3 000 Illumina-like headers with long shared prefixes, in the three orders, and their host restatement"""
    rng = random.Random(3121)
    labels = sd.illumina(rng, 3000, long_prefix=True)
    seqs = ["A" * rng.randint(200, 215) for _ in labels]
    out = {order: sd._set("big_" + order, labels, order, seqs=seqs) for order in ("size", "length", "length_asc")}
    return {order: (s, sd.call(None, s)) for order, s in out.items()}


def rounds_needed(s):
    """label rounds of the uncapped device route, from py_sortby(): a record is placed by the first chunk in which it differs from
    both neighbours of its numeric tie group, equal records by the round in which they end"""
    e = sd.expected(dict(s, opts=dict(s["opts"], topn=sd.INT64_MAX)))
    need = 0
    order = e["order"]
    for x, y in zip(order, order[1:]):
        if s["sizes"][x] != s["sizes"][y] or (s["order"] != "size" and s["lengths"][x] != s["lengths"][y]):
            continue
        a, b = sd.raw(s["labels"][x]), sd.raw(s["labels"][y])
        k = 0
        while k < min(len(a), len(b)) and a[k] == b[k]:
            k += 1
        need = max(need, k // 8 + 1)                     # the chunk of byte k; for equal labels the chunk with their terminating zero
    return need


def on_device(aligner, s, **kw):
    res = sd.call(aligner, s, **kw)
    assert sd.routes(res)[:4] == [0, 0, 0, 0] and res.stats["items"] == len(s["labels"]), res.stats
    return res


@pytest.mark.parametrize("cap", (None, 1, 2), ids=("cap_default", "cap1", "cap2"))
def test_device_equals_host_on_every_set(aligner, sets, host, monkeypatch, cap):
    if cap is None:
        monkeypatch.delenv("VSX_SORTBY_MAX_ROUNDS", raising=False)
    else:
        monkeypatch.setenv("VSX_SORTBY_MAX_ROUNDS", str(cap))
    capped = []
    for s in sets:
        res = on_device(aligner, s)
        assert res.tobytes() == host[s["name"]].tobytes(), s["name"]
        assert np.float64(res.median).tobytes() == np.float64(host[s["name"]].median).tobytes(), s["name"]
        sd.assert_equals_py(res, s)
        if "ref" in s:
            sd.assert_text_equals_golden(res, s)
        need = rounds_needed(s)
        limit = cap if cap is not None else 32
        assert res.stats["max_rounds"] == limit and res.stats["rounds"] == min(need, limit), (s["name"], need, res.stats)
        assert res.stats["host_long_prefix"] == (1 if need > limit else 0), (s["name"], need, res.stats)
        assert (res.stats["capped_items"] > 1) == (need > limit), (s["name"], res.stats)
        if need > limit:
            capped.append(s["name"])
    assert "long_prefix" in capped
    if cap is not None:
        assert {"deep_beside_flat", "first_diff", "label_lengths", "illumina"} <= set(capped)
    else:                                                                     # (the illumina set shares up to 270 bytes: capped too)
        assert not {"deep_beside_flat", "first_diff", "label_lengths", "prefix_labels"} & set(capped)


def test_rounds_and_active_items(aligner, sets, monkeypatch):
    monkeypatch.delenv("VSX_SORTBY_MAX_ROUNDS", raising=False)
    by_name = {s["name"]: s for s in sets}
    st = on_device(aligner, by_name["deep_beside_flat"]).stats
    # the numeric key leaves both groups open; the 64 equal labels end in round 0, the five deep ones stay for nine rounds
    assert (st["active_numeric"], st["rounds"], st["active"]) == (69, 9, [5] * 8) and st["kept"] == 69
    st = on_device(aligner, by_name["many_groups"]).stats
    assert (st["active_numeric"], st["rounds"], st["active"][0]) == (600, 1, 0)
    st = on_device(aligner, by_name["long_prefix"]).stats
    assert (st["rounds"], st["active"], st["capped_items"], st["host_long_prefix"]) == (32, [64] * 8, 64, 1)
    st = on_device(aligner, by_name["n_1"]).stats
    assert (st["active_numeric"], st["rounds"]) == (0, 0)


def test_scattered_and_reversed_offsets(aligner, big):
    s, ref = big["size"]
    rng = random.Random(3122)
    blob, off = bytearray(b"\0\0\0"), [0] * len(s["labels"])              # junk (NUL included) in front of and between the headers
    for k in reversed(range(len(s["labels"]))):                              # the last header first
        off[k] = len(blob)
        blob += sd.raw(s["labels"][k])
        blob += b"M0\x00234:"[:rng.randrange(0, 8)]
    lens = np.array([len(sd.raw(l)) for l in s["labels"]], np.uint32)
    res = on_device(aligner, s, labels=(bytes(blob), np.array(off, np.uint64), lens))
    assert res.tobytes() == ref.tobytes()
    # the header that ends on the blob's last byte in a deep tie, and one at offset 0
    tail = sd._set("tail", ["M01234:56:000000000-ABCDE:1:1101:7", "x", "M01234:56:000000000-ABCDE:1:1101:5"])
    sd.assert_equals_py(on_device(aligner, tail), tail)


def test_call_after_a_larger_call_and_repeatability(aligner, sets, host, big):
    first = {order: on_device(aligner, s) for order, (s, _) in big.items()}
    for order, (s, ref) in big.items():
        assert first[order].tobytes() == ref.tobytes(), order
        sd.assert_equals_py(first[order], s)
    for s in sets:                                                          # small calls of every order on the blocks the large ones used
        assert on_device(aligner, s).tobytes() == host[s["name"]].tobytes(), s["name"]
    for order, (s, _) in big.items():
        assert on_device(aligner, s).tobytes() == first[order].tobytes(), order


def test_host_routes_and_their_counters(aligner, big, monkeypatch):
    s, ref = big["length"]
    assert sd.routes(ref) == [1, 0, 0, 0, 0]                                 # no context
    monkeypatch.setenv("VSX_SORTBY", "host")
    res = sd.call(aligner, s)
    assert sd.routes(res) == [0, 1, 0, 0, 0] and res.tobytes() == ref.tobytes()
    monkeypatch.delenv("VSX_SORTBY")
    monkeypatch.setenv("VSX_SORTBY_DEVICE_COUNT", str(len(s["labels"]) - 1))
    res = sd.call(aligner, s)
    assert sd.routes(res) == [0, 0, 1, 0, 0] and res.tobytes() == ref.tobytes()
    monkeypatch.setenv("VSX_SORTBY_DEVICE_COUNT", str(len(s["labels"])))
    assert sd.routes(sd.call(aligner, s))[:4] == [0] * 4                     # (the long shared prefixes still meet the round cap)
    monkeypatch.delenv("VSX_SORTBY_DEVICE_COUNT")
    monkeypatch.setenv("VSX_SORTBY_PRETEND_BYTES", str(1 << 50))
    res = sd.call(aligner, s)
    assert sd.routes(res) == [0, 0, 0, 1, 0] and res.stats["rounds"] == 0 and res.tobytes() == ref.tobytes()
    monkeypatch.delenv("VSX_SORTBY_PRETEND_BYTES")
    monkeypatch.setenv("VSX_SORTBY_MAX_ROUNDS", "0")                         # every tie group through the host comparator
    res = sd.call(aligner, s)
    assert sd.routes(res) == [0, 0, 0, 0, 1] and res.stats["rounds"] == 0 and res.tobytes() == ref.tobytes()
    assert res.stats["capped_items"] == res.stats["active_numeric"] > 0


def test_digest_under_poisoned_memory(aligner, sets):
    """the digest of every set's device result, under the default round cap and a cap of one, in a child process per poison byte;
    a child that fails, faults or runs into its time limit ends the sequence"""
    want = sd.py_digest(sets)
    assert sd.device_digest(aligner, sets) == want
    digests = []
    for byte in (None, "0x00", "0xA5", "0xFF"):
        env = {k: v for k, v in os.environ.items() if k not in ("VSX_POISON", "VSX_POISON_BYTE", "VSX_SORTBY_MAX_ROUNDS")}
        if byte is not None:
            env.update(VSX_POISON="1", VSX_POISON_BYTE=byte)
        try:
            p = subprocess.run([sys.executable, "-m", "tests.sortby_data", "--digest"], env=env, cwd=ROOT, capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.fail(f"the child under poison byte {byte} ran into its time limit of {CHILD_TIMEOUT} s; no further child was started")
        text = p.stdout + p.stderr
        assert p.returncode == 0 and p.returncode not in FATAL_STATUS and "illegal memory access" not in text, (byte, p.returncode, text[-2000:])
        lines = [l for l in p.stdout.splitlines() if l.startswith("digest ")]
        poison = -1 if byte is None else int(byte, 16)
        assert lines == [f"digest {want} cap None poison {poison}", f"digest {want} cap 1 poison {poison}"], (byte, text[-2000:])
        digests += [l.split()[1] for l in lines]
    assert digests == [want] * 8


def test_20_seeded_rounds(aligner, monkeypatch):
    rng = random.Random(3123)
    seen = set()
    for case in range(20):
        n = rng.randint(200, 3000)
        labels = sd.illumina(rng, n, singletons=0.6, long_prefix=rng.random() < 0.7)
        for _ in range(n // 50):                                              # duplicates and proper prefixes
            a, b = rng.randrange(n), rng.randrange(n)
            labels[a] = labels[b] if rng.random() < 0.5 else labels[b][:rng.randint(1, len(labels[b]))]
        sizes = [1 if rng.random() < 0.6 else rng.choice((2, 2, 3, 10, 2 ** 31, 2 ** 32 - 1)) for _ in labels]
        seqs = ["A" * rng.choice((250, 250, 251, 253, 1, 50000)) for _ in labels]
        opts = {}
        if rng.random() < 0.4:
            opts["minsize"] = rng.choice((0, 1, 2, 3, 11))
        if rng.random() < 0.4:
            opts["maxsize"] = rng.choice((1, 2, 10, 2 ** 31, 2 ** 32))
        if rng.random() < 0.4:
            opts["topn"] = rng.choice((0, 1, n // 2, n, n + 1))
        s = sd._set(f"seeded{case}", labels, rng.choice(("size", "size", "length", "length_asc")), opts, seqs, sizes)
        cap = rng.choice((None, None, 0, 1, 3, 5))
        if cap is None:
            monkeypatch.delenv("VSX_SORTBY_MAX_ROUNDS", raising=False)
        else:
            monkeypatch.setenv("VSX_SORTBY_MAX_ROUNDS", str(cap))
        res = on_device(aligner, s)
        assert res.tobytes() == sd.call(None, s).tobytes(), (case, s["order"], opts, cap)
        sd.assert_equals_py(res, s)
        seen.add((s["order"], res.stats["host_long_prefix"]))
    assert {o for o, _ in seen} == {"size", "length", "length_asc"} and {c for _, c in seen} == {0, 1}


# ---- against the live CLI -----------------------------------------------------------------------------------------------------------
@needs_cli
@pytest.mark.parametrize("order", ("size", "length"))
def test_against_the_live_cli(aligner, order):
    rng = random.Random(3124)
    labels = sd.illumina(rng, 2000, singletons=0.6, long_prefix=True)
    seqs = ["ACGT" * rng.randint(60, 63) for _ in labels]
    s = sd._set("live", labels, order, dict(sizeout=1, topn=1500, **(dict(minsize=1, maxsize=40) if order == "size" else {})), seqs)
    ref = sd.run_cli(s)
    res = on_device(aligner, s)
    sd.assert_text_equals_cli(res, s, ref)
    assert res.n_out == 1500 and res.stats["rounds"] >= 4


# ---- where the project sorted in Python ---------------------------------------------------------------------------------------------
def test_denovo_chimera_session_order(aligner):
    from tests import common
    from vsearch_amd import DenovoChimeraSession
    from vsearch_amd.chimera import header_size, sort_by_abundance
    rng = random.Random(3125)
    db, _ = common.family_db(rng, 6, 50, 120)
    seqs = db[:300]
    assert len(seqs) == 300
    labels = sd.illumina(rng, len(seqs), singletons=0.6)
    labels[7] = labels[3]                                                     # equal headers keep input order
    sizes = [header_size(l) for l in labels]
    session = DenovoChimeraSession(aligner, seqs, labels)
    try:
        stats = sb.last_stats()
        assert session.order == sort_by_abundance(sizes, labels)
        assert session.labels == [labels[k] for k in session.order] and session.sizes == [sizes[k] for k in session.order]
        assert sd.HOST_ROUTES[0] in stats and [stats[r] for r in sd.HOST_ROUTES] == [0] * 5 and stats["items"] == 300
    finally:
        session.close()
