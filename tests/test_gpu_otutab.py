"""The OTU table on the device (vsx_otutab, vsearch_amd.otutab) against the library's host restatement on every result array and
against the reference CLI's recorded files, over the sets of tests/otutab_data.py -- with whole hashes, with three bits and with one
bit of them, so that every comparison of neighbours is decided by the bytes; 50 000 labels at scattered, unordered and shared
offsets and in reversed order; two calls byte for byte; every route to the host with its counter; the digest of all sets under
poisoned device memory; and three commands against the live reference binary build() leaves in oracle/_ref (skipped only where that
binary is absent).
"""
import importlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import common
from tests import otutab_data as od

pytestmark = pytest.mark.gpu

ot = importlib.import_module("vsearch_amd.otutab")
needs_cli = pytest.mark.skipif(not os.path.exists(od.ref_binary()), reason="oracle/_ref/vsearch_ref not built")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ("host_no_context", "host_environment", "host_label_count", "host_memory")
CHILD_TIMEOUT = 120
FATAL_STATUS = (134, 139, -6, -11, 124, 137)


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


@pytest.fixture(scope="module")
def golden():
    return od.load_golden()


def on_device(aligner, q, t, q_target, sizes, matched):
    res = ot.otutab(q, t, q_target, sizes=sizes, matched=matched, aligner=aligner)
    st = res.stats
    assert sum(st[r] for r in ROUTES) == 0 and st["labels_host"] == 0, st
    assert st["labels_device"] == len(res.q_sample) + st["targets_in_adds"]
    assert st["query_groups"] >= len(res.samples) and st["target_groups"] >= len(res.otus)
    return res


def assert_device_is_host(aligner, s):
    args = od.inputs(s)
    res = on_device(aligner, *args)
    ref = ot.otutab_host(args[0], args[1], args[2], sizes=args[3], matched=args[4])
    for k, (a, b) in enumerate(zip(res.arrays(), ref.arrays())):
        assert a == b, (s["name"], k)
    if s["ref"] is not None:
        text = od.texts(res, generated_by=od.generated_by(s["ref"]["biom"]))
        assert text["otutabout"] == s["ref"]["otutabout"] and text["mothur"] == s["ref"]["mothur"], s["name"]
        assert od.mask_date(text["biom"]) == od.mask_date(s["ref"]["biom"]), s["name"]
    return res


def test_every_set(aligner, golden):
    assert [s["name"] for s in golden] == [s["name"] for s in od.all_sets()]
    for s in golden:
        res = assert_device_is_host(aligner, s)
        assert res.stats["query_groups"] == len(res.samples) and res.stats["target_groups"] == len(res.otus), s["name"]    # whole hashes: no split


@pytest.mark.parametrize("bits", [3, 1])
def test_every_set_with_cut_hashes(aligner, golden, monkeypatch, bits):
    """eight hash values, then two, for everything: runs of false neighbours, equal names apart from each other inside them"""
    monkeypatch.setenv("VSX_OTUTAB_HASH_BITS", str(bits))
    split = 0
    for s in golden:
        res = assert_device_is_host(aligner, s)
        split += res.stats["query_groups"] - len(res.samples) + res.stats["target_groups"] - len(res.otus)
    assert split > 0                                                  # the host's merge of split groups was needed
    q, t, q_target, sizes, matched = od.large_random_inputs(6000)
    res = on_device(aligner, q, t, q_target, sizes, matched)
    assert res.arrays() == ot.otutab_host(q, t, q_target, sizes=sizes, matched=matched).arrays()


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
        parts.append(b";" * gap + labels[k])
        off[k] = seen[labels[k]] = at + gap
        at += gap + len(labels[k])
    return ot.LabelBlob.of(b"".join(parts) + b";sample=", off, [len(l) for l in labels])


def test_fifty_thousand_labels_scattered_and_reversed(aligner):
    q, t, q_target, sizes, matched = od.large_random_inputs()
    plain = on_device(aligner, q, t, q_target, sizes, matched)
    assert plain.arrays() == ot.otutab_host(q, t, q_target, sizes=sizes, matched=matched, threads=16).arrays()
    assert len(plain.samples) == 40 and plain.t_otu[295] == od.NONE and len(plain.nz_count) > 1000
    moved = on_device(aligner, scattered(q, 223), scattered(t, 227), q_target, sizes, matched)
    assert moved.arrays() == plain.arrays()
    back = on_device(aligner, q[::-1], t, q_target[::-1], sizes[::-1], matched)
    assert back.arrays()[:7] == plain.arrays()[:7] and np.array_equal(back.q_sample, plain.q_sample[::-1]) and np.array_equal(back.t_otu, plain.t_otu)


def test_repeatable(aligner, golden):
    """two calls, and a call after a larger one on the same context (its scratch blocks come back used)"""
    s = next(g for g in golden if g["name"] == "keyword_offsets")
    a = on_device(aligner, *od.inputs(s))
    b = on_device(aligner, *od.inputs(s))
    on_device(aligner, *od.large_random_inputs(20000, seed=229))
    c = on_device(aligner, *od.inputs(s))
    assert a.arrays() == b.arrays() == c.arrays()


def test_host_routes_and_their_counters(aligner, golden, monkeypatch):
    s = next(g for g in golden if g["name"] == "odd_values")
    args = od.inputs(s)
    ref = ot.otutab_host(args[0], args[1], args[2], sizes=args[3], matched=args[4])
    n = len(args[0]) + len(args[1])

    def routed(counter, al=aligner):
        res = ot.otutab(args[0], args[1], args[2], sizes=args[3], matched=args[4], aligner=al)
        assert {r: res.stats[r] for r in ROUTES} == {r: int(r == counter) for r in ROUTES}
        assert res.stats["labels_device"] == 0 and res.stats["labels_host"] == n and res.arrays() == ref.arrays()

    routed("host_no_context", al=None)
    with monkeypatch.context() as m:
        m.setenv("VSX_OTUTAB", "host")
        routed("host_environment")
    with monkeypatch.context() as m:
        m.setenv("VSX_OTUTAB_DEVICE_LABELS", str(n - 1))
        routed("host_label_count")
    with monkeypatch.context() as m:
        m.setenv("VSX_OTUTAB_DEVICE_LABELS", str(n))
        on_device(aligner, *args)                                     # at the limit the device still answers
    with monkeypatch.context() as m:
        m.setenv("VSX_OTUTAB_PRETEND_BYTES", str(1 << 50))
        routed("host_memory")
    on_device(aligner, *args)


def test_refusals_on_the_device_route(aligner):
    from vsearch_amd import VsxError
    with pytest.raises(VsxError) as e:
        ot.otutab(["a"], ["o"], [1], aligner=aligner)
    assert e.value.code == -1
    with pytest.raises(VsxError) as e:
        ot.otutab(ot.LabelBlob.of(b"abc", [1], [3]), ["o"], [0], aligner=aligner)
    assert e.value.code == -1


def test_digest_under_poisoned_memory(aligner, golden):
    """the digest of every set's device result in a child process per poison byte; a child that fails, faults or runs into its time
    limit ends the sequence"""
    want = od.device_digest(aligner)
    for byte in ("0x00", "0xA5", "0xFF"):
        env = dict(os.environ, VSX_POISON="1", VSX_POISON_BYTE=byte)
        try:
            p = subprocess.run([sys.executable, "-m", "tests.otutab_data", "--digest"], env=env, cwd=ROOT, capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.fail(f"the child under poison byte {byte} ran into its time limit of {CHILD_TIMEOUT} s; no further child was started")
        text = p.stdout + p.stderr
        assert p.returncode == 0 and p.returncode not in FATAL_STATUS and "illegal memory access" not in text, (byte, p.returncode, text[-2000:])
        lines = [l for l in p.stdout.splitlines() if l.startswith("digest ")]
        assert lines == [f"digest {want} poison {int(byte, 16)}"], (byte, text[-2000:])


# ---- against the live CLI -----------------------------------------------------------------------------------------------------------
def live_db(rng):
    """150 targets in families of three (2 % apart), one exact duplicate per tenth family; labels with otu= and tax= on a part"""
    db, labels = [], []
    for f in range(50):
        anc = common.rnd_seq(rng, 120)
        for v in range(3):
            db.append(anc if v == 0 else (db[-1] if f % 10 == 0 and v == 2 else common.mutate(rng, anc, 0.02)))
            l = "t%d_%d" % (f, v)
            if f % 3 == 0:
                l += ";otu=fam%d" % (f if v else f // 2)
            if f % 4 == 0:
                l += ";tax=k:K%d,g:G%d_%d;" % (f % 5, f, v)
            labels.append(l)
    return db, labels


def live_queries(rng, db, n, rate):
    qs, labels = [], []
    for k in range(n):
        r = rng.random()
        qs.append(common.rnd_seq(rng, 120) if r < 0.05 else (lambda s: common.mutate(rng, s, rate) if rate else s)(db[min(len(db) - 1, int(rng.paretovariate(0.8)) - 1)]))
        s = rng.randrange(24)
        labels.append(("smp%d.%d" % (s, k) if s % 2 else "r%d;sample=smp%d" % (k, s)) + ";size=%d" % rng.choice((1, 1, 2, 5, 40)))
    return qs, labels


def assert_files(table, ref):
    text = od.texts(table, generated_by=od.generated_by(ref["biom"]))
    assert text["otutabout"] == ref["otutabout"]
    assert text["mothur"] == ref["mothur"]
    assert od.mask_date(text["biom"]) == od.mask_date(ref["biom"])


def cli_search(tmp, command, db, dbl, qs, ql, extra):
    od.write_fasta(os.path.join(tmp, "db.fa"), [od.B(l) for l in dbl], db)
    od.write_fasta(os.path.join(tmp, "q.fa"), [od.B(l) for l in ql], qs)
    return od.run_cli(tmp, ["--" + command, "q.fa", "--db", "db.fa", "--qmask", "none", "--dbmask", "none"] + extra, ["--sizein"])


@needs_cli
def test_search_exact_against_the_live_cli(aligner, tmp_path):
    from vsearch_amd import SearchSession
    rng = random.Random(233)
    db, dbl = live_db(rng)
    qs, ql = live_queries(rng, db, 2000, 0)
    ref = cli_search(str(tmp_path), "search_exact", db, dbl, qs, ql, [])
    sizes = od.sizes_of([od.B(l) for l in ql])
    sess = SearchSession(aligner, db, sizes=od.sizes_of([od.B(l) for l in dbl]), labels=dbl, id=1.0)
    first, hits, _ = sess.search_exact_raw(qs, sizes=sizes, labels=ql)
    sess.close()
    table = ot.from_search(ql, dbl, first, hits, sizes=sizes, aligner=aligner)
    assert sum(table.stats[r] for r in ROUTES) == 0 and np.any(np.diff(first.astype(np.int64)) > 1)          # second hits occur
    assert_files(table, ref)
    assert ot.from_search(ql, dbl, first, hits, sizes=sizes, host=True).arrays() == table.arrays()


@needs_cli
def test_usearch_global_against_the_live_cli(aligner, tmp_path):
    from vsearch_amd import SearchSession
    rng = random.Random(239)
    db, dbl = live_db(rng)
    qs, ql = live_queries(rng, db, 2000, 0.01)
    ref = cli_search(str(tmp_path), "usearch_global", db, dbl, qs, ql, ["--id", "0.9", "--maxaccepts", "2"])
    sizes = od.sizes_of([od.B(l) for l in ql])
    sess = SearchSession(aligner, db, sizes=od.sizes_of([od.B(l) for l in dbl]), labels=dbl, id=0.9, maxaccepts=2)
    first, hits, _ = sess.search_batch_raw(qs, sizes=sizes, labels=ql)
    sess.close()
    table = ot.from_search(ql, dbl, first, hits, sizes=sizes, aligner=aligner)
    assert sum(table.stats[r] for r in ROUTES) == 0 and np.any(np.diff(first.astype(np.int64)) > 1)
    assert_files(table, ref)


@needs_cli
def test_cluster_size_relabel_against_the_live_cli(aligner, tmp_path):
    from vsearch_amd import SearchSession
    rng = random.Random(241)
    seqs = []
    for f in range(100):
        anc = common.rnd_seq(rng, 150)
        seqs += [common.mutate(rng, anc, rng.choice([0.0, 0.005, 0.01])) for _ in range(20)]
    sz = [rng.choice([1, 1, 1, 2, 3, 5, 9, 30, 200]) for _ in seqs]
    names = [("smp%d.%04d" % (i % 7, i) if i % 2 else "s%04d;sample=smp%d" % (i, i % 7)) + ";size=%d" % sz[i] for i in range(len(seqs))]
    tmp = str(tmp_path)
    od.write_fasta(os.path.join(tmp, "c.fa"), [od.B(l) for l in names], seqs)
    ref = od.run_cli(tmp, ["--cluster_size", "c.fa", "--qmask", "none", "--id", "0.97"], ["--sizein", "--relabel", "OTU_"])
    order = sorted(range(len(seqs)), key=lambda i: (-sz[i], names[i], i))                  # Database::sortbyabundance
    sseqs, snames, ssz = [seqs[i] for i in order], [names[i] for i in order], [sz[i] for i in order]
    sess = SearchSession(aligner, sseqs, sizes=ssz, labels=snames, id=0.97)
    cno, per, ncl = sess.cluster_fast()
    sess.close()
    table = ot.from_clusters(snames, cno, per, sizes=ssz, relabel="OTU_", aligner=aligner)
    assert sum(table.stats[r] for r in ROUTES) == 0 and 50 <= ncl < 2000 and len(table.otus) == ncl
    assert_files(table, ref)
