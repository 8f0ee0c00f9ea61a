"""CPU (-m "not gpu"): the C-ABI library loads and exports every symbol include/vsx.h declares, fails
loudly without a device (no CPU fallback), and the host-side logic (sharding, gather) is correct --
including a world_size-2 gloo run of the multi-GPU gather path."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as g
    g.build()
    from vsearch_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "vsx.h")).read()
    declared = set(re.findall(r"\b(vsx_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    hdr2 = open(os.path.join(ROOT, "include", "vsx_search.h")).read()
    declared2 = set(re.findall(r"\b(vsx_[a-z0-9_]+)\s*\(", hdr2))
    assert declared2 == set(_lib.SEARCH_SYMBOLS), declared2 ^ set(_lib.SEARCH_SYMBOLS)
    for s in declared | declared2:
        assert hasattr(lib, s), s
    assert b"gfx950" in lib.vsx_version_string()


def test_no_cpu_fallback():
    """without a gfx950 device the product path must fail loudly, never route through the oracle"""
    from vsearch_amd import _lib, Aligner, VsxError
    if _lib.load().vsx_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(VsxError) as e:
        Aligner()
    assert e.value.code == _lib.VSX_ENODEVICE
    # and nothing under vsearch_amd/ imports the oracle
    for dirpath, _, files in os.walk(os.path.join(ROOT, "vsearch_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "pyoracle" not in src and "nw_oracle" not in src and "liboracle" not in src, f


def test_shard_queries_partition():
    from vsearch_amd.sharding import shard_queries, shard_pairs
    for n in (0, 1, 7, 100, 1001):
        for w in (1, 2, 3, 8):
            blocks = [shard_queries(n, w, r) for r in range(w)]
            assert blocks[0][0] == 0 and blocks[-1][1] == n
            assert all(blocks[i][1] == blocks[i + 1][0] for i in range(w - 1))
            sizes = [b - a for a, b in blocks]
            assert max(sizes) - min(sizes) <= 1
    rng = np.random.default_rng(0)
    qidx = rng.integers(0, 50, 400)
    tidx = rng.integers(0, 99, 400)
    seen = np.zeros(400, int)
    for r in range(4):
        lq, lt, gi, (lo, hi) = shard_pairs(qidx, tidx, 50, 4, r)
        assert np.array_equal(lq + lo, qidx[gi]) and np.array_equal(lt, tidx[gi])
        seen[gi] += 1
    assert (seen == 1).all()


WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
from vsearch_amd.sharding import shard_pairs, gather_hits
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
rng = np.random.default_rng(7)
nq, npairs = 37, 301
qidx = rng.integers(0, nq, npairs); tidx = rng.integers(0, 1000, npairs)
lq, lt, gi, (lo, hi) = shard_pairs(qidx, tidx, nq, world, rank)
# stand-in for the per-rank alignment: a record that is a pure function of the GLOBAL pair (as the aligner's is)
rec = np.zeros((len(gi), 24), np.uint8)
rec[:, 0] = (qidx[gi] * 7 + tidx[gi]) % 251
rec[:, 1] = tidx[gi] % 256
rec[:, 8] = rank + 1
out = gather_hits(torch.from_numpy(rec), torch.from_numpy(gi), npairs, dist)
exp0 = (qidx * 7 + tidx) % 251
assert np.array_equal(out[:, 0].numpy(), exp0.astype(np.uint8)), "record mismatch"
assert np.array_equal(out[:, 1].numpy(), (tidx % 256).astype(np.uint8))
assert (out[:, 8].numpy() >= 1).all(), "some pair was aligned by no rank"
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_gather_world2_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29541", str(script), ROOT]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.count("ok") == 2


WORKER_RUNS = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
from vsearch_amd import sharding
from oracle import pyoracle
from tests import common
import random
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
rng = random.Random(5)
db, fam = common.family_db(rng, 5, 6, 180, div=0.08)
qs, src = common.queries_from_db(rng, db, 23, 90)
qidx = np.repeat(np.arange(len(qs)), 4)
tidx = np.array([rng.randrange(len(db)) for _ in qidx])
orc = pyoracle.Oracle()
rows = [orc.align(qs[q], db[t]) for q, t in zip(qidx, tidx)]            # the single-rank answer for every pair

# this rank's share, as a GPU rank would export it: records + a dense run buffer with rank-LOCAL offsets, in an
# allocation order of its own (the device allocates runs with an atomic cursor: any order)
lq, lt, gi, (lo, hi) = sharding.shard_pairs(qidx, tidx, len(qs), world, rank)
perm = list(range(len(gi))); random.Random(rank).shuffle(perm)
off, chunks = {}, []
at = 0
for k in perm:
    w = sharding.runs_from_cigar(rows[gi[k]][5])
    off[k] = at; at += len(w); chunks.append(w)
runs = np.concatenate(chunks) if chunks else np.zeros(0, np.uint32)
rec = sharding.pack_records([rows[g][0] for g in gi], [rows[g][1] for g in gi], [rows[g][2] for g in gi], [rows[g][3] for g in gi],
                            [rows[g][4] for g in gi], [len(sharding.runs_from_cigar(rows[g][5])) for g in gi], [off[k] for k in range(len(gi))])
rec_all, runs_all, counts = sharding.gather_results(torch.from_numpy(rec), torch.from_numpy(runs.view(np.int32)), dist)
order = np.concatenate([sharding.shard_pairs(qidx, tidx, len(qs), world, r)[2] for r in range(world)])
assert sum(counts) == len(qidx) and sorted(order.tolist()) == list(range(len(qidx)))
d = sharding.decode_records(rec_all)
cig = sharding.cigars_from_gather(rec_all, runs_all)
for j, g in enumerate(order):
    assert (int(d["score"][j]), int(d["aligned"][j]), int(d["matches"][j]), int(d["mismatches"][j]), int(d["gaps"][j]), cig[j]) == tuple(rows[g]), (j, g)
# the production shape: only rank 0 receives
r0, u0, c0 = sharding.gather_results(torch.from_numpy(rec), torch.from_numpy(runs.view(np.int32)), dist, dst=0)
assert c0 == counts
if rank == 0:
    assert torch.equal(r0, rec_all) and torch.equal(u0, runs_all)
else:
    assert r0 is None and u0 is None
# the ASYNCHRONOUS fixed-capacity form (sharding.FixedGather): three steps in flight back to back -- the same payload, a shorter
# one, the same again -- posted before any is collected; every collected step must equal the synchronous gather of that step
for dst in (0, None):
    fg = sharding.FixedGather(dist, dst=dst)
    steps = [(rec, runs), (rec[: len(rec) // 2], runs[: max(0, int(off[len(rec) // 2]) if len(rec) // 2 in off else 0)]), (rec, runs)]
    # (the half step keeps whole records; their run offsets still point inside its own, shorter, run buffer or are unused)
    tickets = []
    for k, (rc_, rn_) in enumerate(steps):
        tickets.append(fg.post(torch.from_numpy(np.ascontiguousarray(rc_)), torch.from_numpy(np.ascontiguousarray(rn_).view(np.int32))))
        if k >= 1:                                   # at most two in flight (two send buffers)
            got = fg.collect(tickets[k - 1])
            exp = sharding.gather_results(torch.from_numpy(np.ascontiguousarray(steps[k - 1][0])), torch.from_numpy(np.ascontiguousarray(steps[k - 1][1]).view(np.int32)), dist, dst=dst)
            if dst is None or rank == dst:
                assert torch.equal(got[0], exp[0]) and torch.equal(got[1], exp[1]) and got[2] == exp[2], (dst, k)
            else:
                assert got == (None, None, None)
    got = fg.collect(tickets[-1])
    if dst is None or rank == dst:
        assert torch.equal(got[0], rec_all) and torch.equal(got[1], runs_all) and got[2] == counts
    # a step beyond the fixed capacity ON ONE RANK ONLY (ADVICE r03: per-rank sizes differ): the decision is collective -- both
    # ranks redo that step through the synchronous gather inside collect(), nobody is left in another collective sequence; a
    # normal step is already in flight behind it, and the steps after it use the grown capacities
    big = (np.concatenate([rec] * 3), np.concatenate([runs] * 3)) if rank == 1 else (rec, runs)
    seq = [big, (rec, runs), big, (rec, runs)]
    tk = []
    for k, (rc_, rn_) in enumerate(seq):
        tk.append(fg.post(torch.from_numpy(np.ascontiguousarray(rc_)), torch.from_numpy(np.ascontiguousarray(rn_).view(np.int32))))
        if k >= 1:
            got = fg.collect(tk[k - 1])
            exp = sharding.gather_results(torch.from_numpy(np.ascontiguousarray(seq[k - 1][0])), torch.from_numpy(np.ascontiguousarray(seq[k - 1][1]).view(np.int32)), dist, dst=dst)
            if dst is None or rank == dst:
                assert torch.equal(got[0], exp[0]) and torch.equal(got[1], exp[1]) and got[2] == exp[2], (dst, k)
            else:
                assert got == (None, None, None)
    got = fg.collect(tk[-1])
    if dst is None or rank == dst:
        assert torch.equal(got[0], rec_all) and torch.equal(got[1], runs_all) and got[2] == counts
    assert fg.sync_steps == 1, fg.sync_steps          # the first big step only: the second one fits the grown buffers
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_gather_records_and_cigar_runs_world2_gloo(tmp_path, oracle):
    """the final gather carries the hit records AND the CIGAR run words; rank-local run offsets are rebased.
    Two gloo ranks hold oracle-made records of their query blocks; every rank must be able to rebuild every pair's
    score, statistics and CIGAR exactly as a single rank reports them."""
    script = tmp_path / "worker_runs.py"
    script.write_text(WORKER_RUNS)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29543", str(script), ROOT]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.count("ok") == 2


WORKER_SEARCH = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
from vsearch_amd import sharding, _lib
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
HIT = np.dtype(_lib.Hit)

class FakeSession:
    # stands in for SearchSession.search_batch_raw (which needs a GPU): hits are a pure function of the query text, laid out
    # exactly as vsx_search_batch lays them out (first[], vsx_hit structs with batch-local query numbers, NUL-terminated CIGARs)
    def search_batch_raw(self, queries, sizes=None, labels=None):
        first, hits, cig = [0], [], b""
        for k, q in enumerate(queries):
            for j in range(len(q) % 4):
                h = np.zeros((), HIT)
                h["query"] = k; h["target"] = (len(q) * 7 + j) % 1000; h["matches"] = len(q) - j; h["id"] = 100.0 - j
                h["accepted"] = 1; h["cigar_off"] = len(cig)
                cig += (f"{len(q) - j}M{j}I" if j else f"{len(q)}M").encode() + b"\0"
                hits.append(h)
            first.append(len(hits))
        return np.array(first, np.uint64), (np.array(hits, HIT) if hits else np.zeros(0, HIT)), cig

qs = ["A" * (5 + (i * 37) % 23) for i in range(45)] + [""]
ss = FakeSession()
exp = ss.search_batch_raw(qs)
for dst in (None, 0):
    got = sharding.sharded_search(ss, qs, dist, dst=dst)
    if dst is not None and rank != dst:
        assert got is None
        continue
    assert np.array_equal(got[0], exp[0]) and got[2] == exp[2]
    assert got[1].tobytes() == exp[1].tobytes()
assert len(exp[1]) > 40
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_sharded_search_gather_world2_gloo(tmp_path):
    """sharding.sharded_search (config 5's form: queries sharded, one gather of vsx_hit structs + counts + CIGAR text): with a
    stand-in for the GPU search, the gathered result must be byte-identical to the single-rank result (query numbers and CIGAR
    offsets rebased).  The real search runs through it in tests/test_gpu_multirank.py."""
    script = tmp_path / "worker_search.py"
    script.write_text(WORKER_SEARCH)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29545", str(script), ROOT]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.count("ok") == 2


def test_host_worker_pool_selftest():
    """the persistent worker pool behind the planner's and the fetch's parallel passes: 40 000 short regions from two host threads
    at once (the shape that let a worker touch a returned caller's stack before the region counter moved under its mutex)"""
    import ctypes as C
    from vsearch_amd import _lib
    lib = _lib.load()
    lib.vsx_internal_pool_selftest.argtypes = [C.c_int, C.c_int]
    lib.vsx_internal_pool_selftest.restype = C.c_int
    assert lib.vsx_internal_pool_selftest(20000, 12) == 0


def test_cigar_from_runs_and_back():
    """vsx_cigar_from_runs (pushop / finishop on the host, no device needed) against the oracle's CIGARs: run words in
    traceback order -> text, count omitted when 1"""
    import random
    from vsearch_amd import cigar_from_runs
    from vsearch_amd.sharding import runs_from_cigar
    assert cigar_from_runs(np.array([(3 << 2) | 0, (1 << 2) | 2, (12 << 2) | 0, (375 << 2) | 1], np.uint32)) == "375I12MD3M"
    assert cigar_from_runs(np.zeros(0, np.uint32)) == ""
    rng = random.Random(4)
    for _ in range(200):
        ops = []
        for _ in range(rng.randint(1, 30)):
            op = rng.choice("MID")
            if not ops or ops[-1][1] != op:
                ops.append((rng.choice([1, 1, 2, 9, 10, 99, 100, 1000, 65535]), op))
        text = "".join((str(n) if n > 1 else "") + o for n, o in ops)
        assert cigar_from_runs(runs_from_cigar(text)) == text


def test_allpairs_row_sharding_partition():
    """config 4 (allpairs, 1 -> 8 GPUs): interleaved rows -- every pair (i < j) belongs to exactly one rank, pair and cell
    counts balance"""
    from vsearch_amd.sharding import shard_allpairs_rows, allpairs_row_cost
    rng = np.random.default_rng(2)
    for n, world in [(2000, 8), (50_000, 8), (1001, 2), (17, 4)]:
        length = rng.integers(350, 450, n)
        owner = np.full(n, -1)
        pairs, cells = [], []
        for r in range(world):
            rows = shard_allpairs_rows(n, world, r)
            assert (owner[rows] == -1).all()
            owner[rows] = r
            pairs.append(allpairs_row_cost(n, rows))
            cells.append(allpairs_row_cost(n, rows, length))
        assert (owner >= 0).all() and sum(pairs) == n * (n - 1) // 2
        if n >= 1000:
            assert max(pairs) - min(pairs) <= 2 * n                   # within two rows of each other
            assert max(cells) / min(cells) < (1.03 if n < 10_000 else 1.005)
    # the explicit pair sets of a small case
    n, world = 17, 4
    seen = set()
    for r in range(world):
        for i in shard_allpairs_rows(n, world, r):
            for j in range(int(i) + 1, n):
                assert (int(i), j) not in seen
                seen.add((int(i), j))
    assert len(seen) == n * (n - 1) // 2


def test_workload_generator_shapes():
    """the synthetic generator of bench.py (device='cpu' here): family structure + query identity"""
    import torch
    from vsearch_amd import workload
    db, off, ln, fam = workload.make_family_db(500, 300, device="cpu")
    assert len(ln) == 500 and abs(float(ln.mean()) - 300) < 5
    q, qo, ql, src = workload.make_queries(db, off, ln, 40, 100, device="cpu")
    assert abs(float(ql.mean()) - 100) < 3
    qi, ti = workload.family_candidates(src, fam, per_query=8)
    assert len(qi) == 320
    assert (fam[ti.astype(int)] == np.repeat(fam[src], 8)).all()
    for k in range(40):
        assert src[k] in ti[8 * k:8 * k + 8]
        assert len(set(ti[8 * k:8 * k + 8])) == 8
    assert set(np.unique(db.numpy())) <= set(b"ACGT")


def _lma(P, nmm, q, t):
    import ctypes as C
    from vsearch_amd import _lib, scoring_from_tuple
    lib = _lib.load()
    s = scoring_from_tuple(P, nmm)
    v = [C.c_int64() for _ in range(5)]
    cg = C.c_void_p()
    rc = lib.vsx_lma_align(C.byref(s), q.encode(), len(q), t.encode(), len(t), *[C.byref(x) for x in v], C.byref(cg))
    assert rc == 0
    out = tuple(x.value for x in v) + (C.string_at(cg).decode(),)
    C.CDLL(None).free(cg)
    return out


def test_lma_fallback_matches_reference_fixtures():
    """host restatement of LinearMemoryAligner (the callers' fallback on the SHRT_MAX sentinel)
    against outputs of the reference's own LMA (tests/golden/lma_golden.json)"""
    import json
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "lma_golden.json")))
    bad = []
    for c in doc["cases"]:
        sc = doc["scorings"][c["scoring"]]
        got = _lma(sc["P"], sc["n_mismatch"], c["q"], c["t"])
        if list(got) != c["exp"]:
            bad.append((c["scoring"], c["q"][:20], c["t"][:20], c["exp"], got))
    assert not bad, bad[:2]
    assert len(doc["cases"]) >= 200


def test_lma_vs_live_reference():
    import random
    from oracle import pyoracle
    from tests import common
    if not pyoracle.have_ref():
        pytest.skip("oracle/_ref not built here")
    rng = random.Random(8)
    for P, nmm in [(pyoracle.DEFAULT_P, False), ((3, -5, 3, 7, 11, 13, 2, 5, 1, 2, 3, 4, 2, 1), True)]:
        ref = pyoracle.Reference(P, nmm)
        for _ in range(250):
            a = common.rnd_seq(rng, rng.randint(0, 200), "ACGTN")
            b = common.mutate(rng, a, 0.2) + common.rnd_seq(rng, rng.randint(0, 40))
            assert tuple(ref.lma(a, b)) == _lma(P, nmm, a, b), (a, b)
        ref.close()


def test_dust_mask_matches_reference_fixture():
    """host DUST (vsx_mask.cpp = what soft_mask=2 applies to queries) against the reference CLI's --fastx_mask --qmask dust
    output (tests/golden/dust_golden.json, made by oracle/gen_golden.py gen_dust)"""
    import json
    from vsearch_amd import dust_mask
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "dust_golden.json")))
    got = [g.decode() for g in dust_mask(doc["in"], threads=4)]
    bad = [(i, doc["in"][i], got[i], doc["exp"][i]) for i in range(len(got)) if got[i] != doc["exp"][i]]
    assert not bad, bad[:1]
    assert sum(1 for e in doc["exp"] if any(c.islower() for c in e)) > 200
    # idempotent, and the empty / shorter-than-a-region sequences come back upper-cased
    assert [g.decode() for g in dust_mask(got)] == got
    assert [g.decode() for g in dust_mask(["", "acg", "aaaaaaa"])] == ["", "ACG", "AAAAAAA"]


def test_soak_harnesses_draw_valid_reference_commands(tmp_path):
    """the randomized soaks (oracle/soak*.py) run on the GPU box; here, without a GPU, their option generators must keep producing
    command lines the reference CLI accepts (a harness that silently stopped exercising the reference would pin nothing)"""
    import random
    import subprocess
    from oracle import refcli, soak, soak_allpairs, soak_cluster, soak_search, pyoracle
    if not refcli.available() or not pyoracle.have_ref():
        pytest.skip("oracle/_ref not built here")
    rng = random.Random(1)
    tmp = str(tmp_path)
    lines = 0
    for _ in range(6):
        o, sc, cli, sizes, use_self = soak_search.draw_options(rng)
        db, qs, tn, qn, ts, qz = soak_search.draw_data(rng, sizes, use_self)
        refcli.write_fasta(tmp + "/db.fa", tn, db)
        refcli.write_fasta(tmp + "/q.fa", qn, qs)
        p = subprocess.run([refcli.REF_BIN, "--usearch_global", tmp + "/q.fa", "--db", tmp + "/db.fa", "--threads", "1", "--userout", tmp + "/u.tsv",
                            "--userfields", "+".join(soak_search.FIELDS), "--quiet"] + cli, capture_output=True, text=True)
        assert p.returncode == 0, (cli, p.stderr[-500:])
        lines += len(open(tmp + "/u.tsv").read().splitlines())
        o, sc, cli, by_size, rs = soak_cluster.draw(rng)
        seqs, names, sz, order = soak_cluster.data(rng, bool(by_size))
        refcli.write_fasta(tmp + "/c.fa", names, seqs)
        command = "--cluster_unoise" if by_size == "unoise" else ("--cluster_size" if by_size else "--cluster_fast")
        p = subprocess.run([refcli.REF_BIN, command, tmp + "/c.fa", "--threads", "1", "--uc", tmp + "/c.uc",
                            "--quiet"] + cli, capture_output=True, text=True)
        assert p.returncode == 0, (cli, p.stderr[-500:])
        o, sc, cli, aa, sizes = soak_allpairs.draw(rng)
        seqs, names, sz = soak_allpairs.data(rng, sizes, bool(o.get("self_")))
        refcli.write_fasta(tmp + "/a.fa", names, seqs)
        p = subprocess.run([refcli.REF_BIN, "--allpairs_global", tmp + "/a.fa", "--qmask", "none", "--threads", "1", "--userout", tmp + "/ua.tsv",
                            "--userfields", "+".join(soak_allpairs.FIELDS), "--quiet"] + cli, capture_output=True, text=True)
        assert p.returncode == 0, (cli, p.stderr[-500:])
        P, nmm, kind = soak.draw_scoring(rng)
        shape, sq, st = soak.draw_population(rng, 4, 3)
        ref = pyoracle.Reference(P, nmm)
        try:
            assert len(ref.search16(sq[0], st[0])) == 3
        finally:
            ref.close()
    assert lines > 100


def test_abundance_ratio_compare_is_exact_beyond_2_53():
    """abundance filters (--minsizeratio / --maxsizeratio, core/searchcore.cpp:480-537): below 2^53 the ROUNDED double product
    decides (historical boundary behaviour), beyond it the comparison is exact on the double's stored value.  Checked against
    Python's exact rationals / its own double arithmetic; no GPU involved."""
    import ctypes as C
    import math
    import random
    from fractions import Fraction
    from vsearch_amd import _lib
    lib = _lib.load()
    rng = random.Random(53)

    def expect(v, ratio, ref):
        if ref <= 0 or ratio <= 0.0:
            return 1 if v > 0 else 0
        if math.isinf(ratio) or math.isnan(ratio):
            return -1
        if v < (1 << 53) and ref < (1 << 53):
            prod = ratio * float(ref)
            return -1 if float(v) < prod else (1 if float(v) > prod else 0)
        d = Fraction(v) - Fraction(ratio) * ref
        return -1 if d < 0 else (1 if d > 0 else 0)

    ratios = [0.0, -1.0, 1.0, 0.5, 2.0, 1 / 9, 1 / 3, 16.0, 1e-300, 5e-324, 1e300, 1.7976931348623157e308, float("inf"), 3.0000000000000004,
              2.0 ** -60, 2.0 ** 60, 2.0 ** -1074, 0.9999999999999999]
    big = [0, 1, 2, 9, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, (1 << 62) + 12345, (1 << 63) - 1, 3 * (1 << 60) + 7, 9 * ((1 << 53) + 1)]
    n = 0
    for ratio in ratios + [rng.uniform(0, 4) for _ in range(200)] + [2.0 ** rng.randint(-80, 80) * rng.uniform(1, 2) for _ in range(200)]:
        for _ in range(40):
            ref = rng.choice(big + [rng.randrange(1, 1 << rng.randint(1, 63)), 0, -3])
            v = rng.choice(big + [rng.randrange(0, 1 << rng.randint(1, 63))])
            if ref > 0 and rng.random() < 0.3 and 0 < ratio < 1e18:
                v = min((1 << 63) - 1, max(0, int(Fraction(ratio) * ref) + rng.randint(-1, 1)))      # straddle the boundary
            assert lib.vsx_abundance_ratio_cmp(v, ratio, ref) == expect(v, ratio, ref), (v, ratio, ref)
            n += 1
    assert n > 15000


def test_api_adapter_falls_back_to_reference_code_without_a_device(tmp_path):
    """a runtime failure of the fast path -- here: no GPU in this process (ROCR_VISIBLE_DEVICES empty) -- must not
    abort the embedding process; the adapter logs it and answers with the reference's own code.  The reference's api example then
    still prints its in-tree golden TSV and passes its own batch == sequential assertion."""
    import subprocess
    from tests import common
    exe = os.path.join(ROOT, "oracle", "_ref", "example_search_vsx")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/example_search_vsx not built here (make -C oracle ref_full ref_api)")
    ex = common.load_api_examples()
    os.makedirs(tmp_path / "data", exist_ok=True)
    with open(tmp_path / "data" / "chimera_ref.fasta", "w") as f:
        f.write("".join(f">{n}\n{s}\n" for n, s in ex["refs"].items()))
    with open(tmp_path / "data" / "chimera_queries.fasta", "w") as f:
        f.write("".join(f">{n}\n{s}\n" for n, s in ex["queries"].items()))
    env = dict(os.environ, VSX_ADAPTER_TRACE="1", ROCR_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "answering with the reference's code" in p.stderr and "search_batch -> reference code (fast path failed)" in p.stderr, p.stderr[-2000:]
    assert "PASS: batch search matches sequential search" in p.stderr
    got = sorted(tuple(l.split("\t")) for l in p.stdout.splitlines())
    assert got == sorted((e["query"], e["target"], e["id"]) for e in ex["expected_search"])


def test_packed_postings_format_counts_every_posting_once():
    """The packed postings of the device k-mer index (vsx_kmer_pack.h: sorted counters as a 16-bit first value + 14 one-byte gaps
    per unit, dummy counters for gaps above 255 and for the tail of a unit).  The encoder is the code the build kernel runs; the
    decoder restates what the count kernel does with a unit (every byte one increment).  Any set of counters must come back as
    exactly one increment each, with everything else landing on dummies."""
    import ctypes as C
    import random
    from vsearch_amd import _lib
    lib = _lib.load()
    enc = lib.vsx_internal_kmer_pack_encode
    enc.restype = C.c_int64
    enc.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    cnt = lib.vsx_internal_kmer_pack_count
    cnt.restype = None
    cnt.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    c_of = lib.vsx_internal_kmer_pack_counter_of
    c_of.restype = C.c_uint32
    c_of.argtypes = [C.c_uint32]
    s_of = lib.vsx_internal_kmer_pack_seq_of
    s_of.restype = C.c_uint32
    s_of.argtypes = [C.c_uint32]

    # the sequence <-> counter map: a bijection of the tile's 32 630 sequences onto the non-dummy counters, neighbours 252 apart
    seen = set()
    for s in range(32630):
        c = c_of(s)
        assert c < 130 * 252 and c % 252 != 251 and s_of(c) == s
        seen.add(c)
    assert len(seen) == 32630
    assert c_of(1) - c_of(0) == 252 and c_of(130) == 1

    real = [c for c in range(130 * 252) if c % 252 != 251]
    rng = random.Random(2024)

    def check(counters):
        counters = sorted(set(counters))
        a = np.array(counters, dtype=np.uint32)
        n_units = enc(a.ctypes.data, len(a), None, 0)
        assert n_units >= (len(a) + 14) // 15 and (n_units > 0) == (len(a) > 0)
        units = np.zeros(4 * max(1, n_units), dtype=np.uint32)
        assert enc(a.ctypes.data, len(a), units.ctypes.data, n_units) == n_units
        hits = np.zeros(32768, dtype=np.uint32)
        cnt(units.ctypes.data, n_units, hits.ctypes.data)
        want = np.zeros(32768, dtype=np.uint32)
        want[a] = 1
        dummies = np.arange(251, 130 * 252, 252)
        got = hits.copy()
        got[dummies] = 0
        assert np.array_equal(got, want), (len(a), n_units)
        assert hits[130 * 252:].sum() == 0
        assert hits.sum() == 15 * n_units                         # every slot of every unit is an increment somewhere
        return n_units

    check([])
    check([0])
    check([32758])
    check([0, 32758])                                             # one posting, 130 hops, one posting
    check([5, 260, 261, 516, 517, 771])                           # gaps of exactly 255, 1, 255, 1, 254
    check([5, 261, 517])                                          # gaps of 256: one hop each
    check(list(range(0, 15)) + [300])                             # a full unit, then a new one
    check(list(range(0, 16)))
    check([c for c in real if c % 252 == 250])                    # the counter next to every dummy
    check(real)                                                   # every sequence of the tile: 32 630 postings
    for density in (1, 3, 15, 16, 40, 487, 5000):
        for _ in range(6):
            check(rng.sample(real, density))
    # clustered: runs of neighbours far apart
    for _ in range(6):
        starts = rng.sample(range(0, len(real) - 60), 9)
        check([real[s + k] for s in starts for k in range(rng.randrange(1, 50))])
    # dense random buckets stay close to 15 postings per unit
    dense = rng.sample(real, 4000)
    assert check(dense) <= 4000 // 15 + 4000 // 40
    # refused inputs: a dummy, unsorted, out of range
    for bad in ([251], [7, 7], [9, 3], [130 * 252]):
        a = np.array(bad, dtype=np.uint32)
        assert enc(a.ctypes.data, len(a), None, 0) == -1


def test_bench_dry_collectives_world2_gloo():
    """bench.py --dry-collectives (VERDICT r03 'next' 8): only the gather path -- the synchronous gather, the asynchronous fixed-capacity
    form and a step that overflows on ONE rank -- launched exactly as the driver launches an N-GPU run, here over gloo without a GPU"""
    import json
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29547", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--dry-collectives"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["dry_collectives"] == {"gather_results_to_rank0": True, "fixed_gather_async_incl_one_rank_overflow": True, "fixed_gather_sync_steps": 1,
                                     "fixed_gather_overlap_samples": True,
                                     # r06: rank 0's samples say "always waited", rank 1's "never"; steps 3 and 6 overflow on one rank each
                                     "fixed_gather_mixed_votes_one_rank_overflows": True, "fixed_gather_degraded_at_step": 5}, d
    assert d["rccl"]["world"] == 2 and d["rccl"]["backend"] == "gloo" and d["rccl"]["device_of_rank"] == [0, 0]


def test_fixed_gather_overlap_accounting_and_degrade():
    """r05 (sharding.FixedGather): every collected step is sampled -- had its collective finished when it was collected, or was it waited
    for -- and a gather whose first `probe` steps ALL had to wait declares itself degraded (the caller then collects right after posting).
    Driven here with a stand-in for torch.distributed whose collectives complete on demand: no process group needed."""
    import torch
    from vsearch_amd import sharding

    class Work:
        def __init__(self, done):
            self.done = done

        def is_completed(self):
            return self.done

        def wait(self):
            self.done = True

    class Dist:
        class ReduceOp:
            MAX = "max"

        def __init__(self, finished):
            self.finished = finished

        def get_world_size(self):
            return 1

        def get_rank(self):
            return 0

        def all_reduce(self, t, op=None, async_op=False):
            return Work(True) if async_op else None

        def gather(self, buf, recv, dst=0, async_op=False):
            if recv is not None:
                recv[0].copy_(buf)
            return Work(self.finished)

    rec = torch.from_numpy(sharding.pack_records([1, 2], [3, 4], [1, 1], [0, 0], [0, 0], [1, 1], [0, 1]))
    runs = torch.tensor([4, 8], dtype=torch.int32)
    for finished, want_degraded in ((False, True), (True, False)):
        fg = sharding.FixedGather(Dist(finished), dst=0)
        for _ in range(4):
            got = fg.collect(fg.post(rec, runs))
            assert torch.equal(got[0], rec) and got[2] == [2]
        st = fg.stats()
        assert st["collects"] == 4 and st["finished_before_collect"] == (4 if finished else 0) and st["waited_for"] == (0 if finished else 4), st
        assert st["degraded_to_sync"] is want_degraded and fg.degraded is want_degraded
        # an immediate collect (degraded use) is not an overlap sample
        fg.collect(fg.post(rec, runs), immediate=True)
        assert fg.stats()["collects"] == 4


def test_bench_dump_outputs_fields_budget_and_sample(tmp_path, monkeypatch):
    """bench.py --dump-outputs: every field of the fetched results as float32 / float64 .npy, exact; past the byte budget a seeded
    sample of the pairs -- the same rows on every call -- that keeps the files within it"""
    import zlib
    import bench
    rng = np.random.default_rng(3)
    n = 5000
    cig = ["%dM%dI%dM" % (a, b, c) for a, b, c in rng.integers(1, 300, (n, 3))]

    class Results:                              # the fields of vsearch_amd.aligner.AlignmentResults that the dump reads
        score = rng.integers(-32768, 32767, n).astype(np.int16)
        aligned, matches, mismatches, gaps = (rng.integers(0, 65535, n).astype(np.uint16) for _ in range(4))
        cigar = cig

        def __len__(self):
            return n
    res = Results()
    info = bench.dump_outputs(str(tmp_path / "all"), res)
    assert info["pairs"] == info["pairs_dumped"] == n
    load = lambda d, k: np.load(str(tmp_path / d / (k + ".npy")))
    for k in ("score", "aligned", "matches", "mismatches", "gaps"):
        assert load("all", k).dtype == np.float32 and np.array_equal(load("all", k), getattr(res, k))
    assert np.array_equal(load("all", "cigar_len"), [len(c) for c in cig])
    assert load("all", "cigar_crc32").dtype == np.float64 and np.array_equal(load("all", "cigar_crc32"), [zlib.crc32(c.encode()) for c in cig])
    assert np.array_equal(load("all", "pair"), np.arange(n))
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 40 * 1000)
    a, b = bench.dump_outputs(str(tmp_path / "a"), res), bench.dump_outputs(str(tmp_path / "b"), res)
    assert a["pairs_dumped"] == b["pairs_dumped"] == 1000
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) - 128 for f in a["files"]) <= 40 * 1000
    pick = load("a", "pair").astype(np.int64)
    assert np.array_equal(pick, load("b", "pair")) and np.all(np.diff(pick) > 0)
    assert np.array_equal(load("a", "score"), res.score[pick]) and np.array_equal(load("a", "cigar_len"), [len(cig[i]) for i in pick])
