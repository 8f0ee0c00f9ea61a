"""GPU (-m gpu): --uchime_ref on the device (vsearch_amd.ChimeraSession -> vsx_uchime_ref -> vsx_chimera.hip).  The --uchimeout
lines must equal the reference CLI's byte for byte: the stored golden lines of the api_examples chimera data, and live runs of
oracle/_ref/vsearch_ref (--threads 1) on a seeded family database.  The kernel's records must equal the host restatement's
(VSX_CHIMERA=host, a fresh child process) and must not depend on the window size."""
import json
import os
import random
import subprocess
import sys

import pytest

from oracle import refcli
from tests import common

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = {"none": 0, "soft": 1, "dust": 2}


def _need_ref():
    if not refcli.available():
        pytest.skip("oracle/_ref/vsearch_ref not built")


def _ref_lines(tmp, qnames, qs, tnames, db, extra=()):
    qf, df, uo = os.path.join(tmp, "q.fa"), os.path.join(tmp, "db.fa"), os.path.join(tmp, "u.tsv")
    refcli.write_fasta(qf, qnames, qs)
    refcli.write_fasta(df, tnames, db)
    refcli.run(["--uchime_ref", qf, "--db", df, "--uchimeout", uo, "--threads", "1", "--quiet"] + list(extra))
    return open(uo).read().splitlines()


def _chimera(rng, db, k):
    """a k-parent chimera of random parents with random breakpoints, lightly mutated"""
    ps = rng.sample(range(len(db)), k)
    n = min(len(db[p]) for p in ps)
    cuts = sorted(rng.sample(range(n // 6, n - n // 6), k - 1))
    edges = [0] + cuts + [None]
    return common.mutate(rng, "".join(db[p][edges[i]:edges[i + 1]] for i, p in enumerate(ps)), 0.01)


def _dataset(seed=515, n_q=2000):
    rng = random.Random(seed)
    db, _ = common.family_db(rng, 40, 5, 450, div=0.10)          # 200 parents, 300-600 bp after indels
    db = [d[:rng.randint(300, len(d))] if len(d) > 300 else d for d in db]
    qs = []
    for i in range(n_q):
        r = i % 10
        if r < 3:
            qs.append(_chimera(rng, db, 2))
        elif r < 6:
            qs.append(_chimera(rng, db, 3))
        elif r < 9:
            qs.append(common.mutate(rng, db[rng.randrange(len(db))], 0.03))
        else:
            e = (i // 10) % 6
            qs.append([common.rnd_seq(rng, rng.randint(1, 3)), common.rnd_seq(rng, rng.randint(4, 12)), "N" * rng.randint(40, 300),
                       common.rnd_seq(rng, rng.randint(200, 500)), db[rng.randrange(len(db))],
                       common.mutate(rng, db[rng.randrange(len(db))], 0.05, "ACGTNRY")][e])
    return db, [f"p{i}" for i in range(len(db))], qs, [f"q{i}" for i in range(len(qs))]


@pytest.fixture(scope="module")
def data():
    return _dataset()


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


def test_golden_api_examples(aligner):
    """the reference CLI's --uchimeout lines for the api_examples chimera data, stored in tests/golden/chimera_golden.json"""
    from vsearch_amd import ChimeraSession
    gold = json.load(open(os.path.join(common.GOLD, "chimera_golden.json")))
    ex = common.load_api_examples()
    tn, qn = gold["db_order"], gold["query_order"]
    s = ChimeraSession(aligner, [ex["refs"][n] for n in tn], labels=tn)
    got = s.uchimeout([ex["queries"][n] for n in qn], qn)
    assert got == gold["uchimeout"]
    assert any(line.endswith("\tY") for line in got)


@pytest.mark.parametrize("mask", ["dust", "soft", "none"])
def test_matches_reference_cli(aligner, data, tmp_path, mask):
    _need_ref()
    from vsearch_amd import ChimeraSession
    db, tn, qs, qn = data
    exp = _ref_lines(str(tmp_path), qn, qs, tn, db, ["--dbmask", mask, "--qmask", mask])
    s = ChimeraSession(aligner, db, labels=tn, soft_mask=MASK[mask])
    got = s.uchimeout(qs, qn)
    assert s.stats["queries_kernel"] > 0 and s.stats["queries_host"] == 0, s.stats
    assert len(got) == len(exp)
    bad = [(a, b) for a, b in zip(got, exp) if a != b]
    assert not bad, f"{len(bad)} lines differ, first:\n got {bad[0][0]}\n ref {bad[0][1]}"
    flags = [line.rsplit("\t", 1)[1] for line in exp]
    assert flags.count("Y") > 100 and flags.count("N") > 100


def test_matches_reference_cli_mixed_masks_and_parameters(aligner, data, tmp_path):
    _need_ref()
    from vsearch_amd import ChimeraSession
    db, tn, qs, qn = data
    qs, qn = qs[:800], qn[:800]
    par = dict(minh=0.2, mindiv=1.5, mindiffs=4, xn=6.5, dn=1.1)
    exp = _ref_lines(str(tmp_path), qn, qs, tn, db, ["--dbmask", "dust", "--qmask", "none", "--minh", "0.2", "--mindiv", "1.5",
                                                     "--mindiffs", "4", "--xn", "6.5", "--dn", "1.1"])
    got = ChimeraSession(aligner, db, labels=tn, soft_mask=2, qmask=1, **par).uchimeout(qs, qn)
    assert got == exp


def test_sentinel_route(aligner, tmp_path):
    """a chimera of two ~5 100-bp parents: Q x D > 25e6, the 16-bit aligner refuses the pairs, vsx_lma_align realigns them and the
    host restatement answers"""
    _need_ref()
    from vsearch_amd import ChimeraSession
    rng = random.Random(77)
    db = [common.rnd_seq(rng, 5100), common.rnd_seq(rng, 5120), common.rnd_seq(rng, 600)]
    q = common.mutate(rng, db[0][:2400] + db[1][2400:], 0.01)
    assert len(q) * 5100 > 25_000_000
    tn, qn = ["A", "B", "C"], ["chim"]
    exp = _ref_lines(str(tmp_path), qn, [q], tn, db)
    s = ChimeraSession(aligner, db, labels=tn)
    got = s.uchimeout([q], qn)
    assert got == exp
    assert got[0].endswith("\tY")
    assert s.stats["sentinel_pairs"] >= 2 and s.stats["queries_host"] == 1, s.stats


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_chimera import _dataset
from vsearch_amd import Aligner, ChimeraSession
db, tn, qs, qn = _dataset()
with Aligner(device=0) as al:
    s = ChimeraSession(al, db, labels=tn)
    recs = s.uchime_ref(qs)
    print(json.dumps({"recs": [{k: (v.hex() if isinstance(v, float) else v) for k, v in r.items()} for r in recs], "stats": s.stats}))
"""


def test_kernel_equals_host_restatement(aligner, data):
    from vsearch_amd import ChimeraSession
    db, tn, qs, qn = data
    s = ChimeraSession(aligner, db, labels=tn)
    recs = s.uchime_ref(qs)
    assert s.stats["queries_kernel"] > 1000 and s.stats["queries_host"] == 0
    env = dict(os.environ, VSX_CHIMERA="host")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    child = json.loads(p.stdout.strip().splitlines()[-1])
    assert child["stats"]["queries_kernel"] == 0 and child["stats"]["queries_host"] == s.stats["queries_kernel"]
    mine = [{k: (v.hex() if isinstance(v, float) else v) for k, v in r.items()} for r in recs]
    bad = [k for k, (a, b) in enumerate(zip(mine, child["recs"])) if a != b]
    assert len(mine) == len(child["recs"]) and not bad, (len(bad), mine[bad[0]] if bad else None, child["recs"][bad[0]] if bad else None)


def test_window_size_does_not_matter(aligner, data):
    from vsearch_amd import ChimeraSession
    db, tn, qs, qn = data
    qs = qs[:400]
    a = ChimeraSession(aligner, db, labels=tn).uchime_ref(qs)
    s7 = ChimeraSession(aligner, db, labels=tn, window=7)
    b = s7.uchime_ref(qs)
    assert s7.stats["windows"] == (400 + 6) // 7
    assert a == b
    s5 = ChimeraSession(aligner, db, labels=tn, window=50, search_window=5)     # the part search's own window is separate
    assert s5.uchime_ref(qs) == a and s5.stats["windows"] == 8


def _low_complexity(rng, s):
    """s with a DUST-masked stretch (a short tandem repeat) pasted in: the reference's part search does not DUST the query"""
    unit = rng.choice(["A", "AC", "AGT", "CCG", "TTTA"])
    rep = (unit * 40)[:rng.randint(25, 70)]
    k = rng.randrange(len(s) + 1)
    return s[:k] + rep + s[k:]


@pytest.mark.parametrize("extra", [[], ["--hardmask"], ["--qmask", "soft"]], ids=["dust", "dust_hardmask", "soft_query"])
def test_low_complexity_queries_match_reference_cli(aligner, data, tmp_path, extra):
    """queries with tandem repeats: --qmask dust does not DUST-mask the parts in the reference (search_onequery is called directly,
    chimera.cpp:2023) and --hardmask rewrites only the database; the parts' lower case is masked for the k-mers under dust / soft"""
    _need_ref()
    from vsearch_amd import ChimeraSession
    db, tn, qs, qn = data
    rng = random.Random(404)
    qs = [_low_complexity(rng, q) if len(q) > 40 else q for q in qs[:600]]
    qs = [q.lower() if (i % 7 == 3 and "--qmask" in extra) else q for i, q in enumerate(qs)]
    qn = qn[:600]
    exp = _ref_lines(str(tmp_path), qn, qs, tn, db, extra)
    opts = {"hardmask": 3} if "--hardmask" in extra else ({"qmask": 2} if "--qmask" in extra else {})
    got = ChimeraSession(aligner, db, labels=tn, **opts).uchimeout(qs, qn)
    bad = [(a, b) for a, b in zip(got, exp) if a != b]
    assert len(got) == len(exp) and not bad, f"{len(bad)} lines differ, first:\n got {bad[0][0]}\n ref {bad[0][1]}"


def test_bench_database_matches_reference_cli(aligner, tmp_path):
    """bench_chimera.py's 50 000-sequence family database (ties in k-mer counts, DUST intervals in the queries) and a sample of its
    queries, among them q17836, whose part 0 has a DUST interval"""
    _need_ref()
    from bench_chimera import workload
    from vsearch_amd import ChimeraSession
    db, qs = workload(50_000, 20_000)
    tn = [f"r{i}" for i in range(len(db))]
    idx = sorted(set(list(range(0, 20_000, 67)) + [17836]))
    sq, sn = [qs[i] for i in idx], [f"q{i}" for i in idx]
    exp = _ref_lines(str(tmp_path), sn, sq, tn, db)
    got = ChimeraSession(aligner, db, labels=tn).uchimeout(sq, sn)
    bad = [(a, b) for a, b in zip(got, exp) if a != b]
    assert len(got) == len(exp) and not bad, f"{len(bad)} lines differ, first:\n got {bad[0][0]}\n ref {bad[0][1]}"


def test_piped_part_search_matches_reference_cli(aligner, tmp_path):
    """> 32 768 parts in one window: the part search runs as the pipelined window search"""
    _need_ref()
    from vsearch_amd import ChimeraSession
    db, tn, qs, qn = _dataset(seed=616, n_q=8400)
    exp = _ref_lines(str(tmp_path), qn, qs, tn, db)
    s = ChimeraSession(aligner, db, labels=tn)
    got = s.uchimeout(qs, qn)
    assert s.stats["windows"] == 1 and s.stats["parts"] > 32768, s.stats
    bad = [(a, b) for a, b in zip(got, exp) if a != b]
    assert len(got) == len(exp) and not bad, f"{len(bad)} lines differ, first:\n got {bad[0][0]}\n ref {bad[0][1]}"


def test_refuses_a_searcher_without_detection_parameters(aligner):
    import ctypes as C
    from vsearch_amd import ChimeraSession, VsxError, _lib
    s = ChimeraSession(aligner, ["ACGT" * 50])
    o = _lib.SearchOpts()
    _lib.load().vsx_search_opts_default(C.byref(o))
    o.id = 0.9
    s.close()
    blob = b"ACGT" * 50
    h = C.c_void_p()
    import numpy as np
    off, ln = np.zeros(1, np.uint64), np.array([200], np.uint32)
    _lib.check(_lib.load().vsx_searcher_create(aligner.h, C.byref(h), C.byref(o), 1, C.cast(C.c_char_p(blob), C.c_void_p), len(blob),
                                               off.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p)), "create")
    s.h = h
    with pytest.raises(VsxError) as e:
        s.uchime_ref(["ACGT" * 30])
    assert e.value.code == _lib.VSX_EINVAL
    s.close()


def test_a_query_whose_end_wraps_is_refused(aligner):
    """offset 2^64 - 4 with length 8 "ends" at 4: the spans are checked without adding the two, before any device work"""
    import ctypes as C
    import numpy as np
    from vsearch_amd import ChimeraSession, _lib
    lib = _lib.load()
    s = ChimeraSession(aligner, ["ACGT" * 50])
    blob = b"ACGTTGCAACGGTCAT"
    off, ln = np.array([0, (1 << 64) - 4], np.uint64), np.array([8, 8], np.uint32)
    out = (_lib.ChimeraResult * 2)()
    rc = lib.vsx_uchime_ref(s.h, C.byref(s.opts), C.c_uint64(2), C.cast(C.c_char_p(blob), C.c_void_p), C.c_uint64(len(blob)),
                            off.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p), out)
    assert (rc, lib.vsx_last_error()) == (_lib.VSX_EINVAL, b"vsx_uchime_ref: query exceeds the blob")
    s.close()
