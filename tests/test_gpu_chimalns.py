"""GPU (-m gpu): the --uchimealns kernel (vsx_chimalns.hip) and the calls above it.  The kernel against the host restatement and the
Python restatement on the explicit sets of tests/chimalns_data.py and on random triples; batch shapes, windows, repeatability; every
host route with its counter; the digest under poisoned device memory; the text and the three FASTA files against the stored golden
files and against live runs of the reference CLI (oracle/_ref/vsearch_ref, --threads 1) for --uchime_ref and the three de novo forms."""
import os
import random
import subprocess
import sys

import pytest

from oracle import refcli
from tests import chimalns_data as data
from tests import common

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 120
FATAL_STATUS = (134, 139, -6, -11, 124, 137)
ALL = "Y?N"


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


@pytest.fixture(scope="module")
def explicit():
    return data.explicit_sets()


@pytest.fixture(scope="module")
def ordered_random():
    """random triples with the parents in record order, and py_uchimealns' answers"""
    out = []
    for t in data.random_triples(600, seed=4242):
        if data.py_uchimealns(*t)["reverse"]:
            t = (t[0], t[2], t[1], t[4], t[3])
        out.append(t)
    return out


def _need_ref():
    if not refcli.available():
        pytest.skip("oracle/_ref/vsearch_ref not built")


def _same(got, j, exp):
    assert int(got.alnlen[j]) == exp["alnlen"]
    assert tuple(r.decode("latin-1") for r in got.rows(j)) == exp["rows"]
    assert [tuple(int(x) for x in l) for l in got.lines(j)] == exp["lines"]
    assert int(got.best_i[j]) == exp["best_i"] and float(got.h[j]).hex() == exp["h"].hex()
    assert tuple(int(x) for x in got.counts[j]) == exp["counts"]


# ---- the kernel on explicit triples ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [1, 60, 80, 0])
def test_kernel_equals_host_and_python_on_explicit_sets(aligner, explicit, width):
    from vsearch_amd.chimera import alns_host
    names = [k for k, t in explicit.items() if width != 1 or len(t[0]) <= 1000]
    got = data.device_triples(aligner, [explicit[k] for k in names], width)
    assert got.n == len(names) and got.stats["records_kernel"] == len(names)
    for j, k in enumerate(names):
        host = alns_host(*explicit[k], alignwidth=width)
        assert got.rows(j) == host.rows(0) and (got.lines(j) == host.lines(0)).all(), k
        assert (int(got.best_i[j]), float(got.h[j]).hex(), tuple(got.counts[j])) == (int(host.best_i[0]), float(host.h[0]).hex(), tuple(host.counts[0])), k
        _same(got, j, data.py_uchimealns(*explicit[k], width=width))


def test_kernel_equals_python_on_random_triples(aligner, ordered_random):
    got = data.device_triples(aligner, ordered_random, 60, xn=6.5, dn=1.1)
    assert got.n == len(ordered_random)
    for j, t in enumerate(ordered_random):
        exp = data.py_uchimealns(*t, xn=6.5, dn=1.1, width=60)
        if exp["reverse"]:
            continue                                          # (the order was judged under the default xn / dn)
        _same(got, j, exp)


def test_batch_shapes_and_repeatability(aligner, ordered_random):
    """1 / 63 / 64 / 65 records in one call, a small call after a larger one, and the same bytes twice"""
    whole = data.device_triples(aligner, ordered_random[:200], 80)
    again = data.device_triples(aligner, ordered_random[:200], 80)
    assert whole.arrays() == again.arrays()
    for n in (65, 64, 63, 1):
        part = data.device_triples(aligner, ordered_random[:n], 80)
        assert part.n == n
        for j in range(n):
            assert part.rows(j) == whole.rows(j) and (part.lines(j) == whole.lines(j)).all()
        assert part.h.tobytes() == whole.h[:n].tobytes() and part.counts.tobytes() == whole.counts[:n].tobytes()


def test_kernel_entry_refuses_what_the_kernel_does_not_take(aligner):
    from vsearch_amd import _lib
    with pytest.raises(_lib.VsxError, match="beyond the kernel"):
        data.device_triples(aligner, [data.HOST_ONLY["qlen_4097"]()])
    q, a, b, ca, cb = data.explicit_sets()["plain"]
    with pytest.raises(_lib.VsxError, match="reverse branch"):
        data.device_triples(aligner, [(q, b, a, cb, ca)])


def test_digest_under_poisoned_memory(aligner):
    """the digest of the kernel's arrays in a child process per poison byte; a child that fails, faults or runs into its time limit
    ends the sequence"""
    want = data.device_digest(aligner)
    for byte in ("0x00", "0xA5", "0xFF"):
        env = dict(os.environ, VSX_POISON="1", VSX_POISON_BYTE=byte)
        try:
            p = subprocess.run([sys.executable, "-m", "tests.chimalns_data", "--digest"], env=env, cwd=ROOT, capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.fail(f"the child under poison byte {byte} ran into its time limit of {CHILD_TIMEOUT} s; no further child was started")
        text = p.stdout + p.stderr
        assert p.returncode == 0 and p.returncode not in FATAL_STATUS and "illegal memory access" not in text, (byte, p.returncode, text[-2000:])
        lines = [l for l in p.stdout.splitlines() if l.startswith("digest ")]
        assert lines == [f"digest {want} poison {int(byte, 16)}"], (byte, text[-2000:])


# ---- sessions: device against host, windows, routes --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ref_session(aligner):
    from vsearch_amd import ChimeraSession
    tn, db, qn, qs = data.ref_set(60, 8, 4, 260)
    s = ChimeraSession(aligner, db, labels=tn, minh=4.0)        # (a high --minh: part of the scored records keep the flag 'N')
    return s, qn, qs, s.uchime_ref(qs)


def _forced_host(call):
    os.environ["VSX_CHIMALNS"] = "host"
    try:
        return call()
    finally:
        del os.environ["VSX_CHIMALNS"]


def test_session_device_equals_host_and_windows(ref_session):
    s, qn, qs, recs = ref_session
    dev = s.alns_raw(qs, recs, select=ALL)
    scored = sum(r["status"] == "scored" for r in recs)
    assert dev.n == scored >= 40 and dev.stats["records_kernel"] == scored and dev.stats["records_host"] == 0, dev.stats
    assert {recs[int(k)]["flag"] for k in dev.record} >= {"Y", "N"}
    host = _forced_host(lambda: s.alns_raw(qs, recs, select=ALL))
    assert host.stats["records_host"] == host.stats["host_forced"] == scored and host.stats["records_kernel"] == 0, host.stats
    assert dev.arrays() == host.arrays()
    for window in (1, 7):
        w = s.alns_raw(qs, recs, select=ALL, window=window)
        assert w.arrays() == dev.arrays() and w.stats["windows"] == -(-scored // window)
    only_y = s.alns_raw(qs, recs)
    assert [recs[int(k)]["flag"] for k in only_y.record] == ["Y"] * only_y.n and 0 < only_y.n < scored


def test_tampered_record_is_refused(ref_session):
    from vsearch_amd import _lib
    s, qn, qs, recs = ref_session
    k = next(i for i, r in enumerate(recs) if r["flag"] == "Y")
    bad = [dict(r) for r in recs]
    bad[k]["left_yes"] += 1
    with pytest.raises(_lib.VsxError, match="differs from the record"):
        s.alns_raw(qs, bad)
    bad = [dict(r) for r in recs]
    bad[k]["parent_a"], bad[k]["parent_b"] = bad[k]["parent_b"], bad[k]["parent_a"]
    with pytest.raises(_lib.VsxError, match="record's order"):
        s.alns_raw(qs, bad)


def test_a_query_whose_end_wraps_is_refused(ref_session):
    """the query of a selected record at offset 2^64 - 4 with length 8 "ends" at 4: checked without adding the two, before any
    device work"""
    from vsearch_amd import _lib
    from vsearch_amd.search import _blob
    s, qn, qs, recs = ref_session
    k = next(i for i, r in enumerate(recs) if r["flag"] == "Y")
    blob, off, lens = _blob(qs)
    off, lens = off.copy(), lens.copy()
    off[k], lens[k] = (1 << 64) - 4, 8
    with pytest.raises(_lib.VsxError, match="vsx_chimera_alns: query exceeds the blob") as e:
        s._alns(len(lens), blob, off, lens, recs, 80, "Y", 0, 0)
    assert e.value.code == _lib.VSX_EINVAL


def test_sentinel_route(aligner):
    """a pair the 16-bit aligner refuses (more than 25 000 000 cells): realigned on the host, the record rendered there"""
    from vsearch_amd import ChimeraSession
    rng = random.Random(77)
    db = [common.rnd_seq(rng, 5100), common.rnd_seq(rng, 5120), common.rnd_seq(rng, 600)]
    q = common.mutate(rng, db[0][:2400] + db[1][2400:], 0.01)
    s = ChimeraSession(aligner, db, labels=["A", "B", "C"])
    recs = s.uchime_ref([q])
    assert recs[0]["flag"] == "Y"
    got = s.alns_raw([q], recs)
    assert got.n == 1 and got.stats["sentinel_pairs"] == 2 and got.stats["records_host"] == 1 and got.stats["records_kernel"] == 0, got.stats
    assert got.stats["host_long_query"] == got.stats["host_long_alignment"] == got.stats["host_forced"] == 0


def test_long_alignment_route(aligner):
    """a query the kernel would take whose alignment it does not: parents with a 5 300-symbol tail behind the query's end"""
    from vsearch_amd import ChimeraSession, _lib
    rng = random.Random(78)
    core = [common.rnd_seq(rng, 2900), common.rnd_seq(rng, 2900)]
    db = [core[0] + common.rnd_seq(rng, 5300), core[1] + common.rnd_seq(rng, 5300), common.rnd_seq(rng, 600)]
    q = common.mutate(rng, core[0][:1400] + core[1][1400:], 0.01)
    s = ChimeraSession(aligner, db, labels=["A", "B", "C"])
    recs = s.uchime_ref([q])
    assert recs[0]["status"] == "scored", recs[0]
    got = s.alns_raw([q], recs, select=ALL)
    assert got.n == 1 and int(got.alnlen[0]) > _lib.CHIMALNS_MAX_COLS and len(q) <= 4096
    assert got.stats["host_long_alignment"] == got.stats["records_host"] == 1 and got.stats["sentinel_pairs"] == 0, got.stats


# ---- the stored golden files -----------------------------------------------------------------------------------------------------

def _denovo_session(aligner, s, variant):
    from vsearch_amd import DenovoChimeraSession
    kw = {"abskew": s["abskew"]} if "abskew" in s else {}
    return DenovoChimeraSession(aligner, s["seqs"], s["labels"], variant=variant, **kw)


def _lines(ls):
    return "".join(l + "\n" for l in ls)


@pytest.mark.parametrize("name", ["uchime_ref", "uchime", "uchime2", "uchime3"])
def test_golden_text_and_fasta(aligner, name):
    sets, gold = data.load_golden()
    s, g = sets[name], gold[name]
    kw = dict(fasta_score=True, sizeout=True)
    if name == "uchime_ref":
        from vsearch_amd import ChimeraSession
        ses = ChimeraSession(aligner, s["db"], labels=s["db_labels"])
        recs = ses.uchime_ref(s["seqs"])
        for w in data.WIDTHS:
            assert ses.uchimealns(s["seqs"], s["labels"], records=recs, alignwidth=w) == g["uchimealns"][str(w)], w
        src = (s["seqs"], s["labels"])
    else:
        ses = _denovo_session(aligner, s, name)
        recs = ses.uchime_denovo()
        for w in data.WIDTHS:
            assert ses.uchimealns(alignwidth=w) == g["uchimealns"][str(w)], w
        src = ()
    assert _lines(ses.chimeras_fasta(*src, records=recs, **kw)) == g["chimeras"]
    assert _lines(ses.nonchimeras_fasta(*src, records=recs, **kw)) == g["nonchimeras"]
    assert _lines(ses.borderline_fasta(*src, records=recs, **kw)) == g["borderline"]
    sm = ses.summary(*src, records=recs)
    assert sm["chimeras"] == g["chimeras"].count(">") and sm["nonchimeras"] == g["nonchimeras"].count(">")


# ---- against the live CLI --------------------------------------------------------------------------------------------------------

def test_uchime_ref_matches_live_cli(aligner, tmp_path):
    _need_ref()
    from tests.test_gpu_chimera import _dataset
    from vsearch_amd import ChimeraSession
    db, tn, qs, qn = _dataset()
    s = dict(db_labels=tn, db=db, labels=qn, seqs=qs)
    ses = ChimeraSession(aligner, db, labels=tn)
    recs = ses.uchime_ref(qs)
    for w in (80, 0):
        d = tmp_path / f"w{w}"
        d.mkdir()
        exp = data.run_cli("uchime_ref", s, w, str(d))
        assert exp["uchimealns"].count("\nQuery   (") >= 1000
        got = ses.uchimealns(qs, qn, records=recs, alignwidth=w)
        assert got == exp["uchimealns"], w
    kw = dict(records=recs, fasta_score=True, sizeout=True)
    assert _lines(ses.chimeras_fasta(qs, qn, **kw)) == exp["chimeras"]
    assert _lines(ses.nonchimeras_fasta(qs, qn, **kw)) == exp["nonchimeras"]
    assert _lines(ses.borderline_fasta(qs, qn, **kw)) == exp["borderline"]
    st = ses.alns_raw(qs, recs).stats
    assert st["records_kernel"] >= 1000 and st["records_host"] == 0, st


@pytest.mark.parametrize("variant,abskew", [("uchime", None), ("uchime2", None), ("uchime3", 2.0)])
def test_denovo_matches_live_cli(aligner, tmp_path, variant, abskew):
    """tests/denovo_data.golden_set(): it holds sequences above VSX_CHIMERA_MAX_QLEN with chimeras of them, so the long-query route
    is asserted for uchime.  uchime3 at its default abskew of 16 gives one block; abskew 2 is used and its count asserted from the CLI."""
    _need_ref()
    from tests import denovo_data
    from vsearch_amd import DenovoChimeraSession
    labels, seqs = denovo_data.golden_set()
    s = dict(labels=labels, seqs=seqs)
    kw = {}
    if abskew:
        s["abskew"] = abskew
        kw["abskew"] = abskew
    exp = data.run_cli(variant, s, 80, str(tmp_path))
    assert exp["uchimealns"].count("\nQuery   (") >= 10
    ses = DenovoChimeraSession(aligner, seqs, labels, variant=variant, **kw)
    recs = ses.uchime_denovo()
    assert ses.uchimealns(records=recs) == exp["uchimealns"]
    fk = dict(records=recs, fasta_score=True, sizeout=True)
    assert _lines(ses.chimeras_fasta(**fk)) == exp["chimeras"]
    assert _lines(ses.nonchimeras_fasta(**fk)) == exp["nonchimeras"]
    if variant == "uchime":
        assert _lines(ses.borderline_fasta(**fk)) == exp["borderline"]
        raw = ses.alns_raw(recs)
        assert raw.stats["host_long_query"] >= 1 and raw.stats["records_kernel"] >= 10, raw.stats
        assert int(raw.alnlen.max()) > 4096
