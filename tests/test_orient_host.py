"""Orientation without a GPU: the library's host restatement (vsx_internal_orient_host) against the plain-Python restatement field for
field on every set, the formatters against the recorded text of the reference CLI (tests/golden/orient_golden.json), the ABI
surface -- and, from py_orient() alone, that every set reaches the edge it is named after.
"""
import os
import re

import pytest

from tests import orient_data as od


@pytest.fixture(scope="module")
def golden():
    return {s["name"]: s for s in od.load_golden()}


_PY = {}


def py_records(s):
    if s["name"] not in _PY:
        _PY[s["name"]] = od.py_orient(s)
    return _PY[s["name"]]


def host_result(s, **extra):
    from vsearch_amd.orient import orient_host
    o = od.full_opts(s["opts"])
    kw = dict(quals=s["quals"], qmask=o["qmask"], wordlength=o["wordlength"], soft_mask=od.MASK_MODES[o["dbmask"]], hardmask=o["hardmask"])
    kw.update(extra)
    return orient_host(s["db"], s["queries"], **kw)


def test_abi_surface_and_defaults():
    import ctypes as C
    from vsearch_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(od.ROOT, "include", "vsx_orient.h")).read()
    declared = set(re.findall(r"\b(vsx_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.ORIENT_SYMBOLS), declared ^ set(_lib.ORIENT_SYMBOLS)
    for name in _lib.ORIENT_SYMBOLS:
        assert hasattr(lib, name), name
    o = _lib.OrientOpts()
    lib.vsx_orient_opts_default(C.byref(o))
    assert (o.qmask, o.want_text, o.window) == (2, 0, 0)                      # --qmask dust is the reference's default
    assert int(re.search(r"#define VSX_ORIENT_MAX_QLEN\s+(\d+)", hdr).group(1)) == _lib.ORIENT_MAX_QLEN == od.MAX_QLEN
    assert _lib.ORIENT_CLASS_QLEN == od.CLASS_QLEN and od.CLASS_QLEN[-1] == od.MAX_QLEN
    internal = open(os.path.join(od.ROOT, "vsearch_amd", "csrc", "vsx_orient_internal.h")).read()
    m = re.search(r"kOrClassQlen\[OR_CLASSES\] = \{(\d+)u, (\d+)u, VSX_ORIENT_MAX_QLEN\}", internal)
    assert (int(m.group(1)), int(m.group(2)), od.MAX_QLEN) == od.CLASS_QLEN                # the kernels' own class limits
    assert od.DEFAULT_OPTS["wordlength"] == 12
    from vsearch_amd.orient import DEFAULT_WORDLENGTH
    assert DEFAULT_WORDLENGTH == 12                                            # cli.cc:4185-4196: this command's own default


def test_golden_inputs_are_the_builders(golden):
    built = {s["name"]: s for s in od.golden_sets()}
    assert set(built) == set(golden)
    for name, s in built.items():
        assert all(golden[name][k] == s[k] for k in od.INPUT_KEYS), name
        assert set(golden[name]) == set(od.INPUT_KEYS) | {"ref"}
        assert set(golden[name]["ref"]) == {"tabbed", "fasta", "fastq", "notmatched", "log"}


def test_python_restatement_equals_reference_counts(golden):
    for s in golden.values():
        lines = [f"{l}\t{r['strand']}\t{r['count_fwd']}\t{r['count_rev']}" for l, r in zip(s["qlabels"], py_records(s))]
        assert lines == s["ref"]["tabbed"], s["name"]


def test_host_equals_python_field_for_field(golden):
    for s in list(golden.values()) + [od.wordlength_15_set()]:
        res, recs = host_result(s), py_records(s)
        assert res.n == len(recs)
        for q, want in enumerate(recs):
            assert res.record(q) == {k: want[k] for k in ("count_fwd", "count_rev", "strand")}, (s["name"], q)
            assert res.text[q].decode("latin-1") == want["text"], (s["name"], q)
            if s["quals"] is not None:
                assert res.qual[q].decode("latin-1") == want["qual"], (s["name"], q)
        assert res.qual is None or s["quals"] is not None
        assert (res.n_fwd, res.n_rev, res.n_none) == tuple(sum(r["strand"] == c for r in recs) for c in "+-?")
        assert res.stats["words_distinct"] == sum(len(r["words"]) for r in recs), s["name"]


def test_formatters_equal_golden_text(golden):
    for s in golden.values():
        od.assert_text_equals_golden(host_result(s), s)


def test_host_routes_are_counted(golden):
    for name, route in (("wordlength_13", "queries_host_wordlength"), ("wordlength_12", "queries_host_forced"), ("wordlength_3", "queries_host_forced")):
        st = host_result(golden[name]).stats
        assert st[route] == len(golden[name]["queries"]), (name, st)
        assert sum(st[k] for k in st if k.startswith("queries_") and k != "queries_class") == len(golden[name]["queries"])
        assert st["queries_device"] == 0 and st["windows"] == 0


def test_without_text_and_thread_counts(golden):
    s = golden["outputs_fastq"]
    full = host_result(s)
    bare = host_result(s, want_text=False)
    assert bare.text is None and bare.qual is None and bare.tobytes() == b"".join(
        v.tobytes() for _, v in sorted(full.fields().items()))
    assert host_result(s, threads=1).tobytes() == host_result(s, threads=5).tobytes() == full.tobytes()


def test_refusals(golden):
    from vsearch_amd import VsxError
    from vsearch_amd.orient import orient_host
    s = golden["wordlength_8"]
    with pytest.raises(VsxError):
        orient_host(s["db"], s["queries"], wordlength=2)
    with pytest.raises(VsxError):
        orient_host(s["db"], s["queries"], wordlength=16)
    with pytest.raises(VsxError):
        orient_host(s["db"], s["queries"], wordlength=8, qmask=3)
    with pytest.raises(ValueError):
        orient_host(s["db"], s["queries"], quals=["I"] * len(s["queries"]), wordlength=8)
    # overlapping queries cannot both be written back at their own offsets
    blob = s["queries"][0].encode()
    with pytest.raises(VsxError):
        orient_host(s["db"], (blob, [0, 4], [20, 20]), wordlength=8)
    res = orient_host(s["db"], (blob, [0, 4], [20, 20]), wordlength=8, want_text=False)
    assert res.n == 2


# ---- every set reaches the edge it is named after: from py_orient() alone ----------------------------------------------------------
def pairs(recs):
    return [(r["count_fwd"], r["count_rev"]) for r in recs]


def test_ratio_set_reaches_its_edges(golden):
    recs = py_records(golden["ratio_edges"])
    assert [(w[0][1], w[0][2]) for w in (r["words"] for r in recs)] == list(od.RATIO_EDGES)
    assert all(len(r["words"]) == 1 for r in recs)
    # 8 : 1 and 16 : 2 are not "more than eight times"; 9 : 1 and 17 : 2 are
    assert pairs(recs) == [(0, 0), (1, 0), (0, 0), (0, 1), (0, 0), (1, 0), (1, 0), (0, 1), (0, 0)]


def test_verdict_set_reaches_its_edges(golden):
    recs = py_records(golden["verdict_edges"])
    assert pairs(recs) == list(od.VERDICT_EDGES)
    assert "".join(r["strand"] for r in recs) == "?+-?+?-?+?"


def test_palindrome_repeat_and_length_sets_reach_their_edges(golden):
    recs = py_records(golden["palindromes"])
    word, hf, hr = recs[0]["words"][0]
    assert word == od.revcomp(word) and hf == hr == 3 and pairs(recs) == [(0, 0), (1, 0), (0, 0)]
    s = golden["repeats"]
    recs = py_records(s)
    a, b, c = (r["words"][0] for r in recs[:3])
    assert s["queries"][0].count(a[0]) == 3 and len(recs[0]["words"]) == 1 and pairs(recs)[0] == (1, 0)
    assert sum(t.count(b[0]) for t in s["db"]) == 9 and b[1:] == (8, 1) and pairs(recs)[1] == (0, 0)        # twice in one sequence: once
    assert c[1:] == (9, 1) and pairs(recs)[2] == (1, 0)
    assert pairs(recs)[3] == (2, 0)
    s = golden["query_lengths"]
    w = od.full_opts(s["opts"])["wordlength"]
    assert [len(q) for q in s["queries"]] == [w - 1, w, w + 1, w + 1, 0]
    assert [len(r["words"]) for r in py_records(s)] == [0, 1, 2, 2, 0]
    # the reference accepts an empty read: it has no words, is not oriented, and is written to --notmatched as an empty record
    assert s["ref"]["tabbed"][4] == "q4\t?\t0\t0" and s["ref"]["notmatched"][-1] == ">q4"


def test_alphabet_sets_reach_their_edges(golden):
    none, soft, dust = (py_records(golden[f"alphabet_qmask_{m}"]) for m in ("none", "soft", "dust"))
    qs = golden["alphabet_qmask_none"]["queries"]
    assert "U" in qs[1] and "u" in qs[2] and qs[3].islower() and qs[5] == "A" * 48
    assert pairs(none)[:8] == [(1, 0)] * 7 + [(2, 0)]
    assert pairs(soft)[:8] == pairs(dust)[:8] == [(1, 0), (1, 0), (0, 0), (0, 0), (0, 0), (1, 0), (0, 0), (2, 0)]
    # the low-complexity read is one DUST masks whole -- and its word still counts under --qmask dust
    from vsearch_amd import dust_mask
    assert dust_mask([qs[5]])[0].islower() and pairs(dust)[5] == (1, 0)
    assert {q[len(qs[0]) // 2] for q in qs[8:]} == set(od.AMBIGUOUS + od.AMBIGUOUS.lower())
    for recs in (none, soft, dust):
        assert all(p == (0, 0) and not r["words"] for p, r in zip(pairs(recs)[8:], recs[8:]))


def test_dbmask_sets_differ_as_built(golden):
    got = {m: pairs(py_records(golden[f"dbmask_{m}"])) for m in ("none", "soft", "dust", "soft_hardmask", "dust_hardmask")}
    assert got["none"][0] == (1, 0) and got["soft"][0] == (0, 0) and got["dust"][0] == (1, 0)        # the lower-case marker; DUST folds the case
    assert got["none"][2][0] > 0 and got["soft"][2][0] > 0 and got["dust"][2] == (0, 0)             # the low-complexity run
    assert got["soft_hardmask"] == got["soft"]
    assert got["dust_hardmask"][0] == (0, 0)                                                        # ... but not with --hardmask


def test_golden_sets_give_every_verdict(golden):
    seen = {name: {r["strand"] for r in py_records(s)} for name, s in golden.items()}
    assert set().union(*seen.values()) == {"+", "-", "?"}
    for w in (8, 9, 12, 13):
        assert seen[f"wordlength_{w}"] == {"+", "-", "?"}
    assert {r["strand"] for r in py_records(od.wordlength_15_set())} == {"+", "-", "?"}
    out = golden["outputs_fastq"]["ref"]
    assert out["fasta"] and out["fastq"] and out["notmatched"] and golden["outputs_no_queries"]["ref"]["log"][0] == "Forward oriented sequences: 0"
