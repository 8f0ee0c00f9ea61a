"""Read filtering without a device: the C-ABI surface of include/vsx_filter.h and the host restatement (VSX_FILTER=host)
against recorded answers of the reference CLI and against the plain-Python restatement of tests/fastq_filter_data.py.

tests/golden/fastq_filter_golden.json was produced by `python tests/fastq_filter_data.py tests/golden/fastq_filter_golden.json`
(fastq_filter_data.write_golden): the sets of golden_sets() (edge_reads(), three seeded generate() sets, the FASTA set), the
one-read sets of rounding_reads() and the sets of quality_cases() were written as FASTQ / FASTA and given to the reference's
`--fastq_filter` / `--fastx_filter ... --threads 1`; recorded are the lines of --fastqout, --fastqout_discarded and their _rev
siblings with --fastq_eeout (--fastaout and siblings for the FASTA set), the three totals of the log, and for the quality cases
whether the run ended in the reference's fatal error, with the value and the bound of its message.  Data and expected output only.

Where build() has left the reference binary in oracle/_ref, the sets are also given to it again.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from tests import fastq_filter_data as fd

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fastq_filter_golden.json")
KEYS = ("kept", "discarded", "kept_rev", "discarded_rev", "counts")
needs_cli = pytest.mark.skipif(not os.path.exists(fd.ref_binary()), reason="oracle/_ref/vsearch_ref not built")


@pytest.fixture()
def host_filter(monkeypatch):
    monkeypatch.setenv("VSX_FILTER", "host")
    from vsearch_amd.filter import filter_reads

    def run(s, **extra):
        a, k = fd.call_args(s)
        return filter_reads(None, *a, **dict(k, **extra))
    return run


@pytest.fixture(scope="module")
def golden():
    return fd.load_golden(GOLDEN)


def assert_lines(mine, ref, name):
    for key in KEYS:
        assert mine[key] == ref[key], (name, key)


def assert_equals_py(res, s):
    """records against py_analyse, doubles by bit pattern"""
    py = fd.py_filter(s)
    for recs, side in ((res.records, py["fwd"]), (res.rev_records, py["rev"])):
        assert (recs is None) == (side is None)
        if side is None:
            continue
        for name in ("start", "length", "discarded", "truncated"):
            assert recs[name].tolist() == [int(r[name]) for r in side], (s["name"], name)
        assert recs["ee"].view(np.uint64).tolist() == np.array([r["ee"] for r in side], np.float64).view(np.uint64).tolist(), s["name"]
    assert res.pair_discarded.tolist() == [int(v) for v in py["pair_discarded"]]
    assert res.counts() == py["counts"]
    return py


def test_abi_surface_and_defaults():
    from vsearch_amd import _lib
    lib = _lib.load()
    for name in _lib.FILTER_SYMBOLS:
        assert hasattr(lib, name), name
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "vsx_filter.h")).read()
    declared = set(re.findall(r"\b(vsx_fastx_filter[a-z0-9_]*)\s*\(", hdr))
    assert declared == set(_lib.FILTER_SYMBOLS), declared ^ set(_lib.FILTER_SYMBOLS)
    o = _lib.FilterOpts()
    lib.vsx_fastx_filter_opts_default(C.byref(o))
    # src/vsearch.h
    for name, value in fd.DEFAULTS.items():
        assert getattr(o, name) == value, name
    assert fd.DEFAULTS["maxee"] == sys.float_info.max and o.window == 0
    assert C.sizeof(_lib.FilterRecord) == 24
    from vsearch_amd.filter import RECORD_DTYPE
    assert RECORD_DTYPE.itemsize == 24 and RECORD_DTYPE.fields["ee"][1] == 8 and RECORD_DTYPE.fields["discarded"][1] == 16


# what the reference's check_parameters refuses, and the limit of the quality table's index
REFUSED = [{"truncee_rate": -0.0}, {"truncee_rate": -1.0}, {"minqual": -1}, {"maxee": 0.0}, {"maxee": -1.0}, {"maxee_rate": -0.5},
           {"truncee": -0.1}, {"maxlen": 0}, {"maxns": -1}, {"minlen": 0}, {"trunclen": 0}, {"trunclen": -2}, {"trunclen_keep": 0},
           {"trunclen_keep": -5}, {"truncqual": -1}, {"truncqual": 94}, {"stripleft": -1}, {"stripright": -1},
           {"ascii": 64, "qmax": 64}, {"ascii": 33, "qmin": -34}, {"qmin": 10, "qmax": 9}, {"ascii": 128}]
ACCEPTED = [{"truncee_rate": 0.0}, {"maxee_rate": 0.0}, {"truncee": 0.0}, {"truncqual": 0}, {"truncqual": 93}, {"trunclen": 1},
            {"maxns": 0}, {"ascii": 64, "qmax": 63}, {"minsize": -3}]


@pytest.mark.parametrize("opts", REFUSED, ids=[str(o) for o in REFUSED])
def test_refused_options(host_filter, opts):
    from vsearch_amd import VsxError
    s = fd._set("one", opts, [("r", "ACGT", "IIII")])
    with pytest.raises(VsxError) as ei:
        host_filter(s)
    assert ei.value.code == -1          # VSX_EINVAL


@pytest.mark.parametrize("opts", ACCEPTED, ids=[str(o) for o in ACCEPTED])
def test_accepted_options(host_filter, opts):
    s = fd._set("one", opts, [("r", "ACGT", "IIII" if opts.get("ascii") != 64 else "hhhh")])
    assert_equals_py(host_filter(s), s)


def test_no_context_is_an_error_outside_host_mode(monkeypatch):
    from vsearch_amd import VsxError
    from vsearch_amd.filter import filter_reads
    monkeypatch.delenv("VSX_FILTER", raising=False)
    with pytest.raises(VsxError) as ei:
        filter_reads(None, ["ACGT"], ["IIII"])
    assert ei.value.code == -1


def test_reads_beyond_the_blob(monkeypatch):
    from vsearch_amd import _lib
    monkeypatch.setenv("VSX_FILTER", "host")
    lib = _lib.load()
    o = _lib.FilterOpts()
    lib.vsx_fastx_filter_opts_default(C.byref(o))
    blob = b"ACGTACGT"
    raw = C.cast(C.c_char_p(blob), C.c_void_p)
    for off, ln, ok in ((0, 8, True), (8, 0, True), (4, 4, True), (1, 8, False), (9, 0, False), (2 ** 63, 2, False), (0, 2 ** 31, False),
                        (2 ** 64 - 1, 2, False)):
        offs, lens = np.array([0, off], np.uint64), np.array([4, ln], np.uint32)
        reads = _lib.FilterReads(raw, None, len(blob), offs.ctypes.data, lens.ctypes.data, None)
        out = _lib.FilterOut()
        rc = lib.vsx_fastx_filter(None, C.byref(o), C.c_uint64(2), C.byref(reads), None, C.byref(out))
        assert (rc == 0) == ok, (off, ln, rc)
        if ok:
            lib.vsx_fastx_filter_out_free(C.byref(out))
        else:
            assert rc == -1 and not out.fwd
            # the reverse side is checked too
            zeros, fours = np.zeros(2, np.uint64), np.full(2, 4, np.uint32)
            good = _lib.FilterReads(raw, None, len(blob), zeros.ctypes.data, fours.ctypes.data, None)
            assert lib.vsx_fastx_filter(None, C.byref(o), C.c_uint64(2), C.byref(good), C.byref(reads), C.byref(out)) == -1


def test_golden_host_path(host_filter, golden):
    assert [d["input"]["name"] for d in golden["sets"]] == [s["name"] for s in fd.golden_sets()]
    why, cut = set(), set()
    for d, s in zip(golden["sets"], fd.golden_sets()):
        assert d["input"] == s, s["name"]                    # the generators still give what was recorded
        res = host_filter(s)
        assert_lines(fd.library_lines(res, s), d["expected"], s["name"])
        assert res.stats["reads_host"] == res.stats["reads"] == len(s["seqs"]) * (2 if s.get("rev_seqs") is not None else 1)
        py = assert_equals_py(res, s)
        why |= py["discard_causes"]
        cut |= py["truncation_causes"]
    # coverage is a condition: every cause of a discard and of a truncation occurs in what the reference was given
    assert why == set(fd.DISCARD_CAUSES) and cut == set(fd.TRUNCATION_CAUSES)
    fasta = golden["sets"][-1]
    assert fasta["input"]["quals"] is None and ">fa5" in fasta["expected"]["discarded"]      # stripped to length 0: a header alone
    assert fasta["expected"]["discarded"][fasta["expected"]["discarded"].index(">fa5") + 1].startswith(">")


def test_edge_reads_hold_what_they_promise():
    sets = {s["name"]: s for s in fd.edge_reads()}
    py = {name: fd.py_filter(s) for name, s in sets.items()}
    lengths = lambda name: [r["length"] for r in py[name]["fwd"]]      # noqa: E731
    assert [len(x) for x in sets["lengths"]["seqs"]] == list(fd.EDGE_LENGTHS) == lengths("lengths")
    assert {0, 63, 64, 65, 127, 128, 299} <= set(lengths("truncqual"))
    for name in ("truncee", "truncee_rate"):
        assert {63, 64, 65} <= set(lengths(name)) and py[name]["truncation_causes"] == {name}
    for name in ("stripleft", "stripright"):
        assert [len(x) for x in sets[name]["seqs"]][2:5] == [19, 20, 21] and lengths(name)[2:5] == [0, 0, 1]
    assert lengths("trunclen")[2:5] == lengths("trunclen_keep")[2:5] == [19, 20, 20]
    assert [r["discarded"] for r in py["trunclen"]["fwd"]][2:5] == [True, False, False]
    assert [r["discarded"] for r in py["trunclen_keep"]["fwd"]][2:5] == [False, False, False]
    ns = dict(zip(sets["maxns"]["labels"], py["maxns"]["fwd"]))
    assert [ns[f"ns{c}_{t}"]["discarded"] for c in (1, 2, 3) for t in ("in", "out")] == [False, False, False, False, True, True]
    assert not ns["ns_edges"]["discarded"] and sets["maxns"]["seqs"][-1].upper().count("N") == 4
    mq = dict(zip(sets["minqual"]["labels"], py["minqual"]["fwd"]))
    assert [mq[k]["discarded"] for k in ("mq_before", "mq_at", "mq_after", "mq_none", "mq_no_stop", "mq_63", "mq_chunk2")] == \
        [True, False, False, False, True, True, True]
    assert [r["discard_causes"] for r in py["sizes"]["fwd"]] == [{"minsize"}, set(), set(), {"maxsize"}]
    assert py["pairs"]["pair_discarded"] == [False, True, True, True, False, False, True] and "reverse_only" in py["pairs"]["discard_causes"]


def test_rounding_reads(host_filter, golden):
    """(s + e) - e != s at the stop and maxee between the two: the verdict shows that the add and the subtract are both done"""
    sets = fd.rounding_reads()
    assert [d["input"] for d in golden["rounding"]] == sets
    e = 10.0 ** (-2 / 10.0)
    n_up = n_down = 0
    for d, s in zip(golden["rounding"], sets):
        r = fd.py_analyse(s["seqs"][0], s["quals"][0], s["opts"])
        old_sum = fd.py_analyse(s["seqs"][0][:r["length"]], s["quals"][0][:r["length"]], {})["ee"]
        assert r["truncation_causes"] == {"truncqual"} and r["ee"] == (old_sum + e) - e != old_sum
        assert s["opts"]["maxee"] == min(old_sum, r["ee"])
        kept_by_old_sum = not old_sum > s["opts"]["maxee"]
        assert r["discarded"] != (not kept_by_old_sum)
        n_up += r["discarded"]
        n_down += not r["discarded"]
        assert d["expected"]["counts"]["discarded"] == int(r["discarded"])            # the reference follows its own order
        res = host_filter(s)
        assert_lines(fd.library_lines(res, s), d["expected"], s["name"])
        assert_equals_py(res, s)
    assert n_up >= 8 and n_down >= 8


def test_quality_cases(host_filter, golden):
    from vsearch_amd import VsxError
    cases = fd.quality_cases()
    assert [d["input"] for d in golden["quality"]] == [s for s, _ in cases]
    assert {s["opts"].get("ascii", 33) for s, _ in cases} == {33, 64}
    for d, (s, fatal) in zip(golden["quality"], cases):
        assert (list(fatal) if fatal else None) == d["fatal"], s["name"]              # as the reference did
        if fatal is None:
            assert_lines(fd.library_lines(host_filter(s), s), d["expected"], s["name"])
            continue
        with pytest.raises(fd.QualityError) as pe:
            fd.py_filter(s)
        assert (pe.value.kind, pe.value.value, pe.value.bound) == tuple(fatal)
        with pytest.raises(VsxError, match=rf"FASTQ quality value \({fatal[1]}\) {fatal[0]} \({fatal[2]}\)") as ei:
            host_filter(s)
        assert ei.value.code == -1


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_host_equals_python_restatement(host_filter, seed):
    s = fd.generate(seed, 120, read_len=(60, 150, 300)[seed % 3], paired=seed % 2 == 0)
    assert_equals_py(host_filter(s), s)


def test_window_and_offsets_do_not_matter(host_filter, monkeypatch):
    s = fd.generate(77, 100, read_len=90, paired=True)
    base = host_filter(s)
    for window in (1, 7):
        res = host_filter(s, window=window)
        assert res.records.tobytes() == base.records.tobytes() and res.rev_records.tobytes() == base.rev_records.tobytes()
    recs, rrecs, verdict, counts = fd.scattered_call(None, s, seed=5, window=7)
    assert recs.tobytes() == base.records.tobytes() and rrecs.tobytes() == base.rev_records.tobytes()
    assert verdict.tolist() == base.pair_discarded.tolist() and counts == base.counts()


def test_fasta_width(host_filter):
    s = fd.fasta_set()
    res = host_filter(s)
    assert all(len(x) <= 60 for x in res.fasta_lines(s["labels"], width=60))
    flat = res.fasta_lines(s["labels"], "discarded", width=0)
    assert len(flat) == 2 * res.counts()["discarded"] and "" in flat            # unfolded: a line per read, empty for length 0
    with pytest.raises(ValueError):
        res.fastq_lines(s["labels"])


@needs_cli
def test_live_reference(host_filter):
    """the reference binary asked again: a fresh seeded set per form (single, paired), every edge set and the FASTA set"""
    for s in [fd.generate(900, 300, read_len=120), fd.generate(901, 300, read_len=120, paired=True)] + fd.edge_reads() + [fd.fasta_set()]:
        ref = fd.run_reference(s)
        assert ref["returncode"] == 0, ref["stderr"]
        assert_lines(fd.library_lines(host_filter(s), s), ref, s["name"])
