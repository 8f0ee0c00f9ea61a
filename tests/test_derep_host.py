"""Dereplication without a GPU: the library's host restatement (vsx_derep without a context, as under VSX_DEREP=host) against
the plain-Python restatement (tests/derep_data.py: py_derep) field for field, and the package's formatters against the
recorded text of the reference CLI (tests/golden/derep_golden.json, written by `python -m tests.derep_data`) byte for byte.
Also: the quality kernel's threshold table against math.log10, and the calls the library refuses.
"""
import math
import struct

import numpy as np
import pytest

from tests import derep_data as dd


@pytest.fixture(scope="module")
def golden():
    return dd.load_golden()


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def host(s, **extra):
    res = dd.call(None, s, **extra)
    assert res.stats["reads_host"] == res.counts["kept"] and res.stats["windows"] == 0
    return res


def test_golden_inputs_are_the_builders(golden):
    """the recorded inputs are what the builders build today"""
    built = dd.golden_sets()
    assert [g["name"] for g in golden] == [s["name"] for s in built]
    for g, s in zip(golden, built):
        assert {k: g[k] for k in dd.INPUT_KEYS} == {k: s[k] for k in dd.INPUT_KEYS}, s["name"]


def test_host_equals_python_equals_golden(golden):
    for s in golden:
        res = host(s)
        assert dd.result_fields(res) == dd.py_derep(s), s["name"]
        text = dd.formatted(res, s)
        assert set(text) == set(s["ref"]), s["name"]
        for key in text:
            assert text[key] == s["ref"][key], (s["name"], key)


def test_environment_route(golden, monkeypatch):
    """VSX_DEREP=host sends a call through the restatement whatever the context"""
    monkeypatch.setenv("VSX_DEREP", "host")
    s = golden[0]
    assert dd.result_fields(host(s)) == dd.py_derep(s)


def test_worked_examples(golden):
    by_name = {s["name"]: s for s in golden}
    res = host(by_name["worked_examples"])
    clusters = dd.result_fields(res)["clusters"]
    first = next(c for c in clusters if c["rep"] == 0)
    assert first["members"] == [0, 5] and first["strands"] == [0, 1]          # TTTT (a1), then AAAA (s6) on minus
    acgt = next(c for c in clusters if c["rep"] == 1)
    assert acgt["members"] == [1, 3] and acgt["strands"] == [0, 0]            # ACGT / acgu: plus
    assert host(by_name["fastq_worked_avg"]).quality(0) == "&&&&&&&&&&"
    assert host(by_name["fastq_worked_max"]).quality(0) == "IIIIIIIIII"


def test_without_fastqout_no_quality_is_merged(golden):
    s = next(g for g in golden if g["name"] == "fastq_minus_avg")
    res = host(s, want_quality=False)
    assert res.quals is None
    assert dd.result_fields(res) == dd.py_derep(s, want_quality=False)


def test_window_does_not_matter_on_the_host(golden):
    s = next(g for g in golden if g["name"] == "fastq_minus_avg")
    assert dd.result_fields(host(s, window=1)) == dd.result_fields(host(s))


# ---- the threshold table ---------------------------------------------------------------------------------------------------------
def quality_value(p):
    return int(math.trunc(-10.0 * math.log10(p)))


def test_thresholds_are_the_largest_doubles():
    from vsearch_amd.derep import thresholds
    T = thresholds()
    assert len(T) == 129 and all(a > b for a, b in zip(T, T[1:]))
    for v, t in enumerate(T):
        assert quality_value(t) >= v and quality_value(from_bits(bits(t) + 1)) < v, v
        # log10 is monotone around the threshold: the table's comparison and the direct expression agree on every neighbour
        for d in range(-2000, 2001, 37):
            p = from_bits(bits(t) + d)
            assert (quality_value(p) >= v) == (p <= t), (v, d)


def test_table_lookup_equals_the_direct_expression():
    """every pair of input qualities under the size weights of the issue's check: the largest v with p <= T[v] is
    trunc(-10 log10 p)"""
    from vsearch_amd.derep import thresholds
    T = np.array(thresholds()[::-1])                                         # ascending
    prob = np.array([0.75 if q < 2 else math.pow(10.0, -q / 10.0) for q in range(94)])
    p1, p2 = np.meshgrid(prob, prob, indexing="ij")
    checked = 0
    for s1 in list(range(1, 40)) + [1000, 65535, 10 ** 6, 4 * 10 ** 9]:
        for s2 in (1, 2, 3, 7, 1000):
            p3 = ((p1 * float(s1) + p2 * float(s2)) / float(s1 + s2)).ravel()
            looked_up = 128 - np.searchsorted(T, p3, side="left")            # number of thresholds >= p, minus one
            direct = np.array([quality_value(p) for p in np.unique(p3)])
            assert np.array_equal(looked_up[np.unique(p3, return_index=True)[1]], direct), (s1, s2)
            checked += p3.size
    assert checked == 94 * 94 * 43 * 5


# ---- the calls the library refuses -----------------------------------------------------------------------------------------------
def refused(**kw):
    from vsearch_amd import VsxError
    from vsearch_amd.derep import dereplicate
    args = dict(seqs=["ACGT", "ACGT"], labels=["a", "b"], minseqlength=1)
    args.update(kw)
    seqs, labels = args.pop("seqs"), args.pop("labels")
    with pytest.raises(VsxError) as e:
        dereplicate(None, seqs, labels, **args)
    assert e.value.code == -1
    return str(e.value)


def test_error_returns():
    assert "33..126" in refused(quals=["II I", "IIII"])
    assert "33..126" in refused(quals=["II\x7fI", "IIII"])
    assert "0..127" in refused(quals=["IIII", "IIII"], asciiout=64, qmaxout=64)
    assert "0..127" in refused(quals=["IIII", "IIII"], qminout=-40)
    assert "0..127" in refused(quals=["IIII", "IIII"], ascii=128)
    assert "0..127" in refused(quals=["IIII", "IIII"], qminout=30, qmaxout=20)
    assert "want_quality" in refused(want_quality=1)
    assert "2^32" in refused(sizes=[4294967295, 2])
    assert "2^32" in refused(sizes=[1 << 32, 1])
    assert "abundance 0" in refused(sizes=[0, 1])
    assert "window" in refused(window=-1)


def test_a_read_beyond_its_blob_is_refused():
    import ctypes as C
    from vsearch_amd import _lib
    from vsearch_amd.derep import default_opts
    lib = _lib.load()
    seq = b"ACGTACGT"
    off, ln, loff = np.array([0, 4], np.uint64), np.array([4, 5], np.uint32), np.array([0, 1, 2], np.uint64)
    reads = _lib.FilterReads(C.cast(C.c_char_p(seq), C.c_void_p), None, len(seq), off.ctypes.data, ln.ctypes.data, None)
    out = _lib.DerepOut()
    o = default_opts(minseqlength=1)
    assert lib.vsx_derep(None, C.byref(o), 2, C.byref(reads), C.cast(C.c_char_p(b"ab"), C.c_void_p), loff.ctypes.data, C.byref(out)) == _lib.VSX_EINVAL
    assert b"exceeds its blob" in lib.vsx_last_error()


def test_the_sum_just_below_the_limit_is_served():
    from vsearch_amd.derep import dereplicate
    res = dereplicate(None, ["ACGT", "ACGT"], ["a", "b"], sizes=[4294967294, 1], minseqlength=1)
    assert int(res.size[0]) == 4294967295 and res.counts["maxsize"] == 4294967295


def test_the_cli_s_fatal_cases_raise():
    from vsearch_amd import derep
    with pytest.raises(ValueError, match="fastx_uniques"):
        derep.derep_fulllength(None, ["ACGT"], ["a"], quals=["IIII"])
    with pytest.raises(ValueError, match="fastx_uniques"):
        derep.derep_id(None, ["ACGT"], ["a"], quals=["IIII"])
    with pytest.raises(ValueError, match="FASTQ output"):
        derep.fastx_uniques(None, ["ACGT"], ["a"], fastqout=True)
    with pytest.raises(ValueError, match="tab separated"):
        derep.fastx_uniques(None, ["ACGT"], ["a"], tabbedout=True)


def test_command_defaults():
    from vsearch_amd import derep
    seqs, labels = ["ACGT" * 8, "ACGT" * 8, "ACGT"], ["a", "b", "c"]
    assert derep.derep_fulllength(None, seqs, labels).counts["discarded_short"] == 1
    assert derep.fastx_uniques(None, seqs, labels).counts["discarded_short"] == 0
    assert len(derep.derep_id(None, seqs, labels)) == 2                      # the labels differ: nothing joins
