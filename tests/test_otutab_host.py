"""The OTU table's host restatement (vsx_internal_otutab_host, vsearch_amd.otutab) without a GPU: against the plain-Python
restatement with the reference's three patterns (tests/otutab_data.py: py_otutab) on every result array, for every set and for
3 000 seeded random label sets; the three formatters against the reference CLI's recorded files
(tests/golden/otutab_golden.json); the ABI surface and the refusals; and that every set reaches the edge it is named after.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import otutab_data as od

ot = importlib.import_module("vsearch_amd.otutab")
NONE = od.NONE


@pytest.fixture(scope="module")
def golden():
    return od.load_golden()


def test_golden_holds_every_set(golden):
    built = [od.to_json(s) for s in od.all_sets()]
    assert [g["name"] for g in golden] == [b["name"] for b in built]
    for g, b in zip(golden, built):
        assert {k: v for k, v in od.to_json(g).items() if k != "ref"} == b, g["name"]
        assert (g["ref"] is not None) == g["cli"], g["name"]


def test_host_is_python_on_every_set(golden):
    for s in golden:
        t = od.call(None, s, host=True)
        assert t.arrays() == od.expected(s), s["name"]
        st = t.stats
        assert st["labels_device"] == 0 and st["labels_host"] == len(t.q_sample) + st["targets_in_adds"], s["name"]
        via_api = od.call(None, s)                              # vsx_otutab without a context: the same restatement, counted
        assert via_api.arrays() == t.arrays() and via_api.stats["host_no_context"] == 1


def test_formatters_against_the_recorded_files(golden):
    seen = 0
    for s in golden:
        if s["ref"] is None:
            continue
        t = od.call(None, s, host=True)
        text = od.texts(t, generated_by=od.generated_by(s["ref"]["biom"]))
        assert text["otutabout"] == s["ref"]["otutabout"], s["name"]
        assert text["mothur"] == s["ref"]["mothur"], s["name"]
        assert od.mask_date(text["biom"]) == od.mask_date(s["ref"]["biom"]), s["name"]
        seen += 1
    assert seen >= 15


def test_the_issues_worked_examples(golden):
    by = {s["name"]: s for s in golden}
    tab = "\t".join
    assert by["recorded_search"]["ref"]["otutabout"] == "\n".join([
        tab(["#OTU ID", "", "B", "S", "S1", "Z", "xsample", "taxonomy"]), tab(["", "0", "0", "0", "0", "1", "0", "zz"]),
        tab(["otuA", "0", "1", "0", "5", "0", "2", "k:Bact"]), tab(["otuB", "1", "0", "1", "0", "0", "0", ""])]) + "\n"
    assert by["recorded_search"]["ref"]["mothur"].startswith(tab(["label", "Group", "numOtus", "", "otuA", "otuB"]) + "\n" + tab(["vsearch", "", "3"]))
    biom = by["recorded_search"]["ref"]["biom"]
    assert '"shape": [3,6]' in biom and '{"id":"otuB", "metadata":{"taxonomy":""}}' in biom
    assert "".join(biom.split()).endswith('"data":[[0,4,1],[1,1,1],[1,3,5],[1,5,2],[2,0,1],[2,2,1]]}')
    assert '"metadata":null}' in by["second_hit"]["ref"]["biom"].split('"columns"')[0]
    assert by["second_hit"]["ref"]["otutabout"] == "#OTU ID\ts\nfirst\t1\nthird\t0\n"
    assert by["recorded_cluster"]["ref"]["otutabout"] == "#OTU ID\ts1\ts1_a\ts2\ns1.c\t1\t0\t0\ns1_a\t0\t4\t2\n"
    assert by["recorded_cluster_relabel"]["ref"]["otutabout"] == "#OTU ID\ts1\ts1_a\ts2\nOTU_1\t0\t4\t2\nOTU_2\t1\t0\t0\n"


def test_annotated_abundance_counts_without_sizein():
    """found by oracle/soak_commands.py --command otutab: --search_exact and --usearch_global hand otutable_add the header's
    ;size= annotation whether or not --sizein is given; inputs() used to count 1 per query without --sizein.  The expected text is
    the reference CLI's own for this input, with and without --sizein."""
    import os
    for sizein in (False, True):
        s = od.search_set("annotated", ["a;sample=s;size=5", "b;sample=s"], ["o1"], [0, 0], sizein=sizein)
        assert od.inputs(s)[3] == [5, 1]
        assert od.texts(od.call(None, s, host=True))["otutabout"] == "#OTU ID\ts\no1\t6\n"
        if os.path.exists(od.ref_binary()):
            assert od.run_reference(s)["otutabout"] == "#OTU ID\ts\no1\t6\n"


def test_random_label_sets():
    for seed in range(3000):
        q, t, q_target, sizes, matched = od.random_label_set(seed)
        got = ot.otutab_host(q, t, q_target, sizes=sizes, matched=matched, threads=1 + seed % 3)
        assert got.arrays() == od.py_otutab(q, t, q_target, sizes, matched), seed


def test_large_set_on_sixteen_threads():
    q, t, q_target, sizes, matched = od.large_random_inputs()
    a = ot.otutab_host(q, t, q_target, sizes=sizes, matched=matched, threads=16)
    b = ot.otutab_host(q, t, q_target, sizes=sizes, matched=matched, threads=1)
    assert a.arrays() == b.arrays() == od.py_otutab(q, t, q_target, sizes, matched)
    assert len(a.samples) == 40 and a.t_otu[295] == NONE and a.t_otu[296] != NONE and not np.any(a.nz_count == 0)


def test_every_set_reaches_its_edge(golden):
    by = {s["name"]: s for s in golden}
    arrays = {name: od.expected(s) for name, s in by.items()}
    samples, otus, tax = (lambda n: arrays[n][0]), (lambda n: arrays[n][1]), (lambda n: arrays[n][2])
    # lengths: the fallback prefix is the whole label at 63 .. 129 bytes; "sample" is a name, "sample=" an empty one
    assert {len(x) for x in samples("lengths")} == {0, 1, 6, 63, 64, 65, 127, 128, 129}
    # keyword offsets: every label's value is found, none falls back or takes the decoy
    q, t, *_ = od.inputs(by["keyword_offsets"])
    assert len(q) == len(t) == 56 and all(len(l) == 140 for l in q[:27])
    assert sorted(samples("keyword_offsets")) == sorted({b"V%d_%d" % (n, o) for n in (7, 13) for o in range(44, 71)} | {b"V0_7", b"V0_13"})
    # (the tax= targets carry no otu=: their OTU is the prefix before the first ';', decoy included, and each has a taxonomy)
    assert sorted(otus("keyword_offsets")) == sorted({b"V4_%d" % o for o in range(44, 71)} | {b"V0_4"} | {l.split(b";")[0] for l in t[28:]})
    assert sorted(x for x in tax("keyword_offsets") if x is not None) == sorted({b"V4_%d" % o for o in range(44, 71)} | {b"V0_4"})
    assert len(otus("keyword_offsets")) == 56
    # values ending at bytes 63 / 64 / 65 and the 300-byte value
    assert sorted(len(x) for x in samples("value_ends")) == [56, 57, 58, 300]
    assert sorted(len(x) for x in otus("value_ends")) == [59, 60, 61, 63, 64, 65, 299, 300]
    assert samples("odd_values") == [b"", b"A", b"B2", b"Sample", b"a=b", b"ab", b"v2", b"v3", b"xsample"]
    assert otus("odd_values") == [b"", b"O", b"Q", b"nosemi", b"notu=5"] and tax("odd_values") == [b"", b"T", None, None, None]
    assert samples("order") == otus("order") == [b"", b"A", b"S1", b"S10", b"S1_", b"_", b"a", b"\xe9"]
    assert tax("tax_first_then_second") == [b"two"] and tax("tax_second_then_first") == [b"one"] and tax("tax_from_unmatched_pass") == [b"one"]
    assert otus("second_hit") == [b"first", b"third"]
    assert samples("abundance_zero") == [b"s", b"u"] and np.frombuffer(arrays["abundance_zero"][6], np.uint64).tolist() == [3]
    assert np.frombuffer(arrays["sum_above_32_bits"][6], np.uint64).tolist() == [6000000000]
    assert samples("no_query") == [] and otus("no_query") == [b"o1", b"o2"] and otus("no_target") == [] and len(samples("no_target")) == 2
    assert arrays["no_hits"][4] == b"" and otus("no_hits") == [b"o1", b"o2"] and arrays["no_hits"][3]
    assert otus("cluster_relabel") == [b"Otu1", b"Otu2", b"Otu3"] and otus("cluster_relabel_otu_prefix") == [b"Q1", b"Q2", b"Q3"]
    assert otus("cluster_plain") == [b"c1", b"c2", b"c3"]


def test_spans_may_overlap_and_come_in_any_order():
    blob = b"##r1;sample=AB;otu=X;tax=T##"
    q = ot.LabelBlob.of(blob, [2, 5, 2, 12], [12, 9, 12, 2])         # r1;sample=AB | sample=AB | r1;sample=AB | AB
    t = ot.LabelBlob.of(blob, [15, 2], [11, 18])                     # otu=X;tax=T | r1;sample=AB;otu=X
    got = ot.otutab_host(q, t, [0, 1, NONE, 1])
    assert got.samples == [b"AB"] and got.otus == [b"X"] and got.tax == [b"T"] and got.nz_count.tolist() == [3]


def test_abi_surface_and_refusals():
    from vsearch_amd import VsxError, _lib, load_library
    lib = load_library()
    for name in _lib.OTUTAB_SYMBOLS:
        assert hasattr(lib, name), name
    o = _lib.OtutabOpts(threads=7, pad=7)
    lib.vsx_otutab_opts_default(C.byref(o))
    assert (o.threads, o.pad) == (0, 0)
    assert C.sizeof(_lib.Labels) == 40 and C.sizeof(_lib.OtutabStats) == 7 * 8 + 10 * 8
    with pytest.raises(VsxError) as e:
        ot.otutab_host(["a"], ["o"], [1])
    assert e.value.code == -1 and "names target 1 of 1" in str(e.value)
    with pytest.raises(VsxError) as e:
        ot.otutab_host(["a"], [], [0])
    assert e.value.code == -1
    with pytest.raises(VsxError) as e:
        ot.otutab_host(ot.LabelBlob.of(b"abc", [1], [3]), ["o"], [0])
    assert e.value.code == -1 and "query label 0 lies outside its blob" in str(e.value)
    with pytest.raises(VsxError) as e:
        ot.otutab(["a"], ot.LabelBlob.of(b"abc", [4], [0]), [NONE])
    assert e.value.code == -1 and "target label 0" in str(e.value)
    with pytest.raises(VsxError):
        ot.otutab_host(["a"], ["o"], [0], threads=-1)
    assert ot.otutab_host(["a"], ["o"], [NONE]).t_otu.tolist() == [NONE]          # no add names the target: no OTU at all
    out = _lib.OtutabResult()
    lib.vsx_otutab_result_free(C.byref(out))                                       # an empty result may be freed
    lib.vsx_otutab_result_free(None)
