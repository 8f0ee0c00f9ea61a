"""Exact sequence search without a GPU: the library's host restatement (vsx_internal_search_exact_host, a std::unordered_multimap
over the code strings) = the plain-Python restatement (tests/search_exact_data.py) = the recorded lines of the reference CLI.

tests/golden/search_exact_golden.json holds inputs and the reference's output only; `python -m tests.search_exact_data` rewrites it
from oracle/_ref/vsearch_ref (--search_exact --threads 1 with --userout, --uc, --uc_allhits, --dbmatched --sizeout and --log).
"""
import pytest

from tests import search_exact_data as sd


@pytest.fixture(scope="module")
def golden():
    return sd.load_golden()


_HITS = {}


def host_hits(s):
    """the host restatement's answer, computed once per set"""
    if s["name"] not in _HITS:
        from vsearch_amd.search import search_exact_host
        _HITS[s["name"]] = search_exact_host(s["db"], s["queries"], db_sizes=s["db_sizes"], db_labels=s["db_names"], sizes=s["sizes"],
                                             labels=s["names"], **sd.session_opts(s["opts"]))
    return _HITS[s["name"]]


def test_library_exports_the_exact_symbols():
    import vsearch_amd
    lib = vsearch_amd.load_library()
    assert [n for n in vsearch_amd._lib.EXACT_SYMBOLS if not hasattr(lib, n)] == []


def test_golden_inputs_are_the_builders(golden):
    """the golden file's inputs are what the builders make today (a changed builder needs a re-recorded file)"""
    built = {s["name"]: s for s in sd.golden_sets()}
    assert sorted(built) == sorted(g["name"] for g in golden)
    for g in golden:
        for k in sd.INPUT_KEYS:
            assert g[k] == built[g["name"]][k], (g["name"], k)


def test_host_equals_python(golden):
    for s in golden + [sd.selfid_set()]:
        sd.assert_hits_equal_py(host_hits(s), s)


def test_userout_equals_reference(golden):
    for s in golden:
        assert sd.userout_lines(s, host_hits(s)) == s["ref"]["userout"], s["name"]


def test_uc_equals_reference(golden):
    for s in golden:
        assert sd.uc_lines(s, host_hits(s)) == s["ref"]["uc"], s["name"]
        assert sd.uc_lines(s, host_hits(s), uc_allhits=True) == s["ref"]["uc_allhits"], s["name"]


def test_summary_equals_reference(golden):
    """exact_summary against the recorded --dbmatched --sizeout sizes and the log's two "Matching ..." counts"""
    with_total = 0
    for s in golden:
        dbm, unique, total = sd.summary_of(s, host_hits(s))
        ref_unique, ref_total = sd.log_counts(s["ref"]["log"])
        assert dbm == s["ref"]["dbmatched"], s["name"]
        assert unique == ref_unique, s["name"]
        if ref_total is not None:                      # the reference prints the abundance line with --sizein only
            assert total == ref_total, s["name"]
            with_total += 1
    assert with_total >= 10


def test_issue_example_reads_as_stated(golden):
    s = next(g for g in golden if g["name"] == "issue_example")
    got = [[f"t{h['target']}{'-' if h['strand'] else '+'}" for h in hs] for hs in host_hits(s)]
    assert got == [["t0+", "t1+", "t2-", "t7+"], ["t3+", "t3-"], ["t4+"], [], ["t4-"], [], ["t5+"]]


def test_masking_matters_only_with_hardmask(golden):
    by = {g["name"]: [len(hs) for hs in host_hits(g)] for g in golden if g["name"].startswith("masking_")}
    assert by["masking_dust_none_hard"] == [0, 1, 0]       # the low-complexity read misses its own copy, on both strands
    assert by["masking_dust_none"] == by["masking_dust_dust_hard"] == by["masking_none_none_hard"] == [1, 1, 1]


def test_summary_shape():
    from vsearch_amd.search import exact_summary
    hits = [[dict(target=2), dict(target=0)], [], [dict(target=2)]]
    sm = exact_summary(hits, sizes=[3, 5, 7], n_targets=3)
    assert sm["matched"] == [0, 2] and sm["notmatched"] == [1]
    assert sm["dbmatched"] == {0: 3, 1: 0, 2: 10}
    assert (sm["queries_matched"], sm["queries"], sm["abundance_matched"], sm["abundance"]) == (2, 3, 10, 15)
    assert exact_summary(hits)["dbmatched"] == {2: 2, 0: 1}


def test_zero_queries_and_zero_length():
    from vsearch_amd.search import search_exact_host
    assert search_exact_host(["ACGT"], [], strand_both=1) == []
    assert search_exact_host(["ACGT", ""], ["", "ACGT"], strand_both=1) == [[], [dict(sd.expected_record(4, 0, 0), query=1),
                                                                                   dict(sd.expected_record(4, 0, 1), query=1)]]
