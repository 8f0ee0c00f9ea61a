"""Prefix dereplication without a GPU: the library's host restatement (vsx_derep_prefix without a context: the one-pass rule)
against the plain-Python restatement of the reference's loop (tests/derep_prefix_data.py: py_derep_prefix) field for field, on
the recorded sets and on seeded nested sets; the package's formatters against the recorded text of the reference CLI
(tests/golden/derep_prefix_golden.json, written by `python -m tests.derep_prefix_data`) byte for byte; the ABI surface, the
calls the library refuses, and that every set reaches the case it is named after.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import derep_prefix_data as pd


@pytest.fixture(scope="module")
def golden():
    return pd.load_golden()


@pytest.fixture(scope="module")
def by_name(golden):
    return {s["name"]: s for s in golden}


def host(s, **extra):
    res = pd.call(None, s, **extra)
    st = res.stats
    assert st["reads_host"] == res.counts["kept"] and st["windows"] == 0 and st["host_no_context"] == 1
    assert st["host_environment"] + st["host_read_count"] + st["host_memory"] == 0
    return res


def cluster_of(py, s, label):
    k = s["labels"].index(label)
    return next(c for c in py["clusters"] if k in c["members"])


def test_golden_inputs_are_the_builders(golden):
    """the recorded inputs are what the builders build today"""
    built = pd.golden_sets()
    assert [g["name"] for g in golden] == [s["name"] for s in built]
    for g, s in zip(golden, built):
        assert {k: g[k] for k in pd.INPUT_KEYS} == {k: s[k] for k in pd.INPUT_KEYS}, s["name"]
    assert os.path.getsize(pd.GOLDEN) < 1 << 20


def test_host_equals_python_equals_golden(golden):
    for s in golden:
        res = host(s)
        assert pd.result_fields(res) == pd.py_derep_prefix(s), s["name"]
        text = pd.formatted(res, s)
        assert set(text) == set(s["ref"]), s["name"]
        for key in text:
            assert text[key] == s["ref"][key], (s["name"], key)


def test_seeded_nested_sets():
    """3 000 small sets over a two-letter alphabet, heavy nesting, tying labels and annotations: the one-pass rule is the loop"""
    for seed in range(3000):
        s = pd.nested_random_set(seed)
        assert pd.result_fields(host(s)) == pd.py_derep_prefix(s), seed


def test_large_input_sorted_in_slices():
    """40 000 reads: the library ranks them in slices of its worker pool and merges; ranks and clusters are the loop's"""
    s = pd.large_nested_set()
    res = host(s)
    assert res.counts["kept"] == 40000 and res.stats["distinct_lengths"] == 14
    assert pd.result_fields(res) == pd.py_derep_prefix(s)


def test_environment_route(golden, monkeypatch):
    """without a context the call is the host's whatever the environment says; the variable's own counter needs a context
    (tests/test_gpu_derep_prefix.py)"""
    monkeypatch.setenv("VSX_DEREP_PREFIX", "host")
    s = golden[0]
    assert pd.result_fields(host(s)) == pd.py_derep_prefix(s)


def test_window_does_not_matter_on_the_host(by_name):
    s = by_name["selection"]
    assert pd.result_fields(host(s, window=1)) == pd.result_fields(host(s))


# ---- every set reaches the case it is named after (by the loop's own account) ---------------------------------------------------
def test_ladder_is_one_cluster_in_uc_order(by_name):
    s = by_name["ladder"]
    py = pd.py_derep_prefix(s)
    assert len(py["clusters"]) == 1 and py["clusters"][0]["count"] == len(s["seqs"]) == 311
    members = py["clusters"][0]["members"]
    lengths = [len(s["seqs"][m]) for m in members]
    assert lengths[:300] == list(range(300, 0, -1))                          # the heads, from the longest node down
    assert lengths[300:] == sorted(lengths[300:]) and len(lengths[300:]) == 11       # then the duplicates, as the walk met them
    assert [py["rank"][m] for m in members[300:]] == sorted(py["rank"][m] for m in members[300:])


def test_winners(by_name):
    s = by_name["winners"]
    py = pd.py_derep_prefix(s)
    for item, winner, loser in (("len_item", "len_short", "len_long"), ("ab_item", "ab_c;size=5", "ab_a;size=2"),
                                ("lab_item", "lab_aa", "lab_zz")):
        c = cluster_of(py, s, item)
        assert [s["labels"][m] for m in c["members"]] == [winner, item]
        assert cluster_of(py, s, loser)["count"] == 1                        # the loser founds a cluster of its own
    c = cluster_of(py, s, "pos_item")
    assert c["members"] == [9, 11] and cluster_of(py, s, "pos")["rep"] == 9 and [x["members"] for x in py["clusters"]].count([10]) == 1


def test_thousand_extenders(by_name):
    s = by_name["thousand_extenders"]
    py = pd.py_derep_prefix(s)
    assert len(py["clusters"]) == 1000 and sorted(c["count"] for c in py["clusters"]) == [1] * 999 + [2]
    assert [s["labels"][m] for m in py["clusters"][0]["members"]] == ["e0000", "item"]


def test_absorbed_prefix_is_not_joined(by_name):
    s = by_name["absorbed"]
    py = pd.py_derep_prefix(s)
    assert [[s["labels"][m] for m in c["members"]] for c in py["clusters"]] == [["z", "x", "p"], ["y"]]


def test_boundary_lengths_and_near_misses(by_name):
    s = by_name["boundary_lengths"]
    py = pd.py_derep_prefix(s)
    chains = sorted(sorted(len(s["seqs"][m]) for m in c["members"]) for c in py["clusters"] if c["count"] == 3)
    assert chains == [[15, 16, 17], [31, 32, 33], [1023, 1024, 1025]]
    assert sum(1 for c in py["clusters"] if c["count"] == 1) == 9
    s = by_name["near_misses"]
    py = pd.py_derep_prefix(s)
    for l in (32, 33, 40):
        assert cluster_of(py, s, f"miss{l}")["count"] == 1
        assert [s["labels"][m] for m in cluster_of(py, s, f"item{l}")["members"]] == [f"after_g{l}", f"item{l}"]
        assert cluster_of(py, s, f"after_t{l}")["count"] == 1


def test_candidate_lengths(by_name):
    py = pd.py_derep_prefix(by_name["candidate_lengths"])
    assert sorted(c["count"] for c in py["clusters"]) == [64, 65, 66]


def test_alphabet(by_name):
    s = by_name["alphabet"]
    py = pd.py_derep_prefix(s)
    seqs = s["seqs"]
    # per code: the frame, its lower-case extension (...acgu) and the upper-case one (...ACGTA) that extends both: one chain
    for k, c in enumerate(pd.IUPAC):
        if c in "ATUN":
            continue
        chain = cluster_of(py, s, s["labels"][3 * k])
        assert chain["members"] == [3 * k + 2, 3 * k + 1, 3 * k], c
    # N against A: the frame with N goes to its own extension, the frame with A to A's
    n_frame, n_ext, a_ext = 3 * pd.IUPAC.index("N"), 48, 49
    assert seqs[n_ext].endswith("GG") and seqs[a_ext].endswith("GGC") and seqs[a_ext][:-1] != seqs[n_ext]
    assert cluster_of(py, s, s["labels"][n_ext])["members"] == [n_ext, n_frame]
    assert cluster_of(py, s, s["labels"][a_ext])["members"] == [a_ext, 0]
    # U is T: the frames with T and with U are one node, ...CC takes it and the all-u ...CCA extends that
    t_frame, u_frame = 3 * pd.IUPAC.index("T"), 3 * pd.IUPAC.index("U")
    assert sorted(cluster_of(py, s, s["labels"][51])["members"]) == sorted([51, 50, t_frame, u_frame])
    assert len(py["clusters"]) == 18


def test_sizein(by_name):
    with_sum, ignored, plain = (pd.py_derep_prefix(by_name[n]) for n in ("sizein", "sizein_ignored", "sizein_no_annotations"))
    s = by_name["sizein"]
    for py in (with_sum, ignored):                                           # the annotation decides the winner either way
        assert [s["labels"][m] for m in py["clusters"][0]["members"]] == ["c_ext;size=9", "item;size=3", "item2", "c_dup;size=4;"]
    assert [c["size"] for c in with_sum["clusters"]] == [17, 2] and [c["size"] for c in ignored["clusters"]] == [4, 1]
    assert [by_name["sizein_no_annotations"]["labels"][m] for m in plain["clusters"][0]["members"]] == ["a_ext", "item", "item2"]
    assert [c["size"] for c in plain["clusters"]] == [3, 2]


def test_cluster_order_tie_is_broken_by_sorted_rank(by_name):
    py = pd.py_derep_prefix(by_name["cluster_order"])
    assert [c["rep"] for c in py["clusters"]] == [1, 0] and py["rank"] == [1, 0]


def test_selection_and_median(by_name):
    py = pd.py_derep_prefix(by_name["selection"])
    assert [c["size"] for c in py["clusters"]] == [8, 7, 6, 5, 4, 3, 2, 1]
    assert py["counts"]["median"] == 4.5 and py["counts"]["selected"] == 3
    assert len(by_name["selection"]["ref"]["fasta"]) == 3 * 2


def test_one_symbol_reads_empty_and_discards(by_name):
    py = pd.py_derep_prefix(by_name["one_symbol"])
    assert py["counts"]["shortest"] == 1 and py["counts"]["kept"] == 10
    assert len(pd.py_derep_prefix(by_name["empty"])["clusters"]) == 0
    gone = pd.py_derep_prefix(by_name["all_discarded"])
    assert gone["counts"]["kept"] == 0 and gone["counts"]["discarded_short"] == 2 and by_name["all_discarded"]["ref"]["uc"] == []
    d = pd.py_derep_prefix(by_name["discards"])["counts"]
    assert (d["discarded_short"], d["discarded_long"], d["kept"]) == (2, 1, 3)


# ---- the ABI surface ---------------------------------------------------------------------------------------------------------------
def test_abi_surface_and_defaults():
    import vsearch_amd
    from vsearch_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(pd.ROOT, "include", "vsx_derep_prefix.h")).read()
    declared = set(re.findall(r"\b(vsx_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.DEREP_PREFIX_SYMBOLS), declared ^ set(_lib.DEREP_PREFIX_SYMBOLS)
    for name in _lib.DEREP_PREFIX_SYMBOLS:
        assert hasattr(lib, name), name
    o = _lib.DerepPrefixOpts()
    lib.vsx_derep_prefix_opts_default(C.byref(o))
    assert (o.sizein, o.minseqlength, o.maxseqlength, o.minuniquesize, o.maxuniquesize, o.topn, o.window) == \
        (0, 32, 50000, 1, pd.INT64_MAX, pd.INT64_MAX, 0)
    # the ctypes mirrors have the sizes of the header's structs
    assert C.sizeof(_lib.DerepPrefixOpts) == 8 + 6 * 8 and C.sizeof(_lib.DerepPrefixOut) == 12 * 8 + 6 * 8
    assert C.sizeof(_lib.DerepPrefixStats) == 9 * 8 + 10 * 8
    for name in ("derep_prefix", "derep_prefix_host", "DerepPrefixResult"):
        assert hasattr(vsearch_amd, name) and name in vsearch_amd.__all__


# ---- the calls the library refuses -----------------------------------------------------------------------------------------------
def refused(**kw):
    from vsearch_amd import VsxError, derep_prefix_host
    args = dict(seqs=["ACGT", "ACG"], labels=["a", "b"], minseqlength=1)
    args.update(kw)
    seqs, labels = args.pop("seqs"), args.pop("labels")
    with pytest.raises(VsxError) as e:
        derep_prefix_host(seqs, labels, **args)
    assert e.value.code == -1
    return str(e.value)


def test_error_returns():
    assert "2^32" in refused(sizes=[4294967295, 1], sizein=1)                # a total of 2^32
    assert "2^32" in refused(sizes=[1 << 32, 1])                             # one abundance the sort key cannot hold
    assert "abundance 0" in refused(sizes=[0, 1])
    assert "window" in refused(window=-1)


def test_the_sum_just_below_the_limit_is_served(by_name):
    from vsearch_amd import derep_prefix_host
    res = derep_prefix_host(["ACGT", "ACG"], ["a", "b"], sizes=[4294967294, 1], sizein=1, minseqlength=1)
    assert int(res.size[0]) == 4294967295 and res.counts["maxsize"] == 4294967295 and [int(m) for m in res.members(0)] == [0, 1]
    assert pd.py_derep_prefix(by_name["sum_limit"])["clusters"][0]["size"] == (1 << 32) - 1
    # without --sizein the annotations are sort keys only: their sum is no size and is not refused
    res = derep_prefix_host(["ACGT", "ACG"], ["a", "b"], sizes=[4294967295, 4294967295], minseqlength=1)
    assert int(res.size[0]) == 2


def test_malformed_offsets_are_refused():
    from vsearch_amd import _lib
    from vsearch_amd.derep_prefix import default_opts
    lib = _lib.load()
    seq = b"ACGTACGT"
    off, ln = np.array([0, 4], np.uint64), np.array([4, 5], np.uint32)
    reads = _lib.FilterReads(C.cast(C.c_char_p(seq), C.c_void_p), None, len(seq), off.ctypes.data, ln.ctypes.data, None)
    o = default_opts(minseqlength=1)
    labels = C.cast(C.c_char_p(b"ab"), C.c_void_p)
    out = _lib.DerepPrefixOut()
    loff = np.array([0, 1, 2], np.uint64)
    assert lib.vsx_derep_prefix(None, C.byref(o), 2, C.byref(reads), labels, loff.ctypes.data, C.byref(out)) == _lib.VSX_EINVAL
    assert b"exceeds its blob" in lib.vsx_last_error()
    ln[1] = 4
    loff = np.array([0, 2, 1], np.uint64)
    assert lib.vsx_derep_prefix(None, C.byref(o), 2, C.byref(reads), labels, loff.ctypes.data, C.byref(out)) == _lib.VSX_EINVAL
    assert b"label offsets decrease" in lib.vsx_last_error()


def test_strand_both_is_fatal():
    from vsearch_amd import derep_prefix
    with pytest.raises(ValueError, match="strand both"):
        derep_prefix(None, ["ACGT"], ["a"], strand_both=True)
