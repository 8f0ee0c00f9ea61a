"""Abundance and length sorting without a GPU: the library's host restatement (VSX_SORTBY=host) against the plain-Python restatement
of tests/sortby_data.py on the order, n_kept, n_out and the median's bit pattern over every set and 3 000 seeded dense cases, the
writers against the reference's recorded files, the ABI surface and every refusal, and the assertions that the input sets reach the
edges they are named after (computed from py_sortby()).
"""
import ctypes as C
import random
import struct

import numpy as np
import pytest

from tests import sortby_data as sd
from vsearch_amd import _lib
from vsearch_amd import sortby as sb


@pytest.fixture(scope="module")
def sets():
    return sd.all_sets()


@pytest.fixture(scope="module")
def by_name(sets):
    return {s["name"]: s for s in sets}


@pytest.fixture(scope="module")
def expected(sets):
    return {s["name"]: sd.expected(s) for s in sets}


# ---- host restatement == plain Python ------------------------------------------------------------------------------------------
def test_host_equals_python_on_every_set(sets):
    for s in sets:
        res = sd.call(None, s)
        sd.assert_equals_py(res, s)
        assert sd.routes(res) == [1, 0, 0, 0, 0] and res.stats["items"] == len(s["labels"]), res.stats


def test_host_equals_python_on_3000_dense_cases():
    rng = random.Random(3111)
    ties = prefixes = 0
    for _ in range(3000):
        s = sd.seeded_case(rng, rng.randint(0, 30))
        sd.assert_equals_py(sd.call(None, s), s)
        labels = [sd.raw(l) for l in s["labels"]]
        ties += len(labels) - len(set(labels))
        prefixes += sum(1 for a in labels for b in labels if len(a) < len(b) and b.startswith(a))
    assert ties > 3000 and prefixes > 30000


def test_threads_do_not_show():
    rng = random.Random(3112)
    labels = sd.illumina(rng, 150000, long_prefix=True)
    sizes = [sd.header_size(l) for l in labels]
    lengths = [rng.randint(200, 260) for _ in labels]
    for order in ("size", "length", "length_asc"):
        one = sb.sortby_host(labels, lengths, sizes, order, threads=1)
        for threads in (2, 5, 16):
            assert sb.sortby_host(labels, lengths, sizes, order, threads=threads).tobytes() == one.tobytes(), (order, threads)
    small = sd._set("threads", labels[:3000], "length", seqs=["A" * n for n in lengths[:3000]])
    sd.assert_equals_py(sd.call(None, small, threads=16), small)


def test_scattered_and_reversed_offsets(by_name):
    s = by_name["illumina"]
    full = sd.call(None, s)
    rng = random.Random(5)
    blob, off = b"", []
    for l in reversed(s["labels"]):                                          # the last header first, junk between them
        blob += b"M01234:"[:rng.randint(0, 7)]
        off.append(len(blob))
        blob += sd.raw(l)
    off = np.array(off[::-1], np.uint64)
    lens = np.array([len(sd.raw(l)) for l in s["labels"]], np.uint32)
    assert sd.call(None, s, labels=(blob, off, lens)).tobytes() == full.tobytes()


# ---- the writers ---------------------------------------------------------------------------------------------------------------
def test_writers_equal_golden():
    for s in sd.load_golden():
        sd.assert_text_equals_golden(sd.call(None, s), s)


def test_log_line_rounds_half_to_even(by_name):
    assert sb.log_lines(sd.call(None, by_name["median_2_5"])) == ["Median abundance: 2"]
    assert sb.log_lines(sd.call(None, by_name["median_3_5"])) == ["Median abundance: 4"]
    assert sb.log_lines(sd.call(None, by_name["median_length_2_5"])) == ["Median length: 2"]
    assert sb.log_lines(sd.call(None, by_name["n_0"])) == ["Median abundance: 0"]


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def _raw(opts_edit=None, blob=b"bbaacc", off=(0, 2, 4), lens=(2, 2, 2), seqlen=(5, 5, 5), sizes=(1, 1, 1)):
    lib = _lib.load()
    o = _lib.SortbyOpts()
    lib.vsx_sortby_opts_default(C.byref(o))
    if opts_edit:
        opts_edit(o)
    arrays = [np.array(off, np.uint64), np.array(lens, np.uint32), np.array(seqlen, np.uint32), np.array(sizes, np.uint32)]
    res = _lib.SortbyOut()
    rc = lib.vsx_sortby(None, C.byref(o), len(lens), C.cast(C.c_char_p(blob), C.c_void_p), len(blob), *[a.ctypes.data_as(C.c_void_p) for a in arrays],
                        C.byref(res))
    order = None
    if rc == 0:
        order = [C.cast(res.order, C.POINTER(C.c_uint64))[k] for k in range(res.n_out)]
        lib.vsx_sortby_out_free(C.byref(res))
    return rc, order, lib.vsx_last_error().decode()


def edit(**kw):
    def f(o):
        for k, v in kw.items():
            setattr(o, k, v)
    return f


def test_symbols_and_defaults():
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in _lib.SORTBY_SYMBOLS)
    o = _lib.SortbyOpts()
    lib.vsx_sortby_opts_default(C.byref(o))
    assert (o.order, o.threads, o.minsize, o.maxsize, o.topn) == (_lib.SORTBY_SIZE, 0, 0, sd.INT64_MAX, sd.INT64_MAX)
    assert C.sizeof(_lib.SortbyOpts) == 32 and C.sizeof(_lib.SortbyOut) == 5 * 8 and C.sizeof(_lib.SortbyStats) == (7 + 6 + 8 + 6) * 8
    assert (_lib.SORTBY_SIZE, _lib.SORTBY_LENGTH, _lib.SORTBY_LENGTH_ASC) == (0, 1, 2)
    import vsearch_amd
    assert vsearch_amd.sortbysize is sb.sortbysize and vsearch_amd.sortbylength is sb.sortbylength and vsearch_amd.sortby is sb
    import __graft_entry__
    assert "SORTBY_SYMBOLS" in open(__graft_entry__.__file__).read()


def test_refusals():
    assert _raw()[:2] == (0, [1, 0, 2])
    for kw in (dict(order=3), dict(order=-1), dict(topn=-1), dict(threads=-1)):
        rc, _, text = _raw(opts_edit=edit(**kw))
        assert rc == _lib.VSX_EINVAL and text.startswith("vsx_sortby"), (kw, text)
    assert _raw(off=(0, 2, 5))[0] == _lib.VSX_EINVAL                          # beyond the blob
    assert _raw(off=(0, 2, 7), lens=(2, 2, 0))[0] == _lib.VSX_EINVAL          # an empty header may not start beyond it either
    assert _raw(sizes=(1, 0, 1))[0] == _lib.VSX_EINVAL                        # an abundance of 0
    assert _raw(blob=b"bb\0acc")[0] == _lib.VSX_EINVAL                        # a NUL in a header
    assert _raw(blob=b"bb\0acc", off=(0, 3, 4), lens=(2, 1, 2))[:2] == (0, [1, 0, 2])      # ... but not between headers
    assert _raw(off=(0, 0, 4))[:2] == (0, [0, 1, 2])                          # headers may share bytes: nothing is written into them
    assert _raw(blob=b"", off=(), lens=(), seqlen=(), sizes=())[:2] == (0, [])
    assert _raw(opts_edit=edit(topn=0))[:2] == (0, [])
    assert _raw(opts_edit=edit(minsize=-5, maxsize=-1))[:2] == (0, [])        # any bounds are taken as they are


def test_round_cap_is_checked_per_call(monkeypatch):
    monkeypatch.setenv("VSX_SORTBY_MAX_ROUNDS", "33")
    assert _raw()[0] == _lib.VSX_EINVAL
    monkeypatch.setenv("VSX_SORTBY_MAX_ROUNDS", "0")
    assert _raw()[:2] == (0, [1, 0, 2])


def test_python_refuses_what_uint32_cannot_hold():
    with pytest.raises(ValueError):
        sb.sortby_host(["a"], [1], [2 ** 32], "size")
    with pytest.raises(ValueError):
        sb.sortby_host(["a", "b"], [1], [1, 1], "size")
    with pytest.raises(_lib.VsxError):
        sb.sortby_host(["a\0b"], [1], [1], "size")


def test_db_order_without_a_device_is_the_python_sort():
    """sort_by_abundance (the Python sort the chimera sessions used) and the library's order agree"""
    from vsearch_amd.chimera import header_size, sort_by_abundance
    labels = sd.illumina(random.Random(3113), 2000, long_prefix=True)
    sizes = [header_size(l) for l in labels]
    assert [int(k) for k in sb.sortby_host(labels, [1] * len(labels), sizes, "size").order] == sort_by_abundance(sizes, labels)


# ---- the sets reach their edges ------------------------------------------------------------------------------------------------
def _first_diff(a, b):
    a, b = sd.raw(a), sd.raw(b)
    k = 0
    while k < min(len(a), len(b)) and a[k] == b[k]:
        k += 1
    return k


def test_counts_and_label_lengths(by_name):
    assert {len(by_name[f"n_{n}"]["labels"]) for n in (0, 1, 2, 63, 64, 65, 255, 256, 257)} == {0, 1, 2, 63, 64, 65, 255, 256, 257}
    assert sorted(len(l) for l in by_name["label_lengths"]["labels"]) == list(sd.LABEL_LENGTHS)
    assert 0 in {len(l) for l in by_name["label_empty"]["labels"]}
    assert len(set(by_name["label_lengths"]["sizes"])) == 1                  # one tie group: the labels decide


def test_first_differing_bytes_and_prefixes(by_name, expected):
    s, e = by_name["first_diff"], expected["first_diff"]
    ordered = [s["labels"][k] for k in e["order"]]
    assert set(sd.FIRST_DIFFS) <= {_first_diff(a, b) for a, b in zip(ordered, ordered[1:])}
    assert e["order"] != list(range(len(ordered)))
    for name in ("prefix_labels", "label_lengths"):
        s, e = by_name[name], expected[name]
        ordered = [sd.raw(s["labels"][k]) for k in e["order"]]
        assert all(b.startswith(a) and len(a) < len(b) for a, b in zip(ordered, ordered[1:])), name      # every neighbour a proper prefix
        assert {7, 8, 9, 15, 16, 17, 63, 64, 65} <= {len(x) for x in ordered}
    s = by_name["blob_edge"]
    assert expected["blob_edge"]["order"][-2:] == [3, 1] and sd.raw(s["labels"][-1])[:-1] == sd.raw(s["labels"][1])[:-1]


def test_equal_labels_keep_input_order(by_name, expected):
    s, e = by_name["equal_labels"], expected["equal_labels"]
    same = [k for k in e["order"] if s["labels"][k] == "same"]
    assert same == [2, 4, 6] and len({len(x) for x in s["seqs"]}) == len(s["seqs"])


def test_unsigned_bytes(by_name, expected):
    assert [by_name["bytes_7f_80"]["labels"][k] for k in expected["bytes_7f_80"]["order"]] == [b"ab", b"ab\x01", b"ab\x7f", b"ab\x80", b"ab\xff"]
    e = [by_name["bytes_at_chunk_edge"]["labels"][k] for k in expected["bytes_at_chunk_edge"]["order"]]
    assert e == [b"abcdefgh\x01", b"abcdefgh\xff", b"abcdefg\x7f", b"abcdefg\x80", b"abcdefg\xffa"]      # 'h' is 0x68, below 0x7f


def test_tie_groups(by_name, expected):
    assert len(set(by_name["one_tie_group"]["sizes"])) == 1
    s = by_name["deep_beside_flat"]
    assert s["labels"].count("same") == 64
    deep = [l for l in s["labels"] if l != "same"]
    assert len(deep) == 5 and {_first_diff(a, b) for a in deep for b in deep if a != b} == {66} and 66 // 8 + 1 == 9
    sizes = by_name["many_groups"]["sizes"]
    assert sorted(sizes.count(v) for v in set(sizes)) == [2] * 300
    s = by_name["long_prefix"]
    assert len(s["labels"]) == 64 and min(_first_diff(a, b) for a in s["labels"] for b in s["labels"] if a != b) >= 300 > 8 * _lib.SORTBY_MAX_ROUNDS


def test_length_against_abundance(by_name, expected):
    for name in ("length_vs_abundance", "length_asc"):
        s, e = by_name[name], expected[name]
        pairs = [(s["lengths"][k], s["sizes"][k]) for k in e["order"]]
        # ties in length with different abundance (the larger first), and equal abundances that the length separates
        assert any(a[0] == b[0] and a[1] > b[1] for a, b in zip(pairs, pairs[1:]))
        assert any(a[0] != b[0] and a[1] == b[1] for a in pairs for b in pairs)
        assert any(a[0] != b[0] and a[1] < b[1] for a, b in zip(pairs, pairs[1:]))         # the length wins over the abundance
        lengths = [p[0] for p in pairs]
        assert lengths == sorted(lengths, reverse=(name != "length_asc"))
    assert set(by_name["large_abundances"]["sizes"]) == {1, 2 ** 31, 2 ** 32 - 1}
    assert [by_name["large_abundances"]["sizes"][k] for k in expected["large_abundances"]["order"]] == [2 ** 32 - 1] * 2 + [2 ** 31] * 2 + [1] * 2


def test_selection_topn_and_median(by_name, expected):
    kept = {name[7:]: expected[name]["n_kept"] for name in by_name if name.startswith("minmax_")}
    assert kept == {"3_3": 3, "2_4": 6, "4_2": 0, "100_max": 0, "3_max": 6, "0_3": 6, "0_0": 0}
    assert expected["length_ignores_minmax"]["n_kept"] == expected["length_asc_ignores_minmax"]["n_kept"] == 9
    assert {t: (expected[f"topn_{t}"]["n_kept"], expected[f"topn_{t}"]["n_out"]) for t in (0, 1, 6, 7, 8)} == \
        {0: (9, 0), 1: (7, 1), 6: (7, 6), 7: (7, 7), 8: (7, 7)}
    assert [expected[n]["median"] for n in ("median_odd", "median_2_5", "median_3_5", "median_before_topn", "median_length_2_5", "length_asc_median")] == \
        [4.0, 2.5, 3.5, 3.5, 2.5, 2.5]
    assert expected["median_before_topn"]["n_out"] == 1 and expected["minmax_4_2"]["median"] == 0.0
    assert struct.pack("<d", expected["n_0"]["median"]) == struct.pack("<d", 0.0)
