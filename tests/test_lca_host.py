"""--lcaout without a GPU: the library's host restatement (vsx_internal_lca_host) and a host index (vsx_lca_index_create without a
context, whose calls compare prefix numbers) against the plain-Python restatement of the reference's loops (tests/lca_data.py) on
every result array, for every named set under every option combination and for 3 000 seeded random sets; lcaout_lines against the
reference CLI's recorded files (tests/golden/lca_golden.json); the ABI surface and every refusal; that the sets reach the cases
they are named after; and that the text does not depend on the order of the hits.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import lca_data as ld

lc = ld.lca_module()


@pytest.fixture(scope="module")
def golden():
    return ld.load_golden()


@pytest.fixture(scope="module")
def sets():
    """every named set with its split and py_lca()'s answer per combination, made once"""
    out = []
    for s in ld.all_sets():
        S = ld.Split(s["tlabels"])
        s = dict(s, split=S, py={combo: ld.py_lca(s["tlabels"], s["qlabels"], s["hits"], *combo, S=S) for combo in ld.COMBOS})
        out.append(s)
    return out


def test_host_is_python_on_every_set(sets):
    for s in sets:
        with lc.LcaIndex(s["tlabels"]) as index:
            assert index.stats["host_no_context"] == 1 and index.stats["labels_host"] == len(s["tlabels"]) and index.stats["labels_device"] == 0
            st, ln = index.split()
            assert [list(map(int, a)) for a in st] == [sp[0] for sp in s["split"].split], s["name"]
            assert [list(map(int, a)) for a in ln] == [sp[1] for sp in s["split"].split], s["name"]
            for combo in ld.COMBOS:
                lines, info = s["py"][combo]
                want = ld.py_arrays(info)
                res = ld.run_set(s, combo, host=True)
                assert res.arrays() == want, (s["name"], combo)
                assert res.stats["queries_host"] == len(s["hits"]) and res.stats["queries_device"] == 0
                assert lc.lcaout_lines(res, s["qlabels"], s["tlabels"]) == lines, (s["name"], combo)
                via = ld.run_set(s, combo, index=index, junk=0xA5)      # prefix numbers instead of bytes; the unread hit fields hold junk
                assert via.arrays() == want, (s["name"], combo)
                assert via.stats["host_no_context"] == 1 and via.stats["hits_host"] == sum(len(h) for h in s["hits"])


def test_host_is_python_on_3000_random_sets():
    seen = set()
    for seed in range(3000):
        s = ld.random_set(seed)
        _, info = ld.py_lca(s["tlabels"], s["qlabels"], s["hits"], *s["combo"])
        assert ld.run_set(s, s["combo"], host=True).arrays() == ld.py_arrays(info), seed
        seen.update((i["depth"], min(i["n_top"], 65)) for i in info)
        if seed % 10 == 0:
            with lc.LcaIndex(s["tlabels"]) as index:
                assert ld.run_set(s, s["combo"], index=index).arrays() == ld.py_arrays(info), seed
    assert {d for d, _ in seen} >= {0, 1, 2, 3, 4, 5, 6, 7, 9} and {n for _, n in seen} >= {1, 2, 3, 65}


def test_lcaout_lines_are_the_recorded_files(golden):
    tl, ql = [l for l, _ in golden["db"]], [l for l, _ in golden["queries"]]
    assert golden["db"] == [list(x) for x in ld.golden_input()[0]] and golden["queries"] == [list(x) for x in ld.golden_input()[1]]
    assert [{k: v for k, v in r.items() if k != "lcaout"} for r in golden["runs"]] == ld.golden_runs()
    seen = 0
    with lc.LcaIndex(tl) as index:
        for r in golden["runs"]:
            hits = ld.golden_hitlists(golden, r["command"])
            raw = ld.make_hits(hits)
            res = lc.lca_host(tl, raw, lca_cutoff=float(r["cutoff"]), maxhits=r["maxhits"], top_hits_only=r["top_hits_only"])
            text = b"".join(lc.lcaout_lines(res, ql, tl)).decode("latin-1")
            via = lc.lca(index, raw, lca_cutoff=float(r["cutoff"]), maxhits=r["maxhits"], top_hits_only=r["top_hits_only"])
            assert via.arrays() == res.arrays()
            if r["command"] == "search_exact":
                # the reference's --search_exact accepts --lcaout and writes no file (commands/search_exact.cpp never calls
                # results_show_lcaout): there is nothing to compare, the text is py_lca()'s
                assert r["lcaout"] is None
                want = b"".join(ld.py_lca(tl, ql, hits, float(r["cutoff"]), r["maxhits"], r["top_hits_only"])[0]).decode("latin-1")
                assert text == want and any(len(h) > 1 for h in hits)
            else:
                assert text == r["lcaout"], r
                seen += 1
    assert seen == 13
    by = {(r["cutoff"], r["maxhits"], r["top_hits_only"]): r["lcaout"] for r in golden["runs"] if r["command"] == "usearch_global"}
    assert len(set(by.values())) >= 6                                                  # the options matter on this input
    assert by[("0.6666666666666666", 0, False)] != by[("0.67", 0, False)] or by[("0.75", 0, False)] != by[("0.51", 0, False)]
    assert "q_none\t\n" in by[("1.0", 0, False)] and "q_b\t\n" in by[("1.0", 0, False)]      # no hits; hits without a full consensus


def test_the_cutoff_fatal_is_the_recorded_message(golden):
    from vsearch_amd import VsxError
    s = ld.all_sets()[0]
    for c in ("0.5", "1.01"):
        assert golden["fatal"][c] == "Fatal error: The argument to lca_cutoff must be larger than 0.5, but not larger than 1.0"
        with pytest.raises(VsxError) as e:
            ld.run_set(s, (float(c), 0, False), host=True)
        assert e.value.code == -1 and golden["fatal"][c].split(": ", 1)[1] in str(e.value)


def test_abi_surface():
    import vsearch_amd
    from vsearch_amd import _lib
    lib = _lib.load()
    for name in _lib.LCA_SYMBOLS:
        assert hasattr(lib, name), name
    for name in ("LcaIndex", "LcaResult", "lca_host", "lcaout_lines"):
        assert hasattr(vsearch_amd, name) and name in vsearch_amd.__all__
    o = _lib.LcaOpts()
    lib.vsx_lca_opts_default(C.byref(o))
    assert (o.lca_cutoff, o.maxhits, o.top_hits_only, o.threads, o.window) == (1.0, 0, 0, 0, 0)
    assert C.sizeof(_lib.LcaOpts) == 32 and C.sizeof(_lib.LcaResult) == 56 and C.sizeof(_lib.LcaStats) == 10 * 8 + 13 * 8
    assert (lc.LEVELS, lc.NONE) == (9, 0xFFFFFFFF)
    res = lc.lca_host(["t;tax=d:A;"], (np.zeros(1, np.uint64), np.zeros(0, ld.hit_dtype())))
    assert res.arrays() == ld.py_arrays([]) and lc.lcaout_lines(res, [], ["t"]) == []
    st = lc.last_stats()
    assert set(st) == {n for n, _ in _lib.LcaStats._fields_} and st["labels"] == 1


def test_refusals():
    from vsearch_amd import VsxError, _lib
    lib = _lib.load()
    labels = ["a;tax=d:A;", "b;tax=d:B;"]
    good = ld.make_hits([[(0, 99.0), (1, 98.0)], []])

    def refused(call):
        with pytest.raises(VsxError) as e:
            call()
        assert e.value.code == -1 and str(e.value).strip()
        return str(e.value)

    for cutoff in (0.5, 0.0, -1.0, 1.0000001, 2.0, float("nan"), float("inf")):
        assert "lca_cutoff" in refused(lambda: lc.lca_host(labels, good, lca_cutoff=cutoff))
        with lc.LcaIndex(labels) as index:
            assert "lca_cutoff" in refused(lambda: lc.lca(index, good, lca_cutoff=cutoff))
    lc.lca_host(labels, good, lca_cutoff=0.5000001)
    refused(lambda: lc.lca_host(labels, good, maxhits=-1))
    refused(lambda: lc.lca_host(labels, good, threads=-1))
    # a hit whose target is not below the number of labels
    assert "target" in refused(lambda: lc.lca_host(labels, ld.make_hits([[(2, 99.0)]])))
    with lc.LcaIndex(labels) as index:
        assert "target" in refused(lambda: lc.lca(index, ld.make_hits([[(2, 99.0)]])))
    # a first that does not ascend to n_hits
    first, hits = good
    for bad in ([0, 1, 1], [1, 2, 2], [0, 3, 2], [0, 2, 1]):
        assert "first" in refused(lambda: lc.lca_host(labels, (np.array(bad, np.uint64), hits)))
    # a label span outside its blob, a label with a NUL byte
    assert "blob" in refused(lambda: lc.LcaIndex(lc.LabelBlob.of(b"abc", [1], [3])))
    assert "blob" in refused(lambda: lc.lca_host(lc.LabelBlob.of(b"abc", [4], [0]), ld.make_hits([[]])))
    assert "NUL" in refused(lambda: lc.LcaIndex([b"a;tax=d:\0A"]))
    assert "NUL" in refused(lambda: lc.lca_host([b"ok", b"\0"], ld.make_hits([[]])))
    # null arguments
    o, out, H = _lib.LcaOpts(), _lib.LcaResult(), _lib.Hits()
    lib.vsx_lca_opts_default(C.byref(o))
    T = lc.LabelBlob(labels)
    ts = T.struct()
    h = C.c_void_p()
    assert lib.vsx_lca_index_create(None, None, C.byref(h)) == -1 and lib.vsx_lca_index_create(None, C.byref(ts), None) == -1
    assert lib.vsx_lca(None, C.byref(o), C.byref(H), C.byref(out)) == -1
    assert lib.vsx_internal_lca_host(None, C.byref(ts), C.byref(H), C.byref(out)) == -1
    assert lib.vsx_internal_lca_host(C.byref(o), None, C.byref(H), C.byref(out)) == -1
    assert lib.vsx_internal_lca_host(C.byref(o), C.byref(ts), None, C.byref(out)) == -1
    assert lib.vsx_internal_lca_host(C.byref(o), C.byref(ts), C.byref(H), None) == -1
    assert lib.vsx_internal_lca_host(C.byref(o), C.byref(ts), C.byref(H), C.byref(out)) == -1      # first is NULL
    with lc.LcaIndex(labels) as index:
        assert lib.vsx_lca(index.h, None, C.byref(H), C.byref(out)) == -1 and lib.vsx_lca(index.h, C.byref(o), None, C.byref(out)) == -1
        assert lib.vsx_lca(index.h, C.byref(o), C.byref(H), None) == -1
    lib.vsx_lca_result_free(None)
    lib.vsx_lca_index_destroy(None)
    lib.vsx_lca_last_stats(None)


def test_the_split_quirks_by_hand():
    """tax_split on the labels the sets are named after, against values worked out by hand"""
    def names(label):
        label = ld.B(label)
        st, ln = ld.py_tax_split(label)
        return {chr(ld.RANKS[k]): label[st[k]:st[k] + ln[k]] for k in range(9) if st[k]}

    assert names("plain") == {} and names("") == {} and names("abcd") == {}
    assert names("s1xtax=d:A;") == {}                                                   # tax= only behind a byte that is no ';'
    assert names("xtax=d:A;tax=d:B,p:Q;") == {"d": b"B", "p": b"Q"}
    assert ld.py_tax_field(b"ab;tax=") == (3, 7) and ld.py_tax_field(b"ab;tax=d") == (3, 8)      # ;tax= in the last 5 bytes, tax= in the last 5
    assert ld.py_tax_field(b"tax=") is None and ld.py_tax_field(b"tax=d") == (0, 5)     # the loop bound: offset < hlen - 4
    assert names("ab;tax=") == {} and names("ab;tax=d") == {} and names("ab;tax=d:") == {"d": b""} and names("ab;tax=d:X") == {"d": b"X"}
    assert names("tax=d:Y") == {"d": b"Y"} and names("tax=;tax=d:Z") == {}              # the first valid tax= wins, however empty
    assert names("xtax=xtax=;tax=d:W") == {"d": b"W"} and names(";tax=d:A") == {"d": b"A"}
    assert names("a;tax=d:A;tax=d:B") == {"d": b"A"}
    assert names("s;tax=d:A,p:B;size=3,x") == {"d": b"A", "p": b"B;size=3"}            # the comma is looked for beyond the field's ';'
    assert names("u;tax=D:A,P:B,G:g") == {"d": b"A", "p": b"B", "g": b"g"}             # tolower on the rank letter
    assert names("r;tax=d:A,d:B,p:C") == {"d": b"B", "p": b"C"}                        # a later field overwrites
    assert names("e;tax=,d:A,,p:P,") == {"d": b"A", "p": b"P"} and names("e;tax=d:A,pp:P,x:Y,t:T") == {"d": b"A", "t": b"T"}
    assert names("e;tax=d:A;p:P,k:K") == {"d": b"A;p:P"}
    ends = {sp[0][0] + sp[1][0] for sp in (ld.py_tax_split(l) for l in ld.lengths_set()[1])}
    assert ends >= {63, 64, 65, 127, 128, 129}
    assert 300 in {sp[1][6] for sp in (ld.py_tax_split(l) for l in ld.lengths_set()[1])}


def test_the_sets_reach_their_cases(sets):
    every = [(s, combo, i, h) for s in sets for combo in ld.COMBOS for i, h in zip(s["py"][combo][1], s["hits"])]
    assert {i["n_top"] for _, _, i, _ in every} >= {0, 1, 2, 3, 63, 64, 65, 129}

    def some(pred):
        return any(pred(s, combo, i, h) for s, combo, i, h in every)

    # m / n exactly on the cutoff
    assert some(lambda s, c, i, h: c[0] == 0.75 and i["n_top"] == 4 and i["level_match"][0] == 3 and i["depth"] >= 1)
    assert some(lambda s, c, i, h: c[0] == 0.6666666666666666 and i["n_top"] == 3 and i["level_match"][0] == 2 and i["depth"] >= 1)
    assert some(lambda s, c, i, h: c[0] == 0.67 and i["n_top"] == 3 and i["level_match"][0] == 2 and i["depth"] == 0)
    assert 1.0 * 2 / 3 >= 0.6666666666666666 and 1.0 * 2 / 3 < 0.67 and 1.0 * 3 / 4 >= 0.75
    # no majority at the first level; a majority at d .. f lost at g; exact halves
    assert some(lambda s, c, i, h: c[0] == 0.51 and i["n_top"] >= 2 and i["depth"] == 0)
    assert some(lambda s, c, i, h: s["name"] == "lost_at_g" and c[0] == 0.51 and i["n_top"] == 3 and i["depth"] == 6)
    assert some(lambda s, c, i, h: i["n_top"] and i["n_top"] % 2 == 0 and i["depth"] < 9 and 2 * i["level_match"][i["depth"]] == i["n_top"])

    # Boyer-Moore's candidate is not the most frequent prefix at the losing level, and nothing of it is in the arrays
    def bm_differs(s, c, i, h):
        d = i["depth"]
        if c != (0.51, 0, False) or d == 0 or d == 9:
            return False
        count = {}
        for t, _ in h[:i["n_top"]]:
            count[s["split"].names[t][:d + 1]] = count.get(s["split"].names[t][:d + 1], 0) + 1
        return i["level_match"][d] < max(count.values()) and i["matches"][d] == 0 and i["target"][d] == ld.NONE
    assert some(bm_differs)
    # the same genus name under two families: the names at g agree for all top hits, the prefixes do not
    assert some(lambda s, c, i, h: s["name"] == "same_genus" and i["n_top"] == 2 and i["depth"] == 5 and
                len({s["split"].names[t][6] for t, _ in h}) == 1 and len({s["split"].names[t][5] for t, _ in h}) == 2)
    # ranks missing in all hits with a printed level behind them; ranks missing in some hits
    assert some(lambda s, c, i, h: any(i["len"][j] == 0 and any(i["len"][k] > 0 for k in range(j + 1, i["depth"])) for j in range(i["depth"])))
    assert some(lambda s, c, i, h: i["n_top"] >= 2 and any(len({len(s["split"].names[t][j]) > 0 for t, _ in h[:i["n_top"]]}) == 2 for j in range(9)))
    # no tax= at all: every level agrees, nothing is printed
    assert some(lambda s, c, i, h: s["name"] == "no_tax" and i["n_top"] == 3 and i["depth"] == 9 and i["text"] == b"")
    # top_hits_only with 1, 2 and all hits tied; unsorted ids; maxhits below the hit count
    ties = {(len(h), i["n_top"]) for s, c, i, h in every if s["name"] == "ties" and c == (0.51, 0, True)}
    assert ties >= {(3, 1), (3, 2), (3, 3), (4, 2), (5, 5), (70, 67)}
    assert some(lambda s, c, i, h: c[1] and not c[2] and i["n_top"] == c[1] < len(h))
    assert some(lambda s, c, i, h: c == (0.75, 3, True) and i["n_top"] < 3 <= len(h))


def test_the_text_does_not_depend_on_the_order_of_the_hits():
    """the order-free rule: all 720 orders of a 6-hit query through the literal loop give one text, at every cutoff"""
    t = [ld.tax("a", d="A", p="P1", c="C1"), ld.tax("b", d="A", p="P1", c="C2"), ld.tax("c", d="A", p="P2"), ld.tax("x", d="X", p="P1")]
    S = ld.Split(t)
    for hits in ([0, 0, 1, 2, 3, 1], [0, 1, 2, 3, 3, 2], [0, 0, 0, 1, 2, 3], [0, 1, 0, 1, 2, 2]):
        for cutoff in ld.CUTOFFS:
            texts = {ld.py_lca_query(S, ld.flat(p), cutoff)["text"] for p in itertools.permutations(hits)}
            assert len(texts) == 1, (hits, cutoff)
            arrays = {ld.py_arrays([ld.py_lca_query(S, ld.flat(p), cutoff)])[:3] for p in itertools.permutations(hits)}
            assert len(arrays) == 1
    res = [ld.run_set({"tlabels": S.labels, "hits": [ld.flat(p) for p in itertools.permutations([0, 0, 1, 2, 3, 1])]}, (0.51, 0, False), host=True)]
    assert len({bytes(r) for r in res[0].matches}) == 1 and set(res[0].depth) == {3}      # d, the missing k, p
