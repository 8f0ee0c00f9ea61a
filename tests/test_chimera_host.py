"""CPU (-m "not gpu"): the --uchime_ref C-ABI and its Python layer -- defaults, record layout, --uchimeout line formatting."""
import ctypes as C
import json
import os

from tests import common


def test_chimera_opts_defaults():
    from vsearch_amd import _lib
    from vsearch_amd.chimera import default_opts
    o = default_opts()
    # src/vsearch.h:420-484 and chimera_detection_parameters (core/chimera.cpp:2805-2824)
    assert (o.minh, o.mindiv, o.mindiffs, o.xn, o.dn) == (0.28, 0.8, 3, 8.0, 1.4)
    assert (o.search.id, o.search.weak_id, o.search.maxaccepts, o.search.maxrejects) == (0.55, 0.55, 4, 16)
    assert o.search.soft_mask == 2 and o.search.strand_both == 0 and o.window == 0 and o.search.window == 0
    assert C.sizeof(_lib.ChimeraResult) == 104
    lib = _lib.load()
    for s in ("vsx_uchime_ref", "vsx_chimera_last_stats"):
        assert hasattr(lib, s)


def test_uchimeout_lines_from_records():
    """the golden file's lines rebuilt from records: scored lines (chimera.cpp:1810-1875), "no parents" lines (:2320-2340)"""
    from vsearch_amd.chimera import format_uchimeout
    gold = json.load(open(os.path.join(common.GOLD, "chimera_golden.json")))
    names = gold["db_order"]
    for line in gold["uchimeout"]:
        f = line.split("\t")
        if f[2] == "*":
            rec = {"status": "no_parents"}
        else:
            rec = dict(status="scored", score=float(f[0]), parent_a=names.index(f[2]), parent_b=names.index(f[3]),
                       closest=names.index(f[4]), id_query_model=float(f[5]), id_query_a=float(f[6]), id_query_b=float(f[7]),
                       id_a_b=float(f[8]), id_query_top=float(f[9]), left_yes=int(f[10]), left_no=int(f[11]), left_abstain=int(f[12]),
                       right_yes=int(f[13]), right_no=int(f[14]), right_abstain=int(f[15]), divergence=float(f[16]), flag=f[17])
        assert format_uchimeout(rec, f[1], names) == line
    # %.1f rounds the double's exact binary value, as C's printf does
    assert format_uchimeout(dict(status="scored", score=0.28, parent_a=0, parent_b=1, closest=1, id_query_model=99.25,
                                 id_query_a=0.05, id_query_b=84.65, id_a_b=70.0, id_query_top=84.65, left_yes=3, left_no=0,
                                 left_abstain=1, right_yes=4, right_no=1, right_abstain=0, divergence=-0.05, flag="?"),
                            "q", ["a", "b"]) == "0.2800\tq\ta\tb\tb\t99.2\t0.1\t84.7\t70.0\t84.7\t3\t0\t1\t4\t1\t0\t-0.1\t?"
