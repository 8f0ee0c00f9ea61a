"""CPU (-m "not gpu"): the de novo chimera C-ABI and its Python layer -- option defaults per variant, size= parsing, the
sortbyabundance order, the refusals that need no device, and the stored golden file's shape."""
import ctypes as C
import json

from tests import denovo_data


def test_denovo_opts_defaults():
    from vsearch_amd import _lib
    from vsearch_amd.chimera import denovo_default_opts
    for variant, num, abskew in (("uchime", 1, 2.0), ("uchime2", 2, 2.0), ("uchime3", 3, 16.0)):
        o = denovo_default_opts(variant)
        assert o.variant == num and o.abskew == abskew
        # chimera_detection_parameters (core/chimera.cpp:2805-2824) for the de novo forms
        assert (o.base.search.self, o.base.search.selfid, o.base.search.maxsizeratio) == (1, 1, 1.0 / abskew)
        assert (o.base.search.id, o.base.search.weak_id, o.base.search.maxaccepts, o.base.search.maxrejects) == (0.55, 0.55, 4, 16)
        assert (o.base.minh, o.base.mindiv, o.base.mindiffs, o.base.xn, o.base.dn) == (0.28, 0.8, 3, 8.0, 1.4)
        assert o.base.search.soft_mask == 2 and o.base.search.strand_both == 0 and o.base.window == 0
    assert C.sizeof(_lib.ChimeraDenovoOpts) == C.sizeof(_lib.ChimeraOpts) + 16
    lib = _lib.load()
    for s in ("vsx_uchime_denovo", "vsx_chimera_denovo_opts_default", "vsx_chimera_denovo_last_stats"):
        assert hasattr(lib, s)


def test_header_size():
    from vsearch_amd.chimera import header_size
    assert header_size("a;size=12") == 12
    assert header_size("size=5;x") == 5
    assert header_size("a;size=12;") == 12
    assert header_size("a") == 1
    assert header_size("abcsize=7") == 1                       # not after ';'
    assert header_size("a;size=7x;size=9") == 9                # digits must end the attribute
    assert header_size("a;size=;size=3") == 3
    assert header_size("a;size=40;b;size=2") == 40             # the first one


def test_sort_by_abundance_ties():
    from vsearch_amd.chimera import header_size, sort_by_abundance
    labels = ["b;size=7", "a;size=7", "tie;size=7", "z;size=70", "tie;size=7", "a;size=7", "c"]
    sizes = [header_size(x) for x in labels]
    # abundance descending, then strcmp of the header, then input order
    assert sort_by_abundance(sizes, labels) == [3, 1, 5, 0, 2, 4, 6]
    assert sort_by_abundance([1, 1], ["B", "a"]) == [0, 1]            # strcmp: 'B' (0x42) < 'a' (0x61)


def test_refusals_without_device():
    from vsearch_amd import _lib
    from vsearch_amd.chimera import denovo_default_opts
    lib = _lib.load()
    lib.vsx_last_error.restype = C.c_char_p
    out = (_lib.ChimeraResult * 1)()
    o = denovo_default_opts("uchime")
    assert lib.vsx_uchime_denovo(None, C.byref(o), out) == _lib.VSX_EINVAL
    assert b"null argument" in lib.vsx_last_error()
    assert lib.vsx_uchime_denovo(None, None, out) == _lib.VSX_EINVAL
    for field, value, msg in (("variant", 4, b"variant"), ("abskew", 0.5, b"abskew")):
        o = denovo_default_opts("uchime")
        setattr(o, field, value)
        assert lib.vsx_uchime_denovo(None, C.byref(o), out) == _lib.VSX_EINVAL
        assert msg in lib.vsx_last_error()
    o = denovo_default_opts("uchime")
    o.base.xn = 0.0
    assert lib.vsx_uchime_denovo(None, C.byref(o), out) == _lib.VSX_EINVAL


def test_golden_file_shape():
    """the stored reference lines: processing order = the sortbyabundance order of the stored input"""
    from vsearch_amd.chimera import header_size, sort_by_abundance
    g = json.load(open(denovo_data.GOLDEN))
    labels = g["labels"]
    order = sort_by_abundance([header_size(x) for x in labels], labels)
    for variant in ("uchime", "uchime2", "uchime3"):
        lines = g["uchimeout"][variant]
        assert [ln.split("\t")[1] for ln in lines] == [labels[i] for i in order]
        flags = {ln.rsplit("\t", 1)[1] for ln in lines}
        assert "Y" in flags
        if variant != "uchime":
            assert "?" not in flags                               # uchime2 / uchime3 never call a query suspicious
