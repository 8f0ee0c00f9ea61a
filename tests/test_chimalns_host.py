"""CPU (-m "not gpu"): the --uchimealns C-ABI without a device -- the host restatement (vsx_internal_chimalns_host) against the
plain-Python restatement of the reference's loops on explicit sets and on seeded random triples, the formatter against the reference
CLI's blocks stored in tests/golden/uchimealns_golden.json, the FASTA writers against its --chimeras / --nonchimeras files, the ABI
surface and the refusals."""
import ctypes as C
import re

import pytest

from tests import chimalns_data as data


@pytest.fixture(scope="module")
def explicit():
    S = dict(data.explicit_sets())
    S.update({k: f() for k, f in data.HOST_ONLY.items()})
    return S


@pytest.fixture(scope="module")
def golden():
    return data.load_golden()


def _same(got, exp, j=0):
    """a ChimeraAlns record against py_uchimealns' answer"""
    assert int(got.alnlen[j]) == exp["alnlen"]
    assert tuple(r.decode("latin-1") for r in got.rows(j)) == exp["rows"]
    assert [tuple(int(x) for x in l) for l in got.lines(j)] == exp["lines"]
    assert int(got.best_i[j]) == exp["best_i"]
    assert float(got.h[j]).hex() == exp["h"].hex()
    assert tuple(int(x) for x in got.counts[j]) == exp["counts"]


def _host_in_record_order(t, **kw):
    """the host restatement takes the parents as the record names them: swapped when the reference's reverse branch wins"""
    from vsearch_amd.chimera import alns_host
    exp = data.py_uchimealns(*t, **{("width" if k == "alignwidth" else k): v for k, v in kw.items()})
    q, a, b, ca, cb = t
    if exp["reverse"]:
        a, b, ca, cb = b, a, cb, ca
    return alns_host(q, a, b, ca, cb, **kw), exp


def test_sets_reach_their_cases():
    data.check_cases()


@pytest.mark.parametrize("width", [1, 60, 80, 0])
def test_host_equals_python_on_explicit_sets(explicit, width):
    for name, t in explicit.items():
        if width == 1 and len(t[0]) > 1000:
            continue                                          # (one line per column: the long sets add nothing at width 1)
        got, exp = _host_in_record_order(t, alignwidth=width)
        _same(got, exp)
        assert got.n == 1 and int(got.record[0]) == 0, name


def test_host_equals_python_on_random_triples():
    triples = data.random_triples(3000)
    reverse = 0
    for k, t in enumerate(triples):
        got, exp = _host_in_record_order(t, alignwidth=(80, 60, 0, 7)[k % 4], xn=(8.0, 6.5)[k % 2], dn=(1.4, 1.1)[k % 2])
        _same(got, exp)
        reverse += exp["reverse"]
    assert 300 < reverse < 2700                             # both orders of the parents are exercised


def test_parents_out_of_order_are_refused(explicit):
    from vsearch_amd import _lib
    from vsearch_amd.chimera import alns_host
    q, a, b, ca, cb = explicit["plain"]
    with pytest.raises(_lib.VsxError, match="reverse branch"):
        alns_host(q, b, a, cb, ca)


def _blocks(text):
    """the blocks of a --uchimealns file: (whole block text, query label, parent A label, parent B label)"""
    parts = text.split("\n" + "-" * 72 + "\n")
    assert parts[0] == ""
    out = []
    for p in parts[1:]:
        m = re.match(r"Query   \( *\d+ nt\) (.*)\nParentA \( *\d+ nt\) (.*)\nParentB \( *\d+ nt\) (.*)\n", p)
        body = p if p.endswith("\n") else p + "\n"
        out.append(("\n" + "-" * 72 + "\n" + body, m.group(1), m.group(2), m.group(3)))
    return out


@pytest.mark.parametrize("name", ["uchime_ref", "uchime", "uchime2", "uchime3"])
def test_formatter_equals_golden_blocks(golden, name):
    """parents from the golden headers, CIGARs from the scalar oracle aligner, record fields from the Python restatement"""
    from oracle import pyoracle
    from vsearch_amd.chimera import alns_host, format_uchimealns
    sets, gold = golden
    s = sets[name]
    orc = pyoracle.Oracle()
    qseq = dict(zip(s["labels"], s["seqs"]))
    tseq = dict(zip(s["db_labels"], s["db"])) if name == "uchime_ref" else qseq
    for width in data.WIDTHS:
        blocks = _blocks(gold[name]["uchimealns"][str(width)])
        assert len(blocks) >= 3
        for text, ql, al, bl in blocks:
            q, a, b = qseq[ql], tseq[al], tseq[bl]
            ca, cb = orc.align(q, a)[5], orc.align(q, b)[5]
            exp = data.py_uchimealns(q, a, b, ca, cb, width=width)
            assert not exp["reverse"]                      # the headers name the parents after the flip
            got = alns_host(q, a, b, ca, cb, alignwidth=width)
            _same(got, exp)
            assert format_uchimealns(got, 0, exp["rec"], ql, len(q), [al, bl], [len(a), len(b)]) == text


@pytest.mark.parametrize("name", ["uchime_ref", "uchime", "uchime2", "uchime3"])
def test_fasta_writers_equal_golden_files(golden, name):
    """flags and scores read back from the golden headers; what is under test is the header, the numbering and the folding"""
    from vsearch_amd.chimera import chimera_fasta, chimera_summary, header_size, sort_by_abundance
    sets, gold = golden
    s = sets[name]
    labels, seqs = s["labels"], s["seqs"]
    if name != "uchime_ref":
        order = sort_by_abundance([header_size(l) for l in labels], labels)
        labels, seqs = [labels[i] for i in order], [seqs[i] for i in order]
        # the de novo forms print the sequences as DUST left them (the session takes them from the device masker)
        from vsearch_amd.mask import fastx_mask_host
        seqs = [t.decode() for t in fastx_mask_host(seqs, qmask="dust", want_bits=False).text()]
    score_name = "uchime_ref" if name == "uchime_ref" else "uchime_denovo"
    verdict = {}
    for flag, key in (("Y", "chimeras"), ("N", "nonchimeras"), ("?", "borderline")):
        for line in gold[name][key].splitlines():
            if line.startswith(">"):
                head, score = line[1:].rsplit(f";{score_name}=", 1)
                verdict[head] = (flag, float(score))
    from vsearch_amd.derep import strip_size
    sizes = [header_size(l) for l in labels]
    recs = []
    for l, z in zip(labels, sizes):
        flag, score = verdict[strip_size(l)[0] + f";size={z}"]
        recs.append(dict(flag=flag, score=score))
    for flag, key in (("Y", "chimeras"), ("N", "nonchimeras"), ("?", "borderline")):
        got = chimera_fasta(recs, labels, seqs, sizes, flag, score_name, sizeout=True)
        assert "".join(l + "\n" for l in got) == gold[name][key], key
    sm = chimera_summary(recs, sizes)
    assert sm["chimeras"] == gold[name]["chimeras"].count(">") and sm["nonchimeras"] == gold[name]["nonchimeras"].count(">")
    assert sm["chimera_abundance"] + sm["nonchimera_abundance"] + sm["borderline_abundance"] == sm["total_abundance"] == sum(sizes)
    # relabel numbers per file; xsize strips; a trailing separator is not doubled
    got = chimera_fasta(recs, labels, seqs, sizes, "Y", None, relabel="c", fasta_width=0)
    assert got[0] == ">c1" and got[2] == ">c2" and len(got) == 2 * sm["chimeras"]
    assert chimera_fasta([dict(flag="Y", score=-1.0)], ["x;size=3;"], ["ACGT"], [3], "Y", "uchime_ref") == [">x;size=3;uchime_ref=0.0000", "ACGT"]
    assert chimera_fasta([dict(flag="Y", score=0.5)], ["x;size=3;"], ["ACGT"], [3], "Y", "uchime_ref", xsize=True) == [">x;uchime_ref=0.5000", "ACGT"]


def test_abi_surface_and_refusals(explicit):
    from vsearch_amd import _lib
    from vsearch_amd.chimera import alns_host
    lib = _lib.load()
    for sym in _lib.CHIMALNS_SYMBOLS:
        assert hasattr(lib, sym)
    o = _lib.ChimalnsOpts()
    lib.vsx_chimalns_opts_default(C.byref(o))
    assert (o.xn, o.dn, o.alignwidth, o.select, o.window, o.threads) == (8.0, 1.4, 80, _lib.CHIMALNS_Y, 0, 0)
    assert C.sizeof(_lib.ChimalnsOpts) == 40 and C.sizeof(_lib.ChimalnsOut) == 96 and C.sizeof(_lib.ChimalnsStats) == 104
    q, a, b, ca, cb = explicit["plain"]
    for kw, text in ((dict(xn=0.0), "xn"), (dict(dn=-1.0), "dn"), (dict(alignwidth=-1), "alignwidth")):
        with pytest.raises(_lib.VsxError, match=text):
            alns_host(q, a, b, ca, cb, **kw)
    with pytest.raises(_lib.VsxError, match="span"):
        alns_host(q, a, b, "119M", cb)
    with pytest.raises(_lib.VsxError, match="span"):
        alns_host(q, a, b, "60M2I1I60M", cb)                 # adjacent target-only runs: not an alignment the aligner writes
    with pytest.raises(_lib.VsxError, match="no column"):
        alns_host(q, q, q, "120M", "120M")
    # the command refuses its options before it looks at the searcher, and a null searcher after
    res = _lib.ChimalnsOut()
    o.select = 8
    assert lib.vsx_chimera_alns(None, C.byref(o), 0, None, 0, None, None, None, C.byref(res)) == _lib.VSX_EINVAL
    assert b"select" in lib.vsx_last_error()
    o.select = 0
    assert lib.vsx_chimera_alns(None, C.byref(o), 0, None, 0, None, None, None, C.byref(res)) == _lib.VSX_EINVAL
    lib.vsx_chimalns_out_free(C.byref(res))


def test_uchimeout_strips_the_size_annotation_under_xsize(tmp_path):
    """found by oracle/soak_chimera.py --outputs alns: with --xsize the reference prints all four labels of a --uchimeout line
    without their ;size= annotation (header_fprint_strip); format_uchimeout and the sessions' uchimeout() took no xsize.  The
    "no parents" lines are held against the reference CLI's own for the de novo set where its binary is present."""
    from oracle import refcli
    from vsearch_amd.chimera import format_uchimeout
    rec = dict(status="scored", score=1.25, parent_a=0, parent_b=1, closest=1, id_query_model=99.0, id_query_a=95.5, id_query_b=96.0, id_a_b=92.0,
               id_query_top=96.0, left_yes=5, left_no=0, left_abstain=1, right_yes=4, right_no=1, right_abstain=0, divergence=3.0, flag="Y")
    names = ["a;size=9", "b;size=7;"]
    tail = "\t99.0\t95.5\t96.0\t92.0\t96.0\t5\t0\t1\t4\t1\t0\t3.0\tY"
    assert format_uchimeout(rec, "q;size=3", names) == "1.2500\tq;size=3\ta;size=9\tb;size=7;\tb;size=7;" + tail
    assert format_uchimeout(rec, "q;size=3", names, xsize=True) == "1.2500\tq\ta\tb\tb" + tail
    none = dict(rec, status="no_parents")
    assert format_uchimeout(none, "q;size=3", names, xsize=True).startswith("0.0000\tq\t*\t")
    if refcli.available():
        labels, seqs = data.denovo_set()
        f, out = str(tmp_path / "in.fa"), str(tmp_path / "u.tsv")
        refcli.write_fasta(f, labels, seqs)
        refcli.run(["--uchime_denovo", f, "--uchimeout", out, "--xsize", "--threads", "1", "--quiet"])
        lines = open(out).read().splitlines()
        assert len(lines) == len(labels) and not any(";size=" in l for l in lines)
        plain = [l for l in lines if l.split("\t")[2] == "*"]
        assert len(plain) >= 3 and set(plain) <= {format_uchimeout(none, l, labels, xsize=True) for l in labels}
