"""The search hit writers without a GPU: the library's host restatement of vsx_hits_render against the plain-Python restatement of
tests/hitout_data.py, field for field and byte for byte, on every explicit set and on 3 000 seeded random (query, target, CIGAR)
triples; every formatter of vsearch_amd.hitout against the reference CLI's recorded files; the ABI surface and the refusals.
"""
import ctypes as C

import numpy as np
import pytest

from tests import hitout_data as hd
from vsearch_amd import VsxError, _lib
from vsearch_amd import hitout as ho


@pytest.fixture(scope="module")
def golden():
    return hd.load_golden()


def assert_host_is_py(s, want=ho.ALL):
    py = hd.py_render(s)
    st = hd.strands(s)
    r = hd.render_explicit(None, s, want=want, host=True)
    assert r.stats["host_no_context"] == 1 and r.stats["hits_host"] == len(py) and r.stats["hits_device"] == 0
    assert [int(x) for x in r.row_len] == [p["ilen"] for p in py]
    for q, (plus, minus) in enumerate(st):
        assert r.qstrand(q) == plus and (minus is None or r.qstrand(q, True) == minus), (s["name"], q)
    for h, p in enumerate(py):
        if want & ho.ROWS:
            assert (r.qrow(h), r.trow(h)) == (p["qrow"], p["trow"]), (s["name"], h)
        if want & ho.SYMBOLS:
            assert (r.symbols(h), r.alnrow(h)) == (p["sym"], p["aln"]), (s["name"], h)
            if want & ho.ROWS and not s["hits"][h][2]:
                assert r.aln_off[h] == r.qrow_off[h]                           # a plus-strand hit shares one row for both
        if want & ho.SAM:
            assert r.md(h) == p["md"], (s["name"], h)
    return r


def test_the_sets_reach_what_they_must():
    hd.assert_coverage()


@pytest.mark.parametrize("s", hd.explicit_sets(), ids=lambda s: s["name"])
def test_host_restatement_equals_python(s):
    assert_host_is_py(s)


def test_host_restatement_equals_python_on_random_triples():
    assert_host_is_py(hd.random_triples(457, 3000))


@pytest.mark.parametrize("want", (0, ho.ROWS, ho.SYMBOLS, ho.SAM))
def test_nothing_is_made_for_a_bit_that_is_not_set(want):
    r = assert_host_is_py(hd.gaps_set(), want=want)
    assert (r.qrow_off is None) == (r.trow_off is None) == (not want & ho.ROWS)
    assert (r.sym_off is None) == (r.aln_off is None) == (not want & ho.SYMBOLS)
    assert (r.md_off is None) == (r.md_len is None) == (not want & ho.SAM) and (r.md_blob == b"" or want & ho.SAM)
    per_hit = 2 * bool(want & ho.ROWS) + 2 * bool(want & ho.SYMBOLS)
    assert len(r.row_blob) == per_hit * int(r.row_len.sum())


def test_every_formatter_equals_the_recorded_files(golden):
    assert [g["name"] for g in golden] == [s["name"] for s in hd.cli_sets()]
    for s in golden:
        o = hd.full_opts(s["opts"])
        records = hd.hits_from_records(s, s["ref"]["records"])
        raw = hd.raw_hits(len(s["queries"]), records)
        text = ho.render_host(hd.db_text(s), s["queries"], raw, n_mismatch=bool(o["n_mismatch"]), **hd.session_opts(s["opts"]))
        got = hd.format_all(text, s)
        assert set(hd.WRITERS) <= set(s["ref"]) and ("userout_reversed" in s["ref"]) == (s["name"] == "exact")
        for name, body in got.items():
            assert name not in s["ref"] or body == s["ref"][name], (s["name"], name)
        assert hd.sam_header_of(text, s, s["ref"]["samheader"]) == s["ref"]["samheader"], s["name"]


def test_the_recorded_sets_reach_the_layout_cases(golden):
    by = {s["name"]: s for s in golden}
    plain = by["plain"]["ref"]
    widths = {len(l.split()[1]) - 2 for l in (plain["alnout"] + by["long"]["ref"]["alnout"]).splitlines() if l.startswith((" Query ", "Target "))}
    assert {2, 3, 4} <= widths                                                     # number widths of the "nt >" lines
    cols = [int(l.split()[0]) for l in plain["alnout"].splitlines() if " cols, " in l]
    assert any(c % 64 == 0 for c in cols)                                          # a last block of exactly rowlen columns
    assert {by[n]["fmt"].get("rowlen", 64) for n in by} >= {0, 1, 64}
    recs = hd.hits_from_records(by["plain"], plain["records"])
    ties = [(a, b) for a, b in zip(recs, recs[1:]) if a["query"] == b["query"]]
    assert any(a["id"] == b["id"] for a, b in ties) and any(a["id"] > b["id"] for a, b in ties)          # tied and untied second hits
    assert "No hits" in by["plain_no_hits"]["ref"]["alnout"] and "No hits" not in plain["alnout"]
    assert any(l.split("\t")[1] == "4" for l in by["plain_no_hits"]["ref"]["samout"].splitlines())
    assert any(l.split("\t")[1] in ("16", "272") for l in plain["samout"].splitlines())                    # minus-strand hits


def test_abi_surface():
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in _lib.HITOUT_SYMBOLS)
    o = _lib.HitoutOpts()
    lib.vsx_hitout_opts_default(C.byref(o))
    assert (o.want, o.threads, o.window) == (7, 0, 0)
    assert C.sizeof(_lib.HitoutOpts) == 16 and C.sizeof(_lib.HitText) == 8 * 18 and C.sizeof(_lib.HitoutStats) == 8 * 17
    assert (ho.ROWS, ho.SYMBOLS, ho.SAM) == (1, 2, 4)


def refused(db, queries, records, first=None, cigar_blob=None, **kw):
    raw = list(hd.raw_hits(len(queries) if isinstance(queries, list) else len(queries[2]), records))
    if first is not None:
        raw[0] = np.asarray(first, np.uint64)
    if cigar_blob is not None:
        raw[2] = cigar_blob
    with pytest.raises(VsxError) as e:
        ho.render_host(db, queries, tuple(raw), soft_mask=0, **kw)
    assert e.value.code == _lib.VSX_EINVAL
    return str(e.value)


def test_refusals():
    db, qs = ["ACGTACGT"], ["ACGTACG"]
    ok = hd.hit_record(0, 0, 0, "7MI", 7, 8, 7, 0)
    ho.render_host(db, qs, hd.raw_hits(1, [ok]), soft_mask=0)
    assert "target" in refused(db, qs, [dict(ok, target=1)])
    refused(db, qs, [ok], first=[1, 1])                                              # first does not start at 0
    refused(db, qs + ["AC"], [dict(ok, query=0)], first=[0, 0, 1])                   # listed under query 1, names query 0
    assert "sum" in refused(db, qs, [dict(ok, cigar="7M")])                          # the target has 8 symbols
    assert "sum" in refused(db, qs, [dict(ok, cigar="8MI")])
    refused(db, qs, [dict(ok, cigar="7MX")])                                         # an unknown operation
    refused(db, qs, [dict(ok, cigar="7M0D1I")])                                      # an empty run
    raw = hd.raw_hits(1, [ok])
    refused(db, qs, [ok], cigar_blob=raw[2][:-1])                                    # no terminator inside the blob
    hits = raw[1].copy()
    hits[0]["cigar_off"] = len(raw[2])
    with pytest.raises(VsxError):
        ho.render_host(db, qs, (raw[0], hits, raw[2]), soft_mask=0)
    assert "trimmed" in refused(db, qs, [dict(ok, internal_alignmentlength=9)])
    assert "strand" in refused(db, qs, [dict(ok, strand=1)], strand_both=0)
    refused(db, (b"ACGTACG", [1], [7]), [ok])                                        # the query lies outside its blob
    refused(db, qs, [ok], first=[0, 2])                                              # first does not end at n_hits
    with pytest.raises(VsxError):
        ho.render_host(db, qs, hd.raw_hits(1, [ok]), want=8, soft_mask=0)
