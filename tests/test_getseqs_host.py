"""Sequence extraction by label without a GPU: the library's host restatement (vsx_getseqs without a context) against py_getseqs(),
the literal loops of the reference, record for record on every set of tests/getseqs_data.py and on 3 000 seeded random draws; the
writers and read_labels() against what the reference CLI recorded; the ABI surface, every refusal and the host-route counters; and
that every set reaches the case it is named after.
"""
import ctypes as C
import importlib
import os
import random

import numpy as np
import pytest

from tests import getseqs_data as gd

gs = importlib.import_module("vsearch_amd.getseqs")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ("host_no_context", "host_environment", "host_count", "host_memory", "host_needle_length", "host_header_length", "host_lengths")


@pytest.fixture(scope="module")
def host_results():
    """the host restatement of every set, computed once"""
    return {s["name"]: gd.call(None, s) for s in gd.sets()}


def test_host_is_py_on_every_set(host_results):
    for s in gd.sets():
        res = host_results[s["name"]]
        gd.assert_equals_py(res, s)
        st = res.stats
        assert {r: st[r] for r in ROUTES} == dict({r: 0 for r in ROUTES}, host_no_context=1), s["name"]
        assert st["headers_host"] == len(s["headers"]) and st["headers_device"] == 0
        empty = s["needles"] == [b""] and s["substr"]
        assert st["labels_in_table"] == (0 if empty else len(s["needles"]))
        assert st["distinct_lengths"] == (0 if empty else len({len(n) + (len(s["field"]) + 1 if s["field"] is not None else 0) for n in s["needles"]}))
        assert st["table_slots"] >= max(64, 2 * len(s["needles"])) and st["table_slots"] & (st["table_slots"] - 1) == 0


def test_host_threads_and_cut_hashes_do_not_show(monkeypatch):
    for name in ("list_1000_substr", "lengths_300_words", "word_boundaries", "folding_labels", "list_33_exact"):
        s = gd.by_name(name)
        want = gd.call(None, s)
        assert gd.call(None, s, threads=1).arrays() == want.arrays() == gd.call(None, s, threads=16).arrays()
        for bits in ("3", "1"):
            with monkeypatch.context() as m:
                m.setenv("VSX_GETSEQS_HASH_BITS", bits)
                cut = gd.call(None, s)
            assert cut.arrays() == want.arrays(), (name, bits)
            assert cut.stats["verifications"] >= want.stats["verifications"]


def test_three_thousand_random_draws():
    rng = random.Random(20261020)
    seen = set()
    for i in range(3000):
        h, lens, mode, needles, substr, field, subseq = gd.random_draw(rng)
        kw = dict(substr=substr, field=field)
        if subseq:
            kw.update(subseq_start=subseq[0], subseq_end=subseq[1])
        res = gs.getseqs_host(h, np.array(lens, np.uint32), mode, needles[0] if mode in gd.SINGLE else needles, **kw)
        exp = gd.py_getseqs(h, lens, mode, needles, substr, field, subseq)
        assert [res.record(k) for k in range(res.n)] == exp["records"], (i, h, mode, needles, substr, field, subseq)
        assert (res.kept, res.discarded) == (exp["kept"], exp["discarded"])
        if exp["kept"] and exp["discarded"]:
            seen.add((mode, field is not None if mode.startswith("label_word") else bool(substr)))
    assert len(seen) == 8, seen                                   # every row of the mode table with both verdicts in one call


def test_writers_against_the_recorded_cli(host_results):
    golden = gd.load_golden()
    assert sorted(golden) == sorted(s["name"] for s in gd.sets() if s["cli"])
    for s in gd.sets():
        if s["cli"]:
            gd.assert_text_equals_golden(host_results[s["name"]], s)
    s = gd.by_name("subseq_3_10")                                  # the qualities are cut with the sequence's offset
    fq = gs.fastq_lines(host_results[s["name"]], s["headers"], s["seqs"], s["quals"])
    assert fq[1] == s["seqs"][0][2:10] and fq[3] == s["quals"][0][2:10] and fq[3] != s["quals"][0][:8]
    with pytest.raises(ValueError):
        gs.fastq_lines(host_results[s["name"]], s["headers"], s["seqs"], None)


def test_sizeout_prints_the_annotation_without_sizein():
    """found by oracle/soak_commands.py --command getseqs: the three commands hand the writers fastx_get_abundance(), which reads
    the header's ;size= annotation whether or not --sizein is given; sizes_of() used to give 1 without --sizein.  The expected
    text is the reference CLI's own for this input, with and without --sizein."""
    want = dict(fastaout=[">a;size=5", "AC"], notmatched=[">b;size=1", "CGT"])
    for sizein in (False, True):
        s = gd._set("annotated", [b"a;size=5", b"b"], "label", b"A;SIZE=5", seq_lengths=[2, 3], sizeout=True, sizein=sizein)
        assert gd.sizes_of(s) == [5, 1]
        got = gd.texts(gd.call(None, s), s)
        assert {k: got[k] for k in want} == want
        if os.path.exists(gd.ref_binary()):
            ref = gd.run_reference(s)
            assert {k: gd.as_lines(ref[k]) for k in want} == want


def test_log_line_without_sequences():
    res = gs.getseqs_host([], [], "labels", [b"x"])
    assert gs.log_lines(res) == ["0 of 0 sequences extracted"] and res.n == 0 and res.arrays()[4:] == (0, 0)


def test_read_labels(tmp_path):
    golden = gd.load_golden()
    raws = {s["name"]: s["raw"] for s in gd.sets() if s["raw"] is not None and s["cli"]}
    raws.update(nul=b"ab\0cd\nef\n", only_newlines=b"\n\n\n", empty=b"", two_pieces_and_newline=gd.wx(2046) + b"\n", exact_1022=gd.wx(1022) + b"\nq",
                cr_only=b"\r\n\r\n")
    for name, raw in raws.items():
        path = tmp_path / "labels.txt"
        path.write_bytes(raw)
        labels, warn = gs.read_labels(str(path))
        assert (labels, warn) == gd.py_read_labels(raw), name
        if name in golden:
            assert warn == golden[name]["warned"], name
    long = gd.py_read_labels(gd.by_name("labels_1500_byte_line")["raw"])
    assert [len(l) for l in long[0]] == [1023, 477] and long[1]
    assert gd.py_read_labels(gd.by_name("labels_1023_with_newline")["raw"]) == ([gd.wx(1023), b"abc"], True)
    assert gd.py_read_labels(gd.by_name("labels_1023_without_newline")["raw"]) == ([b"def", gd.wx(1023)], True)
    assert gd.py_read_labels(gd.by_name("labels_empty_lines")["raw"]) == ([b"abc", b"def"], False)
    assert gd.py_read_labels(gd.by_name("labels_crlf")["raw"]) == ([b"abc\r", b"def\r"], False)
    assert gd.py_read_labels(b"ab\0cd\nef\n") == ([b"ab", b"ef"], False)
    assert gd.py_read_labels(gd.wx(1022) + b"\nq") == ([gd.wx(1022), b"q"], False)


def test_abi_surface():
    from vsearch_amd import _lib
    lib = _lib.load()
    for name in _lib.GETSEQS_SYMBOLS:
        assert hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "vsx_getseqs.h")).read()
    for name in _lib.GETSEQS_SYMBOLS + ["vsx_getseqs_opts", "vsx_getseqs_record", "vsx_getseqs_out", "vsx_getseqs_stats"]:
        assert name in text, name
    for field, _ in _lib.GetseqsStats._fields_ + _lib.GetseqsOpts._fields_ + _lib.GetseqsOut._fields_:
        assert field in text, field
    o = _lib.GetseqsOpts()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    lib.vsx_getseqs_opts_default(C.byref(o))
    assert (o.mode, o.substr, o.field, o.field_len, o.subseq_start, o.subseq_end, o.window, o.threads) == (gs.LABELS, 0, None, 0, 0, 0, 0, 0)
    assert C.sizeof(_lib.GetseqsOpts) == 56 and C.sizeof(_lib.GetseqsOut) == 32 and C.sizeof(_lib.GetseqsStats) == 6 * 8 + 14 * 8
    for name in ("getseqs", "getseq", "getsubseq", "getseqs_host", "read_labels"):
        assert callable(getattr(importlib.import_module("vsearch_amd"), name))


def refused(*a, **kw):
    from vsearch_amd import VsxError
    with pytest.raises(VsxError) as e:
        gs.getseqs_host(*a, **kw)
    assert e.value.code == -1, e.value
    return str(e.value)


def test_refusals():
    H, L = [b"abc", b"de"], [3, 2]
    refused(H, L, "label_word", b"")                               # an empty needle in a word mode
    refused(H, L, "label_words", [b"a", b""])
    refused(H, L, "label_word", b"", field="f")
    refused(H, L, "labels", gs.LabelBlob.of(b"ab", [0, 1], [1, 0]))          # an empty label inside a list
    refused(H, L, "labels", gs.LabelBlob.of(b"ab", [0, 1], [1, 0]), substr=True)
    refused(H, L, "label", b"a\0b")                                # NUL bytes
    refused(H, L, "labels", [b"ok", b"\0"])
    refused(H, L, "label_word", b"a", field=b"f\0")
    refused(H, L, 4, b"a")                                         # unknown mode and flag
    refused(H, L, -1, b"a")
    refused(H, L, "label", b"a", substr=2)
    refused(H, L, "label", gs.LabelBlob([b"a", b"b"]))             # the single-needle modes take one needle
    refused(H, L, "label_word", gs.LabelBlob([]))
    refused(H, L, "label", b"a", window=-1)
    refused(H, L, "label", b"a", threads=-1)
    refused(gs.LabelBlob.of(b"abc", [1], [3]), [3], "label", b"a")            # spans outside their blob
    refused(gs.LabelBlob.of(b"abc", [4], [0]), [3], "label", b"a")
    refused(H, L, "labels", gs.LabelBlob.of(b"abc", [2], [2]))
    assert "must be at least 1" in refused(H, L, "label", b"a", subseq_start=0, subseq_end=3)
    assert "must be at least 1" in refused(H, L, "label", b"a", subseq_start=1, subseq_end=0)
    assert "must be at least 1" in refused(H, L, "label", b"a", subseq_start=-2, subseq_end=3)
    assert "equal or less" in refused(H, L, "label", b"a", subseq_start=3, subseq_end=2)
    with pytest.raises(ValueError):
        gs.getseqs_host(H, [3], "label", b"a")
    assert gs.getseqs_host(H, L, "labels", []).arrays()[4:] == (0, 2)         # an empty list matches nothing
    assert gs.getseqs_host(H, L, "label_words", [], field="x").arrays()[4:] == (0, 2)
    assert gs.getseqs_host(H, L, "label", b"ABC", field="ignored").kept == 1  # field is ignored by LABEL / LABELS
    assert gs.getseqs_host(H, L, "label_word", b"abc", substr=True).kept == 1 and gs.getseqs_host(H, L, "label_word", b"ab", substr=True).kept == 0


def test_host_counter_without_context_wins_over_the_environment(monkeypatch):
    monkeypatch.setenv("VSX_GETSEQS", "host")
    st = gd.call(None, gd.by_name("prefix_words")).stats
    assert {r: st[r] for r in ROUTES} == dict({r: 0 for r in ROUTES}, host_no_context=1)
    assert st["seconds_total"] >= st["seconds_match"] >= 0 and st["probes"] > 0


def matched(name):
    return [r[0] for r in gd.expected(gd.by_name(name))["records"]]


def test_every_set_reaches_its_case():
    S = gd.by_name
    assert sorted({len(h) for h in S("header_lengths_substr")["headers"]}) == list(gd.HEADER_LENGTHS)
    for name in ("header_lengths_substr", "header_lengths_exact", "header_lengths_words"):
        lens = {len(h) for h, m in zip(S(name)["headers"], matched(name)) if m}
        assert lens >= ({1, 64, 1000} if name.endswith("exact") else set(gd.HEADER_LENGTHS)), name
        assert 0 in matched(name)
    assert matched("empty_header") == [0, 1, 0, 0] and matched("empty_header_exact_empty_needle") == [1, 0, 1]
    assert matched("empty_header_empty_substr") == [0, 1, 0, 1] and matched("empty_substr_needle") == [1, 1, 1, 1]
    assert [len(n) for n in S("needle_lengths_substr")["needles"]] == list(gd.NEEDLE_LENGTHS)
    for name in ("needle_lengths_substr", "needle_lengths_exact", "needle_lengths_words"):
        m, hs = matched(name), S(name)["headers"]
        for j, n in enumerate(gd.NEEDLE_LENGTHS[:len(hs) // 6]):
            assert len(hs[6 * j + 1]) == n and m[6 * j + 1] == 1, (name, n)      # a needle equal to the whole header
    assert matched("needle_lengths_exact")[32] == 0 and len(S("needle_lengths_exact")["headers"][32]) == 1022   # a needle longer than its header
    assert matched("needle_lengths_words")[6 * 3 + 4] == 0 and matched("needle_lengths_words")[6 * 3 + 5] == 1               # ...X refused, _..._ accepted (64 bytes)
    assert matched("positions_label_substr") == [1, 1, 1, 1, 1, 0, 0] == matched("positions_labels_substr")
    assert [h.find(b"WXYZW") for h in S("positions_word")["headers"][:5]] == [0, 62, 63, 64, 135] and len(S("positions_word")["headers"][4]) == 140
    assert matched("positions_word") == [0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 1, 1] and matched("positions_words") == [1, 1, 1, 1, 1, 0, 1, 1]
    assert matched("folding_label") == [1, 1] + [0] * 10
    assert matched("folding_labels") == [1, 1, 0, 0, 0, 0, 1, 1, 0, 1, 1, 1, 1, 0, 0, 0, 1]
    assert matched("folding_words_are_case_sensitive") == [0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0]
    grid = matched("word_boundaries")[:36]
    assert grid == [1 if (gd.SIDES[k // 6] not in (b"x", b"7") and gd.SIDES[k % 6] not in (b"x", b"7")) else 0 for k in range(36)]
    assert matched("word_boundaries")[36:39] == [1, 1, 0]          # first occurrence refused, second accepted
    over = dict(zip(gd.by_name("word_overlap")["headers"], matched("word_overlap")))
    assert over[b"xaaa;"] == 0 and over[b"aaa"] == 0 and over[b";aa;"] == 1 and over[b"aa"] == 1 and over[b"_aaa"] == 0 and over[b"aa_aa"] == 1 and over[b"aaa_aa"] == 1
    fgrid = matched("field_boundaries")[:36]
    assert fgrid == [1 if (gd.SIDES[k // 6] in (b"", b";") and gd.SIDES[k % 6] in (b"", b";")) else 0 for k in range(36)]
    ftail = dict(zip(S("field_boundaries")["headers"][36:], matched("field_boundaries")[36:]))
    assert ftail == {b"xsample=A": 0, b"x;sample=A;y": 1, b"sample=AB;sample=A": 1, b"sample=A;sample=B": 1, b"xsample=A;sample=A": 1,
                     b"sample=sample=A": 0, b"ssample=A;": 0}
    assert matched("empty_field") == [1, 1, 0, 1, 1, 0, 0, 1] == matched("empty_field_words")
    assert sum(matched("list_0_exact")) == 0 and sum(matched("list_1_exact")) == 1 and sum(matched("list_2_exact")) == 3
    assert sum(matched("list_33_exact")) == sum(matched("list_32_exact")) + 1
    assert len(S("list_100000_exact")["needles"]) == 100000 and len({len(n) for n in S("list_100000_exact")["needles"]}) == 1
    big = dict(zip(S("list_100000_exact")["headers"], matched("list_100000_exact")))
    assert big[b"OTU_099999"] == 1 and big[b"nothing"] == 0 and big[b"OTU_0000001"] == 0 and big[b"x;OTU_000999;y"] == 0
    assert len({len(n) for n in S("lengths_300_substr")["needles"]}) == 300
    assert matched("lengths_300_substr") == [1, 1, 0, 1, 0, 0] and matched("lengths_300_words") == [0, 1, 0, 0, 0, 0]
    assert matched("prefix_exact") == [1, 1, 0, 0, 0, 0, 1] and matched("prefix_substr") == [1, 1, 0, 1, 1, 1, 1] and matched("prefix_words") == [1, 1, 0, 0, 0, 1, 0]
    assert matched("last_label_only") == [0] * 13 + [1]
    assert sum(matched("ordinals_all")) == 16 and sum(matched("ordinals_none")) == 0 and matched("ordinals_alternating") == [k % 2 for k in range(16)]
    rec = {n: gd.expected(S(n))["records"] for n in ("subseq_1_5", "subseq_10_10", "subseq_11_20", "subseq_3_10", "subseq_3_99", "subseq_4_4", "subseq_empty_sequence")}
    assert [r[2:] for r in rec["subseq_1_5"]] == [(0, 5), (0, 3), (0, 10), (0, 4), (0, 1), (0, 5), (0, 12)]          # start = 1; end < len, > len
    assert [r[2:] for r in rec["subseq_10_10"]][:2] == [(9, 1), (0, 0)]                                                  # start = end = len; start > len
    assert [r[2:] for r in rec["subseq_11_20"]] == [(0, 0), (0, 0), (0, 10), (0, 0), (0, 0), (10, 10), (0, 12)]        # start = len + 1
    assert [r[2:] for r in rec["subseq_3_10"]][0] == (2, 8) and [r[2:] for r in rec["subseq_3_99"]][5] == (2, 23)     # end = len, end > len
    assert [r[2:] for r in rec["subseq_4_4"]][3] == (3, 1) and rec["subseq_4_4"][2] == (0, 1, 0, 10)                    # the unmatched read stays whole
    assert [r[2:] for r in rec["subseq_empty_sequence"]][0] == (0, 0)
