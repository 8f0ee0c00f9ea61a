"""Restriction-site cutting without a GPU: the library's host restatement (VSX_CUT=host) against the plain-Python restatement of
tests/cut_data.py on every array and on the text, the writers against the reference's recorded files, the ABI surface and its
refusals with the reference's messages, 3 000 seeded dense cases, and the assertions that the input sets reach the cases they are
named after (computed from py_cut() and py_pattern()).
"""
import ctypes as C
import importlib
import random

import numpy as np
import pytest

from tests import cut_data as cd
from vsearch_amd import _lib

ct = importlib.import_module("vsearch_amd.cut")            # (the package exports the function cut under the module's name)


@pytest.fixture(scope="module")
def sets():
    return cd.all_sets()


@pytest.fixture(scope="module")
def by_name(sets):
    return {s["name"]: s for s in sets}


@pytest.fixture(scope="module")
def expected(sets):
    return {s["name"]: cd.py_cut(s["seqs"], s["pattern"]) for s in sets}


# ---- host restatement == plain Python ------------------------------------------------------------------------------------------
def test_host_equals_python_on_every_set(sets):
    for s in sets:
        res = cd.call(None, s)
        cd.assert_equals_py(res, s)
        assert res.stats["host_no_context"] == 1 and res.stats["sequences"] == len(s["seqs"]), res.stats


def test_host_equals_python_on_3000_dense_cases():
    rng = random.Random(2111)
    cut_total = uncut_total = 0
    for case in range(3000):
        p = rng.randint(1, 5)
        body = "".join(rng.choice("ATN") for _ in range(p))
        fwd, rev = rng.randint(0, p), rng.randint(0, p)
        raw = body
        for at, mark in sorted([(fwd, "^"), (rev, "_")], reverse=True) if rng.random() < 0.5 else sorted([(rev, "_"), (fwd, "^")], reverse=True):
            raw = raw[:at] + mark + raw[at:]
        seqs = ["".join(rng.choice("ATN" if rng.random() < 0.9 else "ATNat") for _ in range(rng.randint(0, 24))) for _ in range(rng.randint(1, 6))]
        s = cd._set(f"dense{case}", seqs, raw)
        res = cd.call(None, s)
        cd.assert_equals_py(res, s)
        cut_total += res.cut
        uncut_total += res.uncut_total
    assert cut_total > 3000 and uncut_total > 1000


def test_threads_and_windows_do_not_show(sets):
    big = cd._set("threads", cd.seeded_set(2112, 3000, 0, 120, "ACGTN", site_rate=0.03))
    one = cd.call(None, big, threads=1)
    cd.assert_equals_py(one, big)
    for threads in (2, 5, 16):
        assert cd.call(None, big, threads=threads, window=7).tobytes() == one.tobytes(), threads


def test_each_want_bit_alone(by_name):
    s = by_name["ordinals"]
    full = cd.call(None, s)
    for bits in range(16):
        kw = dict(want_fwd=bool(bits & 1), want_rev=bool(bits & 2), want_rev_text=bool(bits & 4), want_discarded_rev_text=bool(bits & 8))
        part = cd.call(None, s, **kw)
        assert (part.fwd is None) == (not bits & 1) and (part.rev is None) == (not bits & 6)
        assert (part.rev_off is None) == (not bits & 4) and (part.discarded_off is None) == (not bits & 8) and (part.text_blob is None) == (not bits & 12)
        assert (part.n_fwd, part.n_rev, part.n_uncut) == (full.n_fwd, full.n_rev, full.n_uncut)
        cd.assert_same(part, full, bits)
        if bits & 4:
            assert [part.rev_text(x) for x in range(part.n_rev)] == [full.rev_text(x) for x in range(full.n_rev)]
        if bits & 8:
            assert [part.discarded_rev_text(x) for x in range(part.n_uncut)] == [full.discarded_rev_text(x) for x in range(full.n_uncut)]


def test_scattered_and_reversed_offsets(by_name):
    s = by_name["relabel_sizeout"]
    full = cd.call(None, s)
    rng = random.Random(5)
    blob, off = b"", []
    for x in reversed(s["seqs"]):
        blob += b"GAATTC"[:rng.randint(0, 6)]                               # junk that would complete a site across a boundary
        off.append(len(blob))
        blob += x.encode()
    off = np.array(off[::-1], np.uint64)
    lens = np.array([len(x) for x in s["seqs"]], np.uint32)
    assert ct.cut_host((blob, off, lens), s["pattern"]).tobytes() == full.tobytes()


# ---- the writers ---------------------------------------------------------------------------------------------------------------
def test_writers_equal_golden():
    for s in cd.load_golden():
        cd.assert_text_equals_golden(cd.call(None, s), s)


def test_writers_refuse_what_the_call_did_not_return(by_name):
    s = by_name["ordinals"]
    res = cd.call(None, s, want_fwd=False, want_rev=False, want_rev_text=False, want_discarded_rev_text=False)
    for which in ("fastaout", "fastaout_rev", "fastaout_discarded_rev", "nonsense"):
        with pytest.raises(ValueError):
            ct.fasta_lines(res, s["labels"], s["seqs"], which)
    assert len(ct.fasta_lines(res, s["labels"], s["seqs"], "fastaout_discarded")) == 2 * res.n_uncut


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def _raw(pattern=b"G^AATT_C", opts_edit=None, blob=b"ACGAATTCGT", off=(0,), lens=(10,)):
    lib = _lib.load()
    o = _lib.CutOpts()
    lib.vsx_cut_opts_default(C.byref(o))
    o.pattern, o.pattern_len = pattern, len(pattern)
    if opts_edit:
        opts_edit(o)
    off, lens = np.array(off, np.uint64), np.array(lens, np.uint32)
    res = _lib.CutOut()
    rc = lib.vsx_cut(None, C.byref(o), len(lens), C.cast(C.c_char_p(blob), C.c_void_p), len(blob), off.ctypes.data_as(C.c_void_p),
                     lens.ctypes.data_as(C.c_void_p), C.byref(res))
    got = (rc, int(res.total_matches), lib.vsx_last_error().decode())
    if rc == 0:
        lib.vsx_cut_out_free(C.byref(res))
    return got


def test_symbols_and_defaults():
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in _lib.CUT_SYMBOLS)
    o = _lib.CutOpts()
    lib.vsx_cut_opts_default(C.byref(o))
    assert (o.pattern, o.pattern_len, o.want, o.threads, o.window) == (None, 0, 15, 0, 0)
    assert C.sizeof(_lib.CutOpts) == 32 and C.sizeof(_lib.CutOut) == 15 * 8 and C.sizeof(_lib.CutStats) == 19 * 8
    import vsearch_amd
    assert vsearch_amd.cut is ct.cut and vsearch_amd.parse_pattern is ct.parse_pattern and vsearch_amd.CutResult is ct.CutResult


def test_pattern_refusals_carry_the_reference_message():
    fatals = cd.load_fatals()
    assert fatals == cd.PATTERN_FATALS                                      # what the reference printed when the golden file was written
    for pattern, message in fatals.items():
        with pytest.raises(ValueError) as e:
            ct.parse_pattern(pattern)
        assert str(e.value) == message
        with pytest.raises(ValueError) as e:
            cd.py_pattern(pattern)
        assert str(e.value) == message
        with pytest.raises(ValueError) as e:
            ct.cut_host(["ACGT"], pattern)
        assert str(e.value) == message
        rc, _, text = _raw(pattern.encode())
        assert rc == _lib.VSX_EINVAL and text.endswith(message), (pattern, text)
    rc, _, text = _raw(b"")
    assert rc == _lib.VSX_EINVAL and text.endswith("No forward sequence cut site (^) found in pattern")
    # the circumflex is looked at first: a second circumflex is reported before a missing underscore
    with pytest.raises(ValueError, match="Multiple cut sites"):
        ct.parse_pattern("^^")
    with pytest.raises(ValueError, match=r"No forward sequence cut site"):
        ct.parse_pattern("__")


def test_parse_pattern_equals_python():
    for raw in ("G^AATT_C", "G_AATT^C", "^_A", "_^A", "A^_", "A_^", "^A_", "_A^", "GCCNNNN^N_GGC", "n^_u", cd.long_pattern(65, 30, 31)):
        assert ct.parse_pattern(raw) == cd.py_pattern(raw), raw
    assert ct.parse_pattern("G^AATT_C") == ("GAATTC", 1, 5)


def test_refusals():
    assert _raw()[:2] == (0, 1)

    def edit(**kw):
        def f(o):
            for k, v in kw.items():
                setattr(o, k, v)
        return f
    for kw in (dict(want=16), dict(window=-1), dict(threads=-1)):
        assert _raw(opts_edit=edit(**kw))[0] == _lib.VSX_EINVAL, kw
    assert _raw(opts_edit=edit(want=0))[:2] == (0, 1)
    assert _raw(off=(4,), lens=(7,))[0] == _lib.VSX_EINVAL                  # beyond the blob
    assert _raw(off=(0, 2), lens=(10, 8))[:2] == (0, 2)                     # sequences may share bytes: nothing is written into them
    assert _raw(off=(3, 3, 3), lens=(0, 6, 0))[:2] == (0, 0)
    assert _raw(blob=b"", off=(), lens=())[:2] == (0, 0)


def test_tile_is_checked_per_call(monkeypatch):
    for bad in ("0", "63", "100"):
        monkeypatch.setenv("VSX_CUT_TILE", bad)
        assert _raw()[0] == _lib.VSX_EINVAL, bad
    monkeypatch.setenv("VSX_CUT_TILE", "64")
    assert _raw()[:2] == (0, 1)


# ---- the sets reach their cases ------------------------------------------------------------------------------------------------
def test_lengths_are_covered(by_name):
    p = 6
    assert {0} <= {len(x) for x in by_name["empty"]["seqs"]}
    assert {p - 1, p, p + 1} <= {len(x) for x in by_name["lengths"]["seqs"]}
    exp = cd.py_cut(by_name["lengths"]["seqs"], cd.ECORI)
    assert exp["matches"] == [0, 1, 1, 0, 1, 0, 0]


def test_ends_of_a_sequence(by_name, expected):
    # cut_fwd = 0 with a match at 0: the first forward fragment is empty and takes no ordinal; cut_rev = P with a match at L - P
    s, e = by_name["ends_fwd0_revP"], expected["ends_fwd0_revP"]
    assert cd.py_pattern(s["pattern"])[1:] == (0, 6)
    L = len(cd.ENDS)
    assert cd.py_match_positions(cd.ENDS, s["pattern"]) == [0, 8, L - 6]
    assert [r for r in e["fwd"] if r[0] == 0] == [(0, 0, 8), (0, 8, L - 14), (0, L - 6, 6)]                 # 3 matches, 3 fragments
    assert [r for r in e["rev"] if r[0] == 0] == [(0, 0, 6), (0, 6, 8), (0, 14, L - 14)]                    # no empty tail
    assert [r for r in e["fwd"] if r[0] == 1] == [(1, 0, 6)] and [r for r in e["rev"] if r[0] == 1] == [(1, 0, 6)]
    s, e = by_name["ends_rev0_fwdP"], expected["ends_rev0_fwdP"]
    assert cd.py_pattern(s["pattern"])[1:] == (6, 0)
    assert [r for r in e["rev"] if r[0] == 0] == [(0, 0, 8), (0, 8, L - 14), (0, L - 6, 6)]
    assert [r for r in e["fwd"] if r[0] == 0] == [(0, 0, 6), (0, 6, 8), (0, 14, L - 14)]


def test_site_layouts(by_name):
    sites = {name: cd.py_pattern(by_name[name]["pattern"])[1:] for name in by_name}
    assert sites["rev_below_fwd"] == (5, 1) and sites["rev_above_fwd"] == (1, 5)
    assert sites["adjacent_fwd_rev"] == sites["adjacent_rev_fwd"] == (3, 3)
    assert sites["both_at_start"] == sites["both_at_start_swapped"] == (0, 0)
    assert sites["both_at_end"] == sites["both_at_end_swapped"] == (6, 6)
    assert by_name["adjacent_fwd_rev"]["pattern"] != by_name["adjacent_rev_fwd"]["pattern"]


def test_overlaps(by_name, expected):
    assert expected["overlap_aa"]["matches"][0] == 3 and cd.py_match_positions("AAAA", "A^A_") == [0, 1, 2]
    e = expected["every_position"]
    assert e["matches"] == [len(x) for x in by_name["every_position"]["seqs"]] and e["uncut"] == []
    assert expected["code0_n"]["matches"] == [8, 0, 2]                      # a byte with code 0 matches nothing, N included


def test_alphabet(by_name, expected):
    up = cd.IUPAC
    assert set(up) == set(cd.CODE4)
    assert expected["alphabet_a"]["matches"] == [sum(1 for c in up if cd.CODE4[c] & 1)] * 2         # A matches A, R, N, a, ... but not Y
    assert cd.py_match_positions("Y", "^R_") == [] and cd.py_match_positions("N", "^A_") == [0] and cd.py_match_positions("a", "A^_") == [0]
    assert cd.py_match_positions("U", "^T_") == [0] and cd.py_match_positions("t", "^u_") == [0]
    assert expected["alphabet_two"]["matches"][2:] == [3, 3]
    assert expected["code0"]["matches"] == [0, 1, 0, 1, 1]
    assert all(cd.code4(c) == 0 for c in "-* \x00~1")


def test_packed_neighbours_give_no_match(by_name, expected):
    seqs = by_name["neighbours"]["seqs"]
    assert (seqs[0] + seqs[1]).count("GAATTC") == 1 and (seqs[3] + seqs[4]) == "GAATTC"
    assert expected["neighbours"]["matches"] == [0, 0, 1, 0, 0]


def test_the_four_ordinal_runs_differ(by_name):
    s = by_name["ordinals"]
    res = cd.call(None, s)
    text = {w: cd.lib_text(res, s, w) for w in cd.WHICH}
    heads = {w: [l for l in text[w].splitlines() if l.startswith(">")] for w in cd.WHICH}
    assert heads["fastaout_discarded"] == heads["fastaout_discarded_rev"] == [f">F{x + 1}" for x in range(res.n_uncut)]
    assert heads["fastaout"] == [f">F{x + 1}" for x in range(res.n_fwd)] and heads["fastaout_rev"] == [f">F{x + 1}" for x in range(res.n_rev)]
    assert len({res.n_fwd, res.n_rev, res.n_uncut}) == 3
    # the sequence of fragment x differs between the forward and the reverse list from the first empty fragment on
    assert [int(k) for k in res.fwd[0]] != [int(k) for k in res.rev[0]][:res.n_fwd]
    cut_ones = [k for k, m in enumerate(res.matches) if m]
    assert any(b - a > 1 for a, b in zip(cut_ones, cut_ones[1:]))           # uncut sequences between cut ones


def test_pattern_lengths(by_name):
    for p in (63, 64, 65):
        s = by_name[f"pattern_{p}"]
        assert len(cd.py_pattern(s["pattern"])[0]) == p
        exp = cd.py_cut(s["seqs"], s["pattern"])
        assert exp["matches"] == [2, 1, 0, 0, 1, 2], (p, exp["matches"])
        assert cd.call(None, s).stats["pattern_length"] == p
    assert _lib.CUT_DEVICE_MAX_PATTERN == 64


def test_edges_hold_a_match_at_every_place(by_name):
    seqs = by_name["edges"]["seqs"]
    at = [cd.py_match_positions(x, cd.ECORI) for x in seqs]
    assert at[:6] == [[i] for i in range(59, 65)] and at[6:12] == [[i] for i in range(4091, 4097)]
    assert at[12] == [64, 125, 4093, 4158]                                  # the site written at 64 took the last symbol of the one at 59
