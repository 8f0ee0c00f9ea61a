"""CPU (-m "not gpu"): the --chimeras_denovo C-ABI without a device -- defaults, record layout, range checks, the host restatement
of the selection and evaluation (vsx_internal_chimeras_long_host) against the reference lines stored in
tests/golden/chimeras_long_golden.json, and the reading of the reference's region scan that the restatement relies on."""
import ctypes as C
import itertools
import json
import random

import pytest

from tests import chimeras_long_data as data

Q = "q;size=1"


def test_opts_defaults_and_layout():
    from vsearch_amd import _lib
    from vsearch_amd.chimera import chimeras_long_default_opts
    o = chimeras_long_default_opts()
    assert (o.parts, o.parents_max, o.length_min, o.diff_pct, o.abskew, o.window) == (0, 3, 10, 0.0, 1.0, 0)
    # chimera_detection_parameters (core/chimera.cpp:2805-2824) with --abskew 1.0 (cli.cc:4481-4484)
    assert (o.search.id, o.search.weak_id, o.search.maxaccepts, o.search.maxrejects) == (0.55, 0.55, 4, 16)
    assert (o.search.self, o.search.selfid, o.search.maxsizeratio, o.search.soft_mask, o.search.strand_both) == (1, 1, 1.0, 2, 0)
    assert C.sizeof(_lib.ChimerasLongResult) == 432
    assert (_lib.CHIMERAS_LONG_MAX_QLEN, _lib.CHIMERAS_LONG_MAX_CAND) == (data.QMAX, data.CMAX)
    # the common long-read case is inside the kernel's limits: 1 500 bp, 15 parts x 4 accepted hits
    assert data.QMAX >= 1500 and data.CMAX >= 60
    lib = _lib.load()
    for s in ("vsx_chimeras_denovo", "vsx_chimeras_long_opts_default", "vsx_chimeras_denovo_last_stats", "vsx_internal_chimeras_long_host"):
        assert hasattr(lib, s)


def _host(q, cands, cigars, **opts):
    from vsearch_amd import _lib
    from vsearch_amd.chimera import chimeras_long_default_opts, long_record
    lib = _lib.load()
    o = chimeras_long_default_opts()
    for k, v in opts.items():
        setattr(o, k, v)
    n = len(cands)
    t = (C.c_char_p * max(n, 1))(*[c.encode() for c in cands])
    cg = (C.c_char_p * max(n, 1))(*[c.encode() for c in cigars])
    tl = (C.c_uint32 * max(n, 1))(*[len(c) for c in cands])
    out = _lib.ChimerasLongResult()
    rc = lib.vsx_internal_chimeras_long_host(q.encode(), len(q), n, t, tl, cg, C.byref(o), C.byref(out))
    return rc, (long_record(out) if rc == _lib.VSX_OK else None)


def test_option_ranges():
    """cli.cc:4390-4411"""
    from vsearch_amd import _lib
    from vsearch_amd.chimera import chimeras_long_default_opts
    lib = _lib.load()
    lib.vsx_last_error.restype = C.c_char_p
    q, t = "ACGTACGTAC" * 3, ["ACGTACGTAC" * 3]
    assert _host(q, t, ["30M"])[0] == _lib.VSX_OK
    bad = [("length_min", 0), ("parents_max", 1), ("parents_max", 21), ("diff_pct", -0.5), ("diff_pct", 50.5), ("diff_pct", float("nan")),
           ("parts", 1), ("parts", 101), ("parts", -3), ("abskew", 0.5)]
    for field, value in bad:
        assert _host(q, t, ["30M"], **{field: value})[0] == _lib.VSX_EINVAL, (field, value)
        assert field.encode() in lib.vsx_last_error()
        # the command itself refuses the same options before it looks at the searcher
        o = chimeras_long_default_opts()
        setattr(o, field, value)
        out = (_lib.ChimerasLongResult * 1)()
        assert lib.vsx_chimeras_denovo(None, C.byref(o), out) == _lib.VSX_EINVAL
        assert field.encode() in lib.vsx_last_error()
    for field, value in (("length_min", 1), ("parents_max", 2), ("parents_max", 20), ("diff_pct", 50.0), ("parts", 2), ("parts", 100)):
        assert _host(q, t, ["30M"], **{field: value})[0] == _lib.VSX_OK, (field, value)
    o = chimeras_long_default_opts()
    out = (_lib.ChimerasLongResult * 1)()
    assert lib.vsx_chimeras_denovo(None, C.byref(o), out) == _lib.VSX_EINVAL and b"null argument" in lib.vsx_last_error()
    assert lib.vsx_chimeras_denovo(None, None, out) == _lib.VSX_EINVAL
    assert _host(q, t, ["29M"])[0] == _lib.VSX_EINVAL                       # a CIGAR that does not span the sequences


def _case_alignments(name, c):
    """candidates (every sequence before the query, in input order) and the CIGARs of the query against them: gapless by
    construction, but for the inputs built around one insertion.  These are NOT the candidates and alignments the search produces:
    the inputs are built so that every earlier sequence is a candidate and the hand-written alignment is the optimal one, which is
    why the lines agree with the reference's.  The end-to-end check of the same inputs is tests/test_gpu_chimeras_denovo.py."""
    q, cands = c["seqs"][-1], c["seqs"][:-1]
    n = len(q)
    cig = {"insertion_front": f"I{n}M", "insertion_back": f"{n}MI", "one_parent_twice": "200MI99M", "one_parent_uncovered": "100MI199M"}.get(name, f"{n}M")
    if name.startswith("one_parent"):
        cands = cands[:1]
    return q, cands, [cig] * len(cands)


def test_host_restatement_matches_golden():
    """the host restatement on every named edge input (all but the length steps, which hold several queries) gives the reference's
    verdict and, for a chimera, its --tabbedout line"""
    from vsearch_amd.chimera import format_tabbedout
    gold = json.load(open(data.GOLDEN))["edges"]
    seen_y = 0
    for name, c in data.edge_cases().items():
        if name == "lengths":
            continue
        assert gold[name]["digest"] == data.case_digest(c["labels"], c["seqs"]), name
        q, cands, cigars = _case_alignments(name, c)
        opts = {k: v for k, v in c["opts"].items() if k != "parts"}
        rc, rec = _host(q, cands, cigars, **opts)
        assert rc == 0
        if Q in gold[name]["chimeras"]:
            assert rec["flag"] == "Y" and rec["status"] == "chimeric", name
            line = [ln for ln in gold[name]["tabbedout"] if ln.split("\t")[1] == Q][0]
            assert format_tabbedout(rec, Q, c["labels"]) == line, name
            assert sum(rec["len"]) == len(q) and rec["start"] == sorted(rec["start"])
            seen_y += 1
        else:
            assert rec["flag"] == "N" and rec["status"] == "no_parents", name
            assert rec["id_query_top"] == 0.0 and rec["alnlen"] == 0
    assert seen_y >= 20


def test_host_restatement_diff_pct():
    """the same input under four percentages: 'N' with position 50 uncovered at 0 and 0.1, 'Y' with two parents at 1 and 2.5, the
    a region running over the mismatch; a restatement that ignored diff_pct would fail both halves"""
    cases = data.edge_cases()
    recs = {}
    for pct in (0, 0.1, 1, 2.5):
        c = cases[f"diff_pct{pct}"]
        recs[pct] = _host(*_case_alignments(f"diff_pct{pct}", c), diff_pct=pct)[1]
    for pct in (0, 0.1):
        r = recs[pct]
        assert r["flag"] == "N" and r["n_parents"] == 3 and sum(r["len"]) < 600, (pct, r)
        assert all(not (s <= 50 < s + n) for s, n in zip(r["start"], r["len"]))
    for pct in (1, 2.5):
        r = recs[pct]
        assert (r["flag"], r["n_parents"], r["parent"], r["start"][0]) == ("Y", 2, [0, 1], 0), (pct, r)
        assert sum(r["len"]) == 600                                  # position 50 lies inside a region: the mismatch is tolerated
    assert (recs[1]["start"], recs[1]["len"]) == ([0, 251], [251, 349]) and (recs[2.5]["start"], recs[2.5]["len"]) == ([0, 31], [31, 569])
    assert recs[2.5]["len"] != recs[1]["len"]                        # the tolerance decides where the regions meet


def test_host_restatement_records():
    cases = data.edge_cases()
    rec = _host(*_case_alignments("one_parent_twice", cases["one_parent_twice"]))[1]
    assert (rec["parent"], rec["start"], rec["len"], rec["alnlen"]) == ([0, 0], [0, 200], [200, 99], 300)
    assert rec["divergence"] == 100.0 * (100.0 - rec["id_query_top"]) / rec["id_query_top"]
    # the position after the insertion is never covered when the first round takes the segment behind it
    rec = _host(*_case_alignments("one_parent_uncovered", cases["one_parent_uncovered"]))[1]
    assert (rec["flag"], rec["parent"], rec["start"], rec["len"]) == ("N", [0, 0], [0, 101], [100, 198])
    # equal regions within one candidate: the leftmost first, then the other, then the second variant; position 100 stays unused
    rec = _host(*_case_alignments("tie_within_uncovered", cases["tie_within_uncovered"]))[1]
    assert (rec["flag"], rec["n_parents"], rec["parent"], rec["start"], rec["len"]) == ("N", 3, [0, 0, 1], [0, 101, 201], [100, 100, 99])
    rec2 = _host(*_case_alignments("tie_within_uncovered", cases["tie_within_uncovered"]), parents_max=2)[1]
    assert (rec2["parent"], rec2["start"], rec2["len"]) == ([0, 0], [0, 101], [100, 100])       # the leftmost of the equal regions came first
    # equal regions in two candidates: the earlier candidate
    q, cands, cigars = _case_alignments("tie_candidates", cases["tie_candidates"])
    assert _host(q, cands, cigars)[1]["parent"] == [0, 1]
    assert _host(q, [cands[0], cands[2], cands[1]], cigars)[1]["parent"] == [0, 1]
    # twenty parents
    rec = _host(*_case_alignments("parents20_max20", cases["parents20_max20"]), parents_max=20)[1]
    assert rec["parent"] == list(range(20)) and rec["len"] == [15] * 20
    # no candidates, an empty query
    assert _host("ACGT", [], [])[1]["n_parents"] == 0
    assert _host("", [], [])[1]["flag"] == "N"


# ---- the reading of scan_matches (core/chimera.cpp:439-502) ----

def scan_two_pointer(m, pct):
    """the reference's form: prefix sums, suffix maxima, two pointers; (start, length) or None"""
    n = len(m)
    p = [0.0] * (n + 1)
    for i in range(n):
        p[i + 1] = p[i] + (pct if m[i] else pct - 100.0)
    q = [0.0] * (n + 1)
    q[n] = p[n]
    for i in range(n - 1, -1, -1):
        q[i] = max(q[i + 1], p[i])
    best_i, best_d, best_c = 0, -1, -1.0
    i = j = 1
    while j <= n:
        c = q[j] - p[i - 1]
        if c >= 0.0:
            d = j - i + 1
            if d > best_d:
                best_i, best_d, best_c = i, d, c
            j += 1
        else:
            i += 1
    return (best_i - 1, best_d) if best_c >= 0.0 else None


def longest_nonnegative(m, pct):
    """the stated reading: the longest substring whose score is >= 0, the leftmost among the longest (the empty one at 0 if none)"""
    n = len(m)
    for d in range(n, 0, -1):
        for s in range(0, n - d + 1):
            k = sum(m[s:s + d])
            if k * pct + (d - k) * (pct - 100.0) >= 0.0:
                return s, d
    return (0, 0) if n else None


@pytest.mark.parametrize("pct", [0, 2, 50])
def test_scan_reading_exhaustive(pct):
    for n in range(0, 13):
        for m in itertools.product((0, 1), repeat=n):
            got, exp = scan_two_pointer(m, float(pct)), longest_nonnegative(m, float(pct))
            if exp is not None and exp[1] == 0:
                assert got is not None and got[1] == 0, (m, got)       # an empty region: never reaches length_min >= 1
            else:
                assert got == exp, (m, pct, got, exp)


def test_scan_reading_seeded():
    rng = random.Random(99)
    for _ in range(300):
        n = rng.randint(13, 160)
        m = [1 if rng.random() < rng.choice((0.5, 0.9, 0.98)) else 0 for _ in range(n)]
        for pct in (0.0, 2.0, 50.0):
            got, exp = scan_two_pointer(m, pct), longest_nonnegative(m, pct)
            assert got == exp or (got[1] == 0 and exp[1] == 0), (m, pct, got, exp)


def test_host_scan_agrees_with_the_reading():
    """the library's restatement on one candidate and one segment = the two-pointer form, for exact and inexact percentages"""
    rng = random.Random(7)
    for _ in range(120):
        n = rng.randint(20, 120)
        m = [1 if rng.random() < 0.93 else 0 for _ in range(n)]
        q = "".join(rng.choice("ACGT") for _ in range(n))
        t = "".join(ch if ok else data._sub(ch, 1) for ch, ok in zip(q, m))
        for pct in (0.0, 1.0, 2.5, 0.1, 7.3):
            rec = _host(q, [t], [f"{n}M"], parents_max=2, length_min=1, diff_pct=pct)[1]
            exp = scan_two_pointer(m, pct)
            if exp[1] == 0:
                assert rec["n_parents"] == 0
            else:
                # the first round's region is the scan of the whole query; the record lists regions by start
                assert exp in list(zip(rec["start"], rec["len"])), (m, pct, rec)
                assert max(rec["len"]) == exp[1]
