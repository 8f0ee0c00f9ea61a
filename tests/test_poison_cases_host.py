"""What tests/poison_cases.py claims and a device is not needed for: the parsing of the poison hook (vsx_internal_poison_byte, read once
per process, hence child processes), every case builds and its CPU reference runs, and the shapes are what the cases say they are."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from tests import poison_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SNIPPET = "import sys; sys.path.insert(0, %r); from tests import poison_cases as pc; print('BYTE', pc.poison_byte())" % ROOT


def _byte(env):
    e = {k: v for k, v in os.environ.items() if k not in ("VSX_POISON", "VSX_POISON_BYTE")}
    e.update(env)
    p = subprocess.run([sys.executable, "-c", _SNIPPET], env=e, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return int([ln for ln in p.stdout.splitlines() if ln.startswith("BYTE")][-1].split()[1]), p.stderr


@pytest.mark.parametrize("env,want,refused", [
    ({}, -1, False),
    ({"VSX_POISON_BYTE": "0x11"}, -1, False),                        # the byte alone switches nothing on
    ({"VSX_POISON": "1"}, 0xA5, False),
    ({"VSX_POISON": "1", "VSX_POISON_BYTE": "0"}, 0, False),
    ({"VSX_POISON": "1", "VSX_POISON_BYTE": "0xff"}, 255, False),
    ({"VSX_POISON": "1", "VSX_POISON_BYTE": "255"}, 255, False),
    ({"VSX_POISON": "1", "VSX_POISON_BYTE": "256"}, 0xA5, True),
    ({"VSX_POISON": "1", "VSX_POISON_BYTE": "zz"}, 0xA5, True),
    ({"VSX_POISON": "1", "VSX_POISON_BYTE": "-1"}, 0xA5, True),
    ({"VSX_POISON": "1", "VSX_POISON_BYTE": "0x"}, 0xA5, True),
    ({"VSX_POISON": "1", "VSX_POISON_BYTE": ""}, 0xA5, True),
], ids=lambda v: "+".join(f"{k}={x}" for k, x in v.items()) or "unset" if isinstance(v, dict) else None)
def test_poison_byte_parsing(env, want, refused):
    got, err = _byte(env)
    assert got == want
    assert ("VSX_POISON_BYTE" in err) == refused, err


@pytest.mark.parametrize("case", sorted(pc.CASES))
def test_case_builds_and_its_reference_runs(oracle, case):
    c = pc.CASES[case]
    if c.device_reference:
        assert c.input()            # (its reference is the library's host restatement behind a device search: the GPU test runs it)
        return
    ref = c.reference(c.input())
    assert ref and all(isinstance(n, str) and isinstance(bytes(b), bytes) for n, b in ref)
    assert len({n for n, _ in ref}) == len(ref), "section names repeat"
    assert sum(len(bytes(b)) for _, b in ref) > 0
    assert pc.digest(ref) == pc.reference_digest(case) == pc.digest(c.reference(c.input())), "the reference is not deterministic"


@pytest.mark.parametrize("case", sorted(pc.CASES))
def test_history_is_strictly_larger(case):
    c = pc.CASES[case]
    (reads, nbytes), (h_reads, h_bytes) = c.sizes(c.input())
    assert reads > 0 and h_reads > reads and h_bytes > nbytes, (case, reads, nbytes, h_reads, h_bytes)


def _pick_rows(Q):
    """vsx_plan.cpp pick_rows() over vsx_supported_rows(): the first row count R with 16 R >= Q, never more rows than the query has"""
    from vsearch_amd import _lib
    lib = _lib.load()
    lib.vsx_supported_rows.restype = C.POINTER(C.c_int)
    n = C.c_int(0)
    p = lib.vsx_supported_rows(C.byref(n))
    rows = [p[k] for k in range(n.value)]
    idx = next((k for k, r in enumerate(rows) if 16 * r >= Q), len(rows) - 1)
    while idx > 0 and Q < rows[idx]:
        idx -= 1
    return rows[idx], rows


def test_early_rows_shapes():
    P, _ = pc.scoring("default")
    plans = pc.CASES["early_rows"].input()
    assert [R for _, R, _ in plans] == list(pc.EARLY_ROWS) + [10]
    _, supported = _pick_rows(1)
    assert set(pc.EARLY_ROWS) <= set(supported)
    for tag, R, (qs, ts, qi, ti) in plans:
        assert sorted(len(q) for q in qs) == [16 * R - 3, 16 * R], tag
        for q in qs:
            assert _pick_rows(len(q))[0] == R, (tag, len(q))
        byte = tag.endswith("_byte")
        for k, q in enumerate(qs):
            mine = sorted((ts[b] for a, b in zip(qi, ti) if a == k), key=lambda t: -len(t))
            assert len(mine) == 16
            for task, centre in ((mine[:8], len(q) + 800), (mine[8:], len(q) + 400)):      # the planner: falling length, eight to a task
                assert all(abs(len(t) - centre) <= 12 + 3 for t in task), (tag, centre, [len(t) for t in task])
                assert all(pc.tilt_reach(P, len(q), len(t)) < 15800 for t in task), tag
                impure = [t for t in task if not set(t) <= set("ACGT")]
                assert len(impure) == (1 if byte else 0) and all(t.count("N") == 1 for t in impure), tag
            assert (set(q) <= set("ACGT")) != byte or len(q) == 0, tag


def test_chunked_needs_more_than_its_budget():
    """by vsx_internal_ckpt_bytes_estimate (one whole-wave task per pair; without a context it assumes the compressed layout of the
    tilted class, the smaller one): the plan's checkpoints exceed the budget -- even if its one-target tasks shared their waves eight
    at a time, which is more than the sparse classes pack (four)"""
    from vsearch_amd import _lib
    lib = _lib.load()
    qs, ts = pc.CASES["chunked"].input()
    assert len(qs) == 31 and len(qs[-1]) == 3000
    each = [int(lib.vsx_internal_ckpt_bytes_estimate(None, 1, len(q), len(t))) for q, t in zip(qs, ts)]
    assert sum(each) > 8 * pc.CHUNK_BUDGET, each


def test_aligner_history_shape():
    qs, db, qi, ti = pc.aligner_history()
    assert len(qi) == len(ti) == 128 * 24 and all(_pick_rows(len(q))[0] in (20, 22) for q in qs)


def test_large_cluster_has_two_row_tiles():
    """by the library's own tile height (vsx_internal_msa_row_tile, the constant vsx_msa.hip cuts its profile tiles with)"""
    tile = pc.msa_row_tile()
    case = pc.CASES["cluster_msa"]
    sizes = [len(c) for c in case.input()[1][0]]
    assert max(sizes) == case.MEMBERS and -(-case.MEMBERS // tile) == 2
    assert sorted(sizes)[-2] <= tile                                    # every other cluster is one tile
    assert -(-len(case.input()[2][0][0]) // tile) >= 3                  # the history cluster has more tiles than the case


@pytest.mark.parametrize("text,sticky", [
    ("VsxError: vsx_plan_sync: hipEventSynchronize(e) failed: an illegal memory access was encountered (vsx_host.cpp:1)", True),
    ("VsxError: hipStreamSynchronize failed: unspecified launch failure", True),
    ("AssertionError: R16: no task of the row class took the early exit", False),
    ("device != CPU reference: first differing section R16.cigar", False),
    (None, False),
])
def test_driver_knows_a_gpu_fault(text, sticky):
    assert pc.is_sticky(text) == sticky
