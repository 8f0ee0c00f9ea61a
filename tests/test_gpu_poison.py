"""Poisoned-memory parity (tests/poison_cases.py): no result may depend on bytes nobody wrote.

The driver runs every case in a fresh child process, on a fresh handle and on a handle with a history, once per setting of the library's
poison hook (vsx_private.h): off, then every handed-out block and every chunk's part of the shared checkpoint block, strip buffer and
traceback slab filled with 0x00, 0xA5, 0xFF.  The children run one after another, each under its own time limit.  A child that ends on a
signal, an abort, its time limit or a GPU fault ends the sequence: no further child is started and what is missing counts as "not run",
which fails the tests.  Per case: it succeeded under all four settings, fresh == after history in each, the four digests are equal, and
they equal the digest of the case's CPU reference (bit-identical, no tolerance).  Where the reference itself needs a device -- the chimera
commands' host restatement sits behind a device search, allpairs compares its stream with its blocks -- the child computes it and the
unpoisoned child's digest of it is the one that counts."""
import json
import os
import subprocess
import sys

import pytest

from tests import poison_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (name, VSX_POISON_BYTE or None = hook off, what vsx_internal_poison_byte() must say in the child)
SETTINGS = [("off", None, -1), ("0x00", "0x00", 0x00), ("0xA5", "0xA5", 0xA5), ("0xFF", "0xFF", 0xFF)]
CHILD_TIMEOUT = 420
FATAL_STATUS = (134, 139, -6, -11, 124, 137, pc.EXIT_GPU_FAULT)


def _child(tmp, name, byte):
    """-> (report or {}, fatal: why no further child may start, or None)"""
    env = {k: v for k, v in os.environ.items() if k not in ("VSX_POISON", "VSX_POISON_BYTE")}
    if byte is not None:
        env.update(VSX_POISON="1", VSX_POISON_BYTE=byte)
    out = os.path.join(tmp, f"poison_{name}.json")
    fatal, text, rc = None, "", None
    try:
        p = subprocess.run([sys.executable, "-m", "tests.poison_cases", "--out", out], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
        rc, text = p.returncode, p.stdout + p.stderr
        if rc < 0 or rc in FATAL_STATUS:
            fatal = f"child '{name}' ended with status {rc}"
    except subprocess.TimeoutExpired as e:
        text = "".join(x.decode(errors="replace") if isinstance(x, bytes) else (x or "") for x in (e.stdout, e.stderr))
        fatal = f"child '{name}' ran into its time limit of {CHILD_TIMEOUT} s"
    if "illegal memory access" in text:
        fatal = f"child '{name}' reported an illegal memory access"
    report = {}
    if os.path.exists(out):
        with open(out) as f:
            report = json.load(f)
    print(f"--- poison child {name}: status {rc}\n{text[-3000:]}")
    return report, fatal


@pytest.fixture(scope="module")
def reports(gpu_required, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("poison"))
    out, fatal = {}, None
    for name, byte, _ in SETTINGS:
        if fatal is None:
            out[name], fatal = _child(tmp, name, byte)
        else:
            out[name] = {}
    return out, fatal


def test_hook_is_live_in_the_poisoned_children(reports):
    out, fatal = reports
    for name, _, want in SETTINGS:
        assert "_poison_byte" in out[name], f"child '{name}' was not run or wrote no report ({fatal})"
        assert out[name]["_poison_byte"] == want, (name, out[name]["_poison_byte"])


@pytest.mark.parametrize("case", sorted(pc.CASES))
def test_case(reports, case):
    out, fatal = reports
    recs = {}
    for name, _, _ in SETTINGS:
        rec = out[name].get(case)
        assert rec is not None, f"{case} under '{name}': not run ({fatal or 'the child wrote no record'})"
        print(case, name, rec["seconds"], "s")
        assert rec["error"] is None, f"{case} under '{name}': {rec['error']}"
        assert rec["digest"] == rec["digest_history"], f"{case} under '{name}': fresh != after history"
        recs[name] = rec["digest"]
    assert len(set(recs.values())) == 1, f"{case}: the digest moves with the poison byte: {recs}"
    if pc.CASES[case].device_reference:
        # (the reference needs a device: the library's host restatement, as the unpoisoned child computed it)
        expected = out["off"][case]["digest_reference"]
        assert expected is not None and all(out[name][case]["digest_reference"] == expected for name, _, _ in SETTINGS), f"{case}: the host restatement moves"
    else:
        expected = pc.reference_digest(case)
    assert recs["off"] == expected, f"{case}: device != reference (python -m tests.poison_cases --verify --case {case} names the section)"
