"""No GPU: five seeded rounds of every leg of oracle/soak_commands.py with --route host -- the library's host restatement alone against
the reference CLI (oracle/_ref/vsearch_ref, left there by build(); skipped only where that binary is absent), with the seeds of
tests/test_gpu_soak_commands.py.  No context is created."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("filter", "eestats", "fastq_stats", "derep", "derep_prefix", "search_exact", "orient", "sintax", "otutab", "hitout")
SEED, ROUNDS = 20261020, 5

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "vsearch_ref")), reason="oracle/_ref/vsearch_ref not built")


def test_the_registry_holds_these_legs():
    from oracle import soak_commands
    assert sorted(soak_commands.LEGS) == sorted(LEGS)


@pytest.mark.parametrize("leg", LEGS)
def test_host_route_equals_the_reference(tmp_path, leg):
    out = str(tmp_path / "soak.json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "soak_commands.py"), "--command", leg, "--route", "host", "--seconds", "300",
                        "--max-rounds", str(ROUNDS), "--seed", str(SEED), "--out", out], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert os.path.exists(out), p.stderr[-3000:]
    doc = json.load(open(out))
    assert p.returncode == 0 and doc["failing_rounds"] == 0, json.dumps(doc["failures"])[:3000] + p.stderr[-1000:]
    assert doc["rounds"] == ROUNDS and doc["route"] == "host" and doc["lines"] > 0, doc
