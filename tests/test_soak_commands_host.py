"""No GPU: five seeded rounds of every leg of oracle/soak_commands.py with --route host -- the library's host restatement alone against
the reference CLI (oracle/_ref/vsearch_ref, left there by build(); skipped only where that binary is absent), with the seeds of
tests/test_gpu_soak_commands.py.  No context is created.  For the chimera soak's --outputs alns, whose library side needs a device:
the host restatement of --uchimealns (what the device route is compared with there) against the plain-Python restatement at the
widths that soak draws."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("filter", "eestats", "fastq_stats", "derep", "derep_prefix", "search_exact", "orient", "sintax", "otutab", "hitout", "mask", "getseqs",
        "cut")
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


def test_uchimealns_host_equals_python_at_the_soak_widths():
    """300 seeded triples at --alignwidth 1 and 133 next to 0 / 60 / 80 (oracle/soak_chimera.ALIGNWIDTHS), under the --xn / --dn values
    that soak draws: rows, line ends, best_i, h by its bits and the six counts"""
    from oracle import soak_chimera
    from tests import chimalns_data as data
    from tests.test_chimalns_host import _host_in_record_order, _same
    assert sorted(soak_chimera.ALIGNWIDTHS) == [0, 1, 60, 80, 133]
    per_width = {}
    for k, t in enumerate(data.random_triples(300, seed=20261021)):
        width = soak_chimera.ALIGNWIDTHS[k % 5]
        got, exp = _host_in_record_order(t, alignwidth=width, xn=(8.0, 4.0, 6.5)[k % 3], dn=(1.4, 1.1, 2.0)[k % 7 % 3])
        _same(got, exp)
        assert len(exp["lines"]) == (1 if width == 0 else -(-exp["alnlen"] // width))
        per_width[width] = per_width.get(width, 0) + 1
    assert per_width == {w: 60 for w in soak_chimera.ALIGNWIDTHS}
