"""-m gpu: bench.py's two forms on a small workload.  A plain run reports the timed steps only; --full adds the side legs
(fetch, end_to_end, cpu_baseline, search_end_to_end), each checked against the timed step's results."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--queries", "2000", "--qlen", "200", "--db", "20000", "--dlen", "600"]
SIDE = ("fetch_s", "value_incl_fetch", "end_to_end", "value_end_to_end", "cpu_baseline", "search_end_to_end", "shapes")


def _line(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_and_full_bench_lines(gpu_required):
    d = _line([])
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 2 and d["warmup"] == 1
    assert not [k for k in SIDE if k in d], d.keys()

    d = _line(["--full", "--no-shapes", "--e2e-calls", "1", "--ref-search-queries", "200"])
    assert d["value"] > 0 and d["fetch_s"] >= 0 and "shapes" not in d
    assert d["end_to_end"].get("equals_plan_results") is True, d["end_to_end"]
    cb = d["cpu_baseline"]
    assert cb.get("parity_all_fields_match", cb.get("parity_match")) is True, cb
    s = d["search_end_to_end"]
    assert "error" not in s and s["queries"] == 2000 and s["queries_per_s"] > 0, s
