"""-m gpu: a short, seeded run of the randomized soaks of the newer commands (oracle/soak_merge.py: --fastq_mergepairs with random
quality encodings, options, read lengths and windows; oracle/soak_chimera.py: --uchime_ref and the three de novo variants with random
lengths, masks and parameters) against the reference CLI, as tests/test_gpu_soak.py runs the older ones.

The floors are the reference's own line counts for the seed and the round count (`--reference-only`, no device), rounded down to
two significant digits.  The round counts keep the reference CLI's share of a case below 5 s (measured: 0.5 s for the 40 merge
rounds; 2.6 s and 3.7 s for the two chimera cases, where one --uchime_ref round at 3 900-4 200 symbols alone costs it 1-2 s).

The chimera seeds were picked, with the reference alone, so that each fixed set of six rounds contains a --uchime_ref round in the
length class that straddles the kernel's limit of 4 096, a --hardmask round and an --abskew round; the test asserts that on the
soak's own "coverage" record.  Together the two sets hold --uchime_ref in all four length classes and each de novo variant."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHIMERA_MUST = ("uchime_ref@3900-4200", "hardmask", "abskew")


@pytest.mark.parametrize("script,seed,rounds,floor,must", [
    ("soak_merge.py", 20260924, 40, 17_000, ()),          # 17 728 lines: merged FASTQ + eetabbed + not-merged labels
    ("soak_chimera.py", 20260930, 6, 330, CHIMERA_MUST),  # 330 --uchimeout lines
    ("soak_chimera.py", 20260971, 6, 170, CHIMERA_MUST),  # 171 --uchimeout lines
])
def test_seeded_soak(gpu_required, tmp_path, script, seed, rounds, floor, must):
    """a FIXED set of rounds per case (seed + round count: the same configurations on every machine, whatever its speed)"""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "vsearch_ref")):
        pytest.fail("oracle/_ref missing: run `make -C oracle ref ref_full` in the build container")
    out = str(tmp_path / "soak.json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", script), "--seconds", "300", "--max-rounds", str(rounds), "--seed", str(seed), "--out", out],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert os.path.exists(out), p.stderr[-3000:]
    doc = json.load(open(out))
    assert p.returncode == 0, json.dumps({k: v for k, v in doc.items() if k in ("failing_rounds", "failures")})[:3000]
    assert doc["rounds"] == rounds and doc["lines"] >= floor, doc
    for key in must:
        assert doc["coverage"].get(key, 0) >= 1, (key, doc["coverage"])
