"""GPU (-m gpu): vsx_chimera.hip over the whole range of query lengths it accepts (32 .. VSX_CHIMERA_MAX_QLEN = 4096), at the lengths
where its 32-column windows, 32-bit match words and 256-column scan chunks begin or end, with 2 and with 16 candidates, and the
host route just above the limit.  Inputs: tests/chimera_length_data.py.

The --uchimeout lines must equal the reference CLI's (oracle/_ref/vsearch_ref --threads 1) byte for byte, for --uchime_ref under
the default masks and under --qmask none --dbmask none and for the three de novo variants; the kernel's records must equal the
host restatement's bit for bit (VSX_CHIMERA=host, a fresh child process).  What the inputs must provoke is asserted on the
reference's own lines.  The reference commands run once per module, side by side.

Short queries.  A part of 8-10 symbols holds one to three 8-mers, and the family of chimera_length_data.family() (parents 40
symbols longer than the query, 5 % from their ancestor) gets no two candidates from the reference's part search below L = 42:
those queries end as "no parents" in both programs before any kernel runs, and EXTRA_LENGTHS (42, 43, 48, 49) are the shortest at
which that family reaches the kernel.  L = 33 .. 41 (2 .. 10 windows) therefore have inputs of their own, short_lengths(): parents
of exactly L symbols, seeds at which the reference scores the chimera.  For L = 32 (one window) no input was found that the
reference scores (1 200 seeds at four divergences gave none): an observation, not a rule of the reference.  The conditions on
the reference's own lines are asserted without a device in tests/test_chimera_lengths_ref.py."""
import json
import os
import subprocess
import sys

import pytest

from oracle import refcli
from tests import chimera_length_data as cd
from tests.test_gpu_chimera import _ref_lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASKS = {"default": {}, "none": dict(soft_mask=0)}          # ChimeraSession's keywords for chimera_length_data.MASKS
VARIANTS = cd.VARIANTS


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


@pytest.fixture(scope="module")
def data():
    return cd.all_lengths()


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """chimera_length_data.reference_lines(): the reference CLI's lines, computed once"""
    if not refcli.available():
        pytest.skip("oracle/_ref/vsearch_ref not built")
    return cd.reference_lines(str(tmp_path_factory.mktemp("reference")))


def _diff(got, exp):
    assert len(got) == len(exp)
    bad = [(a, b) for a, b in zip(got, exp) if a != b]
    assert not bad, f"{len(bad)} lines differ, first:\n got {bad[0][0]}\n ref {bad[0][1]}"


@pytest.mark.parametrize("mode", list(MASKS))
def test_every_length_matches_reference_cli(aligner, data, reference, mode):
    from vsearch_amd import ChimeraSession
    tn, db, qn, qs = data
    s = ChimeraSession(aligner, db, labels=tn, **MASKS[mode])
    _diff(s.uchimeout(qs, qn), reference[mode])
    # a query with fewer than two candidates is answered before a route is chosen and counts on neither side
    n_long = sum(len(q) > cd.MAX_QLEN for q in qs)
    n_scored = sum(line.split("\t")[2] != "*" for q, line in zip(qs, reference[mode]) if len(q) <= cd.MAX_QLEN)
    assert s.stats["queries_host"] == n_long == 6 * len(cd.HOST_LENGTHS), s.stats
    assert n_scored <= s.stats["queries_kernel"] <= len(qs) - n_long, (s.stats, n_scored)
    assert s.stats["sentinel_pairs"] == 0


@pytest.mark.parametrize("mode", list(MASKS))
def test_two_to_ten_windows_match_reference_cli(aligner, reference, mode):
    """L = 33 .. 41: every query of chimera_length_data.short_lengths() has exactly its two parents as candidates and is scored by
    the reference (tests/test_chimera_lengths_ref.py asserts that on the reference's lines), so every one runs in the kernel"""
    from vsearch_amd import ChimeraSession
    tn, db, qn, qs = cd.short_lengths()
    s = ChimeraSession(aligner, db, labels=tn, **MASKS[mode])
    _diff(s.uchimeout(qs, qn), reference["short_" + mode])
    assert all(line.split("\t")[2] != "*" for line in reference["short_" + mode])
    assert s.stats["queries_kernel"] == len(qs) and s.stats["queries_host"] == 0 and s.stats["pairs_aligned"] == 2 * len(qs), s.stats


@pytest.mark.parametrize("L", [512, 1500])
def test_two_and_sixteen_candidates(aligner, tmp_path, L):
    """16 references built four per quarter of the query (each of the four part searches returns four distinct targets) and a
    database with exactly two relatives of the query"""
    if not refcli.available():
        pytest.skip("oracle/_ref/vsearch_ref not built")
    from vsearch_amd import ChimeraSession
    for build, ncand in ((cd.sixteen_candidates, 16), (cd.two_relatives, 2)):
        tn, db, q = build(L)
        exp = _ref_lines(str(tmp_path), ["q"], [q], tn, db)
        assert exp[0].endswith("\tY"), exp
        s = ChimeraSession(aligner, db, labels=tn)
        assert s.uchimeout([q], ["q"]) == exp
        assert s.stats["pairs_aligned"] == ncand and s.stats["queries_kernel"] == 1, s.stats


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from tests import chimera_length_data as cd
from vsearch_amd import Aligner, ChimeraSession
tn, db, qn, qs = cd.all_lengths()
with Aligner(device=0) as al:
    s = ChimeraSession(al, db, labels=tn)
    recs = s.uchime_ref(qs)
    print(json.dumps({"recs": [{k: (v.hex() if isinstance(v, float) else v) for k, v in r.items()} for r in recs], "stats": s.stats}))
"""


def test_kernel_equals_host_restatement(aligner, data):
    from vsearch_amd import ChimeraSession
    tn, db, qn, qs = data
    s = ChimeraSession(aligner, db, labels=tn)
    recs = s.uchime_ref(qs)
    assert s.stats["queries_kernel"] > 100
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, env=dict(os.environ, VSX_CHIMERA="host"), timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    child = json.loads(p.stdout.strip().splitlines()[-1])
    assert child["stats"]["queries_kernel"] == 0 and child["stats"]["queries_host"] == s.stats["queries_kernel"] + s.stats["queries_host"]
    mine = [{k: (v.hex() if isinstance(v, float) else v) for k, v in r.items()} for r in recs]
    bad = [k for k, (a, b) in enumerate(zip(mine, child["recs"])) if a != b]
    assert len(mine) == len(child["recs"]) and not bad, (len(bad), qn[bad[0]], mine[bad[0]], child["recs"][bad[0]])


@pytest.mark.parametrize("variant", VARIANTS)
def test_denovo_lengths_match_reference_cli(aligner, reference, variant):
    """the parents and chimeras of 1024 / 1500 / 2049 / 4096 / 4097, the parents the more abundant"""
    from vsearch_amd import DenovoChimeraSession
    labels, seqs = cd.denovo_set()
    s = DenovoChimeraSession(aligner, seqs, labels, variant=variant)
    _diff(s.uchimeout(), reference[variant])
    assert sum(line.endswith("\tY") for line in reference[variant]) >= 2 * len(cd.DENOVO_LENGTHS)
    assert s.stats["queries_kernel"] > 0 and s.stats["queries_host"] > 0, s.stats
