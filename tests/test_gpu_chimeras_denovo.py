"""GPU (-m gpu): long-read de novo chimera detection on the device (vsearch_amd.ChimerasDenovoSession -> vsx_chimeras_denovo ->
vsx_chimera_long.hip).  The --tabbedout lines and the --chimeras / --nonchimeras label lists must equal the reference CLI's: the
stored golden outputs (tests/golden/chimeras_long_golden.json: the seeded set and every named edge input of
tests/chimeras_long_data.py) and live runs of oracle/_ref/vsearch_ref under the mask modes and the command's options.  Records must
not depend on the window size, the fix-up must be exercised, and the kernel's records must equal the host restatement's."""
import json
import os
import subprocess
import sys

import pytest

from oracle import refcli
from tests import chimeras_long_data as data

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = data.edge_cases()


def _need_ref():
    if not refcli.available():
        pytest.skip("oracle/_ref/vsearch_ref not built")


@pytest.fixture(scope="module")
def seeded():
    return data.seeded_set()


@pytest.fixture(scope="module")
def gold():
    return json.load(open(data.GOLDEN))


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


def _outputs(s):
    return dict(tabbedout=s.tabbedout(), chimeras=s.chimeras, nonchimeras=s.nonchimeras)


def _same(got, exp, floor=0):
    assert got["chimeras"] == exp["chimeras"] and got["nonchimeras"] == exp["nonchimeras"]
    bad = [(a, b) for a, b in zip(got["tabbedout"], exp["tabbedout"]) if a != b]
    assert not bad, f"{len(bad)} lines differ, first:\n got {bad[0][0]}\n ref {bad[0][1]}"
    assert len(got["tabbedout"]) == len(exp["tabbedout"])
    # a parity test must not pass on an input where nothing is chimeric: the floor comes from the reference's own output on the seed
    assert len(exp["tabbedout"]) >= floor, len(exp["tabbedout"])


def test_golden_seeded(aligner, gold):
    from vsearch_amd import ChimerasDenovoSession
    g = gold["seeded"]
    s = ChimerasDenovoSession(aligner, g["seqs"], g["labels"])
    _same(_outputs(s), g, floor=40)
    assert s.stats["queries_kernel"] > 0 and s.stats["queries_host"] > 0, s.stats


@pytest.mark.parametrize("hardmask", [0, 1])
@pytest.mark.parametrize("mask", ["dust", "soft", "none"])
def test_matches_reference_cli(aligner, seeded, tmp_path, mask, hardmask):
    _need_ref()
    from vsearch_amd import ChimerasDenovoSession
    labels, seqs = seeded
    exp = data.ref_outputs(str(tmp_path), labels, seqs, ["--qmask", mask] + (["--hardmask"] if hardmask else []))
    s = ChimerasDenovoSession(aligner, seqs, labels, soft_mask=mask, hardmask=hardmask)
    _same(_outputs(s), exp, floor=40)


OPTION_CASES = {
    "parts5": (["--chimeras_parts", "5"], dict(parts=5), 40),
    "parents_max2": (["--chimeras_parents_max", "2"], dict(parents_max=2), 25),
    "length_min40": (["--chimeras_length_min", "40"], dict(length_min=40), 30),
    "diff_pct1": (["--chimeras_diff_pct", "1"], dict(diff_pct=1.0), 45),
    "diff_pct2_5": (["--chimeras_diff_pct", "2.5"], dict(diff_pct=2.5), 45),
    "diff_pct0_1": (["--chimeras_diff_pct", "0.1"], dict(diff_pct=0.1), 40),
    "abskew2": (["--abskew", "2"], dict(abskew=2.0), 20),
}


@pytest.mark.parametrize("case", sorted(OPTION_CASES))
def test_matches_reference_cli_options(aligner, seeded, tmp_path, case):
    _need_ref()
    from vsearch_amd import ChimerasDenovoSession
    labels, seqs = seeded
    extra, opts, floor = OPTION_CASES[case]
    exp = data.ref_outputs(str(tmp_path), labels, seqs, extra)
    s = ChimerasDenovoSession(aligner, seqs, labels, **opts)
    _same(_outputs(s), exp, floor=floor)
    if "diff_pct" in opts:
        # multiples of 2^-13 are scanned by the kernel (the set's queries beyond its limits stay on the host), 0.1 is the host's
        if opts["diff_pct"] == 0.1:
            assert s.stats["queries_kernel"] == 0, s.stats
        else:
            assert s.stats["queries_kernel"] > 0 and s.stats["queries_host"] > 0, s.stats


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_input(aligner, gold, monkeypatch, name):
    """device = host restatement = the reference's stored lines"""
    from vsearch_amd import ChimerasDenovoSession
    c = EDGES[name]
    assert gold["edges"][name]["digest"] == data.case_digest(c["labels"], c["seqs"])
    s = ChimerasDenovoSession(aligner, c["seqs"], c["labels"], **c["opts"])
    dev = s.chimeras_denovo()
    _same(_outputs(s), gold["edges"][name])
    kernel = s.stats["queries_kernel"]
    if c["opts"].get("diff_pct", 0) == 0.1:
        assert kernel == 0 and s.stats["queries_host"] > 0, s.stats              # not a multiple of 2^-13: the host restatement
    elif not name.startswith(("qlen", "cand")):
        assert kernel > 0 and s.stats["queries_host"] == 0, s.stats
    if name in ("diff_pct1", "diff_pct2.5"):
        q = dev[-1]
        assert (q["flag"], q["n_parents"], sum(q["len"])) == ("Y", 2, 600)          # a region over the mismatch, on the kernel
        assert q["len"] == ([251, 349] if name == "diff_pct1" else [31, 569])
    if name.startswith("qlen"):
        # the variants and the query have the same length: all on the kernel up to the limit, none beyond it
        assert (s.stats["queries_host"] == 0) == (len(c["seqs"][-1]) <= data.QMAX), s.stats
    if name.startswith("cand"):
        # the query has as many candidates as there are variants (a variant itself has at most three)
        assert s.stats["queries_host"] == (1 if len(c["seqs"]) - 1 > data.CMAX else 0), s.stats
    monkeypatch.setenv("VSX_CHIMERA", "host")
    h = ChimerasDenovoSession(aligner, c["seqs"], c["labels"], **c["opts"])
    assert h.chimeras_denovo() == dev
    assert h.stats["queries_kernel"] == 0


def test_window_independence_and_passes(aligner, seeded):
    from vsearch_amd import ChimerasDenovoSession
    labels, seqs = seeded
    base = None
    passes_max = {}
    for w in (1, 7, 257, 0):
        s = ChimerasDenovoSession(aligner, seqs, labels, window=w)
        recs = s.chimeras_denovo()
        passes_max[w] = s.stats["passes_max"]
        if w == 1:
            assert s.stats["passes_max"] == 1 and s.stats["windows"] == len(recs)
        if base is None:
            base = recs
        else:
            assert recs == base, f"window {w} differs"
    assert passes_max[0] > 1 and passes_max[257] > 1, passes_max
    assert sum(r["flag"] == "Y" for r in base) >= 40


def test_kernel_matches_host_restatement(aligner, seeded, tmp_path):
    from vsearch_amd import ChimerasDenovoSession
    labels, seqs = seeded
    s = ChimerasDenovoSession(aligner, seqs, labels)
    dev = s.chimeras_denovo()
    assert s.stats["queries_kernel"] > 0 and s.stats["queries_host"] > 0, s.stats
    inp = tmp_path / "in.json"
    outp = tmp_path / "out.json"
    inp.write_text(json.dumps({"labels": labels, "seqs": seqs}))
    code = ("import json, sys\n"
            "from vsearch_amd import Aligner, ChimerasDenovoSession\n"
            "d = json.load(open(sys.argv[1]))\n"
            "with Aligner(device=0) as al:\n"
            "    s = ChimerasDenovoSession(al, d['seqs'], d['labels'])\n"
            "    r = s.chimeras_denovo()\n"
            "    json.dump({'recs': r, 'stats': s.stats}, open(sys.argv[2], 'w'))\n")
    env = dict(os.environ, VSX_CHIMERA="host")
    subprocess.run([sys.executable, "-c", code, str(inp), str(outp)], cwd=ROOT, env=env, check=True, timeout=600)
    host = json.loads(outp.read_text())
    assert host["stats"]["queries_kernel"] == 0
    assert host["recs"] == json.loads(json.dumps(dev))
    assert sum(r["flag"] == "Y" for r in dev) >= 40


def test_refusals(aligner):
    import ctypes as C

    from vsearch_amd import _lib
    from vsearch_amd.chimera import chimeras_long_default_opts
    from vsearch_amd.search import _blob, _meta
    lib = _lib.load()
    seqs = ["ACGTACGTTGCA" * 30, "TTGACCAGTACG" * 30]
    labels = ["a;size=4", "b;size=1"]
    blob, off, lens = _blob(seqs)
    out = (_lib.ChimerasLongResult * 2)()

    def run(mutate_search=None, meta=True, mutate_opts=None):
        o = chimeras_long_default_opts()
        if mutate_search:
            mutate_search(o.search)
        h = C.c_void_p()
        rc = lib.vsx_searcher_create(aligner.h, C.byref(h), C.byref(o.search), len(lens), C.cast(C.c_char_p(blob), C.c_void_p),
                                     len(blob), off.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p))
        assert rc == _lib.VSX_OK
        try:
            if meta:
                m, keep = _meta([4, 1], labels, 2)
                assert lib.vsx_searcher_set_meta(h, C.byref(m)) == _lib.VSX_OK
            if mutate_opts:
                mutate_opts(o)
            return lib.vsx_chimeras_denovo(h, C.byref(o), out)
        finally:
            lib.vsx_searcher_destroy(h)

    assert run() == _lib.VSX_OK
    assert run(lambda s: setattr(s, "strand_both", 1)) == _lib.VSX_EINVAL
    assert run(meta=False) == _lib.VSX_EINVAL
    assert run(lambda s: setattr(s, "wordlength", 9)) == _lib.VSX_EINVAL
    assert run(lambda s: setattr(s, "maxsizeratio", 0.5)) == _lib.VSX_EINVAL          # not 1 / abskew
    assert run(lambda s: setattr(s, "selfid", 0)) == _lib.VSX_EINVAL
    assert run(lambda s: setattr(s, "maxaccepts", 1)) == _lib.VSX_EINVAL
    assert run(mutate_opts=lambda o: setattr(o, "abskew", 4.0)) == _lib.VSX_EINVAL     # maxsizeratio no longer 1 / abskew
    assert run(mutate_opts=lambda o: setattr(o, "parents_max", 21)) == _lib.VSX_EINVAL
