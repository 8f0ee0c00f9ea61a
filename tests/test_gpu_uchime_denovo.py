"""GPU (-m gpu): de novo chimera detection on the device (vsearch_amd.DenovoChimeraSession -> vsx_uchime_denovo -> vsx_chimera.hip).
The --uchimeout lines must equal the reference CLI's byte for byte: the stored golden lines (tests/golden/uchime_denovo_golden.json)
and live runs of oracle/_ref/vsearch_ref on the seeded cascade set of tests/denovo_data.py under every variant and mask mode.
Records must not depend on the window size, the fix-up must be exercised (several passes in one window), and the kernel's records
must equal the host restatement's (VSX_CHIMERA=host, a fresh child process)."""
import json
import os
import subprocess
import sys

import pytest

from oracle import refcli
from tests import denovo_data

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _need_ref():
    if not refcli.available():
        pytest.skip("oracle/_ref/vsearch_ref not built")


@pytest.fixture(scope="module")
def cascade():
    return denovo_data.cascade_set()


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


def _diff(got, exp):
    assert len(got) == len(exp)
    bad = [(a, b) for a, b in zip(got, exp) if a != b]
    assert not bad, f"{len(bad)} lines differ, first:\n got {bad[0][0]}\n ref {bad[0][1]}"


@pytest.mark.parametrize("variant", ["uchime", "uchime2", "uchime3"])
def test_golden(aligner, variant):
    from vsearch_amd import DenovoChimeraSession
    gold = json.load(open(denovo_data.GOLDEN))
    s = DenovoChimeraSession(aligner, gold["seqs"], gold["labels"], variant=variant)
    _diff(s.uchimeout(), gold["uchimeout"][variant])
    assert s.stats["queries_kernel"] > 0 and s.stats["queries_host"] > 0, s.stats


@pytest.mark.parametrize("variant", ["uchime", "uchime2", "uchime3"])
@pytest.mark.parametrize("mask", ["dust", "soft", "none"])
def test_matches_reference_cli(aligner, cascade, tmp_path, variant, mask):
    _need_ref()
    from vsearch_amd import DenovoChimeraSession
    labels, seqs = cascade
    exp = denovo_data.ref_lines(str(tmp_path), labels, seqs, variant, ["--qmask", mask])
    s = DenovoChimeraSession(aligner, seqs, labels, variant=variant, soft_mask=mask)
    _diff(s.uchimeout(), exp)
    flags = [line.rsplit("\t", 1)[1] for line in exp]
    assert flags.count("Y") > (0 if variant == "uchime3" else 20), flags.count("Y")     # (abskew 16: few chimeras have two parents)


@pytest.mark.parametrize("case", ["hardmask", "params", "abskew1", "abskew3_5"])
def test_matches_reference_cli_options(aligner, cascade, tmp_path, case):
    _need_ref()
    from vsearch_amd import DenovoChimeraSession
    labels, seqs = cascade
    extra, opts = {
        "hardmask": (["--qmask", "dust", "--hardmask"], dict(hardmask=1)),
        "params": (["--minh", "0.2", "--mindiv", "1.5", "--mindiffs", "4", "--xn", "6.5", "--dn", "1.1"],
                   dict(minh=0.2, mindiv=1.5, mindiffs=4, xn=6.5, dn=1.1)),
        "abskew1": (["--abskew", "1.0"], dict(abskew=1.0)),
        "abskew3_5": (["--abskew", "3.5", "--qmask", "soft", "--hardmask"], dict(abskew=3.5, soft_mask=1, hardmask=1)),
    }[case]
    exp = denovo_data.ref_lines(str(tmp_path), labels, seqs, "uchime", extra)
    got = DenovoChimeraSession(aligner, seqs, labels, **opts).uchimeout()
    _diff(got, exp)


def test_window_independence_and_passes(aligner, cascade):
    from vsearch_amd import DenovoChimeraSession
    labels, seqs = cascade
    base = None
    passes_max = {}
    for w in (1, 7, 257, 0):
        s = DenovoChimeraSession(aligner, seqs, labels, window=w)
        recs = s.uchime_denovo()
        passes_max[w] = s.stats["passes_max"]
        if w == 1:
            assert s.stats["passes_max"] == 1 and s.stats["windows"] == len(recs)
        if base is None:
            base = recs
        else:
            assert recs == base, f"window {w} differs"
    assert passes_max[0] > 1 and passes_max[257] > 1, passes_max


def test_kernel_matches_host_restatement(aligner, cascade, tmp_path):
    from vsearch_amd import DenovoChimeraSession
    labels, seqs = cascade
    s = DenovoChimeraSession(aligner, seqs, labels)
    dev = s.uchime_denovo()
    assert s.stats["queries_kernel"] > 0 and s.stats["queries_host"] > 0, s.stats
    inp = tmp_path / "in.json"
    outp = tmp_path / "out.json"
    inp.write_text(json.dumps({"labels": labels, "seqs": seqs}))
    code = ("import json, sys\n"
            "from vsearch_amd import Aligner, DenovoChimeraSession\n"
            "d = json.load(open(sys.argv[1]))\n"
            "with Aligner(device=0) as al:\n"
            "    s = DenovoChimeraSession(al, d['seqs'], d['labels'])\n"
            "    r = s.uchime_denovo()\n"
            "    json.dump({'recs': r, 'stats': s.stats}, open(sys.argv[2], 'w'))\n")
    env = dict(os.environ, VSX_CHIMERA="host")
    subprocess.run([sys.executable, "-c", code, str(inp), str(outp)], cwd=ROOT, env=env, check=True, timeout=900)
    host = json.loads(outp.read_text())
    assert host["stats"]["queries_kernel"] == 0
    assert host["recs"] == json.loads(json.dumps(dev))


def test_refusals(aligner):
    import ctypes as C

    from vsearch_amd import _lib
    from vsearch_amd.chimera import denovo_default_opts
    from vsearch_amd.search import _blob, _meta
    lib = _lib.load()
    seqs = ["ACGTACGTTGCA" * 30, "TTGACCAGTACG" * 30]
    labels = ["a;size=4", "b;size=1"]
    blob, off, lens = _blob(seqs)
    out = (_lib.ChimeraResult * 2)()

    def run(mutate_search=None, meta=True, mutate_opts=None):
        o = denovo_default_opts("uchime")
        if mutate_search:
            mutate_search(o.base.search)
        h = C.c_void_p()
        rc = lib.vsx_searcher_create(aligner.h, C.byref(h), C.byref(o.base.search), len(lens), C.cast(C.c_char_p(blob), C.c_void_p),
                                     len(blob), off.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p))
        assert rc == _lib.VSX_OK
        try:
            if meta:
                m, keep = _meta([4, 1], labels, 2)
                assert lib.vsx_searcher_set_meta(h, C.byref(m)) == _lib.VSX_OK
            if mutate_opts:
                mutate_opts(o)
            return lib.vsx_uchime_denovo(h, C.byref(o), out)
        finally:
            lib.vsx_searcher_destroy(h)

    assert run() == _lib.VSX_OK
    assert run(lambda s: setattr(s, "strand_both", 1)) == _lib.VSX_EINVAL
    assert run(meta=False) == _lib.VSX_EINVAL
    assert run(lambda s: setattr(s, "wordlength", 9)) == _lib.VSX_EINVAL
    assert run(lambda s: setattr(s, "maxsizeratio", 1.0)) == _lib.VSX_EINVAL          # not 1 / abskew
    assert run(lambda s: setattr(s, "selfid", 0)) == _lib.VSX_EINVAL
    assert run(lambda s: setattr(s, "maxaccepts", 1)) == _lib.VSX_EINVAL
    assert run(mutate_opts=lambda o: setattr(o, "abskew", 4.0)) == _lib.VSX_EINVAL     # maxsizeratio no longer 1 / abskew


def test_bench_workload_prefix(aligner, tmp_path):
    """the bench's workload at 20 000 sequences; the first 2 000 lines against the CLI's run on those 2 000 sequences"""
    _need_ref()
    import bench_uchime_denovo as bench
    from vsearch_amd import DenovoChimeraSession
    labels, seqs = bench.workload(20_000)
    s = DenovoChimeraSession(aligner, seqs, labels)
    got = s.uchimeout()
    assert len(got) == 20_000
    k = 2000
    exp = denovo_data.ref_lines(str(tmp_path), s.labels[:k], s.seqs[:k], "uchime")
    _diff(got[:k], exp)
    assert sum(1 for line in got if line.endswith("\tY")) > 1000
