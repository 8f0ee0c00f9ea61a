"""Read summary statistics on the device (vsx_fastq_stats, vsx_fastq_chars, vsearch_amd.fastq_stats) against the library's host
restatement (VSX_FASTQ_STATS=host) field for field with sum_ee compared by bit pattern, against the recorded texts of the
reference CLI (tests/golden/fastq_stats_golden.json, see tests/test_fastq_stats_host.py for how it was recorded), and once
against the live reference binary build() leaves in oracle/_ref (skipped only where that binary is absent).

No call has more than 2 000 reads and no read more than 300 positions.
"""
import contextlib
import os

import numpy as np
import pytest

from tests import fastq_stats_data as fd

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
needs_cli = pytest.mark.skipif(not os.path.exists(fd.ref_binary()), reason="oracle/_ref/vsearch_ref not built")


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


@pytest.fixture(scope="module")
def golden():
    return fd.load_golden(os.path.join(HERE, "golden", "fastq_stats_golden.json"))


@contextlib.contextmanager
def host_path():
    old = os.environ.get("VSX_FASTQ_STATS")
    os.environ["VSX_FASTQ_STATS"] = "host"
    try:
        yield
    finally:
        if old is None:
            del os.environ["VSX_FASTQ_STATS"]
        else:
            os.environ["VSX_FASTQ_STATS"] = old


def on_device(aligner, s, command, **extra):
    res = fd.call(aligner, s, command, **extra)
    assert res.stats["reads_host"] == 0 and res.stats["reads"] == len(s["quals"])
    assert res.stats["windows"] >= 1 or sum(len(q) for q in s["quals"]) == 0
    return res


_HOST = {}


def on_host(s, command):
    """the host restatement's answer, computed once per set and command"""
    key = (s["name"], command, s["tail"], len(s["quals"]))
    if key not in _HOST:
        with host_path():
            res = fd.call(None, s, command)
        assert res.stats["reads_host"] == res.stats["reads"]
        _HOST[key] = res
    return _HOST[key]


def all_sets():
    return fd.golden_sets() + fd.order_reads()


def test_golden_on_device(aligner, golden):
    for d in golden["sets"] + golden["order"]:
        s = d["input"]
        for command in s["commands"]:
            assert on_device(aligner, s, command).log_lines() == d["expected"][command], (s["name"], command)


@pytest.mark.parametrize("window", [0, 1, 7])
def test_every_set_equals_host(aligner, window):
    for s in all_sets():
        for command in s["commands"]:
            fd.assert_same_tables(on_device(aligner, s, command, window=window), on_host(s, command), f"{s['name']} {command} window {window}")


def test_window_counts(aligner):
    s = fd.generate(77, 100, read_len=90)
    for command in fd.BOTH:
        assert on_device(aligner, s, command).stats["windows"] == 1
        assert on_device(aligner, s, command, window=1).stats["windows"] == 100 and on_device(aligner, s, command, window=7).stats["windows"] == 15


def test_scattered_offsets(aligner):
    """shuffled, non-monotonic offsets into larger blobs with shared bytes and junk between the reads"""
    for s in (fd.generate(77, 100, read_len=90), [x for x in fd.edge_reads() if x["name"] == "reads_257"][0]):
        for command in fd.BOTH:
            base = on_host(s, command)
            for window in (0, 7):
                res = fd.scattered_call(aligner, s, command, seed=5, window=window)
                assert res.stats["reads_host"] == 0
                fd.assert_same_tables(res, base, f"{s['name']} {command} scattered, window {window}")


@pytest.mark.parametrize("seed", [31, 32])
def test_generated_reads_equal_host(aligner, seed):
    """reads up to 300 positions, several workgroups, several steps of the ordered sum, windows that split both"""
    s = fd.generate(seed, 1500, read_len=300, opts={"qmax": 45} if seed % 2 else {}, tail=2 + seed % 2)
    for command in fd.BOTH:
        for window in (0, 700):
            fd.assert_same_tables(on_device(aligner, s, command, window=window), on_host(s, command), f"{s['name']} {command} window {window}")


def test_read_order_shows_and_is_kept(aligner):
    """sum_ee of the reversed input differs in bits from the forward one, on the device as on the host"""
    for s in fd.order_reads():
        r = dict(s, name=s["name"] + "_reversed", quals=s["quals"][::-1], seqs=s["seqs"][::-1])
        forward, backward = on_device(aligner, s, "stats"), on_device(aligner, r, "stats", window=2)
        i = s["position"]
        assert forward.sum_ee.view(np.uint64)[i] != backward.sum_ee.view(np.uint64)[i], s["name"]
        fd.assert_same_tables(forward, on_host(s, "stats"), "forward")
        fd.assert_same_tables(backward, on_host(r, "stats"), "backward")
    s = fd.generate(78, 2000, read_len=80)
    r = dict(s, name="generate_78_reversed", quals=s["quals"][::-1], seqs=s["seqs"][::-1])
    forward, backward = on_device(aligner, s, "stats"), on_device(aligner, r, "stats", window=300)
    assert (forward.sum_ee.view(np.uint64) != backward.sum_ee.view(np.uint64)).any()
    fd.assert_same_tables(forward, on_host(s, "stats"), "forward")
    fd.assert_same_tables(backward, on_host(r, "stats"), "backward")


def test_refused_inputs_name_the_same_read(aligner, golden):
    from vsearch_amd import VsxError
    from vsearch_amd.fastq_stats import chars_of_blob, stats_of_blob
    for d in golden["quality"]:
        s, fatal = d["input"], d["fatal"]
        with host_path(), pytest.raises(VsxError) as host_error:
            fd.call(None, s, "stats")
        for extra in ({}, {"window": 7}, {"window": 1}):
            with pytest.raises(VsxError, match=rf"FASTQ quality value \({fatal[0]}\) out of range \({fatal[1]}-{fatal[2]}\)") as ei:
                fd.call(aligner, s, "stats", **extra)
            assert ei.value.code == -1 and str(ei.value) == str(host_error.value), s["name"]
    # a quality byte outside 33 ... 126, in the second workgroup
    quals = ["IIIIIIII"] * 300
    quals[280] = "IIII\x7fIII"
    qual = "".join(quals).encode()
    off, lens = np.arange(300, dtype=np.uint64) * 8, np.full(300, 8, np.uint32)
    for run in (lambda: stats_of_blob(aligner, qual, off, lens), lambda: chars_of_blob(aligner, b"ACGTACGT" * 300, qual, off, lens, window=64)):
        with pytest.raises(VsxError, match="outside 33 ... 126") as ei:
            run()
        assert ei.value.code == -1


def test_forced_host_route(aligner):
    s = fd.generate(79, 50, read_len=100)
    for command in fd.BOTH:
        with host_path():
            forced = fd.call(aligner, s, command)
        assert forced.stats["reads_host"] == 50 and forced.stats["windows"] == 0
        fd.assert_same_tables(forced, on_device(aligner, s, command))


@needs_cli
def test_live_reference_on_device(aligner):
    s = fd.generate(2024, 2000, read_len=250)
    ref = fd.run_reference(s)
    assert ref["returncode"] == 0, ref["stderr"]
    for command in fd.BOTH:
        assert on_device(aligner, s, command).log_lines() == ref[command], command
