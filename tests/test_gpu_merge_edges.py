"""Paired-end merging on the device at the boundaries of vsx_merge.hip (one wave per pair, 64 lanes striding over positions and
diagonals) and under quality encodings other than the default, against the reference CLI and against the host restatement.

merge_data.boundary_pairs(): read lengths 5 .. 512 around the multiples of 64 with exact overlaps and staggers, truncation points
at 0 / 1 / 63 / 64 / 65 / 127 / 128 / 191 / 192 / 249, low-complexity pairs at 512 x 512 (every diagonal listed and scored), tied
best diagonals, and N counts on --fastq_maxns spread over the lanes.  ENCODING_SETS: --fastq_ascii 64, qmax 93, qmin above and
below 0, qminout / qmaxout: the device reads a slice of the host's quality tables that starts at min(ascii + qmin, ascii).

Every comparison is exact and over all pairs (tests/test_gpu_merge.py: assert_matches, assert_same_records).  The conditions the
inputs must meet are asserted on the reference's own output and on the inputs, never on the kernel's answers;
tests/test_merge_host.py runs the same inputs through the host path without a device.
"""
import pytest

from tests import merge_data as md
from tests.test_gpu_merge import aligner, assert_matches, assert_same_records, host_path, needs_cli  # noqa: F401

pytestmark = pytest.mark.gpu

# (ascii, qmin, qmax, further options); the generated qualities run over qmin .. qmax (from 2 where qmin is left at 0: a
# quality below 2 turns the base into N for the merge)
ENCODING_SETS = [
    ("ascii64_qmin-5", 64, -5, 41, dict(ascii=64, qmin=-5, qmax=41, qmaxout=41)),
    ("qmax93", 33, 0, 93, dict(qmax=93, qmaxout=93)),
    ("qmin10_qmax30", 33, 10, 30, dict(qmin=10, qmax=30)),
    ("ascii64_qmax62_qminout20", 64, 0, 62, dict(ascii=64, qmax=62, qminout=20, qmaxout=62)),
    ("qminout20_qmaxout20", 33, 0, 41, dict(qminout=20, qmaxout=20)),
    ("qmaxout60_truncqual9", 33, 0, 41, dict(qmaxout=60, truncqual=9)),
]


def encoding_data(ascii, qmin, qmax, n=1500):
    """n generated pairs of 120 in the encoding plus the N group (its forced quality symbol is `ascii`, below ascii + qmin when
    qmin > 0)"""
    g = md.generate(20270 + ascii + qmax, n, read_len=120, ascii=ascii, qrange=(qmin if qmin else 2, qmax))
    e = md.n_pairs(ascii=ascii, q=min(qmax, 40))
    return [a + b for a, b in zip(g, e)]


def check_encoding_reference(data, ref, ascii, opts):
    """the conditions of an encoding set, on the reference's output and the inputs"""
    assert ref["returncode"] == 0, ref["stderr"]
    quals = "".join(ref["fastq"][3::4])
    qmaxout, qminout = opts.get("qmaxout", 41), opts.get("qminout", 0)
    assert chr(ascii + qmaxout) in quals, f"no merged quality reaches qmaxout {qmaxout}"
    if qminout > 3:
        assert chr(ascii + qminout) in quals, f"no merged quality sits on qminout {qminout}"
    index = {lab: k for k, lab in enumerate(data[0])}
    nf = nr = 0
    for head, seq in zip(ref["fastq"][0::4], ref["fastq"][1::4]):
        k = index[head[1:].split(";ee=")[0]]
        a, b = md.disagreement_sides(data[1][k], data[2][k], data[3][k], data[4][k], len(seq), ascii, opts.get("truncqual"))
        nf += a > 0
        nr += b > 0
    assert nf > 0 and nr > 0, f"merged pairs with a disagreement won by the forward read: {nf}, by the reverse read: {nr}"


def check_boundary_reference(refs):
    seen = set()
    for ref in refs:
        assert ref["returncode"] == 0, ref["stderr"]
        seen |= set(ref["reasons"]) | ({"ok"} if ref["fastq"] else set())
    assert {"ok", "minovlen", "staggered", "repeat", "maxns", "nokmers"} <= seen, seen


BOUNDARY_RUNS = [{}, dict(minovlen=5), dict(allowmergestagger=True)]


@needs_cli
def test_boundary_pairs_match_reference(aligner):
    from vsearch_amd.merge import merge_pairs
    data = md.boundary_pairs()
    refs = []
    for extra in BOUNDARY_RUNS:
        opts = dict(md.BOUNDARY_OPTS, **extra)
        ref = md.run_reference(*data, **opts)
        refs.append(ref)
        assert ref["returncode"] == 0, ref["stderr"]
        res = merge_pairs(aligner, *data[1:], **opts)
        assert res.stats["pairs_host"] == 0
        assert_matches(res, data[0], ref)
    check_boundary_reference(refs)
    # the groups that need neither truncqual nor maxns, at the reference's defaults
    keep = [k for k, lab in enumerate(data[0]) if not lab.startswith(("trunc_", "n_"))]
    part = [[col[k] for k in keep] for col in data]
    ref = md.run_reference(*part)
    assert ref["returncode"] == 0, ref["stderr"]
    assert_matches(merge_pairs(aligner, *part[1:]), part[0], ref)
    # two tied diagonals below minscore: the first, unstaggered one wins (the reference's verdicts for the cap_* pairs, each
    # on its own, are asserted in tests/test_merge_host.py)
    for k, lab in enumerate(part[0]):
        if lab.startswith("cap_tie"):
            assert merge_pairs(aligner, *[[col[k]] for col in part[1:]]).reason_counts() == {"minscore": 1}


def test_capacity_every_diagonal_scored(aligner):
    """512 x 512 homopolymer: 1 023 diagonals, all but the shortest pass the census; the list of the kernel holds 1 024"""
    from vsearch_amd.merge import merge_pairs
    data = md.boundary_pairs()
    k = data[0].index("cap_homopolymer_512")
    res = merge_pairs(aligner, *[[col[k]] for col in data[1:]])
    assert res.stats["diagonals_scored"] >= 1000 and res.stats["pairs_host"] == 0, res.stats
    assert res.reason_counts() == {"repeat": 1}


def test_boundary_pairs_kernel_equals_host_path(aligner):
    from vsearch_amd.merge import merge_pairs
    data = md.boundary_pairs()
    for extra in BOUNDARY_RUNS + [dict(minovlen=5, allowmergestagger=True, maxns=0, truncqual=30)]:
        opts = dict(md.BOUNDARY_OPTS, **extra)
        dev = merge_pairs(aligner, *data[1:], **opts)
        with host_path():
            host = merge_pairs(None, *data[1:], **opts)
        assert host.stats["pairs_host"] == len(data[0]) and dev.stats["pairs_host"] == 0
        assert_same_records(dev, host)


@needs_cli
@pytest.mark.parametrize("name,ascii,qmin,qmax,opts", ENCODING_SETS, ids=[s[0] for s in ENCODING_SETS])
def test_encoding_sets_match_reference(aligner, name, ascii, qmin, qmax, opts):
    from vsearch_amd.merge import merge_pairs
    data = encoding_data(ascii, qmin, qmax)
    opts = dict(opts, maxns=4)
    ref = md.run_reference(*data, **opts)
    check_encoding_reference(data, ref, ascii, opts)
    res = merge_pairs(aligner, *data[1:], **opts)
    assert res.stats["pairs_host"] == 0
    assert_matches(res, data[0], ref)
    with host_path():
        host = merge_pairs(None, *data[1:], **opts)
    assert_same_records(res, host)


@needs_cli
@pytest.mark.parametrize("swapped,value", [(False, 43), (True, 42)])
def test_quality_error_names_the_first_bad_value(aligner, swapped, value):
    """pair 40 and pair 130 both hold a quality above qmax, one on the host route (reads above 512) and one on the device, in
    different windows: the error names the one the reference meets first"""
    from vsearch_amd import VsxError
    from vsearch_amd.merge import merge_pairs
    data = md.quality_order_pairs(swapped)
    assert (len(data[1][130 if swapped else 40]), len(data[1][40 if swapped else 130])) == (600, 100)
    ref = md.run_reference(*data)
    assert ref["returncode"] != 0 and f"FASTQ quality value ({value}) above qmax (41)" in ref["stderr"], ref["stderr"]
    with pytest.raises(VsxError, match=rf"quality value \({value}\) above qmax \(41\)"):
        merge_pairs(aligner, *data[1:], window=64)
