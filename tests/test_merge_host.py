"""Paired-end merging without a device: the C-ABI surface of include/vsx_merge.h and the host restatement
(VSX_MERGE=host) against recorded answers of the reference CLI.

tests/golden/merge_golden.json was produced by `python tests/merge_data.py tests/golden/merge_golden.json
<reference>/api_examples/data` (merge_data.write_golden): the pairs of merge_data.generate(11, 200, read_len=48) plus
merge_data.edge_pairs() were written as FASTQ and given to the reference's `--fastq_mergepairs ... --threads 1` under the
three option sets of merge_data.GOLDEN_OPTION_SETS; recorded are the lines of --fastqout (with --fastq_eeout) and
--eetabbedout, the labels of --fastqout_notmerged_fwd and the counts of the statistics block in --log.  "example" holds
the reference's own api_examples/data/merge_fwd.fastq / merge_rev.fastq with expected_merge.fasta and the same CLI
outputs at default options.  Data and expected output only.

The quality cases carry the reference CLI's recorded behaviour (fatal error or a normal run); where build() has left the
reference binary in oracle/_ref, the test also asks it again.
"""
import ctypes as C
import json
import os
import sys

import pytest

from tests import merge_data as md

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture()
def host_merge(monkeypatch):
    monkeypatch.setenv("VSX_MERGE", "host")
    from vsearch_amd.merge import merge_pairs
    return lambda *a, **k: merge_pairs(None, *a, **k)


def assert_matches(res, labels, ref):
    assert res.fastq_lines(labels, eeout=True) == ref["fastq"]
    assert res.eetabbed_lines() == ref["eetabbed"]
    assert [labels[k] for k in res.not_merged_indices()] == ref["notmerged"]
    assert res.reason_counts() == ref["reasons"]


def test_abi_surface_and_defaults():
    from vsearch_amd import _lib
    lib = _lib.load()
    for name in _lib.MERGE_SYMBOLS:
        assert hasattr(lib, name), name
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "vsx_merge.h")).read()
    import re
    declared = set(re.findall(r"\b(vsx_merge_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.MERGE_SYMBOLS), declared ^ set(_lib.MERGE_SYMBOLS)
    o = _lib.MergeOpts()
    lib.vsx_merge_opts_default(C.byref(o))
    # src/vsearch.h
    assert (o.fastq_ascii, o.fastq_qmin, o.fastq_qmax, o.fastq_qminout, o.fastq_qmaxout) == (33, 0, 41, 0, 41)
    assert (o.fastq_minovlen, o.fastq_maxdiffs, o.fastq_maxdiffpct) == (10, 10, 100.0)
    assert (o.fastq_minmergelen, o.fastq_maxmergelen) == (0, 1000000)
    assert o.fastq_maxee == sys.float_info.max
    assert o.fastq_truncqual == -2 ** 63 and o.fastq_maxns == 2 ** 63 - 1
    assert (o.fastq_minlen, o.fastq_maxlen) == (1, 2 ** 63 - 1)
    assert o.fastq_allowmergestagger == 0 and o.window == 0
    assert C.sizeof(_lib.MergeRecord) == 64


def test_no_context_is_an_error_outside_host_mode(monkeypatch):
    from vsearch_amd import VsxError
    from vsearch_amd.merge import merge_pairs
    monkeypatch.delenv("VSX_MERGE", raising=False)
    with pytest.raises(VsxError):
        merge_pairs(None, ["ACGT"], ["IIII"], ["ACGT"], ["IIII"])


def test_golden_host_path(host_merge):
    doc = md.load_golden(os.path.join(HERE, "golden", "merge_golden.json"))
    i = doc["inputs"]
    assert len(doc["cases"]) == len(md.GOLDEN_OPTION_SETS)
    seen = set()
    for case in doc["cases"]:
        res = host_merge(i["fwd"], i["fqual"], i["rev"], i["rqual"], **case["opts"])
        assert_matches(res, i["labels"], case)
        assert res.stats["pairs_host"] == len(i["labels"])
        seen |= set(case["reasons"])
    assert seen == {"minlen", "maxlen", "maxns", "minovlen", "maxdiffs", "maxdiffpct", "staggered", "repeat", "minmergelen",
                    "maxmergelen", "maxee", "minscore", "nokmers"}
    e = doc["example"]
    i = e["inputs"]
    res = host_merge(i["fwd"], i["fqual"], i["rev"], i["rqual"])
    assert_matches(res, i["labels"], e)
    assert res.records["merged"].all()
    assert res.sequence(0) == e["expected_fasta"].split("\n", 1)[1].replace("\n", "")
    r = res.records[0]
    assert r["overlap_length"] == r["fwd_trunc"] + r["rev_trunc"] - r["merged_length"]


def test_minovlen_below_five_reads_as_five(host_merge):
    labels, fwd, fqual, rev, rqual = md.generate(3, 300, read_len=120)
    a, b = host_merge(fwd, fqual, rev, rqual, minovlen=5), host_merge(fwd, fqual, rev, rqual, minovlen=1)
    assert a.records.tobytes() == b.records.tobytes() and a.seq_blob == b.seq_blob


FRAG = "GATTACAGGCCTGTAATCAACGTTGCATTCGAGCTAGCTAGGATCCAAGGTTCCAATTGGCCAAGCTTGCATGCCTGCAGGTCGACTCTAGAGGATCCCCGGGTACCGAGCTCGAATTC"


def _pair(fq=None, rq=None):
    rc = md.revcomp(md.np.frombuffer(FRAG.encode(), md.np.uint8)).tobytes().decode()
    f, r = FRAG[:80], rc[:80]
    return [["good", "probe"], [f, f], ["I" * 80, fq or "I" * 80], [r, r], ["I" * 80, rq or "I" * 80]]


def _put(q, pos, ch):
    return q[:pos] + ch + q[pos + 1:]


# (name, pair builder, options, what the reference CLI does: None = runs through, else (kind, value, bound) of its fatal error)
QUALITY_CASES = [
    ("above_qmax_inside", lambda: _pair(rq=_put("I" * 80, 30, "K")), {}, ("above qmax", 42, 41)),
    ("above_qmax_allowed", lambda: _pair(rq=_put("I" * 80, 30, "K")), {"qmax": 42}, None),
    ("below_qmin_inside", lambda: _pair(fq=_put("I" * 80, 10, "$")), {"qmin": 5}, ("below qmin", 3, 5)),
    ("beyond_truncation", lambda: _pair(rq=_put(_put("I" * 80, 60, "#"), 70, "K")), {"truncqual": 2}, None),
    ("at_truncation_first", lambda: _pair(rq=_put(_put("I" * 80, 60, "K"), 70, "#")), {"truncqual": 2}, ("above qmax", 42, 41)),
    ("pair_fails_length_check", lambda: _pair(rq=_put("I" * 80, 30, "K")), {"maxlen": 79}, None),
    ("forward_truncated_below_minlen", lambda: _pair(fq=_put("I" * 80, 5, "#"), rq=_put("I" * 80, 30, "K")),
     {"truncqual": 2, "minlen": 20}, None),
    ("forward_read_first", lambda: _pair(fq=_put("I" * 80, 50, "L"), rq=_put("I" * 80, 3, "K")), {}, ("above qmax", 43, 41)),
]


@pytest.mark.parametrize("name,build,opts,fatal", QUALITY_CASES, ids=[c[0] for c in QUALITY_CASES])
def test_out_of_range_quality(host_merge, name, build, opts, fatal):
    from vsearch_amd import VsxError
    data = build()
    if os.path.exists(md.ref_binary()):
        ref = md.run_reference(*data, **opts)
        assert (ref["returncode"] != 0) == (fatal is not None), ref["stderr"]
        if fatal:
            assert f"FASTQ quality value ({fatal[1]}) {fatal[0]} ({fatal[2]})" in ref["stderr"]
    if fatal is None:
        res = host_merge(*data[1:], **opts)
        assert len(res) == 2
        if os.path.exists(md.ref_binary()):
            assert_matches(res, data[0], ref)
    else:
        with pytest.raises(VsxError, match=rf"FASTQ quality value \({fatal[1]}\) {fatal[0]} \({fatal[2]}\)") as ei:
            host_merge(*data[1:], **opts)
        assert ei.value.code == -1          # VSX_EINVAL


needs_cli = pytest.mark.skipif(not os.path.exists(md.ref_binary()), reason="oracle/_ref/vsearch_ref not built")


@needs_cli
def test_boundary_pairs_host_path(host_merge):
    """merge_data.boundary_pairs() (tests/test_gpu_merge_edges.py runs it through the kernel): the host path against the live
    reference, and the conditions the list must meet, on the reference's own output"""
    from tests.test_gpu_merge_edges import BOUNDARY_RUNS, check_boundary_reference
    data = md.boundary_pairs()
    assert len(set(data[0])) == len(data[0])
    refs = []
    for extra in BOUNDARY_RUNS:
        opts = dict(md.BOUNDARY_OPTS, **extra)
        refs.append(md.run_reference(*data, **opts))
        assert refs[-1]["returncode"] == 0, refs[-1]["stderr"]
        assert_matches(host_merge(*data[1:], **opts), data[0], refs[-1])
    check_boundary_reference(refs)
    k = data[0].index("cap_homopolymer_512")
    assert host_merge(*[[col[k]] for col in data[1:]]).stats["diagonals_scored"] >= 1000
    # each capacity pair on its own, at the reference's defaults: `repeat`; the pairs whose two best diagonals tie below minscore:
    # `minscore` (the first, unstaggered diagonal wins; the second would give `staggered`)
    for k, lab in enumerate(data[0]):
        if lab.startswith("cap_"):
            alone = [[col[k]] for col in data]
            want = {"minscore": 1} if "tie" in lab else {"repeat": 1}
            ref = md.run_reference(*alone)
            assert ref["returncode"] == 0 and ref["reasons"] == want, (lab, ref["reasons"])
            assert host_merge(*alone[1:]).reason_counts() == want, lab


@needs_cli
@pytest.mark.parametrize("which", [0, 2])
def test_encoding_sets_host_path(host_merge, which):
    from tests.test_gpu_merge_edges import ENCODING_SETS, check_encoding_reference, encoding_data
    name, ascii, qmin, qmax, opts = ENCODING_SETS[which]
    data = encoding_data(ascii, qmin, qmax)
    opts = dict(opts, maxns=4)
    ref = md.run_reference(*data, **opts)
    check_encoding_reference(data, ref, ascii, opts)
    assert_matches(host_merge(*data[1:], **opts), data[0], ref)
