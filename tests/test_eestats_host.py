"""Read statistics without a device: the C-ABI surface of include/vsx_eestats.h and the host restatement (VSX_EESTATS=host)
against the plain-Python restatements of tests/eestats_data.py, table for table with sum_ee compared by bit pattern, and
against recorded texts of the reference CLI.

tests/golden/fastq_eestats_golden.json was produced by `python -m tests.eestats_data tests/golden/fastq_eestats_golden.json`
(eestats_data.write_golden): the sets of golden_sets() (edge_reads() and two seeded generate() sets) and the one-read sets of
rounding_reads() were written as FASTQ and given to the reference's `--fastq_eestats` / `--fastq_eestats2 ... --output`; recorded
are the lines of the outputs each set names, and for quality_cases() the value and the bound of the reference's fatal message.
Data and expected output only.

Where build() has left the reference binary in oracle/_ref, fresh sets are also given to it again.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import eestats_data as ed

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fastq_eestats_golden.json")
needs_cli = pytest.mark.skipif(not os.path.exists(ed.ref_binary()), reason="oracle/_ref/vsearch_ref not built")


@pytest.fixture()
def host_stats(monkeypatch):
    monkeypatch.setenv("VSX_EESTATS", "host")

    def run(s, **extra):
        res = ed.call(None, s, **extra)
        assert res.stats["reads_host"] == res.stats["reads"] == len(s["quals"]) and res.stats["windows"] == 0
        return res
    return run


@pytest.fixture(scope="module")
def golden():
    return ed.load_golden(GOLDEN)


def lines_of(res, command):
    return res.eestats_lines() if command == "eestats" else res.eestats2_lines()


def test_abi_surface_and_defaults():
    from vsearch_amd import _lib
    lib = _lib.load()
    for name in _lib.EESTATS_SYMBOLS:
        assert hasattr(lib, name), name
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "vsx_eestats.h")).read()
    declared = set(re.findall(r"\b(vsx_fastq_eestats[a-z0-9_]*)\s*\(", hdr))
    assert declared == set(_lib.EESTATS_SYMBOLS), declared ^ set(_lib.EESTATS_SYMBOLS)
    o = _lib.EEStatsOpts()
    lib.vsx_fastq_eestats_opts_default(C.byref(o))
    # src/vsearch.h
    assert (o.ascii, o.qmin, o.qmax) == (33, 0, 41)
    assert (o.len_shortest, o.len_longest, o.len_increment) == (50, 2 ** 31 - 1, 50)
    assert [o.ee_cutoffs[k] for k in range(o.n_ee_cutoffs)] == [0.5, 1.0, 2.0]
    assert o.want == 3 and o.window == 0 and o.hist_budget == 0
    assert int(re.search(r"VSX_EESTATS_HIST_BUDGET_BYTES \(\(uint64_t\) (\d+) << 30\)", hdr).group(1)) == 4


# what the reference's check_parameters, args_get_length_cutoffs and args_get_ee_cutoffs refuse
REFUSED = [{"ascii": 32}, {"ascii": 65}, {"qmin": 10, "qmax": 9}, {"qmin": -1}, {"ascii": 64, "qmin": -32}, {"qmax": 94},
           {"ascii": 64, "qmax": 63}, {"length_cutoffs": [0, None, 50]}, {"length_cutoffs": [50, 49, 50]}, {"length_cutoffs": [50, None, 0]},
           {"length_cutoffs": [50, None, -1]}, {"ee_cutoffs": [0.5, 0.0]}, {"ee_cutoffs": [-1.0]}, {"ee_cutoffs": [1.0, float("nan")]},
           {"ee_cutoffs": []}, {"window": -1}]
ACCEPTED = [{"ascii": 64, "qmin": -31, "qmax": 62}, {"qmax": 93}, {"length_cutoffs": [1, 1, 1]}, {"length_cutoffs": [50, 50, 7]},
            {"ee_cutoffs": [1e-300]}, {"qmin": 41, "qmax": 41}]


@pytest.mark.parametrize("opts", REFUSED, ids=[str(o) for o in REFUSED])
def test_refused_options(host_stats, opts):
    from vsearch_amd import VsxError
    with pytest.raises(VsxError) as ei:
        host_stats(ed._set("one", opts, ["IIII"]))
    assert ei.value.code == -1          # VSX_EINVAL


@pytest.mark.parametrize("opts", ACCEPTED, ids=[str(o) for o in ACCEPTED])
def test_accepted_options(host_stats, opts):
    s = ed._set("one", opts, ["JJJJ" if opts.get("ascii") != 64 else "hhhh"])
    ed.assert_equals_py(host_stats(s), s)


def test_no_context_is_an_error_outside_host_mode(monkeypatch):
    from vsearch_amd import VsxError
    from vsearch_amd.eestats import read_stats
    monkeypatch.delenv("VSX_EESTATS", raising=False)
    with pytest.raises(VsxError) as ei:
        read_stats(None, ["IIII"])
    assert ei.value.code == -1


def test_reads_beyond_the_blob(monkeypatch):
    from vsearch_amd import VsxError
    from vsearch_amd.eestats import stats_of_blob
    monkeypatch.setenv("VSX_EESTATS", "host")
    blob = b"IIIIIIII"
    for off, ln, ok in ((0, 8, True), (8, 0, True), (4, 4, True), (1, 8, False), (9, 0, False), (2 ** 63, 2, False), (0, 2 ** 31, False),
                        (2 ** 64 - 1, 2, False)):
        if ok:
            assert stats_of_blob(None, blob, [0, off], [4, ln]).n == 2
        else:
            with pytest.raises(VsxError) as ei:
                stats_of_blob(None, blob, [0, off], [4, ln])
            assert ei.value.code == -1, (off, ln)


def test_want_selects_the_tables(host_stats):
    s = ed.generate(3, 30, read_len=60)
    both = host_stats(s)
    one, two = host_stats(s, want="eestats"), host_stats(s, want="eestats2")
    assert one.cutoff_counts is None and two.reads_at is None and two.sum_ee is None
    assert one.eestats_lines() == both.eestats_lines() and two.eestats2_lines() == both.eestats2_lines()
    with pytest.raises(ValueError):
        one.eestats2_lines()
    with pytest.raises(ValueError):
        two.eestats_lines()


def test_golden_host_path(host_stats, golden):
    sets = ed.golden_sets()
    assert [d["input"]["name"] for d in golden["sets"]] == [s["name"] for s in sets]
    for d, s in zip(golden["sets"], sets):
        assert d["input"] == s, s["name"]                    # the generators still give what was recorded
        res = host_stats(s)
        for command in s["commands"]:
            assert lines_of(res, command) == d["expected"][command], (s["name"], command)
        ed.assert_equals_py(res, s)
    assert os.path.getsize(GOLDEN) < 250000


def test_edge_reads_hold_what_they_promise(golden):
    sets = {s["name"]: s for s in ed.edge_reads()}
    expected = {d["input"]["name"]: d["expected"] for d in golden["sets"]}
    lengths = lambda name: [len(q) for q in sets[name]["quals"]]      # noqa: E731
    assert set(ed.EDGE_LENGTHS) <= set(lengths("lengths"))
    # the kernels' tiles: more reads than a workgroup of the walk / a step of the sum, every length at a tile's edge
    tiles = lengths("tiles")
    assert len(tiles) > ed.WALK_READS and set(ed.TILE_LENGTHS) <= set(tiles)
    for tile in (ed.WALK_POSITIONS, ed.SUM_POSITIONS):
        assert {tile - 1, tile, tile + 1} <= set(tiles) | set(lengths("lengths"))
    assert all(tiles[k] == ed.WALK_POSITIONS + 1 for k in (0, ed.WALK_READS - 1, ed.WALK_READS, len(tiles) - 1))
    # quartiles: positions reached by 5, 4, 3, 2, 1 reads, the running count exactly on each share of the reads
    py = ed.py_eestats(sets["quartiles"]["quals"])
    assert py["reads_at"] == [5, 4, 3, 2, 1]
    exact = set()
    for i, reads in enumerate(py["reads_at"]):
        n = 0
        for _, x in sorted(py["hist"][i].items()):
            n += x
            exact |= {share for share in (0.25, 0.50, 0.75) if n == share * reads}
    assert exact == {0.25, 0.50, 0.75}
    # q = 0 everywhere: the last bin of every row, and cutoffs equal to the running sum count
    py = ed.py_eestats(sets["all_q0"]["quals"])
    assert all(list(py["hist"][i]) == [1000 * (i + 1)] for i in range(65)) and py["sum_ee"][:3] == [5.0, 8.0, 9.0]
    py2 = ed.py_eestats2(sets["all_q0"]["quals"], sets["all_q0"]["opts"])
    assert py2["cutoff_counts"][0] == [0, 5, 5] and py2["cutoff_counts"][1] == [0, 0, 4] and py2["cutoff_counts"][2] == [0, 0, 0]
    assert expected["all_q0"]["eestats2"][4].split() == ["1", "0(", "0.0%)", "5(", "83.3%)", "5(", "83.3%)"]
    # the forms of the two lists
    rows = lambda name: [int(line.split()[0]) for line in expected[name]["eestats2"][4:]]      # noqa: E731
    assert rows("lc_1_star_1") == list(range(1, 130)) and rows("lc_60_120_7") == list(range(60, 121, 7))
    assert rows("lc_longest_below") == [10, 20, 30, 40] and max(lengths("lc_longest_below")) > 40
    assert rows("lc_shortest_above") == [500] and set(expected["lc_shortest_above"]["eestats2"][4].split()[1:]) == {"0(", "0.0%)"}
    assert expected["one_cutoff"]["eestats2"][2].count("MaxEE") == 1 and expected["eight_cutoffs"]["eestats2"][2].count("MaxEE") == 8
    assert sets["eight_cutoffs"]["opts"]["ee_cutoffs"] != sorted(sets["eight_cutoffs"]["opts"]["ee_cutoffs"])
    # offset 64 with symbols below it, and the widest quality range
    low = sets["ascii64_qmin-5"]
    assert low["opts"]["qmin"] == -5 and any(ord(c) < 64 for q in low["quals"] for c in q)
    assert any(ord(c) - 33 == 93 for q in sets["qmax93"]["quals"] for c in q)
    # the empty input and reads without a symbol
    assert expected["empty"]["eestats"] == [ed.HEADER] and expected["empty"]["eestats2"][:2] == ["0 reads", ""] and len(expected["empty"]["eestats2"]) == 4
    assert expected["only_empty_reads"]["eestats2"][0] == "2 reads, max len 0, avg 0.0"


def test_rounding_reads(host_stats, golden):
    """the bin and the eestats2 count at the recorded position follow the sum in position order, not a tree sum"""
    sets = ed.rounding_reads()
    assert len(sets) >= 8 and [d["input"] for d in golden["rounding"]] == sets
    for d, s in zip(golden["rounding"], sets):
        i, in_order, tree = s["position"], s["in_order"], s["tree"]
        assert int(1000 * in_order) != int(1000 * tree) and s["opts"]["ee_cutoffs"] == [min(in_order, tree)]
        assert not any(in_order <= c < tree or tree <= c < in_order for c in ed.DEFAULTS["ee_cutoffs"])
        res = host_stats(s)
        assert res.eestats2_lines() == d["expected"]["eestats2"], s["name"]
        assert res.cutoff_counts.tolist() == [[1 if in_order <= tree else 0]]
        assert res.ee_bins[i].tolist() == [min(1000 * (i + 1), int(1000 * in_order))] * 5
        assert res.sum_ee[i] == in_order
        ed.assert_equals_py(res, s)


def test_quality_cases(host_stats, golden):
    from vsearch_amd import VsxError
    cases = ed.quality_cases()
    assert [d["input"] for d in golden["quality"]] == [s for s, _ in cases]
    kinds = set()
    for d, (s, fatal) in zip(golden["quality"], cases):
        assert list(fatal) == d["fatal"], s["name"]              # as the reference did
        kinds.add(fatal[0])
        first = [k for k, q in enumerate(s["quals"]) if any(not s["opts"].get("qmin", 0) <= ord(c) - s["opts"].get("ascii", 33) <= s["opts"].get("qmax", 41) for c in q)]
        assert first[0] > 0 and len(first) > 1                   # not in the first read, and a later read has another one
        for py in (ed.py_eestats, ed.py_eestats2):
            with pytest.raises(ed.QualityError) as pe:
                py(s["quals"], s["opts"])
            assert (pe.value.kind, pe.value.value, pe.value.bound) == tuple(fatal)
        for want in ("both", "eestats", "eestats2"):
            with pytest.raises(VsxError, match=rf"FASTQ quality value \({fatal[1]}\) {fatal[0]} \({fatal[2]}\)") as ei:
                host_stats(s, want=want)
            assert ei.value.code == -1
    assert kinds == {"below qmin", "above qmax"}


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_host_equals_python_restatement(host_stats, seed):
    opts = [{}, {"length_cutoffs": [7, None, 13], "ee_cutoffs": ed.UNSORTED_CUTOFFS}, {"length_cutoffs": [20, 90, 1], "ee_cutoffs": [0.3]},
            {"qmax": 45, "length_cutoffs": [151, None, 50]}][seed - 1]
    s = ed.generate(seed, 120, read_len=(60, 151, 100)[seed % 3], opts=opts)
    ed.assert_equals_py(host_stats(s), s)


def test_window_and_offsets_do_not_matter(host_stats):
    s = ed.generate(77, 100, read_len=90)
    base = host_stats(s)
    for window in (1, 7):
        ed.assert_same_tables(host_stats(s, window=window), base)
    ed.assert_same_tables(ed.scattered_call(None, s, seed=5, window=7), base)


def test_read_order_shows_in_sum_ee(host_stats):
    s = ed.generate(78, 200, read_len=80)
    forward, backward = host_stats(s), host_stats(dict(s, quals=s["quals"][::-1]))
    assert (forward.sum_ee.view(np.uint64) != backward.sum_ee.view(np.uint64)).any()
    for f in ("reads_at", "qual_counts", "ee_bins", "cutoff_counts"):
        assert getattr(forward, f).tolist() == getattr(backward, f).tolist()


@needs_cli
def test_live_reference(host_stats):
    """the reference binary asked again: fresh seeded sets under default and non-default options, and every edge set"""
    fresh = [ed.generate(900, 300, read_len=120), ed.generate(901, 300, read_len=151, opts={"length_cutoffs": [30, 140, 11], "ee_cutoffs": [0.1, 5.0, 1.0]})]
    for s in fresh + ed.edge_reads():
        ref = ed.run_reference(s)
        assert ref["returncode"] == 0, ref["stderr"]
        res = host_stats(s)
        assert res.eestats_lines() == ref["eestats"] and res.eestats2_lines() == ref["eestats2"], s["name"]
