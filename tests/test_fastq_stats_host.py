"""Read summary statistics without a device: the C-ABI surface of include/vsx_fastq_stats.h and the host restatements
(VSX_FASTQ_STATS=host) against the plain-Python restatements of tests/fastq_stats_data.py, table for table with sum_ee compared
by bit pattern, and against recorded texts of the reference CLI.

tests/golden/fastq_stats_golden.json was produced by `python -m tests.fastq_stats_data tests/golden/fastq_stats_golden.json`
(fastq_stats_data.write_golden): the sets of golden_sets() (edge_reads() and a seeded generate() set) and of order_reads() were
written as FASTQ and given to the reference's `--fastq_stats` / `--fastq_chars ... --log`; recorded are the comparable log lines
(after the `Started` line, up to but excluding the blank line in front of `Finished`) of the commands each set names, and for
quality_cases() the value and the range of the reference's fatal message.  Data and expected output only.

Where build() has left the reference binary in oracle/_ref, fresh sets are also given to it again.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import fastq_stats_data as fd

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fastq_stats_golden.json")
needs_cli = pytest.mark.skipif(not os.path.exists(fd.ref_binary()), reason="oracle/_ref/vsearch_ref not built")


@pytest.fixture()
def host(monkeypatch):
    monkeypatch.setenv("VSX_FASTQ_STATS", "host")

    def run(s, command, **extra):
        res = fd.call(None, s, command, **extra)
        assert res.stats["reads_host"] == res.stats["reads"] == len(s["quals"]) and res.stats["windows"] == 0
        return res
    return run


@pytest.fixture(scope="module")
def golden():
    return fd.load_golden(GOLDEN)


def test_abi_surface_and_defaults():
    from vsearch_amd import _lib
    import vsearch_amd
    lib = _lib.load()
    for name in _lib.FASTQ_STATS_SYMBOLS:
        assert hasattr(lib, name), name
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "vsx_fastq_stats.h")).read()
    declared = set(re.findall(r"\b(vsx_fastq_(?:stats|chars)[a-z0-9_]*)\s*\(", hdr))
    assert declared == set(_lib.FASTQ_STATS_SYMBOLS), declared ^ set(_lib.FASTQ_STATS_SYMBOLS)
    o = _lib.FastqStatsOpts()
    lib.vsx_fastq_stats_opts_default(C.byref(o))
    assert (o.ascii, o.qmin, o.qmax, o.window) == (33, 0, 41, 0)          # src/vsearch.h
    c = _lib.FastqCharsOpts()
    lib.vsx_fastq_chars_opts_default(C.byref(c))
    assert (c.tail, c.window) == (4, 0)
    assert int(re.search(r"VSX_FASTQ_STATS_SYMBOLS\s+(\d+)", hdr).group(1)) == 94
    # the ctypes mirrors have the sizes of the header's structs: 4 x 8, 4 x 8 + 5 pointers, 6 doubles + 3 counters, ...
    assert C.sizeof(_lib.FastqStatsOpts) == 32 and C.sizeof(_lib.FastqStatsOut) == 72 and C.sizeof(_lib.FastqStatsStats) == 72
    assert C.sizeof(_lib.FastqCharsOut) == 16 + 3 * 2048 + 1024 + 8 and C.sizeof(_lib.FastqCharsStats) == 64
    for name in ("fastq_stats", "fastq_chars", "FastqStatsResult", "FastqCharsResult"):
        assert hasattr(vsearch_amd, name) and name in vsearch_amd.__all__


# what the reference's check_parameters refuses
REFUSED = [{"ascii": 32}, {"ascii": 65}, {"qmin": 10, "qmax": 9}, {"qmin": -1}, {"ascii": 64, "qmin": -32}, {"qmax": 94},
           {"ascii": 64, "qmax": 63}, {"window": -1}]
ACCEPTED = [{"ascii": 64, "qmax": 62}, {"qmax": 93}, {"qmin": 41, "qmax": 41}, {"window": 3}]


@pytest.mark.parametrize("opts", REFUSED, ids=[str(o) for o in REFUSED])
def test_refused_options(host, opts):
    from vsearch_amd import VsxError
    with pytest.raises(VsxError) as ei:
        host(fd._set("one", ["IIII"], opts=opts), "stats")
    assert ei.value.code == -1          # VSX_EINVAL


@pytest.mark.parametrize("opts", ACCEPTED, ids=[str(o) for o in ACCEPTED])
def test_accepted_options(host, opts):
    window = opts.get("window", 0)
    s = fd._set("one", ["JJJJ" if opts.get("ascii") != 64 else "iiii"], opts={k: v for k, v in opts.items() if k != "window"})
    fd.assert_equals_py(host(s, "stats", window=window), s, "stats")


def test_refused_chars_options_and_arguments(host):
    from vsearch_amd import VsxError
    from vsearch_amd.fastq_stats import chars_of_blob
    s = fd._set("one", ["IIII"])
    for extra in ({"tail": 0}, {"tail": -3}, {"window": -1}):
        with pytest.raises(VsxError) as ei:
            host(s, "chars", **extra)
        assert ei.value.code == -1, extra
    assert host(s, "chars", tail=2 ** 40).tail_counts.sum() == 0
    for seq, qual in ((b"ACGT", None), (None, b"IIII")):
        with pytest.raises(VsxError) as ei:
            chars_of_blob(None, seq, qual, [0], [4])
        assert ei.value.code == -1


def test_no_context_is_an_error_outside_host_mode(monkeypatch):
    from vsearch_amd import VsxError, fastq_chars, fastq_stats
    monkeypatch.delenv("VSX_FASTQ_STATS", raising=False)
    for run in (lambda: fastq_stats(None, ["IIII"]), lambda: fastq_chars(None, ["ACGT"], ["IIII"])):
        with pytest.raises(VsxError) as ei:
            run()
        assert ei.value.code == -1


def test_reads_beyond_the_blob(monkeypatch):
    from vsearch_amd import VsxError
    from vsearch_amd.fastq_stats import chars_of_blob, stats_of_blob
    monkeypatch.setenv("VSX_FASTQ_STATS", "host")
    blob, seq = b"IIIIIIII", b"ACGTACGT"
    calls = (lambda off, ln: stats_of_blob(None, blob, [0, off], [4, ln]), lambda off, ln: chars_of_blob(None, seq, blob, [0, off], [4, ln]))
    for run in calls:
        for off, ln, ok in ((0, 8, True), (8, 0, True), (4, 4, True), (1, 8, False), (9, 0, False), (2 ** 63, 2, False), (0, 2 ** 31, False),
                            (2 ** 64 - 1, 2, False)):
            if ok:
                assert run(off, ln).n == 2
            else:
                with pytest.raises(VsxError) as ei:
                    run(off, ln)
                assert ei.value.code == -1, (off, ln)


@pytest.mark.parametrize("byte", [32, 127, 10, 200])
def test_quality_bytes_outside_33_126(host, byte):
    from vsearch_amd import VsxError
    from vsearch_amd.fastq_stats import chars_of_blob, stats_of_blob
    qual = b"IIII" + b"II" + bytes([byte]) + b"I"
    for run in (lambda: stats_of_blob(None, qual, [0, 4], [4, 4]), lambda: chars_of_blob(None, b"ACGTACGT", qual, [0, 4], [4, 4])):
        with pytest.raises(VsxError, match="outside 33 ... 126") as ei:
            run()
        assert ei.value.code == -1
    # bytes nobody reads may hold anything
    assert stats_of_blob(None, qual, [0, 7], [4, 1]).n == 2 and chars_of_blob(None, b"ACGTACGT", qual, [0, 7], [4, 1]).n == 2


def test_golden_host_path(host, golden):
    sets = fd.golden_sets()
    assert [d["input"]["name"] for d in golden["sets"]] == [s["name"] for s in sets]
    for d, s in zip(golden["sets"], sets):
        assert d["input"] == s, s["name"]                    # the generators still give what was recorded
        assert s["commands"] and set(s["commands"]) <= set(fd.BOTH)
        for command in s["commands"]:
            res = host(s, command)
            assert res.log_lines() == d["expected"][command], (s["name"], command)
            fd.assert_equals_py(res, s, command)
    assert os.path.getsize(GOLDEN) < 130000


def test_edge_reads_hold_what_they_promise(golden):
    sets = {s["name"]: s for s in fd.edge_reads()}
    expected = {d["input"]["name"]: d["expected"] for d in golden["sets"]}
    lengths = lambda name: [len(q) for q in sets[name]["quals"]]      # noqa: E731
    assert set(fd.EDGE_LENGTHS) == {0, 1, 2, 63, 64, 65, 127, 128, 129, 300} and set(fd.EDGE_LENGTHS) <= set(lengths("lengths"))
    # reads per call at the edges of a wave and a workgroup
    assert fd.EDGE_READ_COUNTS == (63, 64, 65, 255, 256, 257)
    for count in fd.EDGE_READ_COUNTS:
        ls = lengths(f"reads_{count}")
        assert len(ls) == count and max(ls) > 0
    # the longest read in the last lane of a wave only
    ls = lengths("last_lane")
    assert len(ls) == fd.WAVE and ls[-1] == 20 and max(ls[:-1]) <= 10
    # a lowest score that falls at position 64: the read counts for every Q threshold up to position 63 and for none from 64 on
    with_it, without = (fd.py_fastq_stats(q)["q_counts"] for q in (sets["lengths"]["quals"], sets["lengths"]["quals"][:-1]))
    assert sets["lengths"]["quals"][-1] == fd.Q_FALLS_AT_64 and fd.Q_FALLS_AT_64.index("&") == 64
    assert [[a - b for a, b in zip(with_it[i], without[i])] for i in (63, 64, 65)] == [[1, 1, 1, 1], [0, 0, 0, 0], [0, 0, 0, 0]]

    # the exact landings of the running expected error (plain Python doubles)
    pe = fd._pe
    assert pe(10) == 0.1 and sum([pe(10)] * 5, 0.0) == 0.5 and pe(0) == 1.0
    q20 = 0.0
    for k in range(25):
        q20 += pe(20)
        if k == 9:
            assert q20 == 0.09999999999999999
    assert q20 == 0.25000000000000006
    py = fd.py_fastq_stats(sets["ee_landings"]["quals"])
    assert fd.EE_LANDINGS == ("+II", "+++++", "!I", "5" * 25, "5" * 10)
    # position 0: Q10 counts for every threshold, Q0 for 1.0 only, the Q20 reads for all
    assert py["ee_counts"][0] == [5, 4, 4, 4]
    # position 4: Q10 x 5 is exactly 0.5: counted for 1.0 and 0.5; the two Q20 reads for all four
    assert py["ee_counts"][4] == [3, 3, 2, 2]
    # position 9: Q20 x 10 is 0.09999999999999999 <= 0.1, in both Q20 reads
    assert py["ee_counts"][9] == [2, 2, 2, 2]
    # position 24: Q20 x 25 is 0.25000000000000006: not <= 0.25 although the real sum is
    assert py["ee_counts"][24] == [1, 1, 0, 0] and py["ee_counts"][23] == [1, 1, 1, 0]
    assert expected["ee_landings"]["stats"] == py["lines"]

    # lowest scores exactly on and one above every threshold
    s = sets["q_edges"]
    py = fd.py_fastq_stats(s["quals"])
    assert [min(ord(c) - 33 for c in q) for q in s["quals"][:8]] == [5, 6, 10, 11, 15, 16, 20, 21]
    assert py["q_counts"][3] == [8, 8, 8, 8] and py["q_counts"][4] == [7, 5, 3, 1] and py["q_counts"][6] == py["q_counts"][4]

    # offset 64: ';' is printed with Q 0 and Pe 1.0
    low = sets["ascii64_low"]
    assert low["opts"] == {"ascii": 64} and any(";" in q for q in low["quals"])
    row = [line for line in expected["ascii64_low"]["stats"] if line.startswith("    ;")]
    assert len(row) == 1 and row[0].split()[:3] == [";", "0", "1.00000"]
    at = [line for line in expected["ascii64_low"]["stats"] if line.startswith("    @")]
    assert at[0].split()[:3] == ["@", "0", "1.00000"]
    assert any(ord(c) == 126 for q in sets["qmax93"]["quals"] for c in q)

    # the empty input prints the headers only; only empty reads: one row in section 1, no Avg-less closing
    empty = expected["empty"]
    assert empty["chars"] == ["Read 0 sequences."]
    assert [line for line in empty["stats"] if line and line[0].isdigit()] == [] and not any("Avg length" in line for line in empty["stats"])
    assert empty["stats"][-2:] == ["         0  Recs (0.0M), 0 too long", "      0.0M  Bases"]
    only = expected["only_empty_reads"]
    assert only["stats"][4] == ">=    0           3   100.0%   100.0%" and "       0.0  Avg length" in only["stats"]
    assert only["chars"][:2] == ["Read 3 sequences.", "Qmin 0, Qmax 0, Range 1"]

    # chars: runs of 1, 2, 64, 65 and a whole read (maxrun is the run minus one); a run across two reads must not continue
    runs = sets["runs"]
    py = fd.py_fastq_chars(runs["seqs"], runs["quals"])
    maxrun = {chr(c): py["maxrun"][c] for c in range(256) if py["seq_counts"][c]}
    assert maxrun["C"] == 1 and maxrun["G"] == 63 and maxrun["T"] == 64 and maxrun["W"] == 69
    assert runs["seqs"][2] == "KKKKK" and runs["seqs"][3] == "KKKKKKK" and maxrun["K"] == 7 - 1
    assert maxrun["Y"] == 0 and maxrun["R"] == 4 and maxrun["U"] == 1 and maxrun["A"] == 1      # lower case continues an upper-case run
    assert not any(chr(c).islower() for c in range(256) if py["seq_counts"][c]) and py["seq_counts"][ord("N")] == 0
    n_row = lambda name: [line for line in expected[name]["chars"] if line.startswith("     N")][0]      # noqa: E731
    assert n_row("n_one_q").endswith("  Q=#") and n_row("n_two_q").endswith("  Q=#..5")
    # tails under tail = 1, 4, the read length (5 and 8) and the read length + 1
    tails = {t: fd.py_fastq_chars(sets[f"tail_{t}"]["seqs"], sets[f"tail_{t}"]["quals"], t)["tail_counts"] for t in (1, 4, 5, 8, 9)}
    count = lambda t: (tails[t][ord("5")], tails[t][ord("I")], tails[t][ord("+")])      # noqa: E731
    assert count(1) == (4, 1, 1) and count(4) == (3, 0, 0) and count(5) == (1, 0, 0) and count(8) == (1, 0, 0) and count(9) == (0, 0, 0)
    quals = sets["tail_4"]["quals"]
    assert quals[0] == "IIII5555" and quals[0][len(quals[0]) - 5] != "5" and quals[1] == "I5555" and "" in quals
    # the five format guesses
    guesses = [[line for line in expected["format_" + name]["chars"] if line.startswith("Guess: ") and "format" in line][0][7:] for name in fd.FORMAT_RANGES]
    assert guesses == list(fd.FORMATS)


def test_order_reads(host, golden):
    """sum_ee follows the read order: the reversed input gives other bits at the recorded position"""
    sets = fd.order_reads()
    assert len(sets) >= 4 and [d["input"] for d in golden["order"]] == sets
    for d, s in zip(golden["order"], sets):
        r = dict(s, quals=s["quals"][::-1], seqs=s["seqs"][::-1])
        forward, backward = host(s, "stats"), host(r, "stats")
        i = s["position"]
        assert forward.sum_ee.view(np.uint64)[i] != backward.sum_ee.view(np.uint64)[i]
        assert (forward.sum_ee.view(np.uint64)[:i] == backward.sum_ee.view(np.uint64)[:i]).all()
        for f in ("length_counts", "symbol_counts", "ee_counts", "q_counts"):
            assert getattr(forward, f).tolist() == getattr(backward, f).tolist()
        assert forward.log_lines() == d["expected"]["stats"], s["name"]
        fd.assert_equals_py(forward, s, "stats")
        fd.assert_equals_py(backward, r, "stats")


def test_quality_cases(host, golden):
    from vsearch_amd import VsxError
    cases = fd.quality_cases()
    assert [d["input"] for d in golden["quality"]] == [s for s, _ in cases]
    recorded = {s["name"]: tuple(f) for s, f in cases}
    assert recorded["negative_qmin"] == (40, -5, 41) and recorded["above"] == (42, 0, 41) and recorded["below"] == (3, 5, 41)
    for d, (s, fatal) in zip(golden["quality"], cases):
        assert list(fatal) == d["fatal"], s["name"]              # as the reference did
        o = dict(fd.DEFAULTS, **s["opts"])
        refused = [k for k, q in enumerate(s["quals"]) if q and not all(
            o["qmin"] % fd.U32 <= fd._score(ord(c), o["ascii"]) <= o["qmax"] % fd.U32 for c in (min(q), max(q)))]
        assert refused[0] > 0 and len(refused) > 1               # not the first read, and a later read is refused too
        with pytest.raises(fd.RangeError) as pe:
            fd.py_fastq_stats(s["quals"], s["opts"])
        assert (pe.value.value, pe.value.qmin, pe.value.qmax) == tuple(fatal)
        for window in (0, 1):
            with pytest.raises(VsxError, match=rf"FASTQ quality value \({fatal[0]}\) out of range \({fatal[1]}-{fatal[2]}\)") as ei:
                host(s, "stats", window=window)
            assert ei.value.code == -1


def test_non_letters_count_as_n(host):
    seqs, quals = ["AC-G*1nN.", "@[`{zZ"], ["IIIIIIIII", "555555"]
    s = fd._set("non_letters", quals, seqs)
    res = host(s, "chars")
    py = fd.assert_equals_py(res, s, "chars")
    assert py["seq_counts"][ord("N")] == 10 and py["seq_counts"][ord("Z")] == 2 and py["maxrun"][ord("N")] == 4      # "*1nN.": five in a row
    assert (res.qmin_n, res.qmax_n) == (ord("5"), ord("I"))


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_host_equals_python_restatement(host, seed):
    opts = [{}, {"qmax": 45}, {"qmin": 0, "qmax": 41}, {}][seed - 1]
    s = fd.generate(seed, 120, read_len=(60, 151, 100)[seed % 3], opts=opts, tail=seed)
    for command in fd.BOTH:
        fd.assert_equals_py(host(s, command), s, command)


def test_window_and_offsets_do_not_matter(host):
    s = fd.generate(77, 100, read_len=90)
    for command in fd.BOTH:
        base = host(s, command)
        for window in (1, 7):
            fd.assert_same_tables(host(s, command, window=window), base)
        fd.assert_same_tables(fd.scattered_call(None, s, command, seed=5, window=7), base)


@needs_cli
def test_live_reference(host):
    """the reference binary asked again: fresh seeded sets under default and non-default options, and every edge set"""
    fresh = [fd.generate(900, 300, read_len=120), fd.generate(901, 300, read_len=151, opts={"qmax": 45}, tail=2)]
    for s in fresh + fd.edge_reads():
        ref = fd.run_reference(s, s["commands"])
        assert ref["returncode"] == 0, ref["stderr"]
        for command in s["commands"]:
            assert host(s, command).log_lines() == ref[command], (s["name"], command)
    for s, fatal in fd.quality_cases():
        assert fd.run_reference(s, ["stats"])["fatal"] == tuple(fatal), s["name"]
