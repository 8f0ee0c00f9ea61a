"""No device: the inputs of tests/marshal_data.py reach the edges they are named after.  Everything is asserted from the scalar
oracle's CIGARs (oracle.pyoracle.Oracle), so tests/test_gpu_marshal.py cannot pass by missing an edge: the digit counts and exact
run lengths, the string lengths mod 4, the zero-run pairs between pairs with many, the host-answered pairs, and the run words and
text bytes that overflow a plan's buffers at their natural size."""
import numpy as np
import pytest

from tests import marshal_data as md


@pytest.fixture(scope="module")
def rows(oracle):
    return {c["name"]: md.oracle_rows(c, oracle) for c in md.digit_edges() + md.wave_edges() + (md.dense_runs(),)}


def test_digit_edges_reach_every_digit_count_and_run_length(rows):
    squares, overhangs = md.digit_edges()
    assert [r[5] for r in rows["squares"]] == ["M"] + [f"{n}M" for n in md.SQUARES[1:]]
    assert [r[5] for r in rows["overhangs"]] == ["9999I8M10000I", "10000I8M9999I", "10000I8M", "32767I8M3I", "3I8M32768I", "65519I8M"]
    assert (len("10000I8M") + 1) % 4 == 1          # a fifth digit counted as four would change this string's padded length
    lengths = {n for name in ("squares", "overhangs") for r in rows[name] for n, _ in md.runs_of(r[5])}
    assert {len(str(n)) for n in lengths if n > 1} == {1, 2, 3, 4, 5} and 1 in lengths
    assert lengths >= {9, 10, 99, 100, 999, 1000, 9999, 10000, 32767, 32768}
    assert {(len(r[5]) + 1) % 4 for r in rows["squares"]} == {0, 1, 2, 3}
    # the size guard (Q + D <= 65535, Q D <= 25e6) admits these and nothing longer
    assert max(len(q) * len(q) for q in squares["queries"]) == 25000000
    assert max(len(md.CORE) + len(t) for t in overhangs["targets"]) == 65535
    assert all(r[0] != 32767 for name in ("squares", "overhangs") for r in rows[name])


def test_wave_edges_mix_empty_and_long_strings_around_the_wave_sizes(rows):
    assert tuple(len(c["qidx"]) - len(c["host"]) for c in md.wave_edges()) == md.WAVE_COUNTS == (1, 63, 64, 65, 255, 256, 257)
    for c in md.wave_edges():
        r = rows[c["name"]]
        n = len(r)
        flt, verdicts = md.filtered_rows(c, r)
        # the host answers exactly the three special pairs; their strings follow the device text
        assert c["host"] == [0, (n - 3) // 2 + 1, n - 1]
        assert [r[k] for k in c["host"]] == [(-8, 7, 0, 0, 7, "7I"), md.SENTINEL_ROW, md.SENTINEL_ROW]
        # one device pair overflows int16 (from 63 pairs on): a sentinel row the DEVICE produces, undecided in a ranked call
        assert c["refused"] == ([] if n < 10 else [10]) and all(r[k] == md.SENTINEL_ROW and verdicts[k] == 0 for k in c["refused"])
        assert all(r[k][0] != 32767 for k in range(n) if k not in c["host"] + c["refused"])
        # every fifth device pair is rejected by the filter (no runs, empty string); the pairs before and after it have runs
        assert all(verdicts[k] == 3 and flt[k][5] == "" and len(md.runs_of(r[k][5])) >= 10 for k in c["unrelated"]), c["name"]
        kept = [k for k in range(n) if verdicts[k] == 1]
        assert len(kept) >= (n - 3) // 2 and set(verdicts) <= {0, 1, 3}
        if n > 10:
            assert len(c["unrelated"]) == (n - 3) // 5 - 1
            assert any(verdicts[k - 1] == 1 and verdicts[k + 1] == 1 for k in c["unrelated"] if k + 1 < n)
            # string lengths vary inside a wave, over every residue mod 4
            assert {(len(x[5]) + 1) % 4 for x in flt} == {0, 1, 2, 3}
            assert len({len(x[5]) for x in flt}) >= 8
        else:
            dev = [k for k in range(n) if k not in c["host"]]
            assert len(dev) == 1 and verdicts[dev[0]] == 1 and len(md.runs_of(r[dev[0]][5])) >= 1


def test_ranked_filter_keeps_some_but_fewer_than_half_of_the_largest_wave_case(rows):
    c = md.wave_case(257)
    _, verdicts = md.filtered_rows(c, rows["wave257"], md.full_filter(**md.RANKED_FILTER))
    kept = verdicts.count(1)
    assert 20 <= kept and 2 * kept <= len(verdicts) and set(verdicts) == {0, 1, 3}, kept


def test_pipeline_caps_split_the_slices_into_overflowing_and_fitting_ones(oracle):
    """PIPE_PAIRS mixed pairs in slices of PIPE_SLICE: the quarter slices stay below PIPE_RUNS_CAP words and PIPE_TEXT_CAP bytes, the
    full ones exceed both"""
    c = md.dense_mixed(md.PIPE_PAIRS)
    r = md.oracle_rows(c, oracle)
    assert [r[k][5] for k in c["host"][:2]] == ["7I", ""] and len(c["host"]) == 43
    assert all(c["qidx"][k] != c["qidx"][k + 1] for k in range(md.PIPE_PAIRS - 1))
    cuts = md.pipeline_cuts(md.PIPE_PAIRS, md.PIPE_SLICE)
    assert cuts == [0, 175, 525, 1155, 1785, 2415, 3045, 3675, 4025, 4200]
    over_runs, over_text = md.slice_overflows(c, r, cuts, md.PIPE_RUNS_CAP, md.PIPE_TEXT_CAP)
    assert over_runs == over_text == [False] + [True] * 7 + [False]


def test_dense_runs_overflow_both_buffers_at_their_natural_size(rows):
    c, r = md.dense_runs(), rows["dense"]
    nruns = np.array([len(md.runs_of(x[5])) for x in r])
    nbytes = np.array([md.padded(x[5]) for x in r])
    assert len(r) == 24 and len({(c["queries"][k], c["targets"][k]) for k in range(24)}) == 24
    assert nruns.min() >= 129 and min(len(x[5]) + 1 for x in r) >= 200, (nruns.min(), nbytes.min())
    # one plan of NATURAL_PAIRS pairs over these 24: the first buffers are max(16 Mi words, 48 per pair) + 1 and
    # max(32 MiB, 128 B per pair) + 16 (the worst-case bounds are far above both)
    idx = md.dense_index(md.NATURAL_PAIRS)
    assert max(16 << 20, 48 * md.NATURAL_PAIRS) + 1 == md.RUNS_CAP_NATURAL and max(32 << 20, 128 * md.NATURAL_PAIRS) + 16 == md.TEXT_CAP_NATURAL
    assert int(nruns[idx].sum()) > md.RUNS_CAP_NATURAL and int(nbytes[idx].sum()) > md.TEXT_CAP_NATURAL
    worst = sum(len(c["queries"][k]) + len(c["targets"][k]) + 1 for k in idx.tolist())
    assert worst > md.RUNS_CAP_NATURAL and 6 * worst > md.TEXT_CAP_NATURAL
