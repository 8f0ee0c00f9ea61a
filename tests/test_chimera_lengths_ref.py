"""No device: what the inputs of tests/test_gpu_chimera_lengths.py (tests/chimera_length_data.py) must provoke, asserted on the
reference CLI's own --uchimeout lines.  Skipped where oracle/_ref/vsearch_ref is not built."""
import pytest

from oracle import refcli
from tests import chimera_length_data as cd

pytestmark = pytest.mark.skipif(not refcli.available(), reason="oracle/_ref/vsearch_ref not built")


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    return cd.reference_lines(str(tmp_path_factory.mktemp("reference")))


def _length(name):
    return int(name.split("_")[0][1:])


def test_all_lengths_provoke_what_they_should(reference):
    """for every L >= 255 some query is flagged Y, some N, and all five chimeras are scored; every length from 42 up has a scored
    query; no pair is large enough for the sentinel route"""
    tn, db, qn, qs = cd.all_lengths()
    assert sorted({_length(n) for n in qn}) == sorted(cd.KERNEL_LENGTHS + cd.EXTRA_LENGTHS + cd.HOST_LENGTHS)
    assert all(len(q) == _length(n) for n, q in zip(qn, qs))
    assert max(len(q) for q in qs) * max(len(t) for t in db) < 25_000_000
    for mode in cd.MASKS:
        flags, scored = {}, {}
        for n, line in zip(qn, reference[mode]):
            f = line.split("\t")
            flags.setdefault(_length(n), set()).add(f[-1])
            scored[_length(n)] = scored.get(_length(n), 0) + (f[2] != "*")
        for L, fl in flags.items():
            if L >= 255:
                assert {"Y", "N"} <= fl, (L, fl)
                assert scored[L] >= 5, (L, scored[L])
            if L >= 42:
                assert scored[L] >= 1, (L, scored[L])


def test_short_lengths_are_scored(reference):
    """L = 33 .. 41: the reference scores every query, with its own two parents, and flags some Y and some N"""
    tn, db, qn, qs = cd.short_lengths()
    assert sorted({_length(n) for n in qn}) == list(range(33, 42))
    assert all(len(q) == _length(n) for n, q in zip(qn, qs)) and all(len(t) == _length(n) for n, t in zip(tn, db))
    for mode in cd.MASKS:
        flags = set()
        for n, line in zip(qn, reference["short_" + mode]):
            f = line.split("\t")
            assert {f[2], f[3]} == {n + "_a", n + "_b"}, line
            flags.add(f[-1])
        assert {"Y", "N"} <= flags


def test_denovo_set_and_candidate_sets(reference, tmp_path):
    from tests.test_gpu_chimera import _ref_lines
    for v in cd.VARIANTS:
        assert sum(line.endswith("\tY") for line in reference[v]) >= 2 * len(cd.DENOVO_LENGTHS)
    for L in (512, 1500):
        for build in (cd.sixteen_candidates, cd.two_relatives):
            tn, db, q = build(L)
            assert _ref_lines(str(tmp_path), ["q"], [q], tn, db)[0].endswith("\tY")
