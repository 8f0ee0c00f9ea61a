"""CPU (-m "not gpu"), needs oracle/_ref/vsearch_ref: the reference CLI's own --tabbedout / --chimeras / --nonchimeras on the named
edge inputs of tests/chimeras_long_data.py.  Every input must provoke what it is named after, and the stored golden lines must be
what the CLI writes today."""
import json

import pytest

from oracle import refcli
from tests import chimeras_long_data as data

pytestmark = pytest.mark.skipif(not refcli.available(), reason="oracle/_ref/vsearch_ref not built")
Q = "q;size=1"


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("chimeras_long_ref"))
    return {name: data.ref_outputs(tmp, c["labels"], c["seqs"], c["cli"]) for name, c in data.edge_cases().items()}


def _line(out, label):
    hit = [ln.split("\t") for ln in out["tabbedout"] if ln.split("\t")[1] == label]
    assert len(hit) == 1, (label, out["tabbedout"])
    return hit[0]


def test_every_case_as_named(ref):
    for name, c in data.edge_cases().items():
        out, exp = ref[name], c["expect"]
        assert sorted(out["chimeras"] + out["nonchimeras"]) == sorted(c["labels"]), name
        assert [ln.split("\t")[1] for ln in out["tabbedout"]] == out["chimeras"], name        # a line per chimera, none otherwise
        for lb in exp.get("chimeric", []):
            assert lb in out["chimeras"], (name, lb)
        for lb in exp.get("clean", []):
            assert lb in out["nonchimeras"], (name, lb)
        for lb, parents in exp.get("parents", {}).items():
            assert _line(out, lb)[2:5] == parents, name


def test_line_format(ref):
    f = _line(ref["parents2_max3"], Q)
    assert f[0] == "99.9999" and f[4] == "*" and f[5] == "100.00" and f[8] == "0.00"
    assert f[10:] == ["0", "0", "0", "0", "0", "0", "0.00", "Y"] and len(f) == 18
    f = _line(ref["parents3_max3"], Q)
    assert f[4] == "v02;size=10" and f[9] == max(f[6:9], key=float)


def test_same_parent_twice(ref):
    f = _line(ref["one_parent_twice"], Q)
    assert f[2] == f[3] == "a;size=10" and f[4] == "*"
    # 299 query positions + the one insertion column; the parent's symbol in it is the only unequal column
    assert f[6] == f[7] == "%.2f" % (100.0 * 299 / 300)
    assert Q in ref["one_parent_uncovered"]["nonchimeras"]


def test_uncovered_position_is_not_chimeric(ref):
    for name in ("uncovered", "tie_within_uncovered"):
        assert ref[name]["chimeras"] == [] and Q in ref[name]["nonchimeras"]


def test_length_min_boundary(ref):
    assert ref["region9"]["chimeras"] == [] and ref["region10"]["chimeras"] == [Q] and ref["region11"]["chimeras"] == [Q]


def test_parents_max(ref):
    for m in (2, 3, 4, 20):
        for pmax in (2, 3, 20):
            assert (ref[f"parents{m}_max{pmax}"]["chimeras"] == [Q]) == (m <= pmax), (m, pmax)


def test_diff_pct_tolerates_a_mismatch(ref):
    """one input, four percentages: the mismatch at position 50 is fatal at 0 and 0.1 and tolerated at 1 and 2.5, where the second
    variant is still needed behind the breakpoint"""
    for pct in (0, 0.1):
        out = ref[f"diff_pct{pct}"]
        assert out["chimeras"] == [] and out["tabbedout"] == [] and Q in out["nonchimeras"], pct
    for pct in (1, 2.5):
        out = ref[f"diff_pct{pct}"]
        assert out["chimeras"] == [Q], pct
        f = _line(out, Q)
        assert f[2:5] == ["v00;size=10", "v01;size=10", "*"] and f[-1] == "Y", pct
    # the percentage decides where the first region ends, hence the two lines are the same here but for nothing else in common:
    # both parents differ from the query at the same 16 positions (15 substitutions in the other half + position 50 or the breakpoint)
    assert _line(ref["diff_pct1"], Q)[6:8] == _line(ref["diff_pct2.5"], Q)[6:8]


def test_insertion_columns_count(ref):
    # 299 positions + 1 insertion column in front of position 0 / after the last: the boundary and mid-segment substitutions
    # (2 per variant) and the inserted symbol are the unequal columns
    for name in ("insertion_front", "insertion_back"):
        f = _line(ref[name], Q)
        assert f[6] == f[7] == "%.2f" % (100.0 * 297 / 300), (name, f)


def test_ambiguity_selection_and_identity(ref):
    f = _line(ref["ambiguity"], Q)
    # N and R match in the selection (the query is covered); in the identities they are unequal columns: v00 N/A, R/A + 2, v01 N/A + 2
    assert f[6] == "%.2f" % (100.0 * 296 / 300) and f[7] == "%.2f" % (100.0 * 297 / 300)


def test_lengths_and_short_sequences(ref):
    out = ref["lengths"]
    assert len(out["chimeras"]) == 5
    for lb in ("one;size=3", "two;size=3", "one_again;size=1", "two_again;size=1"):
        assert lb in out["nonchimeras"]


def test_golden_is_current(ref, tmp_path):
    gold = json.load(open(data.GOLDEN))
    cases = data.edge_cases()
    assert sorted(gold["edges"]) == sorted(cases)
    for name, c in cases.items():
        g = gold["edges"][name]
        assert g["digest"] == data.case_digest(c["labels"], c["seqs"]), name
        assert {k: g[k] for k in ("tabbedout", "chimeras", "nonchimeras")} == ref[name], name
    labels, seqs = data.seeded_set()
    assert (gold["seeded"]["labels"], gold["seeded"]["seqs"]) == (labels, seqs)
    out = data.ref_outputs(str(tmp_path), labels, seqs)
    assert {k: gold["seeded"][k] for k in out} == out
    assert len(out["chimeras"]) >= 40
