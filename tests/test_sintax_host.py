"""SINTAX without a GPU: the library's host restatement (vsx_internal_sintax_host) against the plain-Python restatement field for
field on every set, the formatters against the recorded lines of the reference CLI (tests/golden/sintax_golden.json), the
refusals, the interning of the rank names -- and, from py_sintax() alone, that every set reaches the case it was built for.
"""
import numpy as np
import pytest

from tests import sintax_data as sd


@pytest.fixture(scope="module")
def golden():
    return {s["name"]: s for s in sd.load_golden()}


_PY = {}


def py_records(s):
    if s["name"] not in _PY:
        _PY[s["name"]] = sd.py_sintax(s, rounds=True)
    return _PY[s["name"]]


def host_result(s, **extra):
    from vsearch_amd import sintax_host
    o = sd.full_opts(s["opts"])
    kw = dict(strand_both=o["strand_both"], sintax_random=o["random"], want_candidates=True, wordlength=o["wordlength"],
              soft_mask=sd.MASK_MODES[o["dbmask"]], hardmask=1 if o["hardmask"] else 0)
    kw.update(extra)
    return sintax_host(s["db"], s["db_labels"], s["queries"], o["seed"], **kw)


def comparable(rec):
    return {k: v for k, v in rec.items() if k != "round_counts"}


def all_sets(golden):
    return list(golden.values()) + sd.hardmask_sets()


def test_golden_inputs_are_the_builders(golden):
    built = {s["name"]: s for s in sd.golden_sets()}
    assert set(built) == set(golden)
    for name, s in built.items():
        assert all(golden[name][k] == s[k] for k in sd.INPUT_KEYS), name
        assert set(golden[name]) == set(sd.INPUT_KEYS) | {"ref"} and set(golden[name]["ref"]) == {"tabbed", "log"}


def test_python_restatement_equals_reference_text(golden):
    for s in golden.values():
        recs = py_records(s)
        assert sd.py_tabbed(s, recs) == s["ref"]["tabbed"], s["name"]
        assert sd.py_log(recs) == s["ref"]["log"], s["name"]


def test_host_equals_python_field_for_field(golden):
    for s in all_sets(golden):
        res, recs = host_result(s), py_records(s)
        assert res.n == len(recs)
        for q, want in enumerate(recs):
            assert res.record(q) == comparable(want), (s["name"], q)
        assert res.n_classified == sum(r["classified"] for r in recs)


def test_formatters_equal_golden_text(golden):
    from vsearch_amd import tabbed_lines, log_lines
    for s in golden.values():
        res = host_result(s)
        assert tabbed_lines(res, s["qlabels"], s["db_labels"], sd.full_opts(s["opts"])["cutoff"]) == s["ref"]["tabbed"], s["name"]
        assert log_lines(res) == s["ref"]["log"], s["name"]


def test_host_routes_are_counted(golden):
    assert host_result(golden["sintax_random"]).stats["queries_host_random"] == len(golden["sintax_random"]["queries"])
    assert host_result(golden["wordlength_12"]).stats["queries_host_wordlength"] == len(golden["wordlength_12"]["queries"])
    st = host_result(golden["ties"]).stats
    assert st["queries_host_forced"] == len(golden["ties"]["queries"]) and st["queries_device"] == 0


def test_query_numbers_and_windows(golden):
    """a query's result depends on its number and the seed, not on the call it is in"""
    s = golden["candidates"]
    whole = host_result(s)
    part = host_result(dict(s, queries=s["queries"][5:12]), first_query_no=5)
    rev = host_result(dict(s, queries=s["queries"][::-1]), query_numbers=list(range(len(s["queries"])))[::-1])
    for q in range(5, 12):
        assert part.record(q - 5) == whole.record(q)
    for q in range(len(s["queries"])):
        assert rev.record(len(s["queries"]) - 1 - q) == whole.record(q)
    # the same read under other numbers, and under another seed: different streams
    assert len({tuple(whole.boot_count[q]) for q in range(whole.n)}) > 5
    other = host_result(dict(s, opts=dict(s["opts"], seed=20)))
    assert not np.array_equal(other.boot_count, whole.boot_count)
    recs = sd.py_sintax(dict(s, opts=dict(s["opts"], seed=20)))
    assert all(other.record(q) == r for q, r in enumerate(recs))


def test_refusals(golden):
    from vsearch_amd import sintax_host, VsxError
    s = golden["ties"]
    with pytest.raises(VsxError, match="randseed 0"):
        sintax_host(s["db"], s["db_labels"], s["queries"], 0)
    with pytest.raises(VsxError, match="no labels"):
        sintax_host(s["db"], None, s["queries"], 5)


def test_interning():
    """equal ids at a rank <=> equal (length, bytes); id 0 is the empty name; the names are tax_split's"""
    from vsearch_amd.sintax import intern_labels
    labels = sd.LABEL_QUIRKS + sd.taxonomy_db(__import__("random").Random(3))[1] + ["a;tax=g:Gen;", "b;tax=g:Gen ;", "c;tax=g:gen;", "d;tax=g:Gen;"]
    ids, start, ln = intern_labels(labels)
    names = [sd.tax_split(h) for h in labels]
    for i, h in enumerate(labels):
        for k in range(9):
            assert h[start[i, k]:start[i, k] + ln[i, k]] == names[i][k], (h, k)
            assert (ids[i, k] == 0) == (names[i][k] == "")
    for k in range(9):
        for i in range(len(labels)):
            for j in range(i):
                assert (ids[i, k] == ids[j, k]) == (names[i][k] == names[j][k]), (labels[i], labels[j], k)


def test_label_quirks_are_what_the_set_is_for():
    n = {h: sd.tax_split(h) for h in sd.LABEL_QUIRKS}
    q = sd.LABEL_QUIRKS
    assert n[q[0]] == [""] * 9 and n[q[1]] == [""] * 9                        # no tax=, xtax=
    assert n[q[2]][0] == "First" and n[q[2]][6] == "Gfirst"                    # tax= first in the header
    assert n[q[3]][6] == "Glast"                                               # last, no semicolon
    assert n[q[4]][:3] == ["Upper", "Kup", "Pup"]                              # upper-case rank letters
    assert n[q[5]][2] == "Phy" and n[q[5]][6] == "Gen"                         # unknown letters skipped
    assert n[q[6]][2] == "Late"                                                # a later duplicate overwrites
    assert n[q[7]][5] == "" and n[q[7]][7] == "Sp5"                            # missing middle ranks
    assert n[q[8]][6] == "Spill;note=a"                                        # the comma search passes the end of the field
    assert n[q[9]][6] == "Gen 7" and n[q[9]][7] == "Homo sapiens"              # spaces
    assert n[q[11]][0] == "Second"                                             # xtax= first, then a real tax=


# ---- every set reaches its case (from the Python restatement, not from the code under test) -----------------------------------------
def test_cases_word_counts(golden):
    s = golden["basic_both"]
    k = [len(sd.words_of(q, 8, False)) for q in s["queries"]]
    assert k[:4] == [31, 32, 33, 0] and 0 < k[4] < 32 and 32 <= k[12] < 180 - 7 - 7   # K around 32, short, N's
    r = py_records(s)
    assert r[0]["boot_count"] == [0, 0] and r[0]["round_counts"] == [[], []]         # K = 31: skipped, no draws
    assert len(r[1]["round_counts"][0]) == 100 and len(r[2]["round_counts"][0]) == 100
    assert s["queries"][5].islower() and r[5]["classified"]                         # lower case still classifies
    assert k[6] == 32 and r[6]["classified"] and max(r[6]["round_counts"][0]) < 32  # 32 draws from 32 words repeat
    assert {x["strand"] for x in r if x["classified"]} == {0, 1}
    assert not all(x["classified"] for x in r)
    plus = py_records(golden["basic_plus"])
    assert r[8]["classified"] and r[8]["strand"] == 1 and not plus[8]["classified"]  # a reverse-complemented read under --strand plus


def test_cases_candidate_counts(golden):
    r = py_records(golden["candidates"])
    assert {49, 50, 51} <= {x["boot_count"][0] for x in r}
    assert any(x["boot_count"][0] == 49 and not x["classified"] for x in r) and any(x["boot_count"][0] == 50 and x["classified"] for x in r)
    counts = {c for x in r for c in x["round_counts"][0]}
    assert {1, 2} <= counts
    # two names tied at a rank: the first in candidate order wins
    tied = 0
    for x in r:
        if x["classified"]:
            n, c = x["boot_count"][0], x["candidates"][0]
            for level, (seq, votes) in enumerate(x["ranks"]):
                if 2 * votes == n and level == 1:
                    assert sd.tax_split(golden["candidates"]["db_labels"][c[0]])[1] == sd.tax_split(golden["candidates"]["db_labels"][seq])[1]
                    tied += 1
    assert tied >= 1
    # a printed score that was rounded up, against a cutoff equal to the printed value
    s = golden["candidates"]
    cutoff = s["opts"]["cutoff"]
    hit = 0
    for x, line in zip(py_records(s), s["ref"]["tabbed"]):
        if x["classified"]:
            for level, (seq, votes) in enumerate(x["ranks"]):
                score = votes / x["boot_count"][0]
                if "%.2f" % score == "%.2f" % cutoff and score < cutoff:
                    name = sd.tax_split(s["db_labels"][seq])[level]
                    assert f"{sd.RANKS[level]}:{name}({cutoff:.2f})" in line.split("\t")[1] and f"{sd.RANKS[level]}:{name}" not in line.split("\t")[3].split(",")
                    hit += 1
    assert hit >= 1


def test_cases_ties(golden):
    s = golden["ties"]
    r = py_records(s)
    assert r[0]["ranks"][6][0] == 0 and r[3]["ranks"][6][0] == 0 and r[3]["strand"] == 1     # identical sequences: the lower number
    assert r[1]["ranks"][6][0] == 3 and len(s["db"][3]) < len(s["db"][2])                    # the shorter one, later in the database
    assert r[2]["ranks"][6][0] == 4 and s["db"][5].startswith(s["db"][4])                    # a prefix of another
    assert all(x["classified"] and x["ranks"][6][1] == 100 for x in r[:3])


def test_cases_strands(golden):
    r = py_records(golden["strands"])
    seen = set()
    for x in r:
        b, n = x["best_count"], x["boot_count"]
        if b[0] > b[1]:
            seen.add("plus on best") if x["strand"] == 0 else seen.add("wrong")
        elif b[1] > b[0]:
            seen.add("minus on best") if x["strand"] == 1 else seen.add("wrong")
        elif n[0] > n[1]:
            seen.add("plus on candidates") if x["strand"] == 0 else seen.add("wrong")
        elif n[1] > n[0]:
            seen.add("minus on candidates") if x["strand"] == 1 else seen.add("wrong")
        else:
            seen.add("equal: plus") if x["strand"] == 0 else seen.add("wrong")
    assert seen == {"plus on best", "minus on best", "plus on candidates", "minus on candidates", "equal: plus"}


def test_cases_vote(golden):
    s = golden["vote"]
    r = py_records(s)
    assert any(x["ranks"][5][1] == 100 and x["ranks"][6][1] < 100 and x["ranks"][7][1] <= x["ranks"][6][1] for x in r)   # losers leave below
    assert any(sd.tax_split(s["db_labels"][x["ranks"][5][0]])[5] == "" for x in r)                                     # the empty name wins a vote
    assert [golden[n]["opts"]["cutoff"] for n in ("vote", "vote_cutoff_0.5", "vote_cutoff_0.8", "vote_cutoff_1.0")] == [0.0, 0.5, 0.8, 1.0]
    cols = [[l.split("\t")[3] for l in golden[n]["ref"]["tabbed"]] for n in ("vote_cutoff_0.5", "vote_cutoff_0.8", "vote_cutoff_1.0")]
    assert cols[0] != cols[1] and cols[1] != cols[2]


def test_cases_masking_and_word_lengths(golden):
    cls = {n: [x["classified"] for x in py_records(golden[n])] for n in ("masking_none", "masking_soft", "masking_dust")}
    assert cls["masking_none"] == [1, 1, 1] and cls["masking_soft"] == [0, 1, 1] and cls["masking_dust"] == [0, 1, 1]
    assert [x["classified"] for x in py_records(sd.hardmask_sets()[0])] == [0, 1, 1]
    for w in (3, 5, 12):
        assert golden[f"wordlength_{w}"]["opts"]["wordlength"] == w and any(x["classified"] for x in py_records(golden[f"wordlength_{w}"]))
    assert golden["sintax_random"]["opts"]["random"] == 1 and any(x["classified"] for x in py_records(golden["sintax_random"]))
