"""No device: the inputs of tests/kmer_edge_data.py do what their `expect` says.  Everything here is asserted with the plain-Python
restatement (py_candidates, py_counts) and, where units, gaps or counters are claimed, with the packed format's host entries
(vsx_internal_kmer_pack_encode / _counter_of: the encoder is the code the build kernel runs).  This is what keeps
tests/test_gpu_kmer_edges.py from passing by missing its edges: every named edge is asserted present, none is skipped or filtered."""
import pytest

from tests import kmer_edge_data as ked


def test_counter_map_restated_equals_the_library():
    lib = ked._pack_lib()
    for s in list(range(0, 600)) + [32499, 32500, 32628, 32629]:
        assert lib.vsx_internal_kmer_pack_counter_of(s) == ked.counter_of(s) and ked.seq_of(ked.counter_of(s)) == s
    assert ked.counter_of(ked.TILE_SEQS - 1) == 32758 and ked.seq_of(255) == 391


def test_restatement_on_a_hand_worked_example():
    """by hand: the words of the query are ACGTA CGTAC GTACG (w = 5); t0 holds all three, t1 two (one twice), t2 one through U and
    lower case, t3 none valid (N); order = count desc, length asc, number asc"""
    db = ["ACGTACG", "TTACGTACCGTACTT", "ggtacgg", "ACGTNACG", "ACGUACG", "CGTAC"]
    q = "ACGTACG"
    assert ked.words_of(q, 5) == {"ACGTA", "CGTAC", "GTACG"}
    assert ked.words_of("ACGUacg", 5) == {"ACGTA", "CGTAC", "GTACG"} and ked.words_of("ACGUacg", 5, soft_mask=1) == set()
    assert ked.words_of("ACGTNACGTA", 5) == {"ACGTA"}
    assert ked.py_candidates(db, q, 5, 1, 10) == [(0, 3), (4, 3), (1, 2), (5, 1), (2, 1)]
    assert ked.py_candidates(db, q, 5, 3, 10) == [(0, 3), (4, 3)] and ked.py_candidates(db, q, 5, 9, 1) == [(0, 3)]
    assert ked.py_candidates(db, q, 5, 0, 10) is None and ked.py_candidates(db, "ACG", 5, 3, 10) is None
    assert ked.posting_count(db, 5) == 3 + 10 + 3 + 0 + 3 + 1 and ked.word_value("ACGTT") == 0b0001101111


def test_class_switch_queries_have_254_to_257_words_and_full_counts():
    db, queries, opts, expect = ked.class_switch()
    assert [e["n_words"] for e in expect] == [254, 255, 256, 257]
    for e in expect:
        q = queries[e["query"]]
        assert len(ked.words_of(q, 8)) == e["n_words"] == len(q) - 7, e["edge"]
        cnt = ked.py_counts(db, q, 8)
        exact, sub, pre = sorted(e["counts"])
        assert db[exact] == q and cnt[exact] == e["n_words"], e["edge"]
        assert cnt[sub] == e["n_words"] - 8 and cnt[pre] == e["n_words"] - 1, e["edge"]
        assert ked.py_candidates(db, q, 8, opts["minwordmatches"], ked.tophits_of(opts, len(db)))[:3] == [(exact, cnt[exact]), (pre, cnt[pre]), (sub, cnt[sub])]
    assert len(db) == 4 * 23
    assert max(ked.py_counts(db, queries[1], 8).values()) == 255                  # the byte is full, and nothing is above it


@pytest.mark.parametrize("w", [8, 12])
def test_threshold_groups_sit_in_one_dword_with_counts_around_the_threshold(w):
    db, queries, opts, expect = ked.threshold_edges(w)
    lib = ked._pack_lib()
    assert [len(ked.words_of(q, w)) for q in queries] == [255, 400]
    assert sorted((e["query"], e["minwordmatches"]) for e in expect) == sorted(
        [(0, m) for m in ked.MM_BYTE + (256,)] + [(1, m) for m in ked.MM_HALF])
    assert {e["minwordmatches"] for e in expect} == set(ked.MM_ALL)
    for e in expect:
        q, mm = queries[e["query"]], min(e["minwordmatches"], len(ked.words_of(queries[e["query"]], w)))
        cnt = ked.py_counts(db, q, w)
        slots = sorted(e["targets"])
        got = [cnt[s] for s in slots]
        n = len(ked.words_of(q, w))
        assert got == [mm - 1, mm, min(mm + 1, n), 0], (e["edge"], got)
        # the counters of the group: packed index (w <= 8) through the library's map, tagged index = the sequence number
        cs = [lib.vsx_internal_kmer_pack_counter_of(s) if w <= 8 else s for s in slots]
        assert cs == list(range(cs[0], cs[0] + 4)) and cs[0] % 4 == 0, (e["edge"], cs)
        if e["query"] == 0:
            assert len({c >> 2 for c in cs}) == 1                                  # four bytes of one dword
        else:
            assert cs[0] >> 1 == cs[1] >> 1 and cs[2] >> 1 == cs[3] >> 1           # two halves of one dword, twice
        cands = ked.py_candidates(db, q, w, e["minwordmatches"], ked.tophits_of(opts, len(db)))
        ts = {t for t, _ in cands}
        assert slots[1] in ts and slots[2] in ts and slots[0] not in ts and slots[3] not in ts, e["edge"]
    # the thresholds cross 128 (the sweep's two byte tests) and reach the full byte
    assert {1, 127, 128, 129, 255} <= {min(e["minwordmatches"], 255) for e in expect if e["query"] == 0}


def test_selection_cases_tie_and_fill_the_clamped_bin():
    db, queries, opts, expect = ked.selection_edges()
    keep = ked.tophits_of(opts, len(db))
    assert keep == 10
    assert [len(ked.words_of(q, 8)) for q in queries] == [100, 120, 400, 400, 255]
    for e in expect:
        q = queries[e["query"]]
        got = ked.py_candidates(db, q, 8, opts["minwordmatches"], keep)
        assert got == e["top"] and len(got) == 10, e["edge"]
        everything = ked.py_candidates(db, q, 8, opts["minwordmatches"], len(db))
        assert len(everything) > keep, e["edge"]                                  # the selection has something to cut
        assert sum(1 for _, c in everything if c >= 255) == e["at_or_above_255"]
    a, b, c, d, e5, f = expect
    alla = ked.py_candidates(db, queries[0], 8, 12, len(db))
    assert [x for _, x in alla] == [50] * 10 + list(range(34, 19, -1))
    allb = ked.py_candidates(db, queries[1], 8, 12, len(db))
    assert [x for _, x in allb] == [60] * 13 + [30] * 5
    lens = [len(db[t]) for t, _ in allb[:13]]
    assert lens == sorted(lens) and len(set(lens)) >= 5 and lens[9] == lens[10]          # the cut falls inside a run of equal lengths
    assert [t for t, _ in allb[:13]] != sorted(t for t, _ in allb[:13])                     # and the numbers alone would order otherwise
    assert [x for _, x in ked.py_candidates(db, queries[2], 8, 12, len(db))] == list(range(269, 255, -1)) and c["top"][-1][1] == 260
    assert [x for _, x in ked.py_candidates(db, queries[3], 8, 12, len(db))] == [300] * 14
    assert [x for _, x in ked.py_candidates(db, queries[4], 8, 12, len(db))] == [255] * 13
    assert c["at_or_above_255"] == 14 and d["at_or_above_255"] == 14 and e5["at_or_above_255"] == 13
    assert f["env"] == {"VSX_KMER_CAP": "3"} and f["query"] == c["query"] and a["env"] == {}


def test_bucket_trips_have_their_exact_units():
    db, queries, opts, expect = ked.bucket_trips()
    assert all(len(s) in (16, 24) for s in db) and len(db) <= ked.TILE_SEQS
    single = [e for e in expect if len(e["words"]) == 1]
    assert [e["units"][0] for e in single] == list(ked.TRIP_UNITS) and [e["trips"] for e in single] == [1, 1, 1, 2, 2, 3, 3, 4, 5]
    assert {e["trips"] % 3 for e in single} == {0, 1, 2}
    for e in expect:
        q = queries[e["query"]]
        assert q == "".join(e["words"])
        for word, units in zip(e["words"], e["units"]):
            hs = ked.holders(db, 8, word)
            assert ked.pack_units([ked.counter_of(t) for t in hs]) == units, e["edge"]
            assert 15 * (units - 1) < len(hs) <= 15 * units or units >= 40, e["edge"]
        assert e["trips"] == -(-sum(e["units"]) // 64)
        got = ked.py_candidates(db, q, 8, 1, len(db))
        assert {t for t, _ in got} >= set(ked.holders(db, 8, e["words"][0])) and len(got) >= 1
    a, b = [e for e in expect if len(e["words"]) == 2]
    assert a["units"] == [40, 40] and b["units"] == [64, 1]
    for e in (a, b):
        # the query's words in position order: the markers are words 0 and 8 (wave 0, lanes 0 and 1), the seven between them differ
        q = queries[e["query"]]
        words = [q[i:i + 8] for i in range(9)]
        assert len(set(words)) == 9 and words[0] == e["words"][0] and words[8] == e["words"][1]


def test_primer_buckets_fill_a_tile():
    db, queries, opts, expect = ked.primer_set()
    assert len(db) == 33000 and max(map(len, db)) <= 50 and len(expect) == 13
    for e in expect:
        hs = ked.holders(db, 8, e["word"])
        assert hs == list(range(33000)), e["edge"]
        assert e["units"] == [2176, 25]
        assert [ked.bucket_units(db, 8, e["word"], t) for t in (0, 1)] == e["units"]
    assert len({e["word"] for e in expect}) == 13 and all(q.startswith(db[0][:20]) for q in queries)
    top = ked.tophits_of(opts, len(db))
    for q in queries:
        assert len(ked.words_of(q, 8)) <= 255
        got = ked.py_candidates(db, q, 8, opts["minwordmatches"], len(db))
        assert len(got) == len(db) and got[top - 1][1] > 13               # every sequence qualifies; the heap is filled by relatives
    hit = {t for q in queries for t, _ in ked.py_candidates(db, q, 8, 12, top)}
    assert any(t >= ked.TILE_SEQS for t in hit) and any(t < ked.TILE_SEQS for t in hit)


def test_gap_patterns_have_their_gaps_and_hops():
    db, queries, opts, expect = ked.gap_edges()
    assert len(db) == ked.TILE_SEQS + 10
    by_edge = {tuple(e["counters"]): e for e in expect[:-1]}
    for want in ([0, 255], [0, 256], [0, 257], [3, 1012], [250, 252], [32758]):
        assert tuple(want) in by_edge
    assert sorted(len(e["counters"]) for e in expect[:-1] if len(e["counters"]) > 2) == [15, 16, 30, 31]
    dummies = set(range(251, 130 * 252, 252))
    for e in expect[:-1]:
        hs = ked.holders(db, 8, e["word"])
        assert hs == e["holders"] and sorted(ked.counter_of(t) for t in hs) == e["counters"], e["edge"]
        units = ked.pack_encode(e["counters"])
        incs = ked.pack_decode(units)
        assert len(units) // 4 == e["units"] and len(incs) == 15 * e["units"]
        real = [c for c in incs if c not in dummies]
        assert real == e["counters"], e["edge"]                                   # every posting once, in order
        upto = incs.index(e["counters"][-1])
        assert sum(1 for c in incs[:upto] if c in dummies) == e["hops"], e["edge"]
        assert all(c in dummies for c in incs[upto + 1:])                           # the tail of the last unit rests on a dummy
        got = ked.py_candidates(db, queries[e["query"]], 8, 1, len(db))
        assert sorted(t for t, _ in got) == e["holders"] and all(c == 1 for _, c in got)
    gaps = {tuple(e["counters"]): e["counters"][-1] - e["counters"][0] for e in expect[:-1] if len(e["counters"]) == 2}
    assert sorted(gaps.values()) == [2, 255, 256, 257, 1009]
    assert by_edge[(0, 255)]["hops"] == 0 and by_edge[(0, 256)]["hops"] == 1 and by_edge[(3, 1012)]["hops"] == 4
    assert by_edge[(250, 252)]["hops"] == 0 and 250 % 252 == 250                   # 251 between them is a dummy and is not hopped on
    for n, e in ((len(e["counters"]), e) for e in expect[:-1] if len(e["counters"]) > 2):
        assert e["counters"] == list(range(e["counters"][0], e["counters"][0] + n)) and e["units"] == -(-n // 15)
    edge = expect[-1]
    assert ked.holders(db, 8, edge["word"]) == [32629, 32630] == edge["holders"]
    assert 32629 // ked.TILE_SEQS == 0 and 32630 // ked.TILE_SEQS == 1 and ked.counter_of(32629) == 32758 and ked.counter_of(0) == 0
    assert sorted(t for t, _ in ked.py_candidates(db, queries[edge["query"]], 8, 1, len(db))) == [32629, 32630]
    assert 0 in by_edge[(0, 255)]["holders"]                                       # counter 0 is sequence 0


@pytest.mark.parametrize("w", [9, 12, 15])
def test_tag_buckets_mix_tags(w):
    db, queries, opts, expect = ked.tag_collisions(w)
    n_tags = 4 ** (w - 8)
    main = expect[0]["suffix"]
    bucket = ked.tag_bucket(db, w, main)
    assert len({x for x, _ in bucket}) == n_tags - 1 and len(bucket) > 256          # every tag but one, more than 64 units of four
    assert len(bucket) % 4 != 0                                                     # the last unit carries pads
    absent = [e for e in expect if e["matches"] == 0]
    assert len(absent) == 1 and queries[absent[0]["query"]][:w - 8] not in {x for x, _ in bucket}
    last = expect[1]
    assert queries[last["query"]][:w - 8] == bucket[-1][0] == "T" * (w - 8)          # the bucket is ordered by tag: these end it
    for e in expect:
        q = queries[e["query"]]
        got = ked.py_candidates(db, q, w, 1, len(db))
        assert len(got) == e["matches"], e["edge"]
        b = ked.tag_bucket(db, w, e["suffix"])
        assert len({x for x, _ in b}) > 1, e["edge"]                               # other tags share the bucket
        if "postings" in e:
            assert len(b) == e["postings"], e["edge"]
    assert sorted({e["postings"] for e in expect if "postings" in e}) == [4, 5, 8]
    assert any(len(ked.words_of(queries[e["query"]], w)) > 255 and e["matches"] > 0 for e in expect)
    assert ked.posting_count(db, w) == sum(len(ked.words_of(s, w)) for s in db)
