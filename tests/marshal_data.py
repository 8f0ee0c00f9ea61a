"""Inputs that put the result marshalling (the dense run buffer, vsx_cigar_text_kernel in vsearch_amd/csrc/vsx_tbtext.hip, settle() /
fetch_core() / fetch_ranked_lists() and the exports in vsx_fetch.cpp) on its edges, and what the scalar oracle says they must give.

A case is a dictionary: "name", "P" (scoring in search16_init order), "queries", "targets", "qidx", "tidx" (pairs by index: no
sequence is replicated), "host" (the pairs the library answers without the device: empty query, empty target, size guard) and
"unrelated" (pairs made to be rejected by FILTER).  The builders are deterministic; tests/test_marshal_host.py asserts with the
oracle, without a device, that every case reaches the edge it is named after, and tests/test_gpu_marshal.py compares the device
with the same oracle rows.

Facts used here (vsx_tbtext.hip, vsx_fetch.cpp): a pair's text is its CIGAR + NUL, padded with zero bytes to a multiple of 4 -- for
the pairs the DEVICE formats; the strings of host-answered pairs follow the device text in pair order, CIGAR + NUL back to back
without padding, so their offsets are not dword-aligned by design (fetch_core() writes them byte-wise on the host); one
lane formats one pair, a wave of 64 lanes allocates its strings with one atomic, a block is 256 lanes; a run length has 1 .. 5
digits (Q + D <= 65535) and is omitted when 1; the run buffer of a plan starts at min(worst, max(16 Mi words, 48 per pair)) + 1
words and its text buffer at min(6 worst + 8 pairs, max(32 MiB, 128 B per pair)) + 16 bytes.
"""
import functools
import random
import re

import numpy as np

from tests import common

DEFAULT = (2, -4, 1, 1, 18, 18, 1, 1, 1, 1, 2, 2, 1, 1)
ZERO_TERMINAL = (2, -4, 0, 0, 18, 18, 0, 0, 0, 0, 2, 2, 0, 0)      # terminal gaps are free: a 65 519-symbol overhang keeps its score in int16
CHEAP_GAPS = (2, -40) + (1,) * 12                                   # a mismatch is never taken: alignments are matches and many short gaps
FILTER = dict(id=0.9, weak_id=0.9)                                  # iddef 2; below 90 % a pair is rejected: no runs, empty string
FILTER_FULL = dict(iddef=2, id=0.9, weak_id=0.9, maxid=1.0, mid=0.0, query_cov=0.0, target_cov=0.0, maxsubs=2 ** 31 - 1,
                   maxgaps=2 ** 31 - 1, mincols=0, maxdiffs=2 ** 31 - 1, leftjust=0, rightjust=0)
# the filter of the ranked calls: stricter, so that fewer than half of a case's pairs are kept (tests/test_marshal_host.py asserts it:
# a kept list written twice -- what a plan run again without resetting its list counts would give -- still fits the list's n + 1 entries)
RANKED_FILTER = dict(id=0.97, weak_id=0.97)
SENTINEL_ROW =(32767, 0, 0, 0, 0, "")

SQUARES = (1, 2, 9, 10, 11, 99, 100, 101, 999, 1000, 1001, 4999, 5000)      # 5000 x 5000: the largest square with Q D <= 25e6
CORE = "CGTCGTCG"                                                            # the 8-symbol query of the overhang pairs: no A
# A-flanks left / right of CORE; "10000I8M" and "65519I8M" are 9 bytes with their NUL (a five-digit count miscounted as four would
# fit them into 8), the last one has Q + D = 65535
OVERHANGS = ((9999, 10000), (10000, 9999), (10000, 0), (32767, 3), (3, 32768), (65519, 0))
WAVE_COUNTS = (1, 63, 64, 65, 255, 256, 257)
RUNS_CAP_NATURAL = (16 << 20) + 1
TEXT_CAP_NATURAL = (32 << 20) + 16
NATURAL_PAIRS = 131072


def runs_of(cigar):
    """CIGAR text -> [(length, op)] in text order"""
    return [(int(n) if n else 1, op) for n, op in re.findall(r"(\d*)([MID])", cigar)]


def padded(cigar):
    """bytes of a pair's string in the device text: CIGAR + NUL, rounded up to a dword"""
    return (len(cigar) + 1 + 3) & ~3


def _case(name, P, queries, targets, qidx, tidx, host=(), unrelated=(), refused=()):
    return dict(name=name, P=P, queries=queries, targets=targets, qidx=np.asarray(qidx, np.uint32), tidx=np.asarray(tidx, np.uint32),
                host=sorted(host), unrelated=sorted(unrelated), refused=sorted(refused))


@functools.lru_cache(maxsize=None)
def digit_edges():
    """two cases.  "squares": identical pairs of n symbols -> nM for n in SQUARES (1 | 2 ... 999 | 1000 digits, every string length
    mod 4).  "overhangs": CORE against A...A CORE A...A -> <left>I 8M <right>I with runs of 9999, 10000, 32767, 32768 and 65519."""
    rng = random.Random(20261)
    sq = [common.rnd_seq(rng, n) for n in SQUARES]
    idx = np.arange(len(sq))
    ts = ["A" * a + CORE + "A" * b for a, b in OVERHANGS]
    return (_case("squares", DEFAULT, sq, sq, idx, idx),
            _case("overhangs", ZERO_TERMINAL, [CORE], ts, np.zeros(len(ts)), np.arange(len(ts))))


@functools.lru_cache(maxsize=None)
def wave_edges():
    """one case per device pair count in WAVE_COUNTS (around one wave and one block of the text kernel): queries of 20 .. 60 symbols
    against lightly mutated targets under CHEAP_GAPS (string lengths vary inside a wave), every fifth device pair unrelated (FILTER
    rejects it: zero runs, empty string), plus three pairs the host answers -- an empty query (the closed form "<D>I"), an empty
    target and a size-guard sentinel -- at the front, in the middle and at the end of the pair list.  From 63 pairs on, device pair 9
    is one whose score leaves int16 (CORE against 40 000 A under CHEAP_GAPS): the device aligner refuses it, a ranked call lists it
    as undecided"""
    out = []
    for n in WAVE_COUNTS:
        rng = random.Random(9002 + n)          # (9003: the single pair of the first case is one the filter keeps)
        pairs = []
        for k in range(n):
            q = common.rnd_seq(rng, rng.randint(20, 60))
            if k == 9:
                pairs.append((CORE, "A" * 40000, "refused"))          # score below int16: the device aligner refuses it (sentinel row)
            elif k % 5 == 4:
                pairs.append((q, common.rnd_seq(rng, rng.randint(20, 60)), "unrelated"))
            else:
                pairs.append((q, common.mutate(rng, q, 0.03), "related"))
        specials = [("", common.rnd_seq(rng, 7), "host"), (common.rnd_seq(rng, 12), "", "host"), ("A" * 10, "C" * 65530, "host")]
        for at, pr in zip([0, n // 2 + 1, n + 2], specials):
            pairs.insert(at, pr)
        idx = np.arange(len(pairs))
        out.append(_case(f"wave{n}", CHEAP_GAPS, [p[0] for p in pairs], [p[1] for p in pairs], idx, idx,
                         *[[k for k, p in enumerate(pairs) if p[2] == tag] for tag in ("host", "unrelated", "refused")]))
    return tuple(out)


def wave_case(n):
    return wave_edges()[WAVE_COUNTS.index(n)]


@functools.lru_cache(maxsize=None)
def dense_runs():
    """24 distinct random pairs of about 250 x 330 symbols under CHEAP_GAPS: about 188 runs and 292 text bytes per pair, four times
    the 48 words / 128 bytes a plan's buffers start with per pair.  Used through index arrays (dense_index)."""
    rng = random.Random(1888)
    qs = [common.rnd_seq(rng, rng.randint(240, 260)) for _ in range(24)]
    ts = [common.rnd_seq(rng, rng.randint(320, 340)) for _ in range(24)]
    idx = np.arange(24)
    return _case("dense", CHEAP_GAPS, qs, ts, idx, idx)


def dense_index(n):
    """n pairs over the 24 of dense_runs(): pair k is distinct pair k mod 24"""
    return (np.arange(n) % 24).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def dense_mixed(n):
    """n pairs: the 24 of dense_runs() by index, every 97th (k mod 97 = 48) one the host answers, alternately an empty query (the
    closed form "7I") and an empty target (sentinel).  Neighbouring pairs never share a query, so a pipeline cuts its slices exactly
    where its schedule says (pipeline_cuts)."""
    d = dense_runs()
    rng = random.Random(97)
    queries = d["queries"] + ["", common.rnd_seq(rng, 12)]
    targets = d["targets"] + [common.rnd_seq(rng, 7), ""]
    qidx, tidx, host = dense_index(n).copy(), dense_index(n).copy(), []
    for k in range(48, n, 97):
        qidx[k] = tidx[k] = 24 + (len(host) & 1)
        host.append(k)
    return _case(f"mixed{n}", CHEAP_GAPS, queries, targets, qidx, tidx, host)


PIPE_PAIRS, PIPE_SLICE, PIPE_RUNS_CAP, PIPE_TEXT_CAP = 4200, 700, 60000, 90000


def pipeline_cuts(n, slice_pairs):
    """the slice boundaries vsx_align_pairs takes for n >= 3 slices' worth of pairs whose neighbours never share a query (vsx_align_pairs.cpp
    align_pairs_impl): a quarter and a half slice, the middle in equal parts of at most a slice, a half and a quarter"""
    assert n >= 3 * slice_pairs
    head = [slice_pairs // 4, slice_pairs // 2]
    mid = n - 2 * sum(head)
    k = -(-mid // slice_pairs)
    sizes = head + [mid * (x + 1) // k - mid * x // k for x in range(k)] + head[::-1]
    assert sum(sizes) == n and min(sizes) >= slice_pairs // 16
    return np.cumsum([0] + sizes).tolist()


def oracle_rows(case, oracle):
    """the oracle's row of every pair of a case (each distinct (query, target) once)"""
    memo = {}
    rows = []
    for q, t in zip(case["qidx"].tolist(), case["tidx"].tolist()):
        if (q, t) not in memo:
            memo[(q, t)] = tuple(oracle.align(case["queries"][q], case["targets"][t], case["P"]))
        rows.append(memo[(q, t)])
    return rows


def filtered_rows(case, rows, flt=FILTER_FULL):
    """what a plan with the accept filter returns: (rows, verdicts) -- the oracle's rows with the restated verdict
    (tests/aligner_data.py verdict_py: align_trim + search_acceptable_aligned); a rejected pair keeps its numbers and loses its
    CIGAR, a pair the host answers or the 16-bit aligner refuses (sentinel score) stays undecided"""
    from tests.aligner_data import verdict_py as _verdict_py
    out, verdicts = [], []
    host = set(case["host"])
    for k, row in enumerate(rows):
        q, t = case["queries"][case["qidx"][k]], case["targets"][case["tidx"][k]]
        if k in host or row[0] == 32767:
            v = 0
        else:
            v = _verdict_py(q, t, row, flt)
        verdicts.append(v)
        out.append(row[:5] + ("",) if v == 3 else row)
    return out, verdicts


def full_filter(**kw):
    d = dict(FILTER_FULL)
    d.update(kw)
    return d


def slice_overflows(case, rows, cuts, runs_cap, text_cap):
    """per slice [cuts[i], cuts[i + 1]): do its device pairs need more than runs_cap run words / text_cap text bytes?"""
    host = set(case["host"])
    over_runs, over_text = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        dev = [rows[k] for k in range(a, b) if k not in host]
        over_runs.append(used_words(dev) > runs_cap)
        over_text.append(sum(padded(r[5]) for r in dev) > text_cap)
    return over_runs, over_text


def used_words(rows):
    """run words the device pairs of these rows occupy (a pair the host answers adds its word behind them: count it separately)"""
    return sum(len(runs_of(r[5])) for r in rows)
