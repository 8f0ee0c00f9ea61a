"""Shared inputs and restatements of the aligner tests (tests/test_gpu_parity.py, tests/marshal_data.py, tests/poison_cases.py)."""
import random

from tests import common


def torture_pairs():
    """the torture slice: IUPAC codes, lower case, unknown symbols, length-1 and ragged lengths"""
    rng = random.Random(77)
    pairs = []
    for _ in range(300):
        kind = rng.random()
        if kind < 0.3:
            a = common.rnd_seq(rng, rng.randint(1, 90), common.IUPAC + "acgtn-X")
            b = common.mutate(rng, a, 0.15, common.IUPAC + "acgtn")
        elif kind < 0.5:
            a, b = common.rnd_seq(rng, rng.randint(1, 3)), common.rnd_seq(rng, rng.randint(1, 40))
        elif kind < 0.7:
            a = common.rnd_seq(rng, rng.randint(1, 200))
            b = common.mutate(rng, a, 0.3, "ACGTN")
        else:
            a, b = common.rnd_seq(rng, rng.randint(0, 70)), common.rnd_seq(rng, rng.randint(0, 130))
        pairs.append((a, b))
    return pairs


def accept_py(q, t, row, f):
    """core/searchcore.cpp:343-464 (align_trim) + :664-737 (search_acceptable_aligned), evaluated on one result row
    -> (verdict: 1 accepted, 2 weak, 3 rejected; the identity the filter compares)"""
    import re
    score, al, ma, mi, ga, cigar = row
    runs = [(int(n) if n else 1, op) for n, op in re.findall(r"(\d*)([MID])", cigar)]
    tql = ttl = tqr = ttr = 0
    if runs and runs[0][1] != "M":
        if runs[0][1] == "D": tql = runs[0][0]
        else: ttl = runs[0][0]
    if runs and runs[-1][1] != "M":
        if runs[-1][1] == "D": tqr = runs[-1][0]
        else: ttr = runs[-1][0]
    if tql >= al: tqr = 0
    if ttl >= al: ttr = 0
    indels = al - ma - mi
    ial = al - tql - ttl - tqr - ttr
    iindels = indels - tql - ttl - tqr - ttr
    igaps = ga - (1 if tql + ttl > 0 else 0) - (1 if tqr + ttr > 0 else 0)
    Q, D = len(q), len(t)
    shortest, longest = min(Q, D), max(Q, D)
    iddef = f["iddef"]
    if iddef == 0: idv = 100.0 * ma / shortest if shortest > 0 else 0.0
    elif iddef == 2: idv = 100.0 * ma / ial if ial > 0 else 0.0
    elif iddef == 3: idv = max(0.0, 100.0 * (1.0 - (1.0 * (mi + ga) / longest)))
    else: idv = 100.0 * ma / al if al > 0 else 0.0
    ok = (idv >= 100.0 * f["weak_id"] and mi <= f["maxsubs"] and igaps <= f["maxgaps"] and ial >= f["mincols"]
          and (not f["leftjust"] or tql + ttl == 0) and (not f["rightjust"] or tqr + ttr == 0)
          and ma + mi >= f["query_cov"] * Q and ma + mi >= f["target_cov"] * float(D) and idv <= 100.0 * f["maxid"]
          and (ma + mi > 0 and 100.0 * ma / (ma + mi) >= f["mid"]) and mi + iindels <= f["maxdiffs"])
    if not ok:
        return 3, idv
    return (1 if idv >= 100.0 * f["id"] else 2), idv


def verdict_py(q, t, row, f):
    return accept_py(q, t, row, f)[0]
