"""The batched walk of the tilted traceback (walk() in vsx_traceback_tilt_kernel): a trip consumes up to WB cells of a
diagonal run from one round of LDS reads (tests/test_walk_batch_math.py holds the model).  Every field of every pair, CIGAR included,
against the oracle, in each tile class the kernel is built for: R = 10; R = 14 (LDS-staged checkpoints); R = 16 with 15, 6 and no dummy
rows in position 0; R = 20 and R = 26 in two half tiles of 10 and 13 rows (13 is odd: the junk row).

Targets are copies of the query between random flanks with planted edits.  Two scorings: the default one, whose gap open of 18 keeps
gaps at least seven columns apart, and the same with an interior gap open of 1, under which an optimal alignment keeps planted gaps that
are a single match apart -- so that diagonal runs of every length 1 .. 17 (2 WB + 1 for WB = 8) lie between two gaps, asserted on the
oracle's CIGARs.  The edits begin at every offset 0 .. 16 of the copy and the flanks vary, so batches meet the left edge, the top edge and
the HR boundary of a tile in every phase, and the path reaches row 0 inside a batch."""
import random
import re

import numpy as np
import pytest

from tests import common

DEFAULT = (2, -4, 1, 1, 18, 18, 1, 1, 1, 1, 2, 2, 1, 1)
CHEAP_OPEN = (2, -4, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 1, 1)         # interior gap open 1: a one-symbol gap (3) is cheaper than a mismatch (4)
OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def _edited_copy(rng, q, first, runs, gaps):
    """q with planted edits: `first` clean symbols, then gap, runs[0] clean symbols, gap, runs[1] ... (an 'I' gap = symbols only the
    target has, a 'D' gap = query symbols the target lacks); what is left of q follows clean"""
    out, p = [q[:first]], first
    for n, (kind, glen) in zip(runs, gaps):
        if p + glen + n + 2 > len(q):
            break
        if kind == "I":
            # symbols that match neither neighbour of the cut: the gap cannot slide or pay for itself
            out.append("".join(OTHER[q[p]] if OTHER[q[p]] != q[p - 1] else OTHER[OTHER[q[p]]] for _ in range(glen)))
        else:
            p += glen
        out.append(q[p:p + n])
        p += n
    out.append(q[p:])
    return "".join(out)


def _targets(rng, q, n, min_run):
    """n targets; the clean runs between gaps cycle through min_run .. 17, rotated per target; the first edit at offset x % 17"""
    lens = list(range(min_run, 18))
    kinds = [("I", 1), ("D", 1), ("I", 3), ("D", 2), ("D", 1), ("I", 1), ("I", 2), ("D", 4)]
    ts = []
    for x in range(n):
        runs = [lens[(x * 5 + k) % len(lens)] for k in range(64)]
        gaps = [kinds[(x + k + (k // 8)) % len(kinds)] for k in range(64)]
        copy = _edited_copy(rng, q, x % 17 + (1 if x % 3 else 0) * 17 * (x % 4), runs, gaps)
        left = 0 if x % 8 == 0 else rng.randint(1, 40)
        right = (0, 3, 17, 40)[x % 4] + rng.randint(0, 12)
        ts.append(common.rnd_seq(rng, left) + copy + common.rnd_seq(rng, right))
    return ts


def _between_gaps(cigar):
    """lengths of the M runs that have a gap run on both sides"""
    ops = re.findall(r"(\d*)([MID])", cigar)
    return {int(n or 1) for k, (n, o) in enumerate(ops) if o == "M" and 0 < k < len(ops) - 1}


def _run(oracle, qs, ts, qi, ti, P):
    from vsearch_amd import Aligner
    qi, ti = np.array(qi, np.uint32), np.array(ti, np.uint32)
    with Aligner(scoring=P, n_mismatch=False) as al:
        p = al.plan(al.sequences(qs), al.sequences(ts), qi, ti)
        info = p.describe()
        p.run()
        p.sync()
        res = p.fetch()
        p.close()
    exp = [tuple(oracle.align(qs[qi[k]], ts[ti[k]], P, False)) for k in range(len(qi))]
    for k in range(len(qi)):
        assert res.row(k) == exp[k], (k, len(qs[qi[k]]), len(ts[ti[k]]))
    return info, [e[5] for e in exp]


# Q -> rows per lane of its class
CLASSES = [(150, 10), (220, 14), (241, 16), (250, 16), (256, 16), (300, 20), (400, 26)]


@pytest.mark.gpu
@pytest.mark.parametrize("Q,R", CLASSES)
def test_planted_edits_cheap_gap_open(gpu_required, oracle, Q, R):
    rng = random.Random(7000 + Q)
    q = common.rnd_seq(rng, Q)
    ts = _targets(rng, q, 32, 1)
    info, cigars = _run(oracle, [q], ts, [0] * len(ts), range(len(ts)), CHEAP_OPEN)
    print(Q, info)
    assert info["rows_dominant"] == R and info["tasks_tilted"] == info["tasks"] and info["tasks_tracked"] == 0
    seen, text = set(), " ".join(cigars)
    for c in cigars:
        seen |= _between_gaps(c)
    assert set(range(1, 18)) <= seen, sorted(set(range(1, 18)) - seen)
    # gaps of one symbol and longer, both kinds, each followed directly by M
    for pat in (r"[MD]IM", r"[MI]DM", r"\d+IM", r"\d+DM"):
        assert re.search(pat, text), pat


@pytest.mark.gpu
@pytest.mark.parametrize("Q,R", CLASSES)
def test_planted_edits_default_scoring(gpu_required, oracle, Q, R):
    rng = random.Random(8000 + Q)
    qa, qb = common.rnd_seq(rng, Q), common.rnd_seq(rng, Q)
    ta = _targets(rng, qa, 16, 7)
    # one target with IUPAC symbols; two with the long right overhang of a database hit (the run along the last query row)
    t = list(ta[5])
    for p, s in zip(rng.sample(range(len(t)), 6), "NRYKMW"):
        t[p] = s
    ta[5] = "".join(t)
    ta[6] += common.rnd_seq(rng, 700)
    ta[7] = common.rnd_seq(rng, 300) + ta[7] + common.rnd_seq(rng, 420)
    # an exact copy that starts at column 0: row 0 and column 0 are reached together, at the end of one long diagonal
    ta[8] = qa + common.rnd_seq(rng, 9)
    # a second query with one task of five targets
    tb = _targets(rng, qb, 5, 9)
    qi = [0] * len(ta) + [1] * len(tb)
    info, cigars = _run(oracle, [qa, qb], ta + tb, qi, range(len(qi)), DEFAULT)
    print(Q, info)
    assert info["rows_dominant"] == R and info["tasks_tilted"] == info["tasks"] == 3 and info["tasks_tracked"] == 0
    assert re.search(r"\dM\d*[ID]\d*M", " ".join(cigars))
