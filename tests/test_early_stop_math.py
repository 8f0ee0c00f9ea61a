"""not gpu: the early-stop criterion of the DP kernel (vsx_forward_kernel EARLY), checked in plain Python integers.

Once the alignment has left the query's last row, every remaining target column is the right-terminal gap; the kernel may end the
task as soon as that is PROVEN.  The model below holds
  * the full DP with the 14 penalties and the leave rule of the last row (lv1(j) = cont(j) ? lv1(j - 1) : j, cont = left or ext-left;
    leave = left(D - 1) ? lv1(D - 2) : D - 1),
  * the systolic schedule (pipeline position l works on column t - l at step t and owns R rows; the spare slots of position 0 are dummy
    rows ABOVE row 0 that carry the top border),
  * the criterion after every step, in plain coordinates and in the kernel's tilted, 0x3E00-biased 16-bit form (two per-position
    Horner maxima over 16-bit halves, then 32-bit arithmetic per lane and half).

After step t the computed region is the staircase {(r, j) : j <= t - lane(r)}; a path to (Q - 1, D - 1) leaves it once, through a
frontier cell p = (r, j): a cell of a position's current column, a position's bottom row one column back (its diagonal successor
belongs to the next position), or the top border cell (-1, t).  From p the path has rows = Q - 1 - r rows and cols = D - 1 - j columns
to cover: a diagonal moves (a <= min(rows, cols)), cols - a horizontal and rows - a vertical ones.  With M = the largest score (at
least 0), e = the smallest of the six gap extensions (opens and extensions >= 0) and W0 = M + e it scores at most
    UB(p) = H(p) + (M + 2e) min(rows, cols) - e (rows + cols) = min(H(p) + W0 rows - e cols,  H(p) + W0 cols - e rows),
whatever gap state it leaves p in (E, F <= H, no open is charged).  Extending the last row's own run is a real path:
    LB = E(Q - 1, c + 1) - (D - 2 - c) R_q(right),  c = t - l_last.
If UB(p) < LB strictly for every frontier cell but (Q - 1, c), every optimal path runs along the last row from column c: the full run
ends with score = LB, leave = lv1(c) and left(D - 1) strictly.  Per position the kernel takes min(max_p first form, max_p second form),
which is >= every UB(p) of the position.  For every step at which the criterion holds the tests require exactly that of the full DP.

(The first form alone -- a <= rows only -- can never hold when both ends price a terminal gap alike: the top border cell then keeps
UB = (M + e) Q - e (D - 1) - go - ge whatever t is, and no alignment scores more than M Q - e (D - Q).  What ends a task early is the
second form: too few columns are left for the query to match anywhere else.  test_row_bound_alone_never_fires pins that.)"""
import random

import pytest

BIAS = 0x3E00            # the MAX3 class: values live in [0, 0x7BFF]
DEFAULT = dict(match=2, mismatch=-4, go_q_l=1, go_t_l=1, go_q_i=18, go_t_i=18, go_q_r=1, go_t_r=1,
               ge_q_l=1, ge_t_l=1, ge_q_i=2, ge_t_i=2, ge_q_r=1, ge_t_r=1)


def _p14(s):
    return (s["match"], s["mismatch"], s["go_q_l"], s["go_t_l"], s["go_q_i"], s["go_t_i"], s["go_q_r"], s["go_t_r"],
            s["ge_q_l"], s["ge_t_l"], s["ge_q_i"], s["ge_t_i"], s["ge_q_r"], s["ge_t_r"])


def _dp(q, t, s):
    """plain coordinates, no saturation -> H[i][j], En[j] = E(Q-1, j+1), htop, score, leave, left(D-1) margin, lv1 after each column"""
    Q, D = len(q), len(t)
    QR = lambda x, y: s[f"go_{x}_{y}"] + s[f"ge_{x}_{y}"]
    R = lambda x, y: s[f"ge_{x}_{y}"]
    htop = [-(s["go_q_l"] + (j + 1) * s["ge_q_l"]) for j in range(D)]
    hleft = [-(s["go_t_l"] + (i + 1) * s["ge_t_l"]) for i in range(Q)]
    H = [[0] * D for _ in range(Q)]
    E = [hleft[i] - QR("q", "i" if i < Q - 1 else "r") for i in range(Q)]
    En, lv1s = [0] * D, [0] * D
    lv1, leave, margin = -1, None, None
    for j in range(D):
        qrt, rt = (QR("t", "i"), R("t", "i")) if j < D - 1 else (QR("t", "r"), R("t", "r"))
        F = htop[j] - qrt
        for i in range(Q):
            qrq, rq = (QR("q", "i"), R("q", "i")) if i < Q - 1 else (QR("q", "r"), R("q", "r"))
            if i == 0:
                hd = 0 if j == 0 else htop[j - 1]
            else:
                hd = hleft[i - 1] if j == 0 else H[i - 1][j - 1]
            h1 = max(hd + (s["match"] if q[i] == t[j] else s["mismatch"]), F)
            left = E[i] > h1
            h = max(h1, E[i])
            he, e = h - qrq, E[i] - rq
            if i == Q - 1:
                if j == D - 1:
                    leave = lv1 if left else j
                    margin = E[i] - h1
                lv1 = lv1 if (left or e > he) else j
                lv1s[j] = lv1
            F = max(F - rt, h - qrt)
            E[i] = max(e, he)
            H[i][j] = h
        En[j] = E[Q - 1]
    return H, En, htop, H[Q - 1][D - 1], leave, margin, lv1s


class Schedule:
    """pipeline geometry of a single-strip task: npos positions of R rows, the spare slots of position 0 on top"""

    def __init__(self, Q, R):
        assert Q <= 16 * R
        self.Q, self.R = Q, R
        self.npos = (Q + R - 1) // R
        self.rcnt0 = Q - (self.npos - 1) * R
        self.pad = R - self.rcnt0
        self.l_last = self.npos - 1

    def row(self, l, k):
        return k - self.pad if l == 0 else self.rcnt0 + (l - 1) * self.R + k


def _consts(s):
    M = max(s["match"], s["mismatch"], 0)
    e = min(s[f"ge_{x}_{y}"] for x in "qt" for y in "lir")
    return M + e, e


def _plain_tables(sch, H, htop, s):
    """per (position, column): max over the position's slots of H + W0 rows and of H - e rows -- (all slots, all but slot R-1) each"""
    W0, e = _consts(s)
    Q, R, D = sch.Q, sch.R, len(htop)
    tabs = [[[0] * D for _ in range(sch.npos)] for _ in range(4)]
    for l in range(sch.npos):
        for j in range(D):
            v1, v2 = [], []
            for k in range(R):
                i = sch.row(l, k)
                h = H[i][j] if i >= 0 else htop[j]                    # dummy rows carry the top border
                v1.append(h + W0 * (Q - 1 - i))
                v2.append(h - e * (Q - 1 - i))
            tabs[0][l][j], tabs[1][l][j] = max(v1), max(v1[:-1])
            tabs[2][l][j], tabs[3][l][j] = max(v2), max(v2[:-1])
    return tabs


def _plain_criterion(sch, tabs, H, En, htop, D, s, t, rows_only=False):
    """state after step t -> (holds, LB)"""
    W0, e = _consts(s)
    Q, R = sch.Q, sch.R
    full1, excl1, full2, excl2 = tabs
    c = t - sch.l_last
    LB = En[c] - (D - 2 - c) * s["ge_q_r"]
    for l in range(sch.npos):
        j = t - l
        cols = D - 1 - j
        # (a) the position's current column; (Q-1, c) itself is the run LB extends
        f1 = (excl1 if l == sch.l_last else full1)[l][j] - e * cols
        f2 = (excl2 if l == sch.l_last else full2)[l][j] + W0 * cols
        if l < sch.l_last:                                            # (b) the bottom row one column back
            i = sch.row(l, R - 1)
            f1 = max(f1, H[i][j - 1] + W0 * (Q - 1 - i) - e * (cols + 1))
            f2 = max(f2, H[i][j - 1] - e * (Q - 1 - i) + W0 * (cols + 1))
        if l == 0:                                                    # (c) the top border cell (-1, t)
            f1 = max(f1, htop[t] + W0 * Q - e * cols)
            f2 = max(f2, htop[t] - e * Q + W0 * cols)
        if not (f1 if rows_only else min(f1, f2)) < LB:
            return False, LB
    return True, LB


def _u16(v):
    assert 0 <= v <= 0xFFFF, v
    return v


def _tilted_tables(sch, H, htop, s):
    """the kernel's per-position Horner maxima over 16-bit unsigned halves holding X + (i + j) g + BIAS:
    max_k H*[k] + w (R - 1 - k) for w = W0 + g and w = g - e -- (rows 0 .. R-2 only, all rows) each -- and H*[R-1] itself"""
    W0, e = _consts(s)
    g = s["ge_t_i"]
    R, D = sch.R, len(htop)

    def star(i, j):
        v = (H[i][j] if i >= 0 else htop[j]) + (i + j) * g + BIAS
        assert 0 <= v <= 0x7BFF, v
        return v

    tabs = [[[0] * D for _ in range(sch.npos)] for _ in range(5)]
    for l in range(sch.npos):
        for j in range(D):
            for n, w in enumerate((W0 + g, g - e)):
                m = star(sch.row(l, 0), j)
                for k in range(1, R - 1):
                    m = max(_u16(m + w), star(sch.row(l, k), j))
                m = _u16(m + w)
                tabs[2 * n][l][j] = m
                tabs[2 * n + 1][l][j] = max(m, star(sch.row(l, R - 1), j))
            tabs[4][l][j] = star(sch.row(l, R - 1), j)
    return tabs


def _tilted_criterion(sch, tabs, En, htop, D, s, t):
    """the kernel's form: every packed sum must stay inside a 16-bit half; the per-lane part is 32-bit.  Both sides of the comparison
    carry the common term g (Q - 1) + BIAS.  -> (holds, un-tilted closed-form score)"""
    W0, e = _consts(s)
    g = s["ge_t_i"]
    W1, W2 = W0 + g, g - e
    Q, R = sch.Q, sch.R
    excl1, full1, excl2, full2, last = tabs
    c = t - sch.l_last
    elast = En[c] + (Q + c) * g + BIAS                               # E*[R-1] of the last position after the step
    assert 0 <= elast <= 0x7BFF
    lb = elast - g * (c + 1) - (D - 2 - c) * s["ge_q_r"]
    holds = True
    for l in range(sch.npos):
        j = t - l
        cols = D - 1 - j
        if l < sch.l_last:
            hb = last[l][j - 1]                                       # the other ping-pong set's slot R-1
            m1 = max(full1[l][j], _u16(hb + (g - e)))
            m2 = max(full2[l][j], _u16(hb + (g + W0)))
        else:
            m1, m2 = excl1[l][j], excl2[l][j]
        if l == 0:
            top = htop[t] + (t - 1) * g + BIAS                        # the tilted top-border table entry, biased
            assert 0 <= top <= 0x7BFF
            m1 = max(m1, _u16(top + W1 * sch.rcnt0))
            m2 = max(m2, _u16(top + W2 * sch.rcnt0))
        rows_b = (sch.l_last - l) * R
        f1 = m1 + W1 * rows_b - e * cols - g * j
        f2 = m2 + W2 * rows_b + W0 * cols - g * j
        holds = holds and min(f1, f2) < lb
    score_star = elast - (D - 2 - c) * (s["ge_q_r"] - g)              # H*(Q-1, D-1), what the epilogue un-tilts
    return holds, score_star - BIAS - (Q + D - 2) * g


def _check_pair(q, t, R, s, oracle=None):
    """every step of phase A: both forms agree, and where the criterion holds the closed form is the full DP's answer.
    -> (first firing column c or None, leave, D)"""
    Q, D = len(q), len(t)
    sch = Schedule(Q, R)
    H, En, htop, score, leave, margin, lv1s = _dp(q, t, s)
    if oracle is not None:
        # anchor of the model: the reference recurrence's score, and its traceback's trailing run of 'I' (= D - 1 - leave)
        o = oracle.align(q, t, _p14(s))
        assert o[0] == score
        cig = o[5]
        n_i = 0
        if cig.endswith("I"):
            digits = ""
            k = len(cig) - 2
            while k >= 0 and cig[k].isdigit():
                digits = cig[k] + digits
                k -= 1
            n_i = int(digits) if digits else 1
        assert D - 1 - n_i == leave, (cig, leave)
    ptabs, ttabs = _plain_tables(sch, H, htop, s), _tilted_tables(sch, H, htop, s)
    first = None
    for t_ in range(max(sch.npos, 1), D - 1):                         # all positions at a column >= 1, position 0 before column D-1
        c = t_ - sch.l_last
        plain, LB = _plain_criterion(sch, ptabs, H, En, htop, D, s, t_)
        tilted, sc = _tilted_criterion(sch, ttabs, En, htop, D, s, t_)
        assert plain == tilted, (t_, plain, tilted)
        if plain:
            assert LB == score and sc == score, (t_, LB, sc, score)
            assert lv1s[c] == leave, (t_, lv1s[c], leave)
            assert leave < D - 1 and margin > 0, (t_, leave, margin)    # left(D-1) holds strictly
            if first is None:
                first = c
    return first, leave, D


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _mutate(rng, seq, div):
    out = []
    for ch in seq:
        x = rng.random()
        if x < div * 0.6:
            out.append(rng.choice([b for b in "ACGT" if b != ch]))
        elif x < div * 0.8:
            continue
        elif x < div:
            out.append(ch)
            out.append(rng.choice("ACGT"))
        else:
            out.append(ch)
    return "".join(out)


def _related(rng, Q, D, offset, div):
    t = _rand(rng, D)
    q = _mutate(rng, t[offset:offset + Q], div)
    while len(q) < Q:
        q += rng.choice("ACGT")
    return q[:Q], t


SCORINGS = [
    DEFAULT,
    dict(DEFAULT, match=3, mismatch=-5, ge_q_r=2, ge_t_r=2, ge_q_l=2, ge_t_l=2),          # M + e = 5, R_q(right) > e elsewhere
    dict(DEFAULT, match=1, mismatch=-2, go_q_r=2, ge_q_r=3, ge_t_r=1, ge_q_i=3, ge_t_i=3, go_q_i=10, go_t_i=10),
    dict(DEFAULT, ge_t_r=0, ge_t_l=0),                                                     # e = 0
]


@pytest.mark.parametrize("seed", range(4))
def test_closed_form_equals_full_dp_on_related_pairs(seed, oracle):
    rng = random.Random(seed)
    fired = 0
    for n in range(10):
        s = SCORINGS[n % len(SCORINGS)]
        R = rng.choice([3, 4, 5])
        Q = rng.randint(R + 1, 16 * R)
        long_overhang = n % 2 == 1                                    # every other pair: a close copy near the left end
        D = Q + (rng.randint(120, 160) if long_overhang else rng.randint(40, 160))
        off = rng.randint(0, 10) if long_overhang else rng.randint(0, D - Q)
        q, t = _related(rng, Q, D, off, rng.choice([0.0, 0.03]) if long_overhang else rng.choice([0.0, 0.05, 0.15]))
        first, leave, _ = _check_pair(q, t, R, s, oracle if n < 4 else None)
        fired += first is not None
    assert fired >= 3


@pytest.mark.parametrize("Q,R", [(64, 4), (49, 4), (80, 5), (66, 5)])
def test_no_dummy_rows_and_one_real_row_in_position_zero(Q, R):
    # Q = 16 R: no dummy rows, the top border enters through the table alone; Q = 16 R - 15 (and R = 5: 66): R - 1 dummy rows
    rng = random.Random(Q * 100 + R)
    fired = 0
    for off in (0, 20, 70):
        for s in SCORINGS:
            q, t = _related(rng, Q, Q + 150, off, 0.04)
            first, _, _ = _check_pair(q, t, R, s)
            fired += first is not None
    assert fired > 0


def test_short_overhang():
    # D - Q < 32: phase A is short and the criterion has little room; whatever it decides must be right
    rng = random.Random(5)
    for d in (1, 2, 7, 16, 31):
        for s in SCORINGS[:2]:
            q, t = _related(rng, 48, 48 + d, 0, 0.03)
            _check_pair(q, t, 4, s)
            q, t = _related(rng, 48, 48 + d, d, 0.03)
            _check_pair(q, t, 4, s)


def test_query_at_the_far_right_end_never_fires():
    rng = random.Random(6)
    for s in SCORINGS:
        q, t = _related(rng, 50, 200, 150, 0.03)
        first, leave, D = _check_pair(q, t, 4, s)
        assert first is None and leave >= D - 3                       # (a mutation may shorten the window by a column or two)


def test_unrelated_target():
    rng = random.Random(7)
    for s in SCORINGS:
        for R in (4, 5):
            _check_pair(_rand(rng, 13 * R), _rand(rng, 13 * R + 120), R, s)


def test_weak_copy_followed_by_exact_copy():
    # a weak copy of the query, then an exact one: the alignment belongs to the exact copy, and the criterion must not fire between them
    rng = random.Random(8)
    for s in SCORINGS:
        q = _rand(rng, 56)
        weak = _mutate(rng, q, 0.25)
        t = _rand(rng, 10) + weak + _rand(rng, 30) + q + _rand(rng, 90)
        exact_end = 10 + len(weak) + 30 + len(q) - 1
        first, leave, _ = _check_pair(q, t, 4, s)
        assert first is None or first >= leave
        if s["ge_q_r"] == 1:                                          # (a dearer right end may prefer another alignment altogether)
            assert leave == exact_end
            assert first is not None and first >= exact_end


def test_fires_once_too_few_columns_are_left():
    """A criterion that never fires fails here.  Exact copies at the left end with a 200-column overhang, default scoring, R = 4, Q = 60.
    The top border binds: through (-1, t) a path scores at most -(t + 2) + (M + e) cols - e Q with cols = D - 1 - t, the alignment
    scores 2 Q - (off + 1) - (D - off - Q + 1), so the criterion holds from 4 cols < 4 Q - 1 on, i.e. with fewer than Q columns left.
    In columns of the last row that is c = t - 14 > D - 1 - Q - 14: the model fires with 71 .. 73 columns of the last row left on
    these inputs, i.e. within 130 columns of the leave column off + Q - 1.  Both numbers are what the model gives, not the kernel."""
    rng = random.Random(9)
    for off in (0, 15, 40):
        D = 60 + off + 200
        t = _rand(rng, D)
        q = t[off:off + 60]
        first, leave, _ = _check_pair(q, t, 4, DEFAULT)
        assert leave == off + 59
        assert first is not None and first - leave <= 130, (first, leave)
        assert 70 <= D - 1 - first <= 74, (first, D)


def test_row_bound_alone_never_fires():
    """with both ends pricing a terminal gap alike the bound that counts rows only keeps UB(top border) >= every score: it is inert"""
    rng = random.Random(10)
    t = _rand(rng, 260)
    q = t[:60]
    sch = Schedule(60, 4)
    H, En, htop, score, leave, margin, lv1s = _dp(q, t, DEFAULT)
    tabs = _plain_tables(sch, H, htop, DEFAULT)
    assert not any(_plain_criterion(sch, tabs, H, En, htop, 260, DEFAULT, t_, rows_only=True)[0] for t_ in range(sch.npos, 259))
    assert any(_plain_criterion(sch, tabs, H, En, htop, 260, DEFAULT, t_)[0] for t_ in range(sch.npos, 259))
