"""not gpu: the leave-column rule of the DP kernel's steady loop (vsx_forward_kernel), checked in plain Python integers.

Along the last query row the kernel keeps lv1 = the column of the first cell (scanning left) where an 'I' run does not continue:
lv1(j) = cont(j) ? lv1(j - 1) : j, per 16-bit half of a VGPR, starting from 0xFFFF.  Lane l works on column j = t - l at step t.
The steady loop tracks lv1 + l (wrapping per half) instead and selects the wave-uniform step t, so no per-lane column is formed per
step; the loop converts on entry (+ l) and on exit (- l).  The test requires the same lv1 after every step, on random cont sequences,
phase boundaries and lane skews, and that a half the select never fires in keeps its start value, 0xFFFF included."""
import random

import pytest

M16 = 0xFFFF


def _pack(lo, hi):
    return (lo & M16) | ((hi & M16) << 16)


def _halves(x):
    return x & M16, x >> 16


def _padd(a, b):
    (a0, a1), (b0, b1) = _halves(a), _halves(b)
    return _pack(a0 + b0, a1 + b1)


def _psub(a, b):
    (a0, a1), (b0, b1) = _halves(a), _halves(b)
    return _pack(a0 - b0, a1 - b1)


def _bfi(mask, a, b):
    return (a & mask) | (b & ~mask & 0xFFFFFFFF)


def _cont_mask(c0, c1):
    # v_pk_ashrrev_i16 15 of the ext-left difference: 0xFFFF in a half where cont is true
    return _pack(M16 if c0 else 0, M16 if c1 else 0)


def _per_step(lv1, l, t0, conts):
    """the per-step form (fill and phase B): select the column j = t - l."""
    for k, (c0, c1) in enumerate(conts):
        j = t0 + k - l
        lv1 = _bfi(_cont_mask(c0, c1), lv1, _pack(j, j))
    return lv1


def _steady(lv1, l, t0, conts):
    """the steady loop's form: lv1 + l on entry, select the step t, - l on exit."""
    lpk = _pack(l, l)
    lvt = _psub(lv1, _psub(0, lpk))
    for k, (c0, c1) in enumerate(conts):
        t = t0 + k
        lvt = _bfi(_cont_mask(c0, c1), lvt, (t * 0x00010001) & 0xFFFFFFFF)
    return _psub(lvt, lpk)


@pytest.mark.parametrize("seed", range(8))
def test_steady_leave_tracking_matches_per_step_select(seed):
    rng = random.Random(seed)
    for _ in range(400):
        l = rng.randrange(16)
        t0 = 16 * rng.randrange(1, 64)                 # the steady loop starts at a block boundary, t >= 16 > l
        n = rng.randrange(0, 80)
        p = rng.random()                              # density of cont (long runs and none at all)
        conts = [(rng.random() < p, rng.random() < p) for _ in range(n)]
        start = rng.choice([0xFFFFFFFF, _pack(rng.randrange(t0 - l), rng.randrange(t0 - l)), _pack(M16, rng.randrange(t0 - l))])
        assert _steady(start, l, t0, conts) == _per_step(start, l, t0, conts)


def test_untouched_halves_keep_their_start_value():
    for l in range(16):
        conts = [(True, True)] * 37
        assert _steady(0xFFFFFFFF, l, 16, conts) == 0xFFFFFFFF
        assert _steady(_pack(5, M16), l, 48, conts) == _pack(5, M16)


def test_halves_are_independent():
    # cont false in one half only: that half takes the last such column, the other keeps its value
    l, t0 = 7, 32
    conts = [(k != 11, True) for k in range(20)]
    lo, hi = _halves(_steady(0xFFFFFFFF, l, t0, conts))
    assert lo == t0 + 11 - l and hi == M16
