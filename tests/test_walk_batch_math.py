"""not gpu: the batched walk of the tilted traceback (walk() in vsx_traceback_tilt_kernel) against the one-cell walk, in
plain Python integers over direction-bit tiles in the kernel's own layout.

A trip of the batched walk reads WB dwords of bitsL -- the cell under the cursor and the next WB - 1 cells up the diagonal -- before it
uses any, applies backtrack16's five-way rule to the first and consumes the others for as long as each lies inside the tile and the pair
and has neither LEFT nor UP set (in M state the rule collapses to that test).  The model repeats the kernel's arithmetic: the dword index
and shift of every cell formed on its own (a diagonal crosses the HR boundary of the two-rows-per-register layout; the cells ahead use
the shorter virtual-row form, checked here against the plain one), a cell past the last admissible one re-reading that one, the count
taken as the trailing zeros of a stop mask.  Required: the same sequence of
(op, run length), the same exit cell and the same aligned / gap counts as the one-cell walk, for every start cell, every entry op, tiles
with bit patterns no DP produces, and no read outside bitsL."""
import random

import pytest

UP, EXT_UP, LEFT, EXT_LEFT = 1, 1 << 4, 1 << 16, 1 << 20


class Tile:
    """bitsL of one lane: [column slot 0 .. 16][group of four row pairs]; rows x and x + HR share a byte pair, the high half one slot on"""

    def __init__(self, RT, rng, density, junk):
        self.RT, self.HR = RT, (RT + 1) // 2
        self.NG = (self.HR + 3) // 4
        # words nobody recomputed hold whatever the tile before left there
        self.words = [rng.getrandbits(32) if junk else 0 for _ in range(17 * self.NG)]
        self.reads = 0
        for rv in range(RT):
            for cw in range(16):
                idx, sh = self.where(rv, cw)
                self.words[idx] &= ~((UP | EXT_UP | LEFT | EXT_LEFT) << sh) & 0xFFFFFFFF
                for bit, p in zip((UP, EXT_UP, LEFT, EXT_LEFT), density):
                    if rng.random() < p:
                        self.words[idx] |= bit << sh

    def where(self, rv, cw):
        up_half = rv >= self.HR
        rx = rv - self.HR if up_half else rv
        return (cw + (1 if up_half else 0)) * self.NG + (rx >> 2), (rx & 3) + (8 if up_half else 0)

    def where_v(self, rv, cw):
        """the same place through the virtual row v (cells 1 .. WB - 1 of a trip): v = row in the low half, 4 NG + row - HR in the high
        half; the dword is slot * NG + (v >> 2), bit 4 NG of v selects the byte"""
        assert self.NG <= 2
        v = rv + (4 * self.NG - self.HR) if (4 * self.NG != self.HR and rv >= self.HR) else rv
        return cw * self.NG + (v >> 2), (v & 3) | ((v & (4 * self.NG)) << (0 if self.NG == 2 else 1))

    def read(self, rv, cw, virtual=False):
        """the dword of a cell, shifted so that its UP bit is bit 0 (junk of the neighbouring rows above it)"""
        idx, sh = self.where_v(rv, cw) if virtual else self.where(rv, cw)
        assert (idx, sh) == self.where(rv, cw)
        assert 0 <= rv < self.RT and 0 <= cw < 16 and 0 <= idx < len(self.words), ("read outside the tile", rv, cw)
        self.reads += 1
        return self.words[idx] >> sh


class Cursor:
    def __init__(self, r, j, i, op):
        self.r, self.j, self.i, self.op = r, j, i, op
        self.runlen = 0 if op < 0 else 3
        self.al, self.ga, self.runs, self.trips = 0, 0, [], 0

    def result(self):
        return (self.runs + [(self.op, self.runlen)], (self.r, self.j, self.i), self.al, self.ga)


def _cell0(t, c, r0h, cst):
    """the rule of one cell as the kernel writes it; returns whether the move was diagonal"""
    w = t.read(c.r - r0h, c.j - cst)
    c.al += 1
    inI, inD = int(c.op == 1), int(c.op == 2)
    c1 = inI & (w >> 20)
    c2 = (c1 ^ 1) & inD & (w >> 4)
    c12 = c1 | c2
    c3 = (c12 ^ 1) & (w >> 16)
    c4 = ((c12 | c3) ^ 1) & w
    isI, isD = (c1 | c3) & 1, (c2 | c4) & 1
    newop = isI + 2 * isD
    c.ga += ((c3 & (inI ^ 1)) | (c4 & (inD ^ 1))) & 1
    c.j -= isD ^ 1
    c.i -= isI ^ 1
    c.r -= isI ^ 1
    if newop != c.op:
        if c.op >= 0:
            c.runs.append((c.op, c.runlen))
        c.op, c.runlen = newop, 0
    c.runlen += 1
    return newop == 0


def walk_one(t, c, r0h, cst):
    while c.r >= r0h and c.j >= cst and c.i >= 0:
        c.trips += 1
        _cell0(t, c, r0h, cst)


def walk_batch(t, c, r0h, cst, WB):
    while c.r >= r0h and c.j >= cst and c.i >= 0:
        c.trips += 1
        rv, cw = c.r - r0h, c.j - cst
        kmax = min(rv, cw, c.i, WB - 1)
        # all reads before the first use; a cell past kmax re-reads cell kmax (inside the tile) and is masked by bit kmax
        ahead = [t.read(rv - min(k, kmax), cw - min(k, kmax), virtual=True) for k in range(1, WB)]
        diag = _cell0(t, c, r0h, cst)
        stop = 0
        for k, x in enumerate(ahead, start=1):
            stop |= ((x & 0x00010001) << (k - 1)) & 0xFFFFFFFF            # bit k - 1: UP, bit 16 + k - 1: LEFT
        stop |= (stop >> 16) | (1 << kmax)                                # what stays in bits 16 .. lies above bit kmax
        nd = ((stop & -stop).bit_length() - 1) if diag else 0          # count of trailing zeros
        assert nd <= kmax
        c.al += nd
        c.runlen += nd
        c.i -= nd
        c.r -= nd
        c.j -= nd


# tile rows of the classes the kernel is built for: R = 10, 14, 16, 20 MID (10), 26 MID (13: odd, the junk row), R = 12 or 24 (HR = 6) and the smallest, R = 4
TILES = [10, 14, 16, 13, 12, 4]
# (UP, EXT_UP, LEFT, EXT_LEFT): like a DP at 90 % identity; gap-rich; every bit a coin flip (no DP sets EXT without a way to use it)
DENSITIES = [(0.04, 0.02, 0.04, 0.02), (0.25, 0.3, 0.25, 0.3), (0.5, 0.5, 0.5, 0.5), (0.0, 1.0, 0.0, 1.0), (0.0, 0.0, 0.0, 0.0)]


@pytest.mark.parametrize("RT", TILES)
@pytest.mark.parametrize("dens", range(len(DENSITIES)))
def test_batched_walk_equals_one_cell_walk(RT, dens):
    rng = random.Random(1000 * RT + dens)
    fewer = 0
    for rep in range(1):
        t = Tile(RT, rng, DENSITIES[dens], junk=True)
        # r0h, cst: a MID tile's second half and a tile away from column 0; ibase: i - r, below zero over the dummy rows of position 0
        for (r0h, cst, ibase) in ((0, 0, 0), (RT, 37, 5 * RT), (0, 16, -(RT // 2)), (0, 0, -(RT - 1))):
            for rv in range(RT):
                for cw in range(16):
                    for op in (-1, 0, 1, 2):
                        start = (r0h + rv, cst + cw, r0h + rv + ibase, op)
                        if start[2] < 0:
                            continue
                        ref = Cursor(*start)
                        walk_one(t, ref, r0h, cst)
                        for WB in (2, 4, 8):
                            c = Cursor(*start)
                            walk_batch(t, c, r0h, cst, WB)
                            assert c.result() == ref.result(), (RT, dens, r0h, cst, ibase, rv, cw, op, WB)
                            assert c.trips <= ref.trips
                            fewer += ref.trips - c.trips
    if dens != 2 and dens != 1:
        assert fewer > 0


def test_wb1_is_the_one_cell_walk():
    rng = random.Random(7)
    t = Tile(16, rng, DENSITIES[0], junk=True)
    for rv in range(16):
        for cw in range(16):
            a, b = Cursor(rv, cw, rv, -1), Cursor(rv, cw, rv, -1)
            walk_one(t, a, 0, 0)
            before = t.reads
            walk_batch(t, b, 0, 0, 1)
            assert a.result() == b.result() and a.trips == b.trips and t.reads - before == b.trips


def test_a_clean_diagonal_takes_one_trip_per_wb_cells():
    rng = random.Random(8)
    t = Tile(16, rng, DENSITIES[4], junk=False)
    for WB in (2, 4, 8):
        c = Cursor(15, 15, 15, 0)
        walk_batch(t, c, 0, 0, WB)
        assert c.trips == 16 // WB and c.result() == ([(0, 19)], (-1, -1, -1), 16, 0)
        # the pair ends inside the batch: i reaches -1 after three cells
        c = Cursor(15, 15, 2, 0)
        walk_batch(t, c, 0, 0, WB)
        assert c.result() == ([(0, 6)], (12, 12, -1), 3, 0)
