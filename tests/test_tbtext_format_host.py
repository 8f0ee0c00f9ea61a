"""No device: the CIGAR formatter the traceback epilogues and vsx_cigar_text_kernel share (vsearch_amd/csrc/vsx_tbtext.h:
vsx_cigar_ndigits, vsx_cigar_len, vsx_cigar_format), reached on the host through vsx_internal_cigar_format, against Python's str().

Run words are (length << 2) | op with op 0 = M, 1 = I, 2 = D, in traceback order (the last run of the text first).  The text is the
decimal length when it is above 1, the letter, a NUL, zero padding to a multiple of 4."""
import ctypes as C
import itertools

import numpy as np
import pytest

LENGTHS = (1, 2, 9, 10, 11, 99, 100, 999, 1000, 9999, 10000, 65535)
OPS = "MID"
GUARD = 0xA5


@pytest.fixture(scope="module")
def fmt():
    import __graft_entry__ as g
    g.build()
    from vsearch_amd import _lib
    lib = _lib.load()
    lib.vsx_internal_cigar_format.restype = C.c_uint32
    lib.vsx_internal_cigar_format.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]

    def run(runs_text_order, room=None):
        """[(length, op letter)] in text order -> (padded size the library reports, the bytes it wrote, the bytes behind them)"""
        words = np.array([(n << 2) | OPS.index(op) for n, op in reversed(runs_text_order)], np.uint32)
        want = "".join((str(n) if n > 1 else "") + op for n, op in runs_text_order)
        size = (len(want) + 1 + 3) & ~3
        buf = np.full((size if room is None else room) + 8, GUARD, np.uint8)      # (numpy allocations are at least 16-byte aligned)
        got = lib.vsx_internal_cigar_format(words.ctypes.data_as(C.c_void_p), len(words), buf.ctypes.data_as(C.c_void_p),
                                            size if room is None else room)
        return want, size, int(got), bytes(buf)

    return run


def _check(fmt, runs):
    want, size, got, buf = fmt(runs)
    assert got == size, (runs, got, size)
    assert buf[:size] == want.encode() + b"\0" * (size - len(want)), (runs, buf[:size], want)
    assert buf[size:] == bytes([GUARD]) * 8, f"{runs}: wrote past its {size} bytes"
    return want


@pytest.mark.parametrize("op", OPS)
def test_single_runs(fmt, op):
    """every digit count at both of its edges, for each operation; a count of 1 is omitted"""
    for n in LENGTHS:
        assert _check(fmt, [(n, op)]) == (op if n == 1 else f"{n}{op}")


def test_no_runs_and_one_run(fmt):
    """nruns = 0: the lone NUL in one zero dword; nruns = 1"""
    want, size, got, buf = fmt([])
    assert (want, size, got) == ("", 4, 4) and buf[:4] == b"\0\0\0\0" and buf[4:] == bytes([GUARD]) * 8
    assert _check(fmt, [(250, "M")]) == "250M"


def test_every_length_residue(fmt):
    """strings of 0 .. 24 bytes: every residue mod 4 several times, the NUL completing a dword (3, 7, ...) and opening one (4, 8, ...)"""
    seen = set()
    for nbytes in range(0, 25):
        runs, left, k = [], nbytes, 0
        while left:
            n = 12 if left >= 3 else (7 if left == 2 else 1)              # 3, 2 or 1 bytes of text
            runs.append((n, OPS[k % 3]))
            left -= len(str(n)) + 1 if n > 1 else 1
            k += 1
        want = _check(fmt, runs)
        assert len(want) == nbytes
        seen.add(nbytes % 4)
    assert seen == {0, 1, 2, 3}


def test_mixed_runs_in_text_order(fmt):
    """the words are in traceback order, the text runs left to right: all ordered triples of distinct lengths and operations"""
    for (a, b, c), ops in zip(itertools.permutations((1, 10, 65535, 2, 9999, 100), 3), itertools.cycle(itertools.permutations(OPS))):
        _check(fmt, [(a, ops[0]), (b, ops[1]), (c, ops[2])])
    assert _check(fmt, [(1030, "I"), (20, "M"), (1, "D"), (2, "I"), (1, "M")]) == "1030I20MD2IM"


def test_a_string_that_does_not_fit_is_not_written(fmt):
    want, size, got, buf = fmt([(10000, "I"), (8, "M")], room=8)            # "10000I8M" + NUL = 9 bytes -> 12
    assert got == 12 and buf == bytes([GUARD]) * 16
