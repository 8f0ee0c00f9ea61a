"""No device: the symbol maps and the hash finaliser every kernel and every host restatement share (vsearch_amd/csrc/vsx_symbols.h),
as the host compiles them, reached through vsx_internal_symbols: all 256 byte values of each map against the plain-Python models
the other tests carry, and mix64 against the generator of tests/sintax_data.py."""
import ctypes as C
import random

import numpy as np
import pytest

from tests import chimalns_data as ad
from tests import cut_data as cd
from tests import sintax_data as sx


@pytest.fixture(scope="module")
def symbols():
    import __graft_entry__ as g
    g.build()
    from vsearch_amd import _lib
    lib = _lib.load()
    lib.vsx_internal_symbols.restype = C.c_uint64
    lib.vsx_internal_symbols.argtypes = [C.c_void_p] * 4 + [C.c_uint64]

    def run(word=0):
        tables = [np.full(256 + 8, 0xA5, np.uint8) for _ in range(4)]
        mixed = lib.vsx_internal_symbols(*[t.ctypes.data_as(C.c_void_p) for t in tables], word)
        assert all(bytes(t[256:]) == b"\xa5" * 8 for t in tables), "wrote past a table's 256 bytes"
        return [t[:256] for t in tables], int(mixed)

    return run


def _letter(b):
    return chr(b).isascii() and chr(b).isalpha()


def test_code_of_every_byte(symbols):
    code = symbols()[0][0]
    for b in range(256):
        want = cd.code4(chr(b)) if b < 128 else 0
        assert code[b] == want, (b, code[b], want)
        assert code[b] == (ad.map4(chr(b)) if b < 128 else 0), b
        if not _letter(b):
            assert code[b] == 0, b
    assert {chr(b) for b in range(256) if code[b]} == set("ABCDGHKMNRSTUVWY" + "abcdghkmnrstuvwy")
    assert code[ord("U")] == code[ord("T")] == 8 and code[ord("n")] == 15


def test_ambiguous_of_every_code(symbols):
    (code, amb, _, _), _ = symbols()
    for b in range(256):
        assert amb[b] == (0 if b in (1, 2, 4, 8) else 1), b
    # by symbol: only A C G T U of either case are unambiguous
    assert {chr(b) for b in range(256) if not amb[code[b]]} == set("ACGTUacgtu")


def test_complement_of_every_byte(symbols):
    comp = symbols()[0][2]
    for b in range(256):
        want = cd.complement(chr(b)) if b < 128 else "N"
        assert chr(comp[b]) == want, (b, chr(comp[b]), want)
        if not _letter(b):
            assert comp[b] == ord("N"), b
    assert "".join(chr(comp[ord(c)]) for c in "ACGTUacgtuRYryXx") == "TGCAAtgcaaYRyrNN"
    assert sx.revcomp("AcgTnRx") == "".join(chr(comp[ord(c)]) for c in reversed("AcgTnRx"))


def test_upcase_of_every_byte(symbols):
    up = symbols()[0][3]
    for b in range(256):
        want = ad.upcase(chr(b)) if b < 128 else "N"
        assert chr(up[b]) == want, (b, chr(up[b]), want)
        if not _letter(b):
            assert up[b] == ord("N"), b


def _py_mix64(x):
    """tests/sintax_data.py's generator step is state += GAMMA, then the finaliser: start one step below x"""
    s = sx.Stream.__new__(sx.Stream)
    s.state = (x - sx.GAMMA) & sx.M64
    return s.next()


def test_mix64(symbols):
    rng = random.Random(2201)
    words = [0, 1, 1 << 63, (1 << 64) - 1] + [rng.getrandbits(64) for _ in range(64)]
    for x in words:
        assert symbols(x)[1] == _py_mix64(x), hex(x)
    # splitmix64 seeded with 0: its first output is the finaliser of the increment
    assert _py_mix64(0) == 0 and symbols(sx.GAMMA)[1] == 0xE220A8397B1DCDAF
