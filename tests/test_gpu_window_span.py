"""The span-capacity break of the window planner (vsearch_amd/csrc/vsx_window.h), through every command that plans its windows by
span: vsx_fastx_filter with one side and with two, vsx_fastq_eestats, vsx_fastq_stats and vsx_fastq_chars.

Four reads of 100 symbols lie at offsets 0, 9 MiB, 18 MiB and 27 MiB of blobs of 27 MiB + 100 bytes, junk everywhere else (0x7f
in the quality blob, out of range under every offset; `*` in the sequence blob).  With window=0 nothing but the 16 MiB capacity
closes a window: reads 0 and 1 span 9 MiB + 100 bytes, read 2 would make it 18 MiB + 100, so the call takes 2 windows -- in
ascending and in descending order of the offsets alike -- and every output equals the host route's for the same call.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from tests import eestats_data as ed
from tests import fastq_filter_data as ff
from tests import fastq_stats_data as fs

pytestmark = pytest.mark.gpu

MIB = 1 << 20
OFFSETS = np.array([0, 9 * MIB, 18 * MIB, 27 * MIB], np.uint64)
READ = 100
BLOB_BYTES = 27 * MIB + READ
ORDERS = {"ascending": [0, 1, 2, 3], "descending": [3, 2, 1, 0]}


@pytest.fixture(scope="module")
def aligner(gpu_required):
    from vsearch_amd import Aligner
    with Aligner(device=0) as al:
        yield al


@contextlib.contextmanager
def host_route(variable):
    old = os.environ.get(variable)
    os.environ[variable] = "host"
    try:
        yield
    finally:
        if old is None:
            del os.environ[variable]
        else:
            os.environ[variable] = old


def full_length(s, sides=("quals",)):
    """the first four reads of a generated set that have READ symbols on every side"""
    picked = [k for k in range(len(s[sides[0]])) if all(len(s[side][k]) == READ for side in sides)][:4]
    assert len(picked) == 4, s["name"]
    return picked


_BLOBS = {}


def blob(texts, junk):
    """the four texts at OFFSETS of a blob of BLOB_BYTES, `junk` between them (built once per content)"""
    key = (tuple(texts), junk)
    if key not in _BLOBS:
        b = bytearray(junk * BLOB_BYTES)
        for text, off in zip(texts, OFFSETS):
            assert len(text) == READ
            b[int(off):int(off) + READ] = text.encode()
        _BLOBS[key] = bytes(b)
    return _BLOBS[key]


def layout(order):
    """read k of the call is the one at OFFSETS[order[k]]"""
    return OFFSETS[order].copy(), np.full(4, READ, np.uint32)


def filter_call(aligner, s, picked, order, **extra):
    """vsx_fastx_filter over the blobs -> (records, rev_records or None, pair_discarded, totals, stats)"""
    from vsearch_amd import _lib
    from vsearch_amd.filter import _records, default_opts, last_stats
    lib = _lib.load()
    off, lens = layout(order)
    raw = lambda b: C.cast(C.c_char_p(b), C.c_void_p)      # noqa: E731

    def side(seqs, quals):
        sb, qb = blob([seqs[k] for k in picked], b"*"), blob([quals[k] for k in picked], b"\x7f")
        return _lib.FilterReads(raw(sb), raw(qb), len(sb), off.ctypes.data, lens.ctypes.data, None)

    fwd = side(s["seqs"], s["quals"])
    rev = side(s["rev_seqs"], s["rev_quals"]) if s.get("rev_seqs") is not None else None
    out = _lib.FilterOut()
    o = default_opts(**dict(s["opts"], **extra))
    _lib.check(lib.vsx_fastx_filter(aligner.h if aligner is not None else None, C.byref(o), C.c_uint64(4), C.byref(fwd),
                                    C.byref(rev) if rev is not None else None, C.byref(out)), "vsx_fastx_filter")
    try:
        return (_records(out.fwd, 4), _records(out.rev, 4) if rev is not None else None,
                np.ctypeslib.as_array(out.pair_discarded, shape=(4,)).copy(),
                (int(out.kept), int(out.kept_truncated), int(out.discarded)), last_stats())
    finally:
        lib.vsx_fastx_filter_out_free(C.byref(out))


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("paired", [False, True])
def test_filter_closes_the_window_at_the_capacity(aligner, paired, order):
    s = ff.generate(22 if paired else 21, 40, read_len=READ, paired=paired)
    picked = full_length(s, ("seqs", "quals", "rev_seqs", "rev_quals") if paired else ("seqs", "quals"))
    dev = filter_call(aligner, s, picked, ORDERS[order], window=0)
    with host_route("VSX_FILTER"):
        host = filter_call(None, s, picked, ORDERS[order], window=0)
    assert dev[4]["windows"] == 2 and dev[4]["reads_host"] == 0
    assert host[4]["reads_host"] == host[4]["reads"] == (8 if paired else 4)
    assert (dev[1] is not None) == (host[1] is not None) == paired
    for x, y in ((dev[0], host[0]), (dev[1], host[1])):
        if x is not None:
            assert x.tobytes() == y.tobytes()
    assert dev[2].tolist() == host[2].tolist() and dev[3] == host[3]


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_eestats_closes_the_window_at_the_capacity(aligner, order):
    from vsearch_amd.eestats import stats_of_blob
    s = ed.generate(77, 100, read_len=READ)
    qb = blob([s["quals"][k] for k in full_length(s)], b"\x7f")
    off, lens = layout(ORDERS[order])
    dev = stats_of_blob(aligner, qb, off, lens, **dict(s["opts"], window=0))
    with host_route("VSX_EESTATS"):
        host = stats_of_blob(None, qb, off, lens, **dict(s["opts"], window=0))
    assert dev.stats["windows"] == 2 and dev.stats["reads_host"] == 0
    assert host.stats["reads_host"] == host.stats["reads"] == 4
    ed.assert_same_tables(dev, host, f"eestats {order}")


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("command", fs.BOTH)
def test_fastq_stats_and_chars_close_the_window_at_the_capacity(aligner, command, order):
    from vsearch_amd.fastq_stats import chars_of_blob, stats_of_blob
    s = fs.generate(77, 100, read_len=READ)
    picked = full_length(s, ("seqs", "quals"))
    sb, qb = blob([s["seqs"][k] for k in picked], b"*"), blob([s["quals"][k] for k in picked], b"\x7f")
    off, lens = layout(ORDERS[order])

    def call(al):
        if command == "stats":
            return stats_of_blob(al, qb, off, lens, **dict(s["opts"], window=0))
        return chars_of_blob(al, sb, qb, off, lens, tail=s["tail"], window=0)

    dev = call(aligner)
    with host_route("VSX_FASTQ_STATS"):
        host = call(None)
    assert dev.stats["windows"] == 2 and dev.stats["reads_host"] == 0
    assert host.stats["reads_host"] == host.stats["reads"] == 4
    fs.assert_same_tables(dev, host, f"{command} {order}")
