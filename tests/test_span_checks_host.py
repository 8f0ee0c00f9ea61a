"""No device: "does span k lie inside the blob" (vsxp::check_spans, vsearch_amd/csrc/vsx_private.h) through the commands that take
the host route without a context.  A blob of 16 bytes and two spans, the first always legal: an offset near 2^64 whose sum with the
length wraps to 4 is refused, an empty span at the very end is accepted, a span one byte too long is refused.  The formerly wrapping
checks need a searcher: tests/test_gpu_search.py, test_gpu_chimera.py and test_gpu_chimalns.py carry the first case for them."""
import ctypes as C

import numpy as np
import pytest

from vsearch_amd import _lib

BLOB = b"ACGAATTCGTACGTAC"
WRAPS = ((1 << 64) - 4, 8)           # offset + length = 4 (mod 2^64)
AT_END = (16, 0)
ONE_PAST = (9, 8)


def _cut(span):
    lib = _lib.load()
    o = _lib.CutOpts()
    lib.vsx_cut_opts_default(C.byref(o))
    pattern = b"G^AATT_C"
    o.pattern, o.pattern_len = pattern, len(pattern)
    off, lens = np.array([0, span[0]], np.uint64), np.array([4, span[1]], np.uint32)
    res = _lib.CutOut()
    rc = lib.vsx_cut(None, C.byref(o), 2, C.cast(C.c_char_p(BLOB), C.c_void_p), len(BLOB), off.ctypes.data_as(C.c_void_p),
                     lens.ctypes.data_as(C.c_void_p), C.byref(res))
    if rc == 0:
        lib.vsx_cut_out_free(C.byref(res))
    return rc, lib.vsx_last_error().decode()


def _sortby(span):
    lib = _lib.load()
    o = _lib.SortbyOpts()
    lib.vsx_sortby_opts_default(C.byref(o))
    arrays = [np.array([0, span[0]], np.uint64), np.array([4, span[1]], np.uint32), np.array([5, 5], np.uint32), np.array([1, 2], np.uint32)]
    res = _lib.SortbyOut()
    rc = lib.vsx_sortby(None, C.byref(o), 2, C.cast(C.c_char_p(BLOB), C.c_void_p), len(BLOB), *[a.ctypes.data_as(C.c_void_p) for a in arrays],
                        C.byref(res))
    if rc == 0:
        lib.vsx_sortby_out_free(C.byref(res))
    return rc, lib.vsx_last_error().decode()


def _fastx_mask(span):
    lib = _lib.load()
    o = _lib.MaskOpts()
    lib.vsx_fastx_mask_opts_default(C.byref(o))
    off, lens = np.array([0, span[0]], np.uint64), np.array([4, span[1]], np.uint32)
    res = _lib.MaskOut()
    rc = lib.vsx_fastx_mask(None, C.byref(o), 2, C.cast(C.c_char_p(BLOB), C.c_void_p), len(BLOB), off.ctypes.data_as(C.c_void_p),
                            lens.ctypes.data_as(C.c_void_p), C.byref(res))
    if rc == 0:
        lib.vsx_fastx_mask_out_free(C.byref(res))
    return rc, lib.vsx_last_error().decode()


@pytest.mark.parametrize("call, text", [(_cut, "vsx_cut: a sequence exceeds the blob"), (_sortby, "vsx_sortby: a header exceeds the blob"),
                                        (_fastx_mask, "vsx_fastx_mask: a sequence exceeds the blob")])
def test_spans_are_checked_without_adding(call, text, monkeypatch):
    monkeypatch.setenv("VSX_MASK", "host")               # (vsx_fastx_mask takes no null context otherwise)
    assert call(WRAPS) == (_lib.VSX_EINVAL, text)
    assert call(AT_END)[0] == 0
    assert call(ONE_PAST) == (_lib.VSX_EINVAL, text)
    assert call((9, 7))[0] == 0                          # ... and the same span a byte shorter ends with the blob
