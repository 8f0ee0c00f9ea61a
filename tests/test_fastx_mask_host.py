"""Sequence masking without a GPU: the library's host restatement (VSX_MASK=host) against the plain-Python restatement of
tests/fastx_mask_data.py field for field, the writers against the reference's recorded text, the ABI surface and its refusals, and
the assertions that the input sets reach the cases they are named after (computed from py_fastx_mask()'s own window functions).
"""
import ctypes as C
import random

import numpy as np
import pytest

from tests import fastx_mask_data as md
from vsearch_amd import _lib
from vsearch_amd import mask as mk


@pytest.fixture(scope="module")
def sets():
    return md.all_sets()


@pytest.fixture(scope="module")
def chains(sets):
    """the windows the reference's loop visits, per sequence of the DUST sets that steer the chain"""
    out = {}
    for s in sets:
        if s["name"] in ("lengths", "windows", "segments"):
            out[s["name"]] = [md.py_windows(x) for x in s["seqs"]]
    return out


# ---- host restatement == plain Python ------------------------------------------------------------------------------------------
def test_host_equals_python_on_every_set(sets):
    for s in sets:
        md.assert_equals_py(md.call(None, s), s)


def test_host_equals_python_on_random_sequences():
    rng = random.Random(1911)
    seqs = [md.island_seq(rng, rng.randint(0, 130), alphabet="ACGTacgtNnRYUu", lower=0.2) for _ in range(2000)]
    for k, (qmask, hard) in enumerate(md.MODES):
        part = seqs if qmask == "dust" and not hard else seqs[k * 300:(k + 1) * 300]
        s = md._set(f"random_{qmask}_{hard}", part, dict(qmask=qmask, hardmask=hard, min_unmasked_pct=30.0, max_unmasked_pct=85.0))
        res = md.call(None, s)
        md.assert_equals_py(res, s)
        assert res.stats["sequences_host_forced"] == len(part) and res.stats["sequences"] == len(part)
    assert min(res.discarded_less, res.discarded_more, res.kept) > 0


def test_bits_count_what_unmasked_leaves(sets):
    for s in sets:
        res = md.call(None, s)
        bits = res.bits()
        for k in range(res.n):
            a, b = int(res.offsets[k]), int(res.offsets[k + 1])
            assert int(bits[a:b].sum()) == b - a - int(res.unmasked[k]), (s["name"], k)


def test_want_bits_alone_and_windows(sets):
    s = next(x for x in sets if x["name"] == "fastq")
    full = md.call(None, s)
    for want_text, want_bits in ((True, False), (False, True), (False, False)):
        part = md.call(None, s, want_text=want_text, want_bits=want_bits)
        assert (part.text_blob is None) == (not want_text) and (part.bits_blob is None) == (not want_bits)
        md.assert_same(full, part, (want_text, want_bits))
    assert md.call(None, s, window=7).tobytes() == full.tobytes()


def test_scattered_and_reversed_offsets(sets):
    s = next(x for x in sets if x["name"] == "fastq")
    full = md.call(None, s)
    rng = random.Random(5)
    blob, off = b"", []
    for x in reversed(s["seqs"]):
        blob += b"#" * rng.randint(0, 9)
        off.append(len(blob))
        blob += x.encode()
    off = np.array(off[::-1], np.uint64)
    lens = np.array([len(x) for x in s["seqs"]], np.uint32)
    res = mk.fastx_mask_host((blob, off, lens), **md.mask_kw(s))
    assert res.tobytes() == full.tobytes()


# ---- the writers ---------------------------------------------------------------------------------------------------------------
def test_writers_equal_golden():
    for s in md.load_golden():
        md.assert_text_equals_golden(md.call(None, s), s)


def test_log_lines_appear_only_with_their_option():
    res = md.call(None, md.empty_set())
    assert mk.log_lines(res) == ["%d sequences kept" % res.kept]
    assert len(mk.log_lines(res, 10.0, 100.0)) == 2 and len(mk.log_lines(res, 10.0, 90.0)) == 3


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def _raw(opts_edit=None, handle=None, blob=b"ACGTACGT", off=(0,), lens=(8,), host=True, monkeypatch=None):
    lib = _lib.load()
    o = _lib.MaskOpts()
    lib.vsx_fastx_mask_opts_default(C.byref(o))
    if opts_edit:
        opts_edit(o)
    off, lens = np.array(off, np.uint64), np.array(lens, np.uint32)
    res = _lib.MaskOut()
    rc = lib.vsx_fastx_mask(handle, C.byref(o), len(lens), C.cast(C.c_char_p(blob), C.c_void_p), len(blob), off.ctypes.data_as(C.c_void_p),
                            lens.ctypes.data_as(C.c_void_p), C.byref(res))
    if rc == 0:
        lib.vsx_fastx_mask_out_free(C.byref(res))
    return rc


def test_symbols_and_defaults():
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in _lib.MASK_SYMBOLS)
    o = _lib.MaskOpts()
    lib.vsx_fastx_mask_opts_default(C.byref(o))
    assert (o.qmask, o.hardmask, o.min_unmasked_pct, o.max_unmasked_pct, o.want, o.window) == (2, 0, 0.0, 100.0, 3, 0)


def test_refusals(monkeypatch):
    monkeypatch.delenv("VSX_MASK", raising=False)
    assert _raw() == _lib.VSX_EINVAL                                        # no context and no VSX_MASK=host
    monkeypatch.setenv("VSX_MASK", "host")
    assert _raw() == 0

    def edit(**kw):
        def f(o):
            for k, v in kw.items():
                setattr(o, k, v)
        return f
    for kw in (dict(min_unmasked_pct=-0.1), dict(min_unmasked_pct=100.1), dict(max_unmasked_pct=-1.0), dict(max_unmasked_pct=100.5),
               dict(min_unmasked_pct=60.0, max_unmasked_pct=59.9), dict(min_unmasked_pct=float("nan")), dict(qmask=3), dict(qmask=-1),
               dict(hardmask=2), dict(want=4), dict(window=-1)):
        assert _raw(edit(**kw)) == _lib.VSX_EINVAL, kw
    assert _raw(edit(min_unmasked_pct=60.0, max_unmasked_pct=60.0)) == 0
    assert _raw(off=(4,), lens=(5,)) == _lib.VSX_EINVAL                     # beyond the blob
    assert _raw(off=(0, 3), lens=(4, 4)) == _lib.VSX_EINVAL                 # two sequences share a byte
    assert _raw(off=(4, 0), lens=(4, 5)) == _lib.VSX_EINVAL                 # ... in any order
    assert _raw(off=(4, 0), lens=(4, 4)) == 0
    assert _raw(off=(3, 3, 3), lens=(0, 2, 0)) == 0                         # an empty sequence shares nothing


# ---- the sets reach their cases ------------------------------------------------------------------------------------------------
def test_lengths_are_covered(sets):
    lens = {len(x) for s in sets for x in s["seqs"]}
    assert {0, 1, 7, 8, 9, 63, 64, 65, 95, 96, 97} <= lens
    assert set(md.SEGMENT_LENGTHS) <= lens and all(n % 64 in (63, 0, 1) for n in md.SEGMENT_LENGTHS)


def test_window_cases_are_reached(chains):
    masked = [(i, v, a, b) for name in chains for ch in chains[name] for (i, v, a, b) in ch if v > md.LEVEL]
    assert {7, 31, 32} <= {b for _, _, _, b in masked}
    assert min(b for _, _, _, b in masked) == 7                             # the step bound the long route's 64 entry offsets rest on
    steps = {32 + (32 - b if b < 32 else 0) for _, _, _, b in masked}
    assert max(steps) == md.MAX_STEP and 33 in steps and 32 in steps
    # a final window shorter than 8: visited, and too short to hold a region
    seqs = next(s for s in md.all_sets() if s["name"] == "windows")["seqs"]
    assert any(0 < len(x) - ch[-1][0] < 8 for x, ch in zip(seqs, chains["windows"]))


def test_mode_inputs_hold_every_symbol_class(sets):
    text = "".join(md.MODE_SEQS)
    for c in "NnUuRYKMrykm":
        assert c in text
    assert any(c.islower() for c in text) and any(c in "BDHV" for c in text)
    by = {s["name"]: md.py_fastx_mask(s["seqs"], **md.mask_kw(s)) for s in sets if s["name"].startswith("modes_")}
    assert set(by) == {f"modes_{q}_{h}" for q, h in md.MODES}
    seqs = md.MODE_SEQS
    assert by["modes_none_0"]["text"] == seqs and by["modes_soft_0"]["text"] == seqs
    assert by["modes_none_0"]["unmasked"] == [len(x) for x in seqs]
    # an input N counts as masked under hardmask; a lower-case n outside any interval counts as unmasked under dust + hardmask
    hard = by["modes_dust_1"]
    assert hard["text"][1].startswith("nnnnn") and not any(hard["bits"][len(seqs[0]):len(seqs[0]) + 5])
    k = len(seqs[0]) + seqs[1].index("NNNNN")
    assert all(hard["bits"][k:k + 5])
    assert all(c == "N" for c in by["modes_soft_1"]["text"][1][:5])          # soft + hardmask: 'n' has bit 0x20
    # dust without hardmask: lower-case input comes out upper-case outside the intervals
    soft = by["modes_dust_0"]["text"][2]
    assert soft[:8] == seqs[2][:8].upper() and "a" * 10 in soft
    # U = T for the words: a run of u is low complexity
    assert "u" * 10 in by["modes_dust_0"]["text"][1].replace("U", "u")[0:] and "N" * 10 in hard["text"][1]


def test_percentages_sit_on_and_beside_the_limits(sets):
    s = next(x for x in sets if x["name"] == "percent")
    exp = md.py_fastx_mask(s["seqs"], **md.mask_kw(s))
    pct = [100.0 * u / len(x) for u, x in zip(exp["unmasked"], s["seqs"])]
    assert pct[:4] == [25.0, 75.0, 12.5, 87.5] and exp["verdict"][:4] == [0, 0, 1, 2]
    e = md.py_fastx_mask(md.empty_set()["seqs"], **md.mask_kw(md.empty_set()))
    assert e["verdict"][0] == 0 and e["verdict"][2] == 0                    # NaN fails both comparisons


def test_union_of_all_windows_differs_from_the_chain(sets):
    """an implementation that applied the windows off the chain would mask more"""
    seq = next(s for s in sets if s["name"] == "fastq")["seqs"]
    differ = 0
    for x in seq[:6]:
        chain, union = set(), set()
        for i, v, a, b in md.py_windows(x):
            if v > md.LEVEL:
                chain |= set(range(i + a, i + b + 1))
        for i in range(len(x)):
            v, a, b = md.py_window(x, i)
            if v > md.LEVEL:
                union |= set(range(i + a, i + b + 1))
        assert chain <= union
        differ += chain != union
    assert differ > 0


def test_chain_shifts_phase_against_the_segment_grid(sets, chains):
    s = next(x for x in sets if x["name"] == "segments")
    chain = [i for i, _, _, _ in chains["segments"][-1]]                    # phase_seq()
    assert chain[:4] == [0, 57, 114, 171]
    offsets = [i % 64 for i in chain]
    assert len(set(offsets)) == 64                                          # every phase of a 64-grid
    # a step that lands on a segment's first position, on its last, and the entries 0, 1 and the largest there is (63 + 57 - 64)
    entries = {}
    for p, q in zip(chain, chain[1:]):
        if q // 64 != p // 64:
            entries.setdefault(q % 64, []).append(p % 64)
    assert {0, 1, 56} <= set(entries) and 63 in entries[56] and max(entries) == 56
    assert 63 in offsets and 0 in offsets[1:]
    assert len(s["seqs"][-1]) > 64 * 57
