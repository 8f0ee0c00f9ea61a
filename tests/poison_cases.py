"""Poisoned-memory parity: the cases of tests/test_gpu_poison.py and the child-process driver that runs them.

The rule under test: a result is bit-identical whatever the bytes hold that nobody wrote, and equal to the CPU reference.  The library
reuses device memory on purpose (scratch pool, the checkpoint block and traceback slab the plans of a context share, grow-only window
buffers), so a forgotten memset or a read of a slot its producer skipped shows only in a process with a history.  Two levers:

  VSX_POISON / VSX_POISON_BYTE   the library fills every block it hands out, and every chunk's part of the shared blocks, with the byte
                                 (vsx_private.h); the driver is started once per setting by the test
  history                        every case runs on a fresh handle and again on a handle that has just finished a larger call of
                                 another shape, whose buffers the case then reuses; the two digests must agree inside the child

A case builds its input from the data modules of the suite, runs the device path, asserts that the device path was taken, and returns
its result as named byte sections in an order-insensitive form; the digest is a SHA-256 over them.  reference() gives the same sections
from the CPU reference of the command's own tests (the oracle, the library's host routes, the py_*() restatements, the goldens).
Where that reference sits behind a device search (the chimera commands' VSX_CHIMERA=host, allpairs' blocks) the case says so
(device_reference) and the driver computes it in the child.

    python -m tests.poison_cases --out FILE [--case NAME ...] [--verify]

writes one JSON object, case -> {digest, digest_history, digest_reference, seconds, error}, rewritten after every case, plus "_poison_byte": the hook as
the child's library sees it.  --verify also computes the reference in the child and names the first section that differs.  A case
whose error names a GPU fault ends the driver at once with status 3: nothing more is started on a faulted device.
"""
import argparse
import contextlib
import hashlib
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import common  # noqa: E402
from tests.aligner_data import accept_py, torture_pairs  # noqa: E402

CASES = {}


def digest(sections):
    """SHA-256 over named byte sections [(name, bytes), ...]"""
    h = hashlib.sha256()
    for name, data in sections:
        data = bytes(data)
        h.update(f"{name}:{len(data)}\n".encode())
        h.update(data)
    return h.hexdigest()


def first_difference(a, b):
    """name of the first section in which two results differ, or None"""
    if [n for n, _ in a] != [n for n, _ in b]:
        return "section names: %r != %r" % ([n for n, _ in a][:8], [n for n, _ in b][:8])
    for (n, x), (_, y) in zip(a, b):
        if bytes(x) != bytes(y):
            return n
    return None


class Case:
    """name; build() -> input (built once per process); reference(inp) and device(inp, history) -> sections;
    sizes(inp) -> ((reads, bytes) of the case input, (reads, bytes) of the history input)"""
    name = None
    _inp = None
    device_reference = False        # True: reference() needs a device (the driver computes it in the child)

    def build(self):
        raise NotImplementedError

    def input(self):
        if self._inp is None:
            self._inp = self.build()
        return self._inp

    def reference(self, inp):
        raise NotImplementedError

    def device(self, inp, history):
        raise NotImplementedError

    def sizes(self, inp):
        raise NotImplementedError


def register(cls):
    CASES[cls.name] = cls()
    return cls


def oracle():
    from oracle import pyoracle
    pyoracle.build(ref=True)
    return pyoracle.Oracle()


def scoring(name):
    sc = common.load_golden()["scorings"][name]
    return tuple(sc["P"]), bool(sc["n_mismatch"])


def rows_sections(tag, rows):
    """result rows (score, aligned, matches, mismatches, gaps, cigar) in pair order -> sections"""
    cols = list(zip(*rows)) if rows else [[]] * 6
    out = [(f"{tag}.score", np.array(cols[0], np.int16).tobytes())]
    for k, f in enumerate(("aligned", "matches", "mismatches", "gaps")):
        out.append((f"{tag}.{f}", np.array(cols[k + 1], np.uint16).tobytes()))
    out.append((f"{tag}.cigar", "\n".join(cols[5]).encode()))
    return out


def result_rows(res):
    return [res.row(k) for k in range(len(res))]


# ---- the aligner (vsx_device.hip, vsx_tbtext.hip, vsx_rank.hip) -------------------------------------------------------------------

def tilt_reach(P, Q, D):
    """the planner's bound (vsx_plan.cpp tilt_possible()), as tests/test_gpu_parity.py states it"""
    B = max(abs(P[0]), abs(P[1]), *P[8:14])
    G = max(P[2:8])
    return 4 * G + 2 * (Q + ((D + 3) & ~3) + 64) * B


_ALIGNER_HISTORY = None


def aligner_history():
    """the larger call of another shape: 128 queries of ~330 (row class 22) against 24 family members of ~900 each, 3 072 pairs over
    928 sequences and ~760 kB -- more sequences, more symbols and more pairs than any aligner case below"""
    global _ALIGNER_HISTORY
    if _ALIGNER_HISTORY is None:
        rng = random.Random(9001)
        db, fam = common.family_db(rng, 100, 8, 900)
        qs, src = common.queries_from_db(rng, db, 128, 330)
        qi, ti = [], []
        for k, s in enumerate(src):
            f0 = fam[s]
            for m in range(len(db)):
                if fam[m] in (f0, (f0 + 1) % 100, (f0 + 2) % 100):
                    qi.append(k)
                    ti.append(m)
        _ALIGNER_HISTORY = (qs, db, np.array(qi, np.uint32), np.array(ti, np.uint32))
    return _ALIGNER_HISTORY


def run_aligner_history(al):
    qs, db, qi, ti = aligner_history()
    Q, T = al.sequences(qs), al.sequences(db)
    res = al.align_pairs(Q, T, qi, ti)
    assert len(res) == len(qi)
    Q.close()
    T.close()


def aligner_sizes(seq_lists):
    hq, hd, _, _ = aligner_history()
    mine = [s for lst in seq_lists for s in lst]
    return (len(mine), sum(len(s) for s in mine)), (len(hq) + len(hd), sum(len(s) for s in hq + hd))


def plan_rows(al, qs, ts, qi, ti, dir_budget_bytes=0, runs=1):
    """one plan -> (rows of the last run, rows of every run, describe(), Timing of the last run)"""
    Q, T = al.sequences(qs), al.sequences(ts)
    p = al.plan(Q, T, np.array(qi, np.uint32), np.array(ti, np.uint32), dir_budget_bytes=dir_budget_bytes)
    info = p.describe()
    every = []
    for _ in range(runs):
        p.run()
        tm = p.sync()
        every.append(result_rows(p.fetch()))
    p.close()
    Q.close()
    T.close()
    return every[-1], every, info, tm


@register
class GoldenTorture(Case):
    """the fixtures of search16_golden.json and the torture slice under every scoring set: one-target tasks, the sparse NQ classes"""
    name = "golden_torture"

    def build(self):
        doc = common.load_golden()
        tort = torture_pairs()
        sets = []
        for name in doc["scorings"]:
            gold = [c for c in doc["cases"] if c["scoring"] == name]
            sets.append((name, [(c["q"], c["t"]) for c in gold] + tort, [tuple(c["exp"]) for c in gold]))
        return sets

    def reference(self, inp):
        orc = oracle()
        out = []
        for name, pairs, gold in inp:
            P, nmm = scoring(name)
            rows = [tuple(orc.align(q, t, P, nmm)) for q, t in pairs]
            assert rows[:len(gold)] == gold, f"oracle != golden vectors under {name}"
            out += rows_sections(name, rows)
        return out

    def device(self, inp, history):
        from vsearch_amd import Aligner
        out = []
        for name, pairs, _ in inp:
            P, nmm = scoring(name)
            with Aligner(scoring=P, n_mismatch=nmm) as al:
                if history:
                    run_aligner_history(al)
                idx = np.arange(len(pairs), dtype=np.uint32)
                rows, _, info, _ = plan_rows(al, [q for q, _ in pairs], [t for _, t in pairs], idx, idx)
                # (the sparse classes are sub-classes of the tilted one: a scoring set that cannot be tilted has none)
                assert (info["tasks_sparse"] > 0) == (info["tasks_tilted"] > 0) and (name != "default" or info["tasks_sparse"] > 0), (name, info)
            out += rows_sections(name, rows)
        return out

    def sizes(self, inp):
        return aligner_sizes([[s for pr in inp[0][1] for s in pr]])


EARLY_ROWS = (4, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 32)
_IU = common.IUPAC + "ACGT" * 6


def _early_target(rng, q, n, off, div):
    """n pure-ACGT symbols: random up to column off, a mutated copy of q, a random overhang (tests/test_gpu_early_stop.py _target)"""
    t = common.rnd_seq(rng, off) + common.mutate(rng, q, div)
    t = (t + common.rnd_seq(rng, n))[:n]
    return "".join(c if c in "ACGT" else rng.choice("ACGT") for c in t)


def early_plan(R, byte_profile=False):
    """the plan of one row class: queries of 16 R - 3 and 16 R symbols, each with two tasks of eight targets -- a 5 % mutated copy of
    the query at column 30 .. 40 and a random overhang, lengths within +-12 of Q + 400 and of Q + 800, clipped so that the planner's
    reach stays below the MAX3 limit of 15 800.  byte_profile: an IUPAC query and one N per task keep the tasks out of the split class"""
    # (two tasks of eight per query, not one: the two centres give the class a short and a long overhang -- the exit is taken at
    #  different steps, so the unwritten checkpoints of one task lie beside written ones of the other -- and two tasks keep the
    #  query below the four whole-wave tasks at which the planner would form a PAIR group, which has no early stop)
    P, _ = scoring("default")
    rng = random.Random(5000 + R + (500 if byte_profile else 0))
    qs, ts, qi, ti = [], [], [], []
    for Q in (16 * R - 3, 16 * R):
        q = common.rnd_seq(rng, Q, _IU if byte_profile else "ACGT")
        qs.append(q)
        for centre in (Q + 400, Q + 800):
            for x in range(8):
                n = centre + rng.randint(-12, 12)
                while tilt_reach(P, Q, n) >= 15800:
                    n -= 4
                t = _early_target(rng, q, n, rng.randint(30, 40), 0.05)
                if byte_profile and x == 2:
                    p = rng.randrange(len(t))
                    t = t[:p] + "N" + t[p + 1:]
                qi.append(len(qs) - 1)
                ti.append(len(ts))
                ts.append(t)
    return qs, ts, qi, ti


@register
class EarlyRows(Case):
    """one plan per row class that has the early stop: an early-stopped task leaves the checkpoints of its skipped steps unwritten
    right next to the step blocks every traceback variant addresses (LDS staging, the MID classes, the CK8 fallback)"""
    name = "early_rows"

    def build(self):
        return [(f"R{R}", R, early_plan(R)) for R in EARLY_ROWS] + [("R10_byte", 10, early_plan(10, byte_profile=True))]

    def reference(self, inp):
        orc = oracle()
        out = []
        for tag, _, (qs, ts, qi, ti) in inp:
            out += rows_sections(tag, [tuple(orc.align(qs[a], ts[b])) for a, b in zip(qi, ti)])
        return out

    def device(self, inp, history):
        from vsearch_amd import Aligner
        out = []
        with Aligner() as al:
            if history:
                run_aligner_history(al)
            for tag, R, (qs, ts, qi, ti) in inp:
                rows, _, info, tm = plan_rows(al, qs, ts, qi, ti)
                # (the planner cuts a query's targets, by falling length, eight to a task: 2 queries x 16 targets)
                assert info["rows_dominant"] == R and info["tasks"] == len(ts) // 8 and info["tasks_max3"] == info["tasks"], (tag, info)
                if tag == "R10_byte":
                    assert info["tasks_split"] == 0, (tag, info)
                assert int(tm.steps_skipped) > 0, f"{tag}: no task of the row class took the early exit"
                out += rows_sections(tag, rows)
        return out

    def sizes(self, inp):
        return aligner_sizes([p[2][0] + p[2][1] for p in inp])


def chunked_input():
    """the shapes of tests/test_gpu_parity.py::test_chunked_plan_equals_single_chunk, 6 pairs each, and its 3 000-symbol tracked pair"""
    rng = random.Random(777)
    qs, ts = [], []
    for ql, dl in [(60, 200), (250, 900), (400, 400), (700, 1500), (150, 300)] * 6:
        a = common.rnd_seq(rng, ql)
        b = common.rnd_seq(rng, rng.randint(0, dl // 2)) + common.mutate(rng, a, 0.06) + common.rnd_seq(rng, rng.randint(0, dl // 2))
        qs.append(a)
        ts.append(b)
    qs.append(common.rnd_seq(rng, 3000))
    ts.append(common.rnd_seq(rng, 3000) + qs[-1][:500])                 # two strips, overflow-tracked class
    return qs, ts


CHUNK_BUDGET = 1 << 20


@register
class Chunked(Case):
    """a checkpoint budget of 1 MB cuts the plan into chunks that reuse ONE block, run twice: chunk k + 1 sees chunk k's checkpoints"""
    name = "chunked"

    def build(self):
        return chunked_input()

    def reference(self, inp):
        orc = oracle()
        qs, ts = inp
        rows = [tuple(orc.align(q, t)) for q, t in zip(qs, ts)]
        return rows_sections("whole", rows) + rows_sections("parts", rows) + rows_sections("again", rows)

    def device(self, inp, history):
        from vsearch_amd import Aligner
        qs, ts = inp
        idx = np.arange(len(qs), dtype=np.uint32)
        with Aligner() as al:
            if history:
                run_aligner_history(al)
            whole, _, info1, _ = plan_rows(al, qs, ts, idx, idx)
            _, (parts, again), info, _ = plan_rows(al, qs, ts, idx, idx, dir_budget_bytes=CHUNK_BUDGET, runs=2)
            assert info1["chunks"] == 1 and info["chunks"] > 1, (info1, info)
        return rows_sections("whole", whole) + rows_sections("parts", parts) + rows_sections("again", again)

    def sizes(self, inp):
        return aligner_sizes(inp)


@register
class MultistripTracked(Case):
    """multi-strip queries (Q > 512) in the tilted, the plain and the overflow-tracked class, one task each"""
    name = "multistrip_tracked"

    def build(self):
        rng = random.Random(4242)
        qs, ts = [], []
        # (the last pair is beyond the issue's list: at Q + D >= 7 966 the planner's no_overflow_possible() fails under the default
        #  scoring and the task takes the overflow-tracked class, which 3 000 x 3 500 does not reach)
        for Q, D in ((530, 1100), (700, 1500), (3000, 3500), (3000, 5000)):
            q = common.rnd_seq(rng, Q)
            qs.append(q)
            ts.append((common.rnd_seq(rng, 20) + common.mutate(rng, q, 0.05) + common.rnd_seq(rng, D))[:D])
        return qs, ts

    def reference(self, inp):
        orc = oracle()
        return rows_sections("rows", [tuple(orc.align(q, t)) for q, t in zip(*inp)])

    def device(self, inp, history):
        from vsearch_amd import Aligner
        qs, ts = inp
        idx = np.arange(len(qs), dtype=np.uint32)
        with Aligner() as al:
            if history:
                run_aligner_history(al)
            rows, _, info, _ = plan_rows(al, qs, ts, idx, idx)
            assert info["tasks"] == 4 and info["tasks_tracked"] == 1 and info["tasks_tilted"] >= 2, info
        return rows_sections("rows", rows)

    def sizes(self, inp):
        return aligner_sizes(inp)


@register
class PairProfile(Case):
    """one pure query with 32 pure targets: a PAIR group of four whole-wave tasks (shared dword profile) where the scoring can be tilted"""
    name = "pair_profile"
    SETS = ("default", "distinct12")

    def build(self):
        rng = random.Random(97)
        q = common.rnd_seq(rng, 250)
        ts = [common.rnd_seq(rng, rng.randint(0, 200)) + common.mutate(rng, q, 0.1) + common.rnd_seq(rng, rng.randint(0, 500)) for _ in range(32)]
        return [q], ts

    def reference(self, inp):
        orc = oracle()
        (q,), ts = inp
        out = []
        for name in self.SETS:
            P, nmm = scoring(name)
            out += rows_sections(name, [tuple(orc.align(q, t, P, nmm)) for t in ts])
        return out

    def device(self, inp, history):
        from vsearch_amd import Aligner
        qs, ts = inp
        out = []
        for name in self.SETS:
            P, nmm = scoring(name)
            with Aligner(scoring=P, n_mismatch=nmm) as al:
                if history:
                    run_aligner_history(al)
                rows, _, info, _ = plan_rows(al, qs, ts, [0] * len(ts), range(len(ts)))
                # (distinct12 cannot be tilted -- its two interior gap extensions differ -- and has no pair class)
                assert (info["tasks_pair"] > 0) == (info["tasks_tilted"] > 0) and (name != "default" or info["tasks_pair"] == 4), (name, info)
            out += rows_sections(name, rows)
        return out

    def sizes(self, inp):
        return aligner_sizes(inp)


FILTER = dict(id=0.8, weak_id=0.7)


@register
class FilteredRanked(Case):
    """the sequence set of test_pipelined_slices_equal_one_plan with 2 000 pairs: vsx_align_pairs with and without the device filter,
    and the ranked form (kept-pair lists from the traceback, gather in vsx_rank.hip)"""
    name = "filtered_ranked"

    def build(self):
        rng = random.Random(21)
        fam = [common.rnd_seq(rng, rng.randint(40, 160)) for _ in range(40)]
        seqs = [common.mutate(rng, rng.choice(fam), rng.choice([0.03, 0.1, 0.3])) for _ in range(400)] + ["", "A"]
        qi = np.array([rng.randrange(len(seqs)) for _ in range(2000)], np.uint32)
        qi.sort()
        ti = np.array([rng.randrange(len(seqs)) for _ in range(2000)], np.uint32)
        return seqs, qi, ti

    @staticmethod
    def _ranked_sections(pair, rows, verdict, ident, undecided):
        cols = rows_sections("ranked", rows)
        return ([("ranked.pair", np.array(pair, np.uint32).tobytes())] + cols +
                [("ranked.verdict", np.array(verdict, np.uint8).tobytes()), ("ranked.id", np.array(ident, np.float64).tobytes()),
                 ("ranked.undecided", np.sort(np.array(undecided, np.uint32)).tobytes())])

    def reference(self, inp):
        orc = oracle()
        seqs, qi, ti = inp
        rows = [tuple(orc.align(seqs[a], seqs[b])) for a, b in zip(qi, ti)]
        # (a pair the library answers without DP -- an empty query has a closed form, an empty target the sentinel -- stays undecided and
        #  keeps its row: tests/marshal_data.py filtered_rows)
        from tests.marshal_data import full_filter
        full = full_filter(**FILTER)
        va = [(0, 0.0) if (len(seqs[a]) == 0 or len(seqs[b]) == 0 or r[0] == 32767) else accept_py(seqs[a], seqs[b], r, full)
              for a, b, r in zip(qi, ti, rows)]
        verdict = [v for v, _ in va]
        assert min(verdict.count(v) for v in (0, 1, 2, 3)) > 0
        # (a rejected pair keeps its numbers and loses its CIGAR: tests/marshal_data.py filtered_rows)
        frows = [r[:5] + ("",) if v == 3 else r for r, v in zip(rows, verdict)]
        out = rows_sections("plain", rows) + rows_sections("filtered", frows) + [("filtered.verdict", np.array(verdict, np.uint8).tobytes())]
        keep = [k for k in range(len(rows)) if verdict[k] in (1, 2)]
        # runs of equal query index in list order (qi is sorted: one run per query), id descending, then list order
        keep.sort(key=lambda k: (int(qi[k]), -va[k][1], k))
        return out + self._ranked_sections(keep, [rows[k] for k in keep], [verdict[k] for k in keep], [va[k][1] for k in keep],
                                           [k for k in range(len(rows)) if verdict[k] == 0])

    def device(self, inp, history):
        from vsearch_amd import Aligner
        seqs, qi, ti = inp
        with Aligner() as al:
            if history:
                run_aligner_history(al)
            ss = al.sequences(seqs)
            plain = al.align_pairs_oneshot(ss, ss, qi, ti, filter=None)
            flt = al.align_pairs_oneshot(ss, ss, qi, ti, filter=FILTER)
            rk = al.align_pairs_ranked(ss, ss, qi, ti, FILTER, keep_weak=True)
            ss.close()
        out = rows_sections("plain", result_rows(plain)) + rows_sections("filtered", result_rows(flt))
        out.append(("filtered.verdict", np.ascontiguousarray(flt.verdict, np.uint8).tobytes()))
        rows = [(int(rk["score"][j]), int(rk["aligned"][j]), int(rk["matches"][j]), int(rk["mismatches"][j]), int(rk["gaps"][j]), rk["cigar"][j])
                for j in range(len(rk["pair"]))]
        return out + self._ranked_sections(rk["pair"], rows, rk["verdict"], rk["id"], rk["undecided"])

    def sizes(self, inp):
        return aligner_sizes([inp[0]])


# ---- the read commands: device = host restatement, field for field ------------------------------------------------------------------------

@contextlib.contextmanager
def host_route(var):
    """VSX_<COMMAND>=host for one call, as the command's own tests set it"""
    if var is None:                 # (a command whose host route is simply a call without a context)
        yield
        return
    old = os.environ.get(var)
    os.environ[var] = "host"
    try:
        yield
    finally:
        if old is None:
            del os.environ[var]
        else:
            os.environ[var] = old


def fields_sections(tag, rec):
    """a numpy record array (or None) field by field: doubles go in by bit pattern, padding stays out"""
    if rec is None:
        return [(f"{tag}", b"none")]
    return [(f"{tag}.{name}", np.ascontiguousarray(rec[name]).tobytes()) for name in rec.dtype.names]


def table_sections(tag, res, scalars, tables):
    out = [(f"{tag}.{f}", repr(getattr(res, f)).encode()) for f in scalars]
    for f in tables:
        x = getattr(res, f)
        out.append((f"{tag}.{f}", b"none" if x is None else (str(x.dtype) + str(x.shape)).encode() + np.ascontiguousarray(x).tobytes()))
    return out


def text_size(lists):
    """(reads, bytes) of parallel lists of strings (None entries and None lists count nothing)"""
    lists = [lst for lst in lists if lst is not None]
    return max((len(lst) for lst in lists), default=0), sum(len(x) for lst in lists for x in lst if x is not None)


class ReadCommand(Case):
    """a command over reads: sets() -> [(tag, input)], history_set() -> the module's own generator with 2 000 reads; run(aligner, input)
    -> sections, with aligner None on the host route (env)"""
    env = None

    def sets(self):
        raise NotImplementedError

    def history_set(self):
        raise NotImplementedError

    def run(self, aligner, tag, x, device):
        raise NotImplementedError

    def size_of(self, x):
        raise NotImplementedError

    def build(self):
        return self.sets(), self.history_set()

    def reference(self, inp):
        out = []
        with host_route(self.env):
            for tag, x in inp[0]:
                out += self.run(None, tag, x, False)
        return out

    def device(self, inp, history):
        from vsearch_amd import Aligner
        out = []
        with Aligner(device=0) as al:
            if history:
                self.run(al, "history", inp[1], True)
            for tag, x in inp[0]:
                out += self.run(al, tag, x, True)
        return out

    def sizes(self, inp):
        # (every set is a call of its own on the handle: the largest one is what the history has to exceed)
        each = [self.size_of(x) for _, x in inp[0]]
        return (max(r for r, _ in each), max(b for _, b in each)), self.size_of(inp[1])


@register
class Merge(ReadCommand):
    """fastq_mergepairs (vsx_merge.hip) on merge_data.boundary_pairs() under the option sets of its boundary test"""
    name = "merge"
    env = "VSX_MERGE"

    def sets(self):
        from tests import merge_data as md
        data = md.boundary_pairs()
        runs = [{}, dict(minovlen=5), dict(allowmergestagger=True), dict(minovlen=5, allowmergestagger=True, maxns=0, truncqual=30)]
        return [(f"boundary{k}", (data, dict(md.BOUNDARY_OPTS, **extra))) for k, extra in enumerate(runs)]

    def history_set(self):
        from tests import merge_data as md
        return md.generate(20271, 2000), {}

    def run(self, aligner, tag, x, device):
        from vsearch_amd.merge import merge_pairs
        data, opts = x
        res = merge_pairs(aligner, *data[1:], **opts)
        assert res.stats["pairs_host"] == (0 if device else len(data[0])), (tag, res.stats)
        return fields_sections(tag, res.records) + [(f"{tag}.seq", bytes(res.seq_blob)), (f"{tag}.qual", bytes(res.qual_blob))]

    def size_of(self, x):
        return text_size(x[0][1:])


@register
class Filter(ReadCommand):
    """fastq_filter / fastx_filter (vsx_filter.hip): the edge and rounding reads and 150 generated pairs"""
    name = "filter"
    env = "VSX_FILTER"

    def sets(self):
        from tests import fastq_filter_data as fd
        return [(f"{k}_{s['name']}", s) for k, s in enumerate(fd.edge_reads() + fd.rounding_reads() + [fd.generate(3101, 150, paired=True)])]

    def history_set(self):
        from tests import fastq_filter_data as fd
        return fd.generate(3102, 2000, read_len=300, paired=True)

    def run(self, aligner, tag, s, device):
        from tests import fastq_filter_data as fd
        from vsearch_amd.filter import filter_reads
        a, k = fd.call_args(s)
        res = filter_reads(aligner, *a, **k)
        assert res.stats["reads_host"] == (0 if device else res.stats["reads"]), (tag, res.stats)
        return (fields_sections(tag + ".fwd", res.records) + fields_sections(tag + ".rev", res.rev_records) +
                [(f"{tag}.pair_discarded", np.ascontiguousarray(res.pair_discarded).tobytes()), (f"{tag}.counts", repr(sorted(res.counts().items())).encode())])

    def size_of(self, s):
        return text_size([s["seqs"], s["quals"], s.get("rev_seqs"), s.get("rev_quals")])


@register
class EEStats(ReadCommand):
    """fastq_eestats / fastq_eestats2 (vsx_eestats.hip): the edge reads and 40 generated reads"""
    name = "eestats"
    env = "VSX_EESTATS"

    def sets(self):
        from tests import eestats_data as ed
        return [(f"{k}_{s['name']}", s) for k, s in enumerate(ed.edge_reads() + [ed.generate(51, 40, read_len=100)])]

    def history_set(self):
        from tests import eestats_data as ed
        return ed.generate(3201, 2000, read_len=300)

    def run(self, aligner, tag, s, device):
        from tests import eestats_data as ed
        res = ed.call(aligner, s)
        assert res.stats["reads"] == len(s["quals"]) and res.stats["reads_host"] == (0 if device else res.stats["reads"]), (tag, res.stats)
        return table_sections(tag, res, ("n", "symbols", "len_min", "len_max", "ee_cutoffs", "length_cutoffs"), ed.TABLES)

    def size_of(self, s):
        return text_size([s["quals"]])


@register
class FastqStats(ReadCommand):
    """fastq_stats / fastq_chars (vsx_fastq_stats.hip): the edge reads and 40 generated reads, both commands"""
    name = "fastq_stats"
    env = "VSX_FASTQ_STATS"

    def sets(self):
        from tests import fastq_stats_data as fd
        return [(f"{k}_{s['name']}", s) for k, s in enumerate(fd.edge_reads() + [fd.generate(61, 40, read_len=100)])]

    def history_set(self):
        from tests import fastq_stats_data as fd
        return fd.generate(3301, 2000, read_len=300)

    def run(self, aligner, tag, s, device):
        from tests import fastq_stats_data as fd
        out = []
        for command in s.get("commands", fd.BOTH):
            res = fd.call(aligner, s, command)
            assert res.stats["reads"] == len(s["quals"]) and res.stats["reads_host"] == (0 if device else res.stats["reads"]), (tag, command, res.stats)
            stats = command == "stats"
            out += table_sections(f"{tag}.{command}", res, fd.STATS_FIELDS if stats else fd.CHARS_FIELDS, fd.STATS_TABLES if stats else fd.CHARS_TABLES)
        return out

    def size_of(self, s):
        return text_size([s["quals"], s["seqs"]])


@register
class Derep(ReadCommand):
    """derep_fulllength / fastx_uniques (vsx_derep.hip, a find-or-insert table somebody has to zero): the golden sets and the quality
    blocks"""
    name = "derep"

    def sets(self):
        from tests import derep_data as dd
        return [(f"{k}_{s['name']}", s) for k, s in enumerate(dd.load_golden() + [dd.quality_blocks_set(0), dd.quality_blocks_set(1)])]

    def history_set(self):
        from tests import derep_data as dd
        return dd.random_set(2000, seed=84, fastq=True)

    def run(self, aligner, tag, s, device):
        from tests import derep_data as dd
        res = dd.call(aligner, s)
        assert res.stats["reads_host"] == (0 if device else res.counts["kept"]), (tag, res.stats)
        return [(f"{tag}.fields", repr(dd.result_fields(res)).encode()), (f"{tag}.text", repr(sorted(dd.formatted(res, s).items())).encode())]

    def size_of(self, s):
        return text_size([s["seqs"], s.get("quals")])


@register
class DerepPrefix(ReadCommand):
    """derep_prefix (vsx_derep_prefix.hip): the golden sets"""
    name = "derep_prefix"

    def sets(self):
        from tests import derep_prefix_data as pd
        return [(f"{k}_{s['name']}", s) for k, s in enumerate(pd.load_golden())]

    def history_set(self):
        from tests import derep_prefix_data as pd
        return pd.random_set(2000, seed=180)

    def run(self, aligner, tag, s, device):
        from tests import derep_prefix_data as pd
        res = pd.call(aligner, s)
        assert res.stats["reads_host"] == (0 if device else res.counts["kept"]), (tag, res.stats)
        return [(f"{tag}.fields", repr(pd.result_fields(res)).encode()), (f"{tag}.text", repr(sorted(pd.formatted(res, s).items())).encode()),
                (f"{tag}.nodes", repr((res.stats["nodes"], res.stats["distinct_lengths"])).encode())]

    def size_of(self, s):
        return text_size([s["seqs"]])


class SessionCommand(Case):
    """a command on a SearchSession bound to the set's database: per set a session on ONE aligner; the history call runs the module's
    2 000 generated reads through the SAME session first (its window buffers are grow-only)"""

    def sets(self):
        raise NotImplementedError

    def history_reads(self):
        raise NotImplementedError

    def open(self, aligner, s):
        raise NotImplementedError

    def history_call(self, sess, reads):
        raise NotImplementedError

    def on_device(self, sess, tag, s):
        raise NotImplementedError

    def on_host(self, tag, s):
        raise NotImplementedError

    def build(self):
        return self.sets(), self.history_reads()

    def reference(self, inp):
        return [x for tag, s in inp[0] for x in self.on_host(tag, s)]

    def device(self, inp, history):
        from vsearch_amd import Aligner
        out = []
        with Aligner(device=0) as al:
            for tag, s in inp[0]:
                sess = self.open(al, s)
                try:
                    if history:
                        self.history_call(sess, inp[1])
                    out += self.on_device(sess, tag, s)
                finally:
                    sess.close()
        return out

    def sizes(self, inp):
        each = [text_size([s["queries"]]) for _, s in inp[0]]
        return (max(r for r, _ in each), max(b for _, b in each)), text_size([inp[1]])


@register
class SearchExact(SessionCommand):
    """search_exact (vsx_exact.hip, a find-or-insert table): the golden sets (lengths 1 .. 2 049)"""
    name = "search_exact"

    def sets(self):
        from tests import search_exact_data as sd
        sets = sd.load_golden()
        assert max(len(x) for s in sets for x in s["queries"] + s["db"]) <= 2049
        return [(f"{k}_{s['name']}", s) for k, s in enumerate(sets)]

    def history_reads(self):
        from tests import search_exact_data as sd
        return sd.seeded_set(31, 300, 2000)["queries"]

    def open(self, aligner, s):
        from tests import search_exact_data as sd
        from vsearch_amd import SearchSession
        return SearchSession(aligner, s["db"], sizes=s["db_sizes"], labels=s["db_names"], **sd.session_opts(s["opts"]))

    def history_call(self, sess, reads):
        sess.search_exact_raw(reads)
        assert sess.exact_stats["queries_host"] == 0

    @staticmethod
    def _sections(tag, raw):
        first, hits, cigars = raw
        return [(f"{tag}.first", np.ascontiguousarray(first).tobytes())] + fields_sections(f"{tag}.hits", hits) + [(f"{tag}.cigars", bytes(cigars))]

    def on_device(self, sess, tag, s):
        raw = sess.search_exact_raw(s["queries"], sizes=s["sizes"], labels=s["names"])
        st = sess.exact_stats
        assert st["queries_host"] == 0 and st["queries_device"] == len(s["queries"]), (tag, st)
        return self._sections(tag, raw)

    def on_host(self, tag, s):
        from tests import search_exact_data as sd
        from vsearch_amd.search import search_exact_host
        return self._sections(tag, search_exact_host(s["db"], s["queries"], db_sizes=s["db_sizes"], db_labels=s["db_names"], sizes=s["sizes"],
                                                     labels=s["names"], raw=True, **sd.session_opts(s["opts"])))


@register
class Sintax(SessionCommand):
    """sintax (vsx_sintax.hip): the golden sets; a set whose options send it to a host route is asserted to take that route"""
    name = "sintax"

    def sets(self):
        from tests import sintax_data as sd
        return [(f"{k}_{s['name']}", s) for k, s in enumerate(sd.load_golden())]

    def history_reads(self):
        from tests import sintax_data as sd
        rng = random.Random(3401)
        return [sd.random_seq(rng, rng.randint(60, 300)) for _ in range(2000)]

    @staticmethod
    def _kw(s):
        from tests import sintax_data as sd
        o = sd.full_opts(s["opts"])
        return o, dict(randseed=o["seed"], strand_both=o["strand_both"], sintax_random=o["random"], want_candidates=True)

    def open(self, aligner, s):
        from tests import sintax_data as sd
        from vsearch_amd import SearchSession
        o = sd.full_opts(s["opts"])
        return SearchSession(aligner, s["db"], labels=s["db_labels"], id=0.97, wordlength=o["wordlength"], soft_mask=sd.MASK_MODES[o["dbmask"]],
                             hardmask=1 if o["hardmask"] else 0)

    def history_call(self, sess, reads):
        from vsearch_amd import sintax
        assert sintax(sess, reads, randseed=7, strand_both=True).stats["queries_host_random"] == 0

    @staticmethod
    def _sections(tag, res):
        f = res.fields()
        return [(f"{tag}.{k}", repr(np.asarray(f[k]).dtype).encode() + np.ascontiguousarray(f[k]).tobytes()) for k in sorted(f)] + \
               [(f"{tag}.n_classified", repr(int(res.n_classified)).encode())]

    def on_device(self, sess, tag, s):
        from vsearch_amd import sintax
        o, kw = self._kw(s)
        res = sintax(sess, s["queries"], **kw)
        route = "queries_host_random" if o["random"] else "queries_host_wordlength" if o["wordlength"] > 8 else "queries_device"
        assert res.stats[route] == len(s["queries"]), (tag, res.stats)
        return self._sections(tag, res)

    def on_host(self, tag, s):
        from tests import sintax_data as sd
        from vsearch_amd import sintax_host
        o, kw = self._kw(s)
        return self._sections(tag, sintax_host(s["db"], s["db_labels"], s["queries"], wordlength=o["wordlength"], soft_mask=sd.MASK_MODES[o["dbmask"]],
                                               hardmask=1 if o["hardmask"] else 0, **kw))


@register
class Orient(SessionCommand):
    """orient (vsx_orient.hip, the match-count table mc[4^w] and the distinct-word sets): the golden sets and length_set()"""
    name = "orient"

    def sets(self):
        from tests import orient_data as od
        return [(f"{k}_{s['name']}", s) for k, s in enumerate(od.load_golden() + [od.length_set()])]

    def history_reads(self):
        from tests import orient_data as od
        return od.simulated(3501, 20, 400, 2000, 250)[1]

    def open(self, aligner, s):
        from tests import orient_data as od
        from vsearch_amd.orient import orient_session
        o = od.full_opts(s["opts"])
        return orient_session(aligner, s["db"], wordlength=o["wordlength"], soft_mask=od.MASK_MODES[o["dbmask"]], hardmask=1 if o["hardmask"] else 0)

    def history_call(self, sess, reads):
        from vsearch_amd.orient import orient
        assert orient(sess, reads).n == len(reads)

    @staticmethod
    def _sections(tag, res):
        f = res.fields()
        out = [(f"{tag}.{k}", repr(np.asarray(f[k]).dtype).encode() + np.ascontiguousarray(f[k]).tobytes()) for k in sorted(f)]
        return out + [(f"{tag}.counts", repr((res.n_fwd, res.n_rev, res.n_none, res.stats["words_distinct"])).encode()),
                      (f"{tag}.text", repr(res.text).encode()), (f"{tag}.qual", repr(res.qual).encode())]

    def on_device(self, sess, tag, s):
        from tests import orient_data as od
        from vsearch_amd.orient import orient
        o = od.full_opts(s["opts"])
        res = orient(sess, s["queries"], quals=s["quals"], qmask=o["qmask"])
        route = "queries_host_wordlength" if o["wordlength"] > 12 else "queries_device"
        assert res.stats[route] == res.n == len(s["queries"]), (tag, res.stats)
        return self._sections(tag, res)

    def on_host(self, tag, s):
        from tests import orient_data as od
        from vsearch_amd.orient import orient_host
        o = od.full_opts(s["opts"])
        return self._sections(tag, orient_host(s["db"], s["queries"], quals=s["quals"], wordlength=o["wordlength"], soft_mask=od.MASK_MODES[o["dbmask"]],
                                               hardmask=1 if o["hardmask"] else 0, qmask=o["qmask"]))


# ---- the search stack ---------------------------------------------------------------------------------------------------------------------

@register
class Kmer(Case):
    """the k-mer candidate stage (vsx_kmer.hip: counters, cursors, bucket tables that have to be zeroed) on inputs of
    tests/kmer_edge_data.py, one per route: packed postings at w = 8, tagged postings at w = 12, the 254 .. 257-word queries, the
    exact-heap / ties selection input, a multi-hop gap input.  device == host restatement == py_candidates()"""
    name = "kmer"

    def build(self):
        from tests import kmer_edge_data as ked
        sets = []
        db, qs, opts, _ = ked.threshold_edges(8)
        sets.append(("packed_w8", db, qs, dict(opts, minwordmatches=255)))
        db, qs, opts, _ = ked.threshold_edges(12)
        sets.append(("tagged_w12", db, qs, dict(opts, minwordmatches=129)))
        for tag, (db, qs, opts, _) in (("class_switch", ked.class_switch()), ("selection", ked.selection_edges()), ("gaps", ked.gap_edges())):
            sets.append((tag, db, qs, opts))
        rng = random.Random(3601)
        return sets, [ked.rnd(rng, 300) for _ in range(2000)]

    def reference(self, inp):
        from tests import kmer_edge_data as ked
        return [(tag, repr(ked.expected(db, qs, opts)).encode()) for tag, db, qs, opts in inp[0]]

    def device(self, inp, history):
        from vsearch_amd import Aligner, SearchSession
        out = []
        with Aligner() as al:
            for tag, db, qs, opts in inp[0]:
                ss = SearchSession(al, db, id=0.5, **opts)
                try:
                    if history:
                        assert len(ss.candidates_batch(inp[1], device=True)) == len(inp[1])
                    dev = ss.candidates_batch(qs, device=True)          # (refused with EINVAL where the searcher is off the device path)
                    host = ss.candidates_batch(qs, device=False)
                    assert dev == host, f"{tag}: device != host restatement"
                finally:
                    ss.close()
                out.append((tag, repr(dev).encode()))
        return out

    def sizes(self, inp):
        each = [text_size([qs]) for _, _, qs, _ in inp[0]]
        return (max(r for r, _ in each), max(b for _, b in each)), text_size([inp[1]])


@register
class SearchDust(Case):
    """--usearch_global, 200 queries against 2 000 sequences of mask_data.masked_families, soft_mask = 2 (the database DUST-masked by
    vsx_mask.hip, the queries by the host), both strands: a whole search -- masked index build, scanner windows, ranked alignment, hit
    selection.  The candidate lists of the device must equal those of the searcher's host k-mer route, and every hit's row the scalar
    oracle's for that (query strand, target).  The searcher needs a device, so the reference is computed in the child, on a fresh handle:
    host-route candidates, and the hits with their rows replaced by the oracle's."""
    name = "search_dust"
    device_reference = True
    OPTS = dict(id=0.8, maxaccepts=2, maxrejects=4, strand_both=1, soft_mask=2)
    ROW = ("nwscore", "nwalignmentlength", "matches", "mismatches", "nwgaps", "cigar")

    def build(self):
        from tests import mask_data as md
        rng = random.Random(2020)
        db = md.masked_families(rng, 400, 5, 420, 0.05, False)
        qs = md.queries(rng, db, 200, 200, 0.03, False)
        for k in range(0, len(qs), 2):
            qs[k] = "".join(md.COMP[c] for c in reversed(qs[k]))
        return db, qs, md.queries(random.Random(2021), db, 500, 320, 0.03, False)

    @staticmethod
    def _sections(cands, hits):
        return [("candidates", repr(cands).encode()), ("hits", repr(canon(hits)).encode())]

    def device(self, inp, history):
        from vsearch_amd import Aligner, SearchSession
        db, qs, hq = inp
        with Aligner() as al:
            ss = SearchSession(al, db, **self.OPTS)
            try:
                if history:
                    assert len(ss.search_batch(hq)) == len(hq)
                cands = ss.candidates_batch(qs, device=True)          # (EINVAL if the masking pushed the searcher off the device k-mer path)
                hits = ss.search_batch(qs)
            finally:
                ss.close()
        assert sum(1 for hs in hits if hs) > 150 and any(h["strand"] for hs in hits for h in hs)
        return self._sections(cands, hits)

    def reference(self, inp):
        from tests import mask_data as md
        from vsearch_amd import Aligner, SearchSession
        db, qs, _ = inp
        orc = oracle()
        with Aligner() as al:
            ss = SearchSession(al, db, **self.OPTS)
            try:
                cands = ss.candidates_batch(qs, device=False)
                hits = ss.search_batch(qs)
            finally:
                ss.close()
        for q, hs in zip(qs, hits):
            rc = "".join(md.COMP[c] for c in reversed(q))
            for h in hs:
                assert not h["used_fallback"]
                h.update(zip(self.ROW, orc.align(rc if h["strand"] else q, db[h["target"]])))
        return self._sections(cands, hits)

    def sizes(self, inp):
        return text_size([inp[1]]), text_size([inp[2]])


@register
class DustBits(Case):
    """vsx_mask.hip: the DUST intervals are OR-ed (atomicOr) into a case bitmap somebody has to zero; vsx_internal_mask_bits on the
    inputs of dust_golden.json and 300 generated ones against the host DUST (dust_mask), and the input's own case (mode 1)"""
    name = "dust_bits"

    def build(self):
        from oracle import gen_golden
        with open(os.path.join(common.GOLD, "dust_golden.json")) as f:
            doc = json.load(f)
        seqs = list(doc["in"]) + gen_golden.dust_inputs(random.Random(77), 300) + ["ACGT" * 3, ""]
        return seqs, gen_golden.dust_inputs(random.Random(78), 3000) + ["A" * 70000]

    @staticmethod
    def _sections(bits_by_mode):
        return [(f"mode{m}", np.packbits(b, bitorder="little").tobytes()) for m, b in bits_by_mode]

    def reference(self, inp):
        from vsearch_amd import dust_mask
        seqs = inp[0]
        blob, _, _ = common.blobify(seqs)
        out = []
        for mode in (2, 1):
            text = b"".join(dust_mask(seqs)) if mode == 2 else blob
            out.append((mode, ~np.isin(np.frombuffer(text, np.uint8), np.frombuffer(b"ACGTU", np.uint8))))
        assert out[0][1].sum() > 1000
        return self._sections(out)

    @staticmethod
    def _bits(al, seqs, mode):
        import ctypes as C
        from vsearch_amd import _lib
        lib = _lib.load()
        blob, off, lens = common.blobify(seqs)
        bits = np.zeros((len(blob) + 7) // 8, np.uint8)
        rc = lib.vsx_internal_mask_bits(al.h, C.c_uint64(len(lens)), C.cast(C.c_char_p(blob), C.c_void_p), C.c_uint64(len(blob)),
                                        off.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), C.c_int(mode), bits.ctypes.data_as(C.c_void_p))
        assert rc == 0, lib.vsx_last_error()
        return np.unpackbits(bits, bitorder="little")[:len(blob)].astype(bool)

    def device(self, inp, history):
        from vsearch_amd import Aligner
        with Aligner() as al:
            if history:
                assert self._bits(al, inp[1], 2).any()
            return self._sections([(mode, self._bits(al, inp[0], mode)) for mode in (2, 1)])

    def sizes(self, inp):
        return text_size([inp[0]]), text_size([inp[1]])


def canon(obj):
    """records (dicts, lists, floats ...) as text with every double by its bits"""
    if isinstance(obj, float):
        return obj.hex()
    if isinstance(obj, dict):
        return {k: canon(v) for k, v in sorted(obj.items())}
    if isinstance(obj, (list, tuple)):
        return [canon(v) for v in obj]
    return obj


class ChimeraCase(Case):
    """chimera detection: the part search and the alignments run on the device either way, so the reference -- the library's host
    restatement of parent selection and scoring, VSX_CHIMERA=host set for the call -- needs a device too (device_reference): the
    driver computes it in the child, and the test takes the digest the unpoisoned child reports"""
    device_reference = True
    host_queries_expected = True        # (the de novo sets hold queries beyond the kernels' limits on purpose)

    def records(self, al, inp, history):
        """-> (sections, stats of the case's session(s))"""
        raise NotImplementedError

    def device(self, inp, history):
        from vsearch_amd import Aligner
        with Aligner(device=0) as al:
            out, stats = self.records(al, inp, history)
        assert all(st["queries_kernel"] > 0 for st in stats), stats
        assert self.host_queries_expected or all(st["queries_host"] == 0 for st in stats), stats
        return out

    def reference(self, inp):
        from vsearch_amd import Aligner
        with host_route("VSX_CHIMERA"), Aligner(device=0) as al:
            out, stats = self.records(al, inp, False)
        assert all(st["queries_kernel"] == 0 for st in stats), stats
        return out


@register
class UchimeRef(ChimeraCase):
    """uchime_ref (vsx_chimera.hip) on chimera_length_data.family(L), L = 64, 513, 4 096: one database of unrelated families; the
    history call runs the queries of five other families of the same database through the same session"""
    name = "uchime_ref"
    host_queries_expected = False
    LENGTHS = (64, 513, 4096)
    HISTORY = (1500, 2047, 2048, 2049, 4064)

    def build(self):
        from tests import chimera_length_data as cd
        tn, db, qs, hq = [], [], [], []
        for L in self.LENGTHS + self.HISTORY:
            n, d, _, q = cd.family(L)
            tn += n
            db += d
            (qs if L in self.LENGTHS else hq).extend(q)
        return tn, db, qs, hq

    def records(self, al, inp, history):
        from vsearch_amd import ChimeraSession
        tn, db, qs, hq = inp
        s = ChimeraSession(al, db, labels=tn)
        if history:
            assert len(s.uchime_ref(hq)) == len(hq)
        recs = s.uchime_ref(qs)
        return [("records", repr(canon(recs)).encode())], [dict(s.stats)]

    def sizes(self, inp):
        return text_size([inp[2]]), text_size([inp[3]])


@register
class UchimeDenovo(ChimeraCase):
    """uchime_denovo on denovo_data.cascade_set with 20 families; the history is a session over 60 families on the same context"""
    name = "uchime_denovo"

    def build(self):
        from tests import denovo_data
        return denovo_data.cascade_set(n_families=20), denovo_data.cascade_set(seed=78, n_families=60)

    def records(self, al, inp, history):
        from vsearch_amd import DenovoChimeraSession
        if history:
            labels, seqs = inp[1]
            assert len(DenovoChimeraSession(al, seqs, labels).uchime_denovo()) == len(seqs)
        labels, seqs = inp[0]
        s = DenovoChimeraSession(al, seqs, labels)
        recs = s.uchime_denovo()
        return [("records", repr(canon(recs)).encode())], [dict(s.stats)]

    def sizes(self, inp):
        return text_size([inp[0][1]]), text_size([inp[1][1]])


@register
class ChimerasDenovo(ChimeraCase):
    """chimeras_denovo (vsx_chimera_long.hip) on the edge inputs diff_pct1, diff_pct2.5 (the global suffix-sum scratch), cand64,
    qlen2048, one_parent_twice; the history is a session over a seeded set of 48 families on the same context"""
    name = "chimeras_denovo"
    EDGES = ("diff_pct1", "diff_pct2.5", "cand64", "qlen2048", "one_parent_twice")

    def build(self):
        from tests import chimeras_long_data as data
        edges = data.edge_cases()
        return [(name, edges[name]) for name in self.EDGES], data.seeded_set(seed=32, n_families=48, n_chimeras=140)

    def records(self, al, inp, history):
        from vsearch_amd import ChimerasDenovoSession
        if history:
            labels, seqs = inp[1]
            assert len(ChimerasDenovoSession(al, seqs, labels).chimeras_denovo()) == len(seqs)
        out, stats = [], []
        for name, c in inp[0]:
            s = ChimerasDenovoSession(al, c["seqs"], c["labels"], **c["opts"])
            out.append((name, repr(canon(s.chimeras_denovo())).encode()))
            stats.append(dict(s.stats))
        return out, stats

    def sizes(self, inp):
        each = [text_size([c["seqs"]]) for _, c in inp[0]]
        return (max(r for r, _ in each), max(b for _, b in each)), text_size([inp[1][1]])


@register
class Allpairs(Case):
    """allpairs_global over 200 sequences, accept-all and filtered: vsx_allpairs_stream (blocks of 37 rows, enumeration / alignment /
    completion overlapped) against ONE vsx_allpairs_block call -- both on the device, so the reference is computed in the child; the
    history is an allpairs over 300 longer sequences on the same context"""
    name = "allpairs"
    device_reference = True
    RUNS = ((True, dict(id=0.5)), (False, dict(id=0.8)))

    def build(self):
        def draw(seed, n, lo, hi):
            rng = random.Random(seed)
            fam = [common.rnd_seq(rng, rng.randint(lo, hi)) for _ in range(12)]
            return [common.mutate(rng, rng.choice(fam), rng.choice([0.02, 0.08, 0.2])) for _ in range(n)]
        return draw(77, 200, 60, 220), draw(78, 300, 200, 330)

    def _run(self, inp, history, stream):
        from vsearch_amd import Aligner
        from vsearch_amd.search import SearchSession
        out = []
        with Aligner() as al:
            for acceptall, kw in self.RUNS:
                if history:
                    hs = SearchSession(al, inp[1], **kw)
                    assert len(hs.allpairs(acceptall=acceptall)) == len(inp[1])
                    hs.close()
                ss = SearchSession(al, inp[0], **kw)
                hits = ss.allpairs_stream(block=37, acceptall=acceptall) if stream else ss.allpairs(acceptall=acceptall)
                assert ss.stats["pairs_aligned"] > 0 and len(hits) == len(inp[0])
                if acceptall:
                    assert sum(len(h) for h in hits) == len(inp[0]) * (len(inp[0]) - 1) // 2
                ss.close()
                out.append((f"acceptall{int(acceptall)}", repr(canon(hits)).encode()))
        return out

    def device(self, inp, history):
        return self._run(inp, history, True)

    def reference(self, inp):
        return self._run(inp, False, False)

    def sizes(self, inp):
        return text_size([inp[0]]), text_size([inp[1]])


# ---- the MSA (vsx_msa.hip) --------------------------------------------------------------------------------------------------------------

def msa_row_tile():
    """rows of one tile of the device MSA's profile kernel, as the library says"""
    from vsearch_amd import _lib
    return int(_lib.load().vsx_internal_msa_row_tile())


@register
class ClusterMsa(Case):
    """cluster_fast(round=16) on the ~45 sequences of the --msaout test (vsx_cluster.cpp: speculative rounds, grow-only scratch), then
    vsx_msa_device_batch against the host form on its clusters, on the drawn clusters of test_msa_device_equals_host and on one of
    row tile + 1 = 4 097 members x 70 columns (two row tiles); the profile counters are summed into memory the call has to zero.
    Assignments and CIGARs go into the digest.  The clustering needs a device, so the reference is computed in the child: a
    clustering on a fresh handle gives the assignments, the scalar oracle every member's row against its centroid, the host MSA the rest."""
    name = "cluster_msa"
    device_reference = True
    MEMBERS = 4097

    def build(self):
        from tests.msa_data import cluster_input, random_cluster
        seqs, names = cluster_input()
        order = sorted(range(len(seqs)), key=lambda i: (-len(seqs[i]), names[i]))          # Database::sortbylength
        rng = random.Random(5)
        cl_s, cl_c, cl_a = [], [], []
        for k in range(40):
            n = rng.choice([1, 1, 2, 3, 8, 30, 200])
            alpha = rng.choice(["ACGT", "ACGTacgtNRYn", "ACGTUX*-"])
            s, c = random_cluster(rng, n, rng.choice([1, 7, 64, 65, 255, 256, 257, 400]), alpha, long_ins=(k % 5 == 0))
            cl_s.append(s); cl_c.append(c)
            cl_a.append([rng.choice([0, 1, 1, 3, 2 ** 40 + 7]) for _ in s])
        s, c = random_cluster(rng, self.MEMBERS, 70, "ACGT")
        cl_s.append(s); cl_c.append(c); cl_a.append([rng.randint(0, 5) for _ in s])
        cl_s.append(["ACGT", "", "ACGT"]); cl_c.append([None, "4I", "4M"]); cl_a.append([0, 0, 0])
        hrng = random.Random(6)
        hs, hc = random_cluster(hrng, 2 * 4096 + 1, 150, "ACGT")         # (three row tiles)
        hfam = common.family_db(hrng, 30, 8, 300, div=0.04)[0]
        return [seqs[i] for i in order], (cl_s, cl_c, cl_a), ([hs], [hc], [[hrng.randint(0, 5) for _ in hs]]), sorted(hfam, key=lambda x: -len(x))

    @staticmethod
    def _msa_sections(tag, results):
        out = []
        for k, r in enumerate(results):
            out.append((f"{tag}{k}.rows", "\n".join(r["rows"]).encode()))
            out.append((f"{tag}{k}.consensus", r["consensus"].encode()))
            out.append((f"{tag}{k}.profile", np.array(r["profile"], np.uint64).tobytes()))
        return out

    @staticmethod
    def _cluster(al, sseqs):
        from vsearch_amd import SearchSession
        ss = SearchSession(al, sseqs, id=0.85, maxrejects=8)
        try:
            cno, per, ncl = ss.cluster_fast(round=16)
        finally:
            ss.close()
        members = [[] for _ in range(ncl)]
        for s, c in enumerate(cno):
            members[c].append(s)                       # ascending seqno: the centroid comes first
        assert all(per[m[0]] is None for m in members) and 1 < ncl < len(sseqs)
        return cno, per, members

    @staticmethod
    def _hit_rows(per):
        return [None if h is None else (h["target"], h["nwscore"], h["nwalignmentlength"], h["matches"], h["mismatches"], h["nwgaps"], h["cigar"])
                for h in per]

    def _sections(self, cno, rows, clustered, drawn):
        return ([("cluster.assignment", np.array(cno, np.uint32).tobytes()), ("cluster.hits", repr(rows).encode())] +
                self._msa_sections("m", clustered) + self._msa_sections("c", drawn))

    def device(self, inp, history):
        from vsearch_amd import Aligner, SearchSession, msa_batch
        sseqs, drawn, hist, hfam = inp
        with Aligner() as al:
            if history:
                hs = SearchSession(al, hfam, id=0.85, maxrejects=8)
                assert hs.cluster_fast(round=16)[2] > 1
                hs.close()
                assert len(msa_batch(*hist, al)) == 1
            cno, per, members = self._cluster(al, sseqs)
            clustered = msa_batch([[sseqs[s] for s in m] for m in members], [[None] + [per[s]["cigar"] for s in m[1:]] for m in members], None, al)
            return self._sections(cno, self._hit_rows(per), clustered, msa_batch(*drawn, al))

    def reference(self, inp):
        from vsearch_amd import Aligner, msa_batch
        sseqs, drawn, _, _ = inp
        orc = oracle()
        with Aligner() as al:
            cno, per, members = self._cluster(al, sseqs)
        rows = [None if h is None else (h["target"],) + tuple(orc.align(sseqs[s], sseqs[h["target"]])) for s, h in enumerate(per)]
        assert all(h is None or members[cno[s]][0] == h["target"] for s, h in enumerate(per))
        clustered = msa_batch([[sseqs[s] for s in m] for m in members], [[None] + [rows[s][6] for s in m[1:]] for m in members], None, None)
        return self._sections(cno, rows, clustered, msa_batch(*drawn, None))

    def sizes(self, inp):
        flat = lambda cl: [s for c in cl for s in c]      # noqa: E731
        mine, hist = flat(inp[1][0]), flat(inp[2][0])
        assert len(inp[3]) > len(inp[0]) and sum(map(len, inp[3])) > sum(map(len, inp[0]))
        return (len(mine), sum(len(s) for s in mine)), (len(hist), sum(len(s) for s in hist))


# ---- the driver -----------------------------------------------------------------------------------------------------------------------

def poison_byte():
    from vsearch_amd import _lib
    return int(_lib.load().vsx_internal_poison_byte())


_REFERENCE = {}


def reference_digest(name):
    """the digest of a case's CPU reference (computed once per process)"""
    if name not in _REFERENCE:
        case = CASES[name]
        _REFERENCE[name] = digest(case.reference(case.input()))
    return _REFERENCE[name]


def run_case(name, verify=False):
    case = CASES[name]
    t0 = time.time()
    rec = {"digest": None, "digest_history": None, "digest_reference": None, "seconds": None, "error": None}
    try:
        inp = case.input()
        fresh = case.device(inp, False)
        rec["digest"] = digest(fresh)
        after = case.device(inp, True)
        rec["digest_history"] = digest(after)
        if rec["digest"] != rec["digest_history"]:
            rec["error"] = f"the result depends on the handle's history: first differing section {first_difference(fresh, after)}"
        elif case.device_reference:
            ref = case.reference(inp)
            rec["digest_reference"] = digest(ref)
            if rec["digest_reference"] != rec["digest"]:
                rec["error"] = f"device != host restatement: first differing section {first_difference(fresh, ref)}"
        elif verify:
            ref = case.reference(inp)
            if digest(ref) != rec["digest"]:
                rec["error"] = f"device != CPU reference: first differing section {first_difference(fresh, ref)}"
    except Exception as e:      # noqa: BLE001 -- the report carries the failure; the driver goes on with the next case
        import traceback
        rec["error"] = f"{type(e).__name__}: {e}\n{traceback.format_exc()[-1500:]}"
    rec["seconds"] = round(time.time() - t0, 3)
    return rec


# HIP errors that stay with the process (the device context is lost): after one of them nothing more may be started on the GPU
STICKY = ("illegal memory access", "unspecified launch failure", "launch failure", "hardware exception", "misaligned address",
          "illegal instruction", "invalid program counter", "device-side assert", "uncorrectable ECC", "launch timed out", "hipErrorLaunch",
          "hipErrorIllegal", "hipErrorAssert", "hipErrorUnknown", "unknown error")
EXIT_GPU_FAULT = 3


def is_sticky(text):
    return text is not None and any(word.lower() in text.lower() for word in STICKY)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--case", action="append", choices=sorted(CASES), help="default: every registered case")
    ap.add_argument("--verify", action="store_true", help="also compare with the CPU reference inside the child")
    a = ap.parse_args(argv)
    # as tests/conftest.py: any drift of the ranked path is to be SEEN, and the small fixtures are to reach the sparse-task kernels
    os.environ.setdefault("VSX_RANK_STRICT", "1")
    os.environ.setdefault("VSX_SPARSE_MIN", "1")
    report = {"_poison_byte": poison_byte()}

    def flush():
        tmp = a.out + ".tmp"
        with open(tmp, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, a.out)

    flush()
    failed = False
    for name in a.case or list(CASES):
        report[name] = run_case(name, a.verify)
        failed |= report[name]["error"] is not None
        print(name, report[name]["seconds"], "s", "FAILED: " + report[name]["error"] if report[name]["error"] else "ok", flush=True)
        flush()
        if is_sticky(report[name]["error"]):
            # a GPU fault: the report is on disk, the cases that are left count as not run, and nothing else touches the device --
            # no further case, no destructor of a handle
            print(f"{name}: GPU fault, the driver stops here", flush=True)
            os._exit(EXIT_GPU_FAULT)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
