"""Inputs of tests/test_gpu_chimera_lengths.py: per query length L a small family database and queries of exactly L symbols, built
for the places where vsx_chimera.hip changes behaviour with L (32-column windows, 32-bit match words, 256-column scan chunks,
the limit VSX_CHIMERA_MAX_QLEN = 4096) and for the alignment shapes its column rules depend on.

family(L) -> (parent labels, parents, query labels, queries).  Eight parents of L .. L + 40 symbols, 8-12 % apart: parents 0-4 differ
from the ancestor by substitutions only (their columns coincide, so breakpoints and diagnostic columns are exact), parents 5-7
carry indels.  Queries:
    chim2      parents 0 | 1, the breakpoint within +-1 of a multiple of 256 (the middle where L < 300)
    chim3      parents 0 | 3 | 1
    plain      parent 4, 1 % substitutions
    overhang   parents 0 | 1 cut from inside: both parents carry 5-30 extra symbols before the query's column 0 and at least 5
               after column L - 1 (target insertions at both ends of the alignment)
    ambig      parents 2 | 1 with N / R / Y in the query beside the breakpoint; parent 2 carries N / R / Y there too
    indel      parents 3 | 4 with three symbols deleted directly beside one diagnostic column and three inserted beside another
"""
import random

from tests import common

KERNEL_LENGTHS = [32, 33, 63, 64, 65, 95, 96, 97, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1500, 2047, 2048, 2049, 4064, 4065,
                  4095, 4096]
HOST_LENGTHS = [4097, 4128]
EXTRA_LENGTHS = [42, 43, 48, 49]     # the shortest at which a query of family() gets two candidates from the reference's part search
# short_lengths(): seeds of two unrelated parents of exactly L symbols whose half-and-half chimera the reference scores (found by
# running the reference CLI over seeds L * 1000 ...; most seeds give no candidates: a part of 8-10 symbols holds 1-3 words)
SHORT_SEEDS = {33: [33010, 33046, 33051], 34: [34000, 34001, 34002], 35: [35001, 35002, 35003], 36: [36000, 36002, 36003],
               37: [37000, 37001, 37004], 38: [38000, 38001, 38002], 39: [39000, 39001, 39002], 40: [40000, 40001, 40002],
               41: [41000, 41001, 41002]}
DENOVO_LENGTHS = [1024, 1500, 2049, 4096, 4097]
MAX_QLEN = 4096          # VSX_CHIMERA_MAX_QLEN (include/vsx_search.h)


def subst(rng, s, rate):
    return "".join(rng.choice([b for b in "ACGT" if b != c]) if rng.random() < rate else c for c in s)


def _put(s, pos, ch):
    return s[:pos] + ch + s[pos + len(ch):]


def breakpoint(L):
    if L < 300:
        return L // 2
    return 256 * max(1, round(L / 512)) + (L % 3) - 1


def family(L):
    rng = random.Random(7000 + L)
    anc = common.rnd_seq(rng, L + 40)
    bp = breakpoint(L)
    parents = []
    for k in range(8):
        p = subst(rng, anc, 0.05) if k < 5 else common.mutate(rng, anc, 0.05)
        if k >= 2:
            p = p[:rng.randint(L, min(len(p), L + 40))]
        parents.append(p)
    e = rng.randint(5, 30)
    parents[2] = _put(_put(_put(parents[2], bp - 3, "N"), bp + 2, "R"), max(0, bp - 7), "Y")
    a, b, c, d, f = parents[:5]
    qs = {"chim2": a[:bp] + b[bp:L], "chim3": a[:L // 3] + d[L // 3:2 * L // 3] + b[2 * L // 3:L], "plain": subst(rng, f[:L], 0.01),
          "overhang": a[e:bp + e] + b[bp + e:L + e]}
    amb = c[:bp] + b[bp:L]
    qs["ambig"] = _put(_put(_put(amb, bp - 2, "N"), bp + 1, "Y"), min(L - 1, bp + 4), "R")
    # diagnostic columns of parents 3 | 4 on either side of the breakpoint
    left = [i for i in range(8, bp - 8) if d[i] != f[i]]
    right = [i for i in range(bp + 8, L - 8) if d[i] != f[i]]
    ind = d[:bp] + f[bp:L]
    if left and right:
        i, j = left[len(left) // 2], right[len(right) // 2]
        ind = ind[:i + 1] + ind[i + 4:j] + common.rnd_seq(rng, 3) + ind[j:]
    qs["indel"] = ind
    assert all(len(q) == L for q in qs.values()), {k: len(q) for k, q in qs.items()}
    assert all(L <= len(p) <= L + 40 for p in parents)
    return [f"L{L}_p{k}" for k in range(8)], parents, [f"L{L}_{k}" for k in qs], list(qs.values())


def all_lengths():
    """(parent labels, parents, query labels, queries) of every kernel and host-route length in one database: the families are
    unrelated to each other, so each query meets its own family only"""
    tn, db, qn, qs = [], [], [], []
    for L in KERNEL_LENGTHS + EXTRA_LENGTHS + HOST_LENGTHS:
        for dst, src in zip((tn, db, qn, qs), family(L)):
            dst.extend(src)
    return tn, db, qn, qs


def short_lengths():
    """(parent labels, parents, query labels, queries) for L = 33 .. 41 (2 .. 10 windows of 32 columns): per length three pairs of
    unrelated parents of exactly L symbols and the chimera of their halves, a database of their own"""
    tn, db, qn, qs = [], [], [], []
    for L, seeds in SHORT_SEEDS.items():
        for seed in seeds:
            rng = random.Random(seed)
            a, b = common.rnd_seq(rng, L), common.rnd_seq(rng, L)
            tn += [f"S{L}_{seed}_a", f"S{L}_{seed}_b"]
            db += [a, b]
            qn.append(f"S{L}_{seed}")
            qs.append(a[:L // 2] + b[L // 2:])
    return tn, db, qn, qs


def sixteen_candidates(L):
    """-> (labels, database, query): 16 references, four per quarter of the query, each >= 97 % identical to the query inside its
    quarter and unrelated outside, so each of the four part searches returns four distinct targets"""
    rng = random.Random(1600 + L)
    q = common.rnd_seq(rng, L)
    cut = [L * k // 4 for k in range(5)]
    db = []
    for part in range(4):
        for m in range(4):
            own = subst(rng, q[cut[part]:cut[part + 1]], 0.005 + 0.006 * m)
            db.append(common.rnd_seq(rng, cut[part]) + own + common.rnd_seq(rng, L - cut[part + 1]))
    return [f"c16_{L}_r{k}" for k in range(16)], db, q


def two_relatives(L):
    """-> (labels, database, query): two related parents and six unrelated sequences; the query is a chimera of the two"""
    rng = random.Random(200 + L)
    anc = common.rnd_seq(rng, L + 20)
    a, b = subst(rng, anc, 0.05), subst(rng, anc, 0.05)
    db = [a, b] + [common.rnd_seq(rng, L + rng.randint(0, 40)) for _ in range(6)]
    order = [3, 0, 5, 6, 1, 2, 4, 7]
    return [f"two_{L}_r{k}" for k in range(8)], [db[k] for k in order], a[:L // 2] + b[L // 2:L]


MASKS = {"default": [], "none": ["--qmask", "none", "--dbmask", "none"]}      # the mask modes of the --uchime_ref runs
VARIANTS = ["uchime", "uchime2", "uchime3"]


def reference_lines(tmp):
    """The reference CLI's --uchimeout lines (--threads 1) for everything the length tests compare, the commands side by side:
    {mask mode: all_lengths(), "short_" + mask mode: short_lengths(), variant: denovo_set()}.  tmp: an empty directory."""
    import os
    from concurrent.futures import ThreadPoolExecutor

    from tests import denovo_data
    from tests.test_gpu_chimera import _ref_lines
    tn, db, qn, qs = all_lengths()
    stn, sdb, sqn, sqs = short_lengths()
    labels, seqs = denovo_set()
    jobs = {}
    for m, extra in MASKS.items():
        jobs[m] = lambda d, extra=extra: _ref_lines(d, qn, qs, tn, db, extra)
        jobs["short_" + m] = lambda d, extra=extra: _ref_lines(d, sqn, sqs, stn, sdb, extra)
    for v in VARIANTS:
        jobs[v] = lambda d, v=v: denovo_data.ref_lines(d, labels, seqs, v)
    dirs = {k: os.path.join(tmp, k) for k in jobs}
    for d in dirs.values():
        os.mkdir(d)
    with ThreadPoolExecutor(len(jobs)) as pool:
        futures = {k: pool.submit(f, dirs[k]) for k, f in jobs.items()}
        return {k: f.result() for k, f in futures.items()}


def denovo_set():
    """(labels with ;size=, sequences): the parents and the chimeras of DENOVO_LENGTHS, the parents far more abundant than the
    chimeras, so every chimera finds its parents among the sequences already classified"""
    labels, seqs = [], []
    for L in DENOVO_LENGTHS:
        tn, db, qn, qs = family(L)
        for k, (n, s) in enumerate(zip(tn, db)):
            labels.append(f"{n};size={900 - 10 * k}")
            seqs.append(s)
        for k, (n, s) in enumerate(zip(qn, qs)):
            labels.append(f"{n};size={9 - k}")
            seqs.append(s)
    return labels, seqs
