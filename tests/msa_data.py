"""Drawn clusters and the clustering input of the MSA tests (tests/test_gpu_search.py, tests/poison_cases.py)."""
import random

from tests import common


def cluster_input():
    """-> (sequences, names) of the --cluster_fast --msaout test: eight families of 1 .. 9 members at 2 % or 6 % from their ancestor and
    one member with N / R / Y, shuffled"""
    rng = random.Random(17)
    seqs = []
    for f in range(8):
        anc = common.rnd_seq(rng, rng.randint(150, 200))
        for _ in range(rng.randint(1, 9)):
            seqs.append(common.mutate(rng, anc, rng.choice([0.02, 0.06])))
    seqs.append(common.mutate(rng, seqs[0], 0.03, "ACGTNRY"))
    rng.shuffle(seqs)
    return seqs, [f"s{i:03d}" for i in range(len(seqs))]


def random_cluster(rng, n, clen, alphabet="ACGT", pins=0.03, pdel=0.03, long_ins=False):
    """a centroid and n-1 members with CIGARs drawn directly (member = query, centroid = target: 'D' = symbols only the member has)"""
    cen = "".join(rng.choice(alphabet) for _ in range(clen))
    seqs, cigars = [cen], [None]
    for _ in range(n - 1):
        ops, mem = [], []
        if rng.random() < 0.2:
            k = rng.randint(1, 30 if long_ins else 4); ops.append(("D", k)); mem += [rng.choice(alphabet) for _ in range(k)]
        p = 0
        while p < clen:
            r = rng.random()
            if r < pdel:
                k = min(clen - p, rng.randint(1, 5)); ops.append(("I", k)); p += k
            elif r < pdel + pins and ops and ops[-1][0] != "D":
                k = rng.randint(1, 30 if long_ins else 3); ops.append(("D", k)); mem += [rng.choice(alphabet) for _ in range(k)]
            else:
                k = min(clen - p, rng.randint(1, 40)); ops.append(("M", k))
                mem += [cen[p + j] if rng.random() < 0.9 else rng.choice(alphabet) for j in range(k)]; p += k
        if rng.random() < 0.2 and ops[-1][0] != "D":
            k = rng.randint(1, 6); ops.append(("D", k)); mem += [rng.choice(alphabet) for _ in range(k)]
        merged = []
        for op, k in ops:
            if merged and merged[-1][0] == op:
                merged[-1][1] += k
            else:
                merged.append([op, k])
        cigars.append("".join((str(k) if k > 1 else "") + op for op, k in merged))
        seqs.append("".join(mem))
    return seqs, cigars
