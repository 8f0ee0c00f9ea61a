"""Sequences with low-complexity and soft-masked stretches for the masking tests (tests/test_gpu_mask.py, tests/poison_cases.py)."""
from tests import common

COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "a": "t", "c": "g", "g": "c", "t": "a", "N": "N", "R": "Y", "Y": "R"}


def low_complexity(rng, n):
    p = rng.choice([1, 2, 3, 4])
    u = "".join(rng.choice("ACGT") for _ in range(p))
    return (u * (n // p + 1))[:n]


def masked_families(rng, n_families, members, length, div, lower_case):
    """families whose ancestors carry low-complexity stretches (shared ACROSS families, so unmasked they drag unrelated
    targets into the candidate lists) and, with lower_case, soft-masked stretches of ordinary sequence"""
    shared = [low_complexity(rng, rng.randint(30, 70)) for _ in range(3)]
    db = []
    for _ in range(n_families):
        parts, left = [], length
        while left > 0:
            if rng.random() < 0.35:
                seg = rng.choice(shared)
            else:
                seg = common.rnd_seq(rng, rng.randint(20, 90))
                if lower_case and rng.random() < 0.3:
                    seg = seg.lower()
            parts.append(seg)
            left -= len(seg)
        anc = "".join(parts)
        for _ in range(members):
            m = common.mutate(rng, anc.upper(), div)
            # keep the ancestor's case pattern position by position where the lengths still agree (soft masking is about case)
            if lower_case:
                m = "".join(c.lower() if k < len(anc) and anc[k].islower() else c for k, c in enumerate(m))
            db.append(m)
    return db


def queries(rng, db, n, qlen, div, lower_case):
    qs = []
    for _ in range(n):
        s = db[rng.randrange(len(db))]
        a = rng.randrange(max(1, len(s) - qlen))
        frag = s[a:a + qlen]
        m = common.mutate(rng, frag.upper(), div)
        if lower_case:
            m = "".join(c.lower() if k < len(frag) and frag[k].islower() else c for k, c in enumerate(m))
        qs.append(m)
    return qs
