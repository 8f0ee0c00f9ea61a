"""Inputs of the de novo chimera tests (tests/test_gpu_uchime_denovo.py) and of tests/golden/uchime_denovo_golden.json.

cascade_set(): a seeded family set with Zipf-like abundances and two- / three-parent chimeras, some of them abundant enough to be
candidate parents of later chimeras (so that a status found late in a window changes the candidate lists of later members), plus
abundance ties, duplicate labels, sequences shorter than 4 and than 32, N-rich and low-complexity sequences, sequences longer than
VSX_CHIMERA_MAX_QLEN with chimeras of them, and an abundant sequence equal to one quarter of a rarer one (--selfid).

    python -m tests.denovo_data     rewrites the golden file with the reference CLI (oracle/_ref/vsearch_ref)"""
import json
import os
import random

from tests import common

GOLDEN = os.path.join(common.GOLD, "uchime_denovo_golden.json")


def _chimera(rng, parents):
    n = min(len(p) for p in parents)
    cuts = sorted(rng.sample(range(n // 6, n - n // 6), len(parents) - 1))
    edges = [0] + cuts + [None]
    return common.mutate(rng, "".join(p[edges[i]:edges[i + 1]] for i, p in enumerate(parents)), 0.004)


def cascade_set(seed=77, n_families=400, members=(2, 8), n_chimeras=None, extras=True, length=(300, 500)):
    """(labels, sequences) in input order (not sorted); length: the range of the families' ancestor lengths"""
    rng = random.Random(seed)
    seqs, sizes, names = [], [], []

    def add(s, size, name=None):
        names.append(name or f"u{len(seqs)}")
        seqs.append(s)
        sizes.append(size)

    good = []
    for f in range(n_families):
        anc = common.rnd_seq(rng, rng.randint(*length))
        for m in range(rng.randint(*members)):
            good.append(common.mutate(rng, anc, 0.02))
    ranks = list(range(1, len(good) + 1))
    rng.shuffle(ranks)
    for g, r in zip(good, ranks):
        add(g, max(1, int(5000 / r ** 1.1)))
    n_chim = n_chimeras if n_chimeras is not None else len(good) // 4
    gsz = list(sizes)
    chim = []
    for i in range(n_chim):
        k = 2 if i % 3 else 3
        ps = rng.sample(range(len(good)), k)
        c = _chimera(rng, [good[p] for p in ps])
        top = max(1, min(gsz[p] for p in ps) // 2)
        chim.append(len(seqs))
        add(c, rng.randint(max(1, top // 2), top))
    # chimeras of chimeras: abundant chimeras are candidate parents of later, rarer ones
    for i in range(n_chim // 3):
        a, b = rng.sample(chim, 2)
        c = _chimera(rng, [seqs[a], seqs[b]])
        add(c, max(1, min(sizes[a], sizes[b]) // 3))
    if extras:
        # abundance ties, equal labels included (sortbyabundance falls back to the input order)
        for i in range(12):
            s = common.mutate(rng, good[rng.randrange(len(good))], 0.01)
            add(s, 7, "tie;size=7" if i % 3 == 0 else f"tie{i % 4};size=7")
        # duplicate labels (--self: equal headers mean equal abundances, so it decides only where abskew lets equals through)
        for i in range(6):
            g = rng.randrange(len(good))
            add(common.mutate(rng, good[g], 0.005), 5, f"dup{i % 2};size=5")
            add(_chimera(rng, [good[g], good[rng.randrange(len(good))]]), 5, f"dup{i % 2};size=5")
        # very short, N-rich and low-complexity sequences
        for i in range(8):
            add(common.rnd_seq(rng, rng.randint(1, 3)), rng.randint(1, 40))
            add(common.rnd_seq(rng, rng.randint(4, 31)), rng.randint(1, 40))
            add("N" * rng.randint(40, 300), rng.randint(1, 40))
            add(common.mutate(rng, good[rng.randrange(len(good))], 0.05, "ACGTNRY"), rng.randint(1, 40))
            add("AC" * rng.randint(60, 200) + common.rnd_seq(rng, 50) + "T" * rng.randint(30, 90), rng.randint(1, 40))
            add(good[rng.randrange(len(good))][:200] + "acgt" * 30 + "A" * 60, rng.randint(1, 40))
        # longer than VSX_CHIMERA_MAX_QLEN: a long family and chimeras of it (host restatement inside the passes)
        lanc = common.rnd_seq(rng, 4600)
        longs = [common.mutate(rng, lanc, 0.02) for _ in range(3)]
        for j, s in enumerate(longs):
            add(s, 400 - 50 * j)
        for j in range(3):
            add(_chimera(rng, rng.sample(longs, 2)), 20 + j)
        # an abundant sequence equal to one quarter (the first part) of a rarer query: --selfid compares the part with the target
        for j in range(3):
            q = _chimera(rng, rng.sample(good, 2))
            q = q[:len(q) // 4 * 4]
            add(q[:len(q) // 4], 3000 + j)
            add(q, 2)
    labels = [n if ";size=" in n else f"{n};size={z}" for n, z in zip(names, sizes)]
    order = list(range(len(seqs)))
    rng.shuffle(order)
    return [labels[i] for i in order], [seqs[i] for i in order]


def golden_set():
    return cascade_set(seed=5, n_families=25, members=(2, 8), extras=True)


def ref_lines(tmp, labels, seqs, variant="uchime", extra=()):
    from oracle import refcli
    f, uo = os.path.join(tmp, "in.fa"), os.path.join(tmp, "u.tsv")
    refcli.write_fasta(f, labels, seqs)
    refcli.run([f"--{variant}_denovo", f, "--uchimeout", uo, "--threads", "1", "--quiet"] + list(extra))
    return open(uo).read().splitlines()


def write_golden():
    import tempfile
    labels, seqs = golden_set()
    out = {"labels": labels, "seqs": seqs, "uchimeout": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for v in ("uchime", "uchime2", "uchime3"):
            out["uchimeout"][v] = ref_lines(tmp, labels, seqs, v)
    with open(GOLDEN, "w") as fh:
        json.dump(out, fh, indent=0)
        fh.write("\n")


if __name__ == "__main__":
    write_golden()
