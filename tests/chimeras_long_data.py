"""Inputs of the --chimeras_denovo tests (tests/test_chimeras_long_*.py, tests/test_gpu_chimeras_denovo.py) and of
tests/golden/chimeras_long_golden.json.

seeded_set(): families of 150-450 bp (a handful at 1 500 bp), two- and three-parent chimeras of their members joined at exact
breakpoints (the detector looks for exact regions), each chimera no more abundant than its parents, in a shuffled input order; one
family is longer than the kernel's query limit.

edge_cases(): named small inputs, most of them "mosaics".  mosaic(cuts) takes a random sequence A and makes one variant per
segment [cuts[k], cuts[k + 1]): variant k equals A on its own segment and carries substitutions just outside it and in the middle of
every other segment, so that the query A itself is tiled by exactly one region per variant, region k = segment k, all alignments
being gapless.  Every variant also carries a substitution no other sequence has, so no variant is a chimera of the others.

    python -m tests.chimeras_long_data     rewrites the golden file with the reference CLI (oracle/_ref/vsearch_ref)"""
import json
import os
import random

from tests import common

GOLDEN = os.path.join(common.GOLD, "chimeras_long_golden.json")
QMAX, CMAX = 2048, 64          # VSX_CHIMERAS_LONG_MAX_QLEN, VSX_CHIMERAS_LONG_MAX_CAND (asserted against the library in the host test)


def _sub(ch, shift):
    return "ACGT"[("ACGT".index(ch) + shift) % 4]


def mosaic(rng, cuts, size=10):
    """(labels, seqs, A): one variant per segment; A is the sequence the variants tile"""
    L, m = cuts[-1], len(cuts) - 1
    a = common.rnd_seq(rng, L)
    labels, seqs = [], []
    for k in range(m):
        v = list(a)
        marks = {cuts[j] + (cuts[j + 1] - cuts[j]) // 2 for j in range(m) if j != k}
        marks |= {p for p in (cuts[k] - 1, cuts[k + 1]) if 0 <= p < L}
        for p in marks:
            v[p] = _sub(a[p], 1 + k % 3)
        labels.append(f"v{k:02d};size={size}")
        seqs.append("".join(v))
    return labels, seqs, a


def _edit(s, pos, ch):
    return s[:pos] + ch + s[pos + 1:]


def _even(L, m):
    return [L * k // m for k in range(m + 1)]


def edge_cases():
    """name -> dict(labels, seqs, opts (session keywords), cli (the reference's options), expect).  expect: chimeric = labels that
    must be 'Y', clean = labels that must not be; parents = label -> the parent fields of its --tabbedout line"""
    rng = random.Random(4242)
    cases = {}

    def add(name, labels, seqs, expect, **opts):
        cli = []
        for k, v in opts.items():
            cli += [{"parts": "--chimeras_parts", "parents_max": "--chimeras_parents_max", "length_min": "--chimeras_length_min",
                     "diff_pct": "--chimeras_diff_pct", "abskew": "--abskew"}[k], str(v)]
        cases[name] = dict(labels=list(labels), seqs=list(seqs), opts=opts, cli=cli, expect=expect)

    # the part-count steps: (length + 99) / 100 within 2 .. 100; lengths 1 and 2 have fewer symbols than parts
    labels, seqs, chim = [], [], []
    for L in (99, 100, 101, 200, 201):
        lb, sq, a = mosaic(rng, _even(L, 2))
        labels += [f"L{L}{x}" for x in lb] + [f"L{L}q;size=1"]
        seqs += sq + [a]
        chim.append(f"L{L}q;size=1")
    labels += ["one;size=3", "two;size=3", "one_again;size=1", "two_again;size=1"]
    seqs += ["A", "AC", "A", "AC"]
    add("lengths", labels, seqs, dict(chimeric=chim, clean=["one;size=3", "two;size=3", "one_again;size=1", "two_again;size=1"]))

    # --chimeras_parts 2, 7 and 100 on a 300 bp query (3 bp parts: shorter than a word)
    lb, sq, a = mosaic(rng, _even(300, 2))
    for parts in (2, 7, 100):
        add(f"parts{parts}", lb + ["q;size=1"], sq + [a], dict(chimeric=["q;size=1"]), parts=parts)

    # the second region is exactly length_min - 1, length_min, length_min + 1 (length_min 10)
    for n in (9, 10, 11):
        lb, sq, a = mosaic(rng, [0, 300 - n, 300])
        add(f"region{n}", lb + ["q;size=1"], sq + [a], dict(chimeric=["q;size=1"]) if n >= 10 else dict(clean=["q;size=1"]))

    # two candidates with the same longest region: w equals v01 on its segment and differs from it elsewhere
    lb, sq, a = mosaic(rng, _even(300, 2))
    w = _edit(sq[1], 31, _sub(sq[1][31], 2))
    add("tie_candidates", lb + ["w;size=10", "q;size=1"], sq + [w, a], dict(chimeric=["q;size=1"]))

    # equal regions within one candidate and a position nobody covers: the query differs from every variant at position 100 (a
    # substitution no variant carries), which cuts v00's segment [0, 201) into two regions of 100; three regions are found
    lb, sq, a = mosaic(rng, [0, 201, 300])
    q = _edit(a, 100, _sub(a[100], 3))
    add("tie_within_uncovered", lb + ["q;size=1"], sq + [q], dict(clean=["q;size=1"]))
    lb, sq, a = mosaic(rng, _even(300, 2))
    add("uncovered", lb + ["q;size=1"], sq + [_edit(a, 60, _sub(a[60], 2))], dict(clean=["q;size=1"]))

    # one parent, one insertion in front of position 200: round 1 takes [0, 200), the position after the insertion is skipped in that
    # round and starts the segment [200, 299) of round 2: 'Y' with parent A = parent B
    a = common.rnd_seq(rng, 300)
    add("one_parent_twice", ["a;size=10", "other;size=10", "q;size=1"], [a, common.rnd_seq(rng, 300), a[:200] + a[201:]],
        dict(chimeric=["q;size=1"], parents={"q;size=1": ["a;size=10", "a;size=10", "*"]}))
    # the same with the insertion in the first half: the first round takes the second segment and position 100 is never covered
    add("one_parent_uncovered", ["a;size=10", "other;size=10", "q;size=1"], [a, common.rnd_seq(rng, 300), a[:100] + a[101:]],
        dict(clean=["q;size=1"]))

    # an insertion in front of position 0 and one after the last position
    lb, sq, a = mosaic(rng, _even(300, 2))
    add("insertion_front", lb + ["q;size=1"], sq + [a[1:]], dict(chimeric=["q;size=1"]))
    add("insertion_back", lb + ["q;size=1"], sq + [a[:-1]], dict(chimeric=["q;size=1"]))

    # 2, 3, 4 and 20 parents under --chimeras_parents_max 2, 3 and 20; the fourth field is '*' with two parents
    for m in (2, 3, 4, 20):
        lb, sq, a = mosaic(rng, _even(300, m))
        for pmax in (2, 3, 20):
            exp = dict(chimeric=["q;size=1"]) if m <= pmax else dict(clean=["q;size=1"])
            if m <= pmax:
                exp["parents"] = {"q;size=1": [lb[0], lb[1], lb[2] if m > 2 else "*"]}
            opts = dict(parents_max=pmax)
            if m == 20:
                opts["parts"] = 20               # one part per segment: every variant is the best hit of its own part
            add(f"parents{m}_max{pmax}", lb + ["q;size=1"], sq + [a], exp, **opts)

    # --chimeras_diff_pct: two variants of 600, each exact on its half and with a substitution at every 20th position of the other
    # half, and a query that differs from both at position 50.  At 0 and 0.1 position 50 stays uncovered (one mismatch costs more
    # than 299 matches earn at 0.1); at 1 and 2.5 the first region runs over that mismatch and ends a little behind the breakpoint,
    # where the substitutions cost more than the matches between them earn, and the second variant is still needed for the rest:
    # 'Y' with two parents.  1 and 2.5 are multiples of 2^-13 (the kernel's scan), 0.1 is not (host restatement)
    a = common.rnd_seq(rng, 600)
    sq = []
    for k in range(2):
        v = list(a)
        for p in range(300 * (1 - k) + 10, 300 * (2 - k), 20):
            v[p] = _sub(a[p], 1 + k)
        v[299 + k] = _sub(a[299 + k], 1 + k)
        sq.append("".join(v))
    q = _edit(a, 50, _sub(a[50], 3))
    for pct in (0, 1, 2.5, 0.1):
        exp = dict(clean=["q;size=1"]) if pct in (0, 0.1) else dict(chimeric=["q;size=1"], parents={"q;size=1": ["v00;size=10", "v01;size=10", "*"]})
        exp["clean"] = exp.get("clean", []) + ["v00;size=10", "v01;size=10"]
        add(f"diff_pct{pct}", ["v00;size=10", "v01;size=10", "q;size=1"], sq + [q], exp, diff_pct=pct)

    # ambiguity codes: selection matches by a non-zero AND of the codes, evaluation by equal codes
    lb, sq, a = mosaic(rng, _even(300, 2))
    a = _edit(a, 70, "A")
    sq = [_edit(s, 70, "R") if k == 0 else _edit(s, 70, "A") for k, s in enumerate(sq)]
    add("ambiguity", lb + ["q;size=1"], sq + [_edit(a, 40, "N")], dict(chimeric=["q;size=1"]))

    # the kernel's limits +- 1: query length ...
    for L in (QMAX - 1, QMAX, QMAX + 1):
        lb, sq, a = mosaic(rng, _even(L, 2))
        add(f"qlen{L}", lb + ["q;size=1"], sq + [a], dict(chimeric=["q;size=1"]))
    # ... and candidates: the query has 17 parts of 100; variant v is the query with every second symbol substituted (50 % identity,
    # no shared word: never a hit, and its gapless alignment is the best one) except on part v % 17, which it carries exactly (the
    # first variant of a part) or with one substitution; so every part accepts its own variants and nothing else: m variants = m
    # candidates, and the first 17 tile the query
    for m in (CMAX - 1, CMAX, CMAX + 1):
        a = common.rnd_seq(rng, 1700)
        lb, sq = [], []
        for v in range(m):
            part, r = v % 17, v // 17
            body = "".join(_sub(ch, 1 + v % 3) if (i + v) % 2 == 0 else ch for i, ch in enumerate(a))
            own = a[100 * part:100 * part + 100]
            if r:
                own = _edit(own, 20 * r, _sub(own[20 * r], r))
            lb.append(f"v{v:02d};size=10")
            sq.append(body[:100 * part] + own + body[100 * part + 100:])
        add(f"cand{m}", lb + ["q;size=1"], sq + [a], dict(chimeric=["q;size=1"]), parents_max=20)
    return cases


def _chimera(rng, parents):
    n = min(len(p) for p in parents)
    cuts = sorted(rng.sample(range(n // 6, n - n // 6), len(parents) - 1))
    edges = [0] + cuts + [None]
    return "".join(p[edges[i]:edges[i + 1]] for i, p in enumerate(parents))


def seeded_set(seed=31, n_families=24, members=(3, 7), n_chimeras=70, n_long=4, length=(150, 450)):
    """(labels, sequences) in a shuffled input order: fewer than 300 sequences.  length: the range of the families' lengths (the
    default is the golden set's)"""
    rng = random.Random(seed)
    seqs, sizes = [], []
    good = []
    for f in range(n_families):
        anc = common.rnd_seq(rng, rng.randint(*length))
        for m in range(rng.randint(*members)):
            good.append(common.mutate(rng, anc, 0.03))
    lanc = common.rnd_seq(rng, 1500)
    longs = [common.mutate(rng, lanc, 0.03) for _ in range(n_long)]
    xanc = common.rnd_seq(rng, QMAX + 60)                      # longer than the kernel takes: host restatement inside the passes
    longs += [common.mutate(rng, xanc, 0.03) for _ in range(3)]
    pool = good + longs
    ranks = list(range(1, len(pool) + 1))
    rng.shuffle(ranks)
    for g, r in zip(pool, ranks):
        seqs.append(g)
        sizes.append(max(2, int(3000 / r ** 1.1)))
    n_good = len(good)
    for i in range(n_chimeras):
        k = 2 if i % 3 else 3
        if i % 10 == 9:
            ps = [n_good + x for x in rng.sample(range(n_long), k)]
        elif i % 10 == 4:
            ps = [n_good + n_long + x for x in rng.sample(range(3), k)]
        else:
            fam = rng.sample(range(n_good), k)
            ps = fam
        c = _chimera(rng, [seqs[p] for p in ps])
        if i % 7 == 3:
            c = common.mutate(rng, c, 0.004)           # a few noisy ones: regions interrupted, mostly not chimeric at diff_pct 0
        seqs.append(c)
        sizes.append(rng.randint(1, max(1, min(sizes[p] for p in ps))))
    # soft-masked stretches and a low-complexity tail (the --qmask modes differ on them)
    for i in range(6):
        g = good[rng.randrange(n_good)]
        seqs.append(g[:60] + g[60:120].lower() + g[120:] + "AC" * 20)
        sizes.append(rng.randint(1, 30))
    labels = [f"s{i};size={z}" for i, z in enumerate(sizes)]
    order = list(range(len(seqs)))
    rng.shuffle(order)
    return [labels[i] for i in order], [seqs[i] for i in order]


def _fasta_labels(path):
    return [ln[1:].rstrip("\n") for ln in open(path) if ln.startswith(">")]


def case_digest(labels, seqs):
    """what the golden file keeps of an edge case's input (the generator is seeded; the digest shows a drift)"""
    import hashlib
    return hashlib.sha256("\n".join(list(labels) + list(seqs)).encode()).hexdigest()[:16]


def ref_outputs(tmp, labels, seqs, extra=()):
    """the reference CLI's --tabbedout lines and the labels of its --chimeras / --nonchimeras files, one thread"""
    from oracle import refcli
    f = os.path.join(tmp, "in.fa")
    to, ch, nc = (os.path.join(tmp, x) for x in ("t.tsv", "ch.fa", "nc.fa"))
    refcli.write_fasta(f, labels, seqs)
    refcli.run(["--chimeras_denovo", f, "--tabbedout", to, "--chimeras", ch, "--nonchimeras", nc, "--threads", "1", "--quiet"] + list(extra))
    return dict(tabbedout=open(to).read().splitlines(), chimeras=_fasta_labels(ch), nonchimeras=_fasta_labels(nc))


def write_golden():
    import tempfile
    labels, seqs = seeded_set()
    out = {"seeded": dict(labels=labels, seqs=seqs), "edges": {}}
    with tempfile.TemporaryDirectory() as tmp:
        out["seeded"].update(ref_outputs(tmp, labels, seqs))
        for name, c in edge_cases().items():
            out["edges"][name] = dict(ref_outputs(tmp, c["labels"], c["seqs"], c["cli"]), digest=case_digest(c["labels"], c["seqs"]))
    with open(GOLDEN, "w") as fh:
        json.dump(out, fh, indent=0)
        fh.write("\n")


if __name__ == "__main__":
    write_golden()
