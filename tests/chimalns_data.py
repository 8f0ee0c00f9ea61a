"""Inputs of the --uchimealns tests (tests/test_chimalns_host.py, tests/test_gpu_chimalns.py) and of tests/golden/uchimealns_golden.json.

    py_uchimealns(q, a, b, cigar_a, cigar_b, xn, dn, width)   a plain-Python restatement of the reference's literal loops
                     (core/chimera.cpp:761-875, :1258-1570, :1741-1795), its two-orientation scan and its A / B flip included
    explicit_sets()  named (query, parent A, parent B, CIGAR A, CIGAR B) triples, each built to reach one case; check_cases()
                     asserts from py_uchimealns' answer that it does
    random_triples() seeded (query, A, B) triples around a chimera, CIGARs from the scalar oracle aligner
    golden_sets()    small FASTA inputs of the reference CLI: uchime_ref and the three de novo variants
    run_cli()        --uchimealns at one width plus --chimeras / --nonchimeras / --borderline (--fasta_score --sizeout), --threads 1

    python -m tests.chimalns_data     rewrites the golden file with the reference CLI (oracle/_ref/vsearch_ref)

Two cases the issue lists that no input can reach, so check_cases() asserts what the sets reach instead:
  - an `x` run that reaches alnlen.  The winning branch needs right_yes > right_no >= 0, so at least one column behind best_i votes
    for B and is not ignored; its diff is 'B', which ends the run.
  - an `x` run ended by a lower-cased 'a'.  The run passes only blank and ignored-'A' columns, so that 'a' would be the first counted
    column behind best_i, a vote for A.  There left_yes grows by one and right_no falls by one with everything else unchanged: both
    conditions still hold and both factors of h grow strictly, so that column, not best_i, would hold the maximum."""
import hashlib
import json
import os
import random
import tempfile

from tests import common

GOLDEN = os.path.join(common.GOLD, "uchimealns_golden.json")
WIDTHS = (80, 60, 0)
MAP4 = {"a": 1, "b": 14, "c": 2, "d": 13, "g": 4, "h": 11, "k": 12, "m": 3, "n": 15, "r": 5, "s": 6, "t": 8, "u": 8, "v": 7, "w": 9, "y": 10}


def map4(ch):
    return MAP4.get(ch.lower(), 0)


def upcase(ch):
    return ch.upper() if ch.isalpha() and ch.isascii() else "N"


def parse_cigar(c):
    out, n = [], ""
    for ch in c:
        if ch.isdigit():
            n += ch
        else:
            out.append((ch, int(n) if n else 1))
            n = ""
    return out


def py_uchimealns(q, a, b, cigar_a, cigar_b, xn=8.0, dn=1.4, width=80):
    """-> dict: scored, reverse, alnlen, best_i, h, counts (left y n a, right y n a of the winning branch), rows (A, Q, B, Diffs, Votes,
    Model as the reference PRINTS them: A is the second parent when the reverse branch won) and lines [(end A, end Q, end B)]"""
    L = len(q)
    t, cig = (a, b), (parse_cigar(cigar_a), parse_cigar(cigar_b))
    maxi = [0] * (L + 1)
    for p in range(2):
        pos = 0
        for op, n in cig[p]:
            if op == "I":
                maxi[pos] = max(n, maxi[pos])
            else:
                pos += n
    alnlen = L + sum(maxi)
    paln = []
    for p in range(2):
        aln, inserted, qpos, tpos = [], False, 0, 0
        for op, n in cig[p]:
            if op == "I":
                for j in range(maxi[qpos]):
                    if j < n:
                        aln.append(upcase(t[p][tpos]))
                        tpos += 1
                    else:
                        aln.append("-")
                inserted = True
            else:
                for j in range(n):
                    if not inserted:
                        aln += ["-"] * maxi[qpos]
                    if op == "M":
                        aln.append(upcase(t[p][tpos]))
                        tpos += 1
                    else:
                        aln.append("-")
                    qpos += 1
                    inserted = False
        if not inserted:
            aln += ["-"] * maxi[qpos]
        assert len(aln) == alnlen and tpos == len(t[p]) and qpos == L, (len(aln), alnlen)
        paln.append(aln)
    qaln = []
    for i in range(L):
        qaln += ["-"] * maxi[i] + [upcase(q[i])]
    qaln += ["-"] * maxi[L]
    ignore, diffs = [False] * alnlen, [" "] * alnlen
    for i in range(alnlen):
        qs, p1, p2 = map4(qaln[i]), map4(paln[0][i]), map4(paln[1][i])
        if qs == 0 or p1 == 0 or p2 == 0:
            ignore[i] = True
            if i > 0:
                ignore[i - 1] = True
            if i < alnlen - 1:
                ignore[i + 1] = True
        if any(s not in (1, 2, 4, 8) for s in (qs, p1, p2)):
            ignore[i] = True
        if p1 != 0 and p1 != qs:
            paln[0][i] = paln[0][i].lower()
        if p2 != 0 and p2 != qs:
            paln[1][i] = paln[1][i].lower()
        if qs != 0 and p1 != 0 and p2 != 0:
            if p1 == p2:
                diffs[i] = " " if qs == p1 else "N"
            else:
                diffs[i] = "A" if qs == p1 else ("B" if qs == p2 else "?")
    sumA = sum(1 for i in range(alnlen) if not ignore[i] and diffs[i] == "A")
    sumB = sum(1 for i in range(alnlen) if not ignore[i] and diffs[i] == "B")
    sumN = sum(1 for i in range(alnlen) if not ignore[i] and diffs[i] not in "AB ")
    ln = la = ly = 0
    rn, ra, ry = sumA, sumN, sumB
    best_h, best_i, rev, counts, ties = -1.0, -1, False, None, 0
    for i in range(alnlen):
        if ignore[i] or diffs[i] == " ":
            continue
        d = diffs[i]
        if d == "A":
            ly += 1
            rn -= 1
        elif d == "B":
            ln += 1
            ry -= 1
        else:
            la += 1
            ra -= 1
        if ly > ln and ry > rn:
            h = (ly / ((xn * (ln + dn)) + la)) * (ry / ((xn * (rn + dn)) + ra))
            if h == best_h:
                ties += 1
            if h > best_h:
                best_h, best_i, rev, counts, ties = h, i, False, (ly, ln, la, ry, rn, ra), 0
        elif ln > ly and rn > ry:
            h = (ln / ((xn * (ly + dn)) + la)) * (rn / ((xn * (ry + dn)) + ra))
            if h == best_h:
                ties += 1
            if h > best_h:
                best_h, best_i, rev, counts, ties = h, i, True, (ln, ly, la, rn, ry, ra), 0
    res = dict(scored=best_h >= 0.0, reverse=rev, alnlen=alnlen, best_i=best_i, h=best_h, counts=counts, ties=ties, maxi=maxi,
               ignore=ignore)
    if not res["scored"]:
        return res
    if rev:
        diffs = [{"A": "B", "B": "A"}.get(d, d) for d in diffs]
    votes, model = [" "] * alnlen, [" "] * alnlen
    for i in range(alnlen):
        m = "A" if i <= best_i else "B"
        model[i] = m
        v = " "
        if not ignore[i]:
            d = diffs[i]
            if d in "AB":
                v = "+" if d == m else "!"
            elif d in "N?":
                v = "0"
        votes[i] = v
        if v == "!":
            diffs[i] = diffs[i].lower()
    xlen = 0
    for i in range(best_i + 1, alnlen):
        if diffs[i] in " A":
            model[i] = "x"
            xlen += 1
        else:
            break
    w0 = width if width > 0 else alnlen
    qpos = p1pos = p2pos = 0
    lines = []
    for i in range(0, alnlen, w0):
        w = min(alnlen - i, w0)
        qpos += sum(1 for c in qaln[i:i + w] if c != "-")
        p1pos += sum(1 for c in paln[0][i:i + w] if c != "-")
        p2pos += sum(1 for c in paln[1][i:i + w] if c != "-")
        lines.append((p2pos, qpos, p1pos) if rev else (p1pos, qpos, p2pos))
    ia, ib = (1, 0) if rev else (0, 1)
    # the record's fields (chimera.cpp:1577-1631), parents numbered 0 (A as printed) and 1
    mqa = mqb = mab = mqm = cols = 0
    for i in range(alnlen):
        if ignore[i]:
            continue
        cols += 1
        qs, as_, bs = map4(qaln[i]), map4(paln[ia][i]), map4(paln[ib][i])
        ms = as_ if i <= best_i else bs
        mqa += qs == as_
        mqb += qs == bs
        mab += as_ == bs
        mqm += qs == ms
    QA, QB, AB, QM = 100.0 * mqa / cols, 100.0 * mqb / cols, 100.0 * mab / cols, 100.0 * mqm / cols
    QT = max(QA, QB)
    res["rec"] = dict(score=best_h, parent_a=0, parent_b=1, closest=0 if QA >= QB else 1, status="scored", id_query_model=QM, id_query_a=QA,
                      id_query_b=QB, id_a_b=AB, id_query_top=QT, left_yes=counts[0], left_no=counts[1], left_abstain=counts[2],
                      right_yes=counts[3], right_no=counts[4], right_abstain=counts[5], divergence=QM - QT, flag="Y")
    res.update(rows=tuple("".join(r) for r in (paln[ia], qaln, paln[ib], diffs, votes, model)), lines=lines, xlen=xlen)
    return res


# ---- explicit triples ------------------------------------------------------------------------------------------------------------

def derive(q, edits):
    """a parent of q and the CIGAR of (q against it).  edits: {query position: ('sub', base) | ('ins', text) | ('del', n)}; 'ins' puts
    text in front of the position (position len(q): behind the end), 'del' leaves n query symbols out of the parent"""
    t, ops, i = [], [], 0

    def push(op, n):
        if ops and ops[-1][0] == op:
            ops[-1][1] += n
        else:
            ops.append([op, n])

    while i <= len(q):
        e = edits.get(i)
        if e and e[0] == "ins":
            t.append(e[1])
            push("I", len(e[1]))
            e = edits.get((i, 2))                 # a second edit at the same position, behind the insertion
        if i == len(q):
            break
        if e and e[0] == "del":
            push("D", e[1])
            i += e[1]
            continue
        t.append(e[1] if e and e[0] == "sub" else q[i])
        push("M", 1)
        i += 1
    return "".join(t), "".join(f"{n}{op}" for op, n in ops)


def _other(ch, k=1):
    return "ACGT"[("ACGT".index(ch) + k) % 4]


def _chimera(L, seed, a_edits=None, b_edits=None, a_diffs=None, b_diffs=None, q_edit=None):
    """q of length L; A differs from q at a_diffs (default: three positions of the right half), B at b_diffs (left half): the left
    half votes A, the right half B"""
    rng = random.Random(seed)
    q = list(common.rnd_seq(rng, L))
    for pos, ch in (q_edit or {}).items():
        q[pos] = ch
    q = "".join(q)
    b_diffs = b_diffs if b_diffs is not None else [L // 8, L // 4, 3 * L // 8]
    a_diffs = a_diffs if a_diffs is not None else [5 * L // 8, 3 * L // 4, 7 * L // 8]
    ea = {p: ("sub", _other(q[p]) if q[p] in "ACGT" else "A") for p in a_diffs}
    eb = {p: ("sub", _other(q[p]) if q[p] in "ACGT" else "A") for p in b_diffs}
    ea.update(a_edits or {})
    eb.update(b_edits or {})
    a, ca = derive(q, ea)
    b, cb = derive(q, eb)
    return q, a, b, ca, cb


def explicit_sets():
    """name -> (q, a, b, cigar_a, cigar_b)"""
    S = {}
    S["plain"] = _chimera(120, 1)
    S["ins_a_only"] = _chimera(120, 2, a_edits={50: ("ins", "GG")})
    S["ins_b_only"] = _chimera(120, 3, b_edits={70: ("ins", "TCA")})
    S["ins_both_lengths"] = _chimera(120, 4, a_edits={60: ("ins", "G")}, b_edits={60: ("ins", "TTAC")})
    S["ins_before_0"] = _chimera(120, 5, a_edits={0: ("ins", "ACG")})
    S["ins_after_last"] = _chimera(120, 6, b_edits={120: ("ins", "TT")})
    # a deletion / an insertion column right beside a diff column: the diff is ignored
    S["del_beside_diff"] = _chimera(120, 7, a_edits={31: ("del", 1)}, b_diffs=[15, 30, 40, 45])
    S["ins_beside_diff"] = _chimera(120, 8, a_edits={31: ("ins", "C")}, b_diffs=[15, 30, 40, 45])
    # ambiguous symbols: the differing parent symbol is lower-cased, the vote is blank
    S["n_r_query"] = _chimera(120, 9, q_edit={20: "N", 100: "R"}, a_edits={20: ("sub", "A"), 100: ("sub", "A")},
                              b_edits={20: ("sub", "C"), 100: ("sub", "C")})
    S["n_r_parent"] = _chimera(120, 10, a_edits={20: ("sub", "N")}, b_edits={100: ("sub", "R")})
    # the crossover run: none (a B vote right behind best_i) / carried over an ignored 'A' (an A column beside a gap column)
    S["x_none"] = _chimera(120, 11, b_diffs=[15, 30, 45], a_diffs=[46, 90, 105])
    S["x_over_ignored_a"] = _chimera(120, 13, b_diffs=[15, 30, 45, 70], a_diffs=[80, 90, 105], a_edits={71: ("del", 1)})
    for L in (63, 64, 65, 255, 256, 257):
        S[f"alnlen_{L}"] = _chimera(L, 100 + L)
    S["alnlen_multiple_of_80"] = _chimera(158, 20, a_edits={40: ("ins", "GT")})
    S["qlen_32"] = _chimera(32, 21)
    S["qlen_4096"] = _chimera(4096, 22, a_edits={1000: ("ins", "ACGTAC")}, b_edits={3000: ("del", 3)})
    S["many_runs"] = _chimera(700, 23, a_edits={p: ("del", 1) for p in range(5, 690, 9)}, b_edits={p: ("ins", "A") for p in range(7, 690, 11)})
    # two columns of equal h, votes A A N B B (both parents carry the same wrong symbol at 60): the second A and the N column give
    # products of the same two factors
    q = _chimera(120, 14)[0]
    S["tie"] = _chimera(120, 14, b_diffs=[20, 30], a_diffs=[90, 100], a_edits={60: ("sub", _other(q[60], 2))},
                        b_edits={60: ("sub", _other(q[60], 2))})
    return S


HOST_ONLY = {"qlen_4097": lambda: _chimera(4097, 24)}          # beyond the kernel: the device entry refuses it


def check_cases(S=None):
    """every set reaches the case it is named after, judged from py_uchimealns"""
    S = S or explicit_sets()
    R = {k: py_uchimealns(*v) for k, v in S.items()}
    for k, r in R.items():
        assert r["scored"] and not r["reverse"], k
    mx = lambda k: R[k]["maxi"]
    assert R["ins_a_only"]["alnlen"] == 122 and "-" in R["ins_a_only"]["rows"][2] and R["ins_a_only"]["rows"][0].count("-") == 0
    assert R["ins_b_only"]["alnlen"] == 123 and R["ins_b_only"]["rows"][0].count("-") == 3
    assert mx("ins_both_lengths")[60] == 4 and "g---" in R["ins_both_lengths"]["rows"][0]
    assert mx("ins_before_0")[0] == 3 and R["ins_before_0"]["rows"][1].startswith("---")
    assert mx("ins_after_last")[120] == 2 and R["ins_after_last"]["rows"][1].endswith("--")
    for k in ("del_beside_diff", "ins_beside_diff"):
        r = R[k]
        c = [i for i, ch in enumerate(r["rows"][3]) if ch in "AaBb"]
        assert any(r["ignore"][i] and r["rows"][4][i] == " " for i in c), k
    for k, col in (("n_r_query", 20), ("n_r_parent", 20)):
        r = R[k]
        assert r["rows"][4][col] == " " and r["ignore"][col] and (r["rows"][0][col].islower() or r["rows"][2][col].islower()), k
    assert R["x_none"]["xlen"] == 0
    r = R["x_over_ignored_a"]
    seg = r["rows"][3][r["best_i"] + 1:r["best_i"] + 1 + r["xlen"]]
    assert "A" in seg and r["xlen"] > 0
    assert R["tie"]["ties"] >= 1 and R["tie"]["rows"][3][R["tie"]["best_i"]] == "A"
    for L in (63, 64, 65, 255, 256, 257):
        assert R[f"alnlen_{L}"]["alnlen"] == L
    assert R["alnlen_multiple_of_80"]["alnlen"] == 160
    assert len(S["qlen_32"][0]) == 32 and len(S["qlen_4096"][0]) == 4096 and len(HOST_ONLY["qlen_4097"]()[0]) == 4097
    assert S["many_runs"][3].count("D") > 64 and S["many_runs"][4].count("I") > 60          # more than one chunk of 64 run words
    assert all(r["best_i"] + 1 + r["xlen"] < r["alnlen"] for r in R.values())          # (no run reaches alnlen: module docstring)
    return R


def random_triples(n, seed=2024):
    """(q, a, b, cigar_a, cigar_b): a mutated two-parent chimera with indels, ambiguous symbols now and then; CIGARs from the scalar
    oracle aligner.  Triples without an h score are left out."""
    from oracle import pyoracle
    orc = pyoracle.Oracle()
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        L = rng.randint(40, 160)
        anc = common.rnd_seq(rng, L)
        pa, pb = common.mutate(rng, anc, 0.08), common.mutate(rng, anc, 0.08)
        cut = rng.randint(L // 4, 3 * L // 4)
        q = common.mutate(rng, pa[:cut] + pb[cut:], 0.02, "ACGTN" if rng.random() < 0.2 else "ACGT")
        if len(q) < 8:
            continue
        if rng.random() < 0.5:
            pa, pb = pb, pa
        ca, cb = orc.align(q, pa)[5], orc.align(q, pb)[5]
        if py_uchimealns(q, pa, pb, ca, cb)["scored"]:
            out.append((q, pa, pb, ca, cb))
    return out


# ---- reference CLI ---------------------------------------------------------------------------------------------------------------

def ref_set(n_q=8, families=6, members=3, length=130):
    """a small --uchime_ref input: (db labels, db, query labels with ;size=, queries); the defaults are the golden file's"""
    rng = random.Random(31)
    db, _ = common.family_db(rng, families, members, length, div=0.10)
    tn = [f"p{i};size={rng.randint(1, 9)}" for i in range(len(db))]
    qs = []
    for i in range(n_q):
        ps = rng.sample(range(len(db)), 2)
        n = min(len(db[p]) for p in ps)
        cut = rng.randint(n // 4, 3 * n // 4)
        c = db[ps[0]][:cut] + db[ps[1]][cut:]
        qs.append(common.mutate(rng, c, 0.01) if i % 4 else common.mutate(rng, db[ps[0]], 0.03))
    return tn, db, [f"q{i};size={1 + i % 7}" for i in range(len(qs))], qs


def denovo_set():
    from tests import denovo_data
    return denovo_data.cascade_set(seed=3, n_families=6, members=(2, 4), extras=False, length=(90, 120))


def golden_sets():
    tn, db, qn, qs = ref_set()
    dl, dseq = denovo_set()
    return {"uchime_ref": dict(db_labels=tn, db=db, labels=qn, seqs=qs),
            "uchime": dict(labels=dl, seqs=dseq), "uchime2": dict(labels=dl, seqs=dseq), "uchime3": dict(labels=dl, seqs=dseq, abskew=1.5)}


def digest(s):
    return hashlib.sha256(json.dumps({k: v for k, v in sorted(s.items())}, sort_keys=True).encode()).hexdigest()


def run_cli(name, s, width, tmp, extra=()):
    """-> dict(uchimealns=text, chimeras=..., nonchimeras=..., borderline=...) of the reference CLI, --threads 1"""
    from oracle import refcli
    f = os.path.join(tmp, "in.fa")
    refcli.write_fasta(f, s["labels"], s["seqs"])
    out = {k: os.path.join(tmp, k) for k in ("uchimealns", "chimeras", "nonchimeras", "borderline")}
    args = ["--uchimealns", out["uchimealns"], "--alignwidth", str(width), "--chimeras", out["chimeras"], "--nonchimeras", out["nonchimeras"],
            "--fasta_score", "--sizeout", "--threads", "1", "--quiet"] + list(extra)
    if name == "uchime_ref":
        d = os.path.join(tmp, "db.fa")
        refcli.write_fasta(d, s["db_labels"], s["db"])
        args = ["--uchime_ref", f, "--db", d, "--borderline", out["borderline"]] + args
    else:
        args = [f"--{name}_denovo", f] + args
        if name == "uchime":
            args += ["--borderline", out["borderline"]]
        if "abskew" in s:
            args += ["--abskew", str(s["abskew"])]
    refcli.run(args)
    return {k: open(p).read() if os.path.exists(p) else "" for k, p in out.items()}


def write_golden():
    out = {}
    for name, s in golden_sets().items():
        entry = {"digest": digest(s), "uchimealns": {}}
        for w in WIDTHS:
            with tempfile.TemporaryDirectory() as tmp:
                got = run_cli(name, s, w, tmp)
            entry["uchimealns"][str(w)] = got.pop("uchimealns")
            entry.update(got)
        assert entry["uchimealns"]["80"].count("\nQuery   (") >= 3, (name, "too few blocks")
        out[name] = entry
    with open(GOLDEN, "w") as fh:
        json.dump(out, fh, indent=0)
        fh.write("\n")


def load_golden():
    gold = json.load(open(GOLDEN))
    sets = golden_sets()
    for name, s in sets.items():
        assert gold[name]["digest"] == digest(s), f"{name}: the golden file was written for another input"
    return sets, gold


# ---- the kernel on explicit triples ------------------------------------------------------------------------------------------------

def device_triples(aligner, triples, alignwidth=80, xn=8.0, dn=1.4):
    """vsx_internal_chimalns_device: one launch over the triples (each in record order) -> ChimeraAlns"""
    import ctypes as C
    from vsearch_amd import _lib
    from vsearch_amd.chimera import ChimeraAlns, _alns_opts
    lib = _lib.load()
    n = len(triples)
    cols = [[t[k].encode() for t in triples] for k in range(5)]
    strs = [(C.c_char_p * max(n, 1))(*c) for c in cols]
    lens = [(C.c_uint32 * max(n, 1))(*[len(x) for x in c]) for c in cols[:3]]
    o = _alns_opts(xn, dn, alignwidth, "Y", 0, 0)
    res = _lib.ChimalnsOut()
    _lib.check(lib.vsx_internal_chimalns_device(aligner.h, n, strs[0], lens[0], strs[1], lens[1], strs[2], lens[2], strs[3], strs[4],
                                                C.byref(o), C.byref(res)), "vsx_internal_chimalns_device")
    try:
        return ChimeraAlns(res, alignwidth)
    finally:
        lib.vsx_chimalns_out_free(C.byref(res))


def device_digest(aligner):
    """one digest over the kernel's arrays of every explicit set at the four widths and of 200 random triples"""
    h = hashlib.sha256()
    sets = list(explicit_sets().values())
    rnd = []
    for t in random_triples(200, seed=77):
        rnd.append((t[0], t[2], t[1], t[4], t[3]) if py_uchimealns(*t)["reverse"] else t)
    for w in (1, 60, 80, 0):
        ts = [t for t in sets if w != 1 or len(t[0]) <= 1000] + rnd
        res = device_triples(aligner, ts, w)
        if res.stats["records_kernel"] != len(ts):
            raise RuntimeError("the kernel did not answer")
        h.update(repr(res.arrays()).encode())
    return h.hexdigest()


if __name__ == "__main__":
    import sys
    if "--digest" in sys.argv:
        from vsearch_amd import Aligner, load_library
        with Aligner(device=0) as al:
            print("digest", device_digest(al), "poison", load_library().vsx_internal_poison_byte())
    else:
        check_cases()
        write_golden()
        print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
