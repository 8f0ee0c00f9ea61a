"""Data and the plain-Python restatement for the --lcaout tests (tests/test_lca_host.py, tests/test_gpu_lca.py).

py_tax_split() and py_lca_query() restate the reference's literal loops (core/tax.cpp, core/results.cpp:545-687): tax_split with
its quirks, the Boyer-Moore vote per level, the recount, the `1.0 * m / n < cutoff` test, and the text.  The named sets are built
from (labels, hit lists); no search is needed.  tests/golden/lca_golden.json holds what the reference CLI wrote for one small
input (`python -m tests.lca_data --record`, with the CLI that build() makes); `--digest` prints the digest of every set's device
result (the child of the poisoned-memory test).
"""
import hashlib
import importlib
import json
import os
import random
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lca_golden.json")
NONE = 0xFFFFFFFF
LEVELS = 9
RANKS = b"dkpcofgst"
CUTOFFS = (1.0, 0.51, 0.75, 0.6666666666666666, 0.67)
# (lca_cutoff, maxhits, top_hits_only): what every named set runs under
COMBOS = [(c, 0, False) for c in CUTOFFS] + [(0.51, 0, True), (1.0, 0, True), (0.75, 3, True), (0.51, 1, False), (0.51, 3, False)]


def B(x):
    return x.encode("latin-1") if isinstance(x, str) else bytes(x)


def ref_binary():
    return os.path.join(os.path.dirname(HERE), "oracle", "_ref", "vsearch_ref")


# ---- the reference's loops ----------------------------------------------------------------------------------------------------------
def py_tax_field(h):
    """(tax_start, tax_end) of tax_parse, or None"""
    hlen, offset = len(h), 0
    while offset < hlen - 4:
        p = h.find(b"tax=", offset)
        if p < 0:
            break
        offset = p
        if offset > 0 and h[offset - 1:offset] != b";":
            offset += 5
            continue
        e = h.find(b";", offset + 4)
        return offset, (e if e >= 0 else hlen)
    return None


def py_tax_split(h):
    """(start[9], len[9]) of tax_split on the header bytes h"""
    start, ln = [0] * LEVELS, [0] * LEVELS
    field = py_tax_field(h)
    if field is None:
        return start, ln
    offset, tax_end = field[0] + 4, field[1]
    while offset < tax_end:
        r = RANKS.find(h[offset:offset + 1].lower())
        if r >= 0 and h[offset + 1:offset + 2] == b":":
            start[r] = offset + 2
            comma = h.find(b",", offset + 2)
            ln[r] = (comma - offset - 2) if comma >= 0 else (tax_end - offset - 2)
        comma = h.find(b",", offset)
        offset = comma + 1 if comma >= 0 else tax_end
    return start, ln


class Split:
    """the labels with their splits and names, made once per set"""

    def __init__(self, labels):
        self.labels = [B(l) for l in labels]
        self.split = [py_tax_split(l) for l in self.labels]
        self.names = [tuple(l[s:s + n] for s, n in zip(*sp)) for l, sp in zip(self.labels, self.split)]


def py_lca_query(S, hits, cutoff, maxhits=0, top_hits_only=False):
    """One query.  hits: [(target, id), ...] in the search's order.  -> dict: n_top, depth, level_match and cand (Boyer-Moore's own,
    at every level), text (what follows the tab, without the newline), and the normalised arrays matches / target / start / len."""
    names = S.names
    toreport = min(maxhits, len(hits)) if maxhits else len(hits)
    out = {"n_top": 0, "depth": 0, "level_match": [0] * LEVELS, "cand": [-1] * LEVELS, "text": b"",
           "matches": [0] * LEVELS, "target": [NONE] * LEVELS, "start": [0] * LEVELS, "len": [0] * LEVELS}
    if toreport == 0:
        return out
    votes, cand = [0] * LEVELS, [-1] * LEVELS
    top_hit_id = hits[0][1]
    tophitcount = 0
    for t in range(toreport):
        seqno, ident = hits[t]
        if top_hits_only and ident < top_hit_id:
            break
        tophitcount += 1
        new = names[seqno]
        for k in range(LEVELS):
            if votes[k] == 0:
                cand[k] = seqno
                votes[k] = 1
            elif names[cand[k]][:k + 1] == new[:k + 1]:          # every level 0 .. k: equal length and equal bytes
                votes[k] += 1
            else:
                votes[k] -= 1
    level_match = [0] * LEVELS
    for t in range(tophitcount):
        new = names[hits[t][0]]
        for k in range(LEVELS):
            if names[cand[k]][:k + 1] == new[:k + 1]:
                level_match[k] += 1
    out["n_top"], out["level_match"], out["cand"] = tophitcount, level_match, cand
    parts = []
    depth = 0
    for j in range(LEVELS):
        if 1.0 * level_match[j] / tophitcount < cutoff:
            break
        depth += 1
        st, ln = S.split[cand[j]][0][j], S.split[cand[j]][1][j]
        if ln > 0:
            parts.append(RANKS[j:j + 1] + b":" + S.labels[cand[j]][st:st + ln])
    out["depth"], out["text"] = depth, b",".join(parts)
    for j in range(depth):
        rep = next(hits[t][0] for t in range(tophitcount) if names[hits[t][0]][:j + 1] == names[cand[j]][:j + 1])
        out["matches"][j], out["target"][j] = level_match[j], rep
        out["start"][j], out["len"][j] = S.split[rep][0][j], S.split[rep][1][j]
    return out


def py_lca(tlabels, qlabels, hitlists, cutoff=1.0, maxhits=0, top_hits_only=False, S=None):
    """-> (the --lcaout lines as bytes, the per-query dicts of py_lca_query)"""
    S = S or Split(tlabels)
    info = [py_lca_query(S, h, cutoff, maxhits, top_hits_only) for h in hitlists]
    return [B(q) + b"\t" + i["text"] + b"\n" for q, i in zip(qlabels, info)], info


def py_arrays(info):
    """what LcaResult.arrays() must equal"""
    u = lambda rows: np.array(rows, np.uint32).tobytes()  # noqa: E731
    return (u([i["n_top"] for i in info]), u([i["depth"] for i in info]), u([i["matches"] for i in info]), u([i["target"] for i in info]),
            u([i["start"] for i in info]), u([i["len"] for i in info]))


def hit_dtype():
    from vsearch_amd import _lib
    return np.dtype(_lib.Hit)


def make_hits(hitlists, junk=0):
    """(first, hits) as the raw search calls return them; the fields vsx_lca does not read are filled with `junk`"""
    first = np.zeros(len(hitlists) + 1, np.uint64)
    first[1:] = np.cumsum([len(h) for h in hitlists])
    hits = np.zeros(int(first[-1]), hit_dtype())
    if junk:
        hits.view(np.uint8)[:] = junk
    flat = [x for h in hitlists for x in h]
    hits["target"] = [t for t, _ in flat]
    hits["id"] = [i for _, i in flat]
    hits["query"] = [q for q, h in enumerate(hitlists) for _ in h]
    return first, hits


# ---- the named sets -----------------------------------------------------------------------------------------------------------------
def tax(name, **ranks):
    """name;tax=r:v,...; in the order given"""
    return name + ";tax=" + ",".join("%s:%s" % (r, v) for r, v in ranks.items()) + ";"


def flat(targets, ident=99.0):
    return [(t, ident) for t in targets]


def counts_set():
    t = [tax("a", d="A", p="P1"), tax("b", d="A", p="P2"), tax("c", d="X")]
    q = [flat([1 if i % 3 == 2 else 0 for i in range(n)]) for n in (0, 1, 2, 3, 63, 64, 65, 129)]
    q.append(flat([2] * 70 + [0] * 59))                               # the majority lies in the second step's minority
    return "counts", t, q


def on_cutoff_set():
    t = [tax("a", d="A", p="P1"), tax("b", d="A", p="P2"), tax("c", d="X")]
    return "on_cutoff", t, [flat([0, 0, 0, 2]), flat([0, 0, 2]), flat([2, 0, 0]), flat([0, 1, 0, 1]), flat([0, 2]), flat([0, 0, 2, 2])]


def lost_at_g_set():
    base = dict(d="D", k="K", p="P", c="C", o="O", f="F")
    t = [tax("l%d" % i, g="G%d" % i, s="S%d" % i, **base) for i in range(3)] + [tax("m", d="D", k="K2")]
    return "lost_at_g", t, [flat([0, 1, 2]), flat([0, 1, 2, 3]), flat([3, 0, 1, 2, 0])]


def boyer_moore_set():
    """p: P1 P1 P2 P3 P3 -- Boyer-Moore ends on P3 (2 of 5), no value holds a majority; d holds one"""
    t = [tax("a", d="A", p="P1"), tax("b", d="A", p="P2"), tax("c", d="A", p="P3"), tax("x", d="X", p="P1")]
    return "boyer_moore", t, [flat([0, 0, 1, 2, 2]), flat([0, 0, 1, 2, 2, 1, 1]), flat([0, 3, 1, 2, 2, 2, 0])]


def same_genus_set():
    base = dict(d="D", k="K", p="P", c="C", o="O")
    t = [tax("a", f="F1", g="Gx", **base), tax("b", f="F2", g="Gx", **base), tax("c", f="F1", g="Gx", s="S", **base)]
    return "same_genus", t, [flat([0, 1]), flat([0, 1, 2]), flat([1, 0, 1, 0])]


def missing_ranks_set():
    t = [tax("a", d="A", p="P", g="G"), tax("b", d="A", p="P", g="G", s="S"), tax("c", d="A", g="G"), tax("e", k="K", g="G")]
    return "missing_ranks", t, [flat([0, 1]), flat([0, 1, 0]), flat([0, 2, 2]), flat([2, 0, 0]), flat([3, 3]), flat([0, 3])]


def keyword_set():
    t = ["plain", "s1xtax=d:A;", "xtax=d:A;tax=d:B,p:Q;", "ab;tax=", "ab;tax=d", "ab;tax=d:", "ab;tax=d:X", "tax=", "tax=d:Y", "tax=;tax=d:Z",
         "xtax=;tax=", "xtax=xtax=;tax=d:W", "atax=d:A;;tax=k:K", ";tax=d:A", "abcd", "", ";", "a;tax=d:A;tax=d:B"]
    q = [flat([i]) for i in range(len(t))] + [flat([0, 1]), flat([6, 8]), flat([2, 17, 17])]
    return "keyword", t, q


def field_set():
    t = ["s;tax=d:A,p:B;size=3,x", "s;tax=d:A,p:B;size=3,y", "s;tax=d:A,p:B;size=4,x", "u;tax=D:A,P:B,G:g", "u;tax=d:A,p:B,g:g", "r;tax=d:A,d:B,p:C",
         "r;tax=d:B,p:C", "e;tax=d:,p:P", "e;tax=,d:A,,p:P,", "e;tax=d:A,p", "e;tax=d:A,pp:P,x:Y,t:T", "e;tax=d:A;p:P,k:K", "w;tax=d:A B,p:\xe9\xff"]
    q = [flat([0, 1]), flat([0, 2]), flat([0, 1, 2]), flat([3, 4]), flat([5, 6]), flat([5, 6, 3])] + [flat([i]) for i in range(len(t))]
    return "field", t, q


def lengths_set():
    """names ending at bytes 63 / 64 / 65 of the label, at both sides of a step; a 300-byte name; a label of 64 and of 128 bytes"""
    t = []
    for end in (63, 64, 65, 127, 128, 129):
        head = b"n%03d;tax=d:" % end
        t.append(head + b"N" * (end - len(head)) + b",p:P;")
    t.append(b"long;tax=d:D,g:" + bytes(65 + (i * 7) % 26 for i in range(300)) + b",s:S")
    t.append(b"long;tax=d:D,g:" + bytes(65 + (i * 7) % 26 for i in range(299)) + b"!,s:S")
    for total in (64, 128):
        head = b"z;tax=d:"
        t.append(head + b"Q" * (total - len(head)))
    t.append(b"k" * 60 + b";tax=d:A,p:B")                             # the keyword across a step's end
    t.append(b"k" * 61 + b";tax=d:A,p:B")
    t.append(b"k" * 62 + b";tax=d:A,p:B")
    t.append(b"k" * 63 + b";tax=d:A,p:B")
    t.append(b"k" * 57 + b";tax=d:A,p:B;" + b"j" * 80 + b",c:C")      # a name that ends in a later step, beyond the field
    q = [flat([i]) for i in range(len(t))] + [flat([6, 7]), flat([6, 6, 7]), flat([10, 11, 12, 13]), flat([0, 1])]
    return "lengths", t, q


def ties_set():
    t = [tax("a", d="A", p="P1"), tax("b", d="A", p="P2"), tax("c", d="X", p="P1")]
    q = [[(0, 99.0), (1, 98.0), (2, 97.0)], [(0, 99.0), (1, 99.0), (2, 98.5)], [(0, 99.0), (1, 99.0), (2, 99.0)],
         [(0, 99.0), (2, 99.5), (1, 98.0), (0, 99.0)],                   # unsorted: the loop breaks at the first lower id
         [(0, 99.0), (0, 99.0), (1, 99.0), (2, 99.0), (2, 99.0)], [(2, 100.0)] + [(0, 100.0)] * 66 + [(1, 99.9)] * 3]
    return "ties", t, q


def no_tax_set():
    t = ["t1", "t2;size=3", "t3"]
    return "no_tax", t, [flat([0, 1, 2]), flat([1]), []]


def all_sets():
    out = []
    for name, t, q in (counts_set(), on_cutoff_set(), lost_at_g_set(), boyer_moore_set(), same_genus_set(), missing_ranks_set(), keyword_set(),
                       field_set(), lengths_set(), ties_set(), no_tax_set()):
        out.append({"name": name, "tlabels": [B(l) for l in t], "qlabels": [B("q%d" % i) for i in range(len(q))], "hits": q})
    return out


NAMES = ("Bacteria", "Archaea", "Proteo", "Firmi", "Gamma", "Bacilli", "Entero", "Lacto", "Esch", "coli", "K12", "x", "")


def random_set(seed):
    """labels over 2 - 5 names per level (a level may be missing), a handful of queries of 1 - 200 hits, one option combination"""
    rng = random.Random(seed)
    pool = [[rng.choice(NAMES[:-1]) + str(rng.randrange(3)) for _ in range(rng.randint(2, 5))] for _ in range(LEVELS)]
    labels = []
    for i in range(rng.randint(2, 12)):
        fields = []
        for k in range(LEVELS):
            if rng.random() < 0.75:
                fields.append("%s:%s" % (chr(RANKS[k]).upper() if rng.random() < 0.1 else chr(RANKS[k]), pool[k][min(len(pool[k]) - 1, int(rng.expovariate(1.2)))]))
        if rng.random() < 0.1:
            rng.shuffle(fields)
        labels.append("t%d;tax=%s%s" % (i, ",".join(fields), rng.choice(["", ";", ";size=2", ";x=1,y"])) if rng.random() < 0.95 else "t%d" % i)
    hits = []
    for _ in range(rng.randint(1, 4)):
        n = rng.randint(1, 200) if rng.random() < 0.15 else rng.randint(1, 12)
        fav = rng.randrange(len(labels))
        hits.append([(fav if rng.random() < 0.6 else rng.randrange(len(labels)), rng.choice((100.0, 100.0, 99.5, 97.0))) for _ in range(n)])
    return {"name": "random%d" % seed, "tlabels": [B(l) for l in labels], "qlabels": [B("q%d" % i) for i in range(len(hits))], "hits": hits,
            "combo": (rng.choice(CUTOFFS), rng.choice((0, 0, 1, 3, 50)), rng.random() < 0.3)}


FRAGMENTS = [b"tax=", b";tax=", b";", b";", b",", b",", b":", b"d:", b"K:", b"p:", b"g:", b"s:", b"t:", b"x:", b"dd", b"A", b"Bc", b"xtax=", b"tax", b"ax=",
             b" ", b"\xe9", b"size=3", b"=", b"c:C1", b"o:", b"F:f"]


def random_label(rng, most=400):
    want = rng.choice((0, 3, 8, 20, 60, 64, 70, 128, 200, most))
    parts, n = [], 0
    while n < want:
        f = rng.choice(FRAGMENTS) if rng.random() < 0.7 else bytes(rng.choice(b"abcdkpxyz01") for _ in range(rng.randint(1, 30)))
        parts.append(f)
        n += len(f)
    return b"".join(parts)[:most]


def random_labels(n=20000, seed=401):
    rng = random.Random(seed)
    return [random_label(rng) for _ in range(n)]


# ---- calls --------------------------------------------------------------------------------------------------------------------------
def lca_module():
    return importlib.import_module("vsearch_amd.lca")


def run_set(s, combo, index=None, host=False, window=0, junk=0):
    """the set under one (cutoff, maxhits, top_hits_only): an LcaResult from the index, or from the host restatement"""
    lc = lca_module()
    raw = make_hits(s["hits"], junk)
    if host:
        return lc.lca_host(s["tlabels"], raw, lca_cutoff=combo[0], maxhits=combo[1], top_hits_only=combo[2])
    return lc.lca(index, raw, lca_cutoff=combo[0], maxhits=combo[1], top_hits_only=combo[2], window=window)


def device_digest(aligner):
    lc = lca_module()
    h = hashlib.sha256()
    for s in all_sets():
        with lc.LcaIndex(s["tlabels"], ctx=aligner) as index:
            for a in index.split():
                h.update(a.tobytes())
            for combo in COMBOS:
                res = run_set(s, combo, index=index)
                assert res.stats["queries_device"] == len(s["hits"]), (s["name"], res.stats)
                for a in res.arrays():
                    h.update(a)
    return h.hexdigest()


# ---- the recorded CLI runs -----------------------------------------------------------------------------------------------------------
def seq_of(i, n=100):
    rng = random.Random(7919 * i + 13)
    return "".join(rng.choice("ACGT") for _ in range(n))


def near(seq, k, shift=0):
    """`seq` with k substitutions, spread"""
    s = list(seq)
    for j in range(k):
        p = ((j + 1) * len(s) // (k + 1) + shift) % len(s)
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1) % 4]
    return "".join(s)


def golden_input():
    """three families of database sequences (substitutions only, so that id = 100 * ids / alnlen exactly), queries at a few distances"""
    fam = [seq_of(1), seq_of(2), seq_of(3)]
    db = [("e1;tax=d:Bacteria,p:Proteo,c:Gamma,o:Entero,f:Enterobact,g:Esch,s:Esch_coli;", fam[0]),
          ("e2;tax=d:Bacteria,p:Proteo,c:Gamma,o:Entero,f:Enterobact,g:Esch,s:Esch_fergusonii;", near(fam[0], 1)),
          ("e3;tax=d:Bacteria,p:Proteo,c:Gamma,o:Entero,f:Enterobact,g:Salmonella;", near(fam[0], 2, 3)),
          ("e4;tax=d:Bacteria,p:Proteo,c:Gamma,o:Entero,f:Yersiniaceae,g:Yersinia,s:Y_pestis;", near(fam[0], 3, 5)),
          ("e5;tax=d:Bacteria,p:Proteo,c:Gamma,o:Entero,f:Enterobact,g:Esch,s:Esch_coli;", fam[0]),
          ("b1;tax=d:Bacteria,p:Firmi,c:Bacilli,o:Lacto,f:Lactobacillaceae,g:Lacto;", fam[1]),
          ("b2;tax=d:Bacteria,p:Firmi,c:Bacilli,o:Lacto,f:Lactobacillaceae,g:Lacto,s:L_casei;size=3,x", near(fam[1], 1)),
          ("b3;tax=D:Bacteria,P:Firmi,C:Bacilli", near(fam[1], 2, 7)),
          ("b4", near(fam[1], 3, 11)),
          ("a1;tax=d:Archaea,p:Eury;", fam[2]),
          ("a2;tax=d:Archaea,d:Bacteria,p:Eury;", near(fam[2], 1)),
          ("a3xtax=d:Archaea;", near(fam[2], 2, 9))]
    queries = [("q_e", fam[0]), ("q_e1", near(fam[0], 1, 17)), ("q_e4", near(fam[0], 4, 13)), ("q_b", fam[1]), ("q_b1", near(fam[1], 1, 19)),
               ("q_b5", near(fam[1], 5, 23)), ("q_a", fam[2]), ("q_a2", near(fam[2], 2, 29)), ("q_none", seq_of(9)), ("q_e_again;size=2", near(fam[0], 1))]
    return db, queries


def golden_runs():
    search = ["--id", "0.9", "--maxaccepts", "8", "--maxrejects", "32"]
    runs = []
    for command, base in (("usearch_global", search), ("search_exact", [])):
        for c in ("1.0", "0.51", "0.75", "0.6666666666666666", "0.67"):
            runs.append({"command": command, "search": base, "cutoff": c, "maxhits": 0, "top_hits_only": False})
        for extra in ({"top_hits_only": True}, {"maxhits": 1}, {"maxhits": 3}, {"maxhits": 3, "top_hits_only": True}):
            for c in ("0.51", "1.0"):
                runs.append(dict({"command": command, "search": base, "cutoff": c, "maxhits": 0, "top_hits_only": False}, **extra))
    return runs


def write_fasta(path, records):
    with open(path, "wb") as f:
        for l, s in records:
            f.write(b">" + B(l) + b"\n" + B(s) + b"\n")


def cli(tmp, args):
    return subprocess.run([ref_binary()] + args + ["--threads", "1", "--quiet"], cwd=tmp, capture_output=True, text=True)


def cli_lcaout(tmp, command, search, cutoff, maxhits=0, top_hits_only=False, userout=False):
    """-> (the --lcaout text, or None where the command writes no such file; the --userout rows or None)"""
    for f in ("l.txt", "u.txt"):
        if os.path.exists(os.path.join(tmp, f)):
            os.remove(os.path.join(tmp, f))
    args = ["--" + command, "q.fa", "--db", "db.fa", "--qmask", "none", "--dbmask", "none", "--lcaout", "l.txt", "--lca_cutoff", str(cutoff)] + list(search)
    if maxhits:
        args += ["--maxhits", str(maxhits)]
    if top_hits_only:
        args += ["--top_hits_only"]
    if userout:
        args += ["--userout", "u.txt", "--userfields", "query+target+ids+alnlen"]
    r = cli(tmp, args)
    if r.returncode != 0:
        raise RuntimeError(" ".join(args) + "\n" + r.stderr[-2000:])
    path = os.path.join(tmp, "l.txt")
    text = open(path, "rb").read().decode("latin-1") if os.path.exists(path) else None
    rows = [l.split("\t") for l in open(os.path.join(tmp, "u.txt"), "rb").read().decode("latin-1").splitlines()] if userout else None
    return text, rows


def record_golden(path=GOLDEN):
    db, queries = golden_input()
    out = {"db": db, "queries": queries, "hits": {}, "runs": [], "fatal": {}}
    with tempfile.TemporaryDirectory(prefix="lca_golden_") as tmp:
        write_fasta(os.path.join(tmp, "db.fa"), db)
        write_fasta(os.path.join(tmp, "q.fa"), queries)
        for command, search in (("usearch_global", golden_runs()[0]["search"]), ("search_exact", [])):
            _, rows = cli_lcaout(tmp, command, search, "1.0", userout=True)
            out["hits"][command] = rows
        for r in golden_runs():
            text, _ = cli_lcaout(tmp, r["command"], r["search"], r["cutoff"], r["maxhits"], r["top_hits_only"])
            out["runs"].append(dict(r, lcaout=text))
        for c in ("0.5", "1.01"):
            p = cli(tmp, ["--usearch_global", "q.fa", "--db", "db.fa", "--id", "0.9", "--lcaout", "l.txt", "--lca_cutoff", c])
            assert p.returncode != 0
            out["fatal"][c] = [l for l in p.stderr.splitlines() if l.strip()][-1].strip()
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return out


def load_golden(path=GOLDEN):
    with open(path) as f:
        return json.load(f)


def golden_hitlists(g, command):
    """the recorded --userout rows as hit lists in the queries' order: (target number, 100.0 * ids / alnlen)"""
    qno = {l: i for i, (l, _) in enumerate(g["queries"])}
    tno = {l: i for i, (l, _) in enumerate(g["db"])}
    lists = [[] for _ in g["queries"]]
    for q, t, ids, alnlen in g["hits"][command]:
        if t != "*":
            lists[qno[q]].append((tno[t], 100.0 * int(ids) / int(alnlen)))
    return lists


# ---- the live searches (tests/test_gpu_lca.py, bench_lca.py) ---------------------------------------------------------------------------
def rnd_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def mutate(rng, s, rate):
    """substitutions only"""
    return "".join("ACGT"[("ACGT".index(c) + rng.randint(1, 3)) % 4] if rng.random() < rate else c for c in s)


GENERA = 40


def live_db(rng, n=2000):
    """n labelled sequences: GENERA ancestors, every sequence a few substitutions from its genus' ancestor, SILVA-style labels"""
    anc = [rnd_seq(rng, 150) for _ in range(GENERA)]
    db, labels = [], []
    for i in range(n):
        g = i % GENERA
        db.append(anc[g] if i < GENERA else mutate(rng, anc[g], rng.choice((0.0, 0.01, 0.02, 0.04))))
        ranks = ["d:Bacteria", "p:P%d" % (g % 4), "c:C%d" % (g % 8), "o:O%d" % (g % 16), "f:F%d" % (g % 20), "g:G%d" % g]
        if i % 3:
            ranks.append("s:G%d_sp%d" % (g, (i // GENERA) % 5))
        if i % 11 == 0:
            ranks = ranks[:3]
        labels.append("r%d;tax=%s%s" % (i, ",".join(ranks), ";" if i % 2 else "") if i % 37 else "r%d" % i)
    return db, labels


def live_queries(rng, db, n=2000):
    qs = [rnd_seq(rng, 150) if rng.random() < 0.03 else mutate(rng, db[rng.randrange(len(db))], rng.choice((0.0, 0.01, 0.03))) for _ in range(n)]
    return qs, ["q%d;size=%d" % (k, 1 + k % 3) for k in range(n)]


if __name__ == "__main__":
    if "--record" in sys.argv:
        g = record_golden()
        print("recorded", len(g["runs"]), "runs,", os.path.getsize(GOLDEN), "bytes")
    elif "--digest" in sys.argv:
        sys.path.insert(0, os.path.dirname(HERE))
        from vsearch_amd import Aligner, _lib
        with Aligner(device=0) as al:
            print("digest %s poison %d" % (device_digest(al), _lib.load().vsx_internal_poison_byte()))
