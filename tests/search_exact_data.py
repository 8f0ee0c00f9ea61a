"""Inputs, a plain-Python restatement and the reference-CLI runner for the exact-search tests (--search_exact).

    py_search_exact()   dictionary over normalised strings, the unaligned / aligned filters, the order of the hits
    *_set()             input builders: the issue's worked example, the alphabet, lengths around every chunk size of the kernels,
                        table sizes, filters, masking
    run_reference()     the reference CLI (oracle/_ref/vsearch_ref) on one set: --userout, --uc, --dbmatched --sizeout, --log
    __main__            writes tests/golden/search_exact_golden.json: the sets' inputs and the reference's recorded lines, nothing else

The kernels' sizes (vsearch_amd/csrc/vsx_exact_internal.h): a lane hashes 16 symbols at a time (CHUNK) and a wave 1 024 per pass
(HASH_PASS); a lane compares 32 symbols at a time (PAIR) and a wave 2 048 per pass (CMP_PASS); the probe reads 64 slots per round.
"""
import json
import os
import random
import re
import subprocess
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "search_exact_golden.json")

CHUNK, PAIR, HASH_PASS, CMP_PASS, SLOT_ROUND = 16, 32, 1024, 2048, 64
USERFIELDS = ("query", "target", "id", "alnlen", "mism", "opens", "raw", "caln", "qstrand", "ql", "tl")
IUPAC = "ACGTURYSWKMDBHVN"
CONTAINS = {"R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "D": "AGT", "B": "CGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
MASK_MODES = {"none": 0, "soft": 1, "dust": 2}

# chrmap_4bit and chrmap_complement of the reference (utils/maps.cpp), as tables over the letters
CODE = dict(zip("ABCDGHKMNRSTUVWY", (1, 14, 2, 13, 4, 11, 12, 3, 15, 5, 6, 8, 8, 7, 9, 10)))
COMPLEMENT = dict(zip("ABCDGHKMNRSTUVWY", "TVGHCDMKNYSAABWR"))


def norm(s):
    """the 4-bit codes of a sequence: what two sequences must share to match"""
    return bytes(CODE.get(c.upper(), 0) for c in s)


def revcomp(s):
    return "".join(COMPLEMENT.get(c.upper(), "N") for c in reversed(s))


# ---- options: one dict describes a set's command line, the session's options and the Python restatement's ----------------------
DEFAULT_OPTS = dict(strand_both=1, qmask="none", dbmask="none", hardmask=0, sizein=0)
FILTER_KEYS = ("mintsize", "maxqsize", "minsizeratio", "maxsizeratio", "minqt", "maxqt", "minsl", "maxsl", "mincols")
FLAG_KEYS = ("self", "selfid")


def full_opts(opts):
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    return o


def session_opts(opts):
    """keyword options of SearchSession / search_exact_host for a set"""
    o = full_opts(opts)
    kw = dict(id=1.0, strand_both=o["strand_both"], soft_mask=MASK_MODES[o["dbmask"]], hardmask=3 if o["hardmask"] else 0)
    if o["qmask"] != o["dbmask"]:
        kw["qmask"] = 1 + MASK_MODES[o["qmask"]]
    for k in FILTER_KEYS:
        if k in o:
            kw[k] = o[k]
    if o.get("self"):
        kw["self_"] = 1
    if o.get("selfid"):
        kw["selfid"] = 1
    return kw


def cli_args(opts):
    o = full_opts(opts)
    a = ["--strand", "both" if o["strand_both"] else "plus", "--qmask", o["qmask"], "--dbmask", o["dbmask"]]
    if o["hardmask"]:
        a.append("--hardmask")
    if o["sizein"]:
        a.append("--sizein")
    for k in FILTER_KEYS:
        if k in o:
            a += ["--" + k, repr(o[k])]
    for k in FLAG_KEYS:
        if o.get(k):
            a.append("--" + k)
    return a


# ---- the plain-Python restatement ---------------------------------------------------------------------------------------------
def _hardmasked(seqs, mode):
    """--hardmask: the masked symbols as 'N' (mode soft: the lower-case symbols; dust: the DUST intervals, found by the library's
    host DUST, vsx_dust_mask -- the restatement restates the search, not DUST)"""
    if mode == "none":
        return list(seqs)
    if mode == "soft":
        return ["".join("N" if c.islower() else c for c in s) for s in seqs]
    from vsearch_amd import dust_mask
    return ["".join("N" if c.islower() else c for c in m.decode("latin-1")) for m in dust_mask(list(seqs))]


def py_search_exact(db, queries, opts=None, db_sizes=None, sizes=None, db_labels=None, labels=None):
    """-> per query the accepted hits as (target, strand) pairs, ordered by target (plus before minus)"""
    o = full_opts(opts)
    dbt = _hardmasked(db, o["dbmask"]) if o["hardmask"] else list(db)
    index = {}
    for t, s in enumerate(dbt):
        if s:
            index.setdefault(norm(s), []).append(t)
    out = []
    for q, seq in enumerate(queries):
        hits = []
        strands = [seq] + ([revcomp(seq)] if o["strand_both"] else [])
        if o["hardmask"]:
            strands = _hardmasked(strands, o["qmask"])
        for strand, text in enumerate(strands):
            for t in (index.get(norm(text), []) if text else []):
                hits.append((t, strand))
        qsize = 1 if sizes is None else int(sizes[q])
        kept = []
        for t, strand in sorted(hits):
            tsize = 1 if db_sizes is None else int(db_sizes[t])
            ql = dl = len(seq)
            ok = qsize <= o.get("maxqsize", float("inf")) and tsize >= o.get("mintsize", 0)
            ok = ok and qsize >= o.get("minsizeratio", 0.0) * tsize and qsize <= o.get("maxsizeratio", float("inf")) * tsize
            ok = ok and ql >= o.get("minqt", 0.0) * dl and ql <= o.get("maxqt", float("inf")) * dl
            ok = ok and dl >= o.get("minsl", 0.0) * ql and dl <= o.get("maxsl", float("inf")) * ql
            if o.get("self") and labels is not None and db_labels is not None and labels[q] == db_labels[t]:
                ok = False
            if o.get("selfid"):
                ok = False                                       # an exact match IS the same sequence
            if ql < o.get("mincols", 0):
                ok = False
            if ok:
                kept.append((t, strand))
        out.append(kept)
    return out


def expected_record(qlen, target, strand, match_score=2):
    """the fixed hit record of an exact match (include/vsx_search.h)"""
    d = dict(target=target, strand=strand, count=0, accepted=1, weak=0, used_fallback=0, nwscore=qlen * match_score, nwdiff=0, nwgaps=0,
             nwindels=0, nwalignmentlength=qlen, matches=qlen, mismatches=0, internal_alignmentlength=qlen, internal_gaps=0,
             internal_indels=0, trim_q_left=0, trim_q_right=0, trim_t_left=0, trim_t_right=0, shortest=qlen, longest=qlen,
             nwid=100.0, id=100.0, id0=100.0, id1=100.0, id2=100.0, id3=100.0, id4=100.0, cigar=f"{qlen}M")
    return d


def assert_hits_equal_py(hits, s):
    """`hits` (per-query lists of dicts) = the Python restatement's pairs with the fixed record, field for field"""
    want = py_search_exact(s["db"], s["queries"], s["opts"], s.get("db_sizes"), s.get("sizes"), s.get("db_names"), s.get("names"))
    assert len(hits) == len(want)
    for q, (hs, ws) in enumerate(zip(hits, want)):
        assert [(h["target"], h["strand"]) for h in hs] == ws, (s["name"], q)
        for h in hs:
            exp = expected_record(len(s["queries"][q]), h["target"], h["strand"])
            exp["query"] = q
            assert h == exp, (s["name"], q, h)


# ---- formatting through the package's own formatters ------------------------------------------------------------------------------
def userout_lines(s, hits):
    from vsearch_amd import SearchSession
    stub = types.SimpleNamespace(db=s["db"])
    return SearchSession.userout(stub, s["queries"], qnames=s["names"], tnames=s["db_names"], fields=USERFIELDS, hits=hits)


def uc_lines(s, hits, uc_allhits=False):
    from vsearch_amd import SearchSession
    return SearchSession.exact_uc_lines(s["queries"], s["names"], s["db_names"], hits, uc_allhits=uc_allhits)


# ---- input builders --------------------------------------------------------------------------------------------------------------
def _set(name, db, queries, opts=None, db_sizes=None, sizes=None, db_names=None, names=None):
    o = full_opts(opts)
    if o["sizein"]:
        db_sizes = db_sizes or [1] * len(db)
        sizes = sizes or [1] * len(queries)
    tag = (lambda base, k, sz: f"{base}{k};size={sz[k]}") if o["sizein"] else (lambda base, k, sz: f"{base}{k}")
    return dict(name=name, db=list(db), queries=list(queries), opts=opts or {}, db_sizes=db_sizes, sizes=sizes,
                db_names=db_names or [tag("t", k, db_sizes) for k in range(len(db))],
                names=names or [tag("q", k, sizes) for k in range(len(queries))])


def issue_example():
    db = ["ACGTACGGTTCA", "acguacggttca", "TGAACCGTACGT", "ACGCGT", "ACGTRCGGTTCA", "ACGTNCGGTTCA", "ACGTACGGTTCAA", "ACGTACGGTTCA"]
    qs = ["ACGTACGGTTCA", "ACGCGT", "ACGTRCGGTTCA", "ACGTYCGGTTCA", "TGAACCGYACGT", "ACGTACGGTTC", "acgtncggttca"]
    return _set("issue_example", db, qs)


def alphabet_set():
    """lower case, U, every IUPAC code against itself and against a base it contains, N against N and against A"""
    frame = "GATTACA{}CATTAGGC"
    db, qs = [], []
    for c in IUPAC:
        db.append(frame.format(c))
        qs.append(frame.format(c))
        qs.append(frame.format(c.lower()))
    for c, bases in CONTAINS.items():
        for b in bases:
            qs.append(frame.format(b))              # matches only the database entry of the plain base
    qs.append(frame.format("T").replace("T", "U"))
    qs.append(frame.format("u").lower())
    return _set("alphabet", db, qs)


def random_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def edge_positions(L):
    """the positions at which a difference must be seen: the ends, both sides of every chunk edge the kernels have at this length
    -- counted from the start (plus strand) and from the end (the reverse strand's chunks begin there)"""
    pos = {0, L - 1}
    edges = set()
    for unit in (CHUNK, PAIR):
        edges.update(range(unit, min(L, 8 * unit) + 1, unit))          # the first edges ...
        edges.add(unit * ((L - 1) // unit))                            # ... and the last one
    for unit in (HASH_PASS, CMP_PASS):
        edges.update(range(unit, L + 1, unit))
    for e in edges:
        for p in (e - 1, e, L - e - 1, L - e):
            if 0 <= p < L:
                pos.add(p)
    return sorted(pos)


def substitute(s, p):
    return s[:p] + {"A": "C", "C": "G", "G": "T", "T": "A"}[s[p]] + s[p + 1:]


def length_case(rng, L):
    """a query of length L and a database of: itself, its reverse complement, copies differing at every edge position, copies one
    symbol shorter and longer.  Expected: itself on the plus strand, its reverse complement on the minus strand."""
    q = random_seq(rng, L)
    while revcomp(q) == q:
        q = random_seq(rng, L)
    db = [q, revcomp(q)] + [substitute(q, p) for p in edge_positions(L)] + [q[:-1], q + "A"]
    return q, db


LENGTHS_GOLDEN = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65)
# every length the issue names, and one below, at and above each size of the kernels
LENGTHS_DEVICE = (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, PAIR - 1, PAIR, PAIR + 1, 63, 64, 65, HASH_PASS - 1, HASH_PASS, HASH_PASS + 1,
                  CMP_PASS - 1, CMP_PASS, CMP_PASS + 1, 4095, 4096, 4097, 20000)


def lengths_set(lengths, seed=7, name="lengths"):
    rng = random.Random(seed)
    db, qs = [], []
    for L in lengths:
        q, d = length_case(rng, L)
        qs.append(q)
        db += d
    rng.shuffle(db)
    return _set(name, [d for d in db if d], qs)


def table_set(n, seed=11):
    """n distinct database sequences (the 2/3-fill edges of a power-of-two table), every one of them queried, plus misses"""
    rng = random.Random(seed * 100003 + n)
    seen, db = set(), []
    while len(db) < n:
        s = random_seq(rng, rng.randint(20, 40))
        if s not in seen and revcomp(s) not in seen:
            seen.add(s)
            db.append(s)
    pick = list(range(n)) if n <= 64 else rng.sample(range(n), 64)
    qs = [db[k] for k in pick] + [revcomp(db[k]) for k in pick[:16]] + [substitute(db[k], 3) for k in pick[:16]]
    return _set(f"table_{n}", db, qs)


def duplicates_set(copies=300):
    """`copies` identical sequences and `copies` identical reverse palindromes, probed on both strands"""
    rng = random.Random(13)
    s = random_seq(rng, 37)
    pal = "ACGTTGCATGCAACGT"
    assert revcomp(pal) == pal
    db = [s] * copies + [pal] * copies
    order = list(range(len(db)))
    rng.shuffle(order)
    return _set(f"duplicates_{copies}", [db[k] for k in order], [s, revcomp(s), pal, substitute(s, 5)])


def seeded_set(seed, n_db, n_q, sizein=1, name=None):
    """reads against a database with repeated entries: about 60 % exact copies, half of those reverse-complemented, the rest one
    substitution away"""
    rng = random.Random(seed)
    base = [random_seq(rng, rng.randint(30, 90)) for _ in range(max(1, n_db * 3 // 4))]
    db = [rng.choice(base) if k >= len(base) else base[k] for k in range(n_db)]
    qs = []
    for _ in range(n_q):
        s = rng.choice(db)
        r = rng.random()
        if r < 0.3:
            pass
        elif r < 0.6:
            s = revcomp(s)
        else:
            s = substitute(s, rng.randrange(len(s)))
        qs.append(s)
    return _set(name or f"seeded_{seed}", db, qs, dict(sizein=sizein), db_sizes=[rng.randint(1, 9) for _ in db],
                sizes=[rng.randint(1, 9) for _ in qs])


def filter_sets():
    """each unaligned / aligned filter on a set where it accepts some matches and rejects others"""
    rng = random.Random(17)
    a, b, c = (random_seq(rng, 40) for _ in range(3))
    db, db_sizes = [a, a, b, revcomp(c), a], [1, 4, 2, 8, 16]
    qs, sizes = [a, b, c, substitute(a, 7)], [4, 2, 1, 3]
    out = []
    for name, extra in (("mintsize", dict(mintsize=4)), ("maxqsize", dict(maxqsize=2)), ("minsizeratio", dict(minsizeratio=0.5)),
                        ("maxsizeratio", dict(maxsizeratio=1.0)), ("minqt", dict(minqt=1.01)), ("maxqt", dict(maxqt=0.99)),
                        ("minsl", dict(minsl=1.0)), ("maxsl", dict(maxsl=0.99)), ("mincols_above", dict(mincols=41)),
                        ("mincols_at", dict(mincols=40))):
        o = dict(sizein=1)
        o.update(extra)
        out.append(_set("filter_" + name, db, qs, o, db_sizes=db_sizes, sizes=sizes))
    # --self: a query whose header equals a target's is not matched to it, but to the other copies
    names = ["x;size=4", "y;size=2", "z;size=1", "w;size=3"]
    db_names = ["x;size=4", "other;size=4", "y;size=2", "z;size=8", "more;size=16"]
    out.append(_set("filter_self", db, qs, dict(sizein=1, self=1), db_sizes=[4, 4, 2, 8, 16], sizes=sizes, db_names=db_names, names=names))
    return out


def selfid_set():
    """--selfid rejects every exact match (the reference's command line does not offer it for --search_exact; the library's
    filter honours it): compared with the restatements only"""
    s = filter_sets()[0]
    return _set("filter_selfid", s["db"], s["queries"], dict(sizein=1, selfid=1), db_sizes=s["db_sizes"], sizes=s["sizes"])


def masking_sets():
    """a read with a 40-base homopolymer against its own copy, under the four combinations of query mask, database mask and
    --hardmask the issue checked"""
    rng = random.Random(19)
    read = random_seq(rng, 30) + "A" * 40 + random_seq(rng, 30)
    plain = random_seq(rng, 80)
    db, qs = [read, plain], [read, plain, revcomp(read)]
    combos = (("dust_none_hard", dict(qmask="dust", dbmask="none", hardmask=1)), ("dust_none", dict(qmask="dust", dbmask="none")),
              ("dust_dust_hard", dict(qmask="dust", dbmask="dust", hardmask=1)), ("none_none_hard", dict(qmask="none", dbmask="none", hardmask=1)))
    return [_set("masking_" + n, db, qs, o) for n, o in combos]


def empty_query_set():
    return _set("empty_query", ["ACGTACGT", "TTTTGGGG"], ["ACGTACGT", "", "CCCCAAAA"])


def golden_sets():
    return ([issue_example(), alphabet_set(), lengths_set(LENGTHS_GOLDEN, name="lengths_small"), table_set(5), duplicates_set(5),
             seeded_set(23, 120, 200), seeded_set(29, 60, 80, sizein=0, name="seeded_plain"), empty_query_set()]
            + filter_sets() + masking_sets())


# ---- the reference CLI -----------------------------------------------------------------------------------------------------------
def ref_binary():
    return os.path.join(ROOT, "oracle", "_ref", "vsearch_ref")


def _fasta(path, names, seqs):
    with open(path, "w") as f:
        for n, s in zip(names, seqs):
            f.write(f">{n}\n{s}\n")


def run_reference(s, threads=1, uc_allhits=False):
    """-> dict(userout, uc, dbmatched = {header without ;size: size}, log = the "Matching ..." lines) of the reference CLI"""
    with tempfile.TemporaryDirectory(prefix="vsx_exact_") as tmp:
        p = lambda n: os.path.join(tmp, n)
        _fasta(p("db.fa"), s["db_names"], s["db"])
        _fasta(p("q.fa"), s["names"], s["queries"])
        args = [ref_binary(), "--search_exact", p("q.fa"), "--db", p("db.fa"), "--threads", str(threads), "--userout", p("u.tsv"),
                "--userfields", "+".join(USERFIELDS), "--uc", p("o.uc"), "--dbmatched", p("m.fa"), "--sizeout", "--log", p("log.txt"),
                "--quiet", "--fasta_width", "0"] + cli_args(s["opts"])
        if uc_allhits:
            args.append("--uc_allhits")
        r = subprocess.run(args, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{s['name']}: reference CLI failed: {r.stderr[-2000:]}")
        read = lambda n: open(p(n)).read().splitlines()
        dbm = {}
        for line in read("m.fa"):
            if line.startswith(">"):
                m = re.match(r">(.*?)(?:;size=\d+)*;size=(\d+);?$", line)
                dbm[m.group(1)] = int(m.group(2))
        return dict(userout=read("u.tsv"), uc=read("o.uc"), dbmatched=dbm,
                    log=[l for l in read("log.txt") if l.startswith("Matching ")])


def summary_of(s, hits):
    """exact_summary in the shape run_reference reports: ({target header without ;size: count}, (matched, queries),
    (abundance matched, abundance))"""
    from vsearch_amd.search import exact_summary
    sm = exact_summary(hits, s["sizes"] if full_opts(s["opts"])["sizein"] else None)
    dbm = {re.sub(r";size=\d+$", "", s["db_names"][t]): c for t, c in sm["dbmatched"].items() if c}
    return dbm, (sm["queries_matched"], sm["queries"]), (sm["abundance_matched"], sm["abundance"])


def log_counts(lines):
    """the two counts of the log's closing lines -> ((matched, queries), (abundance matched, abundance) or None)"""
    uniq = total = None
    for l in lines:
        m = re.match(r"Matching unique query sequences: (\d+) of (\d+)", l)
        if m:
            uniq = (int(m.group(1)), int(m.group(2)))
        m = re.match(r"Matching total query sequences: (\d+) of (\d+)", l)
        if m:
            total = (int(m.group(1)), int(m.group(2)))
    return uniq, total


INPUT_KEYS = ("name", "db", "queries", "opts", "db_sizes", "sizes", "db_names", "names")


def write_golden(path=GOLDEN):
    sets = []
    for s in golden_sets():
        rec = {k: s[k] for k in INPUT_KEYS}
        rec["ref"] = run_reference(s)
        rec["ref"]["uc_allhits"] = run_reference(s, uc_allhits=True)["uc"]
        sets.append(rec)
    with open(path, "w") as f:
        json.dump(dict(userfields=list(USERFIELDS), sets=sets), f, indent=0, separators=(",", ":"))
        f.write("\n")
    return sets


def load_golden(path=GOLDEN):
    with open(path) as f:
        return json.load(f)["sets"]


if __name__ == "__main__":
    for rec in write_golden():
        print(f"{rec['name']}: {len(rec['queries'])} queries, {len(rec['db'])} database sequences, {len(rec['ref']['userout'])} hits")
