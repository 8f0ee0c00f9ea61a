"""Inputs, a plain-Python restatement and the reference-CLI runner for the orientation tests (--orient).

    py_orient()       match counts as a dictionary of sets, the two comparisons per distinct word, the verdict, the oriented text
    *_set()           input builders, each the smallest that reaches the edge it is named after
    run_reference()   the reference CLI (oracle/_ref/vsearch_ref) on one set: --tabbedout, --fastaout, --fastqout, --notmatched, --log
    __main__          writes tests/golden/orient_golden.json: the sets' inputs and the reference's recorded text, nothing else

How the sets steer the counts: a MARKER is a random word of the set's word length that is not its own reverse complement.  A
database sequence holds markers joined by runs of N (which also pad it past --minseqlength), so the only valid words of the
database are the markers themselves: hf copies of a marker in hf sequences and hr copies of its reverse complement in hr others
make (mc[marker], mc[rc(marker)]) = (hf, hr).  Queries are markers joined by N in the same way: no junction word exists.
"""
import json
import os
import random
import re
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "orient_golden.json")

MASK_MODES = {"none": 0, "soft": 1, "dust": 2}
AMBIGUOUS = "RYSWKMDBHVN"
# chrmap_complement of the reference (utils/maps.cpp): upper case, and the letters it keeps in lower case
COMPLEMENT = dict(zip("ABCDGHKMNRSTUVWY", "TVGHCDMKNYSAABWR"))
MAX_QLEN = 16384                       # VSX_ORIENT_MAX_QLEN
CLASS_QLEN = (512, 4096, 16384)        # the count kernel's length classes (vsx_orient_internal.h)
PAD = "N" * 32

DEFAULT_OPTS = dict(wordlength=12, qmask="dust", dbmask="dust", hardmask=0, sizein=0, sizeout=0, xsize=0, relabel=None, fasta_width=80)


def full_opts(opts):
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    return o


def complement(c):
    if c.upper() in COMPLEMENT and c.isalpha():
        u = COMPLEMENT[c.upper()]
        return u.lower() if c.islower() else u
    return "N"


def revcomp(s):
    return "".join(complement(c) for c in reversed(s))


def random_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


# ---- the plain-Python restatement ---------------------------------------------------------------------------------------------
def masked_db(db, dbmask, hardmask):
    """the database text as the reference indexes it: --dbmask dust runs DUST (the library's host DUST, vsx_dust_mask -- this file
    restates the orientation, not DUST), --hardmask turns what is masked into N.  DUST with --hardmask does not fold the case
    first (core/mask.cpp:150-158): the DUST intervals become N and the input's own lower case stays, and still poisons"""
    if dbmask == "dust":
        from vsearch_amd import dust_mask
        dusted = [m.decode("latin-1") for m in dust_mask(list(db))] if db else []
        if hardmask:
            return ["".join("N" if m.islower() else c for c, m in zip(s, d)) for s, d in zip(db, dusted)]
        return dusted
    if hardmask and dbmask == "soft":
        return ["".join("N" if c.islower() else c for c in s) for s in db]
    return list(db)


def words_of(seq, w, lower_poisons):
    """the distinct valid words of a sequence as strings over ACGT (U = T), in first-occurrence order"""
    seen, out = set(), []
    for p in range(len(seq) - w + 1):
        word = seq[p:p + w]
        if any(c not in "ACGTUacgtu" for c in word) or (lower_poisons and any(c.islower() for c in word)):
            continue
        word = word.upper().replace("U", "T")
        if word not in seen:
            seen.add(word)
            out.append(word)
    return out


def match_counts(db, w, dbmask="none", hardmask=0):
    """word -> the number of database sequences that contain it"""
    mc = {}
    for s in masked_db(db, dbmask, hardmask):
        for word in words_of(s, w, dbmask != "none"):
            mc[word] = mc.get(word, 0) + 1
    return mc


def py_orient(s):
    """-> per query dict(count_fwd, count_rev, strand '+-?', words = [(word, hf, hr)], text, qual)"""
    o = full_opts(s["opts"])
    w = o["wordlength"]
    mc = match_counts(s["db"], w, o["dbmask"], o["hardmask"])
    quals = s.get("quals") or [None] * len(s["queries"])
    out = []
    for q, qual in zip(s["queries"], quals):
        nf = nr = 0
        words = []
        for word in words_of(q, w, o["qmask"] != "none"):
            hf, hr = mc.get(word, 0), mc.get(revcomp(word), 0)
            words.append((word, hf, hr))
            if hf > (8 * hr) % 2 ** 32:
                nf += 1
            elif hr > (8 * hf) % 2 ** 32:
                nr += 1
        strand = "+" if nf >= 1 and nf >= 4 * nr else "-" if nr >= 1 and nr >= 4 * nf else "?"
        out.append(dict(count_fwd=nf, count_rev=nr, strand=strand, words=words, text=revcomp(q) if strand == "-" else q,
                        qual=None if qual is None else qual[::-1] if strand == "-" else qual))
    return out


def sizes_of(s):
    """the abundances the writers print: the header's size annotation, else 1 -- with or without --sizein
    (fastx_get_abundance, core/fasta.cpp:353-363, reads the header whenever it is asked)"""
    out = []
    for h in s["qlabels"]:
        m = re.search(r"(?:^|;)size=(\d+)(?:;|$)", h)
        out.append(int(m.group(1)) if m else 1)
    return out


# ---- the input sets -----------------------------------------------------------------------------------------------------------
def markers(rng, n, w):
    """n words of length w: none its own reverse complement, no two equal or reverse complements of each other"""
    out, taken = [], set()
    while len(out) < n:
        m = random_seq(rng, w)
        if m == revcomp(m) or m in taken or revcomp(m) in taken:
            continue
        taken.add(m)
        out.append(m)
    return out


def marker_db(pairs):
    """[(marker, hf, hr)] -> database sequences: hf that hold the marker, hr that hold its reverse complement"""
    db = []
    for m, hf, hr in pairs:
        db += [PAD + m + PAD] * hf + [PAD + revcomp(m) + PAD] * hr
    return db


def joined(parts):
    return "N".join(parts)


def _set(name, db, queries, opts=None, qlabels=None, quals=None, db_labels=None):
    return dict(name=name, db=list(db), db_labels=db_labels or [f"t{i}" for i in range(len(db))], queries=list(queries),
                qlabels=qlabels or [f"q{i}" for i in range(len(queries))], quals=quals, opts=opts or {})


RATIO_EDGES = ((8, 1), (9, 1), (1, 8), (1, 9), (16, 2), (17, 2), (1, 0), (0, 1), (0, 0))
VERDICT_EDGES = ((0, 0), (1, 0), (0, 1), (1, 1), (4, 1), (3, 1), (1, 4), (1, 3), (8, 2), (7, 2))


def ratio_set(w=12):
    """one marker per (hf, hr) edge; query k is marker k alone, so its counts are (1, 0), (0, 1) or (0, 0)"""
    rng = random.Random(201)
    ms = markers(rng, len(RATIO_EDGES), w)
    return _set("ratio_edges", marker_db([(m, hf, hr) for m, (hf, hr) in zip(ms, RATIO_EDGES)]), ms, dict(wordlength=w, dbmask="none"))


def verdict_set(w=12):
    """eight markers the database holds forward and four it holds reverse-complemented; a query of a + b of them counts (a, b)"""
    rng = random.Random(211)
    ms = markers(rng, 12, w)
    fwd, rev = ms[:8], ms[8:]
    db = marker_db([(m, 1, 0) for m in fwd] + [(m, 0, 1) for m in rev])
    return _set("verdict_edges", db, [joined(fwd[:a] + rev[:b]) for a, b in VERDICT_EDGES], dict(wordlength=w, dbmask="none"))


def palindrome_set(w=12):
    """a word that is its own reverse complement, in three database sequences: hf = hr, it never counts"""
    rng = random.Random(223)
    half = random_seq(rng, w // 2)
    pal = half + revcomp(half)
    m = markers(rng, 1, w)[0]
    db = [PAD + pal + PAD] * 3 + marker_db([(m, 1, 0)])
    return _set("palindromes", db, [pal, joined([pal, m]), joined([pal, pal])], dict(wordlength=w, dbmask="none"))


def repeats_set(w=12):
    """a word twice in the query counts once; a word twice in ONE database sequence counts once (seven sequences with the marker
    once and one with it twice make hf = 8, not 9: against hr = 1 no count); a word in several sequences counts each (nine: a count)"""
    rng = random.Random(227)
    a, b, c = markers(rng, 3, w)
    db = marker_db([(a, 1, 0)])
    db += [PAD + b + PAD] * 7 + [PAD + b + "N" + b + PAD] + [PAD + revcomp(b) + PAD]
    db += [PAD + c + PAD] * 9 + [PAD + revcomp(c) + PAD]
    return _set("repeats", db, [joined([a, a, a]), b, c, joined([a, b, c, c])], dict(wordlength=w, dbmask="none"))


def length_set(w=12):
    """queries of w - 1, w and w + 1 symbols, and an empty one"""
    rng = random.Random(229)
    m = markers(rng, 1, w)[0]
    return _set("query_lengths", marker_db([(m, 1, 0)]), [m[:w - 1], m, m + "A", "A" + m, ""], dict(wordlength=w, dbmask="none"))


def alphabet_sets(w=12):
    """U for T, every ambiguity code inside the marker, lower case under each --qmask, and an upper-case low-complexity query DUST
    would mask: the reference does not mask the query of this command, so its words count"""
    rng = random.Random(233)
    m = markers(rng, 1, w)[0]
    while "T" not in m:
        m = markers(rng, 1, w)[0]
    low = "A" * 48
    db = marker_db([(m, 1, 0)]) + [low]
    qs = [m, m.replace("T", "U"), m.replace("T", "u"), m.lower(), m[:3] + m[3:].lower(), low, low.lower(), joined([m, low])]
    qs += [m[:w // 2] + c + m[w // 2 + 1:] for c in AMBIGUOUS + AMBIGUOUS.lower()]
    return [_set(f"alphabet_qmask_{mode}", db, qs, dict(wordlength=w, dbmask="none", qmask=mode)) for mode in ("none", "soft", "dust")]


def dbmask_sets(w=12):
    """a lower-case marker and a low-complexity run in the database under every --dbmask, and --hardmask"""
    rng = random.Random(239)
    a, b = markers(rng, 2, w)
    flank = random_seq(rng, 60)
    low = "AC" * 30
    db = [flank[:30] + a.lower() + flank[30:], PAD + b + PAD, random_seq(rng, 40) + low + random_seq(rng, 40)]
    qs = [a, b, low, flank, joined([a, b])]
    out = [_set(f"dbmask_{mode}", db, qs, dict(wordlength=w, dbmask=mode)) for mode in ("none", "soft", "dust")]
    out += [_set(f"dbmask_{mode}_hardmask", db, qs, dict(wordlength=w, dbmask=mode, hardmask=1)) for mode in ("soft", "dust")]
    return out


def mixed_inputs(seed=241, n_db=6, length=160):
    rng = random.Random(seed)
    db = [random_seq(rng, length) for _ in range(n_db)]
    qs = [db[0][10:150], revcomp(db[1][5:140]), random_seq(rng, 120), db[2][:70] + revcomp(db[3][70:140]), db[4][20:60] + "N" + revcomp(db[5][30:50]),
          db[0][:40].lower() + db[0][40:100], revcomp(db[2]), "ACGT"]
    return db, qs


def wordlength_sets():
    db, qs = mixed_inputs()
    return [_set(f"wordlength_{w}", db, qs, dict(wordlength=w)) for w in (3, 8, 9, 12, 13)]


def wordlength_15_set():
    """checked against py_orient() only: the reference CLI's tables at 15 take gigabytes"""
    db, qs = mixed_inputs()
    return _set("wordlength_15", db, qs, dict(wordlength=15))


def output_sets():
    """FASTA and FASTQ input with the header options of the writers; a read of 100 symbols folds at the default width"""
    rng = random.Random(251)
    db, qs = mixed_inputs(seed=257)
    qs = qs[:6] + [db[1][:100], revcomp(db[1][:100])]
    labels = ["plain", "sized;size=5", "size=7;first", "mid;size=3;tail", "trail;size=12;", "nosize;", "long;size=2", "longrev"]
    quals = ["".join(chr(33 + rng.randrange(41)) for _ in q) for q in qs]
    out = [_set("outputs_fasta", db, qs, {}, labels),
           _set("outputs_fastq", db, qs, {}, labels, quals),
           _set("outputs_sizein_sizeout", db, qs, dict(sizein=1, sizeout=1), labels, quals),
           _set("outputs_sizeout", db, qs, dict(sizeout=1), labels),
           _set("outputs_xsize", db, qs, dict(xsize=1), labels, quals),
           _set("outputs_relabel", db, qs, dict(relabel="read", sizein=1, sizeout=1), labels, quals),
           _set("outputs_width_0", db, qs, dict(fasta_width=0), labels),
           _set("outputs_width_7", db, qs, dict(fasta_width=7), labels),
           _set("outputs_no_queries", db, [], {}, [])]
    return out


def golden_sets():
    return ([ratio_set(), verdict_set(), palindrome_set(), repeats_set(), length_set()] + alphabet_sets() + dbmask_sets()
            + wordlength_sets() + output_sets())


EDGES = {
    # set name -> what py_orient() must show for the set to reach the edge it is named after (tests/test_orient_host.py)
    "ratio_edges": "ratio", "verdict_edges": "verdict", "palindromes": "palindrome", "repeats": "repeats", "query_lengths": "lengths",
}


# ---- simulated reads (the live comparison and the benchmark) ---------------------------------------------------------------------
def simulated(seed, n_db, db_len, n_reads, read_len, flipped=0.5, unrelated=0.1, errors=0.02):
    """-> (db, reads): reads cut from the database with substitutions, a share reverse-complemented, a share unrelated"""
    rng = random.Random(seed)
    db = [random_seq(rng, db_len) for _ in range(n_db)]
    reads = []
    for k in range(n_reads):
        if rng.random() < unrelated:
            reads.append(random_seq(rng, read_len))
            continue
        t = db[rng.randrange(n_db)]
        a = rng.randrange(0, db_len - read_len + 1)
        r = list(t[a:a + read_len])
        for i in range(read_len):
            if rng.random() < errors:
                r[i] = rng.choice("ACGT")
        r = "".join(r)
        reads.append(revcomp(r) if rng.random() < flipped else r)
    return db, reads


# ---- the reference CLI -----------------------------------------------------------------------------------------------------------
def ref_binary():
    return os.path.join(ROOT, "oracle", "_ref", "vsearch_ref")


def write_fasta(path, names, seqs):
    with open(path, "w") as f:
        for n, s in zip(names, seqs):
            f.write(f">{n}\n{s}\n")


def write_fastq(path, names, seqs, quals):
    with open(path, "w") as f:
        for n, s, q in zip(names, seqs, quals):
            f.write(f"@{n}\n{s}\n+\n{q}\n")


def cli_args(opts):
    o = full_opts(opts)
    a = ["--wordlength", str(o["wordlength"]), "--qmask", o["qmask"], "--dbmask", o["dbmask"], "--fasta_width", str(o["fasta_width"])]
    for flag in ("hardmask", "sizein", "sizeout", "xsize"):
        if o[flag]:
            a.append("--" + flag)
    if o["relabel"] is not None:
        a += ["--relabel", o["relabel"]]
    return a


def run_reference(s, threads=1, outputs=("tabbed", "fasta", "fastq", "notmatched", "log")):
    """-> dict(tabbed, fasta, fastq (None for FASTA input), notmatched, log): the lines of each output"""
    fastq = s.get("quals") is not None
    with tempfile.TemporaryDirectory(prefix="vsx_orient_") as tmp:
        p = lambda n: os.path.join(tmp, n)
        write_fasta(p("db.fa"), s["db_labels"], s["db"])
        if fastq:
            write_fastq(p("q.fx"), s["qlabels"], s["queries"], s["quals"])
        else:
            write_fasta(p("q.fx"), s["qlabels"], s["queries"])
        args = [ref_binary(), "--orient", p("q.fx"), "--db", p("db.fa"), "--threads", str(threads), "--log", p("log.txt"), "--quiet"]
        args += ["--tabbedout", p("tabbed"), "--fastaout", p("fasta"), "--notmatched", p("notmatched")]
        if fastq:
            args += ["--fastqout", p("fastq")]
        r = subprocess.run(args + cli_args(s["opts"]), capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{s['name']}: reference CLI failed: {r.stderr[-2000:]}")
        read = lambda n: open(p(n)).read().split("\n")[:-1]
        out = {k: read(k) for k in ("tabbed", "fasta", "notmatched") if k in outputs}
        if "fastq" in outputs:
            out["fastq"] = read("fastq") if fastq else None
        if "log" in outputs:
            out["log"] = [l for l in open(p("log.txt")).read().splitlines() if re.match(r"(Forward|Reverse|All|Not) oriented|Total number", l)]
        return out


def writer_kw(s):
    """the writers' keyword arguments for a set's options"""
    o = full_opts(s["opts"])
    return dict(sizes=sizes_of(s), sizeout=bool(o["sizeout"]), xsize=bool(o["xsize"]), relabel=o["relabel"], fasta_width=o["fasta_width"])


def assert_text_equals_golden(res, s):
    """every formatter of vsearch_amd.orient on a result of set `s` against the reference's recorded text, byte for byte"""
    from vsearch_amd.orient import tabbed_lines, fasta_lines, fastq_lines, notmatched_lines, log_lines
    ref, kw = s["ref"], writer_kw(s)
    assert tabbed_lines(res, s["qlabels"]) == ref["tabbed"], s["name"]
    assert fasta_lines(res, s["qlabels"], **kw) == ref["fasta"], s["name"]
    assert notmatched_lines(res, s["qlabels"], **kw) == ref["notmatched"], s["name"]
    if s["quals"] is not None:
        assert fastq_lines(res, s["qlabels"], **kw) == ref["fastq"], s["name"]
    else:
        assert ref["fastq"] is None
    assert log_lines(res) == ref["log"], s["name"]


INPUT_KEYS = ("name", "db", "db_labels", "queries", "qlabels", "quals", "opts")
SHARED_KEYS = ("db", "db_labels", "queries", "qlabels", "quals")


def write_golden(path=GOLDEN):
    """a set whose inputs equal an earlier set's (other options on the same input) is stored as a reference to it"""
    sets, stored = [], []
    for s in golden_sets():
        rec = {k: s[k] for k in INPUT_KEYS}
        rec["ref"] = run_reference(s)
        sets.append(rec)
        same = next((t["name"] for t in sets[:-1] if all(t[k] == rec[k] for k in SHARED_KEYS)), None)
        stored.append(dict(name=rec["name"], opts=rec["opts"], same_inputs_as=same, ref=rec["ref"]) if same else rec)
    with open(path, "w") as f:
        json.dump(dict(sets=stored), f, indent=0, separators=(",", ":"))
        f.write("\n")
    return sets


def load_golden(path=GOLDEN):
    with open(path) as f:
        stored = json.load(f)["sets"]
    by_name, sets = {}, []
    for rec in stored:
        if "same_inputs_as" in rec:
            base = by_name[rec["same_inputs_as"]]
            rec = dict({k: base[k] for k in SHARED_KEYS}, name=rec["name"], opts=rec["opts"], ref=rec["ref"])
        by_name[rec["name"]] = rec
        sets.append(rec)
    return sets


if __name__ == "__main__":
    for rec in write_golden():
        got = [f"{r['strand']}{r['count_fwd']}/{r['count_rev']}" for r in py_orient(rec)]
        ref = ["".join(l.split("\t")[1:2]) + "/".join(l.split("\t")[2:]) for l in rec["ref"]["tabbed"]]
        print(f"{rec['name']}: {len(rec['queries'])} queries, {len(rec['db'])} database sequences; {' '.join(ref)}"
              + ("" if got == ref else f"   PY DIFFERS: {' '.join(got)}"))
