"""Inputs, a plain-Python restatement and the reference-CLI runner for the hit-writer tests (include/vsx_hitout.h,
vsearch_amd/hitout.py).

    explicit_sets()     named sets of explicit hits: a query, a target and a CIGAR chosen by the test, so that the rendering is
                        checked whatever an aligner would pick; assert_coverage() proves from py_render() that they reach every
                        length, run count, MD event, gap shape, symbol and strand case the kernels distinguish
    py_render()         the rows, the symbol row, the --alnout query row and the MD string of every hit, written from the reference's
                        rules (core/showalign.cpp, core/results.cpp) in plain Python
    cli_sets()          small searches that go through the reference CLI with all seven writers; run_reference() runs
                        oracle/_ref/vsearch_ref on one of them, hits_from_records() rebuilds the hit list from the CLI's own --userout
    __main__            records tests/golden/hitout_golden.json: inputs, options and the CLI's files for each CLI set

The kernels walk columns in blocks of 64 and runs in chunks of 64 (vsearch_amd/csrc/vsx_hitout.hip).
"""
import hashlib
import json
import os
import random
import re
import subprocess
import tempfile

import numpy as np

from tests import common

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "hitout_golden.json")

MASK_MODES = {"none": 0, "soft": 1, "dust": 2}
# chrmap_4bit and chrmap_complement of the reference (utils/maps.cpp), as tables over the letters
CODE = dict(zip("ABCDGHKMNRSTUVWY", (1, 14, 2, 13, 4, 11, 12, 3, 15, 5, 6, 8, 8, 7, 9, 10)))
COMPLEMENT = dict(zip("ABCDGHKMNRSTUVWY", "TVGHCDMKNYSAABWR"))
WRITERS = ("alnout", "samout", "blast6out", "fastapairs", "qsegout", "tsegout", "userout")
# what hits_from_records() needs of a hit, printed by the CLI itself
RECORD_FIELDS = ("query", "target", "qstrand", "caln", "raw", "ids", "mism")


def code(c):
    return CODE.get(c.upper(), 0)


def complement(c):
    r = COMPLEMENT.get(c.upper())
    return "N" if r is None else (r.lower() if c.islower() else r)


def revcomp(s):
    return "".join(complement(c) for c in reversed(s))


def runs_of(cigar):
    out, n, digits = [], 0, False
    for ch in cigar:
        if ch.isdigit():
            n, digits = n * 10 + int(ch), True
        else:
            out.append((n if digits else 1, ch))
            n, digits = 0, False
    return out


def cigar_of(ops):
    """column operations "MMDI..." -> CIGAR text as the reference writes it (a count of 1 omitted)"""
    out, i = [], 0
    while i < len(ops):
        j = i
        while j < len(ops) and ops[j] == ops[i]:
            j += 1
        out.append(("" if j - i == 1 else str(j - i)) + ops[i])
        i = j
    return "".join(out)


# ---- options: one dict describes a set's command line, the session's options and the restatement's ------------------------------
DEFAULT_OPTS = dict(strand_both=1, qmask="none", dbmask="none", hardmask=0, n_mismatch=0)


def full_opts(opts):
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    return o


def session_opts(opts):
    """keyword options of SearchSession / render_host for a set (the masking and the strands)"""
    o = full_opts(opts)
    kw = dict(strand_both=o["strand_both"], soft_mask=MASK_MODES[o["dbmask"]], hardmask=3 if o["hardmask"] else 0)
    if o["qmask"] != o["dbmask"]:
        kw["qmask"] = 1 + MASK_MODES[o["qmask"]]
    return kw


def masked(seqs, mode, hard):
    """the text after --qmask / --dbmask `mode` (+ --hardmask); the DUST intervals come from the library's host DUST
    (vsx_dust_mask) -- the restatement restates the writers, not DUST"""
    seqs = list(seqs)
    if mode == "dust":
        from vsearch_amd import dust_mask
        dusted = [m.decode("latin-1") for m in dust_mask(seqs)] if seqs else []
        if not hard:
            return dusted
        # --hardmask: the DUST intervals become 'N' and the text keeps its case (core/mask.cpp:137-191)
        return ["".join("N" if d.islower() else c for c, d in zip(s, m)) for s, m in zip(seqs, dusted)]
    if hard and mode == "soft":
        seqs = ["".join("N" if (ord(c) & 0x20) else c for c in s) for s in seqs]
    return seqs


def db_text(s):
    """the database as indexed: what vsx_searcher_db_text returns"""
    o = full_opts(s["opts"])
    return masked(s["db"], o["dbmask"], o["hardmask"])


def strands(s):
    """per query (plus text, minus text or None), each strand masked on its own (core/search.cpp:294-303)"""
    o = full_opts(s["opts"])
    plus = masked(s["queries"], o["qmask"], o["hardmask"])
    minus = masked([revcomp(q) for q in s["queries"]], o["qmask"], o["hardmask"]) if o["strand_both"] else [None] * len(plus)
    return list(zip(plus, minus))


# ---- the plain-Python restatement -------------------------------------------------------------------------------------------------
def symbol(qc, tc, n_mismatch):
    """get_aligment_symbol (showalign.cpp:122-137)"""
    q, t = code(qc), code(tc)
    if n_mismatch and (q == 15 or t == 15):
        return " "
    if q == t and q in (1, 2, 4, 8):
        return "|"
    if q & t:
        return "+"
    return " "


def py_render_hit(plus, minus, target, strand, cigar, c0, ilen, n_mismatch):
    qs = minus if strand else plus
    qrow, trow, sym, aln, md = [], [], [], [], []
    qpos = tpos = matched = 0
    flag = False
    for n, op in runs_of(cigar):
        if op == "I":
            if not flag:
                md.append(str(matched))
                matched = 0
            md.append("^" + target[tpos:tpos + n])
            flag = False
        for _ in range(n):
            qc = qs[qpos] if op != "I" else "-"
            tc = target[tpos] if op != "D" else "-"
            ac = qc
            if strand and op != "I":
                ac = complement(plus[len(plus) - 1 - qpos])           # showalign.cpp:179-185,345
            qrow.append(qc)
            trow.append(tc)
            aln.append(ac)
            sym.append(symbol(ac, tc, n_mismatch) if op == "M" else " ")
            if op == "M":
                if code(qc) == code(tc):
                    matched += 1
                else:
                    if not flag:
                        md.append(str(matched))
                        matched = 0
                    md.append(tc)
                    flag = False
            qpos += op != "I"
            tpos += op != "D"
    if not flag:
        md.append(str(matched))
    assert qpos == len(qs) and tpos == len(target), (cigar, qpos, len(qs), tpos, len(target))
    cut = lambda r: "".join(r[c0:c0 + ilen])
    return dict(qrow=cut(qrow), trow=cut(trow), sym=cut(sym), aln=cut(aln), md="".join(md), ncols=len(qrow), nruns=len(runs_of(cigar)),
                c0=c0, ilen=ilen)


def trim_of(cigar):
    """align_trim (core/searchcore.cpp:343-421): (trim_q_left, trim_q_right, trim_t_left, trim_t_right)"""
    rs = runs_of(cigar)
    total = sum(n for n, _ in rs)
    ql = qr = tl = tr = 0
    if rs and rs[0][1] != "M":
        ql, tl = (rs[0][0], 0) if rs[0][1] == "D" else (0, rs[0][0])
    if rs and rs[-1][1] != "M":
        qr, tr = (rs[-1][0], 0) if rs[-1][1] == "D" else (0, rs[-1][0])
    if ql >= total:
        qr = 0
    if tl >= total:
        tr = 0
    return ql, qr, tl, tr


def hit_record(q, t, strand, cigar, qlen, tlen, matches, mismatches, raw=0):
    """a vsx_hit as the search fills it from an alignment (align_trim, iddef 2); nwid and nwdiff are not printed by any writer"""
    rs = runs_of(cigar)
    cols = sum(n for n, _ in rs)
    indels = sum(n for n, op in rs if op != "M")
    gaps = sum(1 for _, op in rs if op != "M")
    ql, qr, tl, tr = trim_of(cigar)
    ilen = cols - ql - qr - tl - tr
    shortest, longest = min(qlen, tlen), max(qlen, tlen)
    id1 = 100.0 * matches / cols if cols > 0 else 0.0
    id2 = 100.0 * matches / ilen if ilen > 0 else 0.0
    return dict(query=q, target=t, count=0, accepted=1, weak=0, used_fallback=0, strand=strand, nwscore=raw, nwdiff=cols - matches, nwgaps=gaps,
                nwindels=indels, nwalignmentlength=cols, matches=matches, mismatches=mismatches, internal_alignmentlength=ilen,
                internal_gaps=gaps - (1 if ql + tl > 0 else 0) - (1 if qr + tr > 0 else 0), internal_indels=indels - ql - qr - tl - tr,
                trim_q_left=ql, trim_q_right=qr, trim_t_left=tl, trim_t_right=tr, shortest=shortest, longest=longest, nwid=id1, id=id2,
                id0=100.0 * matches / shortest if shortest > 0 else 0.0, id1=id1, id2=id2,
                id3=max(0.0, 100.0 * (1.0 - (1.0 * (mismatches + gaps) / longest))) if longest else 0.0, id4=id1, cigar=cigar)


def raw_hits(n_queries, records):
    """(first, hits, cigar blob) as SearchSession.search_batch_raw returns them, from hit_record dicts grouped by ascending query"""
    from vsearch_amd import _lib
    hits = np.zeros(len(records), dtype=np.dtype(_lib.Hit))
    first = np.zeros(n_queries + 1, np.uint64)
    blob = b""
    for k, r in enumerate(records):
        assert k == 0 or records[k - 1]["query"] <= r["query"]
        for f, v in r.items():
            if f != "cigar":
                hits[k][f] = v
        hits[k]["cigar_off"] = len(blob)
        blob += r["cigar"].encode() + b"\0"
        first[r["query"] + 1] += 1
    return np.cumsum(first, dtype=np.uint64), hits, blob


def explicit_records(s):
    """the hit records of an explicit set: matches and mismatches counted over the 'M' columns by 4-bit code"""
    st, dbt, out = strands(s), db_text(s), []
    for q, t, strand, cigar in s["hits"]:
        qs = st[q][1] if strand else st[q][0]
        m = x = qpos = tpos = 0
        for n, op in runs_of(cigar):
            for _ in range(n):
                if op == "M":
                    same = code(qs[qpos]) == code(dbt[t][tpos])
                    m, x = m + same, x + (not same)
                qpos += op != "I"
                tpos += op != "D"
        out.append(hit_record(q, t, strand, cigar, len(qs), len(dbt[t]), m, x))
    return out


def py_render(s, records=None):
    """one dict per hit (py_render_hit), in hit order"""
    st, dbt = strands(s), db_text(s)
    o = full_opts(s["opts"])
    records = explicit_records(s) if records is None else records
    return [py_render_hit(st[r["query"]][0], st[r["query"]][1], dbt[r["target"]], r["strand"], r["cigar"],
                          r["trim_q_left"] + r["trim_t_left"], r["internal_alignmentlength"], o["n_mismatch"]) for r in records]


# ---- explicit sets ------------------------------------------------------------------------------------------------------------------
def from_ops(rng, ops, mismatches=(), alphabet="ACGT"):
    """a (query, target) pair whose alignment is exactly `ops`: 'M' columns match except at the listed columns"""
    q, t = [], []
    for c, op in enumerate(ops):
        b = rng.choice(alphabet)
        if op == "M":
            q.append(b)
            t.append(rng.choice([x for x in alphabet if x != b]) if c in mismatches else b)
        elif op == "D":
            q.append(b)
        else:
            t.append(b)
    return "".join(q), "".join(t)


def _explicit(name, pairs, opts=None):
    """pairs: (query, target, strand, cigar); query k and target k belong to hit k"""
    return dict(name=name, db=[p[1] for p in pairs], queries=[p[0] for p in pairs], opts=opts or {},
                hits=[(k, k, p[2], p[3]) for k, p in enumerate(pairs)], names=[f"q{k}" for k in range(len(pairs))],
                db_names=[f"t{k}" for k in range(len(pairs))])


def lengths_set():
    """alignment lengths around the 64-column block, each with a mismatch in its last column"""
    rng = random.Random(401)
    return _explicit("lengths", [from_ops(rng, "M" * n, {n - 1}) + (0, cigar_of("M" * n)) for n in (1, 63, 64, 65, 127, 128, 129)])


def run_counts_set():
    """1, 63, 64, 65 and 129 runs: the chunk of 64 run words, its edges and two carries"""
    rng = random.Random(409)
    pairs = []
    for nr in (1, 63, 64, 65, 129):
        ops = "".join(("M" if k % 2 == 0 else "DI"[(k // 2) % 2]) * (1 + k % 3) for k in range(nr))      # an even count ends in a terminal gap
        assert len(runs_of(cigar_of(ops))) == nr, (nr, cigar_of(ops))
        pairs.append(from_ops(rng, ops, {0}) + (0, cigar_of(ops)))
    return _explicit("run_counts", pairs)


def md_events_set():
    rng = random.Random(419)
    pairs = [from_ops(rng, "M" * 130, {0, 63}) + (0, "130M"),                       # events at lane 0 and lane 63
             from_ops(rng, "M" * 40, {10, 11}) + (0, "40M"),                          # adjacent events: a 0 between them
             from_ops(rng, "M" * 201, {200}) + (0, "201M")]                           # a carry through three blocks without an event
    counts, at, mism = (9, 10, 99, 100, 999, 1000), 0, set()
    for c in counts:
        at += c
        mism.add(at)
        at += 1
    pairs.append(from_ops(rng, "M" * (at + 3), mism) + (0, f"{at + 3}M"))
    return _explicit("md_events", pairs)


def gaps_set():
    rng = random.Random(421)
    shapes = ["DDD" + "M" * 20 + "III", "II" + "M" * 20 + "DD",                      # terminal gaps of both kinds, both ends
              "MMMMM" + "III" + "DD" + "MMMMM" + "DD" + "III" + "MMMMM",              # I directly followed by D, and the reverse
              "MMMMM" + "III" + "M" * 5,                                              # a mismatch directly after an I run (column 8)
              "M" * 60 + "I" * 10 + "M" * 20,                                         # an I run across a block edge
              "M" * 10 + "I" * 70 + "M" * 10]                                         # ... and across a whole block
    pairs = [from_ops(rng, ops, {8} if k == 3 else ()) + (0, cigar_of(ops)) for k, ops in enumerate(shapes)]
    pairs.append(("", "ACGTA", 0, "5I"))                                             # all gap: a zero-length query
    return _explicit("gaps", pairs)


def symbols_sets():
    """N with and without n_mismatch, R against A ('+'), R against R ('+', not '|'), U against T, lower case on either side"""
    pairs = [("ANNRRUTacgtNX", "NANARTUACGtnA", 0, "13M"), ("ACGURYN", "ACGTRYN", 0, "7M")]
    return [_explicit("symbols", pairs), _explicit("symbols_n_mismatch", pairs, dict(n_mismatch=1))]


def minus_set():
    """minus-strand hits under DUST: the plus strand's masked text read backwards differs in case from the separately masked
    reverse complement, so the --alnout row differs from qrow; and the same under --hardmask, where the rows differ in 'N'"""
    rng = random.Random(431)
    for _ in range(2000):
        q = "".join(rng.choice("ACGT") for _ in range(40)) + rng.choice(["AC", "AAT", "A", "GT"]) * 14 + "".join(rng.choice("ACGT") for _ in range(30))
        s = dict(queries=[q], db=[], opts=dict(qmask="dust"))
        plus, minus = strands(s)[0]
        if revcomp(plus) != minus:
            break
    else:
        raise AssertionError("no query whose strands DUST differently")
    t = revcomp(q)
    t = t[:50] + ("A" if t[50] != "A" else "C") + t[51:]
    pairs = [(q, t, 1, f"{len(q)}M"), (q, t[3:] + "GG", 1, f"3D{len(q) - 3}M2I")]
    return [_explicit("minus_dust", pairs, dict(qmask="dust")), _explicit("minus_hardmask", pairs, dict(qmask="dust", hardmask=1))]


def explicit_sets():
    return [lengths_set(), run_counts_set(), md_events_set(), gaps_set()] + symbols_sets() + minus_set()


def random_triples(seed, n=3000, alphabet="ACGTNRYacgtn"):
    """seeded random (query, target, valid CIGAR) triples on both strands, as one explicit set"""
    rng = random.Random(seed)
    pairs = []
    for _ in range(n):
        L = rng.choice((0, 1, 2, 5, 30, 63, 64, 65, 100, 130, 200))
        ops, runs = [], rng.choice((1, 2, 3, 5, 9, 40))
        for r in range(runs):
            ops.append(rng.choice("MMMDI") * max(1, rng.randrange(1, 2 + 2 * L // runs)))
        ops = "".join(ops) if L else "I" * rng.randrange(1, 4)             # a zero-length query: all gap
        q, t = [], []
        for op in ops:
            b = rng.choice(alphabet)
            if op != "I":
                q.append(b)
            if op != "D":
                t.append(b if rng.random() < 0.8 or op != "M" else rng.choice(alphabet))
        strand = rng.randrange(2)
        q = "".join(q)
        # the CIGAR of a minus-strand hit aligns the reverse complement: hand the library the plus strand of it
        pairs.append((revcomp(q) if strand else q, "".join(t), strand, cigar_of(ops)))
    return _explicit(f"random_{seed}", pairs, dict(qmask="none"))


def coverage(sets):
    """what the sets reach, derived from py_render()"""
    got = dict(ncols=set(), nruns=set(), md=[], shapes=set(), symbols=set(), minus_rows_differ=0, empty_query=0)
    for s in sets:
        o = full_opts(s["opts"])
        for (q, t, strand, cigar), r in zip(s["hits"], py_render(s)):
            got["ncols"].add(r["ncols"])
            got["nruns"].add(r["nruns"])
            got["md"].append(r["md"])
            rs = runs_of(cigar)
            ops = [op for _, op in rs]
            got["shapes"].update({"lead" + ops[0], "trail" + ops[-1]} if ops else ())
            got["shapes"].update(a + b for a, b in zip(ops, ops[1:]))
            col = 0
            for n, op in rs:
                if op == "I" and col // 64 != (col + n - 1) // 64:
                    got["shapes"].add("I_across_block")
                col += n
            if strand and r["aln"] != r["qrow"]:
                got["minus_rows_differ"] += 1
            got["empty_query"] += len(s["queries"][q]) == 0 and r["ilen"] == 0
            for a, b, c in zip(r["aln"], r["trow"], r["sym"]):
                got["symbols"].add((a, b, c, o["n_mismatch"]))
    return got


def assert_coverage(sets=None):
    g = coverage(explicit_sets() if sets is None else sets)
    assert {1, 63, 64, 65, 127, 128, 129} <= g["ncols"], sorted(g["ncols"])
    assert {1, 63, 64, 65, 129} <= g["nruns"], sorted(g["nruns"])
    md = g["md"]
    numbers = lambda m: [int(x) for x in re.findall(r"\d+", m)]
    assert any(re.fullmatch(r"0[ACGT]62[ACGT]66", m) for m in md), "events at lane 0 and lane 63"
    assert any(re.fullmatch(r"10[ACGT]0[ACGT]28", m) for m in md), "two adjacent events: a 0 between them"
    assert any(re.fullmatch(r"200[ACGT]0", m) for m in md), "a carry through blocks without an event"
    assert any(numbers(m) == [9, 10, 99, 100, 999, 1000, 3] and "^" not in m for m in md), "match counts around every digit count"
    assert any(re.search(r"\^[ACGT]{3}0[ACGT]", m) for m in md), "a mismatch directly after an I run"
    assert {"leadD", "leadI", "trailD", "trailI", "ID", "DI", "IM", "I_across_block"} <= g["shapes"], sorted(g["shapes"])
    assert g["empty_query"] >= 1
    sy = g["symbols"]
    assert ("N", "A", "+", 0) in sy and ("N", "A", " ", 1) in sy and ("R", "A", "+", 0) in sy and ("R", "R", "+", 0) in sy
    assert ("U", "T", "|", 0) in sy and ("a", "A", "|", 0) in sy and ("t", "t", "|", 0) in sy and ("X", "A", " ", 0) in sy
    assert g["minus_rows_differ"] >= 2
    return g


# ---- the reference CLI ----------------------------------------------------------------------------------------------------------------
def ref_binary():
    return os.path.join(ROOT, "oracle", "_ref", "vsearch_ref")


def write_fasta(path, names, seqs):
    with open(path, "w") as f:
        for n, s in zip(names, seqs):
            f.write(f">{n}\n{s}\n")


def cli_args(s):
    """the options of a set as the CLI takes them; `fmt` are the writers' own"""
    o, f = full_opts(s["opts"]), s["fmt"]
    a = ["--strand", "both" if o["strand_both"] else "plus", "--qmask", o["qmask"], "--dbmask", o["dbmask"], "--fasta_width", str(f.get("fasta_width", 80)),
         "--rowlen", str(f.get("rowlen", 64))]
    if o["hardmask"]:
        a.append("--hardmask")
    if o["n_mismatch"]:
        a.append("--n_mismatch")
    if f.get("maxhits"):
        a += ["--maxhits", str(f["maxhits"])]
    if f.get("top_hits_only"):
        a.append("--top_hits_only")
    if f.get("output_no_hits"):
        a.append("--output_no_hits")
    return a + list(s["search_args"])


def run_reference(s, tmp=None, threads=1):
    """the reference CLI on one set -> dict of the seven files' text, `userout_reversed`, `records` (the hits as the CLI lists them)
    and `samheader`.  The program is started under the name "vsearch" from inside the directory of its inputs, so that the @PG and @SQ
    lines of the SAM header name no path."""
    from vsearch_amd.hitout import USERFIELDS
    own = tempfile.TemporaryDirectory(prefix="vsx_hitout_") if tmp is None else None
    tmp = own.name if own else str(tmp)
    try:
        write_fasta(os.path.join(tmp, "db.fa"), s["db_names"], s["db"])
        write_fasta(os.path.join(tmp, "q.fa"), s["names"], s["queries"])
        base = ["vsearch", "--" + s["command"], "q.fa", "--db", "db.fa", "--threads", str(threads), "--quiet"] + cli_args(s)
        out = {}

        def run(extra):
            r = subprocess.run(base + extra, executable=ref_binary(), cwd=tmp, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"{s['name']}: reference CLI failed: {r.stderr[-2000:]}")

        read = lambda n: open(os.path.join(tmp, n), newline="").read()
        run([x for w in WRITERS for x in ("--" + w, w + ".txt")] + ["--userfields", "+".join(USERFIELDS), "--samheader"])
        for w in WRITERS:
            out[w] = read(w + ".txt")
        # --alnout opens with the command line and the program's banner (which describes the machine): they are not recorded
        out["alnout"] = "".join(out["alnout"].splitlines(True)[2:])
        head = [l for l in out["samout"].splitlines(True) if l.startswith("@")]
        out["samheader"] = "".join(head)
        out["samout"] = out["samout"][len(out["samheader"]):]
        run(["--userout", "rev.txt", "--userfields", "+".join(reversed(USERFIELDS))])
        out["userout_reversed"] = read("rev.txt")
        # the hit list itself: every hit the search kept, whatever the writers' own options cut away
        keep = [a for a in base if a not in ("--top_hits_only", "--output_no_hits")]
        if "--maxhits" in keep:
            k = keep.index("--maxhits")
            del keep[k:k + 2]
        r = subprocess.run(keep + ["--userout", "rec.txt", "--userfields", "+".join(RECORD_FIELDS)], executable=ref_binary(), cwd=tmp, capture_output=True,
                           text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{s['name']}: reference CLI failed: {r.stderr[-2000:]}")
        out["records"] = read("rec.txt")
        return out
    finally:
        if own:
            own.cleanup()


def hits_from_records(s, records):
    """the hit records of a CLI set from the CLI's own listing (RECORD_FIELDS): which hits, their strands, CIGARs and counts; every
    other field follows from the CIGAR as align_trim derives it"""
    qi = {n: k for k, n in enumerate(s["names"])}
    ti = {n: k for k, n in enumerate(s["db_names"])}
    out = []
    for line in records.splitlines():
        f = dict(zip(RECORD_FIELDS, line.split("\t")))
        q, t = qi[f["query"]], ti[f["target"]]
        out.append(hit_record(q, t, 1 if f["qstrand"] == "-" else 0, f["caln"], len(s["queries"][q]), len(s["db"][t]), int(f["ids"]),
                              int(f["mism"]), int(f["raw"])))
    assert all(a["query"] <= b["query"] for a, b in zip(out, out[1:]))
    return out


def format_all(text, s):
    """the seven files (+ the reversed --userout and the SAM header) of a set from rendered hits, as the CLI writes them"""
    from vsearch_amd import hitout as ho
    f = s["fmt"]
    sel = dict(maxhits=f.get("maxhits", 0), top_hits_only=bool(f.get("top_hits_only")))
    nohits = dict(output_no_hits=bool(f.get("output_no_hits")))
    width = f.get("fasta_width", 80)
    join = lambda lines: "".join(l + "\n" for l in lines)
    ql, tl = s["names"], s["db_names"]
    return dict(alnout=ho.alnout_text(text, ql, tl, rowlen=f.get("rowlen", 64), **sel, **nohits),
                samout=join(ho.sam_lines(text, ql, tl, **sel, **nohits)),
                blast6out=join(ho.blast6_lines(text, ql, tl, **sel, **nohits)),
                fastapairs=join(ho.fastapairs_lines(text, ql, tl, fasta_width=width, **sel)),
                qsegout=join(ho.qsegout_lines(text, ql, fasta_width=width, **sel)),
                tsegout=join(ho.tsegout_lines(text, tl, fasta_width=width, **sel)),
                userout=join(ho.userout_lines(text, ql, tl, **sel, **nohits)),
                userout_reversed=join(ho.userout_lines(text, ql, tl, fields=tuple(reversed(ho.USERFIELDS)), **sel, **nohits)))


def sam_header_of(text, s, ref_header):
    """the SAM header of a set; the version and the command line are the recorded @PG line's own"""
    from vsearch_amd import hitout as ho
    pg = dict(x.split(":", 1) for x in ref_header.splitlines()[-1].split("\t")[1:])
    return "".join(l + "\n" for l in ho.sam_header_lines(s["db"], s["db_names"], "db.fa", pg["VN"], pg["CL"]))


# ---- CLI sets ---------------------------------------------------------------------------------------------------------------------------
def _mutate(rng, s, subs, indels):
    s = list(s)
    for _ in range(subs):
        p = rng.randrange(len(s))
        s[p] = rng.choice([b for b in "ACGT" if b != s[p].upper()])
    for _ in range(indels):
        p = rng.randrange(5, len(s) - 5)
        if rng.random() < 0.5:
            del s[p:p + rng.randrange(1, 4)]
        else:
            s[p:p] = [rng.choice("ACGT") for _ in range(rng.randrange(1, 4))]
    return "".join(s)


def _cli_inputs(long=False):
    """one small database and query list shared by the sets: targets of 60, 128 and 121 symbols, a duplicated target (a tied second
    hit), a near copy (an untied one), a copy with a lower-case half, low-complexity stretches (DUST); queries with substitutions,
    indels, overhangs on either side, N, R, U and lower case, reverse complements, a 64-column hit, and one that hits nothing.
    long: a target of 1 100 symbols and a query for it on top (number width 4)"""
    rng = random.Random(443)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    db = [rnd(60), rnd(128), rnd(30) + "AC" * 13 + rnd(30) + "A" * 22 + "T" + rnd(12)]
    db += [db[1], _mutate(rng, db[1], 5, 0), db[0][:30].lower() + db[0][30:]]       # t3 = t1: a tie; t4: an untied hit; t5: lower case
    qs = [db[0], _mutate(rng, db[1], 3, 2), db[1][10:118], "GGTT" + db[0] + "CA", revcomp(_mutate(rng, db[1], 4, 1)), db[2],
          revcomp(_mutate(rng, db[2], 2, 0)), rnd(70), db[0][:20] + "N" + db[0][21:40] + "R" + db[0][41:],
          db[1][:64].replace("T", "U") + db[1][64:].lower(), db[1][:64]]
    if long:
        db.append(rnd(1100))
        qs.append(_mutate(rng, db[-1], 12, 6))
    return db, qs


def _cli(name, opts=None, fmt=None, search_args=("--id", "0.7", "--maxaccepts", "4", "--maxrejects", "16"), command="usearch_global", inputs=None):
    db, qs = inputs or _cli_inputs()
    return dict(name=name, command=command, db=db, queries=qs, opts=opts or {}, fmt=fmt or {}, search_args=list(search_args),
                names=[f"query{k};size={k + 1}" for k in range(len(qs))], db_names=[f"target{k};tax=k:K{k}" for k in range(len(db))])


def cli_sets():
    """`plain` runs everything; the option sets run a few of its queries (0: an exact hit of a target and of its lower-case copy,
    1: indels and a tie, 4: a reverse complement, 5 / 6: low complexity on either strand, 7: no hit, 8: N and R); `long` is one
    short query inside a target of 1 100 symbols"""
    dust = dict(qmask="dust", dbmask="dust")
    db, qs = _cli_inputs()
    pick = lambda *ks: (db, [qs[k] for k in ks])
    two = ("--id", "0.7", "--maxaccepts", "2", "--maxrejects", "16")
    ldb = _cli_inputs(long=True)[0]
    return [_cli("plain"),
            _cli("long", inputs=(ldb[-1:], [ldb[-1][400:460]])),
            _cli("plain_no_hits", fmt=dict(output_no_hits=1, fasta_width=0), inputs=pick(0, 7, 6), search_args=two),
            _cli("rowlen_1", fmt=dict(rowlen=1, maxhits=1, fasta_width=7), inputs=(db[:3], [qs[6]])),
            _cli("rowlen_0", fmt=dict(rowlen=0, top_hits_only=1, output_no_hits=1), inputs=pick(1, 7, 4)),
            _cli("dust", opts=dust, inputs=pick(0, 5, 6, 7), search_args=two),
            _cli("dust_hardmask", opts=dict(dust, hardmask=1), fmt=dict(output_no_hits=1), inputs=pick(0, 5, 6, 7), search_args=two),
            _cli("n_mismatch", opts=dict(n_mismatch=1), inputs=pick(8), search_args=two),
            _cli("exact", command="search_exact", search_args=(), fmt=dict(output_no_hits=1), inputs=pick(0, 5, 7))]


def live_inputs(seed, n_db=2000, n_q=2000):
    """families of four (3 % apart) with a low-complexity stretch in every fifth family; queries: mutated members on either strand,
    some with overhangs, a twentieth random"""
    rng = random.Random(seed)
    db = []
    for f in range(n_db // 4):
        anc = common.rnd_seq(rng, rng.randrange(180, 260))
        if f % 5 == 0:
            p = rng.randrange(20, 100)
            anc = anc[:p] + rng.choice(("AC", "A", "TTG")) * 12 + anc[p:]
        db += [anc] + [common.mutate(rng, anc, 0.03) for _ in range(3)]
    qs = []
    for _ in range(n_q):
        if rng.random() < 0.05:
            qs.append(common.rnd_seq(rng, 200))
            continue
        q = common.mutate(rng, db[rng.randrange(len(db))], 0.02)
        q = q[rng.randrange(0, 12):len(q) - rng.randrange(0, 12)]
        if rng.random() < 0.2:
            q = common.rnd_seq(rng, 5) + q
        qs.append(revcomp(q) if rng.random() < 0.4 else q)
    return db, qs


INPUT_KEYS = ("name", "command", "db", "queries", "opts", "fmt", "search_args", "names", "db_names")


SHARED_KEYS = ("db", "queries", "names", "db_names")


def write_golden(path=GOLDEN):
    """the sets that use the shared inputs record them once"""
    assert_coverage()
    shared = {k: _cli("shared")[k] for k in SHARED_KEYS}
    sets = []
    for s in cli_sets():
        rec = {k: s[k] for k in INPUT_KEYS if k not in SHARED_KEYS or s[k] != shared[k]}
        rec["ref"] = run_reference(s)
        if s["name"] != "exact":                           # the reversed field order is recorded once
            del rec["ref"]["userout_reversed"]
        sets.append(rec)
    with open(path, "w") as f:
        json.dump(dict(shared=shared, sets=sets), f, indent=0, separators=(",", ":"))
        f.write("\n")
    return sets


def load_golden(path=GOLDEN):
    with open(path) as f:
        g = json.load(f)
    return [dict(g["shared"], **s) for s in g["sets"]]


# ---- the device digest (tests/test_gpu_hitout.py, the poison runs) --------------------------------------------------------------------
def render_explicit(aligner, s, want=7, window=0, host=False):
    """an explicit set through vsx_hits_render on the aligner's device (or the host restatement)"""
    from vsearch_amd import SearchSession
    from vsearch_amd import hitout as ho
    o = full_opts(s["opts"])
    raw = raw_hits(len(s["queries"]), explicit_records(s))
    if host:
        return ho.render_host(db_text(s), s["queries"], raw, want=want, n_mismatch=bool(o["n_mismatch"]), **session_opts(s["opts"]))
    sess = SearchSession(aligner, s["db"], id=0.5, **session_opts(s["opts"]))
    try:
        return ho.render(sess, s["queries"], raw, want=want, window=window)
    finally:
        sess.close()


def device_digest(aligners):
    """one digest over the device route's arrays and blobs of every explicit set; aligners: {n_mismatch: Aligner}"""
    h = hashlib.sha256()
    for s in explicit_sets():
        res = render_explicit(aligners[full_opts(s["opts"])["n_mismatch"]], s)
        if res.stats["hits_host"] or res.stats["hits_device"] != len(s["hits"]):
            raise RuntimeError(f"{s['name']}: the device route did not answer")
        for n in res.ARRAYS:
            a = getattr(res, n)
            h.update(b"-" if a is None else a.tobytes())
        for n in res.BLOBS:
            h.update(getattr(res, n))
    return h.hexdigest()


if __name__ == "__main__":
    import sys
    if "--digest" in sys.argv:
        from vsearch_amd import Aligner, load_library
        with Aligner(device=0) as a0, Aligner(device=0, n_mismatch=True) as a1:
            print("digest", device_digest({0: a0, 1: a1}), "poison", load_library().vsx_internal_poison_byte())
    else:
        for rec in write_golden():
            print(rec["name"], {k: len(v) for k, v in rec["ref"].items()})
        print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
