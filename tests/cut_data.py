"""Inputs, a plain-Python restatement and the reference-CLI runner for the restriction-cutting tests (--cut).

    py_cut()         the reference's literal loop (commands/cut.cpp:114-288) with its running frag_start / rc_start and the four
                     ordinal runs; the pieces of the reverse strand are cut out of a whole reverse complement, as the reference does
    py_pattern()     the reference's pattern checks and site arithmetic (commands/cut.cpp:315-384)
    golden_sets()    named input sets, each the smallest that reaches the edges it is named after
    run_cli()        the reference CLI (oracle/refcli.py) on one set: the four FASTA files and the log line
    __main__         writes tests/golden/cut_golden.json: per set the reference's four files (in full where they are short, as SHA-256
                     elsewhere), its log line and a digest of the input; the fatal text of the refused patterns
                     --digest: child-process driver of tests/test_gpu_cut.py
"""
import hashlib
import json
import os
import random
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(HERE, "golden", "cut_golden.json")

WHICH = ("fastaout", "fastaout_rev", "fastaout_discarded", "fastaout_discarded_rev")
DEFAULT_OPTS = dict(sizeout=0, xsize=0, relabel=None, fasta_width=80)
FULL_TEXT_LIMIT = 1500                 # a file of the reference is recorded in full up to this many characters, else as SHA-256
ECORI = "G^AATT_C"

# chrmap_4bit and chrmap_complement of the reference (utils/maps.cpp)
CODE4 = dict(A=1, C=2, G=4, T=8, U=8, M=3, R=5, S=6, V=7, W=9, Y=10, H=11, K=12, D=13, B=14, N=15)
COMPLEMENT = dict(zip("ABCDGHKMNRSTUVWY", "TVGHCDMKNYSAABWR"))
PATTERN_FATALS = {"GAATTC": "No forward sequence cut site (^) found in pattern", "G^AATTC": "No reverse sequence cut site (_) found in pattern",
                  "G^AA^TT_C": "Multiple cut sites not supported", "G^AA_TT_C": "Multiple cut sites not supported",
                  "^_": "Empty cut pattern string", "G^AAXT_C": "Illegal character in cut pattern", "G^AA-T_C": "Illegal character in cut pattern"}


def full_opts(opts):
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    return o


# ---- the plain-Python restatement ---------------------------------------------------------------------------------------------
def code4(c):
    return CODE4.get(c.upper(), 0) if c.isalpha() and c.isascii() else 0


def complement(c):
    if c.isascii() and c.isalpha() and c.upper() in COMPLEMENT:
        u = COMPLEMENT[c.upper()]
        return u.lower() if c.islower() else u
    return "N"


def revcomp(s):
    return "".join(complement(c) for c in reversed(s))


def py_pattern(raw):
    """-> (pattern, cut_fwd, cut_rev), or ValueError with the reference's fatal text"""
    for mark, missing in (("^", "No forward sequence cut site (^) found in pattern"), ("_", "No reverse sequence cut site (_) found in pattern")):
        if raw.count(mark) == 0:
            raise ValueError(missing)
        if raw.count(mark) > 1:
            raise ValueError("Multiple cut sites not supported")
    pattern = raw.replace("^", "").replace("_", "")
    cut_fwd = raw.replace("_", "").find("^")
    cut_rev = raw.replace("^", "").find("_")
    if not pattern:
        raise ValueError("Empty cut pattern string")
    if any(code4(c) == 0 for c in pattern):
        raise ValueError("Illegal character in cut pattern")
    return pattern, cut_fwd, cut_rev


def py_cut(seqs, raw):
    """-> dict(matches, fwd, rev (records (seq, start, length) in forward coordinates), fwd_text, rev_text, uncut, discarded_rev_text,
    cut, uncut_total, total_matches)"""
    pattern, cut_fwd, cut_rev = py_pattern(raw)
    coded = [code4(c) for c in pattern]
    plen = len(pattern)
    res = dict(matches=[], fwd=[], rev=[], fwd_text=[], rev_text=[], uncut=[], discarded_rev_text=[], cut=0, uncut_total=0, total_matches=0)
    for k, seq in enumerate(seqs):
        n = len(seq)
        rc = revcomp(seq)
        codes = [code4(c) for c in seq]
        local = 0
        frag_start, frag_length, rc_start, rc_length = 0, n, n, 0
        for i in range(n - plen + 1):
            if not all(coded[j] & codes[i + j] for j in range(plen)):
                continue
            local += 1
            frag_length = i + cut_fwd - frag_start
            rc_length = rc_start - (n - (i + cut_rev))
            rc_start -= rc_length
            if frag_length > 0:
                res["fwd"].append((k, frag_start, frag_length))
                res["fwd_text"].append(seq[frag_start:frag_start + frag_length])
            if rc_length > 0:
                res["rev"].append((k, n - rc_start - rc_length, rc_length))
                res["rev_text"].append(rc[rc_start:rc_start + rc_length])
            frag_start += frag_length
        if local > 0:
            res["cut"] += 1
            frag_length = n - frag_start
            rc_length = rc_start
            rc_start = 0
            if frag_length > 0:
                res["fwd"].append((k, frag_start, frag_length))
                res["fwd_text"].append(seq[frag_start:frag_start + frag_length])
            if rc_length > 0:
                res["rev"].append((k, n - rc_start - rc_length, rc_length))
                res["rev_text"].append(rc[rc_start:rc_start + rc_length])
        else:
            res["uncut_total"] += 1
            res["uncut"].append(k)
            res["discarded_rev_text"].append(rc)
        res["matches"].append(local)
        res["total_matches"] += local
    return res


def py_match_positions(seq, raw):
    pattern = py_pattern(raw)[0]
    coded = [code4(c) for c in pattern]
    return [i for i in range(len(seq) - len(pattern) + 1) if all(coded[j] & code4(seq[i + j]) for j in range(len(pattern)))]


# ---- builders ------------------------------------------------------------------------------------------------------------------
SITE = "GAATTC"


def _set(name, seqs, pattern=ECORI, opts=None, labels=None):
    return dict(name=name, seqs=list(seqs), labels=labels or [f"s{k}" for k in range(len(seqs))], pattern=pattern, opts=dict(opts or {}))


def background(n, phase=0):
    """n symbols that hold no GAATTC and none of the long patterns' words: a period-5 text over A, C, T"""
    return "".join("ACTCA"[(phase + k) % 5] for k in range(n))


def with_sites(n, at, site=SITE, phase=0):
    s = list(background(n, phase))
    for i in at:
        s[i:i + len(site)] = site
    return "".join(s)[:n]


def long_pattern(p, fwd, rev):
    """p symbols without a period (no overlap with itself), the marks at fwd and rev"""
    rng = random.Random(7000 + p)
    body = "G" + "".join(rng.choice("ACGT") for _ in range(p - 2)) + "G"
    marks = sorted([(fwd, "^"), (rev, "_")], reverse=True)
    for at, m in marks:
        body = body[:at] + m + body[at:]
    return body


def seeded_set(seed, count, lo, hi, alphabet="ACGT", site_rate=0.01, site=SITE):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        n = rng.randint(lo, hi)
        s = [rng.choice(alphabet) for _ in range(n)]
        for _ in range(int(n * site_rate) + (rng.random() < 0.6)):
            i = rng.randrange(0, max(1, n - len(site) + 1))
            s[i:i + len(site)] = site
        out.append("".join(s)[:n])
    return out


IUPAC = "ACGTURYSWKMBDHVN"
ENDS = SITE + "AA" + SITE + "ACT" + SITE                    # matches at 0, in the middle and at L - P
ORDINALS = [ENDS, "ACTACT", "CCCC", SITE + "A", "TTTTTT", "A" + SITE, "ACGT", SITE]


def edge_seqs(tile=4096):
    """GAATTC so that its window straddles a block edge (i = 59 .. 64) and a tile edge (i = tile - 5 .. tile), one sequence per place"""
    out = [with_sites(200, [i], phase=i) for i in range(64 - 6 + 1, 65)]
    out += [with_sites(tile + 300, [i], phase=i) for i in range(tile - 6 + 1, tile + 1)]
    out.append(with_sites(tile + 300, [59, 64, 128 - 3, tile - 3, tile + 64 - 2]))
    return out


def golden_sets():
    sets = [
        _set("lengths", ["GAATT", SITE, SITE + "A", "AATTC", "A" + SITE, "G", "ACGTAC"]),                     # P - 1, P, P + 1
        _set("ends_fwd0_revP", [ENDS, SITE, "A" + SITE + "A"], "^GAATTC_"),
        _set("ends_rev0_fwdP", [ENDS, SITE, "A" + SITE + "A"], "_GAATTC^"),
        _set("rev_below_fwd", [ENDS, "AC" + SITE + "GT"], "G_AATT^C"),
        _set("rev_above_fwd", [ENDS, "AC" + SITE + "GT"], ECORI),
        _set("adjacent_fwd_rev", [ENDS, "AC" + SITE + "GT"], "GAA^_TTC"),
        _set("adjacent_rev_fwd", [ENDS, "AC" + SITE + "GT"], "GAA_^TTC"),
        _set("both_at_start", [ENDS, "AC" + SITE + "GT"], "^_GAATTC"),
        _set("both_at_start_swapped", [ENDS, "AC" + SITE + "GT"], "_^GAATTC"),
        _set("both_at_end", [ENDS, "AC" + SITE + "GT"], "GAATTC^_"),
        _set("both_at_end_swapped", [ENDS, "AC" + SITE + "GT"], "GAATTC_^"),
        _set("overlap_aa", ["AAAA", "AAATAA", "A", "TAAT"], "A^A_"),
        _set("every_position", ["ACGTN", "acgu", "R"], "^N_"),
        _set("alphabet_a", [IUPAC, IUPAC.lower()], "A^_"),
        _set("alphabet_r", [IUPAC, IUPAC.lower()], "^R_"),
        _set("alphabet_y_lower", [IUPAC, IUPAC.lower()], "y_^"),
        _set("alphabet_two", [IUPAC, IUPAC.lower(), "NNNN", "UUuu"], "n^_u"),
        _set("alphabet_b_d", [IUPAC, IUPAC.lower()], "B_^D"),
        _set("neighbours", ["AAAGAA", "TTCAAA", "AA" + SITE, "GAA", "TTC"]),                                   # ...GAA | TTC...: no match
        _set("ordinals", ORDINALS, "^GAA_TTC", dict(relabel="F")),
        _set("edges", edge_seqs()),
        _set("degenerate", seeded_set(2101, 12, 40, 300, "ACGTNacgtRY", site_rate=0.02, site="GCCATTCAGGC"), "GCCNNNN^N_GGC"),
    ]
    for p, fwd, rev in ((63, 1, 62), (64, 64, 0), (65, 30, 31)):
        pat = long_pattern(p, fwd, rev)
        body = pat.replace("^", "").replace("_", "")
        seqs = [background(70 - p % 3) + body + background(40, 2) + body.lower() + "A", body, body[1:], background(130),
                background(64 - p + 1) + body + background(5), body[:-1] + "N" + body]
        sets.append(_set(f"pattern_{p}", seqs, pat))
    mixed = seeded_set(2102, 20, 30, 400, "ACGTacgtNRYU", site_rate=0.015)
    sized = [f"r{k};size={k + 2}" for k in range(len(mixed))]
    sets.append(_set("relabel_sizeout", mixed, ECORI, dict(relabel="M", sizeout=1, fasta_width=0), labels=sized))
    sets.append(_set("xsize_width", mixed, "GG^_CC", dict(xsize=1, fasta_width=33), labels=sized))
    sets.append(_set("sizeout_only", mixed, "R^AATT_Y", dict(sizeout=1), labels=sized))
    return sets


def extra_sets():
    """what the CLI never delivers (its reader strips illegal bytes, and these sets want them): no golden"""
    return [_set("empty", ["", SITE, "", "ACT", ""]),
            _set("code0", ["GAA-TTC", "GAAT*TC" + SITE, "G AATTC", "GAATTC\x00", "~" + SITE + "1"]),
            _set("code0_n", ["AC-GT*AC.GT", "----", "N-N"], "^N_")]


def sizes_of(s):
    out = []
    for lab in s["labels"]:
        m = re.search(r"(?:^|;)size=(\d+)(?:;|$)", lab)
        out.append(int(m.group(1)) if m else 1)
    return out


def writer_kw(s):
    o = full_opts(s["opts"])
    return dict(sizes=sizes_of(s), sizeout=bool(o["sizeout"]), xsize=bool(o["xsize"]), relabel=o["relabel"], fasta_width=o["fasta_width"])


def input_digest(s):
    h = hashlib.sha256()
    for lab, seq in zip(s["labels"], s["seqs"]):
        h.update(lab.encode("latin-1") + b"\0" + seq.encode("latin-1") + b"\n")
    h.update(s["pattern"].encode() + b"\0" + json.dumps(s["opts"], sort_keys=True).encode())
    return h.hexdigest()


# ---- the reference CLI -----------------------------------------------------------------------------------------------------------
def ref_binary():
    from oracle import refcli
    return refcli.REF_BIN


def cli_args(opts):
    o = full_opts(opts)
    a = ["--fasta_width", str(o["fasta_width"]), "--quiet"]                   # (the command takes no --threads: it has one)
    for flag in ("sizeout", "xsize"):
        if o[flag]:
            a.append("--" + flag)
    if o["relabel"] is not None:
        a += ["--relabel", o["relabel"]]
    return a


def run_cli(s):
    """-> dict(fastaout, fastaout_rev, fastaout_discarded, fastaout_discarded_rev: the text of each file; log: the closing line)"""
    from oracle import refcli
    with tempfile.TemporaryDirectory(prefix="vsx_cut_") as tmp:
        p = lambda n: os.path.join(tmp, n)
        refcli.write_fasta(p("in.fa"), s["labels"], [x.encode("latin-1") for x in s["seqs"]])
        args = ["--cut", p("in.fa"), "--cut_pattern", s["pattern"], "--log", p("log.txt")]
        for w in WHICH:
            args += ["--" + w, p(w)]
        refcli.run(args + cli_args(s["opts"]))
        out = {w: open(p(w), encoding="latin-1").read() for w in WHICH}
        out["log"] = [l for l in open(p("log.txt")).read().splitlines() if "sequence(s) cut" in l][0]
        return out


def run_cli_fatal(pattern):
    """the reference's fatal text for a pattern it refuses"""
    with tempfile.TemporaryDirectory(prefix="vsx_cut_") as tmp:
        fa = os.path.join(tmp, "in.fa")
        with open(fa, "w") as f:
            f.write(">a\nACGT\n")
        r = subprocess.run([ref_binary(), "--cut", fa, "--cut_pattern", pattern, "--fastaout", os.path.join(tmp, "o.fa"), "--quiet"],
                           capture_output=True, text=True)
        assert r.returncode != 0, pattern
        lines = [l for l in r.stderr.splitlines() if l.strip()]
        return re.sub(r"^Fatal error: ", "", lines[-1].strip()) if lines else ""


def lib_text(res, s, which):
    """one of the four files as vsearch_amd.cut writes it"""
    from vsearch_amd.cut import fasta_lines
    lines = fasta_lines(res, s["labels"], s["seqs"], which, **writer_kw(s))
    return "".join(l + "\n" for l in lines)


def sha(text):
    return hashlib.sha256(text.encode("latin-1")).hexdigest()


def assert_text_equals_golden(res, s):
    from vsearch_amd.cut import log_lines
    ref = s["ref"]
    for w in WHICH:
        got = lib_text(res, s, w)
        if "text" in ref[w]:
            assert got == ref[w]["text"], (s["name"], w)
        assert sha(got) == ref[w]["sha256"], (s["name"], w)
    assert log_lines(res) == [ref["log"]], s["name"]


def assert_text_equals_cli(res, s, ref):
    from vsearch_amd.cut import log_lines
    for w in WHICH:
        assert lib_text(res, s, w) == ref[w], (s["name"], w)
    assert log_lines(res) == [ref["log"]], s["name"]


def write_golden(path=GOLDEN):
    sets = []
    for s in golden_sets():
        ref = run_cli(s)
        rec = dict(name=s["name"], input_sha256=input_digest(s), log=ref["log"])
        for w in WHICH:
            rec[w] = dict(sha256=sha(ref[w]))
            if len(ref[w]) <= FULL_TEXT_LIMIT:
                rec[w]["text"] = ref[w]
        sets.append(rec)
    fatals = {p: run_cli_fatal(p) for p in PATTERN_FATALS}
    with open(path, "w") as f:
        json.dump(dict(sets=sets, fatals=fatals), f, indent=0, separators=(",", ":"))
        f.write("\n")
    return sets, fatals


def load_golden(path=GOLDEN):
    """the golden sets: the inputs are rebuilt by golden_sets() and checked against the recorded digest"""
    with open(path) as f:
        stored = json.load(f)
    by_name = {r["name"]: r for r in stored["sets"]}
    out = []
    for s in golden_sets():
        ref = by_name[s["name"]]
        assert ref["input_sha256"] == input_digest(s), f"{s['name']}: the input differs from what the golden file was recorded on"
        out.append(dict(s, ref=ref))
    assert len(out) == len(by_name)
    return out


def load_fatals(path=GOLDEN):
    with open(path) as f:
        return json.load(f)["fatals"]


def all_sets():
    return load_golden() + extra_sets()


# ---- calls and comparisons -------------------------------------------------------------------------------------------------------
def call(aligner, s, **extra):
    """the set through vsearch_amd.cut: the device with an aligner, the host restatement without"""
    from vsearch_amd.cut import cut, cut_host
    if aligner is None:
        return cut_host(s["seqs"], s["pattern"], **extra)
    return cut(aligner, s["seqs"], s["pattern"], **extra)


def assert_same(a, b, what):
    """two CutResults field for field, over the fields both have, and the text where both have the same pieces"""
    import numpy as np
    fa, fb = a.fields(), b.fields()
    same_text = (a.rev_off is None) == (b.rev_off is None) and (a.discarded_off is None) == (b.discarded_off is None)
    for k in fa:
        if k in fb and (same_text or not k.endswith("_off")):               # (the offsets of one kind shift with the other kind's text)
            assert np.array_equal(fa[k], fb[k]), (what, k, fa[k][:16], fb[k][:16])
    if same_text:
        assert a.text_blob == b.text_blob, (what, "text")


def assert_equals_py(res, s):
    """a full CutResult against py_cut() on every array and on the text"""
    exp = py_cut(s["seqs"], s["pattern"])
    name = s["name"]
    assert [int(x) for x in res.matches] == exp["matches"], name
    for got, want in ((res.fwd, exp["fwd"]), (res.rev, exp["rev"])):
        assert [(int(a), int(b), int(c)) for a, b, c in zip(*got)] == want, name
    assert [int(x) for x in res.uncut] == exp["uncut"], name
    assert (res.cut, res.uncut_total, res.total_matches) == (exp["cut"], exp["uncut_total"], exp["total_matches"]), name
    assert (res.n_fwd, res.n_rev, res.n_uncut) == (len(exp["fwd"]), len(exp["rev"]), len(exp["uncut"])), name
    assert [res.rev_text(x).decode("latin-1") for x in range(res.n_rev)] == exp["rev_text"], name
    assert [res.discarded_rev_text(x).decode("latin-1") for x in range(res.n_uncut)] == exp["discarded_rev_text"], name
    assert [s["seqs"][k][a:a + l] for k, a, l in exp["fwd"]] == exp["fwd_text"], name
    assert int(res.rev_off[0]) == 0 and int(res.discarded_off[0]) == int(res.rev_off[-1]) and int(res.discarded_off[-1]) == len(res.text_blob), name


HOST_ROUTES = ("host_no_context", "host_environment", "host_count", "host_memory", "host_pattern_length")


def device_digest(aligner, sets=None):
    """SHA-256 over every set's device result; asserts that no call took a host route (but the pattern of 65 symbols, which must)"""
    h = hashlib.sha256()
    for s in sets or all_sets():
        res = call(aligner, s)
        st = res.stats
        long_pattern_set = len(py_pattern(s["pattern"])[0]) > 64
        assert [st[r] for r in HOST_ROUTES] == [0, 0, 0, 0, 1 if long_pattern_set else 0], (s["name"], st)
        h.update(s["name"].encode() + b"\0" + res.tobytes())
    return h.hexdigest()


def _child_digest():
    from vsearch_amd import Aligner, _lib
    with Aligner(device=0) as al:
        print(f"digest {device_digest(al)} poison {_lib.load().vsx_internal_poison_byte()}")


if __name__ == "__main__":
    if "--digest" in sys.argv:
        _child_digest()
    else:
        sets, fatals = write_golden()
        for s, rec in zip(golden_sets(), sets):
            exp = py_cut(s["seqs"], s["pattern"])
            line = "%d sequence(s) cut %d times, %d sequence(s) never cut." % (exp["cut"], exp["total_matches"], exp["uncut_total"])
            print(f"{rec['name']}: {len(s['seqs'])} sequences; {rec['log']}" + ("" if line == rec["log"] else "   PY DIFFERS"))
        for p, text in fatals.items():
            print(f"{p}: {text}" + ("" if text == PATTERN_FATALS[p] else "   EXPECTED " + PATTERN_FATALS[p]))
