"""Input sets and the plain-Python restatement for sequence extraction by label (vsx_getseqs, vsearch_amd.getseqs).

A SET is a dict: name, headers (bytes each), seqs, quals, mode, needles (bytes each; for the list modes what read_labels() gives for
the set's labels file), raw (the labels file's bytes, list modes), substr, field, subseq (start, end) or None, writer options, and
cli: whether the reference CLI can be given the set (it cannot deliver an empty header or an empty sequence).  The sets are built
by code, without random numbers, so tests/golden/getseqs_golden.json stores only what the reference CLI wrote for each of them
(--fastaout, --fastqout, --notmatched, --notmatchedfq, the log line) and a digest of the set's inputs; the two FASTQ files, which
repeat the FASTA files' headers and sequences, in full for the sets about the text (fastq_text) and as SHA-256 for the others.

    python -m tests.getseqs_data            regenerate the golden file with oracle/_ref/vsearch_ref (built by __graft_entry__.build())
    python -m tests.getseqs_data --digest   child of the poisoned-memory test: the digest of every set's device result
"""
import hashlib
import importlib
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(HERE, "golden", "getseqs_golden.json")
MODES = ("label", "labels", "label_word", "label_words")
SINGLE = ("label", "label_word")
WRITER_DEFAULTS = dict(relabel=None, sizeout=False, xsize=False, fasta_width=80, sizein=False)


def B(x):
    return x.encode("latin-1") if isinstance(x, str) else bytes(x)


# ---- the rule, literally -------------------------------------------------------------------------------------------------------------
def fold(c):
    """std::toupper of the C locale on one byte value"""
    return c - 32 if 97 <= c <= 122 else c


def isalnum(c):
    return 48 <= c <= 57 or 65 <= c <= 90 or 97 <= c <= 122


def same_nocase(h, n):
    if len(h) != len(n):
        return False
    for a, b in zip(h, n):
        if fold(a) != fold(b):
            return False
    return True


def contains_nocase(h, n):
    """std::search(h, n) != end(h): an empty needle is found at begin(h), which is end(h) for the empty header"""
    if len(n) == 0:
        return len(h) != 0
    for p in range(0, len(h) - len(n) + 1):
        ok = True
        for j in range(len(n)):
            if fold(h[p + j]) != fold(n[j]):
                ok = False
                break
        if ok:
            return True
    return False


def word_match(h, needle, field):
    """the reference's loop over the occurrences of one needle, restarting one byte behind each"""
    hit = 0
    while True:
        hit = h.find(needle, hit)
        if hit < 0:
            return False
        end = hit + len(needle)
        if field:
            if (hit == 0 or h[hit - 1] == 59) and (end == len(h) or h[end] == 59):
                return True
        elif (hit == 0 or not isalnum(h[hit - 1])) and (end == len(h) or not isalnum(h[end])):
            return True
        hit += 1


def py_match(h, mode, needles, substr, field):
    if mode in ("label", "labels"):
        for n in needles:
            if contains_nocase(h, n) if substr else same_nocase(h, n):
                return True
        return False
    for n in needles:
        if word_match(h, (B(field) + b"=" + n) if field is not None else n, field is not None):
            return True
    return False


def py_getseqs(headers, seqlens, mode, needles, substr=False, field=None, subseq=None):
    """-> dict(records = [(matched, ordinal, start, length)], kept, discarded): the reference's loops, one label after the other"""
    kept = discarded = 0
    rec = []
    for h, n in zip(headers, seqlens):
        if py_match(h, mode, needles, substr, field):
            kept += 1
            start, end = 1, n
            if subseq:
                start, end = max(subseq[0], 1), min(subseq[1], n)
            length, offset = end - start + 1, start - 1
            if length <= 0:
                length, offset = 0, 0
            rec.append((1, kept, offset, length))
        else:
            discarded += 1
            rec.append((0, discarded, 0, n))
    return dict(records=rec, kept=kept, discarded=discarded)


def py_read_labels(raw):
    """fgets(1024) / strlen / one trailing newline dropped / empty pieces skipped -> (labels, warn)"""
    out, at, longest = [], 0, 0
    while at < len(raw):
        piece = bytearray()
        while at < len(raw) and len(piece) < 1023:
            piece.append(raw[at])
            at += 1
            if piece[-1] == 10:
                break
        if 0 in piece:
            piece = piece[:piece.index(0)]
        if piece and piece[-1] == 10:
            piece = piece[:-1]
        if len(piece) == 0:
            continue
        longest = max(longest, len(piece))
        out.append(bytes(piece))
    return out, longest >= 1023


# ---- building blocks -----------------------------------------------------------------------------------------------------------------
def filler(n, phase=0):
    """n bytes of acgt...: no needle of the sets below occurs in it"""
    return (b"acgt" * (n // 4 + 2))[phase % 4:phase % 4 + n] if n > 0 else b""


def reads_for(n, lengths=None):
    """sequences and qualities, every position of a read with another quality symbol"""
    seqs, quals = [], []
    for k in range(n):
        L = lengths[k] if lengths else 5 + k % 7
        seqs.append(("ACGTTGCAGT" * (L // 10 + 2))[k % 3:k % 3 + L])
        quals.append("".join(chr(48 + (k + j) % 26) for j in range(L)))
    return seqs, quals


def _set(name, headers, mode, needles, substr=False, field=None, subseq=None, raw=None, cli=True, seq_lengths=None, **writer):
    headers = [B(h) for h in headers]
    seqs, quals = reads_for(len(headers), seq_lengths)
    if mode in SINGLE:
        needles = [B(needles)]
    else:
        if raw is None:
            raw = b"".join(B(n) + b"\n" for n in needles)
        needles = py_read_labels(raw)[0]
    return dict(name=name, headers=headers, seqs=seqs, quals=quals, mode=mode, needles=needles, raw=raw, substr=substr, field=field,
                subseq=subseq, cli=cli, fastq_text=bool(subseq) or name.startswith(("writers_", "ordinals_")),
                writer=dict(WRITER_DEFAULTS, **writer))


def at(n, pos, needle, fill=filler):
    """an n-byte header of filler with `needle` at byte `pos`"""
    needle = B(needle)
    return fill(pos) + needle + fill(n - pos - len(needle), pos + len(needle))


HEADER_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 1000)
NEEDLE_LENGTHS = (1, 2, 63, 64, 65, 1023)


def wx(n):
    return (b"WXYZ" * (n // 4 + 1))[:n]


def header_length_sets():
    hs = []
    for L in HEADER_LENGTHS:
        hs += [at(L, L - 2, ";w") if L == 1000 else at(L, L - 1, "W")]
        if L < 1000:                                                # (one header of 1 000 bytes: every header is recorded twice)
            hs += [filler(L), at(L, 0, "w")]
        if 2 <= L < 1000:
            hs += [at(L, L - 2, "zq")]
    exact = [hs[0].upper(), hs[8], hs[-1].upper(), filler(1000, 1), filler(64)[:-1] + b"a"]
    return [_set("header_lengths_substr", hs, "labels", [b"W", b"ZQ"], substr=True),
            _set("header_lengths_exact", hs, "labels", exact),
            _set("header_lengths_words", [h.replace(b"c", b";") for h in hs], "label_words", [b"w", b"zq"]),
            _set("empty_header", [b"", b"w", b"", filler(5)], "labels", [b"W"], substr=True, cli=False),
            _set("empty_header_exact_empty_needle", [b"", b"w", b""], "label", b"", cli=False),
            _set("empty_header_empty_substr", [b"", b"w", b"", filler(70)], "label", b"", substr=True, cli=False)]


def needle_length_sets():
    needles = [wx(n) for n in NEEDLE_LENGTHS]
    hs = []
    for nd in needles:
        n = len(nd)
        hs += [filler(7) + b";" + nd + b";" + filler(5), nd, nd[:-1]]
        if n < 1023:                                                # (the long needle in three headers: every header is recorded twice)
            hs += [nd.lower(), nd + b"X", b"_" + nd + b"_"]
    short = hs[:-3]
    return [_set("needle_lengths_substr", hs, "labels", needles, substr=True),
            _set("needle_lengths_exact", hs, "labels", needles),
            _set("needle_lengths_words", short, "label_words", needles),
            _set("needle_1023_single", hs[-3:] + [b"w"], "label", needles[-1], substr=True),
            _set("needle_65_word", hs[24:30], "label_word", needles[4])]


def position_sets():
    nd = b"WXYZW"
    hs = [at(140, p, nd) for p in (0, 62, 63, 64, 135)] + [filler(140), at(140, 62, b"WXYZ;")]
    semi = [at(140, p, b";" + nd + b";") for p in (0, 61, 62, 63, 133)] + [at(140, 135, nd), at(140, 134, b";" + nd), at(140, 0, nd + b";")]
    return [_set("positions_label_substr", hs, "label", nd.lower(), substr=True),
            _set("positions_labels_substr", hs, "labels", [b"nomatch", nd], substr=True),
            _set("positions_word", hs + semi, "label_word", nd),
            _set("positions_words", semi, "label_words", [nd, b"qq"])]


def folding_sets():
    nd = b"ab@[`{Z"
    hs = [b"AB@[`{z", b"ab@[`{Z", b"AB`[`{z", b"AB@{`{z", b"AB@[@{z", b"AB@[`[z", b"CAF\xe9", b"caf\xe9", b"CAF\xc9", b"abc", b"ABC", b"aBc"]
    long = filler(100)
    near = [long, b"t" + long[1:], long[:63] + b"g" + long[64:], long[:-1] + b"a", long.upper()]
    return [_set("folding_label", hs, "label", nd),
            _set("folding_labels", hs + near, "labels", [nd, b"caf\xe9", b"abc", b"ABC", long]),
            _set("folding_substr", [b"x" + h + b"y" for h in hs + near], "labels", [nd, b"caf\xe9", b"abc", b"ABC", long], substr=True),
            _set("folding_words_are_case_sensitive", hs, "label_words", [b"abc", b"CAF\xe9"])]


SIDES = (b"", b"x", b"7", b"_", b";", b"\xff")


def boundary_sets():
    word = [l + b"A1" + r for l in SIDES for r in SIDES]
    more = [b"xA1;A1", b"A1x_A1", b"xA1xA1x", b"xaaa;", b"aaa", b";aa;", b"aa", b"_aaa", b"aa_aa", b"aaa_aa"]
    fh = [l + b"sample=A" + r for l in SIDES for r in SIDES] + [b"xsample=A", b"x;sample=A;y", b"sample=AB;sample=A", b"sample=A;sample=B",
                                                                b"xsample=A;sample=A", b"sample=sample=A", b"ssample=A;"]
    eh = [b"=word", b"a;=word;b", b"k=word", b"=word;", b";=word", b"=words", b"=word=word", b"x=word;=word"]
    return [_set("word_boundaries", word + more, "label_word", b"A1"),
            _set("word_overlap", more, "label_word", b"aa"),
            _set("words_boundaries", word + more, "label_words", [b"zz", b"A1", b"aa"]),
            _set("field_boundaries", fh, "label_word", b"A", field="sample"),
            _set("fields_boundaries", fh, "label_words", [b"B", b"A"], field="sample"),
            _set("empty_field", eh, "label_word", b"word", field=""),
            _set("empty_field_words", eh, "label_words", [b"word"], field="")]


def otu(k):
    return b"OTU_%06d" % k


def list_sets():
    hs = [otu(k) for k in (0, 1, 2, 31, 32, 33, 999, 1000, 99999)] + [b"otu_000001", b"OTU_0000001", b"OTU_00000", b"x;OTU_000999;y", b"nothing"]
    out = []
    for n, kinds in ((0, "esw"), (1, "e"), (2, "es"), (32, "ew"), (33, "ew"), (1000, "esw")):
        if "e" in kinds:
            out.append(_set("list_%d_exact" % n, hs, "labels", [otu(k) for k in range(n)]))
        if "s" in kinds:
            out.append(_set("list_%d_substr" % n, hs, "labels", [otu(k) for k in range(n)], substr=True))
        if "w" in kinds:
            out.append(_set("list_%d_words" % n, hs, "label_words", [otu(k) for k in range(n)]))
    big = [otu(k) for k in range(100000)]
    out.append(_set("list_100000_exact", hs, "labels", big))
    out.append(_set("list_100000_substr", hs, "labels", big, substr=True))
    out.append(_set("list_duplicates", hs, "labels", [otu(1), otu(2), otu(1), otu(1), b"otu_000002", otu(31)] * 3))
    out.append(_set("list_duplicates_words", hs, "label_words", [otu(1), otu(2), otu(1), otu(1), otu(31)] * 3))
    many = [b"Q" + b"w" * (k - 1) for k in range(1, 301)]
    mh = [at(320, 10, many[-1]), at(320, 0, many[149] + b";"), filler(320), at(64, 10, b"q"), at(320, 10, b"w" * 299), filler(64)]
    out.append(_set("lengths_300_substr", mh, "labels", many, substr=True))
    out.append(_set("lengths_300_words", [h.replace(b"c", b";") for h in mh], "label_words", many))
    out.append(_set("lengths_300_exact", mh[2:] + [many[299], many[0].lower(), many[17] + b"w"], "labels", many))
    ph = [b"abcd", b"abc", b"ab", b"abcde", b"xabcd", b"x;abc;abcd", b"ABCD"]
    out.append(_set("prefix_exact", ph, "labels", [b"abc", b"abcd"]))
    out.append(_set("prefix_substr", ph, "labels", [b"abcd", b"abc"], substr=True))
    out.append(_set("prefix_words", ph, "label_words", [b"abc", b"abcd"]))
    out.append(_set("last_label_only", hs, "labels", [b"n%d" % k for k in range(50)] + [b"NOTHING"]))
    return out


def ordinal_sets():
    hs = [b"r%d;sample=%s;size=%d" % (k, b"S1" if k % 2 else b"S2", k % 4 + 1) for k in range(16)]
    return [_set("ordinals_all", hs, "labels", [b"sample="], substr=True),
            _set("ordinals_none", hs, "labels", [b"sample=S3"], substr=True),
            _set("ordinals_alternating", hs, "label_word", b"S1", field="sample"),
            _set("writers_relabel_sizeout", hs, "label_words", [b"S1"], field="sample", relabel="kept", sizeout=True, sizein=True),
            _set("writers_xsize_width", hs, "label_words", [b"S2"], field="sample", xsize=True, fasta_width=3),
            _set("writers_sizeout_width0", hs, "label_word", b"S2", sizeout=True, sizein=True, fasta_width=0)]


def subseq_sets():
    hs = [b"pick;a", b"PICK;b", b"leave", b"pick;c", b"pick;d", b"pick;e", b"other"]
    lens = [10, 3, 10, 4, 1, 25, 12]
    out = [_set("subseq_%d_%d" % se, hs, "label", b"pick", substr=True, subseq=se, seq_lengths=lens)
           for se in ((1, 5), (10, 10), (11, 20), (3, 10), (3, 99), (4, 4), (1, 1), (26, 30))]
    out.append(_set("subseq_exact_label", hs, "label", b"pick;B", subseq=(2, 2), seq_lengths=lens))
    out.append(_set("subseq_empty_sequence", hs, "label", b"pick", substr=True, subseq=(1, 4), seq_lengths=[0, 3, 0, 4, 1, 0, 12], cli=False))
    return out


def empty_needle_sets():
    return [_set("empty_substr_needle", [b"a", filler(64), filler(65), b";"], "label", b"", substr=True)]


def read_labels_sets():
    # (the reference's FASTQ parser drops a carriage return at a line's end, so no header carries one)
    hs = [b"abc", b"abc;r", b"def", b"last", b"xabc"]
    long = hs + [wx(1023), wx(1500)[1023:]]
    return [_set("labels_1500_byte_line", long, "labels", None, raw=wx(1500) + b"\n"),
            _set("labels_1500_byte_line_substr", long + [wx(1500)], "labels", None, raw=wx(1500) + b"\n", substr=True),
            _set("labels_1023_with_newline", long, "labels", None, raw=wx(1023) + b"\nabc\n"),
            _set("labels_1023_without_newline", long, "labels", None, raw=b"def\n" + wx(1023)),
            _set("labels_empty_lines", hs, "labels", None, raw=b"\n\nabc\n\n\ndef\n\n"),
            _set("labels_last_line_unterminated", hs, "label_words", None, raw=b"abc\nlast"),
            _set("labels_crlf", hs, "labels", None, raw=b"abc\r\ndef\r\n")]


def all_sets():
    out = (header_length_sets() + needle_length_sets() + position_sets() + folding_sets() + boundary_sets() + list_sets() + ordinal_sets() +
           subseq_sets() + empty_needle_sets() + read_labels_sets())
    assert len({s["name"] for s in out}) == len(out)
    return out


_SETS = None


def sets():
    global _SETS
    if _SETS is None:
        _SETS = all_sets()
    return _SETS


def by_name(name):
    return next(s for s in sets() if s["name"] == name)


def digest_of_inputs(s):
    h = hashlib.sha256()
    for part in (s["headers"], [B(x) for x in s["seqs"]], [B(x) for x in s["quals"]], s["needles"]):
        for x in part:
            h.update(b"%d:" % len(x) + x)
        h.update(b"|")
    h.update(repr((s["mode"], s["substr"], s["field"], s["subseq"], sorted(s["writer"].items()))).encode())
    return h.hexdigest()


_EXPECTED = {}


def expected(s):
    """py_getseqs() of a set, computed once"""
    if s["name"] not in _EXPECTED:
        _EXPECTED[s["name"]] = py_getseqs(s["headers"], [len(x) for x in s["seqs"]], s["mode"], s["needles"], s["substr"], s["field"], s["subseq"])
    return _EXPECTED[s["name"]]


# ---- seeded random draws ---------------------------------------------------------------------------------------------------------------
ALPHABET = (b"a", b"c", b"G", b"t", b";", b"=", b"_", b"\xe9")


def random_draw(rng):
    """(headers, seqlens, mode, needles, substr, field, subseq): short strings over a small alphabet, so that occurrences, overlaps
    and boundaries are frequent"""
    word = lambda lo, hi: b"".join(rng.choice(ALPHABET) for _ in range(rng.randint(lo, hi)))  # noqa: E731
    mode = rng.choice(MODES)
    nn = 1 if mode in SINGLE else rng.choice((0, 1, 2, 3, 5, 9))
    needles = [word(1, 4) for _ in range(nn)]
    field = rng.choice((None, None, "", "a", "a=", "ct")) if mode.startswith("label_word") else None
    substr = rng.random() < 0.5
    if mode == "label" and rng.random() < 0.1:
        needles = [b""]
    headers = []
    for _ in range(rng.randint(0, 6)):
        h = word(0, 12)
        if needles and rng.random() < 0.6:
            nd = rng.choice(needles)
            nd = (B(field) + b"=" + nd) if field is not None and rng.random() < 0.8 else nd
            p = rng.randint(0, len(h))
            h = h[:p] + nd + h[p:] if rng.random() < 0.7 else nd
            if rng.random() < 0.3:
                h = h.swapcase() if rng.random() < 0.5 else h + nd
        headers.append(h)
    seqlens = [rng.randint(0, 9) for _ in headers]
    subseq = None
    if rng.random() < 0.3:
        a = rng.randint(1, 10)
        subseq = (a, rng.randint(a, 12))
    return headers, seqlens, mode, needles, substr, field, subseq


# ---- calls ----------------------------------------------------------------------------------------------------------------------------
def call_kw(s):
    kw = dict(substr=s["substr"], field=s["field"])
    if s["subseq"]:
        kw.update(subseq_start=s["subseq"][0], subseq_end=s["subseq"][1])
    return kw


def needles_arg(s):
    return s["needles"][0] if s["mode"] in SINGLE else s["needles"]


def call(aligner, s, headers=None, **extra):
    """the set through vsearch_amd.getseqs: the device with an aligner, the host restatement without"""
    gs = importlib.import_module("vsearch_amd.getseqs")
    return gs.getseqs(aligner, s["headers"] if headers is None else headers, s["seqs"], s["mode"], needles_arg(s), **dict(call_kw(s), **extra))


def assert_equals_py(res, s):
    exp = expected(s)
    assert [res.record(k) for k in range(res.n)] == exp["records"], s["name"]
    assert (res.kept, res.discarded) == (exp["kept"], exp["discarded"]), s["name"]


def sizes_of(s):
    """the abundance --sizeout prints: the header's ;size= annotation, WITH OR WITHOUT --sizein (fastx_get_abundance reads the header
    itself; found by oracle/soak_commands.py --command getseqs), 1 where there is none"""
    import re
    out = []
    for h in s["headers"]:
        m = re.search(rb"(?:^|;)size=(\d+)(?:;|$)", h)
        out.append(int(m.group(1)) if m else 1)
    return out


def texts(res, s):
    """the four files and the log line as the writers of vsearch_amd.getseqs give them"""
    gs = importlib.import_module("vsearch_amd.getseqs")
    w = s["writer"]
    kw = dict(sizes=sizes_of(s), sizeout=w["sizeout"], xsize=w["xsize"], relabel=w["relabel"], fasta_width=w["fasta_width"])
    fastq = s["quals"] is not None                                       # (a FASTA input has no FASTQ files: None)
    return dict(fastaout=gs.fasta_lines(res, s["headers"], s["seqs"], True, **kw), notmatched=gs.fasta_lines(res, s["headers"], s["seqs"], False, **kw),
                fastqout=gs.fastq_lines(res, s["headers"], s["seqs"], s["quals"], True, **kw) if fastq else None,
                notmatchedfq=gs.fastq_lines(res, s["headers"], s["seqs"], s["quals"], False, **kw) if fastq else None, log=gs.log_lines(res))


def device_digest(aligner):
    """SHA-256 over every set's device result; asserts that no call took a host route"""
    h = hashlib.sha256()
    for s in sets():
        res = call(aligner, s)
        st = res.stats
        assert st["headers_host"] == 0 and st["headers_device"] == len(s["headers"]), (s["name"], st)
        h.update(s["name"].encode() + b"\0" + repr(res.arrays()).encode())
    return h.hexdigest()


# ---- the reference CLI ------------------------------------------------------------------------------------------------------------------
def ref_binary():
    return os.path.join(ROOT, "oracle", "_ref", "vsearch_ref")


FILES = ("fastaout", "fastqout", "notmatched", "notmatchedfq")


def run_cli(headers, seqs, quals, mode, needles, raw, substr, field, subseq, writer, command=None):
    """the reference CLI on a FASTQ file of the reads -> dict(fastaout, fastqout, notmatched, notmatchedfq: bytes; log: the line).
    quals=None: a FASTA file, and only the two FASTA outputs (the two FASTQ files are None)"""
    with tempfile.TemporaryDirectory(prefix="vsx_getseqs_") as tmp:
        p = lambda n: os.path.join(tmp, n)  # noqa: E731
        fastq = quals is not None
        source = p("in.fq" if fastq else "in.fa")
        with open(source, "wb") as f:
            if fastq:
                for h, sq, q in zip(headers, seqs, quals):
                    f.write(b"@" + h + b"\n" + B(sq) + b"\n+\n" + B(q) + b"\n")
            else:
                for h, sq in zip(headers, seqs):
                    f.write(b">" + h + b"\n" + B(sq) + b"\n")
        files = FILES if fastq else ("fastaout", "notmatched")
        if command is None:
            command = "fastx_getsubseq" if subseq else "fastx_getseqs"
        args = [ref_binary(), "--" + command, source, "--log", p("log.txt"), "--quiet"]
        for n in files:
            args += ["--" + n, p(n)]
        if mode in SINGLE:
            args += ["--" + mode, needles[0]]
        else:
            with open(p("labels.txt"), "wb") as f:
                f.write(raw if raw is not None else b"".join(n + b"\n" for n in needles))
            args += ["--" + mode, p("labels.txt")]
        if substr:
            args.append("--label_substr_match")
        if field is not None:
            args += ["--label_field", field]
        if subseq:
            args += ["--subseq_start", str(subseq[0]), "--subseq_end", str(subseq[1])]
        for flag in ("sizeout", "xsize", "sizein"):
            if writer[flag]:
                args.append("--" + flag)
        if writer["relabel"] is not None:
            args += ["--relabel", writer["relabel"]]
        if writer["fasta_width"] != 80:
            args += ["--fasta_width", str(writer["fasta_width"])]
        r = subprocess.run(args, capture_output=True)
        if r.returncode != 0:
            raise RuntimeError("reference CLI failed: " + r.stderr.decode("latin-1")[-2000:])
        out = {n: open(p(n), "rb").read() if n in files else None for n in FILES}
        out["log"] = [l for l in open(p("log.txt"), encoding="latin-1").read().splitlines() if "sequences extracted" in l]
        out["warned"] = "Labels longer than 1023" in open(p("log.txt"), encoding="latin-1").read()
        return out


def run_reference(s):
    return run_cli(s["headers"], s["seqs"], s["quals"], s["mode"], s["needles"], s["raw"], s["substr"], s["field"], s["subseq"], s["writer"])


def as_lines(data):
    """a file of the CLI as the writers' list of lines"""
    return data.decode("latin-1").split("\n")[:-1]


def recorded(s, name, data):
    """a file as the golden keeps it: its text; the FASTQ files, which repeat the FASTA files' headers and sequences, in full only for
    the sets about the text (subsequences, writers, ordinals: fastq_text) and as SHA-256 for the others"""
    if name in ("fastqout", "notmatchedfq") and not s["fastq_text"]:
        return "sha256:" + hashlib.sha256(data).hexdigest()
    return data.decode("latin-1")


def write_golden(path=GOLDEN):
    """generated with oracle/_ref/vsearch_ref (the reference's sources, built by __graft_entry__.build()): python -m tests.getseqs_data"""
    rec = {}
    for s in sets():
        if not s["cli"]:
            continue
        ref = run_reference(s)
        rec[s["name"]] = dict(inputs=digest_of_inputs(s), log=ref["log"], warned=ref["warned"], **{n: recorded(s, n, ref[n]) for n in FILES})
    head = ("what oracle/_ref/vsearch_ref (the reference CLI, built from its own sources by __graft_entry__.build()) wrote for every set of "
            "tests/getseqs_data.py that it can be given; regenerate with: python -m tests.getseqs_data")
    with open(path, "w") as f:
        json.dump(dict(header=head, sets=rec), f, indent=0, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    return rec


_GOLDEN = None


def load_golden(path=GOLDEN):
    global _GOLDEN
    if _GOLDEN is None:
        with open(path) as f:
            _GOLDEN = json.load(f)["sets"]
    return _GOLDEN


def assert_text_equals_golden(res, s):
    ref = load_golden()[s["name"]]
    assert ref["inputs"] == digest_of_inputs(s), (s["name"], "the golden file was recorded for other inputs")
    got = texts(res, s)
    for n in FILES:
        assert recorded(s, n, "".join(l + "\n" for l in got[n]).encode("latin-1")) == ref[n], (s["name"], n)
    assert got["log"] == ref["log"], s["name"]


def _child_digest():
    from vsearch_amd import Aligner, _lib
    with Aligner(device=0) as al:
        print(f"digest {device_digest(al)} poison {_lib.load().vsx_internal_poison_byte()}")


if __name__ == "__main__":
    if "--digest" in sys.argv:
        _child_digest()
    else:
        rec = write_golden()
        for s in sets():
            if s["cli"]:
                exp = expected(s)
                ok = rec[s["name"]]["log"][0].startswith("%d of %d " % (exp["kept"], exp["kept"] + exp["discarded"]))
                print(f"{s['name']}: {rec[s['name']]['log'][0]}" + ("" if ok else "   PY DIFFERS"))
