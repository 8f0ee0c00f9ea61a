"""Inputs, a plain-Python restatement and the reference-CLI runner for the sorting tests (--sortbysize, --sortbylength).

    py_sortby()      the reference's three comparators, literally (commands/sortbysize.cpp:110-123, commands/sortbylength.cpp:108-128,
                     core/db.cpp:452-469), through functools.cmp_to_key over bytes under sorted(), which is stable; create_deck's
                     selection, the median of find_median_abundance / find_median_length, truncate_deck
    golden_sets()    named input sets, each the smallest that reaches the edge it is named after
    extra_sets()     what the CLI's reader would alter or the CLI has no command for: checked against py_sortby() only
    run_cli()        the reference CLI (oracle/refcli.py) on one set: the --output text and the median line of --log
    __main__         writes tests/golden/sortby_golden.json: per set the reference's --output (in full where it is short, as SHA-256
                     elsewhere), its median line and a digest of the input
                     --digest: child-process driver of tests/test_gpu_sortby.py
"""
import functools
import hashlib
import json
import os
import random
import re
import struct
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(HERE, "golden", "sortby_golden.json")

INT64_MAX = (1 << 63) - 1
DEFAULT_OPTS = dict(minsize=0, maxsize=INT64_MAX, topn=INT64_MAX, sizeout=0, xsize=0, relabel=None, fasta_width=80)
FULL_TEXT_LIMIT = 1200                 # the reference's file is recorded in full up to this many characters, else as SHA-256
HOST_ROUTES = ("host_no_context", "host_environment", "host_count", "host_memory", "host_long_prefix")
SEQ = "ACGT" * 25                      # 100 symbols: two lines at --fasta_width 80


def full_opts(opts):
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    return o


def raw(label):
    return label.encode("latin-1") if isinstance(label, str) else bytes(label)


# ---- the plain-Python restatement ---------------------------------------------------------------------------------------------
def strcmp(a, b):
    """strcmp of two headers without a NUL: bytes compare unsigned, a proper prefix first"""
    return (a > b) - (a < b)


def comparator(order, labels, lengths, sizes):
    def by_size(x, y):
        if sizes[x] < sizes[y]:
            return 1
        if sizes[x] > sizes[y]:
            return -1
        return strcmp(labels[x], labels[y])

    def by_length(x, y):
        if lengths[x] < lengths[y]:
            return 1
        if lengths[x] > lengths[y]:
            return -1
        return by_size(x, y)

    def by_length_shortest(x, y):
        if lengths[x] != lengths[y]:
            return -1 if lengths[x] < lengths[y] else 1
        return by_size(x, y)
    return dict(size=by_size, length=by_length, length_asc=by_length_shortest)[order]


def py_sortby(labels, lengths, sizes, order, minsize=0, maxsize=INT64_MAX, topn=INT64_MAX):
    """-> dict(order, n_kept, n_out, median)"""
    labels = [raw(l) for l in labels]
    deck = [i for i in range(len(labels)) if order != "size" or minsize <= sizes[i] <= maxsize]
    deck = sorted(deck, key=functools.cmp_to_key(comparator(order, labels, lengths, sizes)))
    key = sizes if order == "size" else lengths
    median = 0.0
    if deck:
        mid = len(deck) // 2
        if len(deck) % 2:
            median = key[deck[mid]] * 1.0
        else:
            a, b = key[deck[mid - 1]], key[deck[mid]]
            median = min(a, b) + (max(a, b) - min(a, b)) * 0.5
    return dict(order=deck[:topn], n_kept=len(deck), n_out=min(len(deck), topn), median=median)


def result_bytes(n, n_kept, n_out, median, order):
    """what SortbyResult.tobytes() gives"""
    return struct.pack("<QQQd", n, n_kept, n_out, median) + b"".join(struct.pack("<Q", int(k)) for k in order)


def expected(s):
    o = full_opts(s["opts"])
    return py_sortby(s["labels"], s["lengths"], s["sizes"], s["order"], o["minsize"], o["maxsize"], o["topn"])


def expected_bytes(s):
    e = expected(s)
    return result_bytes(len(s["labels"]), e["n_kept"], e["n_out"], e["median"], e["order"])


# ---- builders ------------------------------------------------------------------------------------------------------------------
def header_size(label):
    m = re.search(rb"(?:^|;)size=(\d+)(?:;|$)", raw(label))
    return int(m.group(1)) if m else 1


def lab(name, size):
    return name if size == 1 else f"{name};size={size}"


def _set(name, labels, order="size", opts=None, seqs=None, sizes=None):
    """labels carry their abundance as ;size= (what the CLI reads); sizes overrides that for the sets the CLI never sees"""
    seqs = list(seqs) if seqs is not None else [SEQ] * len(labels)
    return dict(name=name, labels=list(labels), seqs=seqs, lengths=[len(x) for x in seqs],
                sizes=list(sizes) if sizes is not None else [header_size(l) for l in labels], order=order, opts=dict(opts or {}))


def shuffled_labels(seed, n, size_choices=(1, 1, 1, 2, 3), stem="r"):
    rng = random.Random(seed)
    names = [f"{stem}{rng.randrange(10 ** 6):06d}" for _ in range(n)]
    return [lab(x, rng.choice(size_choices)) for x in names]


ALPHA = "abcdefgh" * 40
LABEL_LENGTHS = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65)
FIRST_DIFFS = (7, 8, 9, 15, 16, 63, 64, 65)
PREFIX300 = ("M01234:56:000000000-ABCDE:1:1101:" * 10)[:300]


def first_diff_labels():
    base = "p" * 70
    out = []
    for d in reversed(FIRST_DIFFS):
        out += [base[:d] + "B" + base[d + 1:], base[:d] + "A" + base[d + 1:]]          # the larger first: the sort has to swap them
    return out


def deep_beside_flat():
    """64 equal labels (final after the first label round) beside five that share 66 bytes (nine rounds)"""
    deep = [lab("q" * 66 + c, 2) for c in "edcba"]
    return ["same"] * 40 + deep[:2] + ["same"] * 24 + deep[2:]


def illumina(rng, n, singletons=0.6, long_prefix=False):
    """Illumina-like headers with ;size=; a share of singletons, the rest 2 .. 50"""
    out = []
    for _ in range(n):
        head = f"M0{rng.randrange(3)}234:56:000000000-ABCDE:1:{rng.choice((1101, 1102, 2101))}:{rng.randrange(1000, 30000)}:{rng.randrange(1000, 30000)}"
        if long_prefix and rng.random() < 0.3:
            head = PREFIX300[:rng.choice((40, 130, 270))] + head
        out.append(lab(head, 1 if rng.random() < singletons else rng.randrange(2, 51)))
    return out


def golden_sets():
    sets = [_set(f"n_{n}", shuffled_labels(3100 + n, n)) for n in (1, 2, 63, 64, 65, 255, 256, 257)]
    sets += [
        _set("label_lengths", [ALPHA[:n] for n in reversed(LABEL_LENGTHS)]),                         # every one a proper prefix of the next longer
        _set("blob_edge", ["first", "zzzzzzzzzzzzzzzzzzzzb", "mid", "zzzzzzzzzzzzzzzzzzzza"]),          # a deep tie that ends on the blob's last byte
        _set("first_diff", first_diff_labels()),
        _set("prefix_labels", ["k" * 9, "k" * 8, "k" * 7, "k" * 17, "k" * 16, "k" * 15, "k" * 65, "k" * 64, "k" * 63]),
        _set("equal_labels", ["m", "k", "same", "a", "same", "z", "same", "b"], seqs=["ACGT" * k for k in range(1, 9)]),
        _set("one_tie_group", [lab(x, 5) for x in shuffled_labels(3201, 40, (1,))]),
        _set("deep_beside_flat", deep_beside_flat()),
        _set("many_groups", [lab(f"g{(k * 7919) % 600:03d}", 2 + (k * 131) % 300) for k in range(600)]),
        _set("length_vs_abundance", [lab("a", 1), lab("b", 3), lab("c", 3), lab("d", 2), lab("e", 1), lab("f", 3), lab("g", 2), lab("h", 1)],
             "length", seqs=["A" * n for n in (7, 7, 9, 9, 7, 5, 9, 5)]),
        _set("large_abundances", [lab("a", 1), lab("b", 2 ** 31), lab("c", 2 ** 32 - 1), lab("d", 2 ** 31), lab("e", 2 ** 32 - 1), lab("f", 1)]),
        _set("long_prefix", [PREFIX300 + f"{(k * 37) % 64:02d}" + ("x" * (k % 3)) for k in range(64)]),
        _set("median_odd", [lab(f"s{k}", v) for k, v in enumerate((9, 1, 4, 2, 7))]),
        _set("median_2_5", [lab(f"s{k}", v) for k, v in enumerate((2, 3, 9, 1))]),                    # prints 2: a half rounds to even
        _set("median_3_5", [lab(f"s{k}", v) for k, v in enumerate((3, 4, 9, 1))]),                    # prints 4
        _set("median_before_topn", [lab(f"s{k}", v) for k, v in enumerate((3, 4, 9, 1))], opts=dict(topn=1)),
        _set("median_length_2_5", ["a", "b", "c", "d"], "length", seqs=["A" * n for n in (3, 9, 1, 2)]),
    ]
    sized = [lab(f"t{k}", v) for k, v in enumerate((1, 2, 3, 3, 4, 5, 7, 3, 2))]
    for lo, hi in ((3, 3), (2, 4), (4, 2), (100, INT64_MAX), (3, INT64_MAX), (0, 3)):
        sets.append(_set(f"minmax_{lo}_{'max' if hi == INT64_MAX else hi}", sized, opts=dict(minsize=lo, maxsize=hi)))
    for topn in (1, 6, 7, 8):                                                                         # n_kept = 7 under minsize 2 .. maxsize 5
        sets.append(_set(f"topn_{topn}", sized, opts=dict(minsize=2, maxsize=5, topn=topn)))
    sets.append(_set("topn_length", sized, "length", opts=dict(topn=3), seqs=["ACG" * (1 + k % 4) for k in range(len(sized))]))
    mixed = shuffled_labels(3301, 30, (1, 1, 2, 5, 5, 11))
    seqs = ["ACGTTGCA" * (3 + (k * 5) % 17) for k in range(len(mixed))]
    sets += [
        _set("sizeout_width0", mixed, opts=dict(sizeout=1, fasta_width=0), seqs=seqs),
        _set("xsize", mixed, opts=dict(xsize=1), seqs=seqs),
        _set("relabel_sizeout", mixed, opts=dict(relabel="R", sizeout=1), seqs=seqs),
        _set("length_sizeout_width0", mixed, "length", opts=dict(sizeout=1, fasta_width=0), seqs=seqs),
        _set("length_xsize_relabel", mixed, "length", opts=dict(xsize=1, relabel="L"), seqs=seqs),
        _set("illumina", illumina(random.Random(3302), 120, long_prefix=True), opts=dict(sizeout=1)),
    ]
    return sets


def extra_sets():
    """no golden: bytes the CLI's reader would alter, an empty header, an empty input, the order no command prints, topn 0, and
    sortbylength with the size bounds it ignores"""
    sized = [lab(f"t{k}", v) for k, v in enumerate((1, 2, 3, 3, 4, 5, 7, 3, 2))]
    lens = ["A" * n for n in (7, 7, 9, 9, 7, 5, 9, 5, 6)]
    return [
        _set("n_0", []),
        _set("label_empty", ["b", "", "a", "", "ab"]),
        _set("bytes_7f_80", [b"ab\x80", b"ab\x7f", b"ab\xff", b"ab\x01", b"ab"]),                     # strcmp is unsigned
        _set("bytes_at_chunk_edge", [b"abcdefg\x80", b"abcdefg\x7f", b"abcdefgh\xff", b"abcdefgh\x01", b"abcdefg\xff" + b"a"]),
        _set("control_bytes", [b"x\x1fy", b"x\ty", b"x y", b"x\x7fy", b"x\x01y"]),
        _set("length_asc", sized, "length_asc", seqs=lens),
        _set("length_asc_median", ["a", "b", "c", "d"], "length_asc", seqs=["A" * n for n in (3, 9, 1, 2)]),
        _set("length_ignores_minmax", sized, "length", opts=dict(minsize=3, maxsize=3), seqs=lens),
        _set("length_asc_ignores_minmax", sized, "length_asc", opts=dict(minsize=100), seqs=lens),
        _set("topn_0", sized, opts=dict(topn=0)),
        _set("minmax_0_0", sized, opts=dict(minsize=0, maxsize=0)),                                      # (the CLI wants maxsize >= 1)
        _set("explicit_sizes", ["a", "b", "c", "d"], sizes=[1, 2 ** 31, 2 ** 32 - 1, 2]),
    ]


def seeded_case(rng, n, alphabet="ab", max_len=20, max_size=3, max_seqlen=4):
    """dense ties and prefixes: a two-letter alphabet, labels of 0 .. max_len bytes (short ones more often), few sizes and lengths"""
    labels = ["".join(rng.choice(alphabet) for _ in range(min(rng.randint(0, max_len), rng.randint(0, max_len), rng.randint(0, max_len)))) for _ in range(n)]
    sizes = [rng.randint(1, max_size) for _ in range(n)]
    seqs = ["A" * rng.randint(1, max_seqlen) for _ in range(n)]
    opts = {}
    if rng.random() < 0.3:
        opts["minsize"] = rng.randint(0, max_size)
    if rng.random() < 0.3:
        opts["maxsize"] = rng.randint(1, max_size + 1)
    if rng.random() < 0.3:
        opts["topn"] = rng.randint(0, n + 1)
    return _set("seeded", labels, rng.choice(("size", "length", "length_asc")), opts, seqs, sizes)


def input_digest(s):
    h = hashlib.sha256()
    for l, seq in zip(s["labels"], s["seqs"]):
        h.update(raw(l) + b"\0" + seq.encode("latin-1") + b"\n")
    h.update(s["order"].encode() + b"\0" + json.dumps(s["opts"], sort_keys=True).encode())
    return h.hexdigest()


# ---- the reference CLI -----------------------------------------------------------------------------------------------------------
def ref_binary():
    from oracle import refcli
    return refcli.REF_BIN


def cli_args(s):
    o = full_opts(s["opts"])
    a = ["--notrunclabels", "--fasta_width", str(o["fasta_width"]), "--quiet"]
    if s["order"] == "size":
        if o["minsize"] != 0:
            a += ["--minsize", str(o["minsize"])]
        if o["maxsize"] != INT64_MAX:
            a += ["--maxsize", str(o["maxsize"])]
    if o["topn"] != INT64_MAX:
        a += ["--topn", str(o["topn"])]
    for flag in ("sizeout", "xsize"):
        if o[flag]:
            a.append("--" + flag)
    if o["relabel"] is not None:
        a += ["--relabel", o["relabel"]]
    return a


def run_cli(s):
    """-> dict(output: the text of --output, log: the median line)"""
    from oracle import refcli
    assert s["order"] in ("size", "length")
    with tempfile.TemporaryDirectory(prefix="vsx_sortby_") as tmp:
        p = lambda n: os.path.join(tmp, n)  # noqa: E731
        with open(p("in.fa"), "wb") as f:
            for l, seq in zip(s["labels"], s["seqs"]):
                f.write(b">" + raw(l) + b"\n" + seq.encode("latin-1") + b"\n")
        refcli.run(["--sortbysize" if s["order"] == "size" else "--sortbylength", p("in.fa"), "--output", p("out.fa"), "--log", p("log.txt")]
                   + cli_args(s))
        return dict(output=open(p("out.fa"), encoding="latin-1").read(),
                    log=[l for l in open(p("log.txt")).read().splitlines() if l.startswith("Median ")][0])


def writer_kw(s):
    o = full_opts(s["opts"])
    return dict(sizes=s["sizes"], sizeout=bool(o["sizeout"]), xsize=bool(o["xsize"]), relabel=o["relabel"], fasta_width=o["fasta_width"])


def lib_text(res, s):
    """--output as vsearch_amd.sortby writes it"""
    from vsearch_amd.sortby import fasta_lines
    return "".join(l + "\n" for l in fasta_lines(res, s["labels"], s["seqs"], **writer_kw(s)))


def sha(text):
    return hashlib.sha256(text.encode("latin-1")).hexdigest()


def assert_text_equals_golden(res, s):
    from vsearch_amd.sortby import log_lines
    ref = s["ref"]
    got = lib_text(res, s)
    if "text" in ref["output"]:
        assert got == ref["output"]["text"], s["name"]
    assert sha(got) == ref["output"]["sha256"], s["name"]
    assert log_lines(res) == [ref["log"]], s["name"]


def assert_text_equals_cli(res, s, ref):
    from vsearch_amd.sortby import log_lines
    assert lib_text(res, s) == ref["output"], s["name"]
    assert log_lines(res) == [ref["log"]], s["name"]


def write_golden(path=GOLDEN):
    sets = []
    for s in golden_sets():
        ref = run_cli(s)
        rec = dict(name=s["name"], input_sha256=input_digest(s), log=ref["log"], output=dict(sha256=sha(ref["output"])))
        if len(ref["output"]) <= FULL_TEXT_LIMIT:
            rec["output"]["text"] = ref["output"]
        sets.append(rec)
    with open(path, "w") as f:
        json.dump(dict(sets=sets), f, indent=0, separators=(",", ":"))
        f.write("\n")
    return sets


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


def all_sets():
    return load_golden() + extra_sets()


# ---- calls and comparisons -------------------------------------------------------------------------------------------------------
def call(aligner, s, labels=None, **extra):
    """the set through vsearch_amd.sortby: the device with an aligner, the host restatement without"""
    from vsearch_amd.sortby import sortby, sortby_host
    o = full_opts(s["opts"])
    kw = dict(minsize=o["minsize"], maxsize=o["maxsize"], topn=o["topn"])
    kw.update(extra)
    labels = s["labels"] if labels is None else labels
    if aligner is None:
        return sortby_host(labels, s["lengths"], s["sizes"], s["order"], **kw)
    return sortby(aligner, labels, s["lengths"], s["sizes"], s["order"], **kw)


def assert_equals_py(res, s):
    e = expected(s)
    assert [int(k) for k in res.order] == e["order"], s["name"]
    assert (res.n, res.n_kept, res.n_out) == (len(s["labels"]), e["n_kept"], e["n_out"]), s["name"]
    assert struct.pack("<d", res.median) == struct.pack("<d", e["median"]), (s["name"], res.median, e["median"])
    assert res.tobytes() == expected_bytes(s), s["name"]


def routes(res):
    return [res.stats[r] for r in HOST_ROUTES]


def device_digest(aligner, sets=None):
    """SHA-256 over every set's device result; asserts that no call left the device but for groups at the round cap"""
    h = hashlib.sha256()
    for s in sets or all_sets():
        res = call(aligner, s)
        assert routes(res)[:4] == [0, 0, 0, 0], (s["name"], res.stats)
        h.update(s["name"].encode() + b"\0" + res.tobytes())
    return h.hexdigest()


def py_digest(sets=None):
    h = hashlib.sha256()
    for s in sets or all_sets():
        h.update(s["name"].encode() + b"\0" + expected_bytes(s))
    return h.hexdigest()


def _child_digest():
    """the digest under the default round cap and under a cap of one round"""
    from vsearch_amd import Aligner, _lib
    with Aligner(device=0) as al:
        for cap in (None, "1"):
            if cap is None:
                os.environ.pop("VSX_SORTBY_MAX_ROUNDS", None)
            else:
                os.environ["VSX_SORTBY_MAX_ROUNDS"] = cap
            print(f"digest {device_digest(al)} cap {cap} poison {_lib.load().vsx_internal_poison_byte()}")


if __name__ == "__main__":
    if "--digest" in sys.argv:
        _child_digest()
    else:
        for s, rec in zip(golden_sets(), write_golden()):
            e = expected(s)
            what = "abundance" if s["order"] == "size" else "length"
            line = "Median %s: %.0f" % (what, e["median"])
            heads = [l[1:] for l in run_cli(dict(s, opts=dict(s["opts"], sizeout=0, xsize=0, relabel=None)))["output"].splitlines() if l.startswith(">")]
            same = heads == [raw(s["labels"][k]).decode("latin-1") for k in e["order"]]
            print(f"{rec['name']}: {len(s['labels'])} records; {rec['log']}" + ("" if line == rec["log"] else "   PY MEDIAN DIFFERS")
                  + ("" if same else "   PY ORDER DIFFERS"))
