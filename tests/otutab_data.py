"""Inputs and oracles of the OTU-table tests (tests/test_otutab_host.py, tests/test_gpu_otutab.py).

    *_set()           input builders, each the smallest input that reaches the edge it is named after
    py_otutab()       a plain-Python restatement: the reference's three patterns literally, with `re` on bytes and sorted() on bytes
    run_reference()   the three files of the reference CLI (oracle/_ref/vsearch_ref) for a set
    __main__          writes tests/golden/otutab_golden.json: the sets' inputs and the reference's recorded three texts

A search set names its hits through sequences: target j has a sequence of its own unless `same[j] = i` gives it target i's, a query
has the sequence of the target it hits or one no target has.  The hits of a query are then all the targets with its sequence, in
database order, and --search_exact (or --usearch_global, for the recorded runs) finds exactly those.  A clustering set lists its
sequences in processing order with the cluster each one joins.
"""
import importlib
import json
import os
import random
import re
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "otutab_golden.json")
NONE = 0xFFFFFFFF
KEYWORDS = (b"sample=", b"barcodelabel=", b"otu=", b"tax=")

RE_SAMPLE = re.compile(rb"(^|;)(sample|barcodelabel)=([^;]*)($|;)")
RE_OTU = re.compile(rb"(^|;)otu=([^;]*)($|;)")
RE_TAX = re.compile(rb"(^|;)tax=([^;]*)($|;)")
RE_WORD = re.compile(rb"[A-Za-z0-9_]*")
RE_SIZE = re.compile(rb"(^|;)size=([0-9]+)(;|$)")


def B(x):
    return x.encode("latin-1") if isinstance(x, str) else bytes(x)


# ---- the plain-Python restatement -----------------------------------------------------------------------------------------------
def py_sample(label):
    m = RE_SAMPLE.search(label)
    return m.group(3) if m else RE_WORD.match(label).group(0)


def py_otu(label):
    m = RE_OTU.search(label)
    return m.group(2) if m else label.split(b";")[0]


def py_tax(label):
    m = RE_TAX.search(label)
    return m.group(2) if m else None


def py_adds(q, t, q_target, sizes, matched):
    """the adds in call order: (query label or None, target label or None, abundance, query number or None, target number or None)"""
    adds = []
    for k, label in enumerate(q):
        tg = int(q_target[k])
        adds.append((label, None if tg == NONE else t[tg], 1 if sizes is None else int(sizes[k]), k, None if tg == NONE else tg))
    if matched is not None:
        adds += [(None, t[j], 0, None, j) for j in range(len(t)) if not matched[j]]
    return adds


def py_otutab(q, t, q_target, sizes=None, matched=None):
    """-> the tuple OtuTable.arrays() returns"""
    samples, otus, tax, count = set(), set(), {}, {}
    for ql, tl, ab, _, _ in py_adds(q, t, q_target, sizes, matched):
        if ql is not None:
            samples.add(py_sample(ql))
        if tl is not None:
            otus.add(py_otu(tl))
            if py_tax(tl) is not None:
                tax[py_otu(tl)] = py_tax(tl)
        if ql is not None and tl is not None and ab != 0:
            key = (py_otu(tl), py_sample(ql))
            count[key] = (count.get(key, 0) + ab) & ((1 << 64) - 1)
    samples, otus = sorted(samples), sorted(otus)
    srank, orank = {s: r for r, s in enumerate(samples)}, {o: r for r, o in enumerate(otus)}
    cells = sorted((orank[o], srank[s], c) for (o, s), c in count.items())
    q_sample = np.array([srank[py_sample(l)] for l in q], np.uint32)
    t_otu = np.full(len(t), NONE, np.uint32)
    for _, tl, _, _, j in py_adds(q, t, q_target, sizes, matched):
        if j is not None:
            t_otu[j] = orank[py_otu(tl)]
    return (samples, otus, [tax.get(o) for o in otus], bool(tax), np.array([c[0] for c in cells], np.uint32).tobytes(),
            np.array([c[1] for c in cells], np.uint32).tobytes(), np.array([c[2] for c in cells], np.uint64).tobytes(),
            q_sample.tobytes(), t_otu.tobytes())


# ---- sets -------------------------------------------------------------------------------------------------------------------------
def sizes_of(labels):
    """--sizein: the ;size= annotation, 1 without one"""
    out = []
    for l in labels:
        m = RE_SIZE.search(l)
        out.append(int(m.group(2)) if m else 1)
    return out


def search_set(name, q, t, hit, same=None, sizein=False, sizes=None, command="search_exact", cli=True, trunc=False):
    """hit[k]: the target whose sequence query k has, or None.  same: {target: the earlier target whose sequence it shares}."""
    return dict(name=name, kind="search", command=command, q=[B(x) for x in q], t=[B(x) for x in t], hit=list(hit),
                same={int(a): int(b) for a, b in (same or {}).items()}, sizein=bool(sizein), sizes=sizes, cli=bool(cli), trunc=bool(trunc))


def cluster_set(name, labels, clusterno, relabel=None, sizein=True, cli=True):
    """labels in processing order; clusterno[s]: the cluster sequence s founds (the next number) or joins"""
    return dict(name=name, kind="cluster", command="cluster_size", q=[B(x) for x in labels], clusterno=list(clusterno),
                relabel=None if relabel is None else B(relabel), sizein=bool(sizein), sizes=None, cli=bool(cli), trunc=False)


def cut(label):
    """what the CLI leaves of a header without --notrunclabels"""
    return re.split(rb"[ \t]", label, maxsplit=1)[0]


def seq_ids(s):
    tid = [s["same"].get(j, j) for j in range(len(s["t"]))]
    qid = [tid[h] if h is not None else 100000 + k for k, h in enumerate(s["hit"])]
    return qid, tid


def inputs(s):
    """-> (query labels, target labels, q_target, sizes or None, matched or None): what vsx_otutab is given"""
    q = [cut(l) for l in s["q"]] if s["trunc"] else s["q"]
    # a search command hands otutable_add the header's ;size= annotation with or without --sizein (commands/search_exact.cpp:489,
    # usearch_global.cpp:448: fastx_get_abundance); only the clustering commands resolve --sizein first (core/cluster.cpp)
    annotated = s["sizein"] or s["kind"] == "search"
    sizes = s["sizes"] if s["sizes"] is not None else (sizes_of(q) if annotated else None)
    if s["kind"] == "cluster":
        ncl = max(s["clusterno"]) + 1 if s["clusterno"] else 0
        centroid = {}
        for k, c in enumerate(s["clusterno"]):
            centroid.setdefault(c, k)
        t = [s["relabel"] + str(c + 1).encode() if s["relabel"] is not None else q[centroid[c]] for c in range(ncl)]
        return q, t, np.array(s["clusterno"], np.uint32), sizes, None
    t = [cut(l) for l in s["t"]] if s["trunc"] else s["t"]
    qid, tid = seq_ids(s)
    q_target = np.full(len(q), NONE, np.uint32)
    matched = np.zeros(len(t), np.uint8)
    for k, x in enumerate(qid):
        hits = [j for j, y in enumerate(tid) if y == x]
        if hits:
            q_target[k] = hits[0]
            matched[hits] = 1
    return q, t, q_target, sizes, matched


def expected(s):
    return py_otutab(*inputs(s))


def call(aligner, s, host=False):
    ot = importlib.import_module("vsearch_amd.otutab")
    q, t, q_target, sizes, matched = inputs(s)
    if host:
        return ot.otutab_host(q, t, q_target, sizes=sizes, matched=matched)
    return ot.otutab(q, t, q_target, sizes=sizes, matched=matched, aligner=aligner)


def texts(table, generated_by="vsearch", date="-"):
    """the three files as the formatters print them (latin-1 text)"""
    ot = importlib.import_module("vsearch_amd.otutab")
    return dict(otutabout=b"".join(l + b"\n" for l in ot.otutabout_lines(table)).decode("latin-1"),
                mothur=b"".join(l + b"\n" for l in ot.mothur_shared_lines(table)).decode("latin-1"),
                biom=ot.biom_text(table, "t.biom", generated_by, date).decode("latin-1"))


def mask_date(biom):
    return re.sub(r'("date": ")[^"]*(")', r"\1-\2", biom)


def generated_by(biom):
    return re.search(r'"generated_by": "([^"]*)"', biom).group(1)


def recorded_search_run():
    """the issue's search run, verbatim: --usearch_global --id 0.9 --maxaccepts 2 --sizein"""
    q = ["S1.r1;size=5", "r2;sample=;x", "r3;barcodelabel=B;sample=A", "xsample=Q_1.7;size=2", ".nohit", "sample=Z;", "S\xe9 blank;sample=W"]
    t = ["otuA;tax=k:Bact;", "x;otu=otuB;size=3", "otuA;tax=k:Arch", ";tax=zz;", "never;otu="]
    return search_set("recorded_search", q, t, [0, 1, 2, 0, None, 3, 1], sizein=True, command="usearch_global", trunc=True)


def recorded_cluster_runs():
    labels = ["s1_a;size=4", "s2.b;size=2", "s1.c;size=1"]
    return [cluster_set("recorded_cluster", labels, [0, 0, 1]), cluster_set("recorded_cluster_relabel", labels, [0, 0, 1], relabel="OTU_")]


def second_hit_set():
    """a target that was only ever a second hit: matched, so not in the unmatched pass, and no query's first hit -- no row"""
    return search_set("second_hit", ["q1;sample=s"], ["first", "second", "third"], [0], same={1: 0})


def lengths_set():
    """labels of 0, 1, 6, 7, 63, 64, 65, 127, 128 and 129 bytes; the long ones are one fallback prefix that ends with the label"""
    def label(n):
        return (b"sample=" + b"w" * 200)[:n] if n <= 7 else (b"W%d_" % n + b"w" * 200)[:n]
    ls = [label(n) for n in (0, 1, 6, 7, 63, 64, 65, 127, 128, 129)]
    return search_set("lengths", ls, ls, list(range(len(ls))), cli=False)


def keyword_offsets_set():
    """each keyword behind a ';' at every offset 44 .. 70 of a 140-byte label (a decoy of it without the ';' before), and at offset 0"""
    q, t = [], []
    for kw in KEYWORDS:
        into = q if kw in KEYWORDS[:2] else t
        for off in range(44, 71):
            head = (b"n" + kw + b"D." + b"p" * 80)[:off - 1] + b";"
            body = head + kw + b"V%d_%d" % (len(kw), off) + b";"
            into.append((body + b"z" * 140)[:140])
        into.append(kw + b"V0_%d;rest" % len(kw))
    hit = [k % len(t) for k in range(len(q))]
    return search_set("keyword_offsets", q, t, hit)


def value_ends_set():
    """values that end exactly at byte 63 / 64 / 65, with and without a ';' behind them, and a 300-byte value"""
    q, t = [], []
    for n in (63, 64, 65):
        q += [b"sample=" + b"v" * (n - 7) + b";tail", b"sample=" + b"v" * (n - 7)]
        t += [b"otu=" + b"o" * (n - 4) + b";tax=" + b"t" * n, b"tax=" + b"t" * (n - 4) + b";otu=" + b"o" * n + b";"]
    q += [b"x;sample=" + b"v" * 300, b"x;sample=" + b"v" * 300 + b";y"]
    t += [b"y;otu=" + b"o" * 300 + b";tax=" + b"t" * 300, b"y;tax=" + b"t" * 300 + b";otu=" + b"o" * 299 + b";"]
    return search_set("value_ends", q, t, list(range(len(q))))


def odd_values_set():
    q = ["r;sample=", "r;sample=;x", "r;sample=a=b;", "xsample=v", "Sample=v", ";;sample=v2", "sample;sample=v3",
         "r;sample=A;barcodelabel=B", "r;barcodelabel=B2;sample=A2", "ab.cd", "ab cd", "ab\xe9cd"]
    t = ["x;tax=T;otu=O", "notu=5;x", ";lead;otu=Q", "nosemi", "e;otu=", "e2;otu=;tax="]
    return search_set("odd_values", q, t, [k % 6 for k in range(len(q))])


def order_set():
    """names "", A, _, a, S1, S10, S1_ and a byte >= 0x80 in one table: memcmp order, the shorter first"""
    names = [b"S10", b"", b"a", b"\xe9", b"S1_", b"A", b"_", b"S1"]
    return search_set("order", [b"r%d;sample=" % k + n for k, n in enumerate(names)], [b"t%d;otu=" % k + n for k, n in enumerate(reversed(names))],
                      list(range(len(names))))


def tax_order_sets():
    """two targets with one OTU name and different taxonomies: the last add decides; once that is the unmatched pass"""
    t = ["o;otu=X;tax=one", "p;otu=X;tax=two", "r;otu=X"]
    return [search_set("tax_first_then_second", ["a", "b", "c"], t, [0, 1, 2]),
            search_set("tax_second_then_first", ["a", "b", "c"], t, [1, 0, 2]),
            search_set("tax_from_unmatched_pass", ["a"], t, [1])]


def abundance_sets():
    return [search_set("abundance_zero", ["a;sample=s", "b;sample=u"], ["o1", "o2"], [0, 1], sizes=[0, 3], cli=False),
            search_set("sum_above_32_bits", ["a;sample=s;size=3000000000", "b;sample=s;size=3000000000"], ["o1"], [0, 0], sizein=True)]


def empty_sets():
    return [search_set("no_query", [], ["o1;tax=t", "o2"], [], cli=False),
            search_set("no_target", ["a", "b;sample=s"], [], [None, None], cli=False),
            search_set("no_hits", ["a", "b;sample=s"], ["o1;tax=t", "o2"], [None, None])]


def cluster_sets():
    labels = ["c1;sample=s1;size=9", "m1;sample=s2;size=5", "c2;barcodelabel=s1;size=4", "m2.x;size=2", "c3;size=1"]
    cno = [0, 0, 1, 1, 2]
    return [cluster_set("cluster_plain", labels, cno), cluster_set("cluster_relabel", labels, cno, relabel="Otu"),
            cluster_set("cluster_relabel_otu_prefix", labels, cno, relabel="P;otu=Q")]


def all_sets():
    return ([recorded_search_run(), second_hit_set()] + recorded_cluster_runs() +
            [lengths_set(), keyword_offsets_set(), value_ends_set(), odd_values_set(), order_set()] + tax_order_sets() + abundance_sets() +
            empty_sets() + cluster_sets())


FRAGMENTS = [b";", b";", b"=", b"_", b".", b"\xe9", b"a", b"S", b"1", b" ", b"sample", b"sample=", b"barcodelabel=", b"barcodelabel", b"otu=", b"otu",
             b"tax=", b"tax", b"ample=", b"tu=", b";sample=", b";otu=", b";tax=", b"label="]


def random_label_set(seed):
    """a few labels made of the keywords' fragments and the bytes that end names"""
    rng = random.Random(seed)
    label = lambda: b"".join(rng.choice(FRAGMENTS) for _ in range(rng.randint(0, 7)))  # noqa: E731
    nq, nt = rng.randint(0, 5), rng.randint(0, 4)
    q, t = [label() for _ in range(nq)], [label() for _ in range(nt)]
    q_target = np.array([rng.randrange(nt) if nt and rng.random() < 0.8 else NONE for _ in range(nq)], np.uint32)
    sizes = None if rng.random() < 0.3 else [rng.choice((0, 1, 1, 2, 7, 1 << 33)) for _ in range(nq)]
    matched = None if rng.random() < 0.3 else [int(rng.random() < 0.6 or j in set(q_target.tolist())) for j in range(nt)]
    return q, t, q_target, sizes, matched


def large_random_inputs(n=50000, seed=211):
    """n queries over 40 samples (half of them by annotation), 300 targets with otu= / tax= on a part, long-tailed hits, 5 % without"""
    rng = random.Random(seed)
    samples = ["smp%d" % k for k in range(40)]
    t = []
    for j in range(300):
        l = "otu%d" % (j // 2 if j % 7 == 0 else j)
        if j % 3 == 0:
            l = "db%d;otu=%s" % (j, l)
        if j % 4 == 0:
            l += ";tax=k:K%d,p:P%d" % (j % 5, j)
        t.append(B(l + (";" if j % 2 else "")))
    q, q_target, sizes = [], [], []
    for k in range(n):
        s = rng.randrange(40)
        q.append(B("%s.%d" % (samples[s], k) if s % 2 else "read%d;sample=%s;size=%d" % (k, samples[s], k % 9)))
        q_target.append(NONE if rng.random() < 0.05 else min(289, int(rng.paretovariate(0.7)) - 1))
        sizes.append(rng.choice((0, 1, 1, 3, 250)))
    matched = np.zeros(300, np.uint8)
    matched[[x for x in q_target if x != NONE]] = 1
    matched[295] = 1                                    # a target that was only ever a later hit
    return q, t, np.array(q_target, np.uint32), sizes, matched


# ---- the reference CLI ----------------------------------------------------------------------------------------------------------
def ref_binary():
    return os.path.join(os.path.dirname(HERE), "oracle", "_ref", "vsearch_ref")


def seq_of(i, n=48):
    rng = random.Random(7919 * i + 13)
    return "".join(rng.choice("ACGT") for _ in range(n))


def near(seq, k=1):
    """`seq` with k substitutions, spread"""
    s = list(seq)
    for j in range(k):
        p = (j + 1) * len(s) // (k + 1)
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1) % 4]
    return "".join(s)


def write_fasta(path, labels, seqs):
    with open(path, "wb") as f:
        for l, s in zip(labels, seqs):
            f.write(b">" + l + b"\n" + s.encode() + b"\n")


def run_cli(tmp, args, extra):
    out = {k: os.path.join(tmp, f) for k, f in (("otutabout", "t.tsv"), ("mothur", "t.shared"), ("biom", "t.biom"))}
    cmd = [ref_binary()] + args + ["--otutabout", "t.tsv", "--mothur_shared_out", "t.shared", "--biomout", "t.biom", "--threads", "1", "--quiet"] + extra
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}\n{r.stderr[-2000:]}")
    return {k: open(p, "rb").read().decode("latin-1") for k, p in out.items()}


def run_reference(s):
    """-> {"otutabout", "mothur", "biom"}: the reference CLI's three files for the set (latin-1 text)"""
    with tempfile.TemporaryDirectory(prefix="vsx_otutab_") as tmp:
        extra = (["--sizein"] if s["sizein"] else []) + ([] if s["trunc"] else ["--notrunclabels"])
        if s["kind"] == "cluster":
            sizes = sizes_of(s["q"])
            seqs, founder = [], {}
            for k, c in enumerate(s["clusterno"]):
                founder.setdefault(c, k)
                seqs.append(seq_of(c) if founder[c] == k else near(seq_of(c), 1 + (k % 2)))
            assert sizes == sorted(sizes, reverse=True)
            write_fasta(os.path.join(tmp, "in.fa"), s["q"], seqs)
            if s["relabel"] is not None:
                extra += ["--relabel", s["relabel"].decode("latin-1")]
            return run_cli(tmp, ["--cluster_size", "in.fa", "--id", "0.9", "--qmask", "none", "--minseqlength", "1"], extra)
        qid, tid = seq_ids(s)
        write_fasta(os.path.join(tmp, "db.fa"), s["t"], [seq_of(i) for i in tid])
        write_fasta(os.path.join(tmp, "q.fa"), s["q"], [seq_of(i) for i in qid])
        args = ["--" + s["command"], "q.fa", "--db", "db.fa", "--qmask", "none", "--dbmask", "none", "--minseqlength", "1"]
        if s["command"] == "usearch_global":
            args += ["--id", "0.9", "--maxaccepts", "2"]
        return run_cli(tmp, args, extra)


def second_hit_reference():
    """the issue's second-hit run as the CLI sees it: `second` one substitution from `first`, --usearch_global --maxaccepts 2"""
    with tempfile.TemporaryDirectory(prefix="vsx_otutab_") as tmp:
        write_fasta(os.path.join(tmp, "db.fa"), [b"first", b"second", b"third"], [seq_of(0), near(seq_of(0)), seq_of(2)])
        write_fasta(os.path.join(tmp, "q.fa"), [b"q1;sample=s"], [seq_of(0)])
        return run_cli(tmp, ["--usearch_global", "q.fa", "--db", "db.fa", "--qmask", "none", "--dbmask", "none", "--minseqlength", "1", "--id", "0.9",
                             "--maxaccepts", "2"], ["--notrunclabels"])


def to_json(s):
    d = dict(s)
    d["q"] = [l.decode("latin-1") for l in s["q"]]
    if "t" in s:
        d["t"] = [l.decode("latin-1") for l in s["t"]]
    if s.get("relabel") is not None:
        d["relabel"] = s["relabel"].decode("latin-1")
    if "same" in s:
        d["same"] = {str(a): b for a, b in s["same"].items()}
    return d


def from_json(d):
    s = dict(d)
    s["q"] = [B(l) for l in d["q"]]
    if "t" in d:
        s["t"] = [B(l) for l in d["t"]]
    if d.get("relabel") is not None:
        s["relabel"] = B(d["relabel"])
    if "same" in d:
        s["same"] = {int(a): int(b) for a, b in d["same"].items()}
    return s


def write_golden(path=GOLDEN):
    out = []
    for s in all_sets():
        d = to_json(s)
        d["ref"] = run_reference(s) if s["cli"] else None
        if s["name"] == "second_hit":
            assert second_hit_reference() == d["ref"]            # duplicates under --search_exact and near copies under --usearch_global agree
        out.append(d)
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


def load_golden(path=GOLDEN):
    with open(path) as f:
        return [from_json(d) for d in json.load(f)]


def device_digest(aligner):
    """one digest over the device route's result arrays of every set"""
    import hashlib
    h = hashlib.sha256()
    for s in all_sets():
        res = call(aligner, s)
        if res.stats["labels_host"] or not (res.stats["labels_device"] or not len(s["q"])):
            raise RuntimeError(f"{s['name']}: the device route did not answer")
        h.update(repr(res.arrays()).encode())
    return h.hexdigest()


if __name__ == "__main__":
    import sys
    if "--digest" in sys.argv:
        from vsearch_amd import Aligner, load_library
        with Aligner(device=0) as al:
            print("digest", device_digest(al), "poison", load_library().vsx_internal_poison_byte())
    else:
        write_golden()
        print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
