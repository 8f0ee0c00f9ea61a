"""Inputs, a plain-Python restatement and the reference-CLI runner for the SINTAX tests (--sintax).

    py_sintax()       words in first-occurrence order, the per-query SplitMix64 stream, rounds, strand choice, vote: plain Python
    py_tabbed()       the --tabbedout lines from py_sintax's records
    *_set()           input builders, one per group of cases
    run_reference()   the reference CLI (oracle/_ref/vsearch_ref) on one set: --tabbedout and the log's closing line
    __main__          writes tests/golden/sintax_golden.json: the sets' inputs and the reference's recorded lines, nothing else
"""
import json
import os
import random
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "sintax_golden.json")

RANKS = "dkpcofgst"
ROUNDS, SUBSET = 100, 32
# The reference's --sintax never runs DUST on the database: with --dbmask dust (its default) the index only leaves out the words over
# lower-case symbols of the input, exactly as --dbmask soft does.  So both map to the searcher's soft masking; "dust_masked" is a
# searcher that really DUST-masks its database (soft_mask 2), which no command line of the reference reaches.
MASK_MODES = {"none": 0, "soft": 1, "dust": 1, "dust_masked": 2}
M64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15
COMPLEMENT = dict(zip("ABCDGHKMNRSTUVWY", "TVGHCDMKNYSAABWR"))
DEFAULT_OPTS = dict(seed=1, strand_both=1, cutoff=0.0, dbmask="dust", hardmask=0, wordlength=8, random=0)


def full_opts(opts):
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    return o


def revcomp(s):
    """chrmap_complement: case kept for the letters that have a complement, everything else N"""
    out = []
    for c in reversed(s):
        u = COMPLEMENT.get(c.upper(), "N")
        out.append(u.lower() if c.islower() and c in "abcdghkmnrstuvwy" else u)
    return "".join(out)


# ---- the stream ------------------------------------------------------------------------------------------------------------------
class Stream:
    def __init__(self, base, index):
        self.state = (base ^ (index * GAMMA)) & M64
        self.state = self.next()

    def next(self):
        self.state = (self.state + GAMMA) & M64
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    def bounded(self, n):
        prod = self.next() * n
        low = prod & M64
        if low < n:
            threshold = ((1 << 64) - n) % n
            while low < threshold:
                prod = self.next() * n
                low = prod & M64
        return prod >> 64


# ---- words -----------------------------------------------------------------------------------------------------------------------
TWO_BIT = {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3}


def words_of(seq, w, lower_masks):
    """the distinct words in first-occurrence order; a symbol outside ACGTU poisons its words, and so does a lower-case symbol
    when lower_masks is set (every --dbmask but none)"""
    out, seen = [], set()
    for p in range(len(seq) - w + 1):
        win = seq[p:p + w]
        if any(c.upper() not in TWO_BIT or (lower_masks and c.islower()) for c in win):
            continue
        v = 0
        for c in win:
            v = (v << 2) | TWO_BIT[c.upper()]
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def masked_db(db, dbmask, hardmask):
    """the database text as it is indexed (the restatement restates the classification, not DUST: vsx_dust_mask finds the intervals)"""
    if dbmask == "dust_masked":
        from vsearch_amd import dust_mask
        db = [m.decode("latin-1") for m in dust_mask(list(db))]
    if hardmask and dbmask != "none":
        db = ["".join("N" if c.islower() else c for c in s) for s in db]
    return list(db)


# ---- labels ----------------------------------------------------------------------------------------------------------------------
def tax_split(h):
    """-> the nine names of a header; tax_parse + tax_split of the reference with their quirks"""
    names = [""] * 9
    offset, found = 0, False
    while offset < len(h) - 4:
        p = h.find("tax=", offset)
        if p < 0:
            break
        offset = p
        if offset > 0 and h[offset - 1] != ";":
            offset += 5
            continue
        tax_start = offset
        e = h.find(";", offset + 4)
        tax_end = e if e >= 0 else len(h)
        found = True
        break
    if not found:
        return names
    offset = tax_start + 4
    while offset < tax_end:
        level = RANKS.find(h[offset].lower())
        if level >= 0 and h[offset + 1:offset + 2] == ":":
            comma = h.find(",", offset + 2)
            names[level] = h[offset + 2:comma] if comma >= 0 else h[offset + 2:tax_end]
        comma = h.find(",", offset)
        offset = comma + 1 if comma >= 0 else tax_end
    return names


# ---- the classification ----------------------------------------------------------------------------------------------------------
def py_sintax(s, first_query_no=0, query_numbers=None, queries=None, rounds=False):
    """-> per query dict(strand, classified, boot_count, best_count, ranks = [(sequence, votes)] * 9, candidates = [plus, minus]);
    with rounds=True also round_counts = every round's winning count per strand, dropped rounds included"""
    o = full_opts(s["opts"])
    w = o["wordlength"]
    db = masked_db(s["db"], o["dbmask"], o["hardmask"])
    index = {}
    for t, seq in enumerate(db):
        for v in words_of(seq, w, o["dbmask"] != "none"):
            index.setdefault(v, []).append(t)
    names = [tax_split(h) for h in s["db_labels"]]
    lengths = [len(x) for x in db]
    out = []
    qs = s["queries"] if queries is None else queries
    for k, q in enumerate(qs):
        qno = first_query_no + k if query_numbers is None else query_numbers[k]
        rng = Stream(o["seed"], qno)
        cands, best, round_counts = [[], []], [0, 0], [[], []]
        for strand in range(2 if o["strand_both"] else 1):
            words = words_of(revcomp(q) if strand else q, w, False)
            if len(words) < SUBSET:
                continue
            for _ in range(ROUNDS):
                taken, sample = set(), []
                for _ in range(SUBSET):
                    x = rng.bounded(len(words))
                    if x not in taken:
                        taken.add(x)
                        sample.append(words[x])
                counts = {}
                for v in sample:
                    for t in index.get(v, ()):
                        counts[t] = counts.get(t, 0) + 1
                if o["random"]:
                    bc, bs, ties = 0, 0, 0
                    for t in range(len(db)):
                        c = counts.get(t, 0)
                        if c > bc:
                            bc, bs, ties = c, t, 1
                        elif c == bc:
                            ties += 1
                            if rng.bounded(ties) == 0:
                                bs = t
                else:
                    bc, bs = 0, 0
                    if counts:
                        bc, _, bs = max((c, -lengths[t], -t) for t, c in counts.items())
                        bs = -bs
                round_counts[strand].append(bc)
                if bc > 1:
                    cands[strand].append(bs)
                    best[strand] = max(best[strand], bc)
        boot = [len(cands[0]), len(cands[1])]
        strand = 0
        if o["strand_both"]:
            if best[1] > best[0] or (best[1] == best[0] and boot[1] > boot[0]):
                strand = 1
        count = boot[strand]
        rec = dict(strand=strand, classified=int(count >= 50), boot_count=boot, best_count=best, candidates=cands,
                   ranks=[(0xffffffff, 0)] * 9)
        if rec["classified"]:
            incl = list(range(count))
            ranks = []
            for level in range(9):
                groups = {}
                for i in incl:
                    groups.setdefault(names[cands[strand][i]][level], []).append(i)
                most = max(len(g) for g in groups.values())
                winner = min(g[0] for g in groups.values() if len(g) == most)
                ranks.append((cands[strand][winner], most))
                incl = groups[names[cands[strand][winner]][level]]
            rec["ranks"] = ranks
        if rounds:
            rec["round_counts"] = round_counts
        out.append(rec)
    return out


def py_tabbed(s, recs, qlabels=None, cutoff=None):
    cutoff = full_opts(s["opts"])["cutoff"] if cutoff is None else cutoff
    qlabels = s["qlabels"] if qlabels is None else qlabels
    lines = []
    for q, r in enumerate(recs):
        if not r["classified"]:
            lines.append(qlabels[q] + ("\t\t\t" if cutoff > 0 else "\t\t"))
            continue
        count = r["boot_count"][r["strand"]]
        full, cut = [], []
        for level, (seq, votes) in enumerate(r["ranks"]):
            name = tax_split(s["db_labels"][seq])[level]
            if name:
                full.append("%s:%s(%.2f)" % (RANKS[level], name, 1.0 * votes / count))
                if 1.0 * votes / count >= cutoff:
                    cut.append("%s:%s" % (RANKS[level], name))
        line = qlabels[q] + "\t" + ",".join(full) + "\t" + "+-"[r["strand"]]
        if cutoff > 0:
            line += "\t" + ",".join(cut)
        lines.append(line)
    return lines


def py_log(recs):
    n, c = len(recs), sum(r["classified"] for r in recs)
    return ["Classified %d of %d sequences" % (c, n) + (" (%.2f%%)" % (100.0 * c / n) if n else "")]


# ---- input builders --------------------------------------------------------------------------------------------------------------
def random_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, rate):
    return "".join(rng.choice([b for b in "ACGT" if b != c]) if rng.random() < rate else c for c in s)


def no_repeat_seq(rng, n, w=8):
    """a sequence of n symbols whose n - w + 1 words are all distinct"""
    while True:
        s = random_seq(rng, n)
        if len(words_of(s, w, False)) == n - w + 1:
            return s


def taxonomy_db(rng, families=3, genera=2, species=2, length=240):
    """families x genera x species sequences: a genus is 8 % from its family's ancestor, a species 3 % from its genus"""
    db, labels = [], []
    for f in range(families):
        fa = random_seq(rng, length)
        for g in range(genera):
            ga = mutate(rng, fa, 0.08)
            for sp in range(species):
                db.append(mutate(rng, ga, 0.03))
                labels.append(f"ref{len(db)};tax=d:Bacteria,k:K{f % 2},p:P{f},c:C{f},o:O{f},f:F{f},g:G{f}_{g},s:S{f}_{g}_{sp},t:T{len(db)};")
    return db, labels


def _set(name, db, labels, queries, opts=None, qlabels=None):
    return dict(name=name, db=list(db), db_labels=list(labels), queries=list(queries), opts=dict(opts or {}),
                qlabels=list(qlabels) if qlabels else [f"q{k};sample=x" for k in range(len(queries))])


def basic_queries(rng, db):
    """K = 31, 32, 33; shorter than a word; N's that leave < 32 words; lower case; both strands; one unrelated read"""
    a = db[0]
    qs = [no_repeat_seq(rng, 38), no_repeat_seq(rng, 39), no_repeat_seq(rng, 40), "ACGTA"]
    qs.append("".join("N" if i % 9 == 8 else c for i, c in enumerate(a[:150])))        # one word between two N's: 16 words
    qs.append(a[20:170].lower())
    qs.append(a[10:49])                                  # K = 32 from the database: 32 draws from 32 words repeat
    qs += [db[3][30:180], revcomp(db[5][30:180]), db[7][:160], revcomp(db[8][40:200]), random_seq(rng, 150)]
    qs.append(a[:100] + "NNNNNNNN" + a[108:180])
    return qs


def basic_set(strand_both=1, cutoff=0.8, name="basic_both", **extra):
    rng = random.Random(101)
    db, labels = taxonomy_db(rng)
    o = dict(seed=7, strand_both=strand_both, cutoff=cutoff)
    o.update(extra)
    return _set(name, db, labels, basic_queries(rng, db), o)


def ties_set():
    """identical sequences (the lower number wins); equal counts with different lengths (the shorter wins, also when it comes
    later); a sequence that is a prefix of another"""
    rng = random.Random(103)
    a, b, c = (random_seq(rng, 200) for _ in range(3))
    db = [a, a, b + random_seq(rng, 40), b, c[:120], c, random_seq(rng, 200)]
    labels = [f"r{k};tax=d:D,p:P{k // 2},g:G{k},s:S{k};" for k in range(len(db))]
    qs = [a[20:150], b[10:160], c[:110], revcomp(a[40:170]), c[5:100]]
    return _set("ties", db, labels, qs, dict(seed=11, strand_both=1))


LABEL_QUIRKS = [
    "plain_no_taxonomy",
    "x;xtax=d:Wrong,g:Wrong;",
    "tax=d:First,p:InFront,g:Gfirst;size=3",
    "id1;size=2;tax=d:Last,p:NoSemicolon,g:Glast",
    "id2;tax=D:Upper,K:Kup,P:Pup,G:Gup;",
    "id3;tax=d:Dom,x:Unknown,p:Phy,z:Zed,g:Gen;",
    "id4;tax=d:Dom,p:Early,g:Gen4,p:Late;",
    "id5;tax=d:Dom,p:Phy,g:NoFamilyOrOrder,s:Sp5;",
    "id6;tax=d:Dom,p:Phy,g:Spill;note=a,b;",
    "id7 with spaces;tax=d:Dom,p:Phy,g:Gen 7,s:Homo sapiens;",
    "id8;tax=d:Dom,k:Kin,p:Phy,c:Cla,o:Ord,f:Fam,g:Gen8,s:Sp8,t:Str8;",
    "id9;xtax=d:No;tax=d:Second,g:AfterX;",
]


def labels_set():
    rng = random.Random(107)
    db = [random_seq(rng, 180) for _ in LABEL_QUIRKS]
    qs = [s[15:165] for s in db]
    return _set("labels", db, LABEL_QUIRKS, qs, dict(seed=13, strand_both=0, cutoff=0.5), qlabels=[f"read {k} from {k}" for k in range(len(qs))])


def vote_set(cutoff=0.0, name=None, copies=4):
    """reads whose halves come from two sequences of different genera (and, for others, different families or only different
    species): the round winners split, names tie or win narrowly, and the losers leave the vote below"""
    rng = random.Random(109)
    db, labels = taxonomy_db(rng, families=2, genera=2, species=2, length=200)
    # a missing middle rank on one species: its empty family name votes against F0
    labels[1] = labels[1].replace(",f:F0", "")
    mixes = [(0, 2), (0, 1), (0, 4), (2, 3), (1, 6)]
    qs = []
    for a, b in mixes:
        qs += [db[a][:75] + db[b][75:150]] * copies
    return _set(name or "vote", db, labels, qs, dict(seed=17, strand_both=0, cutoff=cutoff))


def weak_query(rng, a, b, shared, total=200):
    """a read that shares only `shared` consecutive symbols with each of two sources"""
    fill = total - 2 * shared
    return random_seq(rng, fill // 3) + a[60:60 + shared] + random_seq(rng, fill // 3) + b[90:90 + shared] + random_seq(rng, fill - 2 * (fill // 3))


def candidates_set(copies=16, cutoff=0.0, name="candidates", shared=13):
    """the same weakly matching read many times: every copy has its own query number, hence its own stream, and the candidate
    counts scatter around 50; rounds whose winner counts 1 are dropped, 2 kept.  The winners split between two families."""
    rng = random.Random(113)
    db, labels = taxonomy_db(rng, families=2, genera=1, species=2, length=200)
    q = weak_query(rng, db[0], db[2], shared)
    return _set(name, db, labels, [q] * copies, dict(seed=11, strand_both=0, cutoff=cutoff))


def strands_set(copies=8):
    """reads that equal their own reverse complement (X + rc(X)): both strands read the same text with different draws, so the best
    counts tie or not and the candidate counts decide either way; strong copies tie completely (plus); skewed reads give each
    strand a clear win on the best count"""
    rng = random.Random(127)
    db, labels = taxonomy_db(rng, families=2, genera=1, species=2, length=200)
    x = random_seq(rng, 70) + db[0][60:79] + random_seq(rng, 11)
    weak = x + revcomp(x)
    strong = db[1][40:120] + revcomp(db[1][40:120])
    qs = [weak] * copies + [strong] * 4
    qs += [db[2][10:150] + revcomp(db[3][150:190]), revcomp(db[2][10:150]) + db[3][150:190]]
    return _set("strands", db, labels, qs, dict(seed=5, strand_both=1, cutoff=0.8))


def masking_sets(hardmask=0):
    """a two-letter stretch (lower case in the input, DUST masks it anyway) carries the read's only shared words"""
    rng = random.Random(131)
    low = random_seq(rng, 72, "AT")
    db, labels = taxonomy_db(rng, families=2, genera=1, species=1, length=160)
    db[0] = db[0][:80] + low.lower() + db[0][80:]
    qs = [random_seq(rng, 60) + low + random_seq(rng, 60), db[1][10:150], db[0][:78]]
    return [_set(f"masking_{mode}" + ("_hard" if hard else ""), db, labels, qs, dict(seed=29, strand_both=0, dbmask=mode, hardmask=hard))
            for mode, hard in ((("dust", 1), ("soft", 1)) if hardmask else (("none", 0), ("soft", 0), ("dust", 0)))]


def hardmask_sets():
    """--hardmask on the database and a really DUST-masked database (the searcher's options; the reference's command line refuses
    --hardmask for --sintax and never runs DUST there, so these sets are compared between the restatements and the device only)"""
    out = masking_sets(hardmask=1)
    for s in masking_sets()[:1] + masking_sets(hardmask=1)[:1]:
        t = dict(s, name=s["name"].replace("none", "dust").replace("dust", "dust_masked"), opts=dict(s["opts"], dbmask="dust_masked"))
        t["db"] = [x.upper() for x in s["db"]]
        out.append(t)
    return out


def wordlength_sets():
    out = []
    for w in (3, 5, 12):
        s = basic_set(name=f"wordlength_{w}", wordlength=w)
        out.append(s)
    return out


def random_set():
    rng = random.Random(137)
    db, labels = taxonomy_db(rng, families=2, genera=2, species=2, length=160)
    qs = [db[0][10:150], revcomp(db[5][5:140]), random_seq(rng, 120), db[2][:70] + db[3][70:140], "ACGT"]
    return _set("sintax_random", db, labels, qs, dict(seed=31, strand_both=1, random=1, cutoff=0.5))


def rounding_set():
    """the candidates set (fewer than 100 candidates: scores that are no multiples of 0.01) under a cutoff equal to a printed score
    that was rounded UP: the rank must stay out of the fourth column"""
    s = candidates_set()
    for r in py_sintax(s):
        if not r["classified"]:
            continue
        count = r["boot_count"][r["strand"]]
        for _, votes in r["ranks"]:
            printed = float("%.2f" % (votes / count))
            if printed > votes / count:
                return candidates_set(cutoff=printed)
    raise AssertionError("no score of the candidates set rounds up")


def golden_sets():
    return ([basic_set(), basic_set(strand_both=0, cutoff=0.0, name="basic_plus"), ties_set(), labels_set(), vote_set(),
             vote_set(0.5, "vote_cutoff_0.5"), vote_set(0.8, "vote_cutoff_0.8"), vote_set(1.0, "vote_cutoff_1.0"), rounding_set(),
             strands_set(), random_set()] + masking_sets() + wordlength_sets())


# ---- the reference CLI -----------------------------------------------------------------------------------------------------------
def ref_binary():
    return os.path.join(ROOT, "oracle", "_ref", "vsearch_ref")


def _fasta(path, names, seqs):
    with open(path, "w") as f:
        for n, s in zip(names, seqs):
            f.write(f">{n}\n{s}\n")


def cli_args(opts):
    o = full_opts(opts)
    a = ["--randseed", str(o["seed"]), "--strand", "both" if o["strand_both"] else "plus", "--dbmask", o["dbmask"],
         "--wordlength", str(o["wordlength"])]
    if o["cutoff"] > 0:
        a += ["--sintax_cutoff", repr(o["cutoff"])]
    if o["hardmask"]:
        a.append("--hardmask")
    if o["random"]:
        a.append("--sintax_random")
    return a


def run_reference(s, threads=1):
    """-> dict(tabbed = the --tabbedout lines in query order, log = the "Classified ..." line)"""
    with tempfile.TemporaryDirectory(prefix="vsx_sintax_") as tmp:
        p = lambda n: os.path.join(tmp, n)
        _fasta(p("db.fa"), s["db_labels"], s["db"])
        _fasta(p("q.fa"), s["qlabels"], s["queries"])
        args = [ref_binary(), "--sintax", p("q.fa"), "--db", p("db.fa"), "--tabbedout", p("out.tsv"), "--threads", str(threads),
                "--log", p("log.txt"), "--quiet"] + cli_args(s["opts"])
        r = subprocess.run(args, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{s['name']}: reference CLI failed: {r.stderr[-2000:]}")
        lines = open(p("out.tsv")).read().split("\n")[:-1]
        if threads > 1:
            order = {l: k for k, l in enumerate(s["qlabels"])}
            lines.sort(key=lambda l: order[l.split("\t")[0]])
        return dict(tabbed=lines, log=[l for l in open(p("log.txt")).read().splitlines() if l.startswith("Classified ")])


INPUT_KEYS = ("name", "db", "db_labels", "queries", "qlabels", "opts")


SHARED_KEYS = ("db", "db_labels", "queries", "qlabels")


def write_golden(path=GOLDEN):
    """a set whose sequences and labels equal an earlier set's (another cutoff, strand option or word length on the same
    input) is stored as a reference to it"""
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
        n = sum(1 for l in rec["ref"]["tabbed"] if l.split("\t")[1])
        print(f"{rec['name']}: {len(rec['queries'])} queries, {len(rec['db'])} database sequences, {n} classified; {rec['ref']['log']}")
