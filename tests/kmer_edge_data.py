"""Inputs that put the k-mer candidate stage (vsearch_amd/csrc/vsx_kmer.hip) on its counter, threshold, bucket and selection edges,
and an independent restatement of what it must answer.

py_candidates() restates search_topscores (reference core/searchcore.cpp:260-340 over the words of core/unique.cpp) in plain Python:
the unique valid words of the query, one count per target and shared word, the threshold min(--minwordmatches, words), the order
count descending / length ascending / sequence number ascending, the cut to the heap size.  It works on strings and dictionaries
and shares nothing with vsx_search.cpp.

The builders are deterministic from their seed and return (db, queries, opts, expect): `opts` are SearchSession options, `expect`
one dictionary per edge (its "edge" text names it, "query" is the query it belongs to).  Two facts make exact counts cheap:
a prefix of c + w - 1 symbols of a query whose words are all distinct shares exactly c words with it, and text over ACG never
contains a word that has a T.  Every builder re-draws until the restatement confirms what `expect` claims;
tests/test_kmer_edges_host.py asserts it again, edge by edge, without a device, and tests/test_gpu_kmer_edges.py compares the
device, the host restatement of the library and py_candidates() on the same inputs.

Layout facts used here (vsx_kmer_pack.h, vsx_kmer.hip):
  packed index (word lengths 3..8): tiles of 32 630 sequences; sequence s of a tile owns counter (s mod 130) * 252 + s div 130,
      counters 251 mod 252 are dummies; a bucket is sorted counters in 16-byte units of a 16-bit first value + 14 one-byte gaps;
  tagged index (word lengths 9..15): tiles of 32 768, counter = tile-local sequence, a bucket per last-eight-symbols, four
      postings (tag << 16 | sequence) per unit;
  counters are bytes (four per dword) for queries of at most 255 unique words, 16-bit (two per dword) above;
  query word i of the byte class goes to wave i mod 8, lane i div 8; a wave streams its buckets as one run, 64 units per trip.
"""
import ctypes as C
import functools
import random
from collections import Counter

import numpy as np

TILE_SEQS = 32630
PERIOD, REAL, ROWS = 252, 251, 130
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def word_value(word):
    """2-bit map A0 C1 G2 T3, first symbol most significant"""
    v = 0
    for ch in word:
        v = v * 4 + _CODE[ch]
    return v


def words_of(seq, w, soft_mask=0):
    """the distinct valid words of a sequence, as upper-case ACGT strings: all w symbols A/C/G/T/U, and upper case under soft masking"""
    s = seq if soft_mask else seq.upper()
    ok = [ch in "ACGTU" for ch in s]
    s = s.replace("U", "T")
    if all(ok):
        return {s[i:i + w] for i in range(len(s) - w + 1)}
    out = set()
    run = 0
    for i, good in enumerate(ok):
        run = run + 1 if good else 0
        if run >= w:
            out.add(s[i - w + 1:i + 1])
    return out


_INDEX = {}


def _index(db, w, soft_mask=0):
    """word -> the sequences that contain it (once per sequence), and the number of (word, sequence) pairs"""
    key = (id(db), w, soft_mask)
    hit = _INDEX.get(key)
    if hit is None or hit[0] is not db:
        post, n = {}, 0
        for t, s in enumerate(db):
            ws = words_of(s, w, soft_mask)
            n += len(ws)
            for x in ws:
                post.setdefault(x, []).append(t)
        hit = _INDEX[key] = (db, post, n)
    return hit


def posting_count(db, w, soft_mask=0):
    return _index(db, w, soft_mask)[2]


def holders(db, w, word):
    return list(_index(db, w)[1].get(word, ()))


def py_counts(db, query, w, soft_mask=0):
    post = _index(db, w, soft_mask)[1]
    cnt = Counter()
    for x in words_of(query, w, soft_mask):
        cnt.update(post.get(x, ()))
    return cnt


def py_candidates(db, query, w, minwordmatches, tophits, soft_mask=0):
    mm = min(minwordmatches, len(words_of(query, w, soft_mask)))
    if mm == 0:
        return None                                   # every sequence qualifies: the host route
    hits = [(t, c) for t, c in py_counts(db, query, w, soft_mask).items() if c >= mm]
    hits.sort(key=lambda tc: (-tc[1], len(db[tc[0]]), tc[0]))
    return hits[:tophits]


def tophits_of(opts, n_db):
    """min(maxaccepts + maxrejects + 8, sequences); 0 means all (the library's defaults are 1 and 32)"""
    ma, mr = opts.get("maxaccepts", 1), opts.get("maxrejects", 32)
    ma = n_db if ma == 0 or ma > n_db else ma
    mr = n_db if mr == 0 or mr > n_db else mr
    return min(ma + mr + 8, n_db)


def expected(db, queries, opts, minwordmatches=None):
    mm = opts["minwordmatches"] if minwordmatches is None else minwordmatches
    top = tophits_of(opts, len(db))
    return [py_candidates(db, q, opts["wordlength"], mm, top) for q in queries]


# ---- the packed format, restated and through the library's host entry -----------------------------------------------------------
def counter_of(local_seq):
    return (local_seq % ROWS) * PERIOD + local_seq // ROWS


def seq_of(counter):
    return (counter % PERIOD) * ROWS + counter // PERIOD


@functools.lru_cache(maxsize=None)
def _pack_lib():
    from vsearch_amd import _lib
    lib = _lib.load()
    lib.vsx_internal_kmer_pack_encode.restype = C.c_int64
    lib.vsx_internal_kmer_pack_encode.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    lib.vsx_internal_kmer_pack_count.restype = None
    lib.vsx_internal_kmer_pack_count.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    lib.vsx_internal_kmer_pack_counter_of.restype = C.c_uint32
    lib.vsx_internal_kmer_pack_counter_of.argtypes = [C.c_uint32]
    return lib


def pack_units(counters):
    """the library's encoder (the code the build kernel runs) on a set of counters -> the number of 16-byte units"""
    a = np.array(sorted(counters), dtype=np.uint32)
    n = int(_pack_lib().vsx_internal_kmer_pack_encode(a.ctypes.data, len(a), None, 0))
    assert n >= 0
    return n


def pack_encode(counters):
    a = np.array(sorted(counters), dtype=np.uint32)
    n = pack_units(counters)
    units = np.zeros(4 * max(1, n), dtype=np.uint32)
    assert _pack_lib().vsx_internal_kmer_pack_encode(a.ctypes.data, len(a), units.ctypes.data, n) == n
    return units[:4 * n]


def pack_decode(units):
    """every increment the units make, in order: a 16-bit first counter and fourteen gaps per unit"""
    raw = np.asarray(units, dtype="<u4").tobytes()
    out = []
    for u in range(len(raw) // 16):
        b = raw[16 * u:16 * u + 16]
        acc = b[0] | (b[1] << 8)
        out.append(acc)
        for k in range(2, 16):
            acc += b[k]
            out.append(acc)
    return out


def bucket_units(db, w, word, tile=0):
    """units of one word's bucket in one tile of the packed index over db"""
    cs = [counter_of(t - tile * TILE_SEQS) for t in holders(db, w, word) if t // TILE_SEQS == tile]
    return pack_units(cs)


# ---- pieces ------------------------------------------------------------------------------------------------------------------------
def rnd(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def distinct_words_seq(rng, n_words, w, avoid=()):
    """n_words + w - 1 random symbols whose n_words words are all distinct and not in `avoid`"""
    while True:
        s = [rng.choice("ACGT") for _ in range(w - 1)]
        seen = set()
        while len(seen) < n_words:
            for _ in range(12):
                ch = rng.choice("ACGT")
                wd = "".join(s[len(s) - w + 1:]) + ch
                if wd not in seen and wd not in avoid:
                    break
            else:
                break
            s.append(ch)
            seen.add(wd)
        if len(seen) == n_words:
            return "".join(s)


def prefix_with(q, c, w):
    """the prefix of q that holds its first c words (none for c = 0)"""
    return q[:c + w - 1]


def zero_filler(rng, n, w, words):
    """ACG text that shares no word with `words`"""
    while True:
        s = rnd(rng, n, "ACG")
        if not (words_of(s, w) & words):
            return s


def marker(rng, used):
    """a word with its only T in front: text put together from such markers and ACG filler holds a marker only where one was put"""
    while True:
        m = "T" + rnd(rng, 7, "ACG")
        if m not in used:
            used.add(m)
            return m


def substitute(rng, s, rate):
    return "".join((rng.choice([c for c in "ACGT" if c != ch]) if rng.random() < rate else ch) for ch in s)


# ---- 1. the 255 / 256 class switch ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def class_switch(seed=101):
    rng = random.Random(seed)
    w = 8
    opts = dict(wordlength=w, minwordmatches=12, maxaccepts=1, maxrejects=32)
    while True:
        db, queries, expect, avoid = [], [], [], set()
        for n in (254, 255, 256, 257):
            q = distinct_words_seq(rng, n, w, avoid)
            avoid |= words_of(q, w)
            mid = len(q) // 2
            sub = q[:mid] + rng.choice([c for c in "ACGT" if c != q[mid]]) + q[mid + 1:]
            base = len(db)
            db += [q, sub, q[:-1]] + [rnd(rng, rng.randint(240, 280)) for _ in range(20)]
            expect.append(dict(edge=f"query of exactly {n} unique words ({'byte' if n <= 255 else '16-bit'} counters): an exact copy "
                                    f"(count {n}), one substitution (count {n - w}), a prefix (count {n - 1})",
                               query=len(queries), n_words=n, counts={base: n, base + 1: n - w, base + 2: n - 1}))
            queries.append(q)
        if all(len(words_of(queries[e["query"]], w)) == e["n_words"] and
               all(py_counts(db, queries[e["query"]], w)[t] == c for t, c in e["counts"].items()) for e in expect):
            return db, queries, opts, expect


# ---- 2. thresholds around the counter values, neighbours in one dword ---------------------------------------------------------------
MM_BYTE = (1, 2, 127, 128, 129, 200, 254, 255)
MM_HALF = (255, 256, 257, 300)
MM_ALL = tuple(sorted(set(MM_BYTE + MM_HALF + (256,))))


@functools.lru_cache(maxsize=None)
def threshold_edges(w=8, seed=202):
    """queries 0 (255 words, byte counters) and 1 (400 words, 16-bit counters); for every threshold mm of its class a group of four
    sequences whose counters share a dword (byte class) or two neighbouring dwords (16-bit class: two counters each): prefixes with
    counts mm - 1, mm, min(mm + 1, words) and a sequence that shares nothing.  The GPU test opens one session per --minwordmatches
    of MM_ALL and runs both queries; expect[k]["minwordmatches"] says which session an edge is about."""
    rng = random.Random(seed + w)
    opts = dict(wordlength=w, maxaccepts=1, maxrejects=32)
    n_db = 4 * ROWS
    while True:
        q8 = distinct_words_seq(rng, 255, w)
        q16 = distinct_words_seq(rng, 400, w, words_of(q8, w))
        qwords = words_of(q8, w) | words_of(q16, w)
        db = [None] * n_db
        expect = []
        groups = [(0, mm) for mm in MM_BYTE] + [(1, mm) for mm in MM_HALF]
        for g, (qi, mm) in enumerate(groups):
            q, n = (q8, q16)[qi], (255, 400)[qi]
            slots = [g + ROWS * j for j in range(4)] if w <= 8 else [4 * g + j for j in range(4)]
            counts = (mm - 1, mm, min(mm + 1, n), 0)
            for s, c in zip(slots[:3], counts):
                db[s] = prefix_with(q, c, w)
            expect.append(dict(edge=f"threshold {mm}, {'byte' if qi == 0 else '16-bit'} class: counts {counts} side by side",
                               query=qi, minwordmatches=mm, targets=dict(zip(slots, counts))))
        e255 = next(e for e in expect if e["query"] == 0 and e["minwordmatches"] == 255)
        expect.append(dict(edge="--minwordmatches 256 with 255 words: the threshold is 255, the byte is full",
                           query=0, minwordmatches=256, targets=e255["targets"]))
        for s in range(n_db):
            if db[s] is None:
                db[s] = zero_filler(rng, 30, w, qwords)
        queries = [q8, q16]
        if all(all(py_counts(db, queries[e["query"]], w)[t] == c for t, c in e["targets"].items()) for e in expect):
            return db, queries, opts, expect


# ---- 3. the selection kernel's threshold, ties and clamped bin ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def selection_edges(seed=303):
    """--maxaccepts 1 --maxrejects 1: a heap of 10.  expect[k]["top"] is the list the construction says must come out."""
    rng = random.Random(seed)
    w = 8
    opts = dict(wordlength=w, minwordmatches=12, maxaccepts=1, maxrejects=1)
    while True:
        avoid = set()

        def new_query(n):
            q = distinct_words_seq(rng, n, w, avoid)
            avoid.update(words_of(q, w))
            return q

        qa, qb, qc, qd, qe = new_query(100), new_query(120), new_query(400), new_query(400), new_query(255)
        items = []                                                   # (sequence, query, count)
        items += [(prefix_with(qa, 50, w), 0, 50) for _ in range(10)] + [(prefix_with(qa, c, w), 0, c) for c in range(20, 35)]
        tails = [0, 3, 3, 7, 0, 12, 5, 5, 1, 9, 3, 0, 7]
        items += [(prefix_with(qb, 60, w) + rnd(rng, t, "ACG"), 1, 60) for t in tails] + [(prefix_with(qb, 30, w), 1, 30) for _ in range(5)]
        items += [(prefix_with(qc, c, w), 2, c) for c in range(256, 270)]
        items += [(prefix_with(qd, 300, w) + rnd(rng, t, "ACG"), 3, 300) for t in tails + [2]]
        items += [(qe, 4, 255) for _ in range(13)]
        items += [(rnd(rng, rng.randint(100, 300)), None, 0) for _ in range(30)]
        rng.shuffle(items)
        db = [s for s, _, _ in items]
        queries = [qa, qb, qc, qd, qe]
        edges = ["exactly 10 targets at count 50 and 15 below: the threshold bin holds the heap exactly",
                 "13 targets tied at count 60 with mixed lengths and numbers: length, then number, decides the cut",
                 "16-bit class, 14 distinct counts 256..269 in the clamped bin: the bisection must land on 260",
                 "16-bit class, 14 targets all at 300: the bisection ends with all 14 in hand",
                 "byte class, 255 words, 13 exact copies: the clamped bin reached with counts of exactly 255"]
        expect = []
        for k in range(5):
            mine = sorted(((-c, len(s), t) for t, (s, qi, c) in enumerate(items) if qi == k))
            expect.append(dict(edge=edges[k], query=k, top=[(t, -c) for c, _, t in mine[:10]],
                               at_or_above_255=sum(1 for c, _, _ in mine if -c >= 255), env={}))
        expect.append(dict(expect[2], edge=edges[2] + ", record regions of 3 (VSX_KMER_CAP): the second pass", env={"VSX_KMER_CAP": "3"}))
        if all(py_candidates(db, queries[e["query"]], w, 12, 10) == e["top"] for e in expect):
            return db, queries, opts, expect


# ---- 4. buckets of one unit to several trips ------------------------------------------------------------------------------------------
TRIP_UNITS = (1, 2, 64, 65, 128, 129, 192, 193, 257)


@functools.lru_cache(maxsize=None)
def bucket_trips(seed=404, n_seq=6500):
    """one tile of sequences of 16 or 24 symbols, each two or three slots of eight: a marker word or ACG filler.  Marker M_U sits in
    exactly as many sequences as make its bucket U units long (found with the library's encoder).  Single-word queries stream one
    bucket of U units (T = ceil(U / 64) trips); a query of two markers back to back has them as its words 0 and 8, which one wave
    streams as one run: 40 + 40 units (the second bucket straddles the first trip's end) and 64 + 1."""
    w = 8
    opts = dict(wordlength=w, minwordmatches=1, maxaccepts=0, maxrejects=0)
    rng = random.Random(seed)
    by_counter = sorted(range(n_seq), key=counter_of)
    while True:
        used = set()
        slots = [[] for _ in range(n_seq)]
        wanted = [(f"M{u}", u) for u in TRIP_UNITS] + [("M40a", 40), ("M40b", 40)]
        markers, good = {}, True
        for name, units in sorted(wanted, key=lambda nu: -nu[1]):
            free = [s for s in by_counter if len(slots[s]) < 3]
            if units >= 40:
                rng.shuffle(free)                                     # spread over the tile: gaps of all sizes
            else:
                at = rng.randrange(len(free) - 40)
                free = free[at:at + 40]                               # neighbours in counter space: no hops to pay for
            lo, hi = 1, min(len(free), 15 * units)
            while lo < hi:                                            # the fewest holders that need `units` units
                mid = (lo + hi) // 2
                if pack_units([counter_of(s) for s in free[:mid]]) >= units:
                    hi = mid
                else:
                    lo = mid + 1
            if pack_units([counter_of(s) for s in free[:lo]]) != units:
                good = False
                break
            markers[name] = marker(rng, used)
            for s in free[:lo]:
                slots[s].append(markers[name])
        if not good:
            continue
        db = []
        for s in range(n_seq):
            total = max(len(slots[s]), 3 if rng.random() < 0.3 else 2)
            parts = slots[s] + [rnd(rng, 8, "ACG") for _ in range(total - len(slots[s]))]
            rng.shuffle(parts)
            db.append("".join(parts))
        queries, expect = [], []
        for u in TRIP_UNITS:
            expect.append(dict(edge=f"one bucket of {u} units: {-(-u // 64)} trips", query=len(queries), words=[markers[f"M{u}"]],
                               units=[u], trips=-(-u // 64)))
            queries.append(markers[f"M{u}"])
        for a, b in (("M40a", "M40b"), ("M64", "M1")):
            ua, ub = dict(wanted)[a], dict(wanted)[b]
            expect.append(dict(edge=f"words 0 and 8 of one wave: buckets of {ua} + {ub} units in one run", query=len(queries),
                               words=[markers[a], markers[b]], units=[ua, ub], trips=-(-(ua + ub) // 64)))
            queries.append(markers[a] + markers[b])
        if all([bucket_units(db, w, m) for m in e["words"]] == e["units"] for e in expect):
            return db, queries, opts, expect


@functools.lru_cache(maxsize=None)
def primer_set(seed=405, n_seq=33000, body=30, per_family=100, rate=0.04, minwordmatches=12, n_queries=12):
    """amplicon-like: every sequence starts with one 20-mer (13 words that every sequence holds: per full tile a bucket of
    ceil(32 630 / 15) = 2 176 units, 34 trips), family bodies follow; substitutions only, so all lengths are equal.  The queries
    are the primer and a mutated body of a database sequence, the tile's last and the next tile's first among them."""
    w = 8
    rng = random.Random(seed)
    opts = dict(wordlength=w, minwordmatches=minwordmatches, maxaccepts=1, maxrejects=32)
    primer = distinct_words_seq(rng, 13, w)
    anc = [rnd(rng, body) for _ in range(-(-n_seq // per_family))]
    db = [primer + substitute(rng, anc[i // per_family], rate) for i in range(n_seq)]
    picks = [0, per_family - 1, per_family, n_seq // 2, n_seq - 1]
    if n_seq > TILE_SEQS:
        picks += [TILE_SEQS - 1, TILE_SEQS, TILE_SEQS + 1]
    while len(picks) < n_queries:
        picks.append(rng.randrange(n_seq))
    queries = [primer + substitute(rng, db[i][len(primer):], rate / 2) for i in picks]
    tiles = -(-n_seq // TILE_SEQS)
    last = n_seq - (tiles - 1) * TILE_SEQS
    expect = [dict(edge=f"primer word {k} sits in every sequence: buckets of {[-(-(TILE_SEQS if t < tiles - 1 else last) // 15) for t in range(tiles)]} units",
                   query=0, word=primer[k:k + w], units=[-(-(TILE_SEQS if t < tiles - 1 else last) // 15) for t in range(tiles)])
              for k in range(13)]
    return db, queries, opts, expect


# ---- 5. gaps, hops and unit edges of the packed index ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gap_edges(seed=505):
    """32 640 sequences (one tile and ten): ACG filler, except that each marker word sits in the sequences that own a chosen set of
    counters.  expect[k]: the holders' sequence numbers, their counters (tile 0), the dummy hops the encoder needs between them."""
    w = 8
    opts = dict(wordlength=w, minwordmatches=1, maxaccepts=0, maxrejects=0)
    rng = random.Random(seed)
    n_seq = TILE_SEQS + 10
    patterns = [("a gap of exactly 255 from counter 0: one byte, no hop", [0, 255], 0),
                ("a gap of 256: one hop", [0, 256], 1),
                ("a gap of 257: one hop", [0, 257], 1),
                ("a gap of 252 * 4 + 1: four hops", [3, 3 + PERIOD * 4 + 1], 4),
                ("counters 250 and 252: either side of a dummy", [250, 252], 0),
                ("the tile's last counter 32 758 alone", [ROWS * PERIOD - 2], 0)]
    for k, n in enumerate((15, 16, 30, 31)):
        c0 = PERIOD * (10 + k) + 7
        patterns.append((f"{n} consecutive counters: {'a full unit' if n % 15 == 0 else 'a full unit and one more posting'}"
                         if n < 30 else f"{n} consecutive counters: {-(-n // 15)} units", list(range(c0, c0 + n)), 0))
    used = set()
    parts = [[] for _ in range(n_seq)]
    queries, expect = [], []
    for edge, counters, hops in patterns:
        m = marker(rng, used)
        hs = sorted(seq_of(c) for c in counters)
        for s in hs:
            parts[s].append(m)
        expect.append(dict(edge=edge, query=len(queries), word=m, holders=hs, counters=sorted(counters), hops=hops,
                           units=-(-(len(counters) + hops) // 15)))
        queries.append(m)
    m = marker(rng, used)
    for s in (TILE_SEQS - 1, TILE_SEQS):
        parts[s].append(m)
    expect.append(dict(edge="the tile's last sequence 32 629 (counter 32 758) and the next tile's first", query=len(queries), word=m,
                       holders=[TILE_SEQS - 1, TILE_SEQS], counters=[ROWS * PERIOD - 2], hops=0, units=1))
    queries.append(m)
    db = ["".join(p) if p else rnd(rng, 16, "ACG") for p in parts]
    assert all(holders(db, w, e["word"]) == e["holders"] for e in expect)        # (markers cannot arise by accident)
    return db, queries, opts, expect


# ---- 6. tagged postings: one bucket, many tags ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tag_collisions(w, seed=606):
    """word lengths 9..15 put a word into the bucket of its last eight symbols and carry the leading w - 8 as a tag.  For a suffix S
    the database holds X.S for every leading part X but one (`copies` sequences each), so the bucket of S mixes every tag (a sequence is one word long); the
    queries hold one X.S each -- the first, the last (its postings end the bucket), the absent one (nothing may count), some others --
    two of them back to back, and one as the head of a query of more than 255 words (16-bit counters).  Suffixes S4, S5, S8 have
    buckets of exactly 4, 5 and 8 postings (one full unit, one posting into the second, two full units)."""
    rng = random.Random(seed + w)
    x = w - 8
    opts = dict(wordlength=w, minwordmatches=1, maxaccepts=0, maxrejects=0)
    copies = {1: 101}.get(x, 2 if x <= 4 else 1)
    used = set()
    S = marker(rng, used)
    heads = ["".join("ACGT"[(v >> (2 * (x - 1 - k))) & 3] for k in range(x)) for v in range(4 ** x)]
    absent = heads[len(heads) // 2]
    db = [h + S for h in heads if h != absent for _ in range(copies)]
    small = {}
    for n in (4, 5, 8):
        Sn = marker(rng, used)
        h0, h1 = rng.sample(heads, 2)
        others = [h for h in heads if h not in (h0, h1)]
        hn = [h0, h1, h0] + [rng.choice(others) for _ in range(n - 3)]
        small[n] = (Sn, hn)
        db += [h + Sn for h in hn]
    long_tail = distinct_words_seq(rng, 300, w)
    db += [zero_filler(rng, 40, w, words_of(long_tail, w)) for _ in range(50)]
    rng.shuffle(db)
    queries, expect = [], []

    def add(edge, q, suffix, **more):
        expect.append(dict(edge=edge, query=len(queries), suffix=suffix, **more))
        queries.append(q)

    present = [h for h in heads if h != absent]
    add("the first tag of a mixed bucket", present[0] + S, S, matches=copies)
    add("the last tag of a mixed bucket: the matches end the bucket", present[-1] + S, S, matches=copies)
    add("the one leading part no sequence has: a bucket full of other tags and pads", absent + S, S, matches=0)
    for h in rng.sample(present, 3):
        add("a tag from the middle of a mixed bucket", h + S, S, matches=copies)
    a, b = rng.sample(present, 2)
    add("two words of one bucket in one query", a + S + b + S, S, matches=2 * copies)
    add("16-bit class (more than 255 words) on a mixed bucket", present[-1] + S + long_tail, S, matches=copies)
    for n, (Sn, hn) in small.items():
        add(f"a bucket of exactly {n} postings, the tag held twice", hn[0] + Sn, Sn, matches=2, postings=n)
        add(f"a bucket of exactly {n} postings, a tag held once", hn[1] + Sn, Sn, matches=1, postings=n)
    return db, queries, opts, expect


def tag_bucket(db, w, suffix):
    """the tagged index's bucket of an eight-symbol suffix: (leading part, sequence) of every word that ends in it"""
    post = _index(db, w)[1]
    return sorted((word[:w - 8], t) for word, ts in post.items() if word[w - 8:] == suffix for t in ts)
