"""-m gpu: the candidate-batch dispatch layer (include/vsx_search.h) against the reference CLI itself
(oracle/_ref/vsearch_ref: every translation unit of the reference compiled in place by oracle/Makefile,
SURVEY.md 8c level 2).  --usearch_global ... --userout is compared line for line: same hits, same order,
same %id, alignment length, mismatches, gap opens, raw score and CIGAR."""
import os
import random
import subprocess

import pytest

from tests import common
from tests.msa_data import cluster_input, random_cluster as _random_cluster

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "vsearch_ref")
FIELDS = ["query", "target", "id", "alnlen", "mism", "opens", "exts", "raw", "caln", "id0", "id1", "id2", "id3", "id4"]


def run_reference(tmp, db, qs, extra):
    dbf, qf, uf = os.path.join(tmp, "db.fa"), os.path.join(tmp, "q.fa"), os.path.join(tmp, "u.tsv")
    with open(dbf, "w") as f:
        f.write("".join(f">t{i}\n{s}\n" for i, s in enumerate(db)))
    with open(qf, "w") as f:
        f.write("".join(f">q{i}\n{s}\n" for i, s in enumerate(qs)))
    cmd = [REF_BIN, "--usearch_global", qf, "--db", dbf, "--qmask", "none", "--dbmask", "none", "--threads", "1",
           "--userout", uf, "--userfields", "+".join(FIELDS), "--quiet"] + extra
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return open(uf).read().splitlines()


CASES = [
    ("default_id90", dict(id=0.9), ["--id", "0.9"]),
    ("id97_maxaccepts4", dict(id=0.97, maxaccepts=4), ["--id", "0.97", "--maxaccepts", "4"]),
    ("id70_ma3_mr16", dict(id=0.7, maxaccepts=3, maxrejects=16), ["--id", "0.7", "--maxaccepts", "3", "--maxrejects", "16"]),
    ("id80_all", dict(id=0.8, maxaccepts=0, maxrejects=0), ["--id", "0.8", "--maxaccepts", "0", "--maxrejects", "0"]),
    ("iddef1_weak", dict(id=0.95, weak_id=0.8, iddef=1, maxaccepts=2), ["--id", "0.95", "--weak_id", "0.8", "--iddef", "1", "--maxaccepts", "2"]),
    ("filters", dict(id=0.85, maxaccepts=5, maxgaps=2, maxsubs=20, mincols=100, query_cov=0.5, maxrejects=64),
     ["--id", "0.85", "--maxaccepts", "5", "--maxgaps", "2", "--maxsubs", "20", "--mincols", "100", "--query_cov", "0.5", "--maxrejects", "64"]),
    ("word7", dict(id=0.9, wordlength=7, maxaccepts=2), ["--id", "0.9", "--wordlength", "7", "--maxaccepts", "2"]),
]


@pytest.mark.parametrize("name,opts,extra", CASES, ids=[c[0] for c in CASES])
def test_usearch_global_matches_reference_cli(gpu_required, tmp_path, name, opts, extra):
    if not os.path.exists(REF_BIN):
        pytest.fail("oracle/_ref/vsearch_ref missing: run `make -C oracle ref_full` in the build container "
                    "(it travels to the GPU box with the repo)")
    from vsearch_amd import Aligner, SearchSession
    rng = random.Random(hash(name) & 0xffff)
    db, fam = common.family_db(rng, 25, 12, 420, div=0.06)
    db += [common.rnd_seq(rng, rng.randint(200, 500)) for _ in range(40)]            # unrelated decoys
    db += [common.mutate(rng, db[3], 0.02, "ACGTN") for _ in range(4)]               # N-containing relatives
    qs, _ = common.queries_from_db(rng, db, 120, 160)
    qs += [common.mutate(rng, db[rng.randrange(len(db))], 0.05) for _ in range(30)]  # full-length queries
    qs += [common.rnd_seq(rng, 120), "ACGT" * 30, common.mutate(rng, db[7], 0.04, "ACGTRYN")]
    exp = run_reference(str(tmp_path), db, qs, extra)
    with Aligner() as al:
        ss = SearchSession(al, db, **opts)
        got = ss.userout(qs, fields=FIELDS)
        stats = dict(ss.stats)
    assert len(exp) > 50
    assert got == exp, _first_diff(got, exp)
    assert stats["pairs_aligned"] > 0 and stats["sentinel_pairs"] == 0


def _first_diff(got, exp):
    for i, (a, b) in enumerate(zip(got, exp)):
        if a != b:
            return f"line {i}:\n got {a}\n exp {b}"
    return f"length {len(got)} vs {len(exp)}"


def test_candidate_order_matches_reference_hits(gpu_required, tmp_path):
    """with --maxaccepts 0 --maxrejects 0 --id 0 every candidate is aligned and reported: the reference's
    reported target SET per query must equal our candidate list (search_topscores + minheap order)."""
    if not os.path.exists(REF_BIN):
        pytest.fail("oracle/_ref/vsearch_ref missing")
    from vsearch_amd import Aligner, SearchSession
    rng = random.Random(11)
    db, fam = common.family_db(rng, 8, 6, 300, div=0.1)
    qs, _ = common.queries_from_db(rng, db, 12, 120)
    exp = run_reference(str(tmp_path), db, qs, ["--id", "0.0", "--maxaccepts", "0", "--maxrejects", "0"])
    per_q = {}
    for line in exp:
        c = line.split("\t")
        per_q.setdefault(c[0], set()).add(c[1])
    with Aligner() as al:
        ss = SearchSession(al, db, id=0.0, maxaccepts=0, maxrejects=0)
        for i, q in enumerate(qs):
            cands = ss.candidates(q)
            assert {f"t{t}" for t, _ in cands} == per_q.get(f"q{i}", set()), i
            assert all(cands[k][1] >= cands[k + 1][1] for k in range(len(cands) - 1))


def test_sentinel_pairs_take_the_fallback(gpu_required, tmp_path):
    """pairs the 16-bit aligner refuses (Q*D > 25e6 here) must come back through the linear-memory fallback
    with the reference's hit fields (searchcore.cpp:806-832)"""
    if not os.path.exists(REF_BIN):
        pytest.fail("oracle/_ref/vsearch_ref missing")
    from vsearch_amd import Aligner, SearchSession
    rng = random.Random(21)
    anc = common.rnd_seq(rng, 9000)
    db = [common.mutate(rng, anc, 0.03) for _ in range(3)] + [common.rnd_seq(rng, 800) for _ in range(5)]
    qs = [common.mutate(rng, anc[1000:4200], 0.02), common.mutate(rng, db[4], 0.05)]
    exp = run_reference(str(tmp_path), db, qs, ["--id", "0.8", "--maxaccepts", "3"])
    with Aligner() as al:
        ss = SearchSession(al, db, id=0.8, maxaccepts=3)
        got = ss.userout(qs, fields=FIELDS)
        assert ss.stats["sentinel_pairs"] >= 3
    assert got == exp, _first_diff(got, exp)


def run_reference_allpairs(tmp, db, extra):
    dbf, uf = os.path.join(tmp, "a.fa"), os.path.join(tmp, "ua.tsv")
    with open(dbf, "w") as f:
        f.write("".join(f">t{i}\n{s}\n" for i, s in enumerate(db)))
    cmd = [REF_BIN, "--allpairs_global", dbf, "--qmask", "none", "--threads", "1",
           "--userout", uf, "--userfields", "+".join(FIELDS), "--quiet"] + extra
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return open(uf).read().splitlines()


@pytest.mark.parametrize("name,acceptall,opts,extra", [
    ("id80", False, dict(id=0.8), ["--id", "0.8"]),
    ("acceptall", True, dict(id=0.0), ["--acceptall"]),
    ("id75_filters", False, dict(id=0.75, maxgaps=12, minsl=0.98), ["--id", "0.75", "--maxgaps", "12", "--minsl", "0.98"]),
])
def test_allpairs_global_matches_reference_cli(gpu_required, tmp_path, name, acceptall, opts, extra):
    """--allpairs_global (SURVEY config 4 shape: dense all-vs-all, no k-mer heuristic)"""
    if not os.path.exists(REF_BIN):
        pytest.fail("oracle/_ref/vsearch_ref missing")
    from vsearch_amd import Aligner, SearchSession
    rng = random.Random(31)
    db, fam = common.family_db(rng, 6, 9, 400, div=0.1)
    db += [common.rnd_seq(rng, rng.randint(100, 450)) for _ in range(6)]
    exp = run_reference_allpairs(str(tmp_path), db, extra)
    with Aligner() as al:
        ss = SearchSession(al, db, **opts)
        hits = []
        for first in range(0, len(db), 16):            # walk the database in blocks, as a caller would
            hits += ss.allpairs(first, min(16, len(db) - first), acceptall=acceptall)
        names = [f"t{i}" for i in range(len(db))]
        got = ss.userout(db, qnames=names, tnames=names, fields=FIELDS, hits=hits)
    assert len(exp) > 10
    assert got == exp, _first_diff(got, exp)


def test_allpairs_runtime_overflow_pairs_take_the_fallback(gpu_required, tmp_path):
    """A pair whose 16-bit DP overflows ON THE GPU (a 250-nt fragment against its 40-kb source: the terminal gap alone costs
    more than SHRT_MIN, align_simd.cpp:1774-1786) must still be reported: the ranked device path lists it as undecided and
    vsx_allpairs_rows recovers it through the linear-memory fallback, as the reference does (searchcore.cpp:806-832).
    ADVICE r02 (high): such pairs used to vanish from the ranked path."""
    if not os.path.exists(REF_BIN):
        pytest.fail("oracle/_ref/vsearch_ref missing")
    from vsearch_amd import Aligner, SearchSession
    rng = random.Random(77)
    long_a = common.rnd_seq(rng, 40000)
    frags = [common.mutate(rng, long_a[o:o + 250], 0.03) for o in (100, 9000, 20000, 39700)]
    db, fam = common.family_db(rng, 3, 5, 300, div=0.08)
    db = frags[:2] + db + [long_a] + frags[2:]
    exp = run_reference_allpairs(str(tmp_path), db, ["--id", "0.8"])
    with Aligner() as al:
        ss = SearchSession(al, db, id=0.8)
        hits = ss.allpairs(0, len(db), acceptall=False)
        names = [f"t{i}" for i in range(len(db))]
        got = ss.userout(db, qnames=names, tnames=names, fields=FIELDS, hits=hits)
    li = db.index(long_a)
    assert sum(1 for l in exp if f"t{li}" in l.split("\t")[:2]) == 4          # the four fragment-vs-source hits exist in the reference
    assert got == exp, _first_diff(got, exp)


def run_reference_cluster(tmp, seqs, names, extra, threads=1):
    f_in, f_uc = os.path.join(tmp, "c.fa"), os.path.join(tmp, "c.uc")
    with open(f_in, "w") as f:
        f.write("".join(f">{n}\n{s}\n" for n, s in zip(names, seqs)))
    cmd = [REF_BIN, "--cluster_fast", f_in, "--qmask", "none", "--threads", str(threads), "--uc", f_uc, "--quiet"] + extra
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return open(f_uc).read().splitlines()


@pytest.mark.parametrize("name,opts,extra,round_size", [
    ("id97_round7", dict(id=0.97, maxrejects=8), ["--id", "0.97"], 7),
    ("id97_round64", dict(id=0.97, maxrejects=8), ["--id", "0.97"], 64),
    ("id90_one_round", dict(id=0.9, maxrejects=8), ["--id", "0.9"], 100000),
    ("id94_ma3", dict(id=0.94, maxrejects=8, maxaccepts=3), ["--id", "0.94", "--maxaccepts", "3"], 50),
])
def test_cluster_fast_matches_reference_cli(gpu_required, tmp_path, name, opts, extra, round_size):
    """--cluster_fast --uc (SURVEY config 3 shape: amplicon families at 2 % divergence): S/H/C records byte-identical,
    for several round sizes (the intra-round fix-up, SURVEY 8a row 14, must make the result round-independent)."""
    if not os.path.exists(REF_BIN):
        pytest.fail("oracle/_ref/vsearch_ref missing")
    from vsearch_amd import Aligner, SearchSession
    rng = random.Random(5)
    seqs = []
    for f in range(30):
        anc = common.rnd_seq(rng, rng.randint(280, 320))
        for _ in range(rng.randint(2, 14)):
            seqs.append(common.mutate(rng, anc, rng.choice([0.01, 0.02, 0.04])))
    seqs += [common.rnd_seq(rng, rng.randint(250, 330)) for _ in range(20)]
    seqs += [seqs[3], seqs[3][:-2]]                                           # duplicates / near-duplicates
    rng.shuffle(seqs)
    names = [f"s{i:04d}" for i in range(len(seqs))]
    # Database::sortbylength (core/db.cpp:433-450): length desc, abundance, label
    order = sorted(range(len(seqs)), key=lambda i: (-len(seqs[i]), names[i]))
    sseqs, snames = [seqs[i] for i in order], [names[i] for i in order]
    exp = run_reference_cluster(str(tmp_path), seqs, names, extra)
    with Aligner() as al:
        ss = SearchSession(al, sseqs, **opts)              # cluster_fast default: --maxrejects 8 (cli.cc:4163-4167)
        got = ss.uc_lines(snames, round=round_size)
    assert sum(1 for l in exp if l[0] == "H") > 50
    assert got == exp, _first_diff(got, exp)


def _wrap(seq, width=80):
    return [seq[i:i + width] for i in range(0, len(seq), width)] or [""]


@pytest.mark.parametrize("device_msa", [False, True])
def test_cluster_msa_consensus_profile_match_reference_cli(gpu_required, tmp_path, device_msa):
    """--cluster_fast --msaout --consout --profile: the CIGARs we store per member must drive the reference's star MSA,
    consensus and profile to byte-identical files (the consumer of the CIGAR contract) -- with the MSA
    itself on the host (vsx_msa) and on the device (vsx_msa_device_batch, all clusters in one pass)."""
    if not os.path.exists(REF_BIN):
        pytest.fail("oracle/_ref/vsearch_ref missing")
    from vsearch_amd import Aligner, SearchSession, msa_batch
    seqs, names = cluster_input()
    order = sorted(range(len(seqs)), key=lambda i: (-len(seqs[i]), names[i]))
    sseqs, snames = [seqs[i] for i in order], [names[i] for i in order]
    tmp = str(tmp_path)
    f_in = os.path.join(tmp, "m.fa")
    with open(f_in, "w") as f:
        f.write("".join(f">{n}\n{s}\n" for n, s in zip(names, seqs)))
    p = subprocess.run([REF_BIN, "--cluster_fast", f_in, "--id", "0.85", "--qmask", "none", "--threads", "1", "--quiet",
                        "--msaout", tmp + "/m.msa", "--consout", tmp + "/m.cons", "--profile", tmp + "/m.prof"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    with Aligner() as al:
        ss = SearchSession(al, sseqs, id=0.85, maxrejects=8)
        cno, per, ncl = ss.cluster_fast(round=16)
        members = [[] for _ in range(ncl)]
        for s, c in enumerate(cno):
            members[c].append(s)                       # ascending seqno: the centroid comes first
        assert all(per[m[0]] is None for m in members)
        results = msa_batch([[sseqs[s] for s in m] for m in members],
                            [[None] + [per[s]["cigar"] for s in m[1:]] for m in members], None, al if device_msa else None)
    msa_lines, cons_lines, prof_lines = [], [], []
    for c in range(ncl):
        m = members[c]
        res = results[c]
        msa_lines.append("")
        for k, s in enumerate(m):
            msa_lines.append(">" + ("*" if k == 0 else "") + snames[s])
            msa_lines += _wrap(res["rows"][k])
        msa_lines.append(">consensus")
        msa_lines += _wrap(res["rows"][-1])
        cons_lines.append(f">centroid={snames[m[0]]};seqs={len(m)}")
        cons_lines += _wrap(res["consensus"])
        prof_lines.append(f">centroid={snames[m[0]]};seqs={len(m)}")
        for i, (ch, pr) in enumerate(zip(res["rows"][-1], res["profile"])):
            prof_lines.append("\t".join([str(i), ch] + [str(pr[k]) for k in (0, 1, 2, 3, 5, 4)]))
        prof_lines.append("")
    assert msa_lines == open(tmp + "/m.msa").read().splitlines()
    assert cons_lines == open(tmp + "/m.cons").read().splitlines()
    assert prof_lines == open(tmp + "/m.prof").read().splitlines()


# ---- k-mer candidate counting on the device (vsx_kmer.hip) vs the host restatement of search_topscores ----
def _kmer_case(rng, n_fam, per_fam, L, nq, qlen, iupac=0.0, **opts):
    db, _ = common.family_db(rng, n_fam, per_fam, L, div=0.08)
    if iupac:
        db = ["".join((rng.choice("RYSWKMBDHVN") if rng.random() < iupac else ch) for ch in s) for s in db]
    db += ["", "A", "ACGTACG", common.rnd_seq(rng, 9), common.rnd_seq(rng, 40)]            # shorter than a word / barely longer
    qs, _ = common.queries_from_db(rng, db[:n_fam * per_fam], nq, qlen)
    qs += ["", "ACG", common.rnd_seq(rng, 8), "N" * 50, common.rnd_seq(rng, 700)]
    return db, qs, opts


@pytest.mark.gpu
@pytest.mark.parametrize("case", [
    dict(seed=1, n_fam=20, per_fam=8, L=300, nq=40, qlen=150),
    dict(seed=2, n_fam=10, per_fam=10, L=400, nq=30, qlen=200, iupac=0.01),
    dict(seed=3, n_fam=12, per_fam=6, L=250, nq=25, qlen=120, wordlength=5),
    dict(seed=4, n_fam=12, per_fam=6, L=250, nq=25, qlen=120, wordlength=3, minwordmatches=2),
    dict(seed=5, n_fam=15, per_fam=8, L=300, nq=30, qlen=100, maxaccepts=3, maxrejects=5),
    dict(seed=6, n_fam=6, per_fam=6, L=200, nq=10, qlen=80, minwordmatches=0),            # every sequence qualifies: host path
    # word lengths 9..15 (r03): tagged postings -- buckets by a word's last eight symbols, the rest rides along as a tag
    dict(seed=7, n_fam=14, per_fam=8, L=300, nq=30, qlen=150, wordlength=9),
    dict(seed=8, n_fam=14, per_fam=8, L=300, nq=30, qlen=150, wordlength=10, iupac=0.01),
    dict(seed=9, n_fam=14, per_fam=8, L=300, nq=30, qlen=150, wordlength=12, minwordmatches=3),
    dict(seed=10, n_fam=14, per_fam=8, L=300, nq=30, qlen=150, wordlength=13, minwordmatches=2),   # (the host checker needs 8 B x 4^w: 15 is left to the CLI test below)
    dict(seed=11, n_fam=8, per_fam=5, L=420, nq=20, qlen=400, wordlength=11, minwordmatches=4),   # > 255 words: 16-bit counters
])
def test_device_kmer_candidates_equal_host(gpu_required, case):
    from vsearch_amd import Aligner, SearchSession
    case = dict(case)
    rng = random.Random(case.pop("seed"))
    db, qs, opts = _kmer_case(rng, **case)
    with Aligner() as al:
        ss = SearchSession(al, db, id=0.5, **opts)
        host = ss.candidates_batch(qs, device=False)
        dev = ss.candidates_batch(qs, device=True)
        assert ss.kmer_stats["index_postings"] > 0
    assert len(host) == len(dev) == len(qs)
    assert sum(len(h) for h in host) > 0
    for k, (h, d) in enumerate(zip(host, dev)):
        assert h == d, (k, h[:5], d[:5])


@pytest.mark.gpu
def test_device_kmer_multi_tile(gpu_required):
    """more than 2^15 sequences: several counter tiles per query, candidates from every tile"""
    from vsearch_amd import Aligner, SearchSession
    rng = random.Random(77)
    anc = [common.rnd_seq(rng, 120) for _ in range(700)]
    db = [common.mutate(rng, anc[i % 700], 0.05) for i in range(70_000)]
    # (32 630 sequences per tile in the packed index, 2^15 in the 16-bit one: both kinds of boundary)
    qs = [common.mutate(rng, db[i], 0.02) for i in (0, 1, 129, 130, 32629, 32630, 32631, 32767, 32768, 40000, 65259, 65260, 65535, 65536, 69999)]
    with Aligner() as al:
        ss = SearchSession(al, db, id=0.5, maxaccepts=2, maxrejects=200)
        host = ss.candidates_batch(qs, device=False)
        dev = ss.candidates_batch(qs, device=True)
    assert host == dev
    assert all(len(h) >= 50 for h in host)
    assert any(t >= 65536 for h in host for t, _ in h) and any(t < 32768 for h in host for t, _ in h)


@pytest.mark.gpu
def test_device_kmer_packed_index_on_clustered_and_sparse_postings(gpu_required):
    """The packed index (sorted one-byte gaps, dummy counters for gaps above 255 and for the tail of a unit): families stored as
    contiguous runs of the database (dense stretches of a word's postings, nothing in between) and words that occur in a handful
    of far-apart sequences only (every gap needs hops) must count exactly like the host index."""
    from vsearch_amd import Aligner, SearchSession
    rng = random.Random(91)
    anc = [common.rnd_seq(rng, 110) for _ in range(350)]
    db = [common.mutate(rng, anc[i // 100], 0.03) for i in range(35_000)]          # 350 runs of 100 neighbours, two tiles
    rare = common.rnd_seq(rng, 110)
    for i in (5, 4000, 17000, 32629, 32630, 34999):                                  # six far-apart copies of one sequence
        db[i] = common.mutate(rng, rare, 0.01)
    qs = [common.mutate(rng, db[i], 0.02) for i in (0, 99, 100, 5, 17000, 32629, 32630, 34999, 20050)]
    with Aligner() as al:
        ss = SearchSession(al, db, id=0.5, maxaccepts=2, maxrejects=150)
        host = ss.candidates_batch(qs, device=False)
        dev = ss.candidates_batch(qs, device=True)
    assert host == dev
    assert all(len(h) >= 6 for h in host)


def test_cluster_fast_members_without_words_take_the_host_index(gpu_required, tmp_path):
    """Sequences the device counters cannot serve -- shorter than a word, or all N: min(minwordmatches, 0 words) = 0, every centroid
    is a candidate (searchcore.cpp:283-288) -- are ranked on the host against the growing centroid index, which since r03 is only
    caught up with the centroids when such a member turns up.  Several of them, spread over several rounds, among ordinary families:
    --uc byte-identical to the reference CLI."""
    if not os.path.exists(REF_BIN):
        pytest.fail("oracle/_ref/vsearch_ref missing")
    from vsearch_amd import Aligner, SearchSession
    rng = random.Random(15)
    seqs = []
    for f in range(12):
        anc = common.rnd_seq(rng, rng.randint(60, 90))
        for _ in range(rng.randint(2, 6)):
            seqs.append(common.mutate(rng, anc, 0.02))
    seqs += ["ACGTAC", "ACGTACG", "N" * 40, "ACGTA", "NNNNACGTNNNN", "ACGTAC", "TTGCA"]
    rng.shuffle(seqs)
    names = [f"s{i:04d}" for i in range(len(seqs))]
    order = sorted(range(len(seqs)), key=lambda i: (-len(seqs[i]), names[i]))
    sseqs, snames = [seqs[i] for i in order], [names[i] for i in order]
    exp = run_reference_cluster(str(tmp_path), seqs, names, ["--id", "0.9", "--minseqlength", "1"])
    for round_size in (5, 1000):
        with Aligner() as al:
            ss = SearchSession(al, sseqs, id=0.9, maxrejects=8)
            got = ss.uc_lines(snames, round=round_size)
        assert got == exp, (round_size, _first_diff(got, exp))


@pytest.mark.gpu
def test_device_kmer_long_words_multi_tile_and_repeats(gpu_required):
    """tagged index (word length 12) over more than 2^15 sequences, with sequences that repeat their words many times (a word counts
    once per sequence: unique_count, core/unique.cpp:155-352 -- the build dedups by sorting each tile's keys) and lower-case
    (soft-masked) stretches"""
    from vsearch_amd import Aligner, SearchSession
    rng = random.Random(78)
    anc = [common.rnd_seq(rng, 130) for _ in range(500)]
    db = [common.mutate(rng, anc[i % 500], 0.04) for i in range(40_000)]
    rep = common.rnd_seq(rng, 40)
    db[5] = rep * 6                                       # every word of `rep` six times
    db[33000] = rep * 3 + common.rnd_seq(rng, 50)
    db[100] = db[100][:40] + db[100][40:90].lower() + db[100][90:]
    qs = [common.mutate(rng, db[i], 0.02) for i in (0, 5, 100, 32767, 32768, 33000, 39999)] + [rep * 2]
    with Aligner() as al:
        ss = SearchSession(al, db, id=0.5, maxaccepts=2, maxrejects=100, wordlength=12, minwordmatches=3, soft_mask=1)
        host = ss.candidates_batch(qs, device=False)
        dev = ss.candidates_batch(qs, device=True)
    assert host == dev
    assert any(t >= 32768 for h in host for t, _ in h) and any(t < 32768 for h in host for t, _ in h)
    assert len(host[-1]) >= 2 and {5, 33000} <= {t for t, _ in host[-1]}


@pytest.mark.parametrize("wl", [9, 12, 15])
def test_usearch_global_long_words_match_reference_cli(gpu_required, tmp_path, wl):
    """--wordlength 9..15 end to end against the reference CLI (the device k-mer path serves them now: VERDICT r02 missing #2)"""
    if not os.path.exists(REF_BIN):
        pytest.fail("oracle/_ref/vsearch_ref missing")
    from vsearch_amd import Aligner, SearchSession
    rng = random.Random(90 + wl)
    db, fam = common.family_db(rng, 12, 8, 350, div=0.06)
    db += [common.rnd_seq(rng, 300) for _ in range(10)]
    qs, src = common.queries_from_db(rng, db, 40, 180)
    exp = run_reference(str(tmp_path), db, qs, ["--id", "0.8", "--maxaccepts", "3", "--wordlength", str(wl)])
    with Aligner() as al:
        ss = SearchSession(al, db, id=0.8, maxaccepts=3, wordlength=wl)
        got = ss.userout(qs, fields=FIELDS)
    assert len(exp) > 30
    assert got == exp, _first_diff(got, exp)


@pytest.mark.gpu
def test_device_kmer_region_overflow_second_pass(gpu_required, monkeypatch):
    """a record region smaller than a query's candidate count must trigger the exact-size second pass"""
    from vsearch_amd import Aligner, SearchSession
    rng = random.Random(5)
    db, _ = common.family_db(rng, 6, 30, 300, div=0.05)
    qs, _ = common.queries_from_db(rng, db, 20, 150)
    with Aligner() as al:
        ss = SearchSession(al, db, id=0.5, maxaccepts=4, maxrejects=16)
        host = ss.candidates_batch(qs, device=False)
        monkeypatch.setenv("VSX_KMER_CAP", "3")
        dev = ss.candidates_batch(qs, device=True)
    assert host == dev and max(len(h) for h in host) > 3


@pytest.mark.gpu
def test_device_kmer_sliced_passes_equal_one_pass(gpu_required, monkeypatch):
    """the counting scratch is bounded -- a batch whose per-(query, tile) regions exceed the budget runs as several
    passes over slices of its queries.  With the budget forced down (64 queries per pass; mixed 8-bit / 16-bit counter classes,
    several tiles, a forced second pass on top) the candidate lists must equal the host restatement's"""
    from vsearch_amd import Aligner, SearchSession
    rng = random.Random(6)
    db, _ = common.family_db(rng, 10, 20, 320, div=0.05)
    qs, _ = common.queries_from_db(rng, db, 150, 150)
    long_qs, _ = common.queries_from_db(rng, db, 50, 300)          # > 255 unique words: the 16-bit counter class
    qs = qs[:70] + long_qs + qs[70:]
    with Aligner() as al:
        ss = SearchSession(al, db, id=0.5, maxaccepts=4, maxrejects=16)
        host = ss.candidates_batch(qs, device=False)
        whole = ss.candidates_batch(qs, device=True)
        monkeypatch.setenv("VSX_KMER_SCRATCH_BYTES", "65536")
        sliced = ss.candidates_batch(qs, device=True)
        monkeypatch.setenv("VSX_KMER_CAP", "3")
        sliced2 = ss.candidates_batch(qs, device=True)
    assert host == whole == sliced == sliced2 and max(len(h) for h in host) > 3


def test_infinite_gap_penalties_match_reference_cli(gpu_required, tmp_path):
    """--gapext "2I/*E": terminal gaps longer than one are forbidden (cli.cc:203-228, searchcore.cpp:621-660); every pair
    takes the linear-memory fallback (search16 refuses penalties beyond the 16-bit range, align_simd.cpp:1463-1479)"""
    if not os.path.exists(REF_BIN):
        pytest.fail("oracle/_ref/vsearch_ref missing")
    from vsearch_amd import Aligner, SearchSession
    rng = random.Random(4242)
    db, _ = common.family_db(rng, 6, 6, 220, div=0.05)
    qs = [common.mutate(rng, db[rng.randrange(len(db))], 0.04) for _ in range(25)]
    qs += [db[3][2:], db[8][:-3], "A" + db[11], db[20][1:-1]]                       # terminal gaps of 2, 3, 1, 1+1
    exp = run_reference(str(tmp_path), db, qs, ["--id", "0.8", "--maxaccepts", "3", "--gapext", "2I/*E"])
    INF = 2 ** 31 - 1
    # post-fixup values (vsearch.cc:250-259): open -= extension
    scoring = (2, -4, 2 - INF, 2 - INF, 18, 18, 2 - INF, 2 - INF, INF, INF, 2, 2, INF, INF)
    mask = (1 << 6) | (1 << 7) | (1 << 10) | (1 << 11)
    with Aligner(scoring=scoring) as al:
        ss = SearchSession(al, db, id=0.8, maxaccepts=3, gap_infinite=mask)
        got = ss.userout(qs, fields=FIELDS)
        stats = dict(ss.stats)
    assert len(exp) > 10
    assert got == exp, _first_diff(got, exp)
    assert stats["sentinel_pairs"] > 0 and stats["pairs_aligned"] > 0


def test_strand_both_matches_reference_cli(gpu_required, tmp_path):
    """--strand both: reverse-complemented queries are searched too and the hits of both strands are joined"""
    if not os.path.exists(REF_BIN):
        pytest.fail("oracle/_ref/vsearch_ref missing")
    from vsearch_amd import Aligner, SearchSession
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "R": "Y", "Y": "R", "N": "N", "K": "M", "M": "K"}
    rng = random.Random(606)
    db, _ = common.family_db(rng, 10, 6, 300, div=0.06)
    qs, _ = common.queries_from_db(rng, db, 40, 150)
    for k in range(0, len(qs), 2):                                    # every other query is given on the minus strand
        qs[k] = "".join(comp[c] for c in reversed(qs[k]))
    qs.append(common.mutate(rng, db[4], 0.03, "ACGTRYN"))
    flds = FIELDS + ["qstrand"]
    dbf, qf, uf = str(tmp_path / "db.fa"), str(tmp_path / "q.fa"), str(tmp_path / "u.tsv")
    with open(dbf, "w") as f:
        f.write("".join(f">t{i}\n{s}\n" for i, s in enumerate(db)))
    with open(qf, "w") as f:
        f.write("".join(f">q{i}\n{s}\n" for i, s in enumerate(qs)))
    p = subprocess.run([REF_BIN, "--usearch_global", qf, "--db", dbf, "--qmask", "none", "--dbmask", "none", "--threads", "1",
                        "--userout", uf, "--userfields", "+".join(flds), "--quiet", "--id", "0.8", "--maxaccepts", "2",
                        "--strand", "both"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    exp = open(uf).read().splitlines()
    with Aligner() as al:
        ss = SearchSession(al, db, id=0.8, maxaccepts=2, strand_both=1)
        got = ss.userout(qs, fields=flds)
    assert sum(1 for l in exp if l.endswith("-")) > 10 and sum(1 for l in exp if l.endswith("+")) > 10
    assert got == exp, _first_diff(got, exp)


@pytest.mark.parametrize("extra,opts", [
    (["--id", "0.5", "--maxaccepts", "1", "--maxrejects", "32", "--minwordmatches", "0"], dict(id=0.5, maxaccepts=1, maxrejects=32, minwordmatches=0)),
    (["--id", "0.8", "--maxaccepts", "2", "--weak_id", "0.5"], dict(id=0.8, maxaccepts=2, weak_id=0.5)),
])
def test_strand_both_edge_cases_match_reference_cli(gpu_required, tmp_path, extra, opts):
    """found by oracle/soak_search.py: (1) queries the device counters cannot serve (--minwordmatches 0, queries without a single
    word) take the host restatement, which reads the minus strand as TEXT -- it has to exist then; (2) a query that hits one target
    with the same identity on both strands (its own reverse complement) ties in hit_compare_byid: the reference's qsort (glibc's
    merge sort) keeps the plus-strand hit first"""
    if not os.path.exists(REF_BIN):
        pytest.fail("oracle/_ref/vsearch_ref missing")
    from vsearch_amd import Aligner, SearchSession
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    rc = lambda x: "".join(comp[c] for c in reversed(x))
    rng = random.Random(515)
    db, _ = common.family_db(rng, 12, 5, 260, div=0.06)
    halves = [common.rnd_seq(rng, 90) for _ in range(6)]
    db += [h + rc(h) for h in halves]                                   # reverse-palindromic targets: both strands align alike
    qs, _ = common.queries_from_db(rng, db[:60], 50, 140)
    for k in range(0, len(qs), 2):
        qs[k] = rc(qs[k])
    qs += [h + rc(h) for h in halves[:4]] + [common.mutate(rng, halves[4] + rc(halves[4]), 0.03)]
    qs += ["ACG", "ACGTAC", "T" * 7]                                    # shorter than a word: no k-mers at all
    flds = FIELDS + ["qstrand"]
    dbf, qf, uf = str(tmp_path / "db.fa"), str(tmp_path / "q.fa"), str(tmp_path / "u.tsv")
    with open(dbf, "w") as f:
        f.write("".join(f">t{i}\n{s}\n" for i, s in enumerate(db)))
    with open(qf, "w") as f:
        f.write("".join(f">q{i}\n{s}\n" for i, s in enumerate(qs)))
    p = subprocess.run([REF_BIN, "--usearch_global", qf, "--db", dbf, "--qmask", "none", "--dbmask", "none", "--threads", "1",
                        "--userout", uf, "--userfields", "+".join(flds), "--quiet", "--strand", "both"] + extra, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    exp = open(uf).read().splitlines()
    with Aligner() as al:
        ss = SearchSession(al, db, strand_both=1, **opts)
        got = ss.userout(qs, fields=flds)
    assert sum(1 for l in exp if l.endswith("-")) > 10
    assert got == exp, _first_diff(got, exp)
    # the tie really occurs: some query reports the same target and identity on both strands
    keys = [tuple(l.split("\t")[:3]) for l in exp]
    assert len(keys) > len(set(keys)) or "weak_id" not in opts


def test_msa_device_equals_host(gpu_required):
    """vsx_msa_device_batch == vsx_msa (the host restatement of core/msa.cpp that the reference-CLI test pins), byte for byte:
    rows, consensus row with its '+' censoring, consensus sequence, 64-bit profile -- over IUPAC / lower-case / uncounted symbols,
    abundances (large and zero), terminal insertions, a 9000-member cluster (several row tiles), singletons and empty members."""
    from vsearch_amd import Aligner, msa_batch
    rng = random.Random(5)
    cl_s, cl_c, cl_a = [], [], []
    for k in range(40):
        n = rng.choice([1, 1, 2, 3, 8, 30, 200])
        alpha = rng.choice(["ACGT", "ACGTacgtNRYn", "ACGTUX*-"])
        s, c = _random_cluster(rng, n, rng.choice([1, 7, 64, 65, 255, 256, 257, 400]), alpha, long_ins=(k % 5 == 0))
        cl_s.append(s); cl_c.append(c)
        cl_a.append([rng.choice([0, 1, 1, 3, 2 ** 40 + 7]) for _ in s])
    s, c = _random_cluster(rng, 9000, 300, "ACGT")
    cl_s.append(s); cl_c.append(c); cl_a.append([rng.randint(0, 5) for _ in s])
    cl_s.append(["ACGT", "", "ACGT"]); cl_c.append([None, "4I", "4M"]); cl_a.append([0, 0, 0])      # empty member, all-zero columns
    host = msa_batch(cl_s, cl_c, cl_a, None)
    with Aligner() as al:
        dev = msa_batch(cl_s, cl_c, cl_a, al)
        dev1 = msa_batch(cl_s[:3], cl_c[:3], None, al)
    assert len(dev) == len(host)
    for k, (d, h) in enumerate(zip(dev, host)):
        assert d["rows"] == h["rows"], k
        assert d["consensus"] == h["consensus"], k
        assert d["profile"] == h["profile"], k
    assert dev1 == msa_batch(cl_s[:3], cl_c[:3], None, None)
    assert host[-1]["consensus"] == "----"              # the reference appends the '-' of an all-zero column (msa.cpp:474-483)


def test_msa_device_rejects_bad_cigars(gpu_required):
    from vsearch_amd import Aligner, msa
    from vsearch_amd._lib import VsxError
    with Aligner() as al:
        for seqs, cig in [(["ACGT", "ACG"], [None, "4M"]), (["ACGT", "ACGT"], [None, "3M"]), (["ACGT", "ACGTA"], [None, "5M"]),
                          (["ACGT", "ACGTAA"], [None, "4MDD"])]:
            with pytest.raises(VsxError):
                msa(seqs, cig, aligner=al)


def test_search_window_pipeline_equals_single_thread(gpu_required):
    """vsx_search_batch runs the k-mer stage of window i+1 on a producer thread while window i is aligned; with the window
    forced down to 5 queries the reference-CLI comparisons (userout byte-identical, both strands, '*' penalties) must still hold"""
    import sys
    e = dict(os.environ)
    e["VSX_SEARCH_WINDOW"] = "5"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_search.py"), "-x", "-q",
                        "-k", "usearch_global or strand_both or infinite_gap or candidate_order or sentinel_pairs"], env=e, capture_output=True, text=True, timeout=900, cwd=root)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert " passed" in p.stdout


def test_search_graded_windows_equal_one_window(gpu_required):
    """More than 32 768 queries at the default window take the piped search with graded windows (40 000 queries: cuts of 4 096 /
    8 192 / 15 424 / 8 192 / 4 096, three rank workers, up to three consumers, windows marshalled in whatever order they finished);
    window=65536 runs the same queries as ONE window on the calling thread.  A query's hits do not depend on its window: every hit
    field and every CIGAR must be equal, query by query."""
    import numpy as np
    from vsearch_amd import Aligner
    from vsearch_amd.search import SearchSession, HIT_FIELDS
    rs = np.random.RandomState(40000)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    db = acgt[rs.randint(0, 4, size=(64, 200))]
    nq = 40000
    src, qlen = rs.randint(0, 64, nq), rs.randint(60, 81, nq)
    start = (rs.random_sample(nq) * (201 - qlen)).astype(np.int64)
    minus = rs.random_sample(nq) < 0.5
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    queries = []
    for k in range(nq):
        q = db[src[k], start[k]:start[k] + qlen[k]].copy()
        sub = rs.random_sample(qlen[k]) < 0.03                       # 3 % substitutions: another base
        q[sub] = acgt[(np.searchsorted(acgt, q[sub]) + rs.randint(1, 4, int(sub.sum()))) % 4]
        queries.append((comp[q[::-1]] if minus[k] else q).tobytes())
    dbs = [row.tobytes() for row in db]

    def cigars(hits, cig):
        nul = np.flatnonzero(np.frombuffer(cig, np.uint8) == 0)
        off = hits["cigar_off"].astype(np.int64)
        end = nul[np.searchsorted(nul, off)]
        return [cig[a:b] for a, b in zip(off.tolist(), end.tolist())]

    with Aligner() as al:
        got = []
        for opts in ({}, {"window": 65536}):
            s = SearchSession(al, dbs, id=0.9, strand_both=1, **opts)
            got.append(s.search_batch_raw(queries))
            s.close()
    (f1, h1, c1), (f2, h2, c2) = got
    for first, hits in ((f1, h1), (f2, h2)):
        assert len(first) == nq + 1 and first[0] == 0 and first[nq] == len(hits)
        assert np.all(first[1:] >= first[:-1])
    assert len(h2) > nq // 2                                         # (the queries do find their sources)
    assert np.array_equal(f1, f2)
    assert np.array_equal(h1["query"], np.repeat(np.arange(nq), np.diff(f1).astype(np.int64)))
    for name in HIT_FIELDS:
        assert np.array_equal(h1[name], h2[name]), name
    assert cigars(h1, c1) == cigars(h2, c2)


def test_dust_masking_refuses_overlapping_sequences(gpu_required):
    """DUST rewrites the text in place: sequences that share bytes of the blob would get the union of their masks (the reference
    masks every sequence on its own, mask.cpp:233-249), so the library refuses them -- database and raw queries alike."""
    import ctypes as C
    import numpy as np
    from vsearch_amd import Aligner, _lib
    lib = gpu_required
    rng = random.Random(5)
    blob = common.rnd_seq(rng, 400).encode()
    off = np.array([0, 100, 150], dtype=np.uint64)          # the third starts inside the second
    ln = np.array([100, 100, 200], dtype=np.uint32)
    with Aligner() as al:
        for soft_mask, want in ((2, _lib.VSX_EINVAL), (0, 0)):
            o = _lib.SearchOpts()
            lib.vsx_search_opts_default(C.byref(o))
            o.soft_mask = soft_mask
            o.id = 0.9
            h = C.c_void_p()
            rc = lib.vsx_searcher_create(al.h, C.byref(h), C.byref(o), 3, C.cast(C.c_char_p(blob), C.c_void_p), len(blob),
                                         off.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p))
            assert rc == want, (soft_mask, rc, lib.vsx_last_error())
            if rc != 0:
                assert b"overlap" in lib.vsx_last_error()
            if rc == 0:
                lib.vsx_searcher_destroy(h)
        # disjoint but unordered offsets are fine
        off2 = np.array([200, 0, 100], dtype=np.uint64)
        ln2 = np.array([100, 100, 100], dtype=np.uint32)
        o = _lib.SearchOpts()
        lib.vsx_search_opts_default(C.byref(o))
        o.soft_mask = 2
        o.id = 0.9
        h = C.c_void_p()
        rc = lib.vsx_searcher_create(al.h, C.byref(h), C.byref(o), 3, C.cast(C.c_char_p(blob), C.c_void_p), len(blob),
                                     off2.ctypes.data_as(C.c_void_p), ln2.ctypes.data_as(C.c_void_p))
        assert rc == 0, lib.vsx_last_error()
        lib.vsx_searcher_destroy(h)


@pytest.mark.gpu
def test_a_span_whose_end_wraps_is_refused(gpu_required):
    """offset 2^64 - 4 with length 8 "ends" at 4: the database and the queries are checked without adding the two (before any
    device work: nothing of the blob is read)"""
    import ctypes as C
    import numpy as np
    from vsearch_amd import Aligner, _lib
    lib = gpu_required
    blob = b"ACGTTGCAACGGTCAT"
    vblob = C.cast(C.c_char_p(blob), C.c_void_p)
    good_off, good_len = np.array([0, 8], np.uint64), np.array([8, 8], np.uint32)
    bad_off, bad_len = np.array([0, (1 << 64) - 4], np.uint64), np.array([8, 8], np.uint32)
    with Aligner() as al:
        o = _lib.SearchOpts()
        lib.vsx_search_opts_default(C.byref(o))
        o.id = 0.9
        h = C.c_void_p()
        rc = lib.vsx_searcher_create(al.h, C.byref(h), C.byref(o), 2, vblob, len(blob), bad_off.ctypes.data_as(C.c_void_p), bad_len.ctypes.data_as(C.c_void_p))
        assert (rc, lib.vsx_last_error()) == (_lib.VSX_EINVAL, b"vsx_searcher_create: sequence exceeds the blob")
        rc = lib.vsx_searcher_create(al.h, C.byref(h), C.byref(o), 2, vblob, len(blob), good_off.ctypes.data_as(C.c_void_p), good_len.ctypes.data_as(C.c_void_p))
        assert rc == 0, lib.vsx_last_error()
        try:
            hits = _lib.Hits()
            rc = lib.vsx_search_batch(h, 2, vblob, len(blob), bad_off.ctypes.data_as(C.c_void_p), bad_len.ctypes.data_as(C.c_void_p), C.byref(hits))
            assert (rc, lib.vsx_last_error()) == (_lib.VSX_EINVAL, b"vsx_search_batch: query exceeds the blob")
            cands = _lib.Candidates()
            for device in (1, 0):
                rc = lib.vsx_search_candidates_batch(h, device, 2, vblob, len(blob), bad_off.ctypes.data_as(C.c_void_p), bad_len.ctypes.data_as(C.c_void_p),
                                                     C.byref(cands))
                assert (rc, lib.vsx_last_error()) == (_lib.VSX_EINVAL, b"vsx_search_candidates_batch: query exceeds the blob")
        finally:
            lib.vsx_searcher_destroy(h)


@pytest.mark.gpu
def test_allpairs_stream_equals_blocks(gpu_required):
    """r05: vsx_allpairs_stream overlaps pair enumeration, alignment and hit completion of consecutive blocks; the hits it hands to its
    sink, block after block, must be exactly those of one vsx_allpairs_block call -- ranked path and acceptall (every pair kept)"""
    import random
    from vsearch_amd import Aligner
    from vsearch_amd.search import SearchSession
    rng = random.Random(77)
    fam = [common.rnd_seq(rng, rng.randint(60, 220)) for _ in range(12)]
    seqs = [common.mutate(rng, rng.choice(fam), rng.choice([0.02, 0.08, 0.2])) for _ in range(230)]
    with Aligner() as al:
        for acceptall, kw in ((False, dict(id=0.8)), (True, dict(id=0.5)), (False, dict(id=0.7, maxgaps=3))):
            ss = SearchSession(al, seqs, **kw)
            whole = ss.allpairs(acceptall=acceptall)
            pairs = ss.stats["pairs_aligned"]
            for block in (1, 37, 100, 1000):
                got = ss.allpairs_stream(block=block, acceptall=acceptall)
                assert got == whole, (acceptall, kw, block)
                assert ss.stats["pairs_aligned"] == pairs
            part = ss.allpairs_stream(first=50, count=120, block=50, acceptall=acceptall)
            assert part == whole[50:170]
            ss.close()


_LAZY_SNIPPET = r"""
import hashlib, json, random, sys
sys.path.insert(0, %r)
from tests import common
from vsearch_amd import Aligner
from vsearch_amd.search import SearchSession
rng = random.Random(2026)
fam = [common.rnd_seq(rng, rng.randint(150, 400)) for _ in range(40)]
db = [common.mutate(rng, rng.choice(fam), rng.choice([0.01, 0.04, 0.1, 0.2])) for _ in range(1200)]
qs = [common.mutate(rng, rng.choice(db), rng.choice([0.0, 0.03, 0.08, 0.15]))[:rng.randint(80, 300)] for _ in range(500)] + [common.rnd_seq(rng, 200) for _ in range(20)]
out = {}
with Aligner() as al:
    for name, kw in (("default", dict(id=0.9)), ("three", dict(id=0.93, maxaccepts=3, maxrejects=5)), ("strict", dict(id=0.97, maxaccepts=1, maxrejects=12)),
                     ("all", dict(id=0.8, maxaccepts=0, maxrejects=0)), ("both", dict(id=0.9, strand_both=1, maxaccepts=2)),
                     # r06 (VERDICT r05 "next" 5): few rejects allowed, weak hits reported, both at once on both strands, unlimited accepts with a reject limit
                     ("two_four", dict(id=0.95, maxaccepts=2, maxrejects=4)), ("weak", dict(id=0.96, weak_id=0.85, maxaccepts=1, maxrejects=4)),
                     ("both_weak", dict(id=0.95, weak_id=0.8, strand_both=1, maxaccepts=2, maxrejects=4)), ("all_four", dict(id=0.9, maxaccepts=0, maxrejects=4))):
        ss = SearchSession(al, db, **kw)
        res = ss.search_batch(qs)
        h = hashlib.sha256(json.dumps(res, sort_keys=True).encode()).hexdigest()
        out[name] = (h, int(ss.stats["pairs_aligned"]), sum(len(r) for r in res))
        ss.close()
print("OUT", json.dumps(out))
"""


@pytest.mark.gpu
def test_lazy_first_batches_align_a_subset_with_the_same_hits(gpu_required):
    """r05: vsx_search_batch aligns a query's first batch lazily -- as many candidates as it still needs accepts, then the rest of the
    reference's first eight, then eights.  Nine option sets (default, maxaccepts 3, a strict identity with many first-candidate failures,
    unlimited accepts / rejects, both strands; r06: maxaccepts 2 / maxrejects 4, --weak_id, both strands + weak hits, unlimited accepts
    with maxrejects 4): every hit field identical to the run with the reference's batches (VSX_SEARCH_LAZY=0), and
    never more pairs aligned -- fewer wherever maxaccepts is below eight."""
    import json
    import sys
    outs = {}
    for mode in ("0", "1"):
        e = dict(os.environ, VSX_SEARCH_LAZY=mode)
        p = subprocess.run([sys.executable, "-c", _LAZY_SNIPPET % ROOT], env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
        outs[mode] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("OUT")][-1][4:])
    for name in outs["0"]:
        eager, lazy = outs["0"][name], outs["1"][name]
        assert eager[0] == lazy[0] and eager[2] == lazy[2], name             # same hits, every field
        assert lazy[1] <= eager[1], (name, lazy, eager)                      # a subset of the reference's pairs
        if name in ("default", "three", "strict", "both", "two_four", "weak", "both_weak"):
            assert lazy[1] < eager[1], (name, lazy, eager)
        else:
            assert lazy[1] == eager[1], (name, lazy, eager)                  # unlimited accepts: the first batch is the reference's
