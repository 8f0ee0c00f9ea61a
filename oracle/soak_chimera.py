#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY: randomized soak of chimera detection (vsx_uchime_ref, vsx_uchime_denovo -> vsx_chimera.hip and its
host route) against the REFERENCE CLI's --uchimeout, byte for byte.

A round draws one of --uchime_ref, --uchime_denovo, --uchime2_denovo, --uchime3_denovo; a length class (60-120, 300-500,
1 200-1 600, 3 900-4 200: the last one straddles the kernel's limit of 4 096); the mask mode and --hardmask; --minh, --mindiv,
--mindiffs, --xn, --dn, --abskew (de novo); window and search_window.  Data: for --uchime_ref a family database of 20-40 references
and 30-60 queries (two- and three-parent chimeras, mutated members, odd sequences); for the de novo commands 80-150 sized sequences
of a small tests/denovo_data.cascade_set().  The two long classes divide the number of QUERIES (for the de novo commands: of
sequences, each of which is a query) by 3 and by 8; the database of --uchime_ref keeps its 20-40 references, so a query still
meets up to 16 candidates.  The reference aligns every query with each of them: a full-size round at 4 000 symbols costs it
more than ten seconds.  A round the reference refuses counts as failing.  --reference-only counts the reference's lines without
a device.  The output's "coverage" counts the rounds per command and length class and the rounds with --hardmask / --abskew.

--commands names the commands a round draws from (default: the four above, so a seed's rounds stay what they were).  With
chimeras_denovo in the list, such a round takes a tests/chimeras_long_data.seeded_set() of drawn sizes in a length class of 300-500,
1 200-1 600 or 1 900-2 200 (the last one straddles the kernel's VSX_CHIMERAS_LONG_MAX_QLEN = 2 048), --chimeras_parts (unset, 2, 5,
15), --abskew, the mask mode and --hardmask, and --chimeras_diff_pct 0, 1, 2.5 or 0.125 (the kernel's exact path) or, with
probability 0.15, 0.1 (the host restatement answers: the stats must say so).  Compared: --tabbedout and the labels of --chimeras and
--nonchimeras; then the device's records against the host restatement's (VSX_CHIMERA=host).  Coverage: the length class, "parts",
"diff_pct_host".

--outputs alns (default: off, so a seed's rounds stay byte for byte what they were): every round of the four commands also hands the
CLI --uchimealns, --chimeras, --nonchimeras and --borderline.  Their options come from a second generator seeded from (seed, round
number), so the first stream is untouched: --alignwidth 0 / 1 / 60 / 80 / 133 (the reference takes all five), --fasta_score,
--sizeout / --xsize / --relabel, --fasta_width 0 / 60 / 80; --xn / --dn are the round's.  Compared byte for byte: the four files with
ChimeraSession / DenovoChimeraSession.uchimealns, chimeras_fasta, nonchimeras_fasta, borderline_fasta; then alns_raw of every scored
record on the device with VSX_CHIMALNS=host field for field, and vsx_chimalns_last_stats: host_long_query is non-zero exactly when a
scored query has more than 4 096 symbols (the 3 900-4 200 class), every other record is the kernel's unless one of its pairs is a
sentinel pair.  Coverage: alns, alignwidth0, alignwidth_other (1 or 133), fasta_score, borderline (that file is not empty),
alns_host_long (judged from the reference's --uchimeout).  An exception of a library call ends the script with exit status 3:
nothing more is started on the device.

    python oracle/soak_chimera.py --seconds 120 --seed 1 --out soak_chimera.json
"""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import refcli  # noqa: E402
from tests import chimeras_long_data, common, denovo_data  # noqa: E402

LENGTHS = [((60, 120), 1), ((300, 500), 1), ((1200, 1600), 3), ((3900, 4200), 8)]
MASKS = {"none": 0, "soft": 1, "dust": 2}
COMMANDS = ["uchime_ref", "uchime_denovo", "uchime2_denovo", "uchime3_denovo"]
LONG_LENGTHS = [((300, 500), 1), ((1200, 1600), 3), ((1900, 2200), 6)]


def draw_long(rng):
    """--chimeras_denovo -> ((length range, divisor of the counts), keywords of the session, the CLI's arguments, the set's sizes);
    every number is drawn whether or not its option is then set"""
    length = rng.choice(LONG_LENGTHS)
    o, cli = {}, []
    mask = rng.choice(["none", "soft", "dust"])
    cli += ["--qmask", mask]
    o["soft_mask"] = mask
    if rng.random() < 0.25:
        cli.append("--hardmask")
        o["hardmask"] = 1
    parts, abskew = rng.choice([2, 5, 15]), rng.choice([1.5, 2.0, 3.5])
    if rng.random() < 0.5:
        o["parts"] = parts
        cli += ["--chimeras_parts", str(parts)]
    if rng.random() < 0.3:
        o["abskew"] = abskew
        cli += ["--abskew", str(abskew)]
    pct, host = rng.choice([0, 1, 2.5, 0.125]), rng.random() < 0.15
    pct = 0.1 if host else pct
    if pct:
        o["diff_pct"] = float(pct)
        cli += ["--chimeras_diff_pct", str(pct)]
    w, sw = rng.choice([0, 1, 7, 50]), rng.choice([0, 5, 64])
    if w:
        o["window"] = w
    if sw:
        o["search_window"] = sw
    div = length[1]
    sizes = dict(seed=rng.randrange(1 << 30), n_families=max(2, rng.randint(8, 20) // div), n_chimeras=max(3, rng.randint(20, 50) // div),
                 n_long=rng.randint(3, 4), length=length[0])
    return length, o, cli, sizes


def draw(rng, commands=COMMANDS):
    """-> (command, (length range, divisor of the counts), keywords of the session, the CLI's arguments)"""
    cmd = rng.choice(commands)
    if cmd == "chimeras_denovo":
        return (cmd,) + draw_long(rng)
    length = rng.choice(LENGTHS)
    o, cli = {}, []
    mask = rng.choice(["none", "soft", "dust"])
    if cmd == "uchime_ref":
        cli += ["--qmask", mask, "--dbmask", mask]
    else:
        cli += ["--qmask", mask]
    o["soft_mask"] = MASKS[mask]
    if rng.random() < 0.25:
        cli.append("--hardmask")
        o["hardmask"] = 3 if cmd == "uchime_ref" else 1
    for key, vals in (("minh", [0.1, 0.2, 0.5]), ("mindiv", [0.5, 1.5]), ("mindiffs", [2, 4]), ("xn", [4.0, 6.5]), ("dn", [1.1, 2.0])):
        v = rng.choice(vals)
        if rng.random() < 0.3:
            o[key] = v
            cli += ["--" + key, str(v)]
    v = rng.choice([1.0, 1.5, 3.5, 8.0])
    if cmd != "uchime_ref" and rng.random() < 0.3:
        o["abskew"] = v
        cli += ["--abskew", str(v)]
    w, sw = rng.choice([0, 1, 7, 50]), rng.choice([0, 5, 64])
    if w:
        o["window"] = w
    if sw:
        o["search_window"] = sw
    return cmd, length, o, cli


ALIGNWIDTHS = [0, 1, 60, 80, 133]          # (the reference CLI takes each of them: checked with --reference-only)
ALNS_FILES = ("uchimealns", "chimeras", "nonchimeras", "borderline")
ALNS_ARRAYS = ("record", "alnlen", "text_off", "text", "line_first", "line_end", "best_i", "h", "counts")
MAX_QLEN = 4096                            # VSX_CHIMERA_MAX_QLEN: a longer query's block is rendered on the host


def draw_alns(r):
    """--outputs alns -> the options of the four extra files, from the round's own generator; every number is drawn"""
    w = dict(alignwidth=r.choice(ALIGNWIDTHS), fasta_score=r.random() < 0.5, fasta_width=r.choice([0, 60, 80]))
    sizeout, xsize, relabel = r.random() < 0.3, r.random() < 0.3, r.random() < 0.3
    w.update(sizeout=sizeout, xsize=xsize and not sizeout, relabel="C" if relabel else None)      # (the reference refuses the two together)
    return w


def alns_cli(w, tmp):
    files = {k: os.path.join(tmp, k) for k in ALNS_FILES}
    cli = ["--alignwidth", str(w["alignwidth"]), "--fasta_width", str(w["fasta_width"])]
    for k in ALNS_FILES:
        cli += ["--" + k, files[k]]
    cli += ["--" + k for k in ("fasta_score", "sizeout", "xsize") if w[k]]
    return files, cli + (["--relabel", w["relabel"]] if w["relabel"] else [])


def alns_diff(ses, src, recs, qlens, w, exp):
    """the four files against the session's texts, then alns_raw of every scored record on the device against VSX_CHIMALNS=host
    field for field, and the route counters -> a mismatch record or None"""
    kw = {k: w[k] for k in ("sizeout", "xsize", "relabel", "fasta_width")}
    got = dict(uchimealns=ses.uchimealns(*src, records=recs, alignwidth=w["alignwidth"], xsize=w["xsize"]).splitlines(True))
    for k in ALNS_FILES[1:]:
        got[k] = [l + "\n" for l in getattr(ses, k + "_fasta")(*src, records=recs, fasta_score=w["fasta_score"], **kw)]
    for k in ALNS_FILES:
        if got[k] != exp[k]:
            first = next((i for i, (x, y) in enumerate(zip(got[k], exp[k])) if x != y), min(len(got[k]), len(exp[k])))
            return {"what": k, "lines": [len(got[k]), len(exp[k])], "first_diff": first, "got": got[k][first][:300] if first < len(got[k]) else None,
                    "exp": exp[k][first][:300] if first < len(exp[k]) else None}
    dev = ses.alns_raw(*src[:1], recs, alignwidth=w["alignwidth"], select="Y?N")
    os.environ["VSX_CHIMALNS"] = "host"
    try:
        host = ses.alns_raw(*src[:1], recs, alignwidth=w["alignwidth"], select="Y?N")
    finally:
        del os.environ["VSX_CHIMALNS"]
    for name, x, y in zip(ALNS_ARRAYS, dev.arrays(), host.arrays()):
        if x != y:
            return {"what": f"alns_raw: device and VSX_CHIMALNS=host differ in {name}"}
    st, hs = dev.stats, host.stats
    scored = [k for k, r in enumerate(recs) if r["status"] == "scored"]
    long_queries = sum(qlens[k] > MAX_QLEN for k in scored)
    if hs["records_host"] != len(scored) or hs["host_forced"] != len(scored) or hs["records_kernel"] != 0:
        return {"what": "VSX_CHIMALNS=host: the host did not answer every record", "stats": hs}
    if st["records_selected"] != len(scored) or st["records_kernel"] + st["records_host"] != len(scored) or st["host_forced"] != 0:
        return {"what": "alns_raw: the counters do not add up to the scored records", "stats": st}
    if (st["host_long_query"] > 0) != (long_queries > 0) or st["host_long_query"] > long_queries:
        return {"what": f"alns_raw: {long_queries} scored queries above {MAX_QLEN} symbols, host_long_query says otherwise", "stats": st}
    if st["records_host"] > st["host_long_query"] + st["host_long_alignment"] + st["sentinel_pairs"] or (long_queries == 0 and st["host_long_alignment"]):
        return {"what": "alns_raw: records on the host that are neither long nor sentinel pairs", "stats": st}
    return None


def long_scored(uchimeout, seqs_by_label):
    """does the reference's --uchimeout hold a scored record (it names two parents) of a query above the kernel's limit?"""
    by_name = {l.split(";")[0]: s for l, s in seqs_by_label.items()}          # (the de novo commands print the label without its ;size=)
    for line in uchimeout:
        f = line.split("\t")
        if f[2] != "*" and f[3] != "*" and len(by_name[f[1].split(";")[0]]) > MAX_QLEN:
            return True
    return False


def _chimera(rng, parents):
    n = min(len(p) for p in parents)
    cuts = sorted(rng.sample(range(n // 6, n - n // 6), len(parents) - 1))
    edges = [0] + cuts + [None]
    return common.mutate(rng, "".join(p[edges[i]:edges[i + 1]] for i, p in enumerate(parents)), 0.01)


def ref_data(rng, length, div):
    (lo, hi), n_db, n_q = length, rng.randint(20, 40), max(4, rng.randint(30, 60) // div)
    members = rng.choice([2, 4, 5])
    db = []
    while len(db) < n_db:
        anc = common.rnd_seq(rng, rng.randint(lo, hi))
        db += [common.mutate(rng, anc, rng.choice([0.03, 0.05, 0.08])) for _ in range(min(members, n_db - len(db)))]
    qs = []
    for i in range(n_q):
        r = rng.random()
        if r < 0.35:
            qs.append(_chimera(rng, rng.sample(db, 2)))
        elif r < 0.6 and len(db) >= 3:
            qs.append(_chimera(rng, rng.sample(db, 3)))
        elif r < 0.85:
            qs.append(common.mutate(rng, rng.choice(db), 0.03))
        else:
            qs.append(rng.choice([common.rnd_seq(rng, rng.randint(1, 40)), common.mutate(rng, rng.choice(db), 0.05, "ACGTNRY"),
                                  rng.choice(db).lower(), "AC" * rng.randint(20, 60) + rng.choice(db)[:lo]]))
    return [f"r{i}" for i in range(len(db))], db, [f"q{i}" for i in range(len(qs))], qs


def denovo_data_set(rng, length, div):
    fam, chim = max(2, rng.randint(20, 30) // div), max(2, rng.randint(18, 36) // div)
    return denovo_data.cascade_set(seed=rng.randrange(1 << 30), n_families=fam, members=(2, 4), n_chimeras=chim, extras=False, length=length)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    ap.add_argument("--max-rounds", type=int, default=0, help="stop after this many rounds (0: run for --seconds): a deterministic set of rounds for a given seed")
    ap.add_argument("--reference-only", action="store_true", help="run the reference alone and count its lines (no device)")
    ap.add_argument("--commands", default=",".join(COMMANDS), help="the commands a round draws from, comma-separated (also: chimeras_denovo)")
    ap.add_argument("--outputs", default="", choices=["", "alns"], help="alns: every round of the four commands also writes and compares "
                    "--uchimealns, --chimeras, --nonchimeras and --borderline (default: off, so a seed's rounds stay what they were)")
    a = ap.parse_args()
    alns = a.outputs == "alns"
    commands = a.commands.split(",")
    if not set(commands) <= set(COMMANDS + ["chimeras_denovo"]):
        raise SystemExit(f"--commands: {a.commands}")
    if not refcli.available():
        raise SystemExit("oracle/_ref/vsearch_ref missing: make -C oracle ref_full")
    al = None
    if not a.reference_only:
        from vsearch_amd import Aligner, ChimerasDenovoSession, ChimeraSession, DenovoChimeraSession
        al = Aligner()
    rng = random.Random(a.seed)
    t_end = time.time() + a.seconds
    rounds = lines = bad = 0
    ref_seconds = 0.0
    failing = []
    coverage = {}
    fatal = None
    with tempfile.TemporaryDirectory(prefix="vsxsoakc_") as tmp:
        qf, df, uo = os.path.join(tmp, "q.fa"), os.path.join(tmp, "db.fa"), os.path.join(tmp, "u.tsv")
        while time.time() < t_end and (a.max_rounds <= 0 or rounds < a.max_rounds):
            cmd, (length, div), o, cli, *sizes = draw(rng, commands)
            if cmd == "chimeras_denovo":
                rounds += 1
                for key in [f"{cmd}@{length[0]}-{length[1]}"] + [k for k in ("hardmask", "abskew", "parts") if k in o] + \
                        ["diff_pct_host"] * (o.get("diff_pct") == 0.1):
                    coverage[key] = coverage.get(key, 0) + 1
                labels, seqs = chimeras_long_data.seeded_set(**sizes[0])
                full = [cmd] + cli + [f"length={length}", f"n={len(seqs)}"] + [f"{k}={o[k]}" for k in ("window", "search_window") if k in o]
                t0 = time.time()
                try:
                    exp = chimeras_long_data.ref_outputs(tmp, labels, seqs, cli)
                except Exception as e:
                    exp = None
                    bad += 1
                    if len(failing) < 10:
                        failing.append({"cli": full, "round": rounds - 1, "error": str(e)[-300:]})
                ref_seconds += time.time() - t0
                if exp is None:
                    continue
                lines += sum(len(v) for v in exp.values())
                if a.reference_only:
                    continue
                s = ChimerasDenovoSession(al, seqs, labels, **o)
                recs = s.chimeras_denovo()
                got = dict(tabbedout=s.tabbedout(), chimeras=s.chimeras, nonchimeras=s.nonchimeras)
                diff = next(({"what": k, "lines": [len(got[k]), len(exp[k])],
                              "first_diff": next((i for i, (x, y) in enumerate(zip(got[k], exp[k])) if x != y), min(len(got[k]), len(exp[k])))}
                             for k in exp if got[k] != exp[k]), None)
                if diff is None and o.get("diff_pct") == 0.1 and s.stats["queries_kernel"] != 0:
                    diff = {"what": "diff_pct 0.1 is the host restatement's, the stats count kernel queries", "stats": dict(s.stats)}
                if diff is None and o.get("diff_pct") != 0.1 and s.stats["queries_kernel"] == 0:
                    diff = {"what": "no query reached the kernel", "stats": dict(s.stats)}
                s.close()
                if diff is None:
                    os.environ["VSX_CHIMERA"] = "host"
                    try:
                        h = ChimerasDenovoSession(al, seqs, labels, **o)
                        if h.chimeras_denovo() != recs or h.stats["queries_kernel"] != 0:
                            diff = {"what": "device and host records differ"}
                        h.close()
                    finally:
                        del os.environ["VSX_CHIMERA"]
                if diff is not None:
                    bad += 1
                    if len(failing) < 10:
                        failing.append({"cli": full, "round": rounds - 1, **diff})
                continue
            if cmd == "uchime_ref":
                tn, db, qn, qs = ref_data(rng, length, div)
                refcli.write_fasta(df, tn, db)
                args = ["--uchime_ref", qf, "--db", df]
            else:
                qn, qs = denovo_data_set(rng, length, div)
                args = [f"--{cmd}", qf]
            refcli.write_fasta(qf, qn, qs)
            w, files, alns_args = None, {}, []
            if alns:                                     # (its own generator per round: the first stream is what it was)
                w = draw_alns(random.Random(a.seed * 1000003 + rounds))
                files, alns_args = alns_cli(w, tmp)
            t0 = time.time()
            p = subprocess.run([refcli.REF_BIN] + args + ["--uchimeout", uo, "--threads", "1", "--quiet"] + cli + alns_args, capture_output=True, text=True)
            ref_seconds += time.time() - t0
            rounds += 1
            for key in [f"{cmd}@{length[0]}-{length[1]}"] + [k for k in ("hardmask", "abskew") if k in o]:
                coverage[key] = coverage.get(key, 0) + 1
            full = [cmd] + cli + [f"length={length}", f"n={len(qs)}"] + [f"{k}={o[k]}" for k in ("window", "search_window") if k in o]
            if alns:
                full += [f"{k}={v}" for k, v in w.items()]
            if p.returncode != 0:
                bad += 1
                if len(failing) < 10:
                    failing.append({"cli": full, "round": rounds - 1, "error": p.stderr[-300:]})
                continue
            exp = open(uo).read().splitlines()
            lines += len(exp)
            exp_alns = {k: open(f).read().splitlines(True) for k, f in files.items()}
            if alns:
                lines += sum(len(v) for v in exp_alns.values())
                for key, hit in (("alns", True), ("alignwidth0", w["alignwidth"] == 0), ("alignwidth_other", w["alignwidth"] in (1, 133)),
                                 ("fasta_score", w["fasta_score"]), ("borderline", bool(exp_alns["borderline"])),
                                 ("alns_host_long", long_scored(exp, dict(zip(qn, qs))))):
                    if hit:
                        coverage[key] = coverage.get(key, 0) + 1
            if a.reference_only:
                continue
            diff = None
            try:                                         # any exception of a device call: nothing more is started on the GPU
                if cmd == "uchime_ref":
                    ses, src = ChimeraSession(al, db, labels=tn, **o), (qs, qn)
                    recs = ses.uchime_ref(qs)
                    got, qlens = ses.uchimeout(qs, qn, records=recs, xsize=bool(alns and w["xsize"])), [len(q) for q in qs]
                else:
                    ses, src = DenovoChimeraSession(al, qs, qn, variant=cmd.split("_")[0], **o), ()
                    recs = ses.uchime_denovo()
                    got, qlens = ses.uchimeout(recs, xsize=bool(alns and w["xsize"])), [len(q) for q in ses.seqs]
                if got != exp:
                    first = next((i for i, (x, y) in enumerate(zip(got, exp)) if x != y), min(len(got), len(exp)))
                    diff = {"lines": [len(got), len(exp)], "first_diff": first, "got": got[first] if first < len(got) else None,
                            "exp": exp[first] if first < len(exp) else None}
                elif alns:
                    diff = alns_diff(ses, src, recs, qlens, w, exp_alns)
                ses.close()
            except Exception as e:
                fatal = f"{type(e).__name__}: {e}"
                diff = {"error": fatal[-500:]}
            if diff is not None:
                bad += 1
                if len(failing) < 10:
                    failing.append({"cli": full, "round": rounds - 1, **diff})
            if fatal is not None:
                break
    if al is not None and fatal is None:
        al.close()
    out = {"rounds": rounds, "lines": lines, "failing_rounds": bad, "failures": failing, "seed": a.seed, "seconds": a.seconds,
           "reference_seconds": round(ref_seconds, 3), "coverage": coverage,
           "what": "vsx_uchime_ref / vsx_uchime_denovo vs vsearch_ref --uchime_ref / --uchime*_denovo --uchimeout with the same randomly drawn options"
                   + ("; --uchimealns, --chimeras, --nonchimeras, --borderline vs the sessions' texts, alns_raw on the device vs VSX_CHIMALNS=host" if alns else "")
                   + ("; vsx_chimeras_denovo vs --chimeras_denovo --tabbedout / --chimeras / --nonchimeras, device vs VSX_CHIMERA=host" if "chimeras_denovo" in commands else "")}
    if fatal is not None:
        out["fatal"] = fatal[-2000:]
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f)
    if fatal is not None:                                # a library error that is no mismatch: exit status 3, and no destructor
        sys.stdout.flush()                               # touches the device again
        os._exit(3)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
