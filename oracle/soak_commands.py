#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY: randomized soaks of the newer commands against the REFERENCE CLI (oracle/_ref/vsearch_ref), byte for
byte, and of the device route against the library's host restatement, field for field (floats by their bits).

    --command NAME      one leg of the registry LEGS: filter (--fastq_filter / --fastx_filter), eestats (--fastq_eestats /
                        --fastq_eestats2), fastq_stats (--fastq_stats / --fastq_chars), derep (--derep_fulllength / --fastx_uniques /
                        --derep_id), derep_prefix, search_exact, orient, sintax, otutab (--otutabout / --biomout /
                        --mothur_shared_out), hitout (the seven hit writers of --usearch_global), mask (--fastx_mask / --maskfasta),
                        getseqs (--fastx_getseqs / --fastx_getseq / --fastx_getsubseq), cut (--cut)
    --route device|host device: the library on the device against the CLI, then the host restatement against the device result.
                        host: no context is created; the host restatement alone (the route of a call or searcher without a device, or
                        the leg's VSX_<COMMAND>=host) is compared with the CLI.  Needs no GPU.

A leg is five functions over tests/*_data.py: draw (options), data (a set), reference (the CLI with --threads 1), library, compare;
`same` compares two library results field for field and `cover` names the coverage classes of a round.  A round draws every random
number whether or not the option it belongs to is then set (each with probability 0.3 unless the leg says otherwise), so the stream
does not depend on the choices.  A round the reference refuses counts as failing; a mismatch is recorded and the rounds go on; a
library error that is no mismatch (VSX_EHIP, a sticky device error, any exception of the device call) ends the script at once with
exit status 3: nothing is started on a GPU after a fault.  --reference-only counts the reference's lines without the library.
A leg's `reference` may leave cfg["cover_after"]: coverage classes that only the reference's answer decides.

The legs (data per round; what is drawn beyond the command's own options; the "coverage" classes the output counts):
    filter        100-300 reads of a length in 20 .. 320, in a third of the rounds 63 / 64 / 65 / 127 / 128 / 129 (the kernel walks
                  chunks of 64 positions), paired 0.3, FASTA input 0.15; fastq_filter_data.draw_opts(), the encoding (--fastq_ascii
                  33 / 64, qmin, qmax), in half of the rounds --fastq_truncee / --fastq_maxee set to a sum the walk itself reaches,
                  window 0 / 1 / 7 / 64 / 1000, scattered blobs 0.3.  paired, fasta, ascii64, truncee_or_rate, chunk_edge, scattered,
                  exact_ee
    eestats       100-300 reads up to 300 long; encoding, --length_cutoffs, 1-6 unsorted --ee_cutoffs, window, want (both commands
                  or one).  ascii64, eestats2, window_split
    fastq_stats   100-300 reads, length 0 included; encoding (qmin >= 0), --fastq_tail, window; both commands.  chars, ascii64
    derep         300-1 000 reads of derep_data.random_set(); the command (derep_fulllength, fastx_uniques on FASTA, on FASTQ with
                  and without --fastq_qout_max, derep_id), --strand, --sizein, min / max unique size, --topn, min / max length,
                  --sizeout / --relabel / --xsize, VSX_DEREP_HASH_BITS unset / 3 / 16, scattered blobs, window.  one class per
                  command, fastq, strand_both, hash_cut
    derep_prefix  300-1 000 reads of derep_prefix_data.random_set(); the same options, VSX_DEREP_PREFIX_HASH_BITS.  hash_cut, topn,
                  sizein
    search_exact  200-600 database sequences with duplicates, IUPAC codes, lower case and low complexity, 200-400 queries on both
                  strands; --strand, --qmask / --dbmask, --hardmask, --sizein, window.  dust, hardmask, strand_both
    orient        50-200 database sequences, 100-300 reads on either strand, FASTQ 0.3; --wordlength 3 .. 12, and 13 .. 15 with 0.1
                  (the host answers: the route counters are checked), masks, --hardmask, --sizein / --sizeout / --xsize / --relabel,
                  VSX_ORIENT_HASH_BITS unset / 3, a small VSX_ORIENT_BUILD_KEYS 0.3, window.  wl_le_5, wl_12, wl_host, fastq,
                  hash_cut, build_chunks
    sintax        200-600 references in families 3 % apart with exact, shortened and lengthened copies (tied counts) and taxonomy
                  strings cut at any rank, 100-200 reads; --sintax_cutoff 0 / 0.5 / 0.8 / 1, --strand, --wordlength 3 .. 8 (9 .. 12
                  with 0.1: the host answers), --dbmask, --randseed >= 1, window.  The reference's command line refuses --hardmask
                  for this command, so it is not drawn.  strand_both, cutoff, wl_lt_8, wl_host
    otutab        1-40 otutab_data.random_label_set()s side by side as one --search_exact run, ;size= annotations, --sizein 0.5,
                  VSX_OTUTAB_HASH_BITS unset / 3 / 16; the three files.  hash_cut, biom, mothur
    hitout        hitout_data.live_inputs() at 200 x 200 through --usearch_global; --strand, masks, --hardmask, --n_mismatch,
                  --rowlen 0 / 1 / 64 / 80, --maxhits, --top_hits_only, --output_no_hits, --id 0.7 / 0.9, --maxaccepts 1 .. 4, window
                  0 / 1 / 7; all seven files, --userout in both field orders, the SAM header.  The host route renders the hit list
                  the CLI itself prints.  hardmask, minus_strand, rowlen0, n_mismatch, window1
    mask          100-300 sequences of 1 .. 600 symbols with low-complexity islands, lower case, N and IUPAC codes, in a third of the
                  rounds every length from fastx_mask_data.LENGTHS / SEGMENT_LENGTHS (63 / 64 / 65, 95 / 96 / 97, 191 .. 257), FASTQ 0.3;
                  the command (--maskfasta 0.3), --qmask, --hardmask, --min_unmasked_pct / --max_unmasked_pct drawn or, in half of the
                  rounds, the percentages two of the round's own sequences have exactly (py_fastx_mask: the verdict sits on `<` against
                  `<=`), --sizeout / --xsize / --relabel, --fasta_width 0 / 60 / 80, window 0 / 1 / 7 / 64, scattered blobs with gaps of
                  A 0.3, the long DUST route forced 0.3 (VSX_MASK_LONG_MIN 1 / 64 / 200, VSX_MASK_SEGMENT 64 / 192 / 256: the counters
                  must show long sequences).  dust, soft, hardmask, percent_exact, fastq, maskfasta, long_route, length_edge,
                  discarded (the log counts sequences below AND above the bounds)
    getseqs       200-600 headers in the style of test_gpu_getseqs.live_reads(), every seventh cut or padded to 63 / 64 / 65 / 127 /
                  128 / 129 bytes, sequences of 1 .. 60 symbols, FASTQ 0.3 (a FASTA input has the two FASTA files only); 1-40 needles cut
                  from the round's headers (whole labels, words, pieces across a ; or =, the case swapped in half), misses and one
                  needle of 63 .. 65 bytes, for the list modes in a labels file with blank lines and no final newline half of the time;
                  the mode, the command, --label_substr_match, --label_field (word modes), --subseq_start / --subseq_end (the end past
                  every sequence 0.3), --relabel / --sizeout / --xsize / --sizein, --fasta_width; VSX_GETSEQS_HASH_BITS unset / 3 / 16,
                  VSX_GETSEQS_MAX_LENGTHS below the distinct needle lengths 0.1 (the host answers: its counter is checked), window,
                  scattered and shared spans.  The reference takes --fastx_getseq and --fastx_getsubseq with --label alone and the
                  subsequence options only with the latter, so a round of another mode runs --fastx_getseqs.  one class per mode,
                  substr, field, subseq, fastq, hash_cut, lengths_host, notmatched (both sides of the split are non-empty)
    cut           100-300 sequences of 0 .. 600 symbols over ACGT, lower case, N, R, Y, U, one reading of the pattern planted at
                  cut_data.seeded_set()'s rate, every tenth with it at 0 and at L - P, three of P - 1 / P / P + 1 symbols; a pattern of
                  2 .. 12 IUPAC symbols with ^ and _ at any two places (one place in either order and both ends included), in a fifth
                  of the rounds A^A_A or AC^A_CA over planted runs, 0.1 a pattern of 65 .. 70 symbols (the host answers:
                  host_pattern_length is checked); VSX_CUT_TILE 64 / 128 / unset, the writer options, window, scattered blobs with gaps
                  of A.  Every result is also held against cut_data.py_cut().  tile_small, iupac_pattern, self_overlap, site_at_end,
                  short_sequence, pattern_host, discarded (cut and uncut lists both non-empty)

    python oracle/soak_commands.py --command filter --seconds 60 --seed 1 --out soak_filter.json
"""
import argparse
import contextlib
import importlib
import json
import os
import random
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

REF_BIN = os.path.join(HERE, "_ref", "vsearch_ref")
WINDOWS = [0, 1, 7, 64, 1000]
MASKS = ["none", "soft", "dust"]


class Refused(Exception):
    """the reference CLI did not accept the round"""


class Fatal(Exception):
    """a library error that is not a mismatch: the script ends"""


# ---- shared helpers ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def environment(**kv):
    """set (or, with None, unset) environment variables for the block"""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def seed_of(rng):
    return int(rng.integers(1, 2 ** 31))


def maybe(rng, o, key, value, p=0.3):
    """o[key] = value with probability p; the caller has drawn `value` already, and this draws its one number either way"""
    if rng.random() < p:
        o[key] = value
        return True
    return False


def encoding(rng, negative_qmin=True):
    """-> (options ascii / qmin / qmax where they differ from the defaults, the generators' keywords): --fastq_ascii 33 or 64 and a
    range both programs accept (ascii + qmin >= 33, ascii + qmax <= 126), as oracle/soak_merge.py draws them"""
    ascii = int(rng.choice([33, 64]))
    qmin = int(rng.integers(-5 if ascii == 64 else 0, 11))
    if not negative_qmin:
        qmin = max(qmin, 0)
    qmax = int(rng.integers(qmin + 20, 126 - ascii + 1))
    o = {}
    if ascii != 33:
        o["ascii"] = ascii
    if qmin != 0:
        o["qmin"] = qmin
    if qmax != 41:
        o["qmax"] = qmax
    return o, dict(ascii=ascii, qrange=(qmin if rng.random() < 0.3 else max(qmin, 2), qmax))


def first_diff(what, got, exp):
    """the first difference of two line lists (or two values) as a dict, or None"""
    if got == exp:
        return None
    if isinstance(got, (list, tuple)) and isinstance(exp, (list, tuple)):
        first = next((i for i, (x, y) in enumerate(zip(got, exp)) if x != y), min(len(got), len(exp)))
        return {"what": what, "lines": [len(got), len(exp)], "first_diff": first, "got": repr(got[first])[:300] if first < len(got) else None,
                "exp": repr(exp[first])[:300] if first < len(exp) else None}
    return {"what": what, "got": repr(got)[:300], "exp": repr(exp)[:300]}


def diff_of(pairs):
    for what, got, exp in pairs:
        d = first_diff(what, got, exp)
        if d is not None:
            return d
    return None


def bits(a):
    """an array as a list, floats by their bit patterns"""
    a = np.asarray(a)
    if a.dtype.kind == "f":
        a = np.ascontiguousarray(a, np.float64).view(np.uint64)
    return a.tolist()


def same_arrays(a, b, names, what="device and host"):
    for n in names:
        x, y = getattr(a, n), getattr(b, n)
        if (x is None) != (y is None):
            return {"what": f"{what}: {n} is missing on one side"}
        if x is None:
            continue
        if isinstance(x, np.ndarray):
            if x.shape != y.shape or x.dtype != y.dtype or bits(x) != bits(y):
                return {"what": f"{what}: {n} differs"}
        elif x != y:
            return {"what": f"{what}: {n} differs", "got": repr(x)[:200], "exp": repr(y)[:200]}
    return None


def same_struct(x, y, what):
    """two structured arrays field for field ('pad' bytes are nobody's)"""
    if (x is None) != (y is None):
        return {"what": f"{what}: missing on one side"}
    if x is None:
        return None
    if x.dtype != y.dtype or len(x) != len(y):
        return {"what": f"{what}: shapes differ"}
    for f in x.dtype.names:
        if f != "pad" and bits(x[f]) != bits(y[f]):
            return {"what": f"{what}: field {f} differs"}
    return None


def timed(fn, *a, **kw):
    """-> (result, seconds); an exception that names the reference's refusal becomes Refused"""
    t0 = time.perf_counter()
    try:
        out = fn(*a, **kw)
    except RuntimeError as e:
        if "reference CLI failed" in str(e) or REF_BIN in str(e) or "vsearch" in str(e):
            raise Refused(str(e)[-300:])
        raise
    return out, time.perf_counter() - t0


def scattered_blob(seed, gap_byte=b"#"):
    """a replacement of the packages' _blob: the items in shuffled order with gaps between them; the same lengths give the same
    offsets (a FASTQ call lays its qualities out with a second call)"""
    def blob(items):
        bs = [x.encode("latin-1") if isinstance(x, str) else bytes(x) for x in items]
        rng = random.Random(seed)
        order = list(range(len(bs)))
        rng.shuffle(order)
        off = np.zeros(len(bs), np.uint64)
        parts, at = [], 0
        for k in order:
            gap = rng.randint(0, 37)
            parts.append(gap_byte * gap)
            off[k] = at + gap
            parts.append(bs[k])
            at += gap + len(bs[k])
        return b"".join(parts) + gap_byte * 5, off, np.array([len(b) for b in bs], np.uint32)
    return blob


@contextlib.contextmanager
def patched(module, name, value):
    old = getattr(module, name)
    setattr(module, name, value)
    try:
        yield
    finally:
        setattr(module, name, old)


def hash_cut(rng, values=(None, 3, 16)):
    return values[int(rng.integers(0, len(values)))]


def mask_stretches(rng, seq):
    """a sequence with, at random, a lower-case stretch (soft masking) and a low-complexity stretch (DUST)"""
    if len(seq) > 60 and rng.random() < 0.3:
        a = rng.randrange(0, len(seq) - 40)
        seq = seq[:a] + seq[a:a + 30].lower() + seq[a + 30:]
    if len(seq) > 60 and rng.random() < 0.3:
        a = rng.randrange(0, len(seq) - 40)
        seq = seq[:a] + (rng.choice(("AC", "A", "TTG")) * 20)[:36] + seq[a + 36:]
    return seq


# ---- filter: --fastq_filter / --fastx_filter ----------------------------------------------------------------------------------------
def filter_draw(rng):
    from tests import fastq_filter_data as fd
    o, enc = encoding(rng)
    edge, at_edge, anywhere = rng.random() < 1 / 3, int(rng.choice([63, 64, 65, 127, 128, 129])), int(rng.integers(20, 321))
    read_len = at_edge if edge else anywhere
    cfg = dict(n=int(rng.integers(100, 301)), read_len=read_len, paired=bool(rng.random() < 0.3), fasta=bool(rng.random() < 0.15),
               window=int(rng.choice(WINDOWS)), scattered=bool(rng.random() < 0.3), data_seed=seed_of(rng), layout_seed=seed_of(rng), chunk_edge=bool(edge),
               exact_ee=bool(rng.random() < 0.5))
    drawn = fd.draw_opts(np.random.default_rng(seed_of(rng)), read_len)      # (its own stream: draw_opts draws only what it sets)
    for k in ("truncqual", "minqual"):                                       # relative to the lowest quality of the encoding
        if k in drawn:
            drawn[k] += max(o.get("qmin", 0), 0)
    if cfg["fasta"]:
        o, enc = {}, dict(ascii=33, qrange=(0, 41))
        drawn = {k: v for k, v in drawn.items() if k in ("stripleft", "stripright", "trunclen", "trunclen_keep", "minlen", "maxlen", "maxns", "minsize", "maxsize")}
    cfg.update(opts=dict(o, **drawn), enc=enc)
    cfg["cli"] = dict(cfg["opts"], **{k: cfg[k] for k in ("n", "read_len", "paired", "fasta", "window", "scattered")}, qrange=list(enc["qrange"]))
    return cfg


def filter_data(rng, cfg):
    from tests import fastq_filter_data as fd
    s = fd.generate(cfg["data_seed"], cfg["n"], read_len=cfg["read_len"], paired=cfg["paired"], opts=cfg["opts"], **cfg["enc"])
    o = s["opts"]
    if cfg["exact_ee"] and not cfg["fasta"] and ("truncee" in o or "maxee" in o):
        # the bound IS a sum the walk reaches: --fastq_truncee the running sum of one read at one position, --fastq_maxee the
        # expected error of one read, so that `>` and `>=` part on it (a drawn bound never equals a sum)
        r = random.Random(cfg["data_seed"] ^ 0x5EED)
        ascii = o.get("ascii", 33)
        if "truncee" in o:
            q = s["quals"][r.randrange(len(s["quals"]))][o.get("stripleft", 0):]
            ee = 0.0
            for c in q[:r.randrange(len(q)) + 1 if q else 0]:
                ee += 10.0 ** (-(ord(c) - ascii) / 10.0)
            if ee > 0.0:
                o["truncee"] = ee
        if "maxee" in o:
            k = r.randrange(len(s["seqs"]))
            ee = fd.py_analyse(s["seqs"][k], s["quals"][k], {x: v for x, v in o.items() if x not in ("maxee", "maxee_rate")})["ee"]
            if ee > 0.0:
                o["maxee"] = ee
        cfg["cli"].update({k: o[k] for k in ("truncee", "maxee") if k in o})
    if cfg["fasta"]:
        s["quals"] = None
        if cfg["paired"]:
            s["rev_quals"] = None
    return s


def filter_reference(s, cfg):
    from tests import fastq_filter_data as fd
    ref = fd.run_reference(s)
    if ref["returncode"] != 0:
        raise Refused(ref["stderr"][-300:])
    return ref, ref["seconds"], sum(len(ref[k]) for k in ("kept", "discarded", "kept_rev", "discarded_rev"))


def filter_library(al, s, cfg):
    from tests import fastq_filter_data as fd
    from vsearch_amd.filter import FilterResult, filter_reads, last_stats
    if cfg["scattered"]:
        rec, rrec, verdict, c = fd.scattered_call(al, s, cfg["layout_seed"], window=cfg["window"])
        return FilterResult(rec, rrec, verdict, (c["kept"], c["truncated"], c["discarded"]), s["seqs"], s["quals"], s.get("rev_seqs"),
                            s.get("rev_quals"), last_stats())
    a, k = fd.call_args(s)
    return filter_reads(al, *a, **dict(k, window=cfg["window"]))


def filter_compare(res, s, cfg, ref):
    from tests import fastq_filter_data as fd
    mine = fd.library_lines(res, s)
    return diff_of((k, mine[k], ref[k]) for k in ("kept", "discarded", "kept_rev", "discarded_rev", "counts"))


def filter_same(a, b):
    return same_struct(a.records, b.records, "records") or same_struct(a.rev_records, b.rev_records, "rev_records") or \
        first_diff("pair_discarded", a.pair_discarded.tolist(), b.pair_discarded.tolist()) or first_diff("counts", a.counts(), b.counts())


def filter_cover(cfg, s):
    o = cfg["opts"]
    return [k for k, hit in (("paired", cfg["paired"]), ("fasta", cfg["fasta"]), ("ascii64", o.get("ascii") == 64),
                             ("truncee_or_rate", "truncee" in o or "truncee_rate" in o), ("chunk_edge", cfg["chunk_edge"]),
                             ("scattered", cfg["scattered"]),
                             ("exact_ee", cfg["exact_ee"] and not cfg["fasta"] and ("truncee" in o or "maxee" in o))) if hit]


# ---- eestats: --fastq_eestats / --fastq_eestats2 --------------------------------------------------------------------------------------
EE_POOL = [0.001, 0.05, 0.1, 0.25, 0.5, 1.0, 2.0, 3.0, 5.0, 10.0]


def eestats_draw(rng):
    o, enc = encoding(rng)
    cfg = dict(n=int(rng.integers(100, 301)), read_len=int(rng.integers(20, 301)), data_seed=seed_of(rng))
    lo, span, star, step = int(rng.integers(1, 80)), int(rng.integers(0, 250)), rng.random() < 0.5, int(rng.integers(1, 60))
    maybe(rng, o, "length_cutoffs", [lo, None if star else lo + span, step])
    cutoffs = [float(x) for x in rng.permutation(EE_POOL)[:int(rng.integers(1, 7))]]
    maybe(rng, o, "ee_cutoffs", cutoffs)
    cfg.update(opts=o, enc=enc, window=int(rng.choice(WINDOWS)), want=str(rng.choice(["both", "eestats", "eestats2"])))
    cfg["commands"] = ["eestats", "eestats2"] if cfg["want"] == "both" else [cfg["want"]]
    cfg["cli"] = dict(o, **{k: cfg[k] for k in ("n", "read_len", "window", "want")}, qrange=list(enc["qrange"]))
    return cfg


def eestats_data(rng, cfg):
    from tests import eestats_data as ed
    return ed.generate(cfg["data_seed"], cfg["n"], read_len=cfg["read_len"], opts=cfg["opts"], **cfg["enc"])


def eestats_reference(s, cfg):
    from tests import eestats_data as ed
    ref = ed.run_reference(s, cfg["commands"])
    if ref["returncode"] != 0:
        raise Refused(ref["stderr"][-300:])
    return ref, sum(ref["seconds"].values()), sum(len(ref[c]) for c in cfg["commands"])


def eestats_library(al, s, cfg):
    from tests import eestats_data as ed
    return ed.call(al, s, window=cfg["window"], want=cfg["want"])


def eestats_compare(res, s, cfg, ref):
    return diff_of((c, getattr(res, c + "_lines")(), ref[c]) for c in cfg["commands"])


def eestats_same(a, b):
    from tests import eestats_data as ed
    return same_arrays(a, b, ("n", "symbols", "len_min", "len_max", "ee_cutoffs", "length_cutoffs") + ed.TABLES)


def eestats_cover(cfg, s):
    return [k for k, hit in (("ascii64", cfg["opts"].get("ascii") == 64), ("eestats2", "eestats2" in cfg["commands"]),
                             ("window_split", 0 < cfg["window"] < cfg["n"])) if hit]


# ---- fastq_stats: --fastq_stats / --fastq_chars ---------------------------------------------------------------------------------------
def fastq_stats_draw(rng):
    o, enc = encoding(rng, negative_qmin=False)          # (--fastq_stats reads qmin as unsigned: a negative one refuses every read)
    cfg = dict(n=int(rng.integers(100, 301)), read_len=int(rng.integers(1, 301)), data_seed=seed_of(rng), tail=int(rng.integers(1, 13)),
               window=int(rng.choice(WINDOWS)), opts=o, enc=dict(enc, qrange=(max(enc["qrange"][0], 0), enc["qrange"][1])))
    cfg["cli"] = dict(o, **{k: cfg[k] for k in ("n", "read_len", "tail", "window")}, qrange=list(cfg["enc"]["qrange"]))
    return cfg


def fastq_stats_data(rng, cfg):
    from tests import fastq_stats_data as fs
    return fs.generate(cfg["data_seed"], cfg["n"], read_len=cfg["read_len"], opts=cfg["opts"], tail=cfg["tail"], **cfg["enc"])


def fastq_stats_reference(s, cfg):
    from tests import fastq_stats_data as fs
    ref = fs.run_reference(s)
    if ref["returncode"] != 0:
        raise Refused(ref["stderr"][-300:])
    return ref, sum(ref["seconds"].values()), sum(len(ref[c]) for c in fs.BOTH)


def fastq_stats_library(al, s, cfg):
    from tests import fastq_stats_data as fs
    return {c: fs.call(al, s, c, window=cfg["window"]) for c in fs.BOTH}


def fastq_stats_compare(res, s, cfg, ref):
    return diff_of((c, res[c].log_lines(), ref[c]) for c in ("stats", "chars"))


def fastq_stats_same(a, b):
    from tests import fastq_stats_data as fs
    return same_arrays(a["stats"], b["stats"], fs.STATS_FIELDS + fs.STATS_TABLES, "stats") or \
        same_arrays(a["chars"], b["chars"], fs.CHARS_FIELDS + fs.CHARS_TABLES, "chars")


def fastq_stats_cover(cfg, s):
    return ["chars"] + (["ascii64"] if cfg["opts"].get("ascii") == 64 else [])


# ---- derep: --derep_fulllength / --fastx_uniques / --derep_id ------------------------------------------------------------------------
DEREP_KINDS = ["derep_fulllength", "fastx_uniques_fasta", "fastx_uniques_fastq_avg", "fastx_uniques_fastq_max", "derep_id"]


def selection_opts(rng, o, fmt):
    """the options the two dereplication commands share"""
    maybe(rng, o, "sizein", 1, 0.5)
    maybe(rng, o, "minuniquesize", int(rng.integers(2, 5)))
    maybe(rng, o, "maxuniquesize", int(rng.integers(3, 60)))
    maybe(rng, o, "topn", int(rng.integers(1, 50)))
    maybe(rng, o, "minseqlength", int(rng.integers(33, 60)))
    maybe(rng, o, "maxseqlength", int(rng.integers(80, 120)))
    maybe(rng, fmt, "sizeout", True)
    maybe(rng, fmt, "relabel", "Uniq")
    maybe(rng, fmt, "xsize", True)
    maybe(rng, fmt, "fasta_width", int(rng.choice([0, 60])))
    if fmt.get("sizeout"):
        fmt.pop("xsize", None)                           # (the reference refuses the two together)


def derep_draw(rng):
    kind = DEREP_KINDS[int(rng.integers(0, len(DEREP_KINDS)))]
    o, fmt = {}, {}
    maybe(rng, o, "strand_both", 1)
    selection_opts(rng, o, fmt)
    cfg = dict(kind=kind, n=int(rng.integers(300, 1001)), data_seed=seed_of(rng), opts=o, fmt=fmt, hash_bits=hash_cut(rng),
               scattered=bool(rng.random() < 0.3), layout_seed=seed_of(rng), window=int(rng.choice(WINDOWS)))
    if kind.startswith("fastx_uniques_fastq"):
        o["qout_max"] = int(kind.endswith("max"))
    cfg["cli"] = dict(o, **fmt, **{k: cfg[k] for k in ("kind", "n", "hash_bits", "scattered", "window")})
    return cfg


def derep_data(rng, cfg):
    from tests import derep_data as dd
    fastq = cfg["kind"].startswith("fastx_uniques_fastq")
    s = dd.random_set(cfg["n"], cfg["data_seed"], fastq=fastq)
    s["cmd"] = "fastx_uniques" if cfg["kind"].startswith("fastx_uniques") else cfg["kind"]
    s["opts"], s["fmt"], s["name"] = dict(cfg["opts"]), dict(cfg["fmt"]), f"soak_{cfg['data_seed']}"
    if cfg["kind"] == "derep_id":                        # few identifiers: reads that share identifier AND sequence
        r = random.Random(cfg["data_seed"])
        s["labels"] = [f"id{r.randint(0, 5)};size={r.randint(1, 50)}" for _ in s["labels"]]
    return s


def derep_reference(s, cfg, dd=None):
    dd = dd or importlib.import_module("tests.derep_data")
    ref, seconds = timed(dd.run_reference, s)
    return ref, seconds, sum(len(v) for k, v in ref.items() if k != "log")


def derep_library(al, s, cfg):
    from tests import derep_data as dd
    from vsearch_amd import derep
    blob = scattered_blob(cfg["layout_seed"]) if cfg["scattered"] else derep._blob
    with environment(VSX_DEREP_HASH_BITS=cfg["hash_bits"]), patched(derep, "_blob", blob):
        return dd.call(al, s, window=cfg["window"])


def derep_compare(res, s, cfg, ref, dd=None):
    dd = dd or importlib.import_module("tests.derep_data")
    mine = dd.formatted(res, s)
    return diff_of((k, mine.get(k), ref[k]) for k in ref)


def derep_same(a, b, dd=None):
    dd = dd or importlib.import_module("tests.derep_data")
    fa, fb = dd.result_fields(a), dd.result_fields(b)
    return diff_of([(k, fa[k], fb[k]) for k in fa])


def derep_cover(cfg, s):
    return [cfg["kind"].replace("_fasta", "").replace("_fastq_avg", "").replace("_fastq_max", "")] + \
        [k for k, hit in (("fastq", "fastq" in cfg["kind"]), ("strand_both", cfg["opts"].get("strand_both")), ("hash_cut", cfg["hash_bits"])) if hit]


# ---- derep_prefix -------------------------------------------------------------------------------------------------------------------
def derep_prefix_draw(rng):
    o, fmt = {}, {}
    selection_opts(rng, o, fmt)
    cfg = dict(n=int(rng.integers(300, 1001)), data_seed=seed_of(rng), opts=o, fmt=fmt, hash_bits=hash_cut(rng), window=int(rng.choice(WINDOWS)))
    cfg["cli"] = dict(o, **fmt, **{k: cfg[k] for k in ("n", "hash_bits", "window")})
    return cfg


def derep_prefix_data(rng, cfg):
    from tests import derep_prefix_data as dp
    s = dp.random_set(cfg["n"], cfg["data_seed"])
    s["opts"], s["fmt"], s["name"] = dict(cfg["opts"]), dict(cfg["fmt"]), f"soak_{cfg['data_seed']}"
    return s


def derep_prefix_library(al, s, cfg):
    from tests import derep_prefix_data as dp
    with environment(VSX_DEREP_PREFIX_HASH_BITS=cfg["hash_bits"]):
        return dp.call(al, s, window=cfg["window"])


def derep_prefix_cover(cfg, s):
    return [k for k, hit in (("hash_cut", cfg["hash_bits"]), ("topn", "topn" in cfg["opts"]), ("sizein", cfg["opts"].get("sizein"))) if hit]


# ---- search_exact -------------------------------------------------------------------------------------------------------------------
def search_exact_draw(rng):
    o = {}
    if rng.random() < 0.3:
        o["strand_both"] = 0
    qmask, dbmask = MASKS[int(rng.integers(0, 3))], MASKS[int(rng.integers(0, 3))]
    maybe(rng, o, "qmask", qmask, 0.5)
    maybe(rng, o, "dbmask", dbmask, 0.5)
    maybe(rng, o, "hardmask", 1)
    maybe(rng, o, "sizein", 1)
    cfg = dict(n_db=int(rng.integers(200, 601)), n_q=int(rng.integers(200, 401)), data_seed=seed_of(rng), opts=o, window=int(rng.choice(WINDOWS)))
    cfg["cli"] = dict(o, **{k: cfg[k] for k in ("n_db", "n_q", "window")})
    return cfg


def search_exact_data(rng, cfg):
    """a database with repeated entries, IUPAC codes, lower-case and low-complexity stretches; queries: exact copies on either
    strand, copies in the other case, copies one substitution away"""
    from tests import search_exact_data as sd
    r = random.Random(cfg["data_seed"])
    base = []
    for _ in range(max(1, cfg["n_db"] * 3 // 4)):
        seq = mask_stretches(r, sd.random_seq(r, r.randint(30, 120)))
        if r.random() < 0.2:
            p = r.randrange(len(seq))
            seq = seq[:p] + r.choice("RYSWKMDBHVNU") + seq[p + 1:]
        base.append(seq)
    db = [base[k] if k < len(base) else r.choice(base) for k in range(cfg["n_db"])]
    qs = []
    for _ in range(cfg["n_q"]):
        seq, x = r.choice(db), r.random()
        if x < 0.3:
            pass
        elif x < 0.55:
            seq = sd.revcomp(seq)
        elif x < 0.65:
            seq = seq.swapcase()
        else:
            p = r.randrange(len(seq))
            seq = seq[:p] + r.choice([c for c in "ACGT" if c != seq[p].upper()]) + seq[p + 1:]
        qs.append(seq)
    sizein = cfg["opts"].get("sizein", 0)
    return sd._set(f"soak_{cfg['data_seed']}", db, qs, cfg["opts"], db_sizes=[r.randint(1, 9) for _ in db] if sizein else None,
                   sizes=[r.randint(1, 9) for _ in qs] if sizein else None)


def search_exact_reference(s, cfg):
    from tests import search_exact_data as sd
    ref, seconds = timed(sd.run_reference, s, threads=1)
    return ref, seconds, len(ref["userout"]) + len(ref["uc"])


def search_exact_library(al, s, cfg):
    from tests import search_exact_data as sd
    kw = sd.session_opts(s["opts"])
    if al is None:
        from vsearch_amd.search import search_exact_host
        return search_exact_host(s["db"], s["queries"], db_sizes=s["db_sizes"], db_labels=s["db_names"], sizes=s["sizes"], labels=s["names"], **kw)
    from vsearch_amd import SearchSession
    sess = SearchSession(al, s["db"], sizes=s["db_sizes"], labels=s["db_names"], window=cfg["window"], **kw)
    try:
        hits = sess.search_exact(s["queries"], sizes=s["sizes"], labels=s["names"])
        st = sess.exact_stats
        if st["queries_host"] != 0 or st["queries_device"] != len(s["queries"]):
            raise Fatal(f"search_exact: the device route did not answer: {st}")
        return hits
    finally:
        sess.close()


def search_exact_compare(hits, s, cfg, ref):
    from tests import search_exact_data as sd
    dbm, unique, total = sd.summary_of(s, hits)
    ref_unique, ref_total = sd.log_counts(ref["log"])   # (the log has the line of the abundances only with --sizein)
    return diff_of([("userout", sd.userout_lines(s, hits), ref["userout"]), ("uc", sd.uc_lines(s, hits), ref["uc"]),
                    ("dbmatched", dbm, ref["dbmatched"]), ("log", unique, ref_unique), ("log_total", total if ref_total else None, ref_total)])


def search_exact_same(a, b):
    return first_diff("hits", a, b)


def search_exact_cover(cfg, s):
    o = cfg["opts"]
    return [k for k, hit in (("dust", "dust" in (o.get("qmask"), o.get("dbmask"))), ("hardmask", o.get("hardmask")),
                             ("strand_both", o.get("strand_both", 1))) if hit]


# ---- orient -------------------------------------------------------------------------------------------------------------------------
def orient_draw(rng):
    o = {}
    low, high = int(rng.integers(3, 13)), int(rng.integers(13, 16))
    o["wordlength"] = high if rng.random() < 0.1 else low
    qmask, dbmask = MASKS[int(rng.integers(0, 3))], MASKS[int(rng.integers(0, 3))]
    maybe(rng, o, "qmask", qmask, 0.5)
    maybe(rng, o, "dbmask", dbmask, 0.5)
    for flag in ("hardmask", "sizein", "sizeout", "xsize"):
        maybe(rng, o, flag, 1)
    maybe(rng, o, "relabel", "read")
    maybe(rng, o, "fasta_width", int(rng.choice([0, 60])))
    if o.get("sizeout"):
        o.pop("xsize", None)
    cfg = dict(n_db=int(rng.integers(50, 201)), n_q=int(rng.integers(100, 301)), db_len=int(rng.integers(150, 400)), data_seed=seed_of(rng),
               fastq=bool(rng.random() < 0.3), opts=o, hash_bits=hash_cut(rng, (None, 3)), window=int(rng.choice(WINDOWS)))
    keys = int(rng.integers(500, 5000))
    cfg["build_keys"] = keys if rng.random() < 0.3 else None
    cfg["cli"] = dict(o, **{k: cfg[k] for k in ("n_db", "n_q", "db_len", "fastq", "hash_bits", "build_keys", "window")})
    return cfg


def orient_data(rng, cfg):
    from tests import orient_data as od
    r = random.Random(cfg["data_seed"])
    read_len = r.randint(40, cfg["db_len"])
    db, reads = od.simulated(cfg["data_seed"], cfg["n_db"], cfg["db_len"], cfg["n_q"], read_len)
    db = [mask_stretches(r, t) for t in db]
    reads = [mask_stretches(r, q) if r.random() < 0.2 else q for q in reads]
    for k in range(0, len(reads), 37):                   # short reads, none at all, ambiguity codes
        reads[k] = r.choice(["", "ACGT", reads[k][:r.randint(1, 20)], reads[k].replace("A", "N", 3)])
    labels = [f"q{k}" + (f";size={r.randint(1, 99)}" if r.random() < 0.6 else "") + (";" if r.random() < 0.2 else "") for k in range(len(reads))]
    quals = ["".join(chr(33 + r.randrange(41)) for _ in q) for q in reads] if cfg["fastq"] else None
    return od._set(f"soak_{cfg['data_seed']}", db, reads, cfg["opts"], labels, quals)


def orient_reference(s, cfg):
    from tests import orient_data as od
    ref, seconds = timed(od.run_reference, s)
    return ref, seconds, sum(len(v) for k, v in ref.items() if v is not None and k != "log")


def orient_library(al, s, cfg):
    from tests import orient_data as od
    from vsearch_amd.orient import orient, orient_host, orient_session
    o = od.full_opts(s["opts"])
    kw = dict(wordlength=o["wordlength"], soft_mask=od.MASK_MODES[o["dbmask"]], hardmask=1 if o["hardmask"] else 0)
    if al is None:
        return orient_host(s["db"], s["queries"], quals=s["quals"], qmask=o["qmask"], **kw)
    with environment(VSX_ORIENT_BUILD_KEYS=cfg["build_keys"], VSX_ORIENT_HASH_BITS=cfg["hash_bits"]):
        sess = orient_session(al, s["db"], **kw)
        try:
            res = orient(sess, s["queries"], quals=s["quals"], qmask=o["qmask"], window=cfg["window"])
        finally:
            sess.close()
    n, host = len(s["queries"]), o["wordlength"] > 12
    if res.stats["queries_host_wordlength"] != (n if host else 0) or res.stats["queries_device"] != (0 if host else n):
        raise Fatal(f"orient: the route counters do not fit word length {o['wordlength']}: {res.stats}")
    return res


def orient_compare(res, s, cfg, ref):
    from tests import orient_data as od
    from vsearch_amd.orient import fasta_lines, fastq_lines, log_lines, notmatched_lines, tabbed_lines
    kw = od.writer_kw(s)
    pairs = [("tabbed", tabbed_lines(res, s["qlabels"]), ref["tabbed"]), ("fasta", fasta_lines(res, s["qlabels"], **kw), ref["fasta"]),
             ("notmatched", notmatched_lines(res, s["qlabels"], **kw), ref["notmatched"]), ("log", log_lines(res), ref["log"])]
    if s["quals"] is not None:
        pairs.append(("fastq", fastq_lines(res, s["qlabels"], **kw), ref["fastq"]))
    return diff_of(pairs)


def orient_same(a, b):
    return same_arrays(a, b, ("count_fwd", "count_rev", "strand", "n_fwd", "n_rev", "n_none", "text", "qual"))


def orient_cover(cfg, s):
    w = cfg["opts"]["wordlength"]
    return [k for k, hit in (("wl_le_5", w <= 5), ("wl_12", w == 12), ("wl_host", w > 12), ("fastq", cfg["fastq"]), ("hash_cut", cfg["hash_bits"]),
                             ("build_chunks", cfg["build_keys"])) if hit]


# ---- sintax -------------------------------------------------------------------------------------------------------------------------
def sintax_draw(rng):
    o = dict(seed=int(rng.integers(1, 1000)), cutoff=float(rng.choice([0.0, 0.5, 0.8, 1.0])), strand_both=int(rng.random() < 0.5))
    low, high = int(rng.integers(3, 9)), int(rng.integers(9, 13))
    o["wordlength"] = high if rng.random() < 0.1 else low
    dbmask = MASKS[int(rng.integers(0, 3))]
    maybe(rng, o, "dbmask", dbmask, 0.5)               # (no --hardmask: the reference's command line refuses it for --sintax)
    cfg = dict(families=int(rng.integers(10, 26)), n_q=int(rng.integers(100, 201)), data_seed=seed_of(rng), opts=o, window=int(rng.choice([0, 7, 64])))
    cfg["cli"] = dict(o, **{k: cfg[k] for k in ("families", "n_q", "window")})
    return cfg


def sintax_data(rng, cfg):
    """families x 4 genera x 5 or 6 species (200-600 references 3 % apart; every tenth an exact copy of its neighbour, another
    tenth a shortened or lengthened copy: tied counts); taxonomy strings cut at a random rank for a third of them"""
    from tests import sintax_data as sd
    r = random.Random(cfg["data_seed"])
    db, labels = sd.taxonomy_db(r, families=cfg["families"], genera=4, species=r.choice([5, 6]), length=r.randint(150, 300))
    for k in range(9, len(db), 10):                      # equal counts: a copy (the lower number wins) ...
        db[k] = db[k - 1]
    for k in range(4, len(db), 10):                      # ... and, wherever a read lies in the shared part, a shorter or a longer
        cut = r.randint(10, 60)                          # copy before or behind the other (the shorter wins)
        db[k] = db[k - 1][:-cut] if k % 20 == 4 else db[k - 1] + sd.random_seq(r, cut)
        if r.random() < 0.5:
            db[k - 1], db[k] = db[k], db[k - 1]
    db = [mask_stretches(r, t) for t in db]
    for k, l in enumerate(labels):
        if r.random() < 0.33:
            head, tax = l.rstrip(";").split(";tax=")
            ranks = tax.split(",")
            labels[k] = f"{head};tax={','.join(ranks[:r.randint(1, len(ranks))])};"
    qs = []
    for _ in range(cfg["n_q"]):
        x, t = r.random(), r.choice(db)
        a = r.randrange(0, max(1, len(t) - 60))
        piece = sd.mutate(r, t[a:a + r.randint(40, 200)].upper(), r.choice([0.0, 0.02, 0.05]))
        qs.append(sd.random_seq(r, r.randint(5, 150)) if x < 0.1 else sd.revcomp(piece) if x < 0.5 else piece)
    return sd._set(f"soak_{cfg['data_seed']}", db, labels, qs, cfg["opts"])


def sintax_reference(s, cfg):
    from tests import sintax_data as sd
    ref, seconds = timed(sd.run_reference, s)
    return ref, seconds, len(ref["tabbed"])


def sintax_library(al, s, cfg):
    from tests import sintax_data as sd
    from vsearch_amd import SearchSession, sintax, sintax_host
    o = sd.full_opts(s["opts"])
    kw = dict(randseed=o["seed"], strand_both=o["strand_both"], sintax_random=o["random"], want_candidates=True)
    db = dict(wordlength=o["wordlength"], soft_mask=sd.MASK_MODES[o["dbmask"]], hardmask=1 if o["hardmask"] else 0)
    if al is None:
        return sintax_host(s["db"], s["db_labels"], s["queries"], **kw, **db)
    sess = SearchSession(al, s["db"], labels=s["db_labels"], id=0.97, **db)
    try:
        res = sintax(sess, s["queries"], window=cfg["window"], **kw)
    finally:
        sess.close()
    route = "queries_host_wordlength" if o["wordlength"] > 8 else "queries_device"
    if res.stats[route] != len(s["queries"]):
        raise Fatal(f"sintax: the route counters do not fit word length {o['wordlength']}: {res.stats}")
    return res


def sintax_compare(res, s, cfg, ref):
    from tests import sintax_data as sd
    from vsearch_amd import log_lines, tabbed_lines
    return diff_of([("tabbed", tabbed_lines(res, s["qlabels"], s["db_labels"], sd.full_opts(s["opts"])["cutoff"]), ref["tabbed"]),
                    ("log", log_lines(res), ref["log"])])


def sintax_same(a, b):
    fa, fb = a.fields(), b.fields()
    if set(fa) != set(fb):
        return {"what": "device and host: other fields"}
    for k in fa:
        if not np.array_equal(fa[k], fb[k]) or bits(fa[k]) != bits(fb[k]):
            return {"what": f"device and host: {k} differs"}
    return first_diff("n_classified", a.n_classified, b.n_classified)


def sintax_cover(cfg, s):
    o = cfg["opts"]
    return [k for k, hit in (("strand_both", o["strand_both"]), ("cutoff", o["cutoff"] > 0), ("wl_lt_8", o["wordlength"] < 8),
                             ("wl_host", o["wordlength"] > 8)) if hit]


# ---- otutab: --otutabout / --biomout / --mothur_shared_out --------------------------------------------------------------------------
def otutab_draw(rng):
    cfg = dict(draws=int(rng.integers(1, 41)), data_seed=seed_of(rng), sizein=bool(rng.random() < 0.5), hash_bits=hash_cut(rng))
    cfg["cli"] = {k: cfg[k] for k in ("draws", "data_seed", "sizein", "hash_bits")}
    return cfg


def otutab_data(rng, cfg):
    """the labels of `draws` otutab_data.random_label_set()s side by side as one --search_exact run: every query has the sequence
    of the target it hits (its own otherwise), abundances stand in the labels as ;size=N.  The CLI takes no empty header."""
    from tests import otutab_data as od
    r = random.Random(cfg["data_seed"])
    q, t, hit = [], [], []
    for _ in range(cfg["draws"]):
        lq, lt, q_target, _, _ = od.random_label_set(r.randrange(1 << 30))
        hit += [None if x == od.NONE else int(x) + len(t) for x in q_target]
        q += lq
        t += lt
    if not t:
        t.append(b"otu=alone")
    if not q:
        q, hit = [b"r;sample=alone"], [0]
    size = lambda: b";size=%d" % r.choice((1, 2, 7, 50, 3000000000)) if r.random() < 0.5 else b""      # noqa: E731
    q = [(l or b"q%d" % k) + size() for k, l in enumerate(q)]
    t = [(l or b"t%d" % k) + size() for k, l in enumerate(t)]
    return od.search_set(f"soak_{cfg['data_seed']}", q, t, hit, sizein=cfg["sizein"])


def otutab_reference(s, cfg):
    from tests import otutab_data as od
    ref, seconds = timed(od.run_reference, s)
    return ref, seconds, sum(v.count("\n") for v in ref.values())


def otutab_library(al, s, cfg):
    from tests import otutab_data as od
    if al is None:
        return od.call(None, s, host=True)
    with environment(VSX_OTUTAB_HASH_BITS=cfg["hash_bits"]):
        res = od.call(al, s)
    if res.stats["labels_host"] != 0:
        raise Fatal(f"otutab: the device route did not answer: {res.stats}")
    return res


def otutab_compare(res, s, cfg, ref):
    from tests import otutab_data as od
    text = od.texts(res, generated_by=od.generated_by(ref["biom"]))
    return diff_of([("otutabout", text["otutabout"].splitlines(), ref["otutabout"].splitlines()),
                    ("mothur", text["mothur"].splitlines(), ref["mothur"].splitlines()),
                    ("biom", od.mask_date(text["biom"]).splitlines(), od.mask_date(ref["biom"]).splitlines()),
                    ("bytes", [text["otutabout"], text["mothur"], od.mask_date(text["biom"])], [ref["otutabout"], ref["mothur"], od.mask_date(ref["biom"])])])


def otutab_same(a, b):
    return None if a.arrays() == b.arrays() else {"what": "device and host: arrays differ"}


def otutab_cover(cfg, s):
    return ["biom", "mothur"] + (["hash_cut"] if cfg["hash_bits"] else [])


# ---- hitout: the seven hit writers of --usearch_global -----------------------------------------------------------------------------
_ALIGNERS = {}


def hitout_draw(rng):
    o, fmt = {}, {}
    if rng.random() < 0.3:
        o["strand_both"] = 0
    qmask, dbmask = MASKS[int(rng.integers(0, 3))], MASKS[int(rng.integers(0, 3))]
    maybe(rng, o, "qmask", qmask, 0.5)
    maybe(rng, o, "dbmask", dbmask, 0.5)
    maybe(rng, o, "hardmask", 1)
    maybe(rng, o, "n_mismatch", 1)
    fmt["rowlen"] = int(rng.choice([0, 1, 64, 80]))
    maybe(rng, fmt, "maxhits", int(rng.integers(1, 4)))
    maybe(rng, fmt, "top_hits_only", 1)
    maybe(rng, fmt, "output_no_hits", 1)
    maybe(rng, fmt, "fasta_width", int(rng.choice([0, 60])))
    cfg = dict(opts=o, fmt=fmt, id=float(rng.choice([0.7, 0.9])), maxaccepts=int(rng.integers(1, 5)), window=int(rng.choice([0, 1, 7])),
               data_seed=seed_of(rng))
    cfg["cli"] = dict(o, **fmt, **{k: cfg[k] for k in ("id", "maxaccepts", "window", "data_seed")})
    return cfg


def hitout_data(rng, cfg):
    from tests import hitout_data as hd
    return hd._cli(f"soak_{cfg['data_seed']}", opts=cfg["opts"], fmt=cfg["fmt"], search_args=("--id", str(cfg["id"]), "--maxaccepts", str(cfg["maxaccepts"])),
                   inputs=hd.live_inputs(cfg["data_seed"], 200, 200))


def hitout_reference(s, cfg):
    from tests import hitout_data as hd
    ref, seconds = timed(hd.run_reference, s)
    cfg["ref"] = ref                                     # (the host route renders the CLI's own hit list)
    return ref, seconds, sum(ref[w].count("\n") for w in hd.WRITERS)


def hitout_library(al, s, cfg):
    from tests import hitout_data as hd
    from vsearch_amd import hitout as ho
    o = hd.full_opts(s["opts"])
    if al is None:
        raw = hd.raw_hits(len(s["queries"]), hd.hits_from_records(s, cfg["ref"]["records"]))
        return ho.render_host(hd.db_text(s), s["queries"], raw, n_mismatch=bool(o["n_mismatch"]), **hd.session_opts(s["opts"]))
    from vsearch_amd import Aligner, SearchSession
    if o["n_mismatch"]:
        if "n_mismatch" not in _ALIGNERS:
            _ALIGNERS["n_mismatch"] = Aligner(n_mismatch=True)
        al = _ALIGNERS["n_mismatch"]
    sess = SearchSession(al, s["db"], id=cfg["id"], maxaccepts=cfg["maxaccepts"], **hd.session_opts(s["opts"]))
    try:
        raw = sess.search_batch_raw(s["queries"])
        text = ho.render(sess, s["queries"], raw, window=cfg["window"])
    finally:
        sess.close()
    if text.stats["hits_host"] != 0 or text.stats["hits_device"] != len(raw[1]):
        raise Fatal(f"hitout: the device route did not answer: {text.stats}")
    return text


def hitout_compare(text, s, cfg, ref):
    from tests import hitout_data as hd
    got = hd.format_all(text, s)
    pairs = [(name, got[name].splitlines(True), ref[name].splitlines(True)) for name in hd.WRITERS + ("userout_reversed",)]
    return diff_of(pairs + [("samheader", hd.sam_header_of(text, s, ref["samheader"]), ref["samheader"])])


def hitout_same(a, b):
    d = a.same_as(b)
    return None if d is None else {"what": f"device and host: {d} differs"}


def hitout_cover(cfg, s):
    o, f = cfg["opts"], cfg["fmt"]
    return [k for k, hit in (("hardmask", o.get("hardmask")), ("minus_strand", o.get("strand_both", 1)), ("rowlen0", f["rowlen"] == 0),
                             ("n_mismatch", o.get("n_mismatch")), ("window1", cfg["window"] == 1)) if hit]


# ---- what mask, getseqs and cut share --------------------------------------------------------------------------------------------
SMALL_WINDOWS = [0, 1, 7, 64]


def writer_opts(rng, o, relabel):
    """--sizeout / --xsize / --relabel and --fasta_width 0 / 60 / 80 of the FASTA writers"""
    for flag in ("sizeout", "xsize"):
        maybe(rng, o, flag, 1)
    maybe(rng, o, "relabel", relabel)
    o["fasta_width"] = int(rng.choice([0, 60, 80]))
    if o.get("sizeout"):
        o.pop("xsize", None)                             # (the reference refuses the two together)


def asserted(fn, *a):
    """an assert_* helper of tests/*_data.py as a mismatch record, or None"""
    try:
        fn(*a)
    except AssertionError as e:
        return {"what": f"{fn.__name__}: {str(e)[:400]}"}
    return None


def scattered_labels(labels, seed):
    """a LabelBlob of the labels in another order with gaps between them; equal labels share one span half of the time"""
    from vsearch_amd.otutab import LabelBlob
    rng = random.Random(seed)
    order = list(range(len(labels)))
    rng.shuffle(order)
    off, parts, at, seen = np.zeros(len(labels), np.uint64), [], 0, {}
    for k in order:
        if labels[k] in seen and rng.random() < 0.5:
            off[k] = seen[labels[k]]
            continue
        gap = rng.randint(0, 5)
        parts.append(b"S" * gap + labels[k])
        off[k] = seen[labels[k]] = at + gap
        at += gap + len(labels[k])
    return LabelBlob.of(b"".join(parts) + b";S1", off, [len(l) for l in labels])


# ---- mask: --fastx_mask / --maskfasta ------------------------------------------------------------------------------------------------
MASK_HOST_ROUTES = ("sequences_host_forced", "sequences_host_memory", "sequences_host_long")


def mask_draw(rng):
    o = dict(qmask=MASKS[int(rng.integers(0, 3))])
    maybe(rng, o, "hardmask", 1)
    low, high = float(rng.integers(5, 60)), float(rng.integers(60, 100))
    maybe(rng, o, "min_unmasked_pct", low)
    maybe(rng, o, "max_unmasked_pct", high)
    writer_opts(rng, o, "M")
    cfg = dict(command="maskfasta" if rng.random() < 0.3 else "fastx_mask", n=int(rng.integers(100, 301)), fastq=bool(rng.random() < 0.3),
               length_edge=bool(rng.random() < 1 / 3), percent_exact=bool(rng.random() < 0.5), window=int(rng.choice(SMALL_WINDOWS)),
               scattered=bool(rng.random() < 0.3), data_seed=seed_of(rng), layout_seed=seed_of(rng), opts=o)
    long_min, segment = int(rng.choice([1, 64, 200])), int(rng.choice([64, 192, 256]))
    cfg["long"] = [long_min, segment] if rng.random() < 0.3 else None
    cfg["cli"] = dict(o, **{k: cfg[k] for k in ("command", "n", "fastq", "length_edge", "percent_exact", "window", "scattered", "long", "data_seed")})
    return cfg


def mask_data(rng, cfg):
    """sequences of 1 .. 600 symbols with low-complexity islands, lower-case stretches, N and IUPAC codes; in a third of the rounds
    every length is one at which the window loop or the long route's segments change shape.  percent_exact: the two bounds ARE the
    percentages of two of the round's sequences (py_fastx_mask), so that `<` and `<=` part on them"""
    from tests import fastx_mask_data as md
    r = random.Random(cfg["data_seed"])
    kw = dict(alphabet="ACGTacgtNRYU", lower=0.2)
    if cfg["length_edge"]:
        seqs = [md.island_seq(r, r.choice(md.LENGTHS + md.SEGMENT_LENGTHS), **kw) for _ in range(cfg["n"])]
    else:
        seqs = md.seeded_sequences(cfg["data_seed"], cfg["n"], 1, 600, **kw)
    labels = [f"s{k}" + (f";size={r.randint(1, 99)}" if r.random() < 0.6 else "") for k in range(len(seqs))]
    quals = [md.quality(r, len(x)) for x in seqs] if cfg["fastq"] else None
    o = dict(cfg["opts"])
    if cfg["percent_exact"]:
        exact = sorted(100.0 * md.py_fastx_mask([seqs[k]], o["qmask"], o.get("hardmask", 0))["unmasked"][0] / len(seqs[k])
                       for k in r.sample(range(len(seqs)), 4))
        o["min_unmasked_pct"], o["max_unmasked_pct"] = exact[1], exact[2]
        cfg["cli"].update(min_unmasked_pct=exact[1], max_unmasked_pct=exact[2])
    return md._set(f"soak_{cfg['data_seed']}", seqs, o, labels=labels, quals=quals)


def mask_reference(s, cfg):
    from tests import fastx_mask_data as md
    ref, seconds = timed(md.run_reference, s, ("maskfasta",) if cfg["command"] == "maskfasta" else ("fasta", "fastq", "log"))
    counts = {w: int(l.split()[0]) for l in ref.get("log", ()) for w in ("less", "more") if f"with {w} than" in l}
    cfg["cover_after"] = ["discarded"] if counts.get("less", 0) > 0 and counts.get("more", 0) > 0 else []
    return ref, seconds, sum(len(v) for v in ref.values() if v is not None)


def mask_library(al, s, cfg):
    from tests import fastx_mask_data as md
    from vsearch_amd import mask as mk
    if al is None:
        return md.call(None, s, window=cfg["window"])
    long_min, segment = cfg["long"] or (None, None)
    with environment(VSX_MASK_LONG_MIN=long_min, VSX_MASK_SEGMENT=segment):
        if cfg["scattered"]:
            blob = scattered_blob(cfg["layout_seed"], b"A")          # (gaps of A: a window that leaves its sequence meets a run)
            quals = None if s["quals"] is None else blob(s["quals"])[0]
            res = mk.fastx_mask(al, blob(s["seqs"]), quals=quals, window=cfg["window"], **md.mask_kw(s))
        else:
            res = md.call(al, s, window=cfg["window"])
    st = res.stats
    if sum(st[r] for r in MASK_HOST_ROUTES) != 0 or st["sequences"] != len(s["seqs"]):
        raise Fatal(f"mask: the device route did not answer: {st}")
    if cfg["long"] and md.full_opts(s["opts"])["qmask"] == "dust" and max(len(x) for x in s["seqs"]) >= long_min:
        if st["sequences_long"] == 0 or st["segment"] != segment:
            raise Fatal(f"mask: VSX_MASK_LONG_MIN={long_min} VSX_MASK_SEGMENT={segment}, and no sequence took the long route: {st}")
    return res


def mask_compare(res, s, cfg, ref):
    from tests import fastx_mask_data as md
    from vsearch_amd import mask as mk
    kw, o = md.writer_kw(s), md.full_opts(s["opts"])
    if cfg["command"] == "maskfasta":
        return diff_of([("maskfasta", mk.maskfasta_lines(res, s["labels"], **kw), ref["maskfasta"])])
    pairs = [("fasta", mk.fasta_lines(res, s["labels"], **kw), ref["fasta"]),
             ("log", mk.log_lines(res, o["min_unmasked_pct"], o["max_unmasked_pct"]), ref["log"])]
    if s["quals"] is not None:
        pairs.append(("fastq", mk.fastq_lines(res, s["labels"], **kw), ref["fastq"]))
    return diff_of(pairs)


def mask_same(a, b):
    from tests import fastx_mask_data as md
    return asserted(md.assert_same, a, b, "device and host") or first_diff("device and host: bytes", a.tobytes() == b.tobytes(), True)


def mask_cover(cfg, s):
    o, fastx = s["opts"], cfg["command"] == "fastx_mask"
    return [k for k, hit in (("dust", o["qmask"] == "dust"), ("soft", o["qmask"] == "soft"), ("hardmask", o.get("hardmask")),
                             ("percent_exact", cfg["percent_exact"] and fastx), ("fastq", cfg["fastq"] and fastx), ("maskfasta", not fastx),
                             ("long_route", cfg["long"] and o["qmask"] == "dust"), ("length_edge", cfg["length_edge"])) if hit]


# ---- getseqs: --fastx_getseqs / --fastx_getseq / --fastx_getsubseq ---------------------------------------------------------------------
GETSEQS_COMMANDS = ["fastx_getseq", "fastx_getseqs", "fastx_getsubseq"]
HEADER_EDGES = (63, 64, 65, 127, 128, 129)
GETSEQS_FIELDS = [None, "sample", "size", "xsample"]


def getseqs_draw(rng):
    """the reference takes --label alone for --fastx_getseq and --fastx_getsubseq, the subsequence options only with the latter, and
    any one of the four with --fastx_getseqs (checked with --reference-only): another mode than `label` makes the command
    --fastx_getseqs, and only --fastx_getsubseq carries a subsequence.  --label_field goes with the word modes"""
    from tests import getseqs_data as gd
    mode, command = gd.MODES[int(rng.integers(0, 4))], GETSEQS_COMMANDS[int(rng.integers(0, 3))]
    substr, field = bool(rng.random() < 0.5), GETSEQS_FIELDS[int(rng.integers(0, len(GETSEQS_FIELDS)))]
    start, span, past = int(rng.integers(1, 40)), int(rng.integers(0, 40)), bool(rng.random() < 0.3)
    w = {}
    for flag in ("sizeout", "xsize", "sizein"):
        maybe(rng, w, flag, True)
    maybe(rng, w, "relabel", "kept")
    w["fasta_width"] = int(rng.choice([0, 60, 80]))
    if w.get("sizeout"):
        w.pop("xsize", None)
    if mode != "label":
        command = "fastx_getseqs"
    cfg = dict(mode=mode, command=command, substr=substr, field=field if mode.startswith("label_word") else None,
               subseq=[start, 1000 if past else start + span] if command == "fastx_getsubseq" else None, past_end=past,
               writer=dict(gd.WRITER_DEFAULTS, **w), n=int(rng.integers(200, 601)), n_needles=int(rng.integers(1, 41)), fastq=bool(rng.random() < 0.3),
               hash_bits=hash_cut(rng), lengths_host=bool(rng.random() < 0.1), window=int(rng.choice(SMALL_WINDOWS)),
               scattered=bool(rng.random() < 0.3), data_seed=seed_of(rng), layout_seed=seed_of(rng))
    cfg["cli"] = dict(w, **{k: cfg[k] for k in ("mode", "command", "substr", "field", "subseq", "n", "n_needles", "fastq", "hash_bits", "lengths_host",
                                                "window", "scattered", "data_seed")})
    return cfg


def getseqs_needles(r, heads, count):
    """needles cut from the headers: whole labels, words, pieces across a ';' or '=', the case swapped in half of them; misses; one
    needle of 63 .. 65 bytes"""
    import re
    out = []
    for _ in range(count):
        h, x = r.choice(heads), r.random()
        nd = h
        if 0.3 <= x < 0.6:
            nd = r.choice([w for w in re.split(rb"[^0-9A-Za-z]+", h) if w])
        elif 0.6 <= x < 0.85:
            marks = [i for i, c in enumerate(h) if c in b";="]
            if marks:
                p = r.choice(marks)
                nd = h[max(0, p - r.randint(1, 4)):p + 1 + r.randint(1, 4)]
        elif x >= 0.85:
            nd = b"miss%d" % r.randrange(1000)
        out.append(nd.swapcase() if r.random() < 0.5 else nd)
    L = r.choice((63, 64, 65))
    long = [h for h in heads if len(h) >= L]
    out.insert(r.randrange(len(out) + 1), r.choice(long)[:L] if long else b"Q" * L)
    return out


def getseqs_data(rng, cfg):
    """headers in the style of tests/test_gpu_getseqs.live_reads(), every seventh padded to 63 / 64 / 65 / 127 / 128 / 129 bytes;
    sequences of 1 .. 60 symbols; for the list modes a labels file with blank lines and, half of the time, no final newline"""
    from tests import getseqs_data as gd
    r = random.Random(cfg["data_seed"])
    heads, seqs, quals = [], [], []
    for k in range(cfg["n"]):
        name = r.choice((b"read%d" % k, b"OTU_%d" % r.randrange(300), b"otu_%d" % r.randrange(300)))
        tail = r.choice((b"", b";sample=S%d" % r.randrange(30), b";xsample=S%d;tax=k:B,g:G_%d" % (r.randrange(30), r.randrange(9)),
                         b";sample=S%dx;size=%d" % (r.randrange(30), r.randrange(1, 50)), b"_S%d;sample=s%d;" % (r.randrange(30), r.randrange(30))))
        h = b"OTU_7" if k % 97 == 0 else name + tail
        if k % 7 == 3:
            L = r.choice(HEADER_EDGES)
            h = (h + b";pad=" + gd.filler(L))[:L]
        heads.append(h)
        L = r.randrange(1, 61)
        seqs.append("".join(r.choice("ACGT") for _ in range(L)))
        quals.append("".join(chr(r.randrange(48, 74)) for _ in range(L)))
    needles = getseqs_needles(r, heads, cfg["n_needles"])
    raw = None
    if cfg["mode"] in gd.SINGLE:
        needles = needles[:1]
    else:
        parts = []
        for nd in needles:
            parts += [b"", nd] if r.random() < 0.15 else [nd]
        raw = b"\n".join(parts) + (b"" if r.random() < 0.5 else b"\n")
        needles = gd.py_read_labels(raw)[0]
    s = dict(name=f"soak_{cfg['data_seed']}", headers=heads, seqs=seqs, quals=quals if cfg["fastq"] else None, mode=cfg["mode"], needles=needles,
             raw=raw, substr=cfg["substr"], field=cfg["field"], subseq=tuple(cfg["subseq"]) if cfg["subseq"] else None, writer=cfg["writer"])
    # the host answers a call with more distinct needle lengths than VSX_GETSEQS_MAX_LENGTHS, unless it compares whole headers
    distinct = len({len(nd) for nd in needles})
    exact = cfg["mode"] in ("label", "labels") and not cfg["substr"]
    s["max_lengths"] = distinct - 1 if cfg["lengths_host"] and distinct >= 2 and not exact else None
    return s


def getseqs_reference(s, cfg):
    from tests import getseqs_data as gd
    ref, seconds = timed(gd.run_cli, s["headers"], s["seqs"], s["quals"], s["mode"], s["needles"], s["raw"], s["substr"], s["field"], s["subseq"],
                         s["writer"], command=cfg["command"])
    cfg["cover_after"] = ["notmatched"] if ref["fastaout"] and ref["notmatched"] else []
    return ref, seconds, sum(ref[n].count(b"\n") for n in gd.FILES if ref[n] is not None)


def getseqs_library(al, s, cfg):
    from tests import getseqs_data as gd
    gs = importlib.import_module("vsearch_amd.getseqs")         # (the package exports the function under the module's name)
    if al is None:
        return gd.call(None, s, window=cfg["window"])
    heads, needles = s["headers"], gd.needles_arg(s)
    if cfg["scattered"]:
        heads = scattered_labels(s["headers"], cfg["layout_seed"])
        if s["mode"] not in gd.SINGLE:
            needles = scattered_labels(s["needles"], cfg["layout_seed"] + 1)
    with environment(VSX_GETSEQS_HASH_BITS=cfg["hash_bits"], VSX_GETSEQS_MAX_LENGTHS=s["max_lengths"]):
        res = gs.getseqs(al, heads, s["seqs"], s["mode"], needles, **dict(gd.call_kw(s), window=cfg["window"]))
    st, n = res.stats, len(s["headers"])
    routes = {k: v for k, v in st.items() if k.startswith("host_") and v}
    if s["max_lengths"] is not None:
        if routes != {"host_lengths": 1} or (st["headers_host"], st["headers_device"]) != (n, 0):
            raise Fatal(f"getseqs: VSX_GETSEQS_MAX_LENGTHS={s['max_lengths']}, and the route counters do not say host_lengths: {st}")
    elif routes or (st["headers_host"], st["headers_device"]) != (0, n):
        raise Fatal(f"getseqs: the device route did not answer: {st}")
    return res


def getseqs_compare(res, s, cfg, ref):
    from tests import getseqs_data as gd
    got = gd.texts(res, s)
    return diff_of([(n, got[n], gd.as_lines(ref[n])) for n in gd.FILES if ref[n] is not None] + [("log", got["log"], ref["log"])])


def getseqs_same(a, b):
    names = ("matched", "ordinal", "start", "length", "kept", "discarded")
    return diff_of((f"device and host: {n}", x, y) for n, x, y in zip(names, a.arrays(), b.arrays()))


def getseqs_cover(cfg, s):
    return [cfg["mode"]] + [k for k, hit in (("substr", cfg["substr"] and cfg["mode"] in ("label", "labels")), ("field", cfg["field"] is not None),
                                             ("subseq", cfg["subseq"]), ("fastq", cfg["fastq"]), ("hash_cut", cfg["hash_bits"]),
                                             ("lengths_host", s["max_lengths"] is not None)) if hit]


# ---- cut: --cut ----------------------------------------------------------------------------------------------------------------------
CUT_OVERLAPS = ["A^A_A", "AC^A_CA"]
CUT_BASES = dict(A="A", C="C", G="G", T="T", U="T", R="AG", Y="CT", S="CG", W="AT", K="GT", M="AC", B="CGT", D="AGT", H="ACT", V="ACG", N="ACGT")


def marked(body, fwd, rev):
    """the pattern's symbols with '^' in front of symbol fwd and '_' in front of symbol rev; at one place the order is drawn by the
    caller (rev < 0: '_' first at -rev - 1)"""
    first = rev < 0
    rev = -rev - 1 if first else rev
    out = []
    for i in range(len(body) + 1):
        if i == rev and first:
            out.append("_")
        if i == fwd:
            out.append("^")
        if i == rev and not first:
            out.append("_")
        if i < len(body):
            out.append(body[i])
    return "".join(out)


def cut_draw(rng):
    from tests import cut_data as cd
    symbols = "".join(cd.IUPAC[int(i)] for i in rng.integers(0, len(cd.IUPAC), 70))
    plen, long_len = int(rng.integers(2, 13)), int(rng.integers(65, 71))
    at = [float(x) for x in rng.random(2)]
    underscore_first, kind, overlap = bool(rng.random() < 0.5), float(rng.random()), CUT_OVERLAPS[int(rng.integers(0, 2))]
    if kind < 0.2:
        pattern = overlap
    else:
        body = symbols[:long_len if kind < 0.3 else plen]
        fwd, rev = (int(x * (len(body) + 1)) for x in at)            # any two places, both ends and one place for both included
        pattern = marked(body, fwd, -rev - 1 if underscore_first else rev)
    o = {}
    writer_opts(rng, o, "F")
    tile = [64, 128, None][int(rng.integers(0, 3))]
    cfg = dict(pattern=pattern, self_overlap=kind < 0.2, n=int(rng.integers(100, 301)), tile=tile, window=int(rng.choice(SMALL_WINDOWS)),
               scattered=bool(rng.random() < 0.3), data_seed=seed_of(rng), layout_seed=seed_of(rng), opts=o)
    cfg["cli"] = dict(o, **{k: cfg[k] for k in ("pattern", "n", "tile", "window", "scattered", "data_seed")})
    return cfg


def cut_data(rng, cfg):
    """sequences of 0 .. 600 symbols over ACGT, lower case, N, R, Y and U with one concrete reading of the pattern planted at
    cut_data.seeded_set()'s rate (for the self-overlapping patterns a run of A or of AC); every tenth carries it at 0 and at L - P;
    three have P - 1, P and P + 1 symbols"""
    from tests import cut_data as cd
    r = random.Random(cfg["data_seed"])
    body = cd.py_pattern(cfg["pattern"])[0]
    P = len(body)
    site = "".join(r.choice(CUT_BASES[c]) for c in body)
    if cfg["self_overlap"]:
        site = ("A" * 9 if body == "AAA" else "AC" * 5 + "A")[:r.randint(P, 11)]
    seqs = cd.seeded_set(cfg["data_seed"], cfg["n"], 0, 600, "ACGTacgtNRYU", site_rate=0.01, site=site)
    for k in range(5, len(seqs), 10):
        if len(seqs[k]) >= len(site):
            seqs[k] = site + seqs[k][len(site):len(seqs[k]) - len(site)] + site if len(seqs[k]) >= 2 * len(site) else site
    for k, L in zip(r.sample(range(len(seqs)), 3), (P - 1, P, P + 1)):
        seqs[k] = (site + "A")[:L] if L > P else site[:L]
    labels = [f"s{k}" + (f";size={r.randint(1, 99)}" if r.random() < 0.6 else "") for k in range(len(seqs))]
    return cd._set(f"soak_{cfg['data_seed']}", seqs, cfg["pattern"], cfg["opts"], labels=labels)


def cut_reference(s, cfg):
    from tests import cut_data as cd
    ref, seconds = timed(cd.run_cli, s)
    words = ref["log"].split()                           # "%d sequence(s) cut %d times, %d sequence(s) never cut."
    cfg["cover_after"] = ["discarded"] if int(words[0]) > 0 and int(words[5]) > 0 else []
    return ref, seconds, sum(ref[w].count("\n") for w in cd.WHICH)


def cut_library(al, s, cfg):
    from tests import cut_data as cd
    from vsearch_amd.cut import cut
    if al is None:
        return cd.call(None, s, window=cfg["window"])
    with environment(VSX_CUT_TILE=cfg["tile"]):
        seqs = scattered_blob(cfg["layout_seed"], b"A")(s["seqs"]) if cfg["scattered"] else s["seqs"]     # (gaps any pattern of A matches)
        res = cut(al, seqs, s["pattern"], window=cfg["window"])
    st = res.stats
    host = len(cd.py_pattern(s["pattern"])[0]) > 64
    if [st[r] for r in cd.HOST_ROUTES] != [0, 0, 0, 0, int(host)] or (not host and st["tile"] != (cfg["tile"] or st["tile"])):
        raise Fatal(f"cut: the route counters do not fit a pattern of {st['pattern_length']} symbols and VSX_CUT_TILE={cfg['tile']}: {st}")
    return res


def cut_compare(res, s, cfg, ref):
    from tests import cut_data as cd
    from vsearch_amd.cut import log_lines
    return asserted(cd.assert_equals_py, res, s) or \
        diff_of([(w, cd.lib_text(res, s, w).splitlines(), ref[w].splitlines()) for w in cd.WHICH] +
                [("bytes", [cd.lib_text(res, s, w) for w in cd.WHICH], [ref[w] for w in cd.WHICH]), ("log", log_lines(res), [ref["log"]])])


def cut_same(a, b):
    from tests import cut_data as cd
    return asserted(cd.assert_same, a, b, "device and host") or first_diff("device and host: bytes", a.tobytes() == b.tobytes(), True)


def cut_cover(cfg, s):
    from tests import cut_data as cd
    body = cd.py_pattern(s["pattern"])[0]
    P, coded = len(body), [cd.code4(c) for c in body]
    at_end = any(len(x) >= P and all(coded[j] & cd.code4(x[len(x) - P + j]) for j in range(P)) for x in s["seqs"])
    return [k for k, hit in (("tile_small", cfg["tile"] == 64), ("iupac_pattern", any(c.upper() not in "ACGT" for c in body)),
                             ("self_overlap", cfg["self_overlap"]), ("site_at_end", at_end),
                             ("short_sequence", any(P - 1 <= len(x) <= P + 1 for x in s["seqs"])), ("pattern_host", P > 64)) if hit]


# ---- the registry -------------------------------------------------------------------------------------------------------------------
def leg(name, host_env, what, **fn):
    g = globals()
    parts = {k: fn.get(k) or g[f"{name}_{k}"] for k in ("draw", "data", "reference", "library", "compare", "same", "cover")}
    return types.SimpleNamespace(name=name, host_env=host_env, what=what, **parts)


def _dp(fn):
    return lambda *a: fn(*a, dd=importlib.import_module("tests.derep_prefix_data"))


LEGS = {l.name: l for l in (
    leg("filter", "VSX_FILTER", "vsx_fastx_filter vs vsearch_ref --fastq_filter / --fastx_filter: the four output files and the counts"),
    leg("eestats", "VSX_EESTATS", "vsx_fastq_eestats vs vsearch_ref --fastq_eestats / --fastq_eestats2 --output"),
    leg("fastq_stats", "VSX_FASTQ_STATS", "vsx_fastq_stats / vsx_fastq_chars vs vsearch_ref --fastq_stats / --fastq_chars --log"),
    leg("derep", "VSX_DEREP", "vsx_derep vs vsearch_ref --derep_fulllength / --fastx_uniques / --derep_id: FASTA, FASTQ, tabbed, uc, log"),
    leg("derep_prefix", "VSX_DEREP_PREFIX", "vsx_derep_prefix vs vsearch_ref --derep_prefix: FASTA, uc, log",
        reference=_dp(derep_reference), compare=_dp(derep_compare), same=_dp(derep_same)),
    leg("search_exact", "VSX_EXACT", "vsx_search_exact vs vsearch_ref --search_exact: userout, uc, dbmatched, the log's counts"),
    leg("orient", "VSX_ORIENT", "vsx_orient vs vsearch_ref --orient: tabbedout, fastaout, fastqout, notmatched, log"),
    leg("sintax", "VSX_SINTAX", "vsx_sintax vs vsearch_ref --sintax: tabbedout and the log's count"),
    leg("otutab", "VSX_OTUTAB", "vsx_otutab vs vsearch_ref --search_exact --otutabout --mothur_shared_out --biomout"),
    leg("hitout", "VSX_HITOUT", "vsx_hits_render vs vsearch_ref --usearch_global: alnout, samout (and its header), blast6out, fastapairs, "
        "qsegout, tsegout, userout in both field orders"),
    leg("mask", "VSX_MASK", "vsx_fastx_mask vs vsearch_ref --fastx_mask (fastaout, fastqout, the closing log lines) / --maskfasta --output"),
    leg("getseqs", "VSX_GETSEQS", "vsx_getseqs vs vsearch_ref --fastx_getseqs / --fastx_getseq / --fastx_getsubseq: fastaout, fastqout, "
        "notmatched, notmatchedfq, the log line"),
    leg("cut", "VSX_CUT", "vsx_cut vs vsearch_ref --cut: fastaout, fastaout_rev, fastaout_discarded, fastaout_discarded_rev, the log line; "
        "and vs cut_data.py_cut()"),
)}


# ---- the loop -----------------------------------------------------------------------------------------------------------------------
def is_fatal(e):
    from tests import poison_cases
    from vsearch_amd._lib import VSX_EHIP, VsxError
    return isinstance(e, Fatal) or (isinstance(e, VsxError) and e.code == VSX_EHIP) or poison_cases.is_sticky(str(e))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--command", required=True, choices=sorted(LEGS))
    ap.add_argument("--route", default="device", choices=["device", "host"])
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    ap.add_argument("--max-rounds", type=int, default=0, help="stop after this many rounds (0: run for --seconds): a deterministic set of rounds for a given seed")
    ap.add_argument("--reference-only", action="store_true", help="run the reference alone and count its lines (no library)")
    a = ap.parse_args()
    if not os.path.exists(REF_BIN):
        raise SystemExit("oracle/_ref/vsearch_ref missing: make -C oracle ref_full")
    L = LEGS[a.command]
    al = None
    if not a.reference_only and a.route == "device":
        from vsearch_amd import Aligner
        al = Aligner()
    rng = np.random.default_rng(a.seed)
    t_end = time.time() + a.seconds
    rounds = lines = bad = 0
    ref_seconds = 0.0
    failing, coverage, fatal = [], {}, None

    def fail(cfg, **what):
        nonlocal bad
        bad += 1
        if len(failing) < 10:
            failing.append({"cli": cfg["cli"], "round": rounds - 1, **what})

    def on_host(s, cfg):
        with environment(**{L.host_env: "host"}):
            return L.library(None, s, cfg)

    while time.time() < t_end and (a.max_rounds <= 0 or rounds < a.max_rounds):
        cfg = L.draw(rng)
        s = L.data(rng, cfg)
        rounds += 1
        for key in L.cover(cfg, s):
            coverage[key] = coverage.get(key, 0) + 1
        try:
            ref, seconds, n = L.reference(s, cfg)
        except Refused as e:
            fail(cfg, error=str(e))
            continue
        ref_seconds += seconds
        lines += n
        for key in cfg.get("cover_after", ()):          # (classes only the reference's answer decides)
            coverage[key] = coverage.get(key, 0) + 1
        if a.reference_only:
            continue
        if al is not None:
            try:
                res = L.library(al, s, cfg)
            except Exception as e:                      # any exception of the device call: nothing more is started on the GPU
                fatal = f"{type(e).__name__}: {e}"
                fail(cfg, error=fatal[-500:])
                break
            diff = L.compare(res, s, cfg, ref)
        try:
            host = on_host(s, cfg)
        except Exception as e:
            if is_fatal(e):
                fatal = f"{type(e).__name__}: {e}"
                fail(cfg, error=fatal[-500:])
                break
            fail(cfg, what="the host route refused the round", error=f"{type(e).__name__}: {e}"[-500:])
            continue
        if al is None:
            diff = L.compare(host, s, cfg, ref)
        elif diff is None:
            diff = L.same(res, host)
        if diff is not None:
            fail(cfg, **diff)
    if al is not None and fatal is None:
        al.close()
    out = {"rounds": rounds, "lines": lines, "failing_rounds": bad, "failures": failing, "coverage": coverage, "seed": a.seed,
           "seconds": a.seconds, "reference_seconds": round(ref_seconds, 3), "command": a.command, "route": a.route,
           "what": L.what + " with the same randomly drawn options; device vs host restatement field for field"}
    if fatal is not None:
        out["fatal"] = fatal[-2000:]
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f)
    if fatal is not None:
        sys.stdout.flush()
        os._exit(3)                                      # (no destructor touches the device again)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
