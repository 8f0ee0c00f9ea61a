"""-m gpu: a short, seeded run of the randomized soaks of the newer commands (oracle/soak_merge.py: --fastq_mergepairs with random
quality encodings, options, read lengths and windows; oracle/soak_chimera.py: --uchime_ref and the three de novo variants with random
lengths, masks and parameters, and --chimeras_denovo behind --commands; oracle/soak_commands.py: one leg per command added since --
filter, eestats, fastq_stats, derep, derep_prefix, search_exact, orient, sintax, otutab, hitout, mask, getseqs, cut; and
oracle/soak_chimera.py --outputs alns: --uchimealns at --alignwidth 0 / 1 / 60 / 80 / 133 with the --chimeras / --nonchimeras /
--borderline FASTA writers beside every round of the four chimera commands) against the reference CLI, as tests/test_gpu_soak.py
runs the older ones.

The floors are the reference's own line counts for the seed and the round count (`--reference-only`, no device), rounded down to
two significant digits.  The round counts keep the reference CLI's share of a case below 5 s (measured: 0.5 s for the 40 merge
rounds; 2.6 s and 3.7 s for the two chimera cases, where one --uchime_ref round at 3 900-4 200 symbols alone costs it 1-2 s; the
figures of the newer cases stand beside them and in profiles/soak_commands/INDEX.md): the largest count up to 40 that does.

The chimera seeds were picked, with the reference alone, so that each fixed set of six rounds contains a --uchime_ref round in the
length class that straddles the kernel's limit of 4 096, a --hardmask round and an --abskew round; the test asserts that on the
soak's own "coverage" record.  Together the two sets hold --uchime_ref in all four length classes and each de novo variant.  The
seeds of the newer cases were picked the same way: the fixed rounds hold every coverage class of their leg (MUST) and the
reference refuses none of them.

Found by oracle/soak_commands.py and kept as ordinary tests beside the command's own:
  - otutab: the reference's search commands count the header's ;size= annotation in the OTU table with or without --sizein;
    tests/otutab_data.inputs() counted 1 per query without it (tests/test_otutab_host.py::test_annotated_abundance_counts_without_sizein)
  - getseqs: --fastx_getseqs / --fastx_getseq / --fastx_getsubseq print the header's ;size= annotation under --sizeout with or
    without --sizein; tests/getseqs_data.sizes_of() gave 1 without it -- a wrong expectation of the tests' restatement, the library's
    writers print what they are handed (tests/test_getseqs_host.py::test_sizeout_prints_the_annotation_without_sizein)
Found by oracle/soak_chimera.py --outputs alns:
  - --uchimeout under --xsize: the reference strips the ;size= annotation from the query's, both parents' and the closest parent's
    label; format_uchimeout() and the sessions' uchimeout() took no xsize and printed the labels whole.  They take it now
    (tests/test_chimalns_host.py::test_uchimeout_strips_the_size_annotation_under_xsize)
The mask and cut legs found no mismatch.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHIMERA_MUST = ("uchime_ref@3900-4200", "hardmask", "abskew")
# the coverage classes every fixed set of rounds of a leg of oracle/soak_commands.py must hold
MUST = {
    "filter": ("paired", "fasta", "ascii64", "truncee_or_rate", "chunk_edge", "scattered", "exact_ee"),
    "eestats": ("ascii64", "eestats2", "window_split"),
    "fastq_stats": ("chars", "ascii64"),
    "derep": ("derep_fulllength", "fastx_uniques", "derep_id", "fastq", "strand_both", "hash_cut"),
    "derep_prefix": ("hash_cut", "topn", "sizein"),
    "search_exact": ("dust", "hardmask", "strand_both"),
    "orient": ("wl_le_5", "wl_12", "wl_host", "fastq", "hash_cut", "build_chunks"),
    "sintax": ("strand_both", "cutoff", "wl_lt_8", "wl_host"),
    "otutab": ("hash_cut", "biom", "mothur"),
    "hitout": ("hardmask", "minus_strand", "rowlen0", "n_mismatch", "window1"),
    "mask": ("dust", "soft", "hardmask", "percent_exact", "fastq", "maskfasta", "long_route", "length_edge", "discarded"),
    "getseqs": ("label", "labels", "label_word", "label_words", "substr", "field", "subseq", "fastq", "hash_cut", "lengths_host", "notmatched"),
    "cut": ("tile_small", "iupac_pattern", "self_overlap", "site_at_end", "short_sequence", "pattern_host", "discarded"),
}
# oracle/soak_chimera.py --outputs alns: the classes of the four extra files, beside those every chimera case holds
ALNS_MUST = ("alns", "alignwidth0", "alignwidth_other", "fasta_score", "borderline", "alns_host_long", "hardmask", "abskew")
CHIMERAS_DENOVO_MUST = ("chimeras_denovo@1900-2200", "diff_pct_host", "parts")
TIME_LIMIT = 600


def run_soak(tmp_path, script, extra, seed, rounds, floor, must):
    """a FIXED set of rounds per case (seed + round count: the same configurations on every machine, whatever its speed)"""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "vsearch_ref")):
        pytest.fail("oracle/_ref missing: run `make -C oracle ref ref_full` in the build container")
    out = str(tmp_path / "soak.json")
    cmd = [sys.executable, os.path.join(ROOT, "oracle", script)] + list(extra) + ["--seconds", "300", "--max-rounds", str(rounds), "--seed", str(seed), "--out", out]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=TIME_LIMIT, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"{script} {' '.join(extra)} ran into its time limit of {TIME_LIMIT} s: {str(e.stderr or '')[-3000:]}")
    # exit status 3: a library error that is no mismatch ended the soak (nothing more was started on the device)
    assert p.returncode != 3, p.stderr[-3000:] + p.stdout[-3000:]
    assert os.path.exists(out), p.stderr[-3000:]
    doc = json.load(open(out))
    assert p.returncode == 0, json.dumps({k: v for k, v in doc.items() if k in ("failing_rounds", "failures")})[:3000]
    assert doc["rounds"] == rounds and doc["lines"] >= floor, doc
    for key in must:
        assert doc["coverage"].get(key, 0) >= 1, (key, doc["coverage"])


@pytest.mark.parametrize("script,seed,rounds,floor,must", [
    ("soak_merge.py", 20260924, 40, 17_000, ()),          # 17 728 lines: merged FASTQ + eetabbed + not-merged labels
    ("soak_chimera.py", 20260930, 6, 330, CHIMERA_MUST),  # 330 --uchimeout lines
    ("soak_chimera.py", 20260971, 6, 170, CHIMERA_MUST),  # 171 --uchimeout lines
])
def test_seeded_soak(gpu_required, tmp_path, script, seed, rounds, floor, must):
    """a FIXED set of rounds per case (seed + round count: the same configurations on every machine, whatever its speed)"""
    run_soak(tmp_path, script, (), seed, rounds, floor, must)


@pytest.mark.parametrize("leg,seed,rounds,floor", [
    # leg, seed, rounds, floor         the reference's lines, its seconds (build machine), the case's wall time on the MI355X
    ("filter", 20261020, 40, 40_000),           # 40 083 lines, 0.12 s, 1.5 s
    ("eestats", 20261020, 40, 5_000),           # 5 066 lines, 3.3 s, 3.3 s
    ("fastq_stats", 20261020, 40, 22_000),      # 22 784 lines, 0.22 s, 2.9 s
    ("derep", 20261020, 40, 72_000),            # 72 313 lines, 0.17 s, 1.5 s
    ("derep_prefix", 20261020, 40, 43_000),     # 43 184 lines, 0.14 s, 1.0 s
    ("search_exact", 20261020, 40, 21_000),     # 21 680 lines, 0.25 s, 1.4 s
    ("orient", 20261020, 40, 43_000),           # 43 131 lines, 3.3 s, 2.8 s
    ("sintax", 20261020, 40, 5_800),            # 5 817 lines, 3.3 s, 4.4 s
    ("otutab", 20261020, 40, 7_500),            # 7 564 lines, 0.24 s, 0.7 s
    ("hitout", 20261020, 28, 1_900_000),        # 1 935 410 lines (rowlen 1: a line per column), 4.6 s (30 rounds: 5.4 s), 6.6 s
    ("mask", 20261020, 40, 23_000),             # 23 532 lines, 0.42 s, 1.6 s
    ("getseqs", 20261021, 40, 56_000),          # 56 523 lines, 0.21 s, 1.1 s (20261020 holds no lengths_host round)
    ("cut", 20261020, 40, 760_000),             # 765 445 lines (a pattern of two IUPAC symbols cuts everywhere), 0.41 s, 3.9 s
])
def test_seeded_soak_of_a_command(gpu_required, tmp_path, leg, seed, rounds, floor):
    run_soak(tmp_path, "soak_commands.py", ("--command", leg), seed, rounds, floor, MUST[leg])


def test_seeded_soak_of_chimeras_denovo(gpu_required, tmp_path):
    """5 rounds: 249 lines (--tabbedout + the labels of --chimeras and --nonchimeras), 4.4 s of the reference (6 rounds: 6.0 s), 4.5 s on the MI355X"""
    run_soak(tmp_path, "soak_chimera.py", ("--commands", "chimeras_denovo"), 20261021, 5, 240, CHIMERAS_DENOVO_MUST)


def test_seeded_soak_of_uchimealns_and_the_fasta_writers(gpu_required, tmp_path):
    """10 rounds of the four chimera commands with --outputs alns: 160 353 lines (--uchimeout, --uchimealns -- one block line per column
    at --alignwidth 1 --, --chimeras, --nonchimeras, --borderline), 2.9 s of the reference (11 rounds: 5.3 s), 3.6 s on the MI355X"""
    run_soak(tmp_path, "soak_chimera.py", ("--outputs", "alns"), 20261133, 10, 160_000, ALNS_MUST)
