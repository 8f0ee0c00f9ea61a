"""not gpu: the host star-MSA (vsx_msa) against the reference CLI on its own CIGARs.

The reference CLI's --cluster_fast writes --uc (member -> centroid CIGAR, the string the reference's msa() consumes) next to
--msaout / --consout / --profile; tests/golden/msa_golden.json carries those four files for two seeded inputs
(oracle/gen_golden.py gen_msa).  vsx_msa fed with the uc CIGARs must reproduce the other three byte for byte.
No GPU is involved: the clustering is the reference's, the MSA is host code."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wrap(seq, width=80):
    return [seq[i:i + width] for i in range(0, len(seq), width)] or [""]


@pytest.mark.parametrize("seed", [3, 8])
def test_host_msa_matches_reference_cli(seed):
    from vsearch_amd import msa
    case = json.load(open(os.path.join(ROOT, "tests", "golden", "msa_golden.json")))["cases"][str(seed)]
    by_name = {f"s{i:03d}": s for i, s in enumerate(case["in"])}
    clusters = {}                                          # cluster number -> [(name, cigar or None)], centroid first
    for ln in case["uc"]:
        r = ln.split("\t")
        if r[0] == "S":
            clusters[int(r[1])] = [(r[8], None)]
        elif r[0] == "H":
            assert r[4] == "+"
            cig = r[7] if r[7] != "=" else f"{len(by_name[r[8]])}M"
            clusters[int(r[1])].append((r[8], cig))
    msa_lines, cons_lines, prof_lines = [], [], []
    for c in sorted(clusters):
        m = clusters[c]
        res = msa([by_name[n] for n, _ in m], [g for _, g in m])
        msa_lines.append("")
        for k, (n, _) in enumerate(m):
            msa_lines.append(">" + ("*" if k == 0 else "") + n)
            msa_lines += _wrap(res["rows"][k])
        msa_lines.append(">consensus")
        msa_lines += _wrap(res["rows"][-1])
        cons_lines.append(f">centroid={m[0][0]};seqs={len(m)}")
        cons_lines += _wrap(res["consensus"])
        prof_lines.append(f">centroid={m[0][0]};seqs={len(m)}")
        for i, (ch, pr) in enumerate(zip(res["rows"][-1], res["profile"])):
            prof_lines.append("\t".join([str(i), ch] + [str(pr[k]) for k in (0, 1, 2, 3, 5, 4)]))
        prof_lines.append("")
    assert msa_lines == case["msa"]
    assert cons_lines == case["cons"]
    assert prof_lines == case["prof"]
