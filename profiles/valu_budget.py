#!/usr/bin/env python3
"""profiles/valu_budget.py [--lib vsearch_amd/libvsx.so] [--kernel "16,false,true,true,1,false,true"] [--rows R] [--loop N]

VALU budget of the steady interior loop of one vsx_forward_kernel instantiation, read from the gfx950 code object inside the built
library (llvm-objdump; no GPU needed).  Prints every loop of the kernel (backward branches), then for the chosen one (default: the loop
with the most v_pk_maximum3_f16, i.e. the steady phase-A loop of the MAX3 classes):

  * steps per iteration S = v_pk_maximum3_f16 on the always-taken path / R (every row of a steady step takes the three-way maximum);
  * VALU on the always-taken path per iteration, and in the loop's branch-guarded regions (the 16-step block boundary: next feed
    block, column checkpoint), amortised as once per 16 steps;
  * the split by category.  The split is by opcode, with per-step quotas where one opcode serves two purposes: R v_perm_b32, R v_add_u32
    and one v_pk_sub_i16 (the last row's H - QR) per step are row body; two more v_pk_sub_i16 per step are the last row's own e / hf
    subtractions; one v_pk_sub_i16 per v_pk_ashrrev_i16 is the leave-column difference; what is left of those opcodes is checkpoint
    packing (v_perm_b32, v_pk_sub_i16) or "other" (v_add_u32);
  * VGPRs, SGPRs and scratch of the kernel.
"""
import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mangled(args):
    a = [x.strip() for x in args.split(",")]
    enc = "".join(("Li%sE" % x) if x.lstrip("-").isdigit() else ("Lb%dE" % (x == "true")) for x in a)
    return "_Z18vsx_forward_kernelI" + enc + "Ev12VsxDevParamsPK7VsxTaskPKhS5_PjP15HIP_vector_typeIjLj2EEP10VsxSlotOutj"


def extract(lib, sym, tmp):
    shutil.copy(lib, os.path.join(tmp, "lib.so"))
    subprocess.run([LLVM + "/llvm-objdump", "--offloading", "lib.so"], cwd=tmp, capture_output=True, check=True)
    for f in sorted(os.listdir(tmp)):
        if "gfx950" not in f:
            continue
        p = os.path.join(tmp, f)
        syms = subprocess.run([LLVM + "/llvm-readelf", "-s", "--wide", p], capture_output=True, text=True).stdout
        if (" " + sym + "\n") in syms:
            return p, syms
    sys.exit("kernel %s not found in %s" % (sym, lib))


def meta(syms, sym):
    out = {}
    for k in ("num_vgpr", "numbered_sgpr", "private_seg_size"):
        m = re.search(r"\s([0-9a-f]+)\s+0\s+NOTYPE\s+LOCAL\s+DEFAULT\s+ABS\s+" + re.escape(sym) + r"\." + k + r"\n", syms)
        out[k] = int(m.group(1), 16) if m else None
    m = re.search(r"\s([0-9a-f]+)\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+" + re.escape(sym) + r"\n", syms)
    out["start"], out["size"] = int(m.group(1), 16), int(m.group(2))
    return out


def disasm(co, sym, start):
    txt = subprocess.run([LLVM + "/llvm-objdump", "-d", "--mcpu=gfx950", "--disassemble-symbols=" + sym, co],
                         capture_output=True, text=True, check=True).stdout
    ins = []
    for line in txt.splitlines():
        m = re.match(r"\s+(\S+)\s*(.*?)\s*//\s*([0-9A-F]+):", line)
        if not m:
            continue
        op, rest, addr = m.group(1), m.group(2), int(m.group(3), 16) - start
        t = re.search(r"<" + re.escape(sym) + r"\+0x([0-9a-f]+)>", line)
        ins.append((addr, op, rest, int(t.group(1), 16) if t else None))
    return ins


def is_valu(op):
    return op.startswith("v_")


def category(op, rest):
    if op in ("v_pk_maximum3_f16", "v_pk_max_u16", "v_subrev_u32_e32", "v_sub_u32_e32", "v_subrev_u32_e64", "v_sub_u32_e64"):
        return "row body"
    if op == "v_mov_b32_dpp":
        return "DPP hand-overs (feed, H, F)"
    if op == "v_add_u32_sdwa":
        return "profile row addresses"
    if op in ("v_pk_ashrrev_i16", "v_bfi_b32"):
        return "leave-column tracking"
    if op in ("v_lshl_add_u32", "v_lshlrev_b32_e32", "v_or_b32_e32", "v_and_or_b32") and "s" in rest.split(",")[1]:
        return "feed-slot addresses"
    if op in ("v_lshl_add_u64", "v_add_co_u32_e32", "v_addc_co_u32_e32", "v_mad_u64_u32"):
        return "checkpoint addresses"
    if op == "v_mov_b32_e32":
        return "register copies"
    return None


def budget(body, R, S):
    """per-category VALU counts of a list of (op, rest) for S steps (quotas as in the module doc)."""
    c = collections.Counter()
    quota = {"v_perm_b32": R * S, "v_add_u32_e32": R * S}
    npk = sum(1 for op, _ in body if op == "v_pk_sub_i16")
    nashr = sum(1 for op, _ in body if op == "v_pk_ashrrev_i16")
    pk = [("row body", S), ("last row's own e / hf subtractions", 2 * S), ("leave-column tracking", nashr)]
    for op, rest in body:
        if not is_valu(op):
            continue
        k = category(op, rest)
        if k is None and op in quota:
            if op == "v_add_u32_e32" and re.search(r"0x(1|2)000(1|2)\b", rest):
                k = "leave-column tracking"
            elif quota[op] > 0:
                quota[op] -= 1
                k = "row body"
            else:
                k = "checkpoint pack" if op == "v_perm_b32" else "other"
        if k is None and op == "v_pk_sub_i16":
            for i, (name, n) in enumerate(pk):
                if n > 0:
                    pk[i] = (name, n - 1)
                    k = name
                    break
            else:
                k = "checkpoint pack"
        c[k or "other"] += 1
    return c, npk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "vsearch_amd", "libvsx.so"))
    ap.add_argument("--kernel", default="16,false,true,true,1,false,true", help="template arguments of vsx_forward_kernel")
    ap.add_argument("--rows", type=int, default=None, help="R (default: the first template argument)")
    ap.add_argument("--loop", type=int, default=None, help="loop index to budget (default: most v_pk_maximum3_f16)")
    ap.add_argument("--ops", action="store_true", help="print the opcode histogram of the loop too")
    a = ap.parse_args()
    R = a.rows or int(a.kernel.split(",")[0])
    sym = mangled(a.kernel)
    tmp = tempfile.mkdtemp(prefix="vsx_budget_")
    try:
        co, syms = extract(a.lib, sym, tmp)
        md = meta(syms, sym)
        ins = disasm(co, sym, md["start"])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("vsx_forward_kernel<%s>  (%s)" % (a.kernel, os.path.relpath(a.lib, ROOT) if a.lib.startswith(ROOT) else a.lib))
    print("  code %d B, %d instructions, %d VALU;  VGPR %s  SGPR %s  scratch %s B" % (
        md["size"], len(ins), sum(is_valu(op) for _, op, _, _ in ins), md["num_vgpr"], md["numbered_sgpr"], md["private_seg_size"]))
    idx = {addr: k for k, (addr, _, _, _) in enumerate(ins)}
    # loops: head = target of a backward branch; the loop spans head .. the last backward branch to it
    heads = collections.OrderedDict()
    for k, (addr, op, _, tgt) in enumerate(ins):
        if op.startswith("s_branch") or op.startswith("s_cbranch"):
            if tgt is not None and tgt <= addr and tgt in idx:
                h = idx[tgt]
                heads.setdefault(h, []).append(k)
    loops = []
    for h, bs in heads.items():
        first_back, last = min(bs), max(bs)
        main_path = set(range(h, first_back + 1))
        # forward conditional branches inside the main path skip a region: that region is conditional
        for k in range(h, first_back + 1):
            addr, op, _, tgt = ins[k]
            if op.startswith("s_cbranch") and tgt is not None and tgt > addr and tgt in idx and idx[tgt] <= first_back + 1:
                for j in range(k + 1, idx[tgt]):
                    main_path.discard(j)
        cond = [j for j in range(h, last + 1) if j not in main_path]
        mp = sorted(main_path)
        loops.append(dict(head=h, end=last, main=mp, cond=cond,
                          max3=sum(1 for j in mp if ins[j][1] == "v_pk_maximum3_f16"),
                          valu_main=sum(1 for j in mp if is_valu(ins[j][1])), valu_cond=sum(1 for j in cond if is_valu(ins[j][1]))))
    print("  loops (offset range: VALU on the always-taken path + in branch-guarded regions, v_pk_maximum3_f16):")
    for n, L in enumerate(loops):
        print("    [%d] +0x%04x..+0x%04x: %4d + %4d VALU, %3d max3" % (n, ins[L["head"]][0], ins[L["end"]][0], L["valu_main"], L["valu_cond"], L["max3"]))
    if not loops:
        return
    n = a.loop if a.loop is not None else max(range(len(loops)), key=lambda i: (loops[i]["max3"], -i))
    L = loops[n]
    S = max(1, round(L["max3"] / R))
    body = [(ins[j][1], ins[j][2]) for j in L["main"]]
    cond = [(ins[j][1], ins[j][2]) for j in L["cond"]]
    cm, _ = budget(body, R, S)
    per_step = L["valu_main"] / S + L["valu_cond"] / 16.0
    print("  loop [%d]: %d steps per iteration (R = %d)" % (n, S, R))
    print("    VALU per two steps, always-taken path: %.1f" % (2.0 * L["valu_main"] / S))
    print("    VALU in branch-guarded regions (once per 16 steps): %d" % L["valu_cond"])
    print("    VALU per 16-step block: %.0f   per step: %.2f   (row body %d per step = %.1f %%)" % (
        16 * per_step, per_step, 6 * R, 100.0 * 6 * R / per_step))
    print("    per step, by category (always-taken path / S, + branch-guarded / 16):")
    order = ["row body", "DPP hand-overs (feed, H, F)", "profile row addresses", "feed-slot addresses", "last row's own e / hf subtractions",
             "leave-column tracking", "checkpoint pack", "checkpoint addresses", "register copies", "other"]
    for k in order:
        v = cm.get(k, 0) / S
        if v:
            print("      %-38s %6.2f" % (k, v))
    if L["valu_cond"]:
        print("      %-38s %6.2f  (%d VALU / 16)" % ("16-step block boundary (guarded)", L["valu_cond"] / 16.0, L["valu_cond"]))
    if a.ops:
        for name, lst in (("always-taken path", body), ("branch-guarded", cond)):
            h = collections.Counter(op for op, _ in lst if is_valu(op))
            print("    %s opcodes: %s" % (name, ", ".join("%s %d" % kv for kv in h.most_common())))


if __name__ == "__main__":
    main()
