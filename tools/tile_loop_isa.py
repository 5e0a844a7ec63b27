#!/usr/bin/env python3
"""Developer tool: what the STEP LOOP of the products-only tile kernels is made of, as built for gfx950 (no GPU needed).
    python tools/tile_loop_isa.py > profiles/rNN_tile_loop_isa.txt          (compiles t-route_amd/csrc/trmc.hip itself)
    python tools/tile_loop_isa.py --asm trmc.s                              (an assembly made with -gline-tables-only)

Compiles the device side of trmc.hip to assembly with the flags of the shipped build plus line tables, and for the two headline
instances -- k_mc_tile<float, false, false, true> and k_mc_ctile<float, false, false, true> -- takes the body of the time loop
(`for t = t_lo .. t_hi`: the outermost loop of the kernel that holds the secant iteration) apart by basic block.  A block
belongs to a PATH by the source lines its instructions come from and by its loop depth (the compiler's own loop annotations):

  frame        the step loop outside the segment step: forcing column, junction sum, stores, loop control
  in-bank x1   what a step of ONE secant iteration executes in bank: both points of step_pre by hydraulics_inbank, the first
               secant_iterate, the outflow                                            (depth 1, fast power)
  general x1   the same step with the general body: both points by hydraulics_general   (depth 1, section_at / hydraulics_core)
  iteration    each FURTHER secant iteration, in bank: hydraulics_inbank + secant_iterate   (the inner while loop)
  iteration-g  ... with the general (over-bank) body
  rare         reservoir rows (levelpool.hpp), nudging, the CSR walk of fan-in > 2, the retry loop's bracket widening

Within a path the vector-ALU instructions (v_*) are counted, and of those
  spill        v_readlane_b32 / v_writelane_b32 (a scalar register parked in a vector lane); scratch loads and stores beside them
  literal      v_mov_b32 of a constant
  copy         v_mov_b32 / v_mov_b64 of a register (scalar -> vector copies of uniform values among them)
  address      64-bit integer address arithmetic (v_lshl_add_u64, v_mad_u64_u32, v_mul_lo/hi_u32, v_add_co / v_addc_co)
The count is STATIC: every block of a path once -- a wavefront skips the blocks of branches none of its lanes takes, so a
path's total is an upper bound of what one pass executes; the spill / literal / address columns are exact per block."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "t-route_amd", "csrc")
HEADLINE = ("k_mc_tile<float, false, false, true>", "k_mc_ctile<float, false, false, true>")


def function_lines(path, names):
    """{name: (first, last)} line ranges of the named functions of a source file (brace matching from the name's line)."""
    src = open(path).read().splitlines()
    out = {}
    for name in names:
        for i, l in enumerate(src):
            if re.search(r"\b" + name + r"\s*\(", l) and not l.rstrip().endswith(";") and "return" not in l:
                depth, seen, j = 0, False, i
                while j < len(src):
                    depth += src[j].count("{") - src[j].count("}")
                    seen = seen or "{" in src[j]
                    if seen and depth == 0:
                        break
                    j += 1
                out.setdefault(name, (i + 1, j + 1))
                break
    return out


def source_kinds():
    seg = function_lines(os.path.join(CSRC, "mc_segment.hpp"),
                         ["section_at", "over_bank_pow", "hydraulics_core", "hydraulics_general", "hydraulics_inbank",
                          "secant_residual", "secant_iterate", "step_solve"])
    pw = function_lines(os.path.join(CSRC, "det_pow.h"),
                        ["trmc_det_log2", "trmc_det_powf_from_log", "trmc_det_log2_normal", "trmc_det_powf_from_log_inrange"])
    kinds = []
    for n in ("hydraulics_inbank",):
        kinds.append(("mc_segment.hpp", seg[n], "inbank"))
    for n in ("section_at", "over_bank_pow", "hydraulics_core", "hydraulics_general"):
        kinds.append(("mc_segment.hpp", seg[n], "general"))
    for n in ("secant_residual", "secant_iterate"):
        kinds.append(("mc_segment.hpp", seg[n], "secant"))
    kinds.append(("mc_segment.hpp", seg["step_solve"], "solve"))
    for n in ("trmc_det_log2_normal", "trmc_det_powf_from_log_inrange"):
        kinds.append(("det_pow.h", pw[n], "inbank"))
    for n in ("trmc_det_log2", "trmc_det_powf_from_log"):
        kinds.append(("det_pow.h", pw[n], "general"))
    return kinds


def kind_of(kinds, f, ln):
    if f in ("levelpool.hpp", "reservoir_da.hpp"):
        return "reservoir"
    for kf, (a, b), k in kinds:
        if f == kf and a <= ln <= b:
            return k
    if f in ("kernels_levels.inc", "k_mc_ctile.inc", "k_tile_row.inc"):
        return "frame"  # (k_tile_row.inc: load_row_params, reservoir_row, nudge_row, hand_on_row -- text of the two loops, as before)
    return None  # (dev_math.inc, compiler headers: whatever surrounds them)


def parse(asm_lines, start):
    files, blocks, loc = {}, [], (None, 0)
    cur = {"label": "entry", "depth": 0, "header": None, "ins": []}
    blocks.append(cur)
    for l in asm_lines[start + 1:]:
        s = l.strip()
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", s)
        if m or re.match(r"^; %bb\.\d+:", s):
            d = re.search(r"Depth[= ](\d+)", s)
            cur = {"label": m.group(1) if m else s.split(":")[0][2:], "depth": int(d.group(1)) if d else 0, "ins": [],
                   "header": "Header" in s and "in Loop" not in s}
            blocks.append(cur)
            continue
        d = re.match(r"^;\s+(Child Loop|Parent Loop)", s)
        if d:
            continue
        d = re.match(r"^; =>\s*This (Inner )?Loop Header: Depth=(\d+)", s)
        if d:
            cur["depth"], cur["header"] = int(d.group(2)), True
            continue
        m = re.match(r"^\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            loc = (int(m.group(1)), int(m.group(2)))
            continue
        if not s or s[0] in ".;":
            continue
        m = re.match(r"^([a-z][a-z0-9_]+)\s*(.*?)(?:\s*;.*)?$", s)
        if m:
            cur["ins"].append((m.group(1), m.group(2), loc))
            if m.group(1) == "s_endpgm":
                break
    return blocks


def classify(op, args):
    c = []
    if not op.startswith("v_"):
        if op.startswith("scratch_"):
            c.append("scratch")
        return c
    c.append("valu")
    if op in ("v_readlane_b32", "v_writelane_b32"):
        c.append("spill")
    elif op.startswith("v_mov_b"):
        src = args.split(",")[-1].strip()
        c.append("copy" if re.match(r"^[vs]\d|^[vs]\[|^vcc|^exec", src) else "literal")
    elif op.startswith(("v_lshl_add_u64", "v_mad_u64_u32", "v_mad_i64_i32", "v_mul_lo_u32", "v_mul_hi_u32", "v_add_co_u32",
                        "v_addc_co_u32", "v_lshlrev_b64")):
        c.append("address")
    return c


def report(asm_path):
    kinds = source_kinds()
    lines = open(asm_path).read().splitlines()
    fileno = {}
    for l in lines:
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
        if m:
            fileno[int(m.group(1))] = os.path.basename(m.group(3) or m.group(2))
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if not m:
            continue
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        name = name.replace("(anonymous namespace)::", "")
        inst = next((h for h in HEADLINE if name.startswith("void " + h + "(") or name.startswith(h + "(")), None)
        if not inst:
            continue
        blocks = parse(lines, i)
        # the step loop: the depth-1 loop that holds the secant iteration (the partition's loops before it hold no power)
        first = next(k for k, b in enumerate(blocks) if b["depth"] >= 2 and any(
            kind_of(kinds, fileno.get(f), ln) in ("inbank", "general", "secant") for _, _, (f, ln) in b["ins"]))
        lo = first
        while lo > 0 and blocks[lo - 1]["depth"] >= 1:
            lo -= 1
        hi = first
        while hi + 1 < len(blocks) and blocks[hi + 1]["depth"] >= 1:
            hi += 1
        loop = blocks[lo:hi + 1]
        # kind of every block: the majority of its attributable instructions; none attributable -> the block before it
        prev = "frame"
        for b in loop:
            votes = collections.Counter(k for k in (kind_of(kinds, fileno.get(f), ln) for _, _, (f, ln) in b["ins"]) if k)
            b["kind"] = prev = votes.most_common(1)[0][0] if votes else prev
        res = [k for k, b in enumerate(loop) if b["kind"] == "reservoir"]
        for k in range(res[0], res[-1] + 1) if res else ():
            loop[k]["kind"] = "reservoir"  # (the general power of the reservoir's weir formulas)
        inner = max(b["depth"] for b in loop)
        tot = collections.OrderedDict((p, collections.Counter()) for p in
                                      ("frame", "in-bank x1", "general x1", "iteration", "iteration-g", "rare"))
        for b in loop:
            k, d = b["kind"], b["depth"]
            if k == "reservoir":
                path = "rare"
            elif d == inner:
                path = "iteration-g" if k == "general" else "iteration"
            elif d > 1:
                path = "rare"  # the CSR walk, the retry loop's own blocks
            elif k == "frame":
                path = "frame"
            else:
                path = "general x1" if k == "general" else "in-bank x1"
            t = tot[path]
            t["blocks"] += 1
            for op, args, _ in b["ins"]:
                t["all"] += 1
                for c in classify(op, args):
                    t[c] += 1
        print(f"\n== {inst}: step loop = {len(loop)} basic blocks, loop depth {inner}")
        print(f"   {'path':12s} {'blocks':>6s} {'instr':>6s} {'VALU':>6s} | {'spill':>5s} {'literal':>7s} {'copy':>5s} {'address':>7s} | {'scratch ld/st':>13s}")
        for p, t in tot.items():
            print(f"   {p:12s} {t['blocks']:6d} {t['all']:6d} {t['valu']:6d} | {t['spill']:5d} {t['literal']:7d} {t['copy']:5d} "
                  f"{t['address']:7d} | {t['scratch']:13d}")
        step1 = tot["frame"] + tot["in-bank x1"]
        print(f"   a step of one iteration, in bank (frame + in-bank x1): {step1['valu']} VALU, of them spill {step1['spill']} "
              f"({100.0 * step1['spill'] / max(1, step1['valu']):.1f} %), literal {step1['literal']}, copy {step1['copy']}, "
              f"address {step1['address']}; scratch {step1['scratch']}")
        whole = sum(tot.values(), collections.Counter())
        print(f"   whole loop: {whole['valu']} VALU, spill {whole['spill']}, scratch {whole['scratch']}")
        for j in range(i, min(len(lines), i + 40000)):
            if lines[j].lstrip().startswith("s_endpgm"):
                regs = []
                for k in range(j, min(len(lines), j + 400)):
                    mk = re.search(r";\s*(NumVgprs|NumSgprs|ScratchSize|Occupancy|SGPRSpill|sgpr_spill_count|vgpr_spill_count):?\s*(\d+)", lines[k])
                    if mk:
                        regs.append(f"{mk.group(1)} {mk.group(2)}")
                    if "; -- End function" in lines[k] and regs:
                        break
                print("   " + ", ".join(dict.fromkeys(regs)))
                break


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--asm":
        print(f"step loop of the headline tile kernels, gfx950, from {os.path.basename(sys.argv[2])}")
        report(sys.argv[2])
        return
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "trmc.s")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                               "-ffp-contract=off", "-gline-tables-only", "--cuda-device-only", "-S", "trmc.hip", "-o", asm],
                              cwd=CSRC)
        print("step loop of the headline tile kernels, gfx950, flags of the shipped build (-O3 -ffp-contract=off) + line tables")
        report(asm)


if __name__ == "__main__":
    main()
