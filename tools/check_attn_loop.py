#!/usr/bin/env python3
"""Build-time check of attention_p.hip's ISA: inside the tile loops of every attn64q / attn64p instantiation there must be NO scratch
operation and NO compiler-inserted `s_waitcnt vmcnt` (only the counted waits of the asm statements).  Either one drains the
LDS-DMA pipeline once per tile (a spilled register's reload counts on vmcnt with the DMA loads; a pending compiler-visible
load in front of the loop leaves its wait inside the loop): measured 145 / 165 us against 102 / 110.
Second check, every attn64q instantiation: the MFMA-write -> asm-read distance.  hipcc pads the wait states between an MFMA's write
of a VGPR and a vector read of it for its own instructions only, not for an asm statement's (the pair steps).  For each VGPR an asm
statement reads, the last MFMA that wrote it is found on every path into the statement (into the loop and round its back edge), and
the wait states in between are counted: one per instruction, N + 1 per `s_nop N`.  v_mfma_f32_32x32x16_bf16 (8 passes) needs 12.
The same counter is applied to hipcc's own vector reads of MFMA results: it must find none below 12, or the counting model is wrong.
    python tools/check_attn_loop.py          (compiles into a private temporary directory; exit code 1 on a finding)
    python tools/check_attn_loop.py --varlen (the same checks on attention_varlen.hip: the VARLEN instantiations)
    python tools/check_attn_loop.py --packed (the same checks on attention_packed.hip: the packed instantiations)"""
import os, re, subprocess, sys, tempfile
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = ("attention_varlen.hip" if "--varlen" in sys.argv[1:] else
       "attention_packed.hip" if "--packed" in sys.argv[1:] else "attention_p.hip")
tmp = tempfile.TemporaryDirectory()
out = os.path.join(tmp.name, "check_attn_loop.s")
subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", root + "/include", "-I",
                       root + "/ditto_tts_amd/csrc", "-w", "-fno-honor-nans", "-fno-slp-vectorize", "-S", "--cuda-device-only",
                       root + "/ditto_tts_amd/csrc/" + src, "-o", out])
s = open(out).read()
bad = 0
for name in re.findall(r"^(_ZN\S*attn64[pq]_kernel\S+):", s, re.M):
    i = s.index(name + ":"); j = s.index(".end_amdhsa_kernel", i)
    blocks = re.split(r"\n(\.LBB\d+_\d+):", s[i:j])
    for k in range(1, len(blocks), 2):
        b = blocks[k + 1]
        n = b.count("v_mfma")
        q = "attn64q" in name
        if q and (n not in (4, 28) or not b.count("v_exp") or b.count("v_exp") > 100):      # attn64q: the steady loop's two blocks (28 + 4 MFMAs)
            continue
        if not q and (n != 16 or "Loop" not in b.split("\n")[0] or not re.search(r"Li0ELb[01]EEEv", name)):   # attn64p: the 16-MFMA blocks of its tile loops (product instantiations, dense and VARLEN)
            continue
        in_asm, waits = False, 0
        for l in b.split("\n"):
            if "#ASMSTART" in l: in_asm = True
            elif "#ASMEND" in l: in_asm = False
            elif "vmcnt" in l and not in_asm: waits += 1
        scratch = b.count("scratch_")
        flag = "" if not (waits or scratch) else "   <-- PROBLEM"
        bad += bool(waits or scratch)
        print(f"{name[-44:]:46s} {blocks[k]:10s} mfma {n:2d}  scratch {scratch}  compiler vmcnt waits {waits}{flag}")

# ---- MFMA -> asm read distance (attn64q) ----
NEED = 12          # wait states after v_mfma_f32_32x32x16_bf16 (8 passes) before a vector instruction reads its result
HORIZON = 600      # how far back producers are looked for (a whole loop iteration and more)


def vregs(op):
    m = re.fullmatch(r"v(\d+)", op) or re.fullmatch(r"v\[(\d+):(\d+)\]", op)
    if not m:
        return set()
    lo = int(m.group(1)); hi = int(m.group(2)) if m.lastindex == 2 else lo
    return set(range(lo, hi + 1))


def parse(text):
    """basic blocks of one kernel: [(label, [insn]), ...], insn = (mnemonic, [operands], in_asm, waits); successor lists"""
    blocks, cur, in_asm = [("entry", [])], None, False
    for raw in text.split("\n"):
        l = raw.split(";")[0].strip() if "#ASM" not in raw else raw.strip()
        if "#ASMSTART" in l: in_asm = True; continue
        if "#ASMEND" in l: in_asm = False; continue
        if re.match(r"^\.LBB\d+_\d+:", l):
            blocks.append((l[:-1], [])); continue
        if not l or l.startswith(".") or l.endswith(":"):
            continue
        parts = l.split(None, 1)
        mn = parts[0]
        ops = [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []
        waits = int(ops[0], 0) + 1 if mn == "s_nop" else 1
        blocks[-1][1].append((mn, ops, in_asm, waits))
    names = [b[0] for b in blocks]
    succ = []
    for i, (_, ins) in enumerate(blocks):
        s_ = []
        last = ins[-1] if ins else None
        if last and last[0].startswith("s_cbranch") or last and last[0] == "s_branch":
            s_.append(names.index(last[1][0]))
        if i + 1 < len(blocks) and not (last and last[0] in ("s_branch", "s_endpgm", "s_setpc_b64")):
            s_.append(i + 1)
        succ.append(s_)
    pred = [[] for _ in blocks]
    for i, s_ in enumerate(succ):
        for j in s_: pred[j].append(i)
    return blocks, pred


def writes(mn, ops):
    if mn.startswith(("s_", "ds_write", "ds_store", "global_store", "buffer_store", "scratch_store")) or "lds" in mn or not ops:
        return set()
    w = vregs(ops[0])
    if mn.startswith("v_permlane") and len(ops) > 1: w |= vregs(ops[1])
    return w


def reads(mn, ops):
    if mn.startswith("s_") or not ops:
        return set()
    src = ops if mn.startswith(("ds_write", "ds_store", "global_store", "buffer_store", "scratch_store")) or "lds" in mn else ops[1:]
    r = set()
    for o in src: r |= vregs(o)
    return r


def distance(blocks, pred, bi, ii, reg):
    """fewest wait states between the read at blocks[bi][ii] and an MFMA that last wrote `reg` on some path (None: none within HORIZON)"""
    best, seen, stack = None, {}, [(bi, ii, 0)]
    while stack:
        b, i, d = stack.pop()
        ins = blocks[b][1]
        stop = False
        for k in range(i - 1, -1, -1):
            mn, ops, _, w = ins[k]
            if reg in writes(mn, ops):
                if mn.startswith("v_mfma"): best = d if best is None else min(best, d)
                stop = True; break
            d += w
            if d >= HORIZON: stop = True; break
        if stop: continue
        for p in pred[b]:
            if seen.get(p, HORIZON + 1) > d:
                seen[p] = d
                stack.append((p, len(blocks[p][1]), d))
    return best


for name in re.findall(r"^(_ZN\S*attn64q_kernel\S+):", s, re.M):
    i = s.index(name + ":"); j = s.index(".end_amdhsa_kernel", i)
    blocks, pred = parse(s[i:j])
    asm_reads = asm_mfma = 0; asm_min = cal_min = None; cal_n = 0
    for bi, (_, ins) in enumerate(blocks):
        for ii, (mn, ops, in_asm, _) in enumerate(ins):
            if not mn.startswith("v_") or mn.startswith("v_mfma"):
                continue
            own = set()      # registers the same asm statement wrote before this instruction: not MFMA results
            if in_asm:
                k = ii - 1
                while k >= 0 and ins[k][2]: own |= writes(ins[k][0], ins[k][1]); k -= 1
            for reg in reads(mn, ops) - own:
                dist = distance(blocks, pred, bi, ii, reg)
                if in_asm:
                    asm_reads += 1
                    if dist is not None: asm_mfma += 1; asm_min = dist if asm_min is None else min(asm_min, dist)
                elif dist is not None:
                    cal_n += 1; cal_min = dist if cal_min is None else min(cal_min, dist)
    short = asm_min is not None and asm_min < NEED
    model = cal_min is not None and cal_min < NEED
    bad += bool(short or model or not asm_mfma or not cal_n)
    print(f"{name[-44:]:46s} asm reads {asm_reads:4d}  of MFMA results {asm_mfma:4d}  min wait states {asm_min}  "
          f"(hipcc's own reads {cal_n}, min {cal_min})" + ("   <-- SHORTFALL" if short else "") + ("   <-- MODEL WRONG" if model else "")
          + ("   <-- NOTHING ANALYSED" if not asm_mfma or not cal_n else ""))
sys.exit(1 if bad else 0)
