"""ISA-level invariants of csrc/gemm_frd.hip (the full-row N = 768 GEMM), checked on the cross-compiled code (no GPU needed).

The kernel runs ONE wave per SIMD with 384 pinned fp32 accumulators per lane (256 in AGPRs, 128 in VGPRs) and a main loop whose
every wait is a hand-counted `s_waitcnt vmcnt(N)` (frd_vm).  A spill, a compiler-inserted vmcnt wait in the loop (it turns the
counted waits into drains) or an LDS image beyond the CU's 160 KiB breaks it silently; the bf16 stream's prologue stages the
residual tile through the LDS by hand-written LDS-DMA and must leave all of that as it was."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
CSRC = os.path.join(ROOT, "ditto_tts_amd", "csrc")
SRC = os.path.join(CSRC, "gemm_frd.hip")


@pytest.fixture(scope="module")
def compiled():
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-I", CSRC, "-w", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", "-", SRC],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    bodies = {}
    for m in re.finditer(r"^(_ZN5ditto\S*gemm_frd_kernel[^\s:]+):[^\n]*\n(.*?)^\s*s_endpgm", r.stdout, re.S | re.M):
        bodies[m.group(1)] = m.group(2).splitlines()
    usage = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)"
                         r".*?VGPRs Spill: (\d+)", r.stderr, re.S):
        usage[m.group(1)] = dict(zip(("vgpr", "agpr", "scratch", "occupancy", "spill"), map(int, m.groups()[1:])))
    private = {m.group(1): int(m.group(2)) for m in
               re.finditer(r"\.amdhsa_kernel (\S+).*?\.amdhsa_private_segment_fixed_size (\d+)", r.stdout, re.S)}
    assert len(bodies) == 7 and set(bodies) == {k for k in usage if "gemm_frd_kernel" in k}, (sorted(bodies), sorted(usage))
    return bodies, usage, private


def _loops(lines):
    """(first, last) line ranges closed by a backward branch"""
    label = {}
    out = []
    for i, l in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            label[m.group(1)] = i
        m = re.match(r"^\s*s_cbranch_\w+\s+(\.LBB\d+_\d+)", l) or re.match(r"^\s*s_branch\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in label:
            out.append((label[m.group(1)], i))
    return out


def test_no_scratch_in_any_instantiation(compiled):
    bodies, usage, private = compiled
    for name, lines in bodies.items():
        assert usage[name]["scratch"] == 0 and usage[name]["spill"] == 0 and private[name] == 0, (name, usage[name])
        assert not [l for l in lines if re.match(r"^\s*(scratch_|buffer_(load|store)\S* .*\boffen\b.*\bs\[0:3\])", l)], name


def test_k_loop_waits_are_the_hand_counted_ones(compiled):
    """Inside the K loop every `s_waitcnt` that names vmcnt sits in an asm statement of the source (between #ASMSTART / #ASMEND):
    hipcc adds none of its own, and none of the loop's waits is a drain (vmcnt(0))."""
    bodies, _, _ = compiled
    for name, lines in bodies.items():
        kloops = [(a, b) for a, b in _loops(lines) if sum("v_mfma_f32_32x32x16_bf16" in l for l in lines[a:b]) >= 96]
        assert len(kloops) == 1, (name, kloops)                     # the slab loop: 4 stages x 24 MFMAs
        a, b = kloops[0]
        in_asm, mine, theirs = False, [], []
        for l in lines[a:b]:
            if "#ASMSTART" in l:
                in_asm = True
            elif "#ASMEND" in l:
                in_asm = False
            elif re.search(r"s_waitcnt\b.*vmcnt", l):
                (mine if in_asm else theirs).append(l.strip())
        assert not theirs, (name, theirs)
        assert len(mine) == 25, (name, len(mine))                   # 24 W fragments + the next A slab
        assert not [w for w in mine if re.search(r"vmcnt\(0\)", w)], (name, mine)
        assert not [l for l in lines[a:b] if re.match(r"^\s*scratch_", l)], name


def test_lds_image_fits_the_cu(compiled):
    """The launch asks for D_LDS bytes of dynamic LDS (no static LDS in the kernel): at most the 160 KiB of a gfx950 CU, and the
    bf16 stream's residual staging (two units per wave behind the bias row) ends inside it."""
    bodies, _, _ = compiled
    env = {}
    for st in re.finditer(r"^constexpr int ([^;()]+);", open(SRC).read(), re.M):       # the file-scope layout constants, in order
        for name, expr in re.findall(r"(\w+) = (.+?)(?:, (?=\w+ = )|$)", st.group(1)):
            env[name] = eval(expr, {"__builtins__": {}}, dict(env))
    assert env["D_LDS"] <= 160 * 1024, env["D_LDS"]
    assert env["D_RSTG"] >= env["D_BIAS"] + 768 * 4 and env["D_RSTG"] + 4 * 2 * env["D_RUNIT"] <= env["D_LDS"], env
    text = subprocess.run(["grep", "-c", "D_LDS, s, fp", SRC], capture_output=True, text=True).stdout
    assert int(text) == 1                                            # the one launch site passes D_LDS


def test_register_budget_is_one_wave_per_simd_with_384_pinned_accumulators(compiled):
    """256 accumulators in AGPRs + 128 in VGPRs + the W ring, A fragments and addresses: inside 512 registers per lane, i.e. one
    wave per SIMD, which is what __launch_bounds__(256, 1) plans for."""
    _, usage, _ = compiled
    for name, u in usage.items():
        if "gemm_frd_kernel" not in name:
            continue
        assert u["agpr"] == 256 and 128 < u["vgpr"] <= 256 and u["occupancy"] >= 1, (name, u)


def test_bf16_stream_prologue_stages_the_residual_through_the_lds(compiled):
    """<LN, RES, HB> with RES and HB: 48 LDS-DMA pieces and 96 ds_read_b64 per wave in front of the main loop, and no 8-byte global
    load in the accumulator layout left."""
    bodies, _, _ = compiled
    for name, lines in bodies.items():
        m = re.search(r"gemm_frd_kernelILb(\d)ELb(\d)ELb(\d)EE", name)
        ln, res, hb = (int(x) for x in m.groups())
        a = min(a for a, b in _loops(lines) if sum("v_mfma" in l for l in lines[a:b]) >= 96)
        pro = lines[:a]
        dma = sum("global_load_lds_dwordx4" in l for l in pro)
        rd = sum(bool(re.match(r"^\s*ds_read_b64\b", l)) for l in pro)
        if res and hb:
            assert dma >= 48 + 4 and rd == 96, (name, dma, rd)
            assert not [l for l in pro if "global_load_dwordx2" in l], name
        else:
            assert dma <= 3 + 4 + 4 and rd == 0, (name, dma, rd)
