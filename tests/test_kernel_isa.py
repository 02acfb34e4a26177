"""ISA-level invariants of the hand-scheduled kernels, checked on the cross-compiled code (no GPU needed)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_attention_tile_loops_hold_no_scratch_and_no_compiler_vmcnt_wait():
    """attn64q's tile loops run behind COUNTED `s_waitcnt vmcnt` of their LDS-DMA loads.  A spilled register reloaded in the loop, or a
    compiler-visible load left pending in front of it, puts another vmcnt wait inside the loop and turns every counted wait into a
    drain (measured 145 / 165 us against 102 / 110).  tools/check_attn_loop.py compiles attention_p.hip and scans the loop blocks of
    every instantiation for both."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_attn_loop.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("mfma 28") >= 6 and "PROBLEM" not in r.stdout, r.stdout


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_attn64q_asm_pair_steps_read_mfma_results_after_enough_wait_states():
    """hipcc pads the MFMA-write -> vector-read wait states of its own instructions only; the asm pair steps of attn64q read score
    accumulators whose MFMAs hipcc schedules (the prologue's freely).  tools/check_attn_loop.py follows every path into each asm
    read back to the MFMA that wrote the register and counts the wait states: >= 12 for v_mfma_f32_32x32x16_bf16, and its counter
    must see hipcc's own reads of MFMA results at >= 12 too.  At least the 32 pair steps x 2 registers of each instantiation's loop
    must have been analysed (no vacuous pass)."""
    import re
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_attn_loop.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = re.findall(r"asm reads\s+(\d+)\s+of MFMA results\s+(\d+)\s+min wait states (\d+)\s+\(hipcc's own reads (\d+), min (\d+)\)",
                      r.stdout)
    assert len(rows) == 6, r.stdout                       # every attn64q instantiation
    for _, n_mfma, dmin, n_own, own_min in rows:
        assert int(n_mfma) >= 64 and int(dmin) >= 12, r.stdout
        assert int(n_own) > 0 and int(own_min) >= 12, r.stdout
    assert "SHORTFALL" not in r.stdout and "MODEL WRONG" not in r.stdout and "NOTHING ANALYSED" not in r.stdout
    print("\n".join(l for l in r.stdout.splitlines() if "asm reads" in l))
