"""The launches of one forward follow its plan (csrc/forward_plan.hip): under every pinned kernel class the engine's profile
scopes count exactly the launches of that class, and ditto_full_row_plan_opts answers what the forward then does.

d = 768, 12 heads, L = 2, B = 2, N = 128, T = 64 (256 rows: enough for every class's kernels, the 128-row ones included), synthetic
weights, default options.  Every kernel class but `layernorm` has the same count under every pin; the LayerNorm LAUNCHES tell the
classes apart (counts read off the parent commit's forward with this same body):

    pin 1024   low-latency: fc2's finish chains norm1, the out-projection's finish writes norm3     L      = 2
    pin 4096   tiled                                                                                3L - 1 = 5
    pin 8192   tiled, norm2 fused into the q-projection                                             2L - 1 = 3
    pin 11264  64-row full-row                                                                      0
    pin 16384  the exact-round exception: tiled, with the fused q-projection                        2L - 1 = 3
    pin 32768  128-row full-row, bf16 stream                                                        0

Under the 1024 pin the four ll_mask values give 3L - 1, 2L, 2L - 1 and L LayerNorm launches.  Bit 0 changes no bit of eps; bit 1
does (the out-projection summed as two K halves: rel-L2 3.6e-5 here, on the parent commit as on this one), as kernels.h says and
tests/test_gpu_model.py::test_low_latency_class_fusions_change_no_bit already holds it to.
"""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.modules import DiTTO
from ditto_tts_amd.synth import synthetic_inputs, synthetic_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
L, B, N, T = 2, 2, 128, 64
CFG = DiTTOConfig(768, L, 12, 256, 768, 50)
# pin -> (layernorm scopes, (outproj, fc2) of the plan, bf16 stream)
CLASSES = {1024: (L, (False, False), False), 4096: (3 * L - 1, (False, False), False), 8192: (2 * L - 1, (False, False), False),
           11264: (0, (True, True), False), 16384: (2 * L - 1, (False, False), False), 32768: (0, (True, True), True)}
FIXED = {"adaln": 1, "gemm_qkv_rope": L, "attn_self": L, "gemm_q_proj": L, "attn_cross": L, "gemm_out_proj": L, "gemm_gated_mlp": L,
         "gemm_fc2": L, "gemm_final": 1, "p_sample_update": 0}


def counted_forward(eng, x, cond, t):
    """eps of one forward and the number of profile scopes per kernel class it opened"""
    eng.profile_read()                       # drop anything pending
    eps = eng.forward(x, cond, t)
    torch.cuda.synchronize()
    return eps, {k: n for k, (n, _) in eng.profile_read().items()}


@torch.no_grad()
def test_launches_per_pinned_class_follow_the_plan():
    m = DiTTO(CFG.hidden_dim, CFG.num_layers, CFG.num_heads, CFG.time_dim, CFG.text_dim, CFG.diffusion_steps)
    m.load_state_dict(synthetic_state_dict(CFG, 7))
    eng = m.to(DEV).eval().engine()
    x, text, t = (z.to(DEV) for z in synthetic_inputs(CFG, B, N, T, seed=8))
    cond = eng.prepare_text(text, N)
    eng.profile_enable(True)
    try:
        for pin, (layernorms, plan, bf16) in CLASSES.items():
            with hip.batch_class(pin):
                eps, got = counted_forward(eng, x, cond, t)
                print(f"pin {pin}: {got}")
                assert torch.isfinite(eps).all()
                assert got == {**FIXED, "layernorm": layernorms}, f"pin {pin}"
                assert hip.full_row_plan(CFG, B, N) == plan, f"pin {pin}"
                assert hip.stream_is_bf16(CFG, B, N) == bf16, f"pin {pin}"
        # The low-latency class without its launch fusions (ll_mask 0): every norm1 but block 0's and every norm3 is a LayerNorm
        # launch again, 3L - 1 in all.  Bit 0 (fc2's finish writes the next norm1) is a launch fusion only: the same eps bits with
        # and without it.  Bit 1 runs the out-projection as TWO K-splits: another summation order, so eps moves by fp32
        # accumulation noise (measured on the parent commit, as here: not bit-equal; 3e-3 is test_gpu_model.py's bound for it).
        with hip.batch_class(1024):
            eps, want = {}, {0: 3 * L - 1, 1: 2 * L, 2: 2 * L - 1, 3: L}
            try:
                for mask in (0, 1, 2, 3):
                    hip.set_option("ll_mask", mask)
                    eps[mask], got = counted_forward(eng, x, cond, t)
                    print(f"pin 1024, ll_mask {mask}: {got}")
                    assert got == {**FIXED, "layernorm": want[mask]}, f"ll_mask {mask}"
            finally:
                hip.set_option("ll_mask", 3)
            rel = float(torch.linalg.norm(eps[0].double() - eps[3].double()) / torch.linalg.norm(eps[3].double()))
            print(f"eps: ll_mask 0 == 1 {torch.equal(eps[0], eps[1])}, 2 == 3 {torch.equal(eps[2], eps[3])}, 0 against 3 rel-L2 {rel:.3e}")
            assert torch.equal(eps[0], eps[1]) and torch.equal(eps[2], eps[3])
            assert not torch.equal(eps[0], eps[3]) and rel < 3e-3
    finally:
        eng.profile_enable(False)
        eng.profile_read()
