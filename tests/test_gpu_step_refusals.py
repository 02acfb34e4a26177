"""-m gpu: which refusal comes FIRST from each of the 13 ditto_guided_step_packed*_opts entries, through the C ABI alone.

Every call here passes workspace_bytes = 0.  The step's forward refuses that last of all, before anything is launched
(DITTO_ERR_SIZE, "workspace too small"), so no row launches a kernel whatever the entry does; with every other argument valid that
refusal is the one reported (the always-on rows: the arguments reach the forward), and with one defect the defect's own refusal has
to come first — its return code, a distinctive part of ditto_last_error and the entry's name in it.  The expected codes and texts are
written by hand from the entries' argument checks.  Launches: creating the model and preparing the text conditioning, nothing else."""
import ctypes as C

import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.modules import DiTTO
from ditto_tts_amd.synth import hash_normal, synthetic_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = DiTTOConfig(256, 2, 4, 256, 256, 50)
B, LENS, TEXTS = 2, (5, 9), (3, 4)
S, MAX_N, S_T, MAX_T, D = sum(LENS), max(LENS), sum(TEXTS), max(TEXTS), CFG.hidden_dim
G, S_G = 1, LENS[0]                                   # the mixed step: utterance 0 is guided, its copy in rows [S, S + 5)
ARG, SHAPE, SIZE = hip.ERR_ARG, hip.ERR_SHAPE, hip.ERR_SIZE
GUARD = (SIZE, "workspace too small")

# the names this file gives to parameters the header spells out; the host struct `step` of the multistep entries is "mstep" here,
# beside the strided entries' Philox tag `step`
ALIAS = {"x2": "x", "cu_speech": "cu", "cu_text": "cut", "prompt_len": "pl", "suffix_len": "ql", "rope_cos": "rc", "rope_sin": "rs",
         "workspace": "ws", "workspace_bytes": "wsb"}


def _by_name(entry, args):
    """`args` (this file's names) as the keyword arguments of hip.call: the parameter names of include/ditto_hip.h"""
    return {name: args["mstep" if name == "step" and ctype is C.c_void_p else ALIAS.get(name, name)]
            for name, ctype in hip.PROTOTYPES[entry][1]}


STRIDED = [f"ditto_guided_step_packed_{k}opts" for k in ("", "tags_", "prompt_", "tags_prompt_", "window_", "tags_window_")]
MIXED, RESCALE, MS_RESCALE = (f"ditto_guided_step_packed_{k}_opts" for k in ("mixed", "rescale", "multistep_rescale"))
REUSE, MS_REUSE = "ditto_guided_step_packed_reuse_opts", "ditto_guided_step_packed_multistep_reuse_opts"
MULTISTEP = ["ditto_guided_step_packed_multistep_opts", "ditto_guided_step_packed_multistep_window_opts"]
assert sorted(STRIDED + MULTISTEP + [MIXED, RESCALE, MS_RESCALE, REUSE, MS_REUSE]) == \
    sorted(n for n in hip.PROTOTYPES if n.startswith("ditto_guided_step_packed"))                 # the 13 entries of the header

BIG = dict(B=32768, S=40000)                          # past the step kernels' 32767 utterances, within every other limit
POSITIVE = "S_T and max_T must be positive"           # check_packed
ROWS_LE = "need max_N <= S"                           # check_packed
IN_RANGE = "S must lie in [1, 2^30)"
TOO_MANY = "more than 32767 utterances"
NULL_X = "null x2 / eps2"
NEEDS_W = "classifier-free guidance needs w"
EXCLUSIVE = "noise and seeds are exclusive"
ALIGNED = "the rescale scratch must be 256-byte aligned"
NEEDS_BYTES = "the rescale scratch needs"


def _rows():
    """(entry, id, overrides of the valid call, expected code, expected part of the message)"""
    rows = []

    def add(entry, what, over, code, text, variant=""):
        rows.append(pytest.param(entry, variant, over, code, text, id=f"{entry[len('ditto_guided_step_packed_'):-5] or 'plain'}{variant}-{what}"))

    for e in STRIDED:                                 # m; check_guided_update; seeds need tags; the limits
        add(e, "guard", {}, *GUARD)
        add(e, "model_null", dict(m=None), ARG, "bad argument to")
        add(e, "x2_null", dict(x=None), ARG, NULL_X)
        add(e, "noise_and_seeds", dict(noise="noise", seeds="seeds"), ARG, EXCLUSIVE)
        add(e, "cfg_without_w", dict(w=None), ARG, NEEDS_W)
        add(e, "B_0", dict(B=0), SHAPE, "B, N and d must be positive")
        add(e, "B_32768", BIG, SHAPE, TOO_MANY)
        add(e, "S_0", dict(S=0), SHAPE, IN_RANGE)
        add(e, "S_2_30", dict(S=1 << 30), SHAPE, IN_RANGE)
        if "prompt" in e:
            add(e, "prompt_len_null", dict(pl=None), ARG, "null prompt_len (int32 [B])")
        if "window" in e:
            add(e, "suffix_len_null", dict(ql=None), ARG, "null suffix_len (int32 [B])")
    for e in MULTISTEP:                               # m; check_multistep; the limits
        add(e, "guard", {}, *GUARD)
        add(e, "model_null", dict(m=None), ARG, "bad argument to")
        add(e, "x2_null", dict(x=None), ARG, "null x2 / eps2 / q / cu")
        add(e, "q_null", dict(q=None), ARG, "null x2 / eps2 / q / cu")
        add(e, "step_null", dict(mstep=None), ARG, "exactly one of step (host) and coefs")
        add(e, "cfg_without_w", dict(w=None), ARG, NEEDS_W)
        add(e, "B_0", dict(B=0), SHAPE, "B, max_N and d must be positive")
        add(e, "B_32768", BIG, SHAPE, TOO_MANY)
        add(e, "S_0", dict(S=0), SHAPE, IN_RANGE)
        add(e, "S_2_30", dict(S=1 << 30), SHAPE, IN_RANGE)
        if "window" in e:
            add(e, "suffix_len_null", dict(ql=None), ARG, "null suffix_len (int32 [B])")
    for e, v in ((MIXED, ""), (RESCALE, "+partner")):  # [w]; m; check_mixed (check_packed inside); the limits; check_rescale
        add(e, "guard", {}, *GUARD, v)
        add(e, "model_null", dict(m=None), ARG, "bad argument to", v)
        add(e, "x2_null", dict(x=None), ARG, NULL_X, v)
        add(e, "noise_and_seeds", dict(noise="noise", seeds="seeds"), ARG, EXCLUSIVE, v)
        add(e, "cfg_without_w", dict(w=None), ARG, NEEDS_W if e == MIXED else "guidance rescale needs w", v)
        add(e, "B_0", dict(B=0), SHAPE, "B, N and d must be positive", v)
        add(e, "B_32768", BIG, SHAPE, TOO_MANY, v)
        add(e, "S_0", dict(S=0), SHAPE, POSITIVE, v)
        add(e, "S_2_30", dict(S=1 << 30), SHAPE, IN_RANGE, v)
        add(e, "max_N_S_plus_1", dict(max_N=S + 1), SHAPE, ROWS_LE, v)
        add(e, "G_above_B", dict(G=B + 1, S_G=S), SHAPE, "need 0 <= G <= B", v)
    add(MIXED, "partner_null", dict(partner=None), ARG, "null cu / partner")
    add(RESCALE, "misaligned_scratch", dict(scratch="scratch+16"), ARG, ALIGNED, "+partner")
    add(RESCALE, "small_scratch", dict(scratch_bytes="need-1"), SIZE, NEEDS_BYTES, "+partner")
    e = RESCALE                                       # partner NULL: w; m; check_rescale (check_packed inside); check_guided_update; limits
    add(e, "guard", {}, *GUARD)
    add(e, "model_null", dict(m=None), ARG, "bad argument to")
    add(e, "x2_null", dict(x=None), ARG, "null eps2 / phi / cu / scratch")
    add(e, "noise_and_seeds", dict(noise="noise", seeds="seeds"), ARG, EXCLUSIVE)
    add(e, "cfg_without_w", dict(w=None), ARG, "guidance rescale needs w")
    add(e, "B_0", dict(B=0), SHAPE, POSITIVE)
    add(e, "B_32768", BIG, SHAPE, TOO_MANY)
    add(e, "S_0", dict(S=0), SHAPE, POSITIVE)
    add(e, "S_2_30", dict(S=1 << 30), SHAPE, IN_RANGE)
    add(e, "max_N_S_plus_1", dict(max_N=S + 1), SHAPE, ROWS_LE)
    add(e, "misaligned_scratch", dict(scratch="scratch+16"), ARG, ALIGNED)
    add(e, "small_scratch", dict(scratch_bytes="need-1"), SIZE, NEEDS_BYTES)
    e = MS_RESCALE                                    # m; check_multistep; the limits; check_rescale (check_packed inside)
    add(e, "guard", {}, *GUARD)
    add(e, "model_null", dict(m=None), ARG, "bad argument to")
    add(e, "x2_null", dict(x=None), ARG, "null x2 / eps2 / q / cu")
    add(e, "q_null", dict(q=None), ARG, "null x2 / eps2 / q / cu")
    add(e, "coefs_null", dict(coefs=None), ARG, "exactly one of step (host) and coefs")
    add(e, "B_0", dict(B=0), SHAPE, "B, max_N and d must be positive")
    add(e, "B_32768", BIG, SHAPE, TOO_MANY)
    add(e, "S_0", dict(S=0), SHAPE, IN_RANGE)
    add(e, "S_2_30", dict(S=1 << 30), SHAPE, IN_RANGE)
    add(e, "max_N_S_plus_1", dict(max_N=S + 1), SHAPE, ROWS_LE)
    add(e, "misaligned_scratch", dict(scratch="scratch+16"), ARG, ALIGNED)
    add(e, "small_scratch", dict(scratch_bytes="need-1"), SIZE, NEEDS_BYTES)
    for e in (REUSE, MS_REUSE):                       # m; [step]; check_guided_update / check_multistep; check_reuse; the limits
        ms = e == MS_REUSE
        add(e, "guard", {}, *GUARD)
        add(e, "guard_store", dict(mode=1), *GUARD)
        add(e, "model_null", dict(m=None), ARG, "bad argument to")
        add(e, "x2_null", dict(x=None), ARG, "null x2 / eps2 / q / cu" if ms else NULL_X)
        add(e, "cfg_without_w", dict(w=None), ARG, NEEDS_W)
        add(e, "B_0", dict(B=0), SHAPE, "B, max_N and d must be positive" if ms else "B, N and d must be positive")
        add(e, "B_32768", BIG, SHAPE, TOO_MANY)
        add(e, "S_0", dict(S=0), SHAPE, POSITIVE)
        add(e, "S_2_30", dict(S=1 << 30), SHAPE, IN_RANGE)
        add(e, "max_N_S_plus_1", dict(max_N=S + 1), SHAPE, ROWS_LE)
        add(e, "delta_null", dict(delta=None), ARG, "null delta (fp32 [S, d])")
        add(e, "mode_3", dict(mode=3), ARG, "mode must be 1 (STORE) or 2 (LOAD), not 3")
        add(e, "store_with_mirror", dict(mode=1, mirror=1), ARG, "mirror belongs to LOAD")
        if ms:
            add(e, "q_null", dict(q=None), ARG, "null x2 / eps2 / q / cu")
            add(e, "step_null", dict(mstep=None), ARG, "null step (host ditto_multistep_coef)")
        else:
            add(e, "noise_and_seeds", dict(noise="noise", seeds="seeds"), ARG, EXCLUSIVE)
    return rows


@pytest.fixture(scope="module")
def valid():
    """every argument of every entry by name, valid but for wsb = 0, and what owns the memory behind the pointers"""
    model = DiTTO(CFG.hidden_dim, CFG.num_layers, CFG.num_heads, CFG.time_dim, CFG.text_dim, CFG.diffusion_steps)
    model.load_state_dict(synthetic_state_dict(CFG, seed=3))
    eng = model.to(DEV).eval().engine(torch.device("cuda:0"))
    lib = hip.lib()
    ct = [0, TEXTS[0], S_T]
    text = hash_normal((2 * S_T, CFG.text_dim), "refusal_text", 1).to(DEV)
    cond = eng.prepare_text_packed(text, ct + [S_T + c for c in ct[1:]])              # [text; null]: 2B utterances over 2 S_T rows
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)                   # noqa: E731
    f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=DEV)        # noqa: E731
    need = int(lib.ditto_guidance_rescale_bytes(B, MAX_N, D))
    rc, rs = eng.rope_tables(MAX_N)
    keep = dict(x=f32(2 * S, D), cond=cond.buf, t=torch.zeros(2 * B, dtype=torch.int64, device=DEV),
                cu=i32([0, LENS[0], S, S + LENS[0], 2 * S]), cut=cond.cu_seqlens, noise=f32(S, D),
                seeds=torch.zeros(B, dtype=torch.int64, device=DEV), tags=i32([0] * B), w=f32(B), a=f32(B), ce=f32(B), cz=f32(B),
                phi=f32(B), pl=i32([1, 0]), ql=i32([0, 2]), q=f32(S, D), delta=f32(S, D), coefs=f32(B, 8), partner=i32([0, -1]),
                scratch=torch.zeros(need + 256, dtype=torch.uint8, device=DEV), rc=rc, rs=rs, ws=eng.workspace_packed(2 * B, 2 * S, 2 * S_T))
    torch.cuda.synchronize()
    v = {k: t.data_ptr() for k, t in keep.items()}
    assert v["scratch"] % 256 == 0 and v["coefs"] % 16 == 0
    v.update(m=eng.handle, mstep=hip.MultistepCoef(0.8, 1.9, -1.6, 0.4, -0.1, 0.0, 1, 0), step=0, B=B, S=S, max_N=MAX_N, S_T=2 * S_T,
             max_T=MAX_T, cfg=1, G=G, S_G=S_G, mode=2, mirror=0, wsb=0, scratch_bytes=need, stream=None, opts=None)
    return lib, v, (keep, eng, model)                                                # alive for the module: the handle is the engine's


@pytest.mark.parametrize("entry, variant, over, code, text", _rows())
def test_first_refusal(valid, entry, variant, over, code, text):
    lib, v, _ = valid
    args = dict(v, noise=None, seeds=None)                                           # by default no noise: cz is never read
    if entry in MULTISTEP:
        args["coefs"] = None                                                         # the host step's form
    if entry == RESCALE and not variant:
        args.update(partner=None, G=0, S_G=0)
    for k, val in over.items():
        if val == "scratch+16":
            val = v["scratch"] + 16
        elif val == "need-1":
            val = v["scratch_bytes"] - 1
        elif isinstance(val, str):
            val = v[val]
        args[k] = val
    if args["B"] != B:                                                               # the scratch a batch of that size would need
        args["scratch_bytes"] = int(lib.ditto_guidance_rescale_bytes(max(args["B"], 1), MAX_N, D))
    rc = hip.call(entry, **_by_name(entry, args))
    msg = lib.ditto_last_error().decode()
    print(f"{entry} {over}: rc {rc}, {msg!r}")
    assert rc == code and text in msg, (rc, msg)
    if (code, text) != GUARD:
        assert entry in msg                                                          # the refusal names its entry
