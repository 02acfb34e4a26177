"""The C-ABI library loads on a GPU-less host and exports every symbol include/ditto_hip.h declares.
No compute call is made here."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from ditto_tts_amd import hip
from ditto_tts_amd.config import PRESETS, DiTTOConfig


def declared_functions():
    txt = open(os.path.join(ROOT, "include", "ditto_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(ditto_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_exported_and_bound():
    names = declared_functions()
    assert len(names) >= 20
    lib = hip.lib()
    for n in names:
        assert hasattr(lib, n), f"{n} declared in ditto_hip.h but not exported by libditto_hip.so"
        assert n in hip.SYMBOLS, f"{n} has no ctypes prototype in ditto_tts_amd/hip.py"
    assert sorted(hip.SYMBOLS) == names
    assert lib.ditto_abi_version() == 10


def test_train_rows_header_declared_exported_and_bound():
    """include/ditto_train_rows.h, a table of its own beside ditto_hip.h's: declared = exported = bound"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ditto_train_rows.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ditto_[a-z0-9_]+)\s*\(", txt)))
    assert len(names) == 15 and all(n.startswith("ditto_bwd_") for n in names)
    assert sorted(hip.TRAIN_ROWS_PROTOTYPES) == sorted(hip.TRAIN_ROWS_SYMBOLS) == names
    assert not set(names) & set(hip.SYMBOLS) and not set(names) & set(hip.OPTIM_SYMBOLS)
    lib = hip.lib()
    for n in names:
        fn = getattr(lib, n)                                                         # AttributeError: declared but not exported
        res, params = hip.TRAIN_ROWS_PROTOTYPES[n]
        assert fn.restype is res and list(fn.argtypes) == [t for _, t in params], n
        pnames = [p for p, _ in params]
        assert len(set(pnames)) == len(pnames), n
        if res is C.c_int:                                                            # every pointer is followed by its byte size
            for i, (p, t) in enumerate(params):
                if t is C.c_void_p and p != "stream":
                    assert params[i + 1] == (p + "_bytes", C.c_size_t), (n, p)
    assert hip.TRAIN_ROWS_PROTOTYPES["ditto_bwd_colsum_scratch_bytes"] == (C.c_size_t, [("M", C.c_int), ("n", C.c_int)])
    assert hip.TRAIN_ROWS_PROTOTYPES["ditto_bwd_reduce_partials"][1][4:6] == [("chunks", C.c_int), ("n", C.c_size_t)]
    assert hip.TRAIN_ROWS_PROTOTYPES["ditto_bwd_softmax_rows"][1][11] == ("seed", C.c_uint64)


def test_prototypes_are_parsed_from_the_header():
    """hip.PROTOTYPES (and SYMBOLS, its view) come from include/ditto_hip.h by one type rule: the same functions as the name
    scan above, distinct parameter names, and the declarations that are awkward to parse."""
    P, vp, i, sz = hip.PROTOTYPES, C.c_void_p, C.c_int, C.c_size_t
    assert sorted(P) == declared_functions() and len(P) == 143
    for name, (res, params) in P.items():
        names = [n for n, _ in params]
        assert len(set(names)) == len(names) and all(n.isidentifier() for n in names), name
        assert hip.SYMBOLS[name] == (res, [t for _, t in params])
    assert P["ditto_last_error"] == (C.c_char_p, [])                                  # returns const char*, (void)
    assert P["ditto_abi_version"] == (i, [])
    assert P["ditto_slp_destroy"] == (None, [("m", vp)])                              # returns void
    assert P["ditto_set_option"][1] == [("name", C.c_char_p), ("value", i)]
    assert P["ditto_regroup_packed"][1] == [("table", vp), ("n_seg", i), ("src", vp), ("src_bytes", vp), ("dst", vp),   # const void* const*,
                                            ("dst_bytes", vp), ("n_bufs", i), ("seeds", vp), ("n_seeds", i),            # const size_t*
                                            ("max_bytes", sz), ("stream", vp)]
    assert P["ditto_noise_normal"][1][2] == ("step", C.c_uint32)                      # uint32_t step
    assert P["ditto_guided_step_packed_multistep_opts"][1][8:10] == [("step", vp), ("coefs", vp)]   # host struct and device array
    co = hip.MultistepCoef(0.5, 1.0, 0.0, 0.0, 0.0, 0.0, 0, 0)                         # ... so a bare host struct goes by reference
    same = C.CFUNCTYPE(vp, vp)(lambda p: p)
    assert same(co) == same(C.byref(co)) == C.addressof(co)
    assert P["ditto_train_forward"][1][9:11] == [("dropout_p", C.c_float), ("seed", C.c_uint64)]
    res, params = P["ditto_model_create"]                                             # spans two lines; struct pointers, a handle out
    assert res is i and [n for n, _ in params] == ["cfg", "w", "arena", "arena_bytes", "stream", "out"]
    assert [t for _, t in params] == [C.POINTER(hip.Config), C.POINTER(hip.Weights), vp, sz, vp, vp]
    res, params = P["ditto_attention_train_resid_bf16"]                               # every device pointer is followed by its byte size
    for n in "q k v resid_in resid_out out lse_out cu_q cu_kv".split():
        at = [p for p, _ in params].index(n)
        assert params[at] == (n, vp) and params[at + 1] == (n + "_bytes", sz)
    assert P["ditto_train_backward"][1][14] == ("grads", C.POINTER(hip.Grads))
    assert P["ditto_slp_create"][1][:2] == [("cfg", C.POINTER(hip.SlpConfig)), ("w", C.POINTER(hip.SlpWeights))]
    assert P["ditto_gemm_epilogue_bf16"][1][0] == ("args", C.POINTER(hip.GemmEpilogueArgs))
    res, params = P["ditto_guided_step_packed_rescale_opts"]                          # the longest: seven lines
    assert len(params) == 32 and params[-2:] == [("stream", vp), ("opts", C.POINTER(hip.CallOpts))]
    assert [n for n, _ in params[:6]] == "m x2 cond t cu_speech cu_text".split()
    assert [n for n, _ in params[-8:-2]] == "rope_cos rope_sin workspace workspace_bytes scratch scratch_bytes".split()


@pytest.mark.parametrize("text, names", [
    ("int ditto_x(ditto_new_t a);", ("ditto_x", "ditto_new_t")),                      # a scalar type the rule does not know
    ("typedef void* ditto_stream_t;\nint ditto_y(ditto_stream_t s, const ditto_thing* p);", ("ditto_y", "ditto_thing")),
    ("int ditto_z(int (*cb)(int), void* p);", ("ditto_z",)),                          # a function pointer
    ("int ditto_u(int);", ("ditto_u",)),                                              # a parameter without a name
    ("long ditto_v(void);", ("ditto_v", "long"))])
def test_a_prototype_the_rule_cannot_type_raises_and_is_named(text, names):
    with pytest.raises(TypeError) as e:
        hip.parse_prototypes(text)
    assert all(n in str(e.value) for n in names), str(e.value)


def test_parser_reads_declaration_forms():
    got = hip.parse_prototypes("""
        #define X 1
        typedef struct ditto_s { int a; /* x; */ float b; } ditto_s;
        enum { A = 0, B };
        /* int ditto_not_this(int a); */
        size_t ditto_f(const ditto_s* s,   // trailing
                       const void* const* pp, float f);
        void ditto_g(void);""")
    assert got == {"ditto_f": (C.c_size_t, [("s", C.c_void_p), ("pp", C.c_void_p), ("f", C.c_float)]), "ditto_g": (None, [])}


def test_call_by_name_orders_by_the_header_and_takes_no_defaults(monkeypatch):
    lib = hip.lib()
    c = hip.make_config(PRESETS["C2"]["cfg"])
    got = {}
    for how in ("positional", "by_name"):
        a, b, h = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        if how == "positional":
            rc = lib.ditto_full_row_plan_opts(C.byref(c), 32, 1024, None, C.byref(a), C.byref(b), C.byref(h))
        else:                                                                         # in another order than the header's
            rc = hip.call("ditto_full_row_plan_opts", stream_bf16=C.byref(h), fc2=C.byref(b), N=1024, outproj=C.byref(a), opts=None,
                          B=32, cfg=C.byref(c))
        got[how] = (rc, a.value, b.value, h.value)
    assert got["by_name"] == got["positional"] == (hip.OK, 1, 1, 1)
    refused = dict(x=None, eps=None, noise=None, t=None, betas=None, alphas=None, alphas_cumprod=None, B=1, elems_per_utt=4, stream=None)
    assert hip.call("ditto_p_sample_update", **refused) == lib.ditto_p_sample_update(*refused.values()) == hip.ERR_ARG
    assert b"ditto_p_sample_update" in lib.ditto_last_error()
    # a wrong set of names never reaches the library: the bound function is replaced by a counter
    calls = []
    monkeypatch.setattr(lib, "ditto_p_sample_update", lambda *a: calls.append(a) or hip.OK)
    assert hip.call("ditto_p_sample_update", **refused) == hip.OK and len(calls) == 1 and calls[0] == tuple(refused.values())
    missing = {k: v for k, v in refused.items() if k != "betas"}
    for kw, said in ((missing, "missing betas"), (dict(refused, gamma=None), "no parameter named gamma"),
                     (dict(missing, beta=None), "missing betas; no parameter named beta")):
        with pytest.raises(TypeError, match="ditto_p_sample_update: " + said):
            hip.call("ditto_p_sample_update", **kw)
    with pytest.raises(TypeError, match="ditto_p_sample_updat: include/ditto_hip.h declares no such entry"):
        hip.call("ditto_p_sample_updat", **refused)
    assert len(calls) == 1


def test_struct_layout_matches_header():
    # 14 model-level pointers + layers pointer; 18 per-layer pointers; 7 int32 config fields
    assert C.sizeof(hip.Config) == 28
    assert C.sizeof(hip.LayerWeights) == 18 * 8
    assert C.sizeof(hip.Weights) == 15 * 8
    assert C.sizeof(hip.CallOpts) == 32


def test_size_queries_and_errors():
    lib = hip.lib()
    c = hip.make_config(PRESETS["C2"]["cfg"])
    arena = lib.ditto_arena_bytes(C.byref(c))
    # bf16 live parameters of 12L/768 = 137.83 M -> ~276 MB, plus fp32 vectors and the time table, plus
    # (d = 768) the stage-major second copies of the cross out-proj and fc2 weights the full-row GEMM reads: 12 x 5.9 MB,
    # and of the cross q-projection for the fused norm2 + q-projection kernel (one image per MFMA shape: 12 x 2 x 1.2 MB)
    assert 340e6 < arena < 385e6
    ws = lib.ditto_workspace_bytes(C.byref(c), 32, 1024, 1024)
    cond = lib.ditto_cond_bytes(C.byref(c), 32, 1024)
    assert cond >= 32 * 1024 * 12 * 2 * 768 * 2
    assert ws >= 32 * 1024 * 768 * (4 + 2 + 6 + 8 + 4 + 4)
    bad = hip.Config(768, 12, 12, 256, 512, 50, 0)          # text_dim != hidden_dim
    assert lib.ditto_arena_bytes(C.byref(bad)) == 0
    assert b"text_dim" in lib.ditto_last_error()
    bad = hip.Config(96, 1, 1, 64, 96, 10, 0)                # not a multiple of 64
    assert lib.ditto_arena_bytes(C.byref(bad)) == 0
    bad = hip.Config(192, 1, 3, 64, 192, 10, hip.CFG_FP8_LINEAR)   # fp8 needs hidden_dim % 128 == 0
    assert lib.ditto_arena_bytes(C.byref(bad)) == 0
    # head_dim % 64 != 0 (the reference takes any hidden_dim % num_heads == 0, src/components/DiT.py:78-86) runs on PADDED heads:
    # the paper's XL shape 1152 / 16 = 72 -> heads at a stride of 128 inside the block, attention-side buffers 2048 wide
    xl = hip.Config(1152, 2, 16, 256, 1152, 50, 0)
    plain = hip.Config(1152, 2, 18, 256, 1152, 50, 0)          # 18 heads of 64: no padding
    assert lib.ditto_arena_bytes(C.byref(xl)) > lib.ditto_arena_bytes(C.byref(plain)) > 0
    assert lib.ditto_cond_bytes(C.byref(xl), 2, 64) >= 2 * 64 * 2 * 2 * 2048 * 2
    assert lib.ditto_workspace_bytes(C.byref(xl), 2, 64, 64) > lib.ditto_workspace_bytes(C.byref(plain), 2, 64, 64)
    bad = hip.Config(90, 1, 2, 64, 90, 10, 0)                # hidden_dim itself must stay a multiple of 64 (the GEMMs' K tile)
    assert lib.ditto_arena_bytes(C.byref(bad)) == 0 and b"hidden_dim" in lib.ditto_last_error()
    bad = hip.Config(192, 1, 64, 64, 192, 10, 0)             # head_dim 3: odd (no half-split rotation)
    assert lib.ditto_arena_bytes(C.byref(bad)) == 0 and b"even" in lib.ditto_last_error()
    bad = hip.Config(384, 1, 4, 64, 384, 10, hip.CFG_FP8_LINEAR)   # fp8 linears: no padded heads (head_dim 96)
    assert lib.ditto_arena_bytes(C.byref(bad)) == 0 and b"fp8" in lib.ditto_last_error()
    for kc, name in enumerate(hip.KERNEL_CLASSES):
        assert lib.ditto_kernel_class_name(kc).decode() == name
    assert lib.ditto_attention_workspace_bytes(1, 1, 64, 64, 64) == 0
    assert lib.ditto_attention_workspace_bytes(1, 1, 64, 64, 768) > 0


def test_null_arguments_are_refused_not_crashed():
    lib = hip.lib()
    assert lib.ditto_model_create(None, None, None, 0, None, None) == hip.ERR_ARG
    assert lib.ditto_forward(None, None, None, None, 1, 1, 1, None, None, None, None, 0, None) == hip.ERR_ARG
    assert lib.ditto_p_sample_update(None, None, None, None, None, None, None, 1, 4, None) == hip.ERR_ARG
    with pytest.raises(hip.DittoHipError):
        hip.check(lib.ditto_gemm_bf16(None, 0, None, None, None, None, 0, 1, 1, 1, 0, None))
    assert lib.ditto_gemm_epilogue_bf16(None, 0, None, None) == hip.ERR_ARG
    assert lib.ditto_gemm_epilogue_fp8(None, None, 0, None, None) == hip.ERR_ARG
    assert lib.ditto_adaln_rows(None, None, None, None, 1, None, 0, None, 0, None, None, None, 1, 1, 64, None) == hip.ERR_ARG
    assert lib.ditto_adaln_rows_packed(None, None, None, None, 1, None, None, 0, None, 0, None, None, None, 1, 64, None) == hip.ERR_ARG
    assert lib.ditto_splitk_finish(None, 1, 64, None, None, None, None, 0, None, None, None, 0, 1, 64, None) == hip.ERR_ARG
    assert lib.ditto_text_mod(None, None, None, None, None, None, 1, 1, 64, 64, None) == hip.ERR_ARG
    assert lib.ditto_text_mod_packed(None, None, 1, 1, None, None, None, None, 1, 64, 64, None) == hip.ERR_ARG
    assert lib.ditto_time_table(None, None, None, None, None, None, None, None, 1, 64, 64, None) == hip.ERR_ARG
    assert lib.ditto_packed_row_map(None, 1, 1, 1, None, None, None) == hip.ERR_ARG


def test_config_rejects_what_the_reference_cannot_run():
    with pytest.raises(ValueError):
        DiTTOConfig(768, 12, 12, 256, 512, 50)
    with pytest.raises(ValueError):
        DiTTOConfig(770, 12, 12, 256, 770, 50)


def test_full_row_plan_is_judged_per_launch_and_pinnable():
    """the full-row kernel addresses its A operand with 32-bit byte offsets, so each of a block's two fused
    launches must be admitted on the stride IT reads with (fc2: lda = 4 d), and the class must be pinnable from the
    unsplit batch so that shards of one batch agree (ditto_full_row_plan: host arithmetic, no GPU call)."""
    cfg = PRESETS["C2"]["cfg"]
    try:
        assert hip.full_row_plan(cfg, 32, 1024) == (True, True)      # the headline shape: 256 row tiles
        assert hip.full_row_plan(cfg, 17, 1024) == (True, True)      # 136 tiles of 128 rows: the 128-row kernel's threshold
        assert hip.full_row_plan(cfg, 15, 1024) == (True, True)      # below it the 64-row kernel, from 176 of its tiles on ...
        assert hip.full_row_plan(cfg, 11, 1024) == (True, True)
        assert hip.full_row_plan(cfg, 10, 1024) == (False, False)
        assert hip.full_row_plan(cfg, 16, 1024) == (False, False)    # ... except where the tiled GEMMs make one exact round:
                                                                     # a shard of the 32 batch on its own...
        with hip.batch_class(32 * 1024):                             # ...and pinned to the class of the unsplit batch
            assert hip.full_row_plan(cfg, 16, 1024) == (True, True)
            assert hip.full_row_plan(cfg, 1, 1024) == (True, True)
            assert hip.full_row_plan(cfg, 1, 64) == (True, True)     # one 64-row tile: the 64-row kernel (same bits)
            with pytest.raises(hip.DittoHipError, match="pinned"):   # fewer rows than that cannot take the pinned class:
                hip.full_row_plan(cfg, 1, 48)                        # an error (as from the forward), never another class
        assert hip.full_row_plan(cfg, 1, 48) == (False, False)       # unpinned: the tiled GEMMs
        assert hip.full_row_plan(cfg, 16, 1024) == (False, False)    # the pin is gone
        # M * lda * 2 >= 2^32 with lda = 4 d = 3072: M >= 699051 rows.  The out-projection (lda = d) still fits.
        assert hip.full_row_plan(cfg, 682, 1024) == (True, True)     # 698368 rows
        assert hip.full_row_plan(cfg, 683, 1024) == (True, False)    # 699392 rows: fc2's A offsets would wrap
        assert hip.full_row_plan(cfg, 2731, 1024) == (False, False)  # M * d * 2 >= 2^32 as well
        hip.set_option("fr_mask", 1)
        assert hip.full_row_plan(cfg, 32, 1024) == (True, False)
        hip.set_option("fr_mask", 2)
        assert hip.full_row_plan(cfg, 32, 1024) == (False, True)
        hip.set_option("fr_mask", 0)
        assert hip.full_row_plan(cfg, 32, 1024) == (False, False)
    finally:
        hip.set_option("fr_mask", 3)
        hip.set_option("fr_class_rows", 0)
    # d = 1024 (BASELINE config C5) runs the 64-row kernel (csrc/gemm_fr64.hip), judged on 64-row tiles (>= 192 of them).  Its
    # cross out-projection is bf16 in the fp8 configuration too (LayerNorm output written as fp8); fc2 only in the bf16 one.
    c5 = PRESETS["C5"]["cfg"]
    assert hip.full_row_plan(c5, 16, 1024) == (True, False)
    assert hip.full_row_plan(c5, 8, 1024) == (False, False)
    c5b = PRESETS["C5_bf16"]["cfg"]
    # round 5: at 16 x 1024 rows the tiled fc2 makes ONE whole round of 256 x 256 tiles (kernels.h gemm256_whole_rounds) and, with
    # a LayerNorm launch, beats the 64-row full-row fc2 (which re-streams all of W per 64 rows); other row counts keep the fusion
    assert hip.full_row_plan(c5b, 16, 1024) == (True, False)
    assert hip.full_row_plan(c5b, 14, 1024) == (True, True)
    with hip.batch_class(14 * 1024):
        assert hip.full_row_plan(c5b, 16, 1024) == (True, True)        # (decided on the CLASS rows)
    assert hip.full_row_plan(c5b, 11, 1024) == (False, False)
    with pytest.raises(hip.DittoHipError):
        hip.set_option("fr_class_rows", -1)


def test_attention_kernel_thresholds_are_validated_options():
    """Round 6: the grids from which the 64-queries-per-wave attention kernels run (attn64p / attn64q) are two process defaults,
    one for the residual form (self-attention) and one for the plain form (cross-attention); both are read back, both refuse
    values below 1.  Host arithmetic only: no GPU call."""
    a, b = hip.get_option("attn64p_min_wgs"), hip.get_option("attn64p_min_wgs_plain")
    assert (a, b) == (768, 192) or "DITTO_ATTN64P_MIN_WGS" in "".join(__import__("os").environ)
    try:
        hip.set_option("attn64p_min_wgs", 512)
        hip.set_option("attn64p_min_wgs_plain", 96)
        assert hip.get_option("attn64p_min_wgs") == 512 and hip.get_option("attn64p_min_wgs_plain") == 96
        for name in ("attn64p_min_wgs", "attn64p_min_wgs_plain"):
            with pytest.raises(hip.DittoHipError):
                hip.set_option(name, 0)
    finally:
        hip.set_option("attn64p_min_wgs", a)
        hip.set_option("attn64p_min_wgs_plain", b)


def test_composed_attention_budget_is_a_validated_option():
    """"attn_generic_kib": the scratch budget of the GEMM-composed attention (default 2 GiB).  Every size query of that path follows
    it — whole pairs that fit, at least one, at most B H — and values below 1 are refused.  Host arithmetic only: no GPU call."""
    l = hip.lib()
    B, H, Sq, Skv, dh = 3, 2, 40, 70, 128
    one = 40 * 128 * 4 + 40 * 128 * 2 + 128 * 128 * 2       # fp32 scores, bf16 probabilities, V^T at Skv rounded up to 64
    queries = (l.ditto_attention_causal_workspace_bytes, l.ditto_attention_workspace_bytes)
    assert hip.get_option("attn_generic_kib") == 2097152
    assert all(f(B, H, Sq, Skv, dh) == B * H * one for f in queries)
    try:
        for room in (5, 3, 1):
            hip.set_option("attn_generic_kib", (room * one + 1023) // 1024)
            assert all(f(B, H, Sq, Skv, dh) == room * one for f in queries)
        hip.set_option("attn_generic_kib", 1)                # less than one pair: the floor of one pair stays
        assert all(f(B, H, Sq, Skv, dh) == one for f in queries)
        for bad in (0, -1):
            with pytest.raises(hip.DittoHipError):
                hip.set_option("attn_generic_kib", bad)
        assert hip.get_option("attn_generic_kib") == 1
    finally:
        hip.set_option("attn_generic_kib", 2097152)
    assert l.ditto_attention_workspace_bytes(B, H, Sq, Skv, 64) == 0     # the fused head_dim-64 kernels need none, whatever the budget


def test_call_options_are_per_call_and_per_thread():
    """ABI 9: the switches that decide which bits an utterance gets — kernel class pin, residual-stream
    type, fused launches — are a ditto_call_opts ARGUMENT or a scope of the CALLING THREAD (ditto_call_opts_push / _pop), not
    process state: a second thread never sees the first one's pin, nesting restores, fields at -1 inherit, bad values and an
    unbalanced pop are errors.  Host arithmetic only (ditto_full_row_plan_opts / ditto_call_opts_current): no GPU call."""
    import threading
    cfg = PRESETS["C2"]["cfg"]
    base = hip.current_opts()
    assert (base.class_rows, base.residual_bf16, base.fr_mask, base.lnq) == (0, 1, 3, 32)
    # per-call argument: the same question, two answers, no state in between
    assert hip.full_row_plan(cfg, 16, 1024) == (False, False)
    assert hip.full_row_plan(cfg, 16, 1024, hip.CallOpts(class_rows=32 * 1024)) == (True, True)
    assert hip.full_row_plan(cfg, 32, 1024, hip.CallOpts(fr_mask=1)) == (True, False)
    assert hip.full_row_plan(cfg, 16, 1024) == (False, False)
    assert hip.stream_is_bf16(cfg, 32, 1024) and not hip.stream_is_bf16(cfg, 32, 1024, hip.CallOpts(residual_bf16=0))
    assert not hip.stream_is_bf16(cfg, 16, 1024) and hip.stream_is_bf16(cfg, 16, 1024, hip.CallOpts(class_rows=32 * 1024))
    assert not hip.stream_is_bf16(cfg, 12, 1024)      # the 64-row full-row kernel's batches keep the fp32 stream
    # thread scope: nests, inherits, restores; another thread is untouched while this one is inside its scope
    seen = {}
    inside, done = threading.Event(), threading.Event()

    def other():
        inside.wait(10)
        seen["other"] = (hip.current_opts().class_rows, hip.full_row_plan(cfg, 16, 1024))
        with hip.batch_class(777):
            seen["other_in"] = hip.current_opts().class_rows
        done.set()

    th = threading.Thread(target=other)
    th.start()
    with hip.call_opts(class_rows=32 * 1024, residual_bf16=0):
        inside.set()
        assert done.wait(10)
        o = hip.current_opts()
        assert (o.class_rows, o.residual_bf16, o.fr_mask) == (32 * 1024, 0, 3)
        with hip.call_opts(fr_mask=2):                    # class_rows and residual_bf16 inherit the enclosing scope
            o = hip.current_opts()
            assert (o.class_rows, o.residual_bf16, o.fr_mask) == (32 * 1024, 0, 2)
            assert hip.full_row_plan(cfg, 16, 1024) == (False, True)
        assert hip.current_opts().fr_mask == 3
        assert hip.get_option("fr_class_rows") == 0 and hip.get_option("residual_bf16") == 1   # the process defaults never moved
    th.join()
    assert seen == {"other": (0, (False, False)), "other_in": 777}
    assert hip.current_opts().class_rows == 0
    # validation
    import ctypes as C
    lib = hip.lib()
    bad = hip.CallOpts(); bad.lnq = 7
    assert lib.ditto_call_opts_push(C.byref(bad)) == hip.ERR_ARG
    bad = hip.CallOpts(); bad.reserved[2] = 1
    assert lib.ditto_call_opts_push(C.byref(bad)) == hip.ERR_ARG
    bad = hip.CallOpts(); bad.class_rows = -5
    a, b = C.c_int(), C.c_int()
    c = hip.make_config(cfg)
    assert lib.ditto_full_row_plan_opts(C.byref(c), 1, 64, C.byref(bad), C.byref(a), C.byref(b), None) == hip.ERR_ARG
    assert lib.ditto_call_opts_pop() == hip.ERR_ARG and b"without a matching push" in lib.ditto_last_error()
    for _ in range(16):
        assert lib.ditto_call_opts_push(None) == hip.OK
    assert lib.ditto_call_opts_push(None) == hip.ERR_ARG          # depth limit
    for _ in range(16):
        assert lib.ditto_call_opts_pop() == hip.OK
