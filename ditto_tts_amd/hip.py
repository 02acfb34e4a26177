"""ctypes binding of libditto_hip.so (include/ditto_hip.h).

There is NO fallback: if the library is missing or a call fails this module raises.
Build it with `python -m ditto_tts_amd.build` (hipcc, gfx950).
"""
from __future__ import annotations

import ctypes as C
import os
import re

from .build import INCLUDE

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DITTO_HIP_LIB") or os.path.join(HERE, "libditto_hip.so")   # override: diagnostic builds (tools/)

OK, ERR_ARG, ERR_SHAPE, ERR_HIP, ERR_SIZE = range(5)
CFG_FP8_LINEAR = 1

KERNEL_CLASSES = ["layernorm", "gemm_qkv_rope", "gemm_q_proj", "gemm_out_proj", "gemm_gated_mlp", "gemm_fc2",
                  "gemm_final", "attn_self", "attn_cross", "adaln", "p_sample_update"]
KC_COUNT = len(KERNEL_CLASSES)


class DittoHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libditto_hip error {code}: {msg}")
        self.code = code


class Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("hidden_dim", "num_layers", "num_heads", "time_dim", "text_dim", "diffusion_steps", "flags")]


_LAYER_FIELDS = ["norm1_weight", "norm1_bias", "attn_in_proj_weight", "attn_in_proj_bias",
                 "norm2_weight", "norm2_bias", "cross_in_proj_weight", "cross_in_proj_bias",
                 "cross_out_proj_weight", "cross_out_proj_bias", "norm3_weight", "norm3_bias",
                 "mlp_fc1_weight", "mlp_fc1_bias", "gate_weight", "gate_bias", "mlp_fc2_weight", "mlp_fc2_bias"]
_GLOBAL_FIELDS = ["t_embedding_weight", "time_embed_0_weight", "time_embed_0_bias", "time_embed_2_weight",
                  "time_embed_2_bias", "ada_time_mlp_weight", "ada_time_mlp_bias", "ada_text_mlp_weight",
                  "ada_text_mlp_bias", "proj_in_weight", "proj_in_bias", "proj_out_weight", "proj_out_bias",
                  "rotary_inv_freq"]

# struct field -> reference state_dict key (layer keys are relative to "blocks.{i}.")
LAYER_KEY = {
    "norm1_weight": "norm1.weight", "norm1_bias": "norm1.bias",
    "attn_in_proj_weight": "attn.in_proj_weight", "attn_in_proj_bias": "attn.in_proj_bias",
    "norm2_weight": "norm2.weight", "norm2_bias": "norm2.bias",
    "cross_in_proj_weight": "cross_attn.in_proj_weight", "cross_in_proj_bias": "cross_attn.in_proj_bias",
    "cross_out_proj_weight": "cross_attn.out_proj.weight", "cross_out_proj_bias": "cross_attn.out_proj.bias",
    "norm3_weight": "norm3.weight", "norm3_bias": "norm3.bias",
    "mlp_fc1_weight": "mlp_fc1.weight", "mlp_fc1_bias": "mlp_fc1.bias",
    "gate_weight": "gate.weight", "gate_bias": "gate.bias",
    "mlp_fc2_weight": "mlp_fc2.weight", "mlp_fc2_bias": "mlp_fc2.bias",
}
GLOBAL_KEY = {
    "t_embedding_weight": "t_embedding.weight",
    "time_embed_0_weight": "time_embed.0.weight", "time_embed_0_bias": "time_embed.0.bias",
    "time_embed_2_weight": "time_embed.2.weight", "time_embed_2_bias": "time_embed.2.bias",
    "ada_time_mlp_weight": "ada_ln.time_mlp.1.weight", "ada_time_mlp_bias": "ada_ln.time_mlp.1.bias",
    "ada_text_mlp_weight": "ada_ln.text_mlp.1.weight", "ada_text_mlp_bias": "ada_ln.text_mlp.1.bias",
    "proj_in_weight": "proj_in.weight", "proj_in_bias": "proj_in.bias",
    "proj_out_weight": "proj_out.weight", "proj_out_bias": "proj_out.bias",
    "rotary_inv_freq": "rotary.inv_freq",
}


class LayerWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _LAYER_FIELDS]


class Weights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _GLOBAL_FIELDS] + [("layers", C.POINTER(LayerWeights))]


# the speech-length predictor's decoder stack: struct field -> state_dict key relative to "transformer.layers.{i}."
SLP_LAYER_KEY = {
    "self_in_proj_weight": "self_attn.in_proj_weight", "self_in_proj_bias": "self_attn.in_proj_bias",
    "self_out_proj_weight": "self_attn.out_proj.weight", "self_out_proj_bias": "self_attn.out_proj.bias",
    "cross_in_proj_weight": "multihead_attn.in_proj_weight", "cross_in_proj_bias": "multihead_attn.in_proj_bias",
    "cross_out_proj_weight": "multihead_attn.out_proj.weight", "cross_out_proj_bias": "multihead_attn.out_proj.bias",
    "linear1_weight": "linear1.weight", "linear1_bias": "linear1.bias",
    "linear2_weight": "linear2.weight", "linear2_bias": "linear2.bias",
    "norm1_weight": "norm1.weight", "norm1_bias": "norm1.bias", "norm2_weight": "norm2.weight",
    "norm2_bias": "norm2.bias", "norm3_weight": "norm3.weight", "norm3_bias": "norm3.bias",
}


class SlpConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("d_model", "nhead", "num_layers", "dim_feedforward", "num_classes")]


class SlpLayerWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in SLP_LAYER_KEY]


class SlpWeights(C.Structure):
    _fields_ = [("layers", C.POINTER(SlpLayerWeights)), ("length_predictor_weight", C.c_void_p),
                ("length_predictor_bias", C.c_void_p)]


class CallOpts(C.Structure):
    """ditto_call_opts (ABI 9): the per-call switches that decide which bits an utterance gets.  -1 = inherit."""
    _fields_ = [("class_rows", C.c_int32), ("residual_bf16", C.c_int32), ("fr_mask", C.c_int32), ("lnq", C.c_int32),
                ("reserved", C.c_int32 * 4)]

    def __init__(self, class_rows=None, residual_bf16=None, fr_mask=None, lnq=None):
        super().__init__(-1 if class_rows is None else min(int(class_rows), 0x7FFFFFFF),
                         -1 if residual_bf16 is None else int(residual_bf16),
                         -1 if fr_mask is None else int(fr_mask), -1 if lnq is None else int(lnq))

    def __repr__(self):
        return f"CallOpts(class_rows={self.class_rows}, residual_bf16={self.residual_bf16}, fr_mask={self.fr_mask}, lnq={self.lnq})"


class GemmEpilogueArgs(C.Structure):
    """ditto_gemm_epilogue_args: the fields of one bf16 GEMM launch (ditto_gemm_epilogue_bf16, unit tests)."""
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int), ("W", C.c_void_p), ("ldw", C.c_int), ("w_rows", C.c_int),
                ("bias", C.c_void_p), ("residual", C.c_void_p), ("ldr", C.c_int), ("out", C.c_void_p), ("ldo", C.c_int),
                ("out2_bf16", C.c_void_p), ("ldo2", C.c_int), ("rope_cos", C.c_void_p), ("rope_sin", C.c_void_p),
                ("rope_rows_per_batch", C.c_int), ("rope_cols", C.c_int), ("rope_freq_rev", C.c_void_p),
                ("rope_pos", C.c_void_p), ("pre_bf16", C.c_void_p), ("ldpre", C.c_int), ("colsum_partial", C.c_void_p),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int)]


REUSE_STORE, REUSE_LOAD = 1, 2   # the `mode` of the ditto_*_reuse entries: a refresh step keeps delta = c - u, a reuse step reads it


class MultistepCoef(C.Structure):
    """ditto_multistep_coef: one utterance's step of the second-order multistep solver (sampler.multistep_schedule), 32 bytes."""
    _fields_ = [("a", C.c_float), ("kx", C.c_float), ("ke", C.c_float), ("b", C.c_float), ("g", C.c_float), ("w", C.c_float),
                ("use_prev", C.c_int32), ("reserved", C.c_int32)]
    _as_parameter_ = property(C.byref)   # given bare as a host `step` (a c_void_p parameter), it goes by reference


RESCALE_CHUNK_QUADS = 4096    # DITTO_RESCALE_CHUNK_QUADS: 16-byte quads per partial of the guidance-rescale statistics (part of its bits)


def rescale_scratch_layout(B: int):
    """(byte offset of scale fp32 [B], byte offset of the partials) in the scratch of ditto_guidance_rescale_bytes; coef_out — fp32 [B]
    or ditto_multistep_coef [B] — stands at byte 0."""
    al = lambda n: (n + 255) // 256 * 256
    return al(32 * B), al(32 * B) + al(4 * B)


REGROUP_BUFS = 6
REGROUP_SEG_WORDS = 8      # ditto_regroup_seg as int32 / uint32 words: kind, source, dest, aux, src_off, dst_off, n, dup_off (16-byte units)
REGROUP_COPY, REGROUP_DRAW = 0, 1

# ditto_layer_grads / ditto_grads have the layout of the weight structs (one pointer per state_dict key)
LayerGrads, Grads = LayerWeights, Weights

# ---- the C ABI.  include/ditto_hip.h is its single description: csrc/ is compiled against it, and the prototypes below are parsed
# from it once, here.  One type rule, no per-function exceptions: a scalar by its spelling (_SCALARS); `const char*` = c_char_p; a
# pointer to a struct of _STRUCTS = POINTER(that class); every other pointer = c_void_p (it takes a device address as an int, None,
# C.byref(...), a ctypes array or pointer); `void` returns None.  ditto_multistep_coef is deliberately not in _STRUCTS: the header
# uses it both for a host struct (`step`) and for device arrays (`coefs`); a bare MultistepCoef goes by reference (_as_parameter_).
_SCALARS = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "ditto_stream_t": C.c_void_p, "ditto_model_t": C.c_void_p, "ditto_slp_t": C.c_void_p}
_STRUCTS = {"ditto_config": Config, "ditto_weights": Weights, "ditto_grads": Grads, "ditto_call_opts": CallOpts,
            "ditto_gemm_epilogue_args": GemmEpilogueArgs, "ditto_slp_config": SlpConfig, "ditto_slp_weights": SlpWeights}
_POINTEES = {"void", "char", "int", "float", "size_t", "int32_t", "int64_t", "uint32_t", "uint64_t"}   # beside the header's own types


def _ctype(decl: str, known, what: str):
    """the ctypes type of the type `decl` (`known`: the type names the header itself declares); TypeError naming `what`"""
    words = decl.replace("*", " * ").split()
    base, stars = [w for w in words if w not in ("const", "*")], words.count("*")
    if len(base) == 1:
        base = base[0]
        if stars == 0 and base in _SCALARS:
            return _SCALARS[base]
        if stars == 1 and base == "char":
            return C.c_char_p
        if stars == 1 and base in _STRUCTS:
            return C.POINTER(_STRUCTS[base])
        if stars >= 1 and base != "char" and (base in _POINTEES or base in _SCALARS or base in known):
            return C.c_void_p
    raise TypeError(f"include/ditto_hip.h: no ctypes type for `{decl.strip()}` in `{what}`")


def parse_prototypes(text: str, known=()) -> dict:
    """name -> (restype, [(parameter name, ctype), ...]) of every function the C header `text` declares (`known`: type names of a
    header it includes, beside its own).  Every statement beside
    comments, preprocessor lines and `struct / enum {...}` bodies is a typedef or a prototype; one that is neither, or has a type the
    rule above does not cover, raises TypeError naming it: nothing falls back to c_void_p."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    known = set(known) | set(re.findall(r"typedef\s+(?:struct|enum)\s+\w*\s*\{[^{}]*\}\s*(\w+)\s*;", text))
    text = re.sub(r"(?:typedef\s+)?(?:struct|enum)\s*\w*\s*\{[^{}]*\}\s*\w*\s*;", "", text)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    protos = {}
    for stmt in (" ".join(s.split()) for s in text.split(";")):
        if not stmt:
            continue
        td = re.fullmatch(r"typedef [\w\s*]+?(\w+)", stmt)
        if td:
            known.add(td.group(1))
            continue
        fn = re.fullmatch(r"([\w\s*]+?)(\w+) ?\(([^()]*)\)", stmt)
        if not fn:
            raise TypeError(f"include/ditto_hip.h: neither a typedef nor a prototype: `{stmt}`")
        ret, name, params = fn.groups()
        params = [] if params.strip() in ("", "void") else [re.fullmatch(r"(.*?)(\w+)", q.strip()) for q in params.split(",")]
        if None in params or name in protos:
            raise TypeError(f"include/ditto_hip.h: cannot read the parameters of `{stmt}`")
        protos[name] = (None if ret.split() == ["void"] else _ctype(ret, known, stmt),
                        [(q.group(2), _ctype(q.group(1), known, stmt)) for q in params])
    return protos


with open(os.path.join(INCLUDE, "ditto_hip.h")) as _f:
    PROTOTYPES = parse_prototypes(_f.read())
# name -> (restype, argtypes): what lib() binds and the tools and tests read
SYMBOLS = {name: (res, [t for _, t in params]) for name, (res, params) in PROTOTYPES.items()}
_ORDER = {name: tuple(p for p, _ in params) for name, (_, params) in PROTOTYPES.items()}


# The fused optimizer's entries (include/ditto_optim.h, csrc/optim.hip) are exported by the same library but are a table of their
# own: PROTOTYPES / SYMBOLS stay exactly the functions of ditto_hip.h.  lib() binds them and call() reaches them by parameter name.
with open(os.path.join(INCLUDE, "ditto_optim.h")) as _f:
    OPTIM_PROTOTYPES = parse_prototypes(_f.read())
OPTIM_SYMBOLS = {name: (res, [t for _, t in params]) for name, (res, params) in OPTIM_PROTOTYPES.items()}
_ORDER.update({name: tuple(p for p, _ in params) for name, (_, params) in OPTIM_PROTOTYPES.items()})
OPTIM_CHUNK_QUADS = 4096      # DITTO_OPTIM_CHUNK_QUADS: 16-byte quads per chunk of a segment (part of the norm's bits)


# The backward pass's row kernels, one launch each with every buffer's byte size (include/ditto_train_rows.h,
# csrc/train_rows_api.hip): a third table, built and bound the same way; the tests reach its entries through call() only.
with open(os.path.join(INCLUDE, "ditto_train_rows.h")) as _f:
    TRAIN_ROWS_PROTOTYPES = parse_prototypes(_f.read())
TRAIN_ROWS_SYMBOLS = {name: (res, [t for _, t in params]) for name, (res, params) in TRAIN_ROWS_PROTOTYPES.items()}
_ORDER.update({name: tuple(p for p, _ in params) for name, (_, params) in TRAIN_ROWS_PROTOTYPES.items()})
SMALL_LINEAR_FWD, SMALL_LINEAR_BWD_W, SMALL_LINEAR_BWD_X = range(3)   # the `mode` of ditto_bwd_small_linear

# The text side of training for classifier-free guidance — the packed backward with the text gradient, condition dropout's select
# forward and backward (include/ditto_text_grad.h, csrc/text_grad.hip, csrc/ditto_train.hip): a fourth table, built and bound the same way.
with open(os.path.join(INCLUDE, "ditto_text_grad.h")) as _f:
    TEXT_GRAD_PROTOTYPES = parse_prototypes(_f.read())
TEXT_GRAD_SYMBOLS = {name: (res, [t for _, t in params]) for name, (res, params) in TEXT_GRAD_PROTOTYPES.items()}
_ORDER.update({name: tuple(p for p, _ in params) for name, (_, params) in TEXT_GRAD_PROTOTYPES.items()})

# Guidance reuse in a request stream — the three-kind update and its step (include/ditto_refresh.h, csrc/guided_refresh.hip,
# csrc/ditto_api.hip): a fifth table, built and bound the same way.
with open(os.path.join(INCLUDE, "ditto_refresh.h")) as _f:
    REFRESH_PROTOTYPES = parse_prototypes(_f.read())
REFRESH_SYMBOLS = {name: (res, [t for _, t in params]) for name, (res, params) in REFRESH_PROTOTYPES.items()}
_ORDER.update({name: tuple(p for p, _ in params) for name, (_, params) in REFRESH_PROTOTYPES.items()})
KIND_PLAIN, KIND_REFRESH, KIND_REUSE = 0, 1, 2   # the `kind` of the ditto_*_refresh entries, per utterance

# Projected guidance (APG) for packed guided sampling — the direction and its statistics, the two updates and their steps
# (include/ditto_project.h, csrc/guided_project.hip, csrc/ditto_api.hip): a sixth table, built and bound the same way.
with open(os.path.join(INCLUDE, "ditto_project.h")) as _f:
    PROJECT_PROTOTYPES = parse_prototypes(_f.read(), known=("ditto_multistep_coef",))
PROJECT_SYMBOLS = {name: (res, [t for _, t in params]) for name, (res, params) in PROJECT_PROTOTYPES.items()}
_ORDER.update({name: tuple(p for p, _ in params) for name, (_, params) in PROJECT_PROTOTYPES.items()})


# Projected guidance in a request stream — the direction, the three-kind update and the step over the mixed layout
# (include/ditto_project_stream.h, csrc/guided_project_mixed.hip, csrc/ditto_api.hip): a seventh table, built and bound the same way.
with open(os.path.join(INCLUDE, "ditto_project_stream.h")) as _f:
    PROJECT_STREAM_PROTOTYPES = parse_prototypes(_f.read(), known=("ditto_project_coef",))
PROJECT_STREAM_SYMBOLS = {name: (res, [t for _, t in params]) for name, (res, params) in PROJECT_STREAM_PROTOTYPES.items()}
_ORDER.update({name: tuple(p for p, _ in params) for name, (_, params) in PROJECT_STREAM_PROTOTYPES.items()})
# the `kind` of the ditto_*_project_mixed entries, per utterance: plain, guided without projection, projected (2 stays KIND_REUSE's)
KIND_CFG, KIND_PROJECT = 1, 3


class ProjectCoef(C.Structure):
    """ditto_project_coef: one utterance's parameters of a projected-guidance step (a device array [B]), 32 bytes."""
    _fields_ = [("kx", C.c_float), ("ke", C.c_float), ("w", C.c_float), ("eta", C.c_float), ("r", C.c_float), ("beta", C.c_float),
                ("use_prev", C.c_int32), ("reserved", C.c_int32)]


def project_scratch_layout(B: int):
    """byte offset of the partials in the scratch of ditto_guidance_project_bytes; pcoef fp32 [B, 4] stands at byte 0"""
    return (16 * B + 255) // 256 * 256


class OptimSeg(C.Structure):
    """ditto_optim_seg: one parameter tensor of the optimizer's device table, 72 bytes."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("ema", C.c_void_p),
                ("n", C.c_uint64), ("slot0", C.c_uint32), ("reserved", C.c_uint32), ("lr", C.c_double), ("weight_decay", C.c_double)]


class OptimHyper(C.Structure):
    """ditto_optim_hyper: the hyper-parameters all segments share (a host struct)."""
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("max_norm", C.c_double),
                ("ema_decay", C.c_double), ("skip_nonfinite", C.c_int32), ("reserved", C.c_int32)]
    _as_parameter_ = property(C.byref)


OPTIM_STATE_BYTES = 128       # ditto_optim_state: two 32-byte slots (beta1^t, beta2^t fp64; step, skipped int64), then the report:
OPTIM_STATE_NORM64, OPTIM_STATE_NORM32, OPTIM_STATE_CLIP, OPTIM_STATE_SKIP = 64, 72, 76, 80   # byte offsets of norm, norm32, clip, skip


def optim_chunks(n: int) -> int:
    """chunks of a segment of n elements"""
    return (((int(n) + 3) // 4) + OPTIM_CHUNK_QUADS - 1) // OPTIM_CHUNK_QUADS


_lib = None


def lib() -> C.CDLL:
    """Load libditto_hip.so (once).  Raises if it has not been built — there is no other path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP extension is the only compute path of ditto_tts_amd. "
                "Build it with `python -m ditto_tts_amd.build` (needs hipcc).")
        # torch first: libditto_hip.so and torch must share ONE HIP runtime (both want SONAME libamdhip64.so.7; the
        # first one loaded wins).  Loading ours first binds the process to /opt/rocm's runtime, under which torch's
        # device initialisation and ours disagreed on a GPU box ("no ROCm-capable device is detected" at the first launch).
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        frozen = bool(os.environ.get("DITTO_HIP_LIB"))   # a diagnostic or FROZEN earlier build for same-box A/Bs (tools/):
        for name, (res, args) in (*SYMBOLS.items(), *OPTIM_SYMBOLS.items(), *TRAIN_ROWS_SYMBOLS.items(),
                                  *TEXT_GRAD_SYMBOLS.items(), *REFRESH_SYMBOLS.items(), *PROJECT_SYMBOLS.items(),
                                  *PROJECT_STREAM_SYMBOLS.items()):   # it may predate entries added since (then absent)
            try:
                fn = getattr(l, name)  # AttributeError if the .so does not export a declared symbol
            except AttributeError:
                if frozen:
                    continue
                raise
            fn.restype, fn.argtypes = res, args
        if l.ditto_abi_version() != 10 and not (frozen and l.ditto_abi_version() in (7, 8, 9)):
            raise RuntimeError("libditto_hip.so ABI version mismatch")
        _lib = l
    return _lib


def check(rc: int):
    if rc != OK:
        raise DittoHipError(rc, lib().ditto_last_error().decode(errors="replace"))


def call(name: str, **kw) -> int:
    """The entry `name` with its arguments BY THE HEADER'S PARAMETER NAMES, in any order; returns its status.  No defaults: every
    parameter of the prototype is given (None = NULL).  A missing or an unknown name is a TypeError naming the entry and the
    parameter, raised before the library is entered."""
    order = _ORDER.get(name)
    if order is None:
        header = "ditto_optim.h" if name.startswith("ditto_optim_") else "ditto_train_rows.h" if name.startswith("ditto_bwd_") else \
            "ditto_text_grad.h" if name.startswith("ditto_text_select_") else \
            "ditto_refresh.h" if "_packed_refresh" in name else "ditto_project_stream.h" if "_project_mixed" in name else \
            "ditto_project.h" if "_project" in name else "ditto_hip.h"
        raise TypeError(f"{name}: include/{header} declares no such entry")
    if len(kw) != len(order) or not all(p in kw for p in order):
        missing, unknown = [p for p in order if p not in kw], [p for p in kw if p not in order]
        raise TypeError(f"{name}: " + "; ".join(f"{what} {', '.join(ps)}" for what, ps in
                                                 (("missing", missing), ("no parameter named", unknown)) if ps))
    return getattr(lib(), name)(*[kw[p] for p in order])


def set_option(name: str, value: int):
    """ditto_set_option: process-wide tuning switches of libditto_hip.so (include/ditto_hip.h)."""
    check(lib().ditto_set_option(name.encode(), int(value)))


def get_option(name: str) -> int:
    """ditto_get_option: the current value of a switch."""
    v = C.c_int(0)
    check(lib().ditto_get_option(name.encode(), C.byref(v)))
    return int(v.value)


def has_varlen() -> bool:
    """Does the loaded library have the variable-length entry points (detected by symbol, as the call options are)?"""
    return hasattr(lib(), "ditto_attention_varlen_bf16")


def _has_call_opts() -> bool:
    return hasattr(lib(), "ditto_call_opts_push") and lib().ditto_abi_version() >= 9


class call_opts:
    """Context manager: the per-call options (class_rows, residual_bf16, fr_mask, lnq) in force for every library call THIS
    THREAD makes inside the block (ditto_call_opts_push / _pop).  Nothing process-wide changes: other threads and streams keep
    their own options.  Nests; a field left None inherits the enclosing block, else the process default (set_option)."""

    def __init__(self, class_rows=None, residual_bf16=None, fr_mask=None, lnq=None):
        self.opts = CallOpts(class_rows, residual_bf16, fr_mask, lnq)
        self._legacy = None

    def __enter__(self):
        if _has_call_opts():
            check(lib().ditto_call_opts_push(C.byref(self.opts)))
        else:   # a frozen pre-ABI-9 library (DITTO_HIP_LIB, tools/ A/Bs): the old process-wide switches
            names = {"fr_class_rows": self.opts.class_rows, "residual_bf16": self.opts.residual_bf16,
                     "fr_mask": self.opts.fr_mask, "lnq": self.opts.lnq}
            self._legacy = {k: get_option(k) for k, v in names.items() if v >= 0}
            for k, v in names.items():
                if v >= 0:
                    set_option(k, v)
        return self

    def __exit__(self, *exc):
        if self._legacy is None:
            check(lib().ditto_call_opts_pop())
        else:
            for k, v in self._legacy.items():
                set_option(k, v)
            self._legacy = None
        return False


class batch_class(call_opts):
    """Context manager: every forward THIS THREAD makes inside decides its kernel class (low-latency / tiled GEMM + LayerNorm /
    full-row GEMM with the LayerNorms fused: different summation orders, so different last bits) as a batch of `rows` = B x N
    rows would.  A caller that splits one batch over several launches or GPUs wraps the pieces in `batch_class(rows of the
    unsplit batch)` — or passes CallOpts(class_rows=...) to the engine call itself: an utterance's bits are then the same however
    the batch was split (dist.sample_sharded and SpeechGenerator's seeds= path do).  Since ABI 9 this is a property of the
    CALLS, not of the process (ditto_call_opts): no other thread's forwards are affected.  Nests.  A launch that cannot take the
    pinned class (a full-row class with fewer than 64 rows in the launch) raises DittoHipError instead of silently running
    another class."""

    def __init__(self, rows: int):
        super().__init__(class_rows=int(rows))
        self.rows = int(rows)


def current_opts() -> CallOpts:
    """The options a call made by this thread NOW (without its own CallOpts) would run under, every field resolved."""
    o = CallOpts()
    if _has_call_opts():
        check(lib().ditto_call_opts_current(C.byref(o)))
    else:
        o.class_rows, o.residual_bf16 = get_option("fr_class_rows"), get_option("residual_bf16")
        o.fr_mask, o.lnq = get_option("fr_mask"), get_option("lnq")
    return o


def full_row_plan(cfg, B: int, N: int, opts: "CallOpts | None" = None):
    """(outproj, fc2): which of a block's two fused GEMM + LayerNorm launches a forward over B x N rows takes
    (ditto_full_row_plan; host arithmetic, no GPU call) under this thread's options, or under `opts`."""
    a, b = C.c_int(0), C.c_int(0)
    c = make_config(cfg)
    if opts is not None:
        check(lib().ditto_full_row_plan_opts(C.byref(c), B, N, C.byref(opts), C.byref(a), C.byref(b), None))
    else:
        check(lib().ditto_full_row_plan(C.byref(c), B, N, C.byref(a), C.byref(b)))
    return bool(a.value), bool(b.value)


def stream_is_bf16(cfg, B: int, N: int, opts: "CallOpts | None" = None) -> bool:
    """Does a forward of B x N rows carry its residual stream as bf16 (ditto_forward's rule, answered by the library)?"""
    a, b, h = C.c_int(0), C.c_int(0), C.c_int(0)
    c = make_config(cfg)
    check(lib().ditto_full_row_plan_opts(C.byref(c), B, N, C.byref(opts) if opts is not None else None, C.byref(a), C.byref(b),
                                         C.byref(h)))
    return bool(h.value)


def set_low_latency(on: bool = True):
    """The explicit split-K rule of rounds 1-3 (a workgroup target of 256) for the long-K GEMMs of 1-2 utterance batches.
    Since round 4 the DEFAULT already splits them (the low-latency class: a rule that depends on K only, so that inside the
    class an utterance's bits do not depend on its batch neighbours); this switch trades that invariance for one more split at
    B = 1.  set_option("splitk_wgs", -1) turns every split off."""
    set_option("splitk_wgs", 256 if on else 0)


def make_config(cfg) -> Config:
    return Config(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps,
                  CFG_FP8_LINEAR if getattr(cfg, "fp8_linear", False) else 0)
