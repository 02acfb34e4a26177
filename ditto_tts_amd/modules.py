"""nn.Module façade with the reference's class names, constructor signatures, attribute names and
state_dict keys whose forward() runs on libditto_hip.so.

    reference class                         this file
    components.DiT.GlobalAdaLN   (:8-40)    GlobalAdaLN
    components.DiT.RotaryEmbedding (:43-72) RotaryEmbedding
    components.DiT.DiT           (:75-157)  DiT
    model.DiTTO.DiTTO            (:7-126)   DiTTO

torch.nn modules are used only as PARAMETER CONTAINERS (so `state_dict()`, `.to()`, optimisers and the
reference's checkpoints work unchanged); none of their forward()s is ever called.  There is no CPU or
eager-PyTorch fallback: a non-CUDA input or a missing libditto_hip.so raises.

Training: `DiTTO.forward` under autograd runs ditto_train_forward / ditto_train_backward
through a torch.autograd.Function, so the reference's training closure (src/TrainDiTTO.py:55-95) drives the HIP
path unchanged: `model.train()`, `loss.backward()`, any torch optimizer over `model.parameters()`.  Gradients
reach every live parameter; `blocks.i.attn.out_proj.*` get none (dead in the reference too), and neither do `x`
and `text_emb` (frozen-encoder outputs in the reference) — asking for those raises.  The standalone
`DiT` / `GlobalAdaLN` modules stay forward-only.

Training for classifier-free guidance: `DiTTO.train_forward_packed` (and the padded `train_forward` over it) does produce the
gradient of `text_emb`, and takes `null_text_emb=` / `drop=` — condition dropout with a learned null embedding, whose rows the
guided samplers take as `null_text_emb=`.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import hip
from .varlen import cond_dropout_layout, validate_cu_seqlens, validate_lengths
from .config import DiTTOConfig
from .engine import TEXT_GRAD_KEY, DenoiseEngine, TextCond, _stream, require_fused_attention
from .synth import cosine_betas


def _require_cuda(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"{what} is on {t.device}: ditto_tts_amd runs only on an MI355X through libditto_hip.so "
                           "(no CPU / eager fallback). Move the module and its inputs to 'cuda'.")


def _refuse_autograd(module: nn.Module):
    if torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters(recurse=True)):
        raise NotImplementedError(
            "ditto_tts_amd: the standalone DiT / GlobalAdaLN modules are forward-only (the backward pass is built for "
            "the whole model: train through DiTTO.forward). Call under torch.no_grad() / torch.inference_mode().")


class _DiTTOTrainFn(torch.autograd.Function):
    """The trainable forward of either layout with its tape, and its backward.  `run(opts)` runs the layout's engine forward and
    returns (eps, backward, release): backward(state, grad_output, piece_cb=, layers_per_piece=) is the engine's backward over
    what that forward left (tape, inputs, options), release() hands the tape back.  `who`: the DiTTO method the caller used.
    `text`: the text rows `run` feeds the forward, as a differentiable input (packed batches: backward(..., text_grad=True) is asked
    for their gradient when autograd needs it), or None (the dense layout, which produces none)."""

    @staticmethod
    def forward(ctx, model, who, run, keys, text, *params):
        # the options in force where forward() is CALLED (a hip.batch_class / hip.call_opts scope of this thread) are this
        # step's options: autograd runs backward() on its own worker thread, where no such scope exists, so they travel with `run`
        out, ctx.run_backward, ctx.release_tape = run(hip.current_opts() if hip._has_call_opts() else None)
        ctx.model, ctx.who, ctx.keys = model, who, keys
        ctx.sig = model._watch.sig
        ctx.text_dtype = None if text is None else text.dtype
        return out

    @staticmethod
    def backward(ctx, grad_out):
        model = ctx.model
        if model._watch.sig != ctx.sig or model._watch.changed(model._path_tensors()):
            raise RuntimeError("DiTTO parameters changed between forward and backward")
        if ctx.release_tape is None:
            raise RuntimeError(f"backward through the same {ctx.who} twice (the activation tape was released)")
        sd = {k: v for k, v in model.state_dict(keep_vars=True).items() if not k.startswith("nac.")}
        sync = getattr(model, "_grad_sync", None)      # dist.GradSync: the gradient exchange overlapped with this backward
        # the text gradient only when autograd has a use for it: without, the backward is the call it always was
        want_text = {"text_grad": True} if ctx.text_dtype is not None and ctx.needs_input_grad[4] else {}
        try:
            grads = ctx.run_backward(sd, grad_out, piece_cb=sync.reduce if sync is not None else None,
                                  layers_per_piece=getattr(model, "_grad_sync_layers", 1), **want_text)
        except BaseException:
            if sync is not None:
                sync.abort()                           # no stale tensors in the next step's buckets
            raise
        if sync is not None:
            sync.finish()                              # the compute stream waits for the exchange: the gradients returned are the means
        ctx.release_tape()
        ctx.run_backward = ctx.release_tape = None
        d_text = grads.get(TEXT_GRAD_KEY)
        if d_text is not None and d_text.dtype != ctx.text_dtype:
            d_text = d_text.to(ctx.text_dtype)
        return (None,) * 4 + (d_text,) + tuple(grads.get(k) for k in ctx.keys)


class _CondDropoutFn(torch.autograd.Function):
    """Condition dropout over a packed batch: the effective text [S_T', text_dim] — every utterance's own rows, or the null embedding's
    when dropped — by one launch of ditto_text_select_packed, and its backward by one of ditto_text_select_packed_bwd: kept rows'
    gradients are copies, dropped utterances' text rows get exact zeros, and the null rows the sum over the dropped utterances in
    ascending order (no atomics: the same bits every time)."""

    @staticmethod
    def forward(ctx, eng, text, null_rows, table, S_out):
        out, tdev = eng.text_select_packed(eng._f32(text, "text_emb"), eng._f32(null_rows, "null_text_emb"), table, S_out)
        ctx.eng, ctx.table, ctx.table_dev = eng, table, tdev
        ctx.shape = (int(text.shape[0]), int(null_rows.shape[0]), text.dtype, null_rows.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        S_T, T0, text_dtype, null_dtype = ctx.shape
        d_text, d_null = ctx.eng.text_select_packed_bwd(g, ctx.table, ctx.table_dev, S_T, T0)
        return None, d_text.to(text_dtype), d_null.to(null_dtype), None, None


class _ParamWatch:
    """Detects parameter changes (optimizer step, load_state_dict, .to()) so packed weights are rebuilt lazily."""

    def __init__(self):
        self.sig = None

    def changed(self, tensors) -> bool:
        sig = tuple((t.data_ptr(), t._version) for t in tensors)
        if sig != self.sig:
            self.sig = sig
            return True
        return False


class GlobalAdaLN(nn.Module):
    """Global Adaptive LayerNorm — reference src/components/DiT.py:8-40."""

    def __init__(self, hidden_dim, time_dim, text_dim):
        super().__init__()
        self.time_mlp = nn.Sequential(nn.SiLU(), nn.Linear(time_dim, 2 * hidden_dim))
        self.text_mlp = nn.Sequential(nn.SiLU(), nn.Linear(text_dim, 2 * hidden_dim))
        self.norm = nn.LayerNorm(hidden_dim, elementwise_affine=False)
        self._dims = (hidden_dim, time_dim, text_dim)

    def forward(self, x, time_emb, text_emb):
        _require_cuda(x, "x")
        _refuse_autograd(self)
        lib = hip.lib()
        d, td, dt = self._dims
        xf = x.float().contiguous()
        te = time_emb.to(x.device).float().contiguous()
        tx = text_emb.to(x.device).float().contiguous()
        B, N, _ = xf.shape
        T = tx.shape[1]
        out = torch.empty_like(xf)
        scratch = torch.empty(lib.ditto_global_adaln_scratch_bytes(B, d, td, dt), dtype=torch.uint8, device=x.device)
        w = [self.time_mlp[1].weight, self.time_mlp[1].bias, self.text_mlp[1].weight, self.text_mlp[1].bias]
        w = [p.detach().float().contiguous() for p in w]
        hip.check(lib.ditto_global_adaln(xf.data_ptr(), te.data_ptr(), tx.data_ptr(), *[p.data_ptr() for p in w],
                                         B, N, T, d, td, dt, out.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                         _stream()))
        return out.to(x.dtype)


class RotaryEmbedding(nn.Module):
    """RoPE — reference src/components/DiT.py:43-72."""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim
        inv_freq = 1.0 / (10000 ** (torch.arange(0, dim, 2).float() / dim))
        self.register_buffer("inv_freq", inv_freq)

    def _rotate_half(self, x):
        x1, x2 = x.chunk(2, dim=-1)
        return torch.cat((-x2, x1), dim=-1)

    def forward(self, seq_len, device):
        # the [N, dh] ANGLE table the reference hands to its blocks; an index outer product, not a hot op
        t = torch.arange(seq_len, device=device).type_as(self.inv_freq)
        freqs = torch.outer(t, self.inv_freq.to(device))
        return torch.cat((freqs, freqs), dim=-1)

    def apply_rope(self, pos, t):
        _require_cuda(t, "t")
        B, N, H, dh = t.shape
        tf = t.float().contiguous()
        out = torch.empty_like(tf)
        posf = pos.to(t.device).float().contiguous()
        hip.check(hip.lib().ditto_apply_rope_f32(posf.data_ptr(), tf.data_ptr(), out.data_ptr(), B, N, H, dh,
                                                 _stream()))
        return out.to(t.dtype)


class DiT(nn.Module):
    """Single DiT block — reference src/components/DiT.py:75-157.

    Parameter containers are the same torch modules the reference instantiates, so the key set is identical
    (including the dead `attn.out_proj.*`)."""

    def __init__(self, hidden_dim, num_heads, time_dim, text_dim):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = hidden_dim // num_heads
        self.norm1 = nn.LayerNorm(hidden_dim)
        self.attn = nn.MultiheadAttention(hidden_dim, num_heads)
        self.rotary = RotaryEmbedding(self.head_dim)
        self.norm2 = nn.LayerNorm(hidden_dim)
        self.cross_attn = nn.MultiheadAttention(hidden_dim, num_heads, dropout=0.1)
        self.norm3 = nn.LayerNorm(hidden_dim)
        self.mlp_fc1 = nn.Linear(hidden_dim, 4 * hidden_dim)
        self.act = nn.GELU()
        self.gate = nn.Linear(hidden_dim, 4 * hidden_dim)
        self.mlp_fc2 = nn.Linear(4 * hidden_dim, hidden_dim)
        self._cfg = DiTTOConfig(hidden_dim, 1, num_heads, time_dim, text_dim, 1)
        self._engine: Optional[DenoiseEngine] = None
        self._watch = _ParamWatch()

    def _standalone_engine(self, device) -> DenoiseEngine:
        tensors = list(self.parameters())
        if self._engine is None or self._watch.changed(tensors) or self._engine.device != device:
            sd = {"blocks.0." + k: v for k, v in self.state_dict().items()}
            self._engine = _BlocksOnlyEngine(self._cfg, sd, device)
            self._watch.changed(tensors)
        return self._engine

    def forward(self, x, text_emb, time_emb, rotary_pos, taps=None):
        """`time_emb` is accepted and ignored, exactly as in the reference.  `taps` (an extension, for
        segment-wise parity tests): a dict that receives the residual stream "after_self" / "after_cross"."""
        _require_cuda(x, "x")
        _refuse_autograd(self)
        eng = self._standalone_engine(x.device)
        half = self.head_dim // 2
        ang = rotary_pos.to(x.device).float()[:, :half].contiguous()   # cat(freqs, freqs): first half suffices
        rope = (torch.cos(ang).contiguous(), torch.sin(ang).contiguous())
        cond = eng.prepare_text(text_emb, x.shape[1])
        h = x.float().contiguous().clone()
        eng.block_forward_(0, h, cond, 0, rope, taps=taps)
        return h.to(x.dtype)


class _BlocksOnlyEngine(DenoiseEngine):
    """An engine over DiT blocks only (no model-level weights): ditto_model_create with NULL globals."""
    _pack_globals = False


class _SpanLossFn(torch.autograd.Function):
    """DiTTO.span_loss_packed: the loss and its gradient with respect to eps in one launch of ditto_span_mse_packed"""

    @staticmethod
    def forward(ctx, eps, eng, cu_seqlens, prompt_lengths, seeds, tag, noise, suffix_lengths=None):
        loss, grad = eng.span_mse_packed(eps.detach().float().contiguous(), cu_seqlens, prompt_lengths, seeds=seeds, tag=tag,
                                         noise=noise, suffix_lengths=suffix_lengths)
        ctx.save_for_backward(grad)
        ctx.eps_dtype = eps.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g).to(ctx.eps_dtype), None, None, None, None, None, None, None


class _SpanVLossFn(torch.autograd.Function):
    """DiTTO.span_loss_packed(prediction="v"): the weighted v loss and its gradient with respect to the prediction in one launch of
    ditto_span_vloss_window"""

    @staticmethod
    def forward(ctx, pred, eng, x0, ca, cs, lw, cu_seqlens, prompt_lengths, seeds, tag, noise, suffix_lengths):
        loss, grad = eng.span_vloss_packed(pred.detach().float().contiguous(), x0, cu_seqlens, prompt_lengths, ca, cs, lw, seeds=seeds,
                                           tag=tag, noise=noise, suffix_lengths=suffix_lengths)
        ctx.save_for_backward(grad)
        ctx.pred_dtype = pred.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return ((grad * g).to(ctx.pred_dtype),) + (None,) * 11


def loss_weight_vector(loss_weights, B: int):
    """`loss_weights` (None, or a list / tuple / tensor of B finite numbers >= 0) as a CPU fp32 tensor [B], or None"""
    if loss_weights is None:
        return None
    if isinstance(loss_weights, torch.Tensor):
        if loss_weights.dtype == torch.bool or loss_weights.is_complex():
            raise ValueError(f"loss_weights: a real tensor is needed, got {loss_weights.dtype}")
        w = loss_weights.detach().to("cpu", torch.float32)
    elif isinstance(loss_weights, (list, tuple)) and all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in loss_weights):
        w = torch.tensor([float(v) for v in loss_weights], dtype=torch.float32)
    else:
        raise ValueError(f"loss_weights: None, a list / tuple of {B} numbers or a tensor [{B}] is needed")
    if w.dim() != 1 or w.shape[0] != B:
        raise ValueError(f"loss_weights: shape [{B}] expected, got {list(w.shape)}")
    if not (torch.isfinite(w).all() and (w >= 0).all()):
        raise ValueError("loss_weights: every weight must be finite and >= 0")
    return w.contiguous()


class DiTTO(nn.Module):
    """Full DiT noise predictor — reference src/model/DiTTO.py:7-126.

    Same keyword arguments.  The reference unconditionally builds `NAC(lambda_factor)` (HF-hub downloads) and
    `torch.load(nac_model_path)`; neither is on the denoise path, so two OPTIONAL escapes are added:
    `nac=` (an already-built codec module to attach as `self.nac`) and `nac_model_path=None` (no codec:
    `self.nac` is None and only the denoise surface works).  With a path, the codec class is imported from the
    caller's own tree (`model.NeuralAudioCodec.NAC`, as the reference does, src/model/DiTTO.py:4)."""

    def __init__(self, hidden_dim=768, num_layers=12, num_heads=12, time_dim=256, text_dim=768,
                 diffusion_steps=1000, lambda_factor=0.1, nac_model_path=None, nac: Optional[nn.Module] = None,
                 fp8_linear: bool = False):
        super().__init__()
        # fp8_linear (extra, optional): QKV / FFN GEMMs with fp8 e4m3 operands (BASELINE config 5)
        self.cfg = DiTTOConfig(hidden_dim, num_layers, num_heads, time_dim, text_dim, diffusion_steps,
                               fp8_linear=fp8_linear)
        if nac is not None:
            self.nac = nac
        elif nac_model_path is not None:
            print("[INFO] Loading NAC model...")
            from model.NeuralAudioCodec import NAC  # the caller's (reference) tree; not part of this package
            self.nac = NAC(lambda_factor=lambda_factor)
            nac_info = torch.load(nac_model_path)
            self.nac.load_state_dict(nac_info["model_state_dict"])
            self.nac.eval()
            for p in self.nac.language_model.parameters():
                p.requires_grad = False
            for p in self.nac.audio_encoder.parameters():
                p.requires_grad = False
            print("[INFO] NAC Loaded.")
        else:
            self.nac = None

        self.t_embedding = nn.Embedding(diffusion_steps, time_dim)
        self.time_embed = nn.Sequential(nn.Linear(time_dim, time_dim), nn.SiLU(), nn.Linear(time_dim, time_dim))
        self.ada_ln = GlobalAdaLN(hidden_dim, time_dim, text_dim)
        self.blocks = nn.ModuleList([DiT(hidden_dim, num_heads, time_dim, text_dim) for _ in range(num_layers)])
        self.proj_in = nn.Linear(hidden_dim, hidden_dim)
        self.proj_out = nn.Linear(hidden_dim, hidden_dim)
        self.rotary = RotaryEmbedding(hidden_dim // num_heads)
        # bug-for-bug: the buffer named alphas_cumprod holds the clipped betas
        self.register_buffer("alphas_cumprod", self.cosine_beta_schedule(diffusion_steps))

        self._engine: Optional[DenoiseEngine] = None
        self._watch = _ParamWatch()
        self._cond_key = None
        self._cond: Optional[TextCond] = None
        self._cond_src: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ engine plumbing
    def _path_tensors(self):
        return [p for n, p in self.named_parameters() if not n.startswith("nac.")] + [self.rotary.inv_freq]

    def engine(self, device=None, train: bool = False) -> DenoiseEngine:
        """The packed HIP model for the current parameters (rebuilt lazily after they change); `train` also packs
        the transposed copies the backward's dgrad GEMMs read."""
        device = torch.device(device) if device is not None else self.proj_in.weight.device
        if device.type != "cuda":
            raise RuntimeError("DiTTO parameters are not on a CUDA (ROCm) device: call .to('cuda') first; "
                               "ditto_tts_amd has no CPU path")
        tensors = self._path_tensors()
        if self._engine is None or self._engine.device != device:
            sd = {k: v for k, v in self.state_dict().items() if not k.startswith("nac.")}
            self._engine = DenoiseEngine(self.cfg, sd, device)
            self._watch.changed(tensors)
            self._cond_key = None
            self._train_packed = False
        elif self._watch.changed(tensors):
            self._engine.repack({k: v for k, v in self.state_dict().items() if not k.startswith("nac.")})
            self._cond_key = None
            self._train_packed = False
        if train and not getattr(self, "_train_packed", False):
            self._engine.train_attach({k: v for k, v in self.state_dict().items() if not k.startswith("nac.")})
            self._train_packed = True
        return self._engine

    def set_grad_sync(self, sync, layers_per_piece: int = 1):
        """Data-parallel training: `sync` (ditto_tts_amd.dist.GradSync, or None to switch off) receives every piece of the
        backward's gradients as soon as that piece is enqueued (engine.train_backward piece_cb) and exchanges them on a side
        stream while the layers below are computed; `loss.backward()` then returns gradients that already are the mean over the
        data-parallel group — no allreduce_gradients call afterwards.  The reference has no distributed training
        (src/utils/Trainer.py:16 trains on one device); this is the hook a multi-GPU Trainer would use."""
        self._grad_sync, self._grad_sync_layers = sync, int(layers_per_piece)

    def text_cond(self, text_emb: torch.Tensor, N_hint: int = 1, text_lengths=None) -> TextCond:
        """Step-invariant text work, cached while the caller keeps passing the same text_emb tensor (the
        sampler does for all its steps, reference src/model/SpeechGenerator.py:161-163) and the same text lengths."""
        eng = self.engine()
        tl = None if text_lengths is None else tuple(validate_lengths(text_lengths, text_emb.shape[0], text_emb.shape[1],
                                                                      "text_lengths").tolist())
        key = (text_emb.data_ptr(), text_emb._version, tuple(text_emb.shape), text_emb.dtype, text_emb.device, tl)
        if key != self._cond_key or self._cond is None:
            self._cond = eng.prepare_text(text_emb, N_hint, text_lengths=None if tl is None else list(tl))
            self._cond_key = key
            # the entry is keyed by ADDRESS: keep the keyed tensor alive for as long as the entry is, or the caching
            # allocator hands the same address (version 0, same shape) to the next utterance's temporary
            # (`text.to(device)` of a CPU tensor, a function-local `wte(tokens)`) and the stale K/V would hit
            self._cond_src = text_emb
        return self._cond

    def invalidate(self):
        """Force a repack of the weights and drop the cached text conditioning on the next call.  Needed only after
        updates the version counters cannot see: in-place writes through `.data` (`p.data.copy_(ema)`,
        some legacy optimizers) do not bump `Tensor._version`."""
        self._watch.sig = None
        self._cond_key = None
        self._cond = None
        self._cond_src = None

    def _inference_only(self, what: str, x, text_emb):
        if torch.is_grad_enabled() and (x.requires_grad or text_emb.requires_grad or
                                        any(p.requires_grad for n, p in self.named_parameters() if not n.startswith("nac."))):
            raise NotImplementedError(f"ditto_tts_amd: {what} are inference only (run under torch.no_grad() or with frozen "
                                      "parameters)")

    def _refuse_fp8_training(self):
        if self.cfg.fp8_linear:
            raise NotImplementedError("ditto_tts_amd: training with fp8_linear=True is not supported")

    @staticmethod
    def _refuse_input_grads(x, text_emb):
        """(packed training produces text_emb's gradient: train_forward_packed passes x for both)"""
        if torch.is_grad_enabled() and (x.requires_grad or text_emb.requires_grad):
            raise NotImplementedError("ditto_tts_amd: gradients with respect to x / text_emb are not produced (the "
                                      "reference feeds frozen-encoder outputs, src/TrainDiTTO.py:66-73); detach them")

    @staticmethod
    def condition_dropout_mask(B: int, p_uncond: float, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """Who trains unconditionally this step: a CPU bool tensor [B], True with probability `p_uncond` per utterance, drawn from
        torch's CPU generator (`generator`, else the default one: torch.manual_seed reproduces it, as it does the cross-attention
        dropout seed).  The `drop=` of train_forward_packed / train_forward."""
        if isinstance(B, bool) or not isinstance(B, int) or B < 1:
            raise ValueError(f"B: a positive int is needed, got {B!r}")
        if not 0.0 <= float(p_uncond) <= 1.0:
            raise ValueError(f"p_uncond: a probability in [0, 1] is needed, got {p_uncond!r}")
        return torch.rand(B, generator=generator) < float(p_uncond)

    def _live_params(self):
        return [(n, p) for n, p in self.named_parameters() if not n.startswith("nac.") and ".attn.out_proj." not in n]

    def _train(self, x, named, who, step, text=None):
        """The trainable forward of either layout under autograd (`named`: _live_params(); `who`: the calling method, for
        messages).  step(eng, p_drop, seed, opts) runs the engine's training forward and returns what _DiTTOTrainFn's `run` does.
        `text`: the text rows `step` feeds it, when their gradient can be produced (packed batches)."""
        # cross-attention dropout is active in train mode only (nn.MultiheadAttention(dropout=0.1),
        # reference src/components/DiT.py:90-91); its mask seed comes from torch's CPU generator
        p_drop = float(self.blocks[0].cross_attn.dropout) if self.training else 0.0
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p_drop > 0 else 0
        out = _DiTTOTrainFn.apply(self, who, lambda opts: step(self.engine(x.device, train=True), p_drop, seed, opts),
                                  tuple(n for n, _ in named), text, *[p for _, p in named])
        return out if x.dtype == torch.float32 else out.to(x.dtype)

    # ------------------------------------------------------------------ reference surface
    def forward(self, x, text_emb, t, *, speech_lengths=None, text_lengths=None):
        """x [B,N,d] noisy latents, text_emb [B,T,text_dim], t [B] long -> predicted noise [B,N,d]
        (reference src/model/DiTTO.py:66-94).  `speech_lengths` / `text_lengths` (list, tuple or int tensor [B]): a
        variable-length batch in the padded layout — utterance b is x[b, :speech_lengths[b]] with text_emb[b, :text_lengths[b]];
        eps rows past its length are 0, and padding contents never reach a valid row (inference only, head_dim 64)."""
        _require_cuda(x, "x")
        varlen = speech_lengths is not None or text_lengths is not None
        if varlen:
            self._inference_only("variable-length batches", x, text_emb)
            eng = self.engine(x.device)
            cond = self.text_cond(text_emb.to(x.device), x.shape[1], text_lengths=text_lengths)
            out = eng.forward(x, cond, t, speech_lengths=speech_lengths)
            return out if x.dtype == torch.float32 else out.to(x.dtype)
        self._refuse_input_grads(x, text_emb)
        named = self._live_params()
        if torch.is_grad_enabled() and any(p.requires_grad for _, p in named):
            self._refuse_fp8_training()

            def step(eng, p_drop, seed, opts):
                out, tape, xf, tt = eng.train_forward(x, text_emb.to(x.device), t, p_drop, seed, opts=opts)
                B, N, T = xf.shape[0], xf.shape[1], text_emb.shape[1]
                return (out, lambda sd, g, **pieces: eng.train_backward(sd, g, xf, tt, T, tape, p_drop, seed, opts=opts, **pieces),
                        lambda: eng.release_tape(tape, B, N, T))
            return self._train(x, named, "DiTTO.forward", step)
        eng = self.engine(x.device)
        cond = self.text_cond(text_emb.to(x.device), x.shape[1])
        out = eng.forward(x, cond, t)
        return out if x.dtype == torch.float32 else out.to(x.dtype)

    def forward_packed(self, x, cu_seqlens, text_emb, text_cu_seqlens, t, *, max_seqlen=None, max_text_seqlen=None):
        """forward over a PACKED batch: x [S, d] with utterance b in rows [cu_seqlens[b], cu_seqlens[b+1]), text_emb [S_T, text_dim]
        with its text in rows [text_cu_seqlens[b], text_cu_seqlens[b+1]), t [B] long -> eps [S, d].  Utterance b gets what
        forward(x[cu[b]:cu[b+1]][None], text_emb[cu_t[b]:cu_t[b+1]][None], t[b:b+1]) gives; no padding is allocated or computed.
        Offsets: list, tuple or int tensor [B + 1] (validated on the host); max_seqlen / max_text_seqlen bound the lengths (default:
        the longest).  Inference only, head_dim 64, bf16 linears."""
        # the refusals first: each is decided by the configuration and the grad mode alone
        self._inference_only("packed batches", x, text_emb)
        require_fused_attention(self.cfg, "packed batches")
        _require_cuda(x, "x")
        eng = self.engine(x.device)
        cond = eng.prepare_text_packed(text_emb.to(x.device), text_cu_seqlens, max_text_seqlen)
        out = eng.forward_packed(x, cond, t, cu_seqlens, max_seqlen)
        return out if x.dtype == torch.float32 else out.to(x.dtype)

    def train_forward_packed(self, x, cu_seqlens, text_emb, text_cu_seqlens, t, *, null_text_emb=None, drop=None, max_seqlen=None,
                             max_text_seqlen=None):
        """The TRAINABLE forward over a packed batch (arguments and validation of forward_packed): eps [S, d] attached to autograd.
        Utterance b's rows are what forward(x[cu[b]:cu[b+1]][None], text_emb[cu_t[b]:cu_t[b+1]][None], t[b:b+1]) gives under
        autograd for it alone — attention over its own keys, the AdaLN text pool over its own text rows, RoPE from its own first row,
        cross-attention dropout (train mode) from the counter hash at utterance-local indices — and backward() leaves in every live
        parameter's .grad the gradient of the caller's loss over the S rows (no padding row exists: F.mse_loss(eps, noise_packed)
        is the mean over real elements).  No gradient for x or `.attn.out_proj.*`, as forward.  head_dim 64, bf16 linears.
        `text_emb.requires_grad` is served: text_emb.grad [S_T, text_dim] arrives from backward() — per layer dkv_l Wkv_l, and the
        AdaLN pool's dpooled[b] / T_b on every row of utterance b — summed in a fixed order (the same bits every time) and without
        changing one bit of a parameter's gradient.
        CONDITION DROPOUT (training for classifier-free guidance): `null_text_emb` [T0, text_dim] — usually an nn.Parameter the caller
        owns and hands its optimizer; it is not registered here, the state_dict keys stay the reference's — and `drop`, a sequence or
        CPU bool tensor [B] (condition_dropout_mask draws one); both or neither.  A dropped utterance runs with the T0 null rows as
        its text: its own K/V, its own pool over T0 rows, its own cross-attention dropout stream; null_text_emb.grad is the sum over
        the dropped utterances, in utterance order, and their rows of text_emb.grad are exactly 0.  The trained rows are what
        stream.submit(null_text_emb=...) takes, and sample_guided_packed(null_text_emb=...) once per utterance (null.repeat(B, 1) with
        null_text_cu_seqlens = the multiples of T0).  With neither, the call is what it was."""
        require_fused_attention(self.cfg, "packed batches")
        self._refuse_fp8_training()
        self._refuse_input_grads(x, x)      # x's gradient stays refused; text_emb's is produced below
        if (null_text_emb is None) != (drop is None):
            raise ValueError("train_forward_packed: null_text_emb= and drop= are given together or not at all")
        if x.dim() != 2 or text_emb.dim() != 2:
            raise ValueError("train_forward_packed: x [S, d] and text_emb [S_T, text_dim] expected")
        B = len(cu_seqlens) - 1
        # validated here, before any launch (the engine validates again on its own entry)
        validate_cu_seqlens(cu_seqlens, B, int(x.shape[0]), int(x.shape[0]) if max_seqlen is None else int(max_seqlen), "cu_seqlens")
        validate_cu_seqlens(text_cu_seqlens, B, int(text_emb.shape[0]),
                            int(text_emb.shape[0]) if max_text_seqlen is None else int(max_text_seqlen), "text_cu_seqlens")
        if x.shape[1] != self.cfg.hidden_dim or text_emb.shape[1] != self.cfg.text_dim or tuple(t.shape) != (B,):
            raise ValueError(f"train_forward_packed: x [S, {self.cfg.hidden_dim}], text_emb [S_T, {self.cfg.text_dim}] and t [{B}] expected")
        layout = None
        if drop is not None:
            if not isinstance(null_text_emb, torch.Tensor) or null_text_emb.dim() != 2 or null_text_emb.shape[1] != self.cfg.text_dim \
                    or null_text_emb.shape[0] < 1 or not null_text_emb.dtype.is_floating_point:
                raise ValueError(f"train_forward_packed: null_text_emb [T0 >= 1, {self.cfg.text_dim}] (floating point) expected, got "
                                 f"{list(null_text_emb.shape) if isinstance(null_text_emb, torch.Tensor) else type(null_text_emb).__name__}")
            layout = cond_dropout_layout(text_cu_seqlens, drop, int(null_text_emb.shape[0]))
        _require_cuda(x, "x")      # the arguments are sound: now the device (there is no CPU path)
        text_in = text_emb.to(x.device)
        if layout is not None:     # the effective text, its offsets and its longest utterance replace the caller's
            text_cu_seqlens, table, max_text_seqlen = layout
            text_in = _CondDropoutFn.apply(self.engine(x.device), text_in, null_text_emb.to(x.device), table, int(text_cu_seqlens[-1]))

        def step(eng, p_drop, seed, opts):
            out, st = eng.train_forward_packed(x, cu_seqlens, text_in, text_cu_seqlens, t, p_drop, seed,
                                               max_seqlen=max_seqlen, max_text_seqlen=max_text_seqlen, opts=opts)
            return (out, lambda sd, g, **pieces: eng.train_backward_packed(sd, g, st, opts=opts, **pieces),
                    lambda: eng.release_tape_packed(st["tape"]))
        return self._train(x, self._live_params(), "DiTTO.train_forward_packed", step, text=text_in)

    def train_forward(self, x, text_emb, t, *, speech_lengths, text_lengths, null_text_emb=None, drop=None):
        """The trainable forward for a batch in the reference's padded collate (src/utils/MLS.py:136-151): x [B, N, d], text_emb
        [B, T, text_dim], utterance b valid on its first speech_lengths[b] / text_lengths[b] rows.  The valid rows are gathered into
        the packed layout, train_forward_packed runs on them, and eps [B, N, d] is scattered into zeros: padded eps rows are exactly
        0, padding contents (NaN included) reach nothing, and gradient arriving on padded rows is dropped.  Speech prompts
        (span_noise_packed / span_loss_packed) exist in the packed layout only: pack the batch first.
        `null_text_emb` / `drop`: condition dropout, passed through to train_forward_packed after packing (text_emb's gradient
        arrives through the gather: padded text rows get zeros)."""
        require_fused_attention(self.cfg, "variable-length batches")
        self._refuse_fp8_training()
        if (null_text_emb is None) != (drop is None):
            raise ValueError("train_forward: null_text_emb= and drop= are given together or not at all")
        if x.dim() != 3 or text_emb.dim() != 3 or text_emb.shape[0] != x.shape[0]:
            raise ValueError("train_forward: x [B, N, d] and text_emb [B, T, text_dim] expected")
        B, N, d = x.shape
        T = text_emb.shape[1]
        sl = validate_lengths(speech_lengths, B, N, "speech_lengths")
        tl = validate_lengths(text_lengths, B, T, "text_lengths")
        _require_cuda(x, "x")
        cu = [0] + torch.cumsum(sl.long(), 0).tolist()
        cu_t = [0] + torch.cumsum(tl.long(), 0).tolist()
        dev = x.device
        sld, tld = sl.to(dev).long(), tl.to(dev).long()
        rows = torch.nonzero((torch.arange(N, device=dev)[None, :] < sld[:, None]).reshape(-1)).reshape(-1)
        trows = torch.nonzero((torch.arange(T, device=dev)[None, :] < tld[:, None]).reshape(-1)).reshape(-1)
        xp = x.reshape(B * N, d).index_select(0, rows)
        tp = text_emb.to(dev).reshape(B * T, text_emb.shape[2]).index_select(0, trows)
        eps_p = self.train_forward_packed(xp, cu, tp, cu_t, t, null_text_emb=null_text_emb, drop=drop, max_seqlen=int(sl.max()),
                                          max_text_seqlen=int(tl.max()))
        out = torch.zeros(B * N, d, dtype=eps_p.dtype, device=dev).index_copy(0, rows, eps_p)
        return out.reshape(B, N, d)

    def span_noise_packed(self, x0, cu_seqlens, prompt_lengths, t, *, seeds=None, tag=0, noise=None, suffix_lengths=None):
        """The forward diffusion of a packed batch with SPEECH PROMPTS (span-masked training): x0 [S, d] clean latents, utterance b
        in rows [cu_seqlens[b], cu_seqlens[b+1]); its first prompt_lengths[b] rows (0 <= P_b < N_b) stay clean — bit copies — and
        the rest become x_in = ca[b] x0 + cs[b] z.  (ca, cs) is the pair q_sample uses for t[b], bug-for-bug: sqrt(c) and
        sqrt(1 - c) with c read from the same mis-named buffer.  z: `noise` (packed [S, d]; its prompt rows are ignored), or
        Philox of (`seeds`[b], `tag`) at the index local to the generated rows — span_loss_packed regenerates it from the same
        (seeds, tag), so it never exists in memory.  One kernel (csrc/span_train.hip).  Returns fp32 [S, d].
        `suffix_lengths` (list / tuple / int tensor [B], Q_b >= 0, P_b + Q_b <= N_b - 1): the span ANYWHERE — the last Q_b rows stay
        clean as well and the window in between is noised, the Philox index local to it (infilling objectives;
        the same kernel).  `prompt_lengths` may then be None (P = 0).  None: the call as it was.
        The padded collate (train_forward) has no prompts: pack the batch first."""
        _require_cuda(x0, "x0")
        eng = self.engine(x0.device)
        c = self.alphas_cumprod.to(x0.device).float()[t.to(x0.device).long()]
        return eng.span_noise_packed(x0.detach().float().contiguous(), cu_seqlens, prompt_lengths, c.sqrt().contiguous(),
                                     (1.0 - c).sqrt().contiguous(), seeds=seeds, tag=tag, noise=noise,
                                     suffix_lengths=suffix_lengths)

    def span_loss_packed(self, eps, cu_seqlens, prompt_lengths, *, seeds=None, tag=0, noise=None, suffix_lengths=None,
                         prediction="eps", x0=None, t=None, loss_weights=None):
        """The span-masked MSE of a packed batch with speech prompts: mean over the GENERATED rows' elements of (eps - z)^2, z as in
        span_noise_packed (the same `noise`, or the same `seeds` and `tag`).  A scalar attached to autograd: backward() hands
        grad_output * (2 / n)(eps - z) — exactly 0 on the prompt rows, whatever eps holds there — to eps's producer
        (train_forward_packed).  Loss and gradient come from one kernel that reads eps once; the reduction is ordered, so the same
        call twice gives the same bits.
        `suffix_lengths`: as in span_noise_packed — the mean runs over the window's d x sum of G_b elements and the gradient is
        exactly 0 on both contexts.  None: the call as it was.
        `prediction`: "eps" (default: the call as it was; `x0`, `t` and `loss_weights` then raise ValueError), or "v" — the network
        is trained to predict v = ca z - cs x0 (Salimans & Ho 2022), the parameterisation a near-zero terminal SNR needs (Lin et al.
        2024): the mean over the generated elements of lw_b (pred - v)^2 from one kernel (ditto_span_vloss_window) that regenerates z
        as above and reads `x0` (the clean latents span_noise_packed was given, [S, d]) beside the prediction.  `t` (the timesteps
        span_noise_packed was given, [B]) picks (ca, cs) exactly as that call does — sqrt(c) and sqrt(1 - c) of the same mis-named
        buffer, bug for bug — so x_in = ca x0 + cs z and v = ca z - cs x0 are consistent whatever c is: ca^2 + cs^2 = 1.  Both are
        required.  `loss_weights` (None, or a list / tuple / tensor of B finite values >= 0): a per-utterance weight on the squared
        error and its gradient, which makes timestep weightings one host line — e.g. min-SNR-gamma for v (Hang et al. 2023), with
        snr = c / (1 - c): [min(s, gamma) / (s + 1) for s in snr].  The gradient is exactly 0 on the context rows and on every row
        of an utterance whose weight is 0.  A model trained this way is sampled with sample_guided_packed(prediction="v") over the
        table it was trained on."""
        if prediction not in ("eps", "v"):
            raise ValueError(f"prediction: one of ('eps', 'v') is needed, got {prediction!r}")
        if prediction == "eps":
            for name, v in (("x0", x0), ("t", t), ("loss_weights", loss_weights)):
                if v is not None:
                    raise ValueError(f'{name}= belongs to prediction="v": the eps loss takes no clean latents, timesteps or weights')
            _require_cuda(eps, "eps")
            return _SpanLossFn.apply(eps, self.engine(eps.device), cu_seqlens, prompt_lengths, seeds, tag, noise, suffix_lengths)
        for name, v in (("x0", x0), ("t", t)):
            if v is None:
                raise ValueError(f'prediction="v" needs {name}= (what span_noise_packed was given)')
        B = len(cu_seqlens) - 1
        lw = loss_weight_vector(loss_weights, B)
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.shape[0] != B or t.dtype.is_floating_point:
            raise ValueError(f"t: an integer tensor [{B}] is needed")
        if not isinstance(x0, torch.Tensor) or x0.shape != eps.shape:
            raise ValueError(f"x0: a tensor of the prediction's shape {list(eps.shape)} is needed")
        _require_cuda(eps, "eps")
        _require_cuda(x0, "x0")
        eng = self.engine(eps.device)
        c = self.alphas_cumprod.to(eps.device).float()[t.to(eps.device).long()]           # span_noise_packed's lines, to the letter
        return _SpanVLossFn.apply(eps, eng, x0.detach().float().contiguous(), c.sqrt().contiguous(), (1.0 - c).sqrt().contiguous(),
                                  None if lw is None else lw.to(eps.device), cu_seqlens, prompt_lengths, seeds, tag, noise,
                                  suffix_lengths)

    def cosine_beta_schedule(self, timesteps, s=0.008):
        """Reference src/model/DiTTO.py:96-104 (a dozen-element host-side table, torch ops as in the reference)."""
        if s != 0.008:
            steps = timesteps + 1
            x = torch.linspace(0, timesteps, steps)
            ac = torch.cos(((x / timesteps) + s) / (1 + s) * torch.pi * 0.5) ** 2
            ac = ac / ac[0]
            return torch.clip(1 - (ac[1:] / ac[:-1]), 0.0001, 0.9999)
        return cosine_betas(timesteps)

    def q_sample(self, x_start, t, noise=None):
        """Forward diffusion, reference src/model/DiTTO.py:106-126 (uses the mis-named buffer, bug-for-bug)."""
        _require_cuda(x_start, "x_start")
        if noise is None:
            noise = torch.randn_like(x_start)
        x0 = x_start.float().contiguous()
        nz = noise.to(x_start.device).float().contiguous()
        tt = t.to(x_start.device).long().contiguous()
        buf = self.alphas_cumprod.to(x_start.device).float().contiguous()
        out = torch.empty_like(x0)
        B = x0.shape[0]
        hip.check(hip.lib().ditto_q_sample(x0.data_ptr(), nz.data_ptr(), tt.data_ptr(), buf.data_ptr(), out.data_ptr(),
                                           B, x0.numel() // B, _stream()))
        return out.to(x_start.dtype)
