"""DenoiseEngine — host-side owner of one packed model on one GPU.

PyTorch is plumbing here: it owns device memory (arena / workspace / cond buffers are uint8 tensors) and
the stream; every FLOP of the path runs in libditto_hip.so.  One engine per process per GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping, Optional, Tuple

import torch

from . import hip
from .varlen import doubled_cu_seqlens, validate_cu_seqlens, validate_lengths
from .config import DiTTOConfig


TEXT_GRAD_KEY = "<text_emb>"      # train_backward_packed(text_grad=True): the text gradient's key beside the state_dict names (none of them)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def require_fused_attention(cfg: DiTTOConfig, what: str):
    """variable-length and packed batches (`what`) run the fused head_dim-64 attention and bf16 linears only
    (NotImplementedError otherwise)"""
    if cfg.head_dim != 64:
        raise NotImplementedError(f"{what} need head_dim 64 (the fused attention kernels); this model's is {cfg.head_dim}")
    if getattr(cfg, "fp8_linear", False):
        raise NotImplementedError(f"{what} are not supported with fp8_linear=True")


class TextCond:
    """Step-invariant conditioning of one utterance batch: cached cross-attention K/V of every layer and the
    text half of the AdaLN modulation (ditto_text_precompute)."""

    def __init__(self, buf: torch.Tensor, B: int, T: int, text_lengths: Optional[torch.Tensor] = None,
                 cu_seqlens: Optional[torch.Tensor] = None, max_len: Optional[int] = None):
        # text_lengths: device int32 [B] of a variable-length batch (ditto_text_precompute_varlen), carried with the K/V cache so
        # that a forward cannot pair this conditioning with other lengths; None = every utterance has all T rows
        self.buf, self.B, self.T, self.text_lengths = buf, B, T, text_lengths
        # cu_seqlens: device int32 [B + 1] of a PACKED conditioning (ditto_text_precompute_packed): T is then the packed text rows
        # S_T and max_len the longest utterance's; only the *_packed entries take it
        self.cu_seqlens, self.max_len = cu_seqlens, max_len


class StepGraph:
    """One captured reverse-diffusion step.  The HIP graph holds raw device addresses; this object owns a reference
    to every buffer behind them (state, conditioning, t, noise, schedule tables, the engine's workspace and RoPE
    tables AT CAPTURE TIME), so the engine growing its workspace or dropping its RoPE cache later cannot hand that
    memory to someone else while the graph can still be replayed.  A repack of the weights (new model handle, arena
    rewritten) invalidates the graph: replay() then raises instead of running on a half-updated arena."""

    def __init__(self, engine, graph, keep):
        self._engine, self._graph, self._keep = engine, graph, keep
        self._generation = engine._generation

    def replay(self):
        if self._generation != self._engine._generation:
            raise RuntimeError("this step graph was captured before the engine's weights were repacked; capture again")
        self._graph.replay()


class DenoiseEngine:
    def __init__(self, cfg: DiTTOConfig, state: Mapping[str, torch.Tensor], device: Optional[torch.device] = None):
        """`state`: reference state_dict keys -> tensors; fp32 CUDA copies are made as needed.
        `nac.*`, `blocks.i.attn.out_proj.*`, `blocks.i.rotary.inv_freq` and `alphas_cumprod` are ignored here."""
        self.lib = hip.lib()
        if not torch.cuda.is_available():
            raise RuntimeError("DenoiseEngine needs an MI355X (torch.cuda.is_available() is False); "
                               "ditto_tts_amd has no CPU path")
        self.cfg = cfg
        self.device = torch.device(device if device is not None else "cuda")
        self._ccfg = hip.make_config(cfg)
        nbytes = self.lib.ditto_arena_bytes(C.byref(self._ccfg))
        if nbytes == 0:
            raise hip.DittoHipError(hip.ERR_SHAPE, self.lib.ditto_last_error().decode())
        self.arena = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.handle = C.c_void_p()
        self._ws: Optional[torch.Tensor] = None
        self._rope: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}
        self._generation = 0            # bumped by every (re)pack: outstanding StepGraphs check it
        self._pack(state)

    # ------------------------------------------------------------------ weights
    def _struct(self, state: Mapping[str, torch.Tensor], ptr=None, globals_: bool = True, skip=()):
        """One ditto_weights (ditto_grads has the same layout) over `state`: field f <- ptr(f's state_dict key), for every layer
        and, with `globals_`, for the model-level fields but `skip`.  `ptr` None: the address of the key's tensor as fp32 on this
        device — no copy when it already is fp32, contiguous and here (an nn.Parameter itself), else a staging copy that the
        keepalive holds.  Returns (struct, keepalive)."""
        keep = []

        def staged(key):
            if key not in state:
                raise KeyError(f"state_dict is missing '{key}'")
            t = state[key].detach().to(device=self.device, dtype=torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()

        ptr = ptr or staged
        L = self.cfg.num_layers
        layers = (hip.LayerWeights * L)()
        for l in range(L):
            for f, k in hip.LAYER_KEY.items():
                setattr(layers[l], f, ptr(f"blocks.{l}.{k}"))
        w = hip.Weights()
        if globals_:
            for f, k in hip.GLOBAL_KEY.items():
                if f not in skip:
                    setattr(w, f, ptr(k))
        w.layers = layers
        keep.append(layers)
        return w, keep

    _pack_globals = True    # False: an engine over DiT blocks only (ditto_model_create with NULL model-level weights)

    def _pack(self, state: Mapping[str, torch.Tensor]):
        w, keep = self._struct(state, globals_=self._pack_globals)  # staging copies must outlive the (stream-ordered) pack kernels
        with torch.cuda.device(self.device):
            if self.handle:
                hip.check(self.lib.ditto_model_destroy(self.handle))
                self.handle = C.c_void_p()
            hip.check(self.lib.ditto_model_create(C.byref(self._ccfg), C.byref(w), self.arena.data_ptr(),
                                                  self.arena.numel(), _stream(), C.byref(self.handle)))
            torch.cuda.current_stream().synchronize()  # staging copies may now be freed
        self._rope.clear()
        self._generation += 1
        self._train_attached = False    # a new handle: the transposed training copies must be re-attached

    def repack(self, state: Mapping[str, torch.Tensor]):
        self._pack(state)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.ditto_model_destroy(self.handle)
        except Exception:
            pass

    # ------------------------------------------------------------------ buffers
    def _grow_ws(self, need: int, attr: str = "_ws") -> torch.Tensor:
        """the grow-only buffer `attr` (the one workspace; "_train_ws": the training step's), grown to `need` bytes (0: the
        library refused the shape)"""
        if need == 0:
            raise hip.DittoHipError(hip.ERR_SHAPE, self.lib.ditto_last_error().decode())
        if getattr(self, attr, None) is None or getattr(self, attr).numel() < need:
            setattr(self, attr, None)       # the old buffer goes before the new one comes
            setattr(self, attr, torch.empty(need, dtype=torch.uint8, device=self.device))
        return getattr(self, attr)

    def workspace(self, B: int, N: int, T: int) -> torch.Tensor:
        return self._grow_ws(self.lib.ditto_workspace_bytes(C.byref(self._ccfg), B, N, T))

    def workspace_packed(self, B: int, S: int, S_T: int) -> torch.Tensor:
        return self._grow_ws(self.lib.ditto_packed_workspace_bytes(C.byref(self._ccfg), B, S, S_T))

    def rope_tables(self, N: int):
        if N not in self._rope:
            half = self.cfg.head_dim // 2
            c = torch.empty(N, half, dtype=torch.float32, device=self.device)
            s = torch.empty_like(c)
            hip.check(self.lib.ditto_rope_tables(self.handle, N, c.data_ptr(), s.data_ptr(), _stream()))
            self._rope[N] = (c, s)
        return self._rope[N]

    # ------------------------------------------------------------------ path
    def _f32(self, t: torch.Tensor, name: str) -> torch.Tensor:
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA (ROCm) tensor: ditto_tts_amd has no CPU path")
        return t.to(dtype=torch.float32).contiguous()

    def prepare_text(self, text_emb: torch.Tensor, N_hint: int = 1, text_lengths=None) -> TextCond:
        """text_emb [B, T, text_dim] -> TextCond (K/V cache of all layers + text modulation).  `text_lengths` (list / tuple /
        int tensor [B]): a variable-length batch — utterance b's text is text_emb[b, :text_lengths[b]], the rest padding."""
        text = self._f32(text_emb, "text_emb")
        B, T, dt = text.shape
        if dt != self.cfg.text_dim:
            raise ValueError(f"text_emb last dim {dt} != text_dim {self.cfg.text_dim}")
        nb = self.lib.ditto_cond_bytes(C.byref(self._ccfg), B, T)
        buf = torch.empty(nb, dtype=torch.uint8, device=self.device)
        ws = self.workspace(B, max(N_hint, 1), T)
        if text_lengths is not None:
            require_fused_attention(self.cfg, "variable-length batches")
            tl = validate_lengths(text_lengths, B, T, "text_lengths").to(self.device)
            hip.check(self.lib.ditto_text_precompute_varlen(self.handle, text.data_ptr(), tl.data_ptr(), B, T, buf.data_ptr(), nb,
                                                            ws.data_ptr(), ws.numel(), _stream()))
            return TextCond(buf, B, T, tl)
        hip.check(self.lib.ditto_text_precompute(self.handle, text.data_ptr(), B, T, buf.data_ptr(), nb,
                                                 ws.data_ptr(), ws.numel(), _stream()))
        return TextCond(buf, B, T)

    @staticmethod
    def _cu(cu_seqlens, B: int, rows: int, max_len: Optional[int], name: str):
        """(validated CPU int32 offsets [B + 1] over `rows` rows, the longest utterance: `max_len`, else the offsets' own)"""
        cu = validate_cu_seqlens(cu_seqlens, B, rows, rows if max_len is None else int(max_len), name)
        return cu, int((cu[1:] - cu[:-1]).max()) if max_len is None else int(max_len)

    def prepare_text_packed(self, text_emb: torch.Tensor, text_cu_seqlens, max_text_seqlen: Optional[int] = None) -> TextCond:
        """text_emb [S_T, text_dim], utterance b in rows [cu[b], cu[b+1]) -> TextCond of a packed batch
        (ditto_text_precompute_packed): the K/V rows of every layer over the S_T rows and the per-utterance text modulation."""
        require_fused_attention(self.cfg, "packed batches")
        text = self._f32(text_emb, "text_emb")
        if text.dim() != 2 or text.shape[1] != self.cfg.text_dim:
            raise ValueError(f"text_emb: [S_T, {self.cfg.text_dim}] expected, got {list(text.shape)}")
        S_T = int(text.shape[0])
        B = len(text_cu_seqlens) - 1
        ct, max_T = self._cu(text_cu_seqlens, B, S_T, max_text_seqlen, "text_cu_seqlens")
        nb = self.lib.ditto_packed_cond_bytes(C.byref(self._ccfg), B, S_T)
        if nb == 0:
            raise hip.DittoHipError(hip.ERR_SHAPE, self.lib.ditto_last_error().decode())
        buf = torch.empty(nb, dtype=torch.uint8, device=self.device)
        ws = self.workspace_packed(B, B, S_T)
        ctd = ct.to(self.device)
        hip.check(self.lib.ditto_text_precompute_packed(self.handle, text.data_ptr(), ctd.data_ptr(), B, S_T, max_T, buf.data_ptr(), nb,
                                                        ws.data_ptr(), ws.numel(), _stream()))
        return TextCond(buf, B, S_T, cu_seqlens=ctd, max_len=max_T)

    def prepare_text_packed_into(self, text: torch.Tensor, text_cu_seqlens, buf: torch.Tensor, at: int = 0) -> int:
        """prepare_text_packed's library call with the image (K/V rows | tmod) written into the uint8 device buffer `buf` at byte
        `at` (a multiple of 256) instead of a fresh buffer: the same arithmetic, so the same bits.  `text`: fp32 CUDA [S_T,
        text_dim], contiguous.  Returns the bytes of the image (ditto_packed_cond_bytes)."""
        require_fused_attention(self.cfg, "packed batches")
        if not (text.is_cuda and text.dtype == torch.float32 and text.is_contiguous() and text.dim() == 2
                and text.shape[1] == self.cfg.text_dim):
            raise ValueError(f"text: a contiguous fp32 CUDA tensor [S_T, {self.cfg.text_dim}] is needed")
        S_T = int(text.shape[0])
        B = len(text_cu_seqlens) - 1
        ct, max_T = self._cu(text_cu_seqlens, B, S_T, None, "text_cu_seqlens")
        nb = self.lib.ditto_packed_cond_bytes(C.byref(self._ccfg), B, S_T)
        if nb == 0:
            raise hip.DittoHipError(hip.ERR_SHAPE, self.lib.ditto_last_error().decode())
        if at % 256 or buf.dtype != torch.uint8 or at + nb > buf.numel():
            raise ValueError("the conditioning image does not fit the buffer at that offset")
        ws = self.workspace_packed(B, B, S_T)
        ctd = ct.to(self.device)
        hip.check(self.lib.ditto_text_precompute_packed(self.handle, text.data_ptr(), ctd.data_ptr(), B, S_T, max_T,
                                                        buf.data_ptr() + at, nb, ws.data_ptr(), ws.numel(), _stream()))
        return int(nb)

    def _packed_cond(self, cond: TextCond, B: int):
        if cond.cu_seqlens is None:
            raise ValueError("a packed call needs a packed conditioning (prepare_text_packed)")
        if cond.B != B:
            raise ValueError(f"the conditioning holds {cond.B} utterances, the call {B}")

    def forward_packed(self, x: torch.Tensor, cond: TextCond, t: torch.Tensor, cu_seqlens, max_seqlen: Optional[int] = None,
                       out: Optional[torch.Tensor] = None, opts: Optional[hip.CallOpts] = None):
        """DiTTO.forward over a packed batch (ditto_forward_packed_opts): x [S, d], utterance b in rows [cu[b], cu[b+1]), with the
        packed conditioning `cond` and t [B] -> eps fp32 [S, d]."""
        require_fused_attention(self.cfg, "packed batches")
        xf = self._f32(x, "x")
        if xf.dim() != 2 or xf.shape[1] != self.cfg.hidden_dim:
            raise ValueError(f"x: [S, {self.cfg.hidden_dim}] expected, got {list(xf.shape)}")
        S = int(xf.shape[0])
        B = len(cu_seqlens) - 1
        self._packed_cond(cond, B)
        cu, max_N = self._cu(cu_seqlens, B, S, max_seqlen, "cu_seqlens")
        tt = self._t64(t, B)
        if out is None:
            out = torch.empty_like(xf)
        ws = self.workspace_packed(B, S, cond.T)
        c, s = self.rope_tables(max_N)
        cud = cu.to(self.device)
        hip.check(self.lib.ditto_forward_packed_opts(self.handle, xf.data_ptr(), cond.buf.data_ptr(), tt.data_ptr(), cud.data_ptr(),
                                                     cond.cu_seqlens.data_ptr(), B, S, max_N, cond.T, cond.max_len, c.data_ptr(),
                                                     s.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(),
                                                     None if opts is None else C.byref(opts)))
        return out

    def guided_offsets_packed(self, cu_seqlens, S: int, max_seqlen: Optional[int], cfg: bool):
        """(device int32 offsets of the step's forward — [cu; S + cu[1:]] under guidance —, max_N) of a packed guided step"""
        require_fused_attention(self.cfg, "packed batches")
        cu, max_N = self._cu(cu_seqlens, len(cu_seqlens) - 1, S, max_seqlen, "cu_seqlens")
        return (doubled_cu_seqlens(cu) if cfg else cu).to(self.device), max_N

    def _packed_step_args(self, who, x2, cond, t, B, doubled, offsets, cu_seqlens, max_seqlen, prompt_len, suffix_len, mirror, opts):
        """The checks every packed guided step shares, after _guided_args' on x2.  `doubled`: x2 [2S, d] = [x; x], cond over
        [text; null], t [2B], offsets [2B + 1] (under guidance, or a refresh of the reuse steps); else x2 [S, d], cond over the text
        alone, t [B], offsets [B + 1].  `mirror` (None outside the reuse steps): x2 is a view of the first S rows of a [2S, d] state.
        Returns (S, nb, max_N, head, tail): the arguments every step entry starts and ends with, by the names include/ditto_hip.h
        gives them (hip.call) — m, x2, cond, t, cu_speech, cu_text; rope_cos, rope_sin, workspace, workspace_bytes, stream, opts."""
        rows, d = int(x2.shape[0]), int(x2.shape[1])
        if doubled and rows % 2:
            raise ValueError("x2 must hold [x; x] " + ("under guidance" if mirror is None else "at a refresh step"))
        S = rows // 2 if doubled else rows
        if mirror and (x2.storage_offset() + 2 * S * d) * 4 > x2.untyped_storage().nbytes():
            raise ValueError(f"{who}: mirror writes rows [S, 2S): x2 must be the first {S} rows of a [{2 * S}, {d}] buffer")
        nb = 2 * B if doubled else B
        self._packed_cond(cond, nb)
        if offsets is None:
            offsets = self.guided_offsets_packed(cu_seqlens, S, max_seqlen, doubled)
        cud, max_N = offsets
        if cud.shape != (nb + 1,):
            raise ValueError(f"offsets: [{nb + 1}] expected")
        for name, v in (("prompt_len", prompt_len), ("suffix_len", suffix_len)):
            if v is not None and not (v.is_cuda and v.dtype == torch.int32 and v.is_contiguous() and v.shape == (B,)):
                raise ValueError(f"{name} must be a contiguous int32 CUDA tensor of shape [{B}]")
        tt = self._t64(t, nb)
        self._step_keep = tt, cud   # until the next step: a t converted or offsets built here must outlive the caller's own allocations
        ws = self.workspace_packed(nb, rows, cond.T)
        c, s = self.rope_tables(max_N)
        head = dict(m=self.handle, x2=x2.data_ptr(), cond=cond.buf.data_ptr(), t=tt.data_ptr(), cu_speech=cud.data_ptr(),
                    cu_text=cond.cu_seqlens.data_ptr())
        tail = dict(rope_cos=c.data_ptr(), rope_sin=s.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel(), stream=_stream(),
                    opts=None if opts is None else C.byref(opts))
        return S, nb, max_N, head, tail

    @staticmethod
    def _rows_like(name, v, S, d):
        if not (v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.shape == (S, d)):
            raise ValueError(f"{name} must be a contiguous fp32 CUDA tensor of shape [{S}, {d}]")

    def guided_step_packed_(self, x2: torch.Tensor, cond: TextCond, t: torch.Tensor, B: int, a: torch.Tensor, ce: torch.Tensor,
                            cz: torch.Tensor, w: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                            seeds: Optional[torch.Tensor] = None, step: int = 0, cu_seqlens=None, max_seqlen: Optional[int] = None,
                            offsets=None, opts: Optional[hip.CallOpts] = None, prompt_len: Optional[torch.Tensor] = None,
                            phi: Optional[torch.Tensor] = None, rescale_scratch: Optional[torch.Tensor] = None,
                            suffix_len: Optional[torch.Tensor] = None):
        """guided_step_ over a packed batch, IN PLACE on x2 fp32 [2S, d] ([x; x], w given) or [S, d]
        (ditto_guided_step_packed_opts).  `offsets`: guided_offsets_packed(...) built once per sampling call (else built here from
        `cu_seqlens`); `cond`: prepare_text_packed over [text; null] (2B utterances) or text.  noise: packed fp32 [S, d].
        `prompt_len` (device int32 [B], validated by the caller: varlen.validate_prompt_lengths): the first prompt_len[b] rows of
        utterance b are a speech prompt the update leaves alone (ditto_guided_step_packed_prompt_opts).
        `phi` (device fp32 [B] in [0, 1], with w): guidance rescale — ditto_guided_step_packed_rescale_opts computes each utterance's
        s32 from this step's eps and the same update runs with ce s32; `rescale_scratch`: rescale_scratch(B, max_N) built once per
        sampling call (else taken here).
        `suffix_len` (device int32 [B], validated by the caller: varlen.validate_suffix_lengths): speech infilling — the last
        suffix_len[b] rows of utterance b are clean context too and the update runs over the window in between
        (ditto_guided_step_packed_window_opts; prompt_len may be None).  Not together with phi."""
        sd, noise = self._guided_args("guided_step_packed_", x2, 2, B, a, ce, cz, w, noise, seeds)
        cfg = w is not None
        S, _, max_N, head, tail = self._packed_step_args("guided_step_packed_", x2, cond, t, B, cfg, offsets, cu_seqlens, max_seqlen,
                                                         prompt_len, suffix_len, None, opts)
        if suffix_len is not None and phi is not None:
            raise NotImplementedError("guidance rescale has no windowed form (suffix_len with phi)")
        update = dict(noise=_ptr(noise), seeds=_ptr(sd), step=int(step) & 0xFFFFFFFF, w=_ptr(w), a=a.data_ptr(), ce=ce.data_ptr(),
                      cz=cz.data_ptr())
        shape = dict(B=B, S=S, max_N=max_N, S_T=cond.T, max_T=cond.max_len)
        if phi is not None:
            if not cfg:
                raise ValueError("guidance rescale needs the guidance scales w")
            phi, rs = self._rescale_args(phi, rescale_scratch, B, max_N)
            hip.check(hip.call("ditto_guided_step_packed_rescale_opts", **head, partner=None, prompt_len=_ptr(prompt_len), **update,
                               tags=None, phi=phi.data_ptr(), **shape, G=0, S_G=0, **tail, scratch=rs.data_ptr(),
                               scratch_bytes=rs.numel()))
            return x2
        if suffix_len is not None:
            entry, spans = "ditto_guided_step_packed_window_opts", dict(prompt_len=_ptr(prompt_len), suffix_len=suffix_len.data_ptr())
        elif prompt_len is not None:
            entry, spans = "ditto_guided_step_packed_prompt_opts", dict(prompt_len=prompt_len.data_ptr())
        else:
            entry, spans = "ditto_guided_step_packed_opts", {}
        hip.check(hip.call(entry, **head, **spans, **update, **shape, cfg=int(cfg), **tail))
        return x2

    def guided_step_packed_multistep_(self, x2: torch.Tensor, cond: TextCond, t: torch.Tensor, B: int, q: torch.Tensor,
                                      coef: Optional[hip.MultistepCoef], w: Optional[torch.Tensor] = None, cu_seqlens=None,
                                      max_seqlen: Optional[int] = None, offsets=None, opts: Optional[hip.CallOpts] = None,
                                      prompt_len: Optional[torch.Tensor] = None, coefs: Optional[torch.Tensor] = None,
                                      phi: Optional[torch.Tensor] = None, rescale_scratch: Optional[torch.Tensor] = None,
                                      suffix_len: Optional[torch.Tensor] = None):
        """guided_step_packed_ with the update of the second-order multistep solver (ditto_guided_step_packed_multistep_opts), IN
        PLACE on x2 and on the history `q` fp32 [S, d]: the previous step's x0 prediction, read only when coef.use_prev and
        rewritten by every step.  `coef`: the step every utterance stands at (sampler.multistep_schedule; its w is ignored, the
        guidance scales are `w` fp32 [B]).  x2, cond, t, offsets, opts, prompt_len: as guided_step_packed_.
        `coefs` (instead of coef and w: device fp32 [B, 8], one ditto_multistep_coef per utterance, its guidance scale inside) with
        `phi` (device fp32 [B]): guidance rescale under guidance — ditto_guided_step_packed_multistep_rescale_opts, the per-utterance
        update with ke s32; `rescale_scratch` as in guided_step_packed_.
        `suffix_len`: as in guided_step_packed_ (ditto_guided_step_packed_multistep_window_opts; the context rows of q are untouched)."""
        if (coefs is None) != (phi is None) or (coefs is None) == (coef is None):
            raise ValueError("guided_step_packed_multistep_: coef (with w), or coefs with phi")
        self._guided_args("guided_step_packed_multistep_", x2, 2, B, None, None, None, w, None, None)
        cfg = w is not None or coefs is not None
        if coefs is not None and not (coefs.is_cuda and coefs.dtype == torch.float32 and coefs.is_contiguous()
                                      and coefs.shape == (B, 8) and coefs.data_ptr() % 16 == 0):
            raise ValueError(f"coefs must be a contiguous, 16-byte aligned fp32 CUDA tensor of shape [{B}, 8]")
        S, _, max_N, head, tail = self._packed_step_args("guided_step_packed_multistep_", x2, cond, t, B, cfg, offsets, cu_seqlens,
                                                         max_seqlen, prompt_len, suffix_len, None, opts)
        self._rows_like("q", q, S, x2.shape[1])
        if suffix_len is not None and phi is not None:
            raise NotImplementedError("guidance rescale has no windowed form (suffix_len with phi)")
        shape = dict(B=B, S=S, max_N=max_N, S_T=cond.T, max_T=cond.max_len)
        if coefs is not None:
            phi, rs = self._rescale_args(phi, rescale_scratch, B, max_N)
            hip.check(hip.call("ditto_guided_step_packed_multistep_rescale_opts", **head, prompt_len=_ptr(prompt_len), q=q.data_ptr(),
                               coefs=coefs.data_ptr(), phi=phi.data_ptr(), **shape, **tail, scratch=rs.data_ptr(),
                               scratch_bytes=rs.numel()))
            return x2
        if suffix_len is not None:
            entry, spans = "ditto_guided_step_packed_multistep_window_opts", dict(prompt_len=_ptr(prompt_len), suffix_len=suffix_len.data_ptr())
        else:
            entry, spans = "ditto_guided_step_packed_multistep_opts", dict(prompt_len=_ptr(prompt_len))
        hip.check(hip.call(entry, **head, **spans, q=q.data_ptr(), step=C.byref(coef), coefs=None, w=_ptr(w), **shape, cfg=int(cfg),
                           **tail))
        return x2

    # ------------------------------------------------------------------ guidance reuse (csrc/guided_reuse.hip)
    @staticmethod
    def _reuse_mode(who, mode, mirror, w) -> bool:
        """The checks of both reuse steps' mode; True at STORE (a refresh: the doubled state), False at LOAD (a reuse step)"""
        if mode not in (hip.REUSE_STORE, hip.REUSE_LOAD):
            raise ValueError(f"{who}: mode must be hip.REUSE_STORE or hip.REUSE_LOAD, got {mode!r}")
        if mode == hip.REUSE_STORE and mirror:
            raise ValueError(f"{who}: mirror belongs to a reuse step (a refresh writes both halves anyway)")
        if w is None:
            raise ValueError(f"{who}: guidance reuse needs the guidance scales w")
        return mode == hip.REUSE_STORE

    def guided_step_packed_reuse_(self, x2: torch.Tensor, cond: TextCond, t: torch.Tensor, B: int, delta: torch.Tensor,
                                  a: torch.Tensor, ce: torch.Tensor, cz: torch.Tensor, w: torch.Tensor, mode: int, mirror: bool = False,
                                  noise: Optional[torch.Tensor] = None, seeds: Optional[torch.Tensor] = None, step: int = 0,
                                  cu_seqlens=None, max_seqlen: Optional[int] = None, offsets=None,
                                  opts: Optional[hip.CallOpts] = None, prompt_len: Optional[torch.Tensor] = None,
                                  suffix_len: Optional[torch.Tensor] = None):
        """One strided (DDIM) step of a loop that reuses the guidance direction (ditto_guided_step_packed_reuse_opts), IN PLACE on
        x2 and `delta` fp32 [S, d].  mode hip.REUSE_STORE — a refresh: guided_step_packed_'s guided step on x2 [2S, d] (the same
        forward, the same bits on x2) that also keeps delta = c - u.  mode hip.REUSE_LOAD — a reuse step: the forward over the B
        conditional utterances of x2 [S, d] alone, with `cond` over the text only, and the update with e = c + (w - 1) delta; with
        `mirror`, x' is written to rows [S, 2S) of the buffer x2 is the first half of as well (what the next refresh reads).
        Everything else as guided_step_packed_."""
        who = "guided_step_packed_reuse_"
        sd, noise = self._guided_args(who, x2, 2, B, a, ce, cz, w if mode == hip.REUSE_STORE else None, noise, seeds)
        self._guided_args(who, x2, 2, B, None, None, None, w, None, None)
        store = self._reuse_mode(who, mode, mirror, w)
        S, _, max_N, head, tail = self._packed_step_args(who, x2, cond, t, B, store, offsets, cu_seqlens, max_seqlen, prompt_len,
                                                         suffix_len, bool(mirror), opts)
        self._rows_like("delta", delta, S, x2.shape[1])
        hip.check(hip.call("ditto_guided_step_packed_reuse_opts", **head, prompt_len=_ptr(prompt_len), suffix_len=_ptr(suffix_len),
                           delta=delta.data_ptr(), noise=_ptr(noise), seeds=_ptr(sd), step=int(step) & 0xFFFFFFFF, w=w.data_ptr(),
                           a=a.data_ptr(), ce=ce.data_ptr(), cz=cz.data_ptr(), B=B, S=S, max_N=max_N, S_T=cond.T, max_T=cond.max_len,
                           mode=int(mode), mirror=int(bool(mirror)), **tail))
        return x2

    def guided_step_packed_multistep_reuse_(self, x2: torch.Tensor, cond: TextCond, t: torch.Tensor, B: int, q: torch.Tensor,
                                            delta: torch.Tensor, coef: hip.MultistepCoef, w: torch.Tensor, mode: int,
                                            mirror: bool = False, cu_seqlens=None, max_seqlen: Optional[int] = None, offsets=None,
                                            opts: Optional[hip.CallOpts] = None, prompt_len: Optional[torch.Tensor] = None,
                                            suffix_len: Optional[torch.Tensor] = None):
        """guided_step_packed_reuse_ with the update of the second-order multistep solver
        (ditto_guided_step_packed_multistep_reuse_opts), IN PLACE on x2, the history `q` fp32 [S, d] and `delta`.  `coef`: the step
        every utterance stands at, as in guided_step_packed_multistep_ (no per-utterance `coefs` form)."""
        who = "guided_step_packed_multistep_reuse_"
        self._guided_args(who, x2, 2, B, None, None, None, w, None, None)
        store = self._reuse_mode(who, mode, mirror, w)
        S, _, max_N, head, tail = self._packed_step_args(who, x2, cond, t, B, store, offsets, cu_seqlens, max_seqlen, prompt_len,
                                                         suffix_len, bool(mirror), opts)
        self._rows_like("delta", delta, S, x2.shape[1])
        self._rows_like("q", q, S, x2.shape[1])
        hip.check(hip.call("ditto_guided_step_packed_multistep_reuse_opts", **head, prompt_len=_ptr(prompt_len),
                           suffix_len=_ptr(suffix_len), q=q.data_ptr(), delta=delta.data_ptr(), step=C.byref(coef), w=w.data_ptr(), B=B, S=S,
                           max_N=max_N, S_T=cond.T, max_T=cond.max_len, mode=int(mode), mirror=int(bool(mirror)), **tail))
        return x2

    # ------------------------------------------------------------------ guidance rescale (csrc/guided_rescale.hip)
    def rescale_scratch(self, B: int, max_N: int) -> torch.Tensor:
        """the scratch of a guidance rescale over B utterances of at most max_N rows (ditto_guidance_rescale_bytes): uint8, zeroed"""
        need = int(self.lib.ditto_guidance_rescale_bytes(int(B), int(max_N), self.cfg.hidden_dim))
        if need == 0:
            raise hip.DittoHipError(hip.ERR_SHAPE, self.lib.ditto_last_error().decode())
        return torch.zeros(need, dtype=torch.uint8, device=self.device)

    def _rescale_args(self, phi, scratch, B, max_N):
        if not (phi.is_cuda and phi.dtype == torch.float32 and phi.is_contiguous() and phi.shape == (B,)):
            raise ValueError(f"phi must be a contiguous fp32 CUDA tensor of shape [{B}]")
        if scratch is None:
            scratch = self.rescale_scratch(B, max_N)
        if not (scratch.is_cuda and scratch.dtype == torch.uint8 and scratch.is_contiguous() and scratch.data_ptr() % 256 == 0):
            raise ValueError("rescale_scratch must be a contiguous, 256-byte aligned uint8 CUDA tensor")
        return phi, scratch

    def guidance_rescale_packed(self, eps2: torch.Tensor, offsets: torch.Tensor, phi: torch.Tensor, B: int, S: int, max_N: int, *,
                                w: Optional[torch.Tensor] = None, coef_in: Optional[torch.Tensor] = None,
                                coefs: Optional[torch.Tensor] = None, prompt_len: Optional[torch.Tensor] = None,
                                partner: Optional[torch.Tensor] = None, G: int = 0, S_G: int = 0,
                                scratch: Optional[torch.Tensor] = None):
        """The guidance-rescale statistics alone (ditto_guidance_rescale_packed) over eps2 fp32 [2S, d] (partner None: the
        unconditional half at row offset S) or [S + S_G, d] (partner device int32 [B]: the mixed layout of guided_mixed.hip);
        `offsets`: the device int32 offsets the step's update reads.  Either `coef_in` and `w` (fp32 [B]) or `coefs` (fp32 [B, 8]:
        ditto_multistep_coef).  Returns (coef_out — fp32 [B], or [B, 8] with ke scaled —, scale fp32 [B]): views of `scratch`."""
        phi, scratch = self._rescale_args(phi, scratch, B, max_N)
        hip.check(self.lib.ditto_guidance_rescale_packed(
            eps2.data_ptr(), _ptr(w), phi.data_ptr(), _ptr(coef_in), _ptr(coefs), offsets.data_ptr(), _ptr(prompt_len), _ptr(partner),
            B, int(G), S, int(S_G), max_N, int(eps2.shape[1]), scratch.data_ptr(), scratch.numel(), _stream()))
        o_scale, _ = hip.rescale_scratch_layout(B)
        out = scratch[:32 * B].view(torch.float32).view(B, 8) if coefs is not None else scratch[:4 * B].view(torch.float32)
        return out, scratch[o_scale:o_scale + 4 * B].view(torch.float32)

    # ------------------------------------------------------------------ projected guidance (csrc/guided_project.hip)
    def project_scratch(self, B: int, max_N: int) -> torch.Tensor:
        """the scratch of a projected-guidance step over B utterances of at most max_N rows (ditto_guidance_project_bytes): uint8, zeroed"""
        need = int(self.lib.ditto_guidance_project_bytes(int(B), int(max_N), self.cfg.hidden_dim))
        if need == 0:
            raise hip.DittoHipError(hip.ERR_SHAPE, self.lib.ditto_last_error().decode())
        return torch.zeros(need, dtype=torch.uint8, device=self.device)

    def _project_args(self, proj, direction, scratch, B, S, d, max_N):
        if not (proj.is_cuda and proj.dtype == torch.float32 and proj.is_contiguous() and proj.shape == (B, 8)
                and proj.data_ptr() % 16 == 0):
            raise ValueError(f"proj must be a contiguous, 16-byte aligned fp32 CUDA tensor of shape [{B}, 8] (ditto_project_coef)")
        self._rows_like("direction", direction, S, d)
        if scratch is None:
            scratch = self.project_scratch(B, max_N)
        if not (scratch.is_cuda and scratch.dtype == torch.uint8 and scratch.is_contiguous() and scratch.data_ptr() % 256 == 0):
            raise ValueError("project_scratch must be a contiguous, 256-byte aligned uint8 CUDA tensor")
        return scratch

    def guidance_project_packed(self, x2: torch.Tensor, eps2: torch.Tensor, direction: torch.Tensor, proj: torch.Tensor,
                                offsets: torch.Tensor, B: int, S: int, max_N: int, *, prompt_len: Optional[torch.Tensor] = None,
                                suffix_len: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None):
        """The direction and statistics of one projected-guidance step alone (ditto_guidance_project_packed; include/ditto_project.h):
        x2, eps2 fp32 [2S, d], `direction` fp32 [S, d] updated IN PLACE on the window rows, `proj` fp32 [B, 8] (ditto_project_coef per
        utterance), `offsets` the device int32 offsets the step's update reads.  Returns pcoef fp32 [B, 4] = (fx, fc, fd, 0): a view
        of `scratch`, which the update entries read."""
        d = int(eps2.shape[1])
        scratch = self._project_args(proj, direction, scratch, B, S, d, max_N)
        hip.check(hip.call("ditto_guidance_project_packed", x2=x2.data_ptr(), eps2=eps2.data_ptr(), dir=direction.data_ptr(),
                           proj=proj.data_ptr(), cu=offsets.data_ptr(), prompt_len=_ptr(prompt_len), suffix_len=_ptr(suffix_len), B=B, S=S,
                           max_N=max_N, d=d, scratch=scratch.data_ptr(), scratch_bytes=scratch.numel(), stream=_stream()))
        return scratch[:16 * B].view(torch.float32).view(B, 4)

    def guided_step_packed_project_(self, x2: torch.Tensor, cond: TextCond, t: torch.Tensor, B: int, direction: torch.Tensor,
                                    proj: torch.Tensor, a: torch.Tensor, ce: torch.Tensor, cz: torch.Tensor,
                                    noise: Optional[torch.Tensor] = None, seeds: Optional[torch.Tensor] = None, step: int = 0,
                                    cu_seqlens=None, max_seqlen: Optional[int] = None, offsets=None,
                                    opts: Optional[hip.CallOpts] = None, prompt_len: Optional[torch.Tensor] = None,
                                    suffix_len: Optional[torch.Tensor] = None, project_scratch: Optional[torch.Tensor] = None):
        """One strided (DDIM) step with projected guidance (APG; ditto_guided_step_packed_project_opts), IN PLACE on x2 fp32 [2S, d]
        and `direction` fp32 [S, d]: guided_step_packed_'s guided forward, then the direction and its statistics on that eps, then
        the update with e = fx x + fc c + fd m'.  `proj`: device fp32 [B, 8], one ditto_project_coef per utterance (kx, ke, w, eta,
        r, beta, use_prev) — the guidance scale travels inside; `project_scratch`: project_scratch(B, max_N) built once per
        sampling call (else taken here).  Everything else as guided_step_packed_."""
        who = "guided_step_packed_project_"
        sd, noise = self._guided_args(who, x2, 2, B, a, ce, cz, a, noise, seeds)   # in w's place: x2 is the doubled state
        S, _, max_N, head, tail = self._packed_step_args(who, x2, cond, t, B, True, offsets, cu_seqlens, max_seqlen, prompt_len,
                                                         suffix_len, None, opts)
        rs = self._project_args(proj, direction, project_scratch, B, S, int(x2.shape[1]), max_N)
        hip.check(hip.call("ditto_guided_step_packed_project_opts", **head, prompt_len=_ptr(prompt_len), suffix_len=_ptr(suffix_len),
                           dir=direction.data_ptr(), proj=proj.data_ptr(), noise=_ptr(noise), seeds=_ptr(sd),
                           step=int(step) & 0xFFFFFFFF, tags=None, a=a.data_ptr(), ce=ce.data_ptr(), cz=cz.data_ptr(), B=B, S=S,
                           max_N=max_N, S_T=cond.T, max_T=cond.max_len, **tail, scratch=rs.data_ptr(), scratch_bytes=rs.numel()))
        return x2

    def guided_step_packed_multistep_project_(self, x2: torch.Tensor, cond: TextCond, t: torch.Tensor, B: int, q: torch.Tensor,
                                              direction: torch.Tensor, proj: torch.Tensor, coef: hip.MultistepCoef, cu_seqlens=None,
                                              max_seqlen: Optional[int] = None, offsets=None, opts: Optional[hip.CallOpts] = None,
                                              prompt_len: Optional[torch.Tensor] = None, suffix_len: Optional[torch.Tensor] = None,
                                              project_scratch: Optional[torch.Tensor] = None):
        """guided_step_packed_project_ with the update of the second-order multistep solver
        (ditto_guided_step_packed_multistep_project_opts), IN PLACE on x2, the history `q` fp32 [S, d] and `direction`.  `coef`: the
        step every utterance stands at, as in guided_step_packed_multistep_ (its w is ignored: the scales travel in `proj`)."""
        who = "guided_step_packed_multistep_project_"
        self._guided_args(who, x2, 2, B, None, None, None, None, None, None)
        S, _, max_N, head, tail = self._packed_step_args(who, x2, cond, t, B, True, offsets, cu_seqlens, max_seqlen, prompt_len,
                                                         suffix_len, None, opts)
        self._rows_like("q", q, S, x2.shape[1])
        rs = self._project_args(proj, direction, project_scratch, B, S, int(x2.shape[1]), max_N)
        hip.check(hip.call("ditto_guided_step_packed_multistep_project_opts", **head, prompt_len=_ptr(prompt_len),
                           suffix_len=_ptr(suffix_len), q=q.data_ptr(), dir=direction.data_ptr(), proj=proj.data_ptr(), step=C.byref(coef),
                           coefs=None, B=B, S=S, max_N=max_N, S_T=cond.T, max_T=cond.max_len, **tail, scratch=rs.data_ptr(),
                           scratch_bytes=rs.numel()))
        return x2

    # ------------------------------------------------------------------ span-masked training (csrc/span_train.hip)
    def _span_args(self, who, buf, cu_seqlens, prompt_lengths, seeds, noise, suffix_lengths=None):
        """the checks of span_noise_packed / span_mse_packed: (device offsets, device prompt lengths, B, max_N, generated rows,
        seeds int64 [B] or None, noise fp32 [S, d] or None, device suffix lengths or None).  With `suffix_lengths` the prompt lengths
        may be None (device None: P = 0)."""
        from .varlen import validate_prompt_lengths, validate_suffix_lengths
        if not (buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous() and buf.dim() == 2 and buf.shape[1] % 64 == 0):
            raise ValueError(f"{who} needs a contiguous fp32 CUDA tensor [S, d] with d % 64 == 0")
        if (seeds is None) == (noise is None):
            raise ValueError(f"{who}: exactly one of seeds= and noise= is needed")
        S = int(buf.shape[0])
        B = len(cu_seqlens) - 1
        cu, max_N = self._cu(cu_seqlens, B, S, None, "cu_seqlens")
        ql = None if suffix_lengths is None else validate_suffix_lengths(suffix_lengths, cu, prompt_lengths)
        pl = None if (prompt_lengths is None and ql is not None) else validate_prompt_lengths(prompt_lengths, cu)
        if noise is not None:
            noise = self._f32(noise, "noise")
            if noise.shape != buf.shape:
                raise ValueError(f"noise must have shape {list(buf.shape)}")
        sd = self._t64(seeds, B) if seeds is not None else None
        gen = S - (0 if pl is None else int(pl.sum())) - (0 if ql is None else int(ql.sum()))
        return (cu.to(self.device), None if pl is None else pl.to(self.device), B, max_N, gen, sd, noise,
                None if ql is None else ql.to(self.device))

    def span_noise_packed(self, x0: torch.Tensor, cu_seqlens, prompt_lengths, ca: torch.Tensor, cs: torch.Tensor, seeds=None,
                          tag: int = 0, noise=None, suffix_lengths=None) -> torch.Tensor:
        """x_in fp32 [S, d]: x0 on each utterance's prompt rows, ca[b] x0 + cs[b] z on its generated rows (ditto_span_noise_packed).
        `suffix_lengths`: the last Q_b rows stay clean too (ditto_span_noise_window; prompt_lengths may then be None)."""
        cud, pld, B, max_N, _, sd, noise, qld = self._span_args("span_noise_packed", x0, cu_seqlens, prompt_lengths, seeds, noise,
                                                                suffix_lengths)
        for name, v in (("ca", ca), ("cs", cs)):
            if not (v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.shape == (B,)):
                raise ValueError(f"{name} must be a contiguous fp32 CUDA tensor of shape [{B}]")
        out = torch.empty_like(x0)
        if qld is not None:
            hip.check(self.lib.ditto_span_noise_window(x0.data_ptr(), _ptr(noise), _ptr(sd), int(tag) & 0xFFFFFFFF, ca.data_ptr(),
                                                       cs.data_ptr(), cud.data_ptr(), _ptr(pld), qld.data_ptr(), out.data_ptr(), B,
                                                       x0.shape[0], max_N, x0.shape[1], _stream()))
            return out
        hip.check(self.lib.ditto_span_noise_packed(x0.data_ptr(), _ptr(noise), _ptr(sd), int(tag) & 0xFFFFFFFF, ca.data_ptr(),
                                                   cs.data_ptr(), cud.data_ptr(), pld.data_ptr(), out.data_ptr(), B, x0.shape[0], max_N,
                                                   x0.shape[1], _stream()))
        return out

    def span_mse_packed(self, eps: torch.Tensor, cu_seqlens, prompt_lengths, seeds=None, tag: int = 0, noise=None, suffix_lengths=None):
        """(loss fp32 [], grad_eps fp32 [S, d]) of the MSE over the generated rows (ditto_span_mse_packed; with `suffix_lengths`
        ditto_span_mse_window: the rows between the two contexts, normalised by d x their number)"""
        cud, pld, B, max_N, gen_rows, sd, noise, qld = self._span_args("span_mse_packed", eps, cu_seqlens, prompt_lengths, seeds, noise,
                                                                       suffix_lengths)
        S, d = int(eps.shape[0]), int(eps.shape[1])
        grad = torch.empty_like(eps)
        loss = torch.empty((), dtype=torch.float32, device=eps.device)
        part = torch.empty(B * min(1024, (max_N * d // 4 + 255) // 256), dtype=torch.float32, device=eps.device)
        if qld is not None:
            hip.check(self.lib.ditto_span_mse_window(eps.data_ptr(), _ptr(noise), _ptr(sd), int(tag) & 0xFFFFFFFF, cud.data_ptr(),
                                                     _ptr(pld), qld.data_ptr(), gen_rows * d, grad.data_ptr(), loss.data_ptr(),
                                                     part.data_ptr(), part.numel() * 4, B, S, max_N, d, _stream()))
            return loss, grad
        hip.check(self.lib.ditto_span_mse_packed(eps.data_ptr(), _ptr(noise), _ptr(sd), int(tag) & 0xFFFFFFFF, cud.data_ptr(),
                                                 pld.data_ptr(), gen_rows * d, grad.data_ptr(), loss.data_ptr(), part.data_ptr(),
                                                 part.numel() * 4, B, S, max_N, d, _stream()))
        return loss, grad

    def span_vloss_packed(self, pred: torch.Tensor, x0: torch.Tensor, cu_seqlens, prompt_lengths, ca: torch.Tensor, cs: torch.Tensor,
                          lw=None, seeds=None, tag: int = 0, noise=None, suffix_lengths=None):
        """(loss fp32 [], grad_pred fp32 [S, d]) of the v objective over the generated rows (ditto_span_vloss_window): target =
        ca[b] z - cs[b] x0, squared error weighted by lw[b] (fp32 CUDA [B], or None: 1).  prompt_lengths and suffix_lengths may each
        be None."""
        if prompt_lengths is None and suffix_lengths is None:
            prompt_lengths = [0] * (len(cu_seqlens) - 1)
        cud, pld, B, max_N, gen_rows, sd, noise, qld = self._span_args("span_vloss_packed", pred, cu_seqlens, prompt_lengths, seeds, noise,
                                                                       suffix_lengths)
        if not (x0.is_cuda and x0.dtype == torch.float32 and x0.is_contiguous() and x0.shape == pred.shape):
            raise ValueError(f"x0 must be a contiguous fp32 CUDA tensor of shape {list(pred.shape)}")
        for name, v in (("ca", ca), ("cs", cs), ("lw", lw)):
            if v is not None and not (v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.shape == (B,)):
                raise ValueError(f"{name} must be a contiguous fp32 CUDA tensor of shape [{B}]")
        S, d = int(pred.shape[0]), int(pred.shape[1])
        grad = torch.empty_like(pred)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        part = torch.empty(B * min(1024, (max_N * d // 4 + 255) // 256), dtype=torch.float32, device=pred.device)
        hip.check(self.lib.ditto_span_vloss_window(pred.data_ptr(), x0.data_ptr(), _ptr(noise), _ptr(sd), int(tag) & 0xFFFFFFFF,
                                                   ca.data_ptr(), cs.data_ptr(), _ptr(lw), cud.data_ptr(), _ptr(pld), _ptr(qld),
                                                   gen_rows * d, grad.data_ptr(), loss.data_ptr(), part.data_ptr(), part.numel() * 4,
                                                   B, S, max_N, d, _stream()))
        return loss, grad

    def _lengths(self, speech_lengths, cond: TextCond, B: int, N: int, halves: int = 1):
        """(speech, text) device int32 [halves * B] of a varlen call, or None for a dense one.  `speech_lengths`: the B
        utterances' (list / tuple / int tensor), repeated by each half of a guided [x; x] (halves 2); the text lengths are the
        conditioning's own."""
        if speech_lengths is None and cond.text_lengths is None:
            return None
        require_fused_attention(self.cfg, "variable-length batches")
        sl = (validate_lengths(speech_lengths, B, N, "speech_lengths") if speech_lengths is not None
              else torch.full((B,), N, dtype=torch.int32))
        tl = (cond.text_lengths if cond.text_lengths is not None
              else torch.full((halves * B,), cond.T, dtype=torch.int32, device=self.device))
        return sl.repeat(halves).to(self.device), tl

    def prepare_text_into(self, text_emb: torch.Tensor, N_hint: int, cond: TextCond) -> TextCond:
        """Recompute the conditioning of a new utterance batch into an EXISTING TextCond buffer (same B, T), so
        captured graphs bound to that buffer stay valid."""
        text = self._f32(text_emb, "text_emb")
        B, T, _ = text.shape
        if cond.text_lengths is not None:
            raise NotImplementedError("prepare_text_into on a variable-length conditioning: call prepare_text(..., text_lengths=)")
        if (B, T) != (cond.B, cond.T):
            raise ValueError("prepare_text_into needs the same (B, T) as the existing conditioning")
        ws = self.workspace(B, max(N_hint, 1), T)
        hip.check(self.lib.ditto_text_precompute(self.handle, text.data_ptr(), B, T, cond.buf.data_ptr(),
                                                 cond.buf.numel(), ws.data_ptr(), ws.numel(), _stream()))
        return cond

    def _t64(self, t: torch.Tensor, B: int) -> torch.Tensor:
        if t.shape != (B,):
            raise ValueError(f"t must have shape [{B}]")
        return t.to(device=self.device, dtype=torch.int64).contiguous()

    def _call_varlen(self, name, lens, head, tail, opts):
        """`name` of a dense batch (lens None: through _call), else `name`_varlen_opts with the (speech, text) length pointers
        between the arguments `head` and `tail`"""
        if lens is None:
            self._call(name, *head, *tail, opts=opts)
        else:
            hip.check(getattr(self.lib, name + "_varlen_opts")(*head, lens[0].data_ptr(), lens[1].data_ptr(), *tail,
                                                               None if opts is None else C.byref(opts)))

    def _call(self, name, *args, opts=None):
        """`name`_opts(*args, opts) — the entry point with this call's ditto_call_opts (None = NULL: every field inherits the
        thread's scope / the process defaults); a frozen pre-ABI-9 library (DITTO_HIP_LIB: tools/ A/Bs) has only `name`."""
        if hip._has_call_opts():
            hip.check(getattr(self.lib, name + "_opts")(*args, None if opts is None else C.byref(opts)))
        elif opts is not None:
            raise RuntimeError("per-call options need an ABI-9 libditto_hip.so")
        else:
            hip.check(getattr(self.lib, name)(*args))

    def forward(self, x: torch.Tensor, cond: TextCond, t: torch.Tensor, out: Optional[torch.Tensor] = None,
                opts: Optional[hip.CallOpts] = None, speech_lengths=None):
        """DiTTO.forward(x, text_emb, t) with text_emb pre-digested into `cond` -> eps fp32 [B,N,d].  `opts`: this call's
        hip.CallOpts (kernel class pin, residual-stream type ...: include/ditto_hip.h ditto_call_opts).  `speech_lengths` (or a
        `cond` with text lengths): a variable-length batch; eps rows past an utterance's length are 0."""
        xf = self._f32(x, "x")
        B, N, d = xf.shape
        if d != self.cfg.hidden_dim or B != cond.B:
            raise ValueError("x shape does not match the model / the conditioning batch")
        tt = self._t64(t, B)
        if out is None:
            out = torch.empty_like(xf)
        ws = self.workspace(B, N, cond.T)
        c, s = self.rope_tables(N)
        self._call_varlen("ditto_forward", self._lengths(speech_lengths, cond, B, N),
                          (self.handle, xf.data_ptr(), cond.buf.data_ptr(), tt.data_ptr()),
                          (B, N, cond.T, c.data_ptr(), s.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), opts)
        return out

    def p_sample_(self, x: torch.Tensor, cond: TextCond, t: torch.Tensor, noise: Optional[torch.Tensor],
                  betas: torch.Tensor, alphas: torch.Tensor, alphas_cumprod: torch.Tensor,
                  opts: Optional[hip.CallOpts] = None, speech_lengths=None):
        """One reverse-diffusion step IN PLACE on the fp32 CUDA state x [B,N,d] (varlen: rows past a length become 0)."""
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
            raise ValueError("p_sample_ needs a contiguous fp32 CUDA state tensor (it is updated in place)")
        B, N, d = x.shape
        tt = self._t64(t, B)
        ws = self.workspace(B, N, cond.T)
        c, s = self.rope_tables(N)
        if noise is not None:
            noise = self._f32(noise, "noise")
        self._call_varlen("ditto_p_sample", self._lengths(speech_lengths, cond, B, N),
                          (self.handle, x.data_ptr(), cond.buf.data_ptr(), tt.data_ptr(), _ptr(noise)),
                          (betas.data_ptr(), alphas.data_ptr(), alphas_cumprod.data_ptr(), B, N, cond.T, c.data_ptr(), s.data_ptr(),
                           ws.data_ptr(), ws.numel(), _stream()), opts)
        return x

    def noise_normal_(self, out: torch.Tensor, seeds: torch.Tensor, step: int):
        """out[b] <- N(0,1) of (seeds[b], step): Philox4x32-10 + Box-Muller in libditto_hip (ditto_noise_normal).  A function
        of the utterance's seed, the step and the element index only — independent of batch composition and GPU."""
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()):
            raise ValueError("noise_normal_ needs a contiguous fp32 CUDA tensor")
        B = out.shape[0]
        sd = self._t64(seeds, B)
        hip.check(self.lib.ditto_noise_normal(out.data_ptr(), sd.data_ptr(), int(step) & 0xFFFFFFFF, B,
                                              out.numel() // B, _stream()))
        return out

    def p_sample_seeded_(self, x: torch.Tensor, cond: TextCond, t: torch.Tensor, seeds: torch.Tensor, step: int,
                         betas: torch.Tensor, alphas: torch.Tensor, alphas_cumprod: torch.Tensor,
                         opts: Optional[hip.CallOpts] = None, speech_lengths=None):
        """p_sample_ with the step's noise generated inside the update kernel from per-utterance seeds
        (bit-identical to noise_normal_(z, seeds, step) + p_sample_(x, ..., z))."""
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
            raise ValueError("p_sample_seeded_ needs a contiguous fp32 CUDA state tensor (it is updated in place)")
        B, N, d = x.shape
        tt, sd = self._t64(t, B), self._t64(seeds, B)
        ws = self.workspace(B, N, cond.T)
        c, s = self.rope_tables(N)
        self._call_varlen("ditto_p_sample_seeded", self._lengths(speech_lengths, cond, B, N),
                          (self.handle, x.data_ptr(), cond.buf.data_ptr(), tt.data_ptr(), sd.data_ptr()),
                          (int(step) & 0xFFFFFFFF, betas.data_ptr(), alphas.data_ptr(), alphas_cumprod.data_ptr(), B, N, cond.T,
                           c.data_ptr(), s.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), opts)
        return x

    def guided_lengths(self, speech_lengths, cond: TextCond, B: int, N: int, cfg: bool):
        """(speech, text) device int32 [2B] (cfg) or [B] of a guided step, or None for a dense one.  `speech_lengths`: the B
        utterances' (list / tuple / int tensor); under guidance the unconditional half repeats them.  The text lengths are the
        conditioning's own (prepare_text(..., text_lengths=) over [text; null])."""
        nb = 2 * B if cfg else B
        if cond.B != nb:
            raise ValueError(f"the conditioning holds {cond.B} utterances; a guided step of {B} needs {nb}")
        return self._lengths(speech_lengths, cond, B, N, 2 if cfg else 1)

    def _guided_args(self, who, x2, dim, B, a, ce, cz, w, noise, seeds):
        """The checks of both guided steps: the state x2 ([x; x] under guidance: w given), noise / seeds, the fp32 [B]
        coefficients.  Returns (seeds as int64 [B], noise as fp32 of x2's first half), each None when not given."""
        if not (x2.is_cuda and x2.dtype == torch.float32 and x2.is_contiguous() and x2.dim() == dim):
            raise ValueError(f"{who} needs a contiguous fp32 CUDA state tensor of {dim} dimensions (it is updated in place)")
        if noise is not None and seeds is not None:
            raise ValueError("noise and seeds are exclusive")
        if noise is not None:
            noise = self._f32(noise, "noise")
            half = (x2.shape[0] // 2 if w is not None else x2.shape[0], *x2.shape[1:])
            if noise.shape != half:
                raise ValueError(f"noise must have shape {half}")
        for name, v in (("a", a), ("ce", ce), ("cz", cz), ("w", w)):
            if v is not None and not (v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.shape == (B,)):
                raise ValueError(f"{name} must be a contiguous fp32 CUDA tensor of shape [{B}]")
        return (self._t64(seeds, B) if seeds is not None else None), noise

    def guided_step_(self, x2: torch.Tensor, cond: TextCond, t: torch.Tensor, B: int, a: torch.Tensor, ce: torch.Tensor,
                     cz: torch.Tensor, w: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                     seeds: Optional[torch.Tensor] = None, step: int = 0, lengths=None, speech_lengths=None,
                     opts: Optional[hip.CallOpts] = None):
        """One guided strided step IN PLACE on x2 (ditto_guided_step_opts): the forward over x2's 2B (w given: [x; x] x
        [text; null]) or B utterances, then the fused update x' = a x + ce e + cz z with e = w (eps_c - eps_u) + eps_u (or eps),
        written to both halves.  a / ce / cz / w: device fp32 [B]; z from `noise` fp32 [B, N, d], from Philox of `seeds` at tag
        `step`, or none (cz unused).  `lengths`: guided_lengths(...) built once per sampling call (else it is built here from
        `speech_lengths` and the conditioning).  Rows past an utterance's length become 0 in both halves."""
        sd, noise = self._guided_args("guided_step_", x2, 3, B, a, ce, cz, w, noise, seeds)
        cfg = w is not None
        nb, N, d = x2.shape
        if nb != (2 * B if cfg else B):
            raise ValueError(f"x2 holds {nb} utterances; a guided step of {B} needs {2 * B if cfg else B}")
        tt = self._t64(t, nb)
        lens = lengths if lengths is not None else self.guided_lengths(speech_lengths, cond, B, N, cfg)
        ws = self.workspace(nb, N, cond.T)
        c, s = self.rope_tables(N)
        hip.check(hip.call("ditto_guided_step_opts", m=self.handle, x2=x2.data_ptr(), cond=cond.buf.data_ptr(), t=tt.data_ptr(),
                           speech_len=None if lens is None else lens[0].data_ptr(), text_len=None if lens is None else lens[1].data_ptr(),
                           noise=_ptr(noise), seeds=_ptr(sd), step=int(step) & 0xFFFFFFFF, w=_ptr(w), a=a.data_ptr(), ce=ce.data_ptr(),
                           cz=cz.data_ptr(), B=B, N=N, T=cond.T, cfg=int(cfg), rope_cos=c.data_ptr(), rope_sin=s.data_ptr(),
                           workspace=ws.data_ptr(), workspace_bytes=ws.numel(), stream=_stream(),
                           opts=None if opts is None else C.byref(opts)))
        return x2

    def denoise_steps_(self, x: torch.Tensor, cond: TextCond, t_begin: int, t_end: int, noises: Optional[torch.Tensor],
                       betas: torch.Tensor, alphas: torch.Tensor, alphas_cumprod: torch.Tensor,
                       opts: Optional[hip.CallOpts] = None):
        """The sampling loop t_begin .. t_end (inclusive, descending) as ONE library call, in place on x;
        noises fp32 [t_begin - t_end + 1, B, N, d] in execution order."""
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
            raise ValueError("denoise_steps_ needs a contiguous fp32 CUDA state tensor (it is updated in place)")
        B, N, _ = x.shape
        nsteps = t_begin - t_end + 1
        if noises is not None:
            noises = self._f32(noises, "noises")
            if noises.shape != (nsteps, *x.shape):
                raise ValueError(f"noises must have shape {(nsteps, *x.shape)}")
        ws = self.workspace(B, N, cond.T)
        c, s = self.rope_tables(N)
        tt = torch.empty(B, dtype=torch.int64, device=self.device)
        self._call("ditto_denoise_steps", self.handle, x.data_ptr(), cond.buf.data_ptr(), int(t_begin), int(t_end),
                                                    _ptr(noises), betas.data_ptr(), alphas.data_ptr(),
                                                    alphas_cumprod.data_ptr(), B, N, cond.T, c.data_ptr(), s.data_ptr(),
                                                    tt.data_ptr(), ws.data_ptr(), ws.numel(), _stream(), opts=opts)
        return x

    def capture_p_sample(self, x: torch.Tensor, cond: TextCond, t: torch.Tensor, noise: torch.Tensor,
                         betas: torch.Tensor, alphas: torch.Tensor, alphas_cumprod: torch.Tensor,
                         opts: Optional[hip.CallOpts] = None):
        """Capture ONE reverse-diffusion step (the ~122 stream-ordered launches of ditto_p_sample) into a HIP
        graph bound to these exact tensors; returns a StepGraph (which keeps them, the workspace and the
        RoPE tables alive).  Replaying it advances `x` in place using whatever
        `t` and `noise` hold at replay time, so a sampling loop is: fill t, draw noise, graph.replay().
        Worth it when the step is launch-bound (small batches); the library calls neither allocate nor
        synchronise, so they are capturable as they are."""
        for name, v in (("x", x), ("noise", noise)):
            if not (v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous fp32 CUDA tensor")
        if t.dtype != torch.int64 or not t.is_cuda:
            raise ValueError("t must be an int64 CUDA tensor")
        B, N, _ = x.shape
        ws = self.workspace(B, N, cond.T)      # allocate outside the capture
        rope = self.rope_tables(N)
        self.p_sample_(x, cond, t, noise, betas, alphas, alphas_cumprod, opts=opts)   # warm-up (lazy kernel attributes)
        torch.cuda.current_stream().synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.p_sample_(x, cond, t, noise, betas, alphas, alphas_cumprod, opts=opts)
        return StepGraph(self, g, (ws, rope, cond.buf, x, t, noise, betas, alphas, alphas_cumprod, self.arena))

    def block_forward_(self, layer: int, h: torch.Tensor, cond: TextCond, cond_layer: Optional[int] = None,
                       rope: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, taps: Optional[dict] = None):
        """DiT block `layer` in place on the fp32 residual stream h [B,N,d].  `taps` (optional dict) receives the
        stream after the self-attention and after the cross-attention segment ("after_self", "after_cross")."""
        if not (h.is_cuda and h.dtype == torch.float32 and h.is_contiguous()):
            raise ValueError("block_forward_ needs a contiguous fp32 CUDA tensor")
        B, N, _ = h.shape
        ws = self.workspace(B, N, cond.T)
        c, s = rope if rope is not None else self.rope_tables(N)
        ta = tb = None
        if taps is not None:
            ta, tb = torch.empty_like(h), torch.empty_like(h)
            taps.update(after_self=ta, after_cross=tb)
        hip.check(self.lib.ditto_block_forward_taps(self.handle, layer, h.data_ptr(), cond.buf.data_ptr(),
                                                    layer if cond_layer is None else cond_layer, B, N, cond.T,
                                                    c.data_ptr(), s.data_ptr(), _ptr(ta), _ptr(tb), ws.data_ptr(),
                                                    ws.numel(), _stream()))
        return h

    # ------------------------------------------------------------------ training
    def train_attach(self, state: Mapping[str, torch.Tensor]):
        """Pack the transposed weight copies the dgrad GEMMs read (after every weight change)."""
        nb = self.lib.ditto_train_arena_bytes(C.byref(self._ccfg))
        if getattr(self, "_train_arena", None) is None:
            self._train_arena = torch.empty(nb, dtype=torch.uint8, device=self.device)
            self._tapes = {}
            self._train_ws = None
        w, keep = self._struct(state)
        hip.check(self.lib.ditto_train_attach(self.handle, C.byref(w), self._train_arena.data_ptr(), nb, _stream()))
        torch.cuda.current_stream().synchronize()
        self._train_attached = True

    def _require_attached(self):
        if not getattr(self, "_train_attached", False):
            raise RuntimeError("train_attach() has not been called for the current weights")

    # the two tape pools differ on purpose (tests assert both): a padded tape is pooled by its shape (B, N, T) and keeps its record in
    # the handle when released; a packed tape is pooled by capacity and its record is forgotten on release
    def _take_tape(self, B, N, T):
        need = self.lib.ditto_tape_bytes(C.byref(self._ccfg), B, N, T)
        pool = self._tapes.setdefault((B, N, T), [])
        return pool.pop() if pool else torch.empty(need, dtype=torch.uint8, device=self.device)

    def release_tape(self, tape, B, N, T):
        self._tapes.setdefault((B, N, T), []).append(tape)

    # ---- packed variable-length batches: x [S, d], text [S_T, text_dim], utterance b in rows [cu[b], cu[b+1]) of each.  S and S_T differ
    # every step, so tapes and the workspace are pooled by CAPACITY (bytes), not by shape: after the largest batch has been seen a step
    # takes a tape that is large enough and allocates no device memory
    def _take_tape_packed(self, need: int):
        """the smallest free tape of at least `need` bytes; when none fits, the largest free one is dropped for a new one (the loop of
        one forward, one backward converges on ONE tape of the largest size; several forwards outstanding at growing sizes keep
        allocating until each has its own)"""
        pool = self._tapes.setdefault("packed", [])
        fit = [i for i, tp in enumerate(pool) if tp.numel() >= need]
        if fit:
            return pool.pop(min(fit, key=lambda i: pool[i].numel()))
        if pool:   # every free tape is too small: the largest one makes room for its replacement
            big = pool.pop(max(range(len(pool)), key=lambda i: pool[i].numel()))
            hip.check(self.lib.ditto_train_tape_forget(self.handle, big.data_ptr()))
            del big
        return torch.empty(need, dtype=torch.uint8, device=self.device)

    def release_tape_packed(self, tape):
        """the tape's backward is done (or will never run): its record leaves the handle, the buffer returns to the pool"""
        hip.check(self.lib.ditto_train_tape_forget(self.handle, tape.data_ptr()))
        self._tapes.setdefault("packed", []).append(tape)

    def _rope_tables_cap(self, N: int):
        """RoPE tables of at least N rows (row i = position i, whatever the table's length): grown, never shrunk"""
        cur = getattr(self, "_rope_cap", None)
        if cur is None or cur[0].shape[0] < N or cur[2] != self._generation:
            c, s = self.rope_tables(N)
            self._rope_cap = (c, s, self._generation)
        return self._rope_cap[0], self._rope_cap[1]

    def train_forward_packed(self, x, cu_seqlens, text_emb, text_cu_seqlens, t, dropout_p: float, seed: int,
                             max_seqlen: Optional[int] = None, max_text_seqlen: Optional[int] = None,
                             opts: Optional[hip.CallOpts] = None):
        """The training forward over a packed batch (ditto_train_forward_packed_opts): returns (eps fp32 [S, d], state) where
        `state` carries what train_backward_packed needs (tape, inputs, offsets).  Utterance b's rows of eps are what train_forward
        gives for it alone."""
        require_fused_attention(self.cfg, "packed batches")
        self._require_attached()
        xf, text = self._f32(x, "x"), self._f32(text_emb, "text_emb")
        if xf.dim() != 2 or xf.shape[1] != self.cfg.hidden_dim:
            raise ValueError(f"x: [S, {self.cfg.hidden_dim}] expected, got {list(xf.shape)}")
        if text.dim() != 2 or text.shape[1] != self.cfg.text_dim:
            raise ValueError(f"text_emb: [S_T, {self.cfg.text_dim}] expected, got {list(text.shape)}")
        S, S_T = int(xf.shape[0]), int(text.shape[0])
        B = len(cu_seqlens) - 1
        if len(text_cu_seqlens) - 1 != B:
            raise ValueError("cu_seqlens and text_cu_seqlens describe different numbers of utterances")
        cu, max_N = self._cu(cu_seqlens, B, S, max_seqlen, "cu_seqlens")
        ct, max_T = self._cu(text_cu_seqlens, B, S_T, max_text_seqlen, "text_cu_seqlens")
        tt = self._t64(t, B)
        need = self.lib.ditto_tape_bytes_packed(C.byref(self._ccfg), B, S, S_T)
        if need == 0:
            raise hip.DittoHipError(hip.ERR_SHAPE, self.lib.ditto_last_error().decode())
        ws = self._grow_ws(self.lib.ditto_train_workspace_bytes_packed(C.byref(self._ccfg), B, S, max_N, S_T, max_T), "_train_ws")
        tape = self._take_tape_packed(need)
        c, s = self._rope_tables_cap(max_N)
        cud, ctd = cu.to(self.device), ct.to(self.device)
        out = torch.empty_like(xf)
        try:
            hip.check(self.lib.ditto_train_forward_packed_opts(
                self.handle, xf.data_ptr(), text.data_ptr(), tt.data_ptr(), cud.data_ptr(), ctd.data_ptr(), B, S, max_N, S_T, max_T,
                c.data_ptr(), s.data_ptr(), float(dropout_p), int(seed), out.data_ptr(), tape.data_ptr(), tape.numel(), ws.data_ptr(),
                ws.numel(), _stream(), None if opts is None else C.byref(opts)))
        except BaseException:
            self.release_tape_packed(tape)
            raise
        state = dict(tape=tape, xf=xf, tt=tt, cu=cud, cu_t=ctd, B=B, S=S, S_T=S_T, max_N=max_N, max_T=max_T, rope=(c, s),
                     dropout_p=float(dropout_p), seed=int(seed))
        return out, state

    def train_backward_packed(self, state: Mapping[str, torch.Tensor], grad_eps, st, opts: Optional[hip.CallOpts] = None,
                              piece_cb=None, layers_per_piece: int = 1, text_grad: bool = False) -> Dict[str, torch.Tensor]:
        """Backward of train_forward_packed (`st`: its second result): fp32 gradients keyed by the reference state_dict names.
        `piece_cb`: as train_backward — pieces of `layers_per_piece` layers, top first (ditto_train_backward_packed_layers),
        bit-identical to the single call.
        `text_grad`: the gradient with respect to the text rows too, fp32 [S_T, text_dim] under the key TEXT_GRAD_KEY
        (ditto_train_backward_packed_text_layers: the same parameter gradients, bit for bit; it is no piece of `piece_cb`'s).
        False: the call as it was — the same entry, workspace and launches."""
        g = self._f32(grad_eps, "grad_output")
        if tuple(g.shape) != (st["S"], self.cfg.hidden_dim):
            raise ValueError(f"grad_output: [{st['S']}, {self.cfg.hidden_dim}] expected, got {list(g.shape)}")
        size = self.lib.ditto_train_workspace_bytes_packed_text if text_grad else self.lib.ditto_train_workspace_bytes_packed
        ws = self._grow_ws(size(C.byref(self._ccfg), st["B"], st["S"], st["max_N"], st["S_T"], st["max_T"]), "_train_ws")
        c, s = st["rope"]
        tape = st["tape"]
        d_text = torch.empty(st["S_T"], self.cfg.text_dim, dtype=torch.float32, device=self.device) if text_grad else None
        grads = self._train_backward(
            state, None, "ditto_train_backward_packed_text_layers" if text_grad else "ditto_train_backward_packed_layers", g,
            (st["xf"].data_ptr(), st["tt"].data_ptr(), st["cu"].data_ptr(), st["cu_t"].data_ptr(), st["B"], st["S"], st["max_N"],
             st["S_T"], st["max_T"], c.data_ptr(), s.data_ptr(), st["dropout_p"], st["seed"], tape.data_ptr(), tape.numel()),
            ws, opts, piece_cb, layers_per_piece, after=(d_text.data_ptr(), d_text.numel() * 4) if text_grad else ())
        if text_grad:
            grads[TEXT_GRAD_KEY] = d_text
        return grads

    # ---- condition dropout (classifier-free guidance training): every utterance's text is its own rows or the null embedding's
    def text_select_packed(self, text: torch.Tensor, null_rows: torch.Tensor, table: torch.Tensor, S_out: int):
        """ditto_text_select_packed: text fp32 [S_T, dt], null_rows fp32 [T0, dt], `table` CPU int32 [3B + 2]
        (varlen.cond_dropout_layout) -> (text_eff fp32 [S_out, dt], the table on the device, for the backward)."""
        B = (int(table.numel()) - 2) // 3
        tdev = table.to(self.device)
        out = torch.empty(S_out, text.shape[1], dtype=torch.float32, device=self.device)
        hip.check(hip.call("ditto_text_select_packed", text=text.data_ptr(), text_bytes=text.numel() * 4, null_rows=null_rows.data_ptr(),
                           null_rows_bytes=null_rows.numel() * 4, table=tdev.data_ptr(), table_bytes=tdev.numel() * 4,
                           table_host=table.data_ptr(), table_host_bytes=table.numel() * 4, text_eff=out.data_ptr(),
                           text_eff_bytes=out.numel() * 4, B=B, S_T=int(text.shape[0]), S_out=int(S_out), T0=int(null_rows.shape[0]),
                           dt=int(text.shape[1]), stream=_stream()))
        return out, tdev

    def text_select_packed_bwd(self, d_text_eff: torch.Tensor, table: torch.Tensor, table_dev: torch.Tensor, S_T: int, T0: int):
        """ditto_text_select_packed_bwd: d_text_eff fp32 [S_out, dt] -> (d_text fp32 [S_T, dt], d_null fp32 [T0, dt])"""
        g = self._f32(d_text_eff, "grad_output")
        B, dt = (int(table.numel()) - 2) // 3, int(g.shape[1])
        d_text = torch.empty(S_T, dt, dtype=torch.float32, device=self.device)
        d_null = torch.empty(T0, dt, dtype=torch.float32, device=self.device)
        hip.check(hip.call("ditto_text_select_packed_bwd", d_text_eff=g.data_ptr(), d_text_eff_bytes=g.numel() * 4,
                           table=table_dev.data_ptr(), table_bytes=table_dev.numel() * 4, table_host=table.data_ptr(),
                           table_host_bytes=table.numel() * 4, d_text=d_text.data_ptr(), d_text_bytes=d_text.numel() * 4,
                           d_null=d_null.data_ptr(), d_null_bytes=d_null.numel() * 4, B=B, S_T=int(S_T), S_out=int(g.shape[0]),
                           T0=int(T0), dt=dt, stream=_stream()))
        return d_text, d_null

    def train_forward(self, x, text_emb, t, dropout_p: float, seed: int, opts: Optional[hip.CallOpts] = None):
        """DiTTO.forward in train mode: returns (eps fp32 [B,N,d], tape).  The library records against the tape how it wrote it
        (bf16 or fp32 stream rows): train_backward reads it that way whatever the options are by then."""
        self._require_attached()
        xf, text = self._f32(x, "x"), self._f32(text_emb, "text_emb")
        B, N, d = xf.shape
        T = text.shape[1]
        if d != self.cfg.hidden_dim or text.shape[0] != B or text.shape[2] != self.cfg.text_dim:
            raise ValueError("x / text_emb shapes do not match the model")
        tt = self._t64(t, B)
        tape = self._take_tape(B, N, T)
        ws = self._grow_ws(self.lib.ditto_train_workspace_bytes(C.byref(self._ccfg), B, N, T), "_train_ws")
        c, s = self.rope_tables(N)
        out = torch.empty_like(xf)
        self._call("ditto_train_forward", self.handle, xf.data_ptr(), text.data_ptr(), tt.data_ptr(), B, N, T,
                                                    c.data_ptr(), s.data_ptr(), float(dropout_p), int(seed), out.data_ptr(),
                                                    tape.data_ptr(), tape.numel(), ws.data_ptr(), ws.numel(), _stream(), opts=opts)
        return out, tape, xf, tt

    def train_backward(self, state: Mapping[str, torch.Tensor], grad_eps, xf, tt, T: int, tape, dropout_p: float,
                       seed: int, opts: Optional[hip.CallOpts] = None, piece_cb=None,
                       layers_per_piece: int = 1) -> Dict[str, torch.Tensor]:
        """Backward of train_forward: fp32 gradients keyed by the reference state_dict names (fresh tensors).

        `piece_cb` (optional): the backward runs in pieces of `layers_per_piece` layers, top layer first
        (ditto_train_backward_layers: bit-identical to the single call), and after each piece is ENQUEUED piece_cb(list of that
        piece's gradient tensors) is called — dist.GradSync.reduce starts their data-parallel exchange on a side stream while
        the layers below are still being computed."""
        B, N, d = xf.shape
        g = self._f32(grad_eps, "grad_output")
        if g.shape != xf.shape:
            raise ValueError(f"grad_output: {list(xf.shape)} expected, got {list(g.shape)}")
        ws = self._grow_ws(self.lib.ditto_train_workspace_bytes(C.byref(self._ccfg), B, N, T), "_train_ws")
        c, s = self.rope_tables(N)
        return self._train_backward(
            state, "ditto_train_backward", "ditto_train_backward_layers", g,
            (xf.data_ptr(), tt.data_ptr(), B, N, T, c.data_ptr(), s.data_ptr(), float(dropout_p), int(seed), tape.data_ptr(),
             tape.numel()), ws, opts, piece_cb, layers_per_piece)

    def _train_backward(self, state, plain, layers, g, mid, ws, opts, piece_cb, layers_per_piece, after=()):
        """The backward of either layout.  `plain`: the name of the whole backward's entry (through _call; None: the layers entry
        over every layer), `layers`: the name of the entry that takes a layer range, `mid`: the layout's own arguments, between
        grad_output and the gradient struct, `after`: the entry's arguments behind the layer range (the text gradient's buffer)."""
        L = self.cfg.num_layers
        w, keep = self._struct(state)
        no_grad = ("rotary_inv_freq",)
        keys = [f"blocks.{l}.{k}" for l in range(L) for k in hip.LAYER_KEY.values()] + \
               [k for f, k in hip.GLOBAL_KEY.items() if f not in no_grad]
        # one tensor of its own per parameter (the allocator aligns to 512 B): autograd's AccumulateGrad takes such a
        # gradient over as .grad without a copy; views of one flat buffer cost a copy kernel per parameter per step
        grads = {k: torch.empty(state[k].shape, dtype=torch.float32, device=self.device) for k in keys}
        gs, gkeep = self._struct(grads, lambda k: grads[k].data_ptr(), skip=no_grad)
        args = (self.handle, C.byref(w), g.data_ptr(), *mid, C.byref(gs), ws.data_ptr(), ws.numel(), _stream())
        o = None if opts is None else C.byref(opts)
        if piece_cb is None or not hip._has_call_opts():
            if plain is not None:
                self._call(plain, *args, opts=opts)
            else:
                hip.check(getattr(self.lib, layers)(*args, o, L - 1, 0, *after))
            if piece_cb is not None:
                # a frozen pre-ABI-9 library (DITTO_HIP_LIB) has no entry that takes a layer range: one call, then every tensor as
                # one piece (the caller's exchange then simply runs after the backward instead of under it)
                piece_cb(list(grads.values()))
            return grads
        head = ("proj_in.weight", "proj_in.bias", "proj_out.weight", "proj_out.bias")     # written by the piece that starts at the top
        tail = [k for k in keys[L * len(hip.LAYER_KEY):] if k not in head]                # ... that ends at layer 0
        step = max(int(layers_per_piece), 1)
        hi = L - 1
        while hi >= 0:
            lo = max(hi - step + 1, 0)
            hip.check(getattr(self.lib, layers)(*args, o, hi, lo, *after))
            piece = [grads[k] for k in head] if hi == L - 1 else []
            piece += [grads[f"blocks.{l}.{k}"] for l in range(hi, lo - 1, -1) for k in hip.LAYER_KEY.values()]
            if lo == 0:
                piece += [grads[k] for k in tail]
            piece_cb(piece)
            hi = lo - 1
        return grads

    # ------------------------------------------------------------------ profiling (bench.py)
    def profile_enable(self, on: bool):
        hip.check(self.lib.ditto_profile_enable(self.handle, 1 if on else 0))

    def profile_read(self):
        n = (C.c_int32 * hip.KC_COUNT)()
        ms = (C.c_float * hip.KC_COUNT)()
        hip.check(self.lib.ditto_profile_read(self.handle, n, ms))
        return {hip.KERNEL_CLASSES[i]: (int(n[i]), float(ms[i])) for i in range(hip.KC_COUNT)}
