"""The fused training optimizer: torch.optim.AdamW's update with gradient clipping by global norm, an on-device skip of a step whose
gradient norm is not finite, and an exponential moving average (EMA) of the weights — csrc/optim.hip through include/ditto_optim.h,
three launches a step (one when neither clipping nor skipping is asked for).

    opt = ditto_tts_amd.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-2, max_norm=1.0, skip_nonfinite=True,
                                    ema_decay=0.9999)
    loss.backward(); opt.step(); opt.zero_grad()
    with opt.ema_weights():            # sample from the average; the trained weights come back on exit
        ...

The constructor is the reference trainer's (`self.optimizer(self.model.parameters(), lr=..., weight_decay=...)`, src/utils/Trainer.py:69);
the reference itself has neither clipping nor an EMA.  There is no fallback: without libditto_hip.so's entries step() raises.

step() covers the parameters whose .grad is not None.  It builds the segment table on the host (the gradient tensors are fresh every
backward), uploads it with one asynchronous copy from pinned memory and enqueues the launches on the current stream: no host
synchronisation, and after the first step no device allocation.  Whether a step was skipped is decided and acted on by the device; the
host learns of it only by reading `skipped_steps`.  The parameters' version counters are bumped (torch.autograd.graph.increment_version),
so DiTTO repacks its weights on the next forward by itself — also after a skipped step, which costs a repack and changes nothing.
All covered parameters share ONE step count (the state block's); a state dict whose per-parameter steps differ is refused.
"""
from __future__ import annotations

import contextlib
import math
import struct

import numpy as np
import torch

from . import hip

STATE_KEYS = ("step", "exp_avg", "exp_avg_sq")      # torch.optim.AdamW's per-parameter state, in its order
EMA_KEY = "ema"                                     # ours, beside them
SEG_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("ema", "<u8"), ("n", "<u8"), ("slot0", "<u4"),
                      ("reserved", "<u4"), ("lr", "<f8"), ("weight_decay", "<f8")])       # ditto_optim_seg
assert SEG_DTYPE.itemsize == 72
MAX_SEGS = 65535


def chunk_bases(sizes):
    """(slot0 of every segment, n_chunks) for segments of `sizes` elements: slot0 = the chunks of the segments in front"""
    slots, total = [], 0
    for n in sizes:
        if int(n) < 1:
            raise ValueError(f"a segment of {n} elements")
        slots.append(total)
        total += hip.optim_chunks(n)
    return slots, total


def fill_table(rows: np.ndarray, ptrs, sizes, lrs, wds):
    """Write the table of len(sizes) segments into the SEG_DTYPE array `rows`; ptrs: (p, g, m, v, ema) address lists (0 = NULL).
    -> n_chunks"""
    slots, total = chunk_bases(sizes)
    k = len(sizes)
    for name, col in zip(("p", "g", "m", "v", "ema"), ptrs):
        rows[name][:k] = col
    rows["n"][:k] = sizes
    rows["slot0"][:k] = slots
    rows["reserved"][:k] = 0
    rows["lr"][:k] = lrs
    rows["weight_decay"][:k] = wds
    return total


def state_block(beta1: float, beta2: float, step: int, skipped: int = 0) -> bytes:
    """ditto_optim_state of an optimizer that has applied `step` steps: beta^step as the device forms it, a running fp64 product"""
    p1 = p2 = 1.0
    for _ in range(int(step)):
        p1 *= beta1
        p2 *= beta2
    slot = struct.pack("<ddqq", p1, p2, int(step), int(skipped))
    return slot + slot + struct.pack("<dffi", 0.0, 0.0, 1.0, 0) + bytes(44)


def new_state(p: torch.Tensor, ema: bool) -> dict:
    """the state of a parameter before its first step: torch.optim.AdamW's keys (+ the average, which starts at the weights)"""
    st = {"step": torch.tensor(0.0), "exp_avg": torch.zeros_like(p, memory_format=torch.contiguous_format),
          "exp_avg_sq": torch.zeros_like(p, memory_format=torch.contiguous_format)}
    if ema:
        st[EMA_KEY] = p.detach().clone(memory_format=torch.contiguous_format)
    return st


class _Staging:
    """Pinned host tables with the event of their last upload: a table is reused only once its copy has run."""

    def __init__(self):
        self.bufs = []

    def take(self, nbytes: int):
        for entry in self.bufs:
            if entry[0].numel() >= nbytes and entry[1].query():
                return entry
        entry = [torch.empty(max(nbytes, 4096), dtype=torch.uint8).pin_memory(), torch.cuda.Event()]
        self.bufs.append(entry)
        return entry


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW's arguments and defaults; keyword-only: max_norm (clip the global gradient norm, None = off),
    skip_nonfinite (leave a step with a non-finite gradient norm out, on the device), ema_decay (keep an average of the weights, None =
    off).  Parameter groups carry their own lr and weight_decay (LR schedulers work unchanged); betas and eps are shared."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, max_norm=None, skip_nonfinite=False,
                 ema_decay=None, amsgrad=False, maximize=False):
        if not (isinstance(betas, (tuple, list)) and len(betas) == 2 and all(0.0 <= float(b) < 1.0 for b in betas)):
            raise ValueError(f"betas {betas!r}: two numbers in [0, 1)")
        if not (math.isfinite(float(eps)) and float(eps) >= 0.0):
            raise ValueError(f"eps {eps!r}: a finite number >= 0")
        if max_norm is not None and not (math.isfinite(float(max_norm)) and float(max_norm) > 0.0):
            raise ValueError(f"max_norm {max_norm!r}: a finite number > 0, or None")
        if ema_decay is not None and not (0.0 <= float(ema_decay) <= 1.0):
            raise ValueError(f"ema_decay {ema_decay!r}: a number in [0, 1], or None")
        self.max_norm = None if max_norm is None else float(max_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self._device = None
        super().__init__(params, dict(lr=lr, betas=tuple(float(b) for b in betas), eps=float(eps), weight_decay=weight_decay,
                                      amsgrad=amsgrad, maximize=maximize))
        self._check_groups()
        self._calls = 0                  # the phase of the next step (include/ditto_optim.h)
        self._staging = _Staging()
        self._table = None               # device uint8: the uploaded table
        self._scratch = None             # device: one fp64 partial per chunk
        self._cache_key, self._cache = None, None
        self._hyper = hip.OptimHyper(*self.param_groups[0]["betas"], self.param_groups[0]["eps"], self.max_norm or 0.0,
                                     self.ema_decay if self.ema_decay is not None else 0.0, int(self.skip_nonfinite), 0)
        self._dev = torch.empty(hip.OPTIM_STATE_BYTES, dtype=torch.uint8, device=self._device)
        self._write_state(0, 0)

    # ------------------------------------------------------------------ checks
    def _check_groups(self):
        g0 = self.param_groups[0]
        for gi, group in enumerate(self.param_groups):
            for flag in ("amsgrad", "maximize"):
                if group.get(flag, False):
                    raise ValueError(f"{flag}=True is not supported by ditto_tts_amd.optim.AdamW (parameter group {gi})")
            if tuple(group["betas"]) != tuple(g0["betas"]) or float(group["eps"]) != float(g0["eps"]):
                raise ValueError(f"parameter group {gi}: betas {group['betas']} / eps {group['eps']} differ from group 0's "
                                 f"{g0['betas']} / {g0['eps']}; only lr and weight_decay may differ between groups")
            for flag in ("lr", "weight_decay"):
                v = float(group[flag])
                if not math.isfinite(v) or v < 0.0:
                    raise ValueError(f"parameter group {gi}: {flag} {group[flag]!r} is negative or not finite")
        for gi, group in enumerate(self.param_groups):
            names = group.get("param_names")
            for pi, p in enumerate(group["params"]):
                who = f"parameter {names[pi]!r}" if names else f"parameter {pi} of group {gi} (shape {tuple(p.shape)})"
                if p.dtype != torch.float32:
                    raise ValueError(f"{who}: dtype {p.dtype}, the fused optimizer updates fp32 parameters only")
                if p.device.type != "cuda":
                    raise ValueError(f"{who}: on {p.device}, the fused optimizer has no CPU path (move the model to the GPU first)")
                if self._device is None:
                    self._device = p.device
                if p.device != self._device:
                    raise ValueError(f"{who}: on {p.device}, the other parameters are on {self._device}")
                if not p.is_contiguous() or p.data_ptr() % 16 or p.numel() < 1:
                    raise ValueError(f"{who}: not contiguous, not 16-byte aligned or empty")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_calls"):
            self._check_groups()
            self._cache_key = None

    # ------------------------------------------------------------------ the device state block
    def _write_state(self, step: int, skipped: int):
        b1, b2 = self.param_groups[0]["betas"]
        host = torch.frombuffer(bytearray(state_block(b1, b2, step, skipped)), dtype=torch.uint8)
        self._dev.copy_(host)
        self._f32, self._i64 = self._dev.view(torch.float32), self._dev.view(torch.int64)

    @property
    def grad_norm(self) -> torch.Tensor:
        """the global gradient norm of the last step, before clipping (device fp32 scalar; reading it synchronises)"""
        return self._f32[hip.OPTIM_STATE_NORM32 // 4]

    @property
    def clip_coef(self) -> torch.Tensor:
        """the factor the last step's gradients were multiplied by (device fp32 scalar; 1 when nothing was clipped)"""
        return self._f32[hip.OPTIM_STATE_CLIP // 4]

    @property
    def skipped_steps(self) -> torch.Tensor:
        """how many steps were skipped for a non-finite gradient norm (device int64 scalar)"""
        return self._i64[(self._calls & 1) * 4 + 3]

    @property
    def steps_applied(self) -> torch.Tensor:
        """how many steps were applied (device int64 scalar)"""
        return self._i64[(self._calls & 1) * 4 + 2]

    # ------------------------------------------------------------------ the table
    def _covered(self, need_grad: bool):
        ps, lrs, wds = [], [], []
        for group in self.param_groups:
            lr, wd = float(group["lr"]), float(group["weight_decay"])
            for p in group["params"]:
                if need_grad and p.grad is None:
                    continue
                if not need_grad and EMA_KEY not in self.state.get(p, ()):
                    continue
                ps.append(p), lrs.append(lr), wds.append(wd)
        return ps, lrs, wds

    def _upload(self, ps, grads, lrs, wds, with_ema: bool):
        """the table of `ps` on the device (one async copy) -> (device address, n_seg, n_chunks)"""
        if len(ps) > MAX_SEGS:
            raise ValueError(f"{len(ps)} parameter tensors: the table holds {MAX_SEGS}")
        key = (tuple(id(p) for p in ps), with_ema)
        if key != self._cache_key:          # what does not change from step to step: addresses of p, m, v, ema, sizes, chunk bases
            st = [self.state[p] for p in ps]
            self._cache = ([p.data_ptr() for p in ps], [s["exp_avg"].data_ptr() for s in st], [s["exp_avg_sq"].data_ptr() for s in st],
                           [s[EMA_KEY].data_ptr() if with_ema and EMA_KEY in s else 0 for s in st], [p.numel() for p in ps])
            self._cache_key = key
        pp, mp, vp, ep, sizes = self._cache
        nbytes = len(ps) * SEG_DTYPE.itemsize
        entry = self._staging.take(nbytes)
        rows = entry[0].numpy()[:nbytes].view(SEG_DTYPE)
        n_chunks = fill_table(rows, (pp, grads, mp, vp, ep), sizes, lrs, wds)
        if self._table is None or self._table.numel() < nbytes:
            self._table = torch.empty(max(nbytes, 4096), dtype=torch.uint8, device=self._device)
        self._table[:nbytes].copy_(entry[0][:nbytes], non_blocking=True)
        entry[1].record()
        return self._table.data_ptr(), len(ps), n_chunks

    def _stream(self):
        return torch.cuda.current_stream(self._device).cuda_stream

    # ------------------------------------------------------------------ step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ps, lrs, wds = self._covered(need_grad=True)
        if not ps:
            return loss
        grads = []
        for p in ps:
            g = p.grad
            if g.is_sparse or g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous() or g.data_ptr() % 16:
                raise ValueError(f"the gradient of a parameter of shape {tuple(p.shape)} is sparse, not fp32, not contiguous, not "
                                 "16-byte aligned or on another device")
            if p not in self.state or not self.state[p]:
                self.state[p] = new_state(p, self.ema_decay is not None)
                self._cache_key = None
            elif self.ema_decay is not None and EMA_KEY not in self.state[p]:      # a state loaded from torch.optim.AdamW
                self.state[p][EMA_KEY] = p.detach().clone(memory_format=torch.contiguous_format)
                self._cache_key = None
            grads.append(g.data_ptr())
        with torch.cuda.device(self._device):
            table, n_seg, n_chunks = self._upload(ps, grads, lrs, wds, self.ema_decay is not None)
            normed = self.max_norm is not None or self.skip_nonfinite
            if normed and (self._scratch is None or self._scratch.numel() < n_chunks):
                self._scratch = torch.empty(hip.lib().ditto_optim_scratch_bytes(n_chunks) // 8, dtype=torch.float64, device=self._device)
            hip.check(hip.call("ditto_optim_adamw_step", table=table, n_seg=n_seg, n_chunks=n_chunks, hyper=self._hyper,
                               state=self._dev.data_ptr(), phase=self._calls & 1,
                               scratch=self._scratch.data_ptr() if normed else None,
                               scratch_bytes=self._scratch.numel() * 8 if normed else 0, grid_limit=0, stream=self._stream()))
        self._calls += 1
        torch.autograd.graph.increment_version(ps)      # the update is in place: DiTTO's _ParamWatch and autograd's checks see it
        return loss

    # ------------------------------------------------------------------ the average
    def _swap(self):
        ps, lrs, wds = self._covered(need_grad=False)
        if not ps:
            raise RuntimeError("no averaged weights yet: ema_decay is None, or no step has run")
        with torch.cuda.device(self._device):
            table, n_seg, n_chunks = self._upload(ps, [0] * len(ps), lrs, wds, True)
            hip.check(hip.call("ditto_optim_swap", table=table, n_seg=n_seg, n_chunks=n_chunks, grid_limit=0, stream=self._stream()))
        torch.autograd.graph.increment_version(ps)

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the parameters hold the averaged weights (and the EMA buffers the trained ones): one bit-exact exchange on
        entry, one on exit — also when the block raises.  No step() inside."""
        self._swap()
        try:
            yield self
        finally:
            self._swap()

    def ema_state_dict(self, model: torch.nn.Module) -> dict:
        """`model.state_dict()` as clones, with the averaged weights in place of every parameter that has an average (the others —
        frozen ones, those that never get a gradient — as they are): loadable with load_state_dict."""
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        for name, p in model.named_parameters():
            st = self.state.get(p)
            if st and EMA_KEY in st and name in sd:
                sd[name] = st[EMA_KEY].detach().clone()
        return sd

    # ------------------------------------------------------------------ state dict
    def state_dict(self):
        """torch.optim.AdamW's layout: per parameter `step` (the shared count, read from the device: this synchronises), `exp_avg`,
        `exp_avg_sq`, and `ema` where an average is kept; beside "state" and "param_groups" the count of skipped steps."""
        step, skipped = int(self.steps_applied.item()), int(self.skipped_steps.item())
        for st in self.state.values():
            if st:
                st["step"] = torch.tensor(float(step))
        sd = super().state_dict()
        sd["skipped_steps"] = skipped
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._check_groups()
        steps = {int(float(st["step"])) for st in self.state.values() if st}
        if len(steps) > 1:
            raise ValueError(f"per-parameter step counts {sorted(steps)} differ: the fused optimizer keeps one count for all parameters")
        for p, st in self.state.items():
            for k in ("exp_avg", "exp_avg_sq", EMA_KEY):
                if k in st:
                    st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous()
        g0 = self.param_groups[0]
        self._hyper.beta1, self._hyper.beta2, self._hyper.eps = g0["betas"][0], g0["betas"][1], g0["eps"]
        self._write_state(steps.pop() if steps else 0, int(state_dict.get("skipped_steps", 0)))
        self._calls = 0
        self._cache_key = None
