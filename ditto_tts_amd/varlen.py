"""Variable-length batches: per-utterance query / key lengths in the padded layout (include/ditto_hip.h, the *_varlen_* entries).

Utterance b owns rows [0, len[b]) of its padded [Sq] / [Skv] block; the rows past them are padding, never read and never written.
The library takes the lengths as device int32 [B] and cannot check them without a sync, so they are validated here, on the host,
before they go to the device.
"""
from __future__ import annotations

import torch

from . import hip


def validate_lengths(lengths, B: int, maxlen: int, name: str = "lengths") -> torch.Tensor:
    """`lengths` (list / tuple of ints, or an integer tensor on any device) as a CPU int32 tensor of shape [B], every value in
    [1, maxlen].  Anything else raises ValueError."""
    if isinstance(lengths, torch.Tensor):
        if lengths.dtype.is_floating_point or lengths.dtype.is_complex or lengths.dtype == torch.bool:
            raise ValueError(f"{name}: an integer tensor is needed, got {lengths.dtype}")
        t = lengths.detach().to("cpu", torch.int64)
    elif isinstance(lengths, (list, tuple)):
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in lengths):
            raise ValueError(f"{name}: a list / tuple of ints is needed")
        t = torch.tensor(list(lengths), dtype=torch.int64)
    else:
        raise ValueError(f"{name}: a list, tuple or integer tensor is needed, got {type(lengths).__name__}")
    if t.dim() != 1 or t.shape[0] != B:
        raise ValueError(f"{name}: shape [{B}] expected, got {list(t.shape)}")
    if B and (int(t.min()) < 1 or int(t.max()) > maxlen):
        raise ValueError(f"{name}: every length must lie in [1, {maxlen}], got [{int(t.min())}, {int(t.max())}]")
    return t.to(torch.int32)


def validate_prompt_lengths(prompt_lengths, cu, name: str = "prompt_lengths") -> torch.Tensor:
    """Speech-prompt lengths of a packed batch: `prompt_lengths` (list / tuple of ints, or an integer tensor) as a CPU int32 tensor
    [B] with 0 <= P_b < N_b (N_b from the validated offsets `cu` [B + 1]: at least one row of every utterance is generated).
    Anything else raises ValueError naming the utterance."""
    B = len(cu) - 1
    if isinstance(prompt_lengths, torch.Tensor):
        if prompt_lengths.dtype.is_floating_point or prompt_lengths.dtype.is_complex or prompt_lengths.dtype == torch.bool:
            raise ValueError(f"{name}: an integer tensor is needed, got {prompt_lengths.dtype}")
        t = prompt_lengths.detach().to("cpu", torch.int64)
    elif isinstance(prompt_lengths, (list, tuple)):
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in prompt_lengths):
            raise ValueError(f"{name}: a list / tuple of ints is needed")
        t = torch.tensor(list(prompt_lengths), dtype=torch.int64)
    else:
        raise ValueError(f"{name}: a list, tuple or integer tensor is needed, got {type(prompt_lengths).__name__}")
    if t.dim() != 1 or t.shape[0] != B:
        raise ValueError(f"{name}: shape [{B}] expected, got {list(t.shape)}")
    n = torch.as_tensor(cu).detach().to("cpu", torch.int64)
    n = n[1:] - n[:-1]
    bad = torch.nonzero((t < 0) | (t >= n)).reshape(-1)
    if bad.numel():
        b = int(bad[0])
        raise ValueError(f"{name}: utterance {b} has {int(n[b])} rows, its prompt must hold 0 .. {int(n[b]) - 1} of them, got {int(t[b])}")
    return t.to(torch.int32)


def validate_suffix_lengths(suffix_lengths, cu, prompt_lengths=None, name: str = "suffix_lengths") -> torch.Tensor:
    """Suffix-context lengths of a packed batch (speech infilling): `suffix_lengths` (list / tuple of ints, or an integer tensor) as a
    CPU int32 tensor [B] with Q_b >= 0 and P_b + Q_b <= N_b - 1 (N_b from the validated offsets `cu` [B + 1], P_b from the validated
    `prompt_lengths`, None: 0 — at least one row of every utterance is generated).  Anything else raises ValueError naming the
    utterance."""
    B = len(cu) - 1
    if isinstance(suffix_lengths, torch.Tensor):
        if suffix_lengths.dtype.is_floating_point or suffix_lengths.dtype.is_complex or suffix_lengths.dtype == torch.bool:
            raise ValueError(f"{name}: an integer tensor is needed, got {suffix_lengths.dtype}")
        t = suffix_lengths.detach().to("cpu", torch.int64)
    elif isinstance(suffix_lengths, (list, tuple)):
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in suffix_lengths):
            raise ValueError(f"{name}: a list / tuple of ints is needed")
        t = torch.tensor(list(suffix_lengths), dtype=torch.int64)
    else:
        raise ValueError(f"{name}: a list, tuple or integer tensor is needed, got {type(suffix_lengths).__name__}")
    if t.dim() != 1 or t.shape[0] != B:
        raise ValueError(f"{name}: shape [{B}] expected, got {list(t.shape)}")
    n = torch.as_tensor(cu).detach().to("cpu", torch.int64)
    n = n[1:] - n[:-1]
    p = torch.zeros(B, dtype=torch.int64) if prompt_lengths is None else validate_prompt_lengths(prompt_lengths, cu).to(torch.int64)
    bad = torch.nonzero((t < 0) | (p + t > n - 1)).reshape(-1)
    if bad.numel():
        b = int(bad[0])
        raise ValueError(f"{name}: utterance {b} has {int(n[b])} rows and a prompt of {int(p[b])}, its suffix must hold 0 .. "
                         f"{int(n[b]) - 1 - int(p[b])} of them, got {int(t[b])}")
    return t.to(torch.int32)


def _dev_lengths(lengths, B, maxlen, name, device):
    if lengths is None:
        return None
    return validate_lengths(lengths, B, maxlen, name).to(device)


def _check_qkv(q, k, v, H):
    for n, x in (("q", q), ("k", k), ("v", v)):
        if x.dtype != torch.bfloat16 or x.dim() != 3 or not x.is_cuda or x.stride(2) != 1 or x.stride(0) != x.shape[1] * x.stride(1):
            raise ValueError(f"{n}: a bf16 [B, S, H * 64] tensor on the GPU with unit column stride is needed")
        if x.shape[2] < H * 64:
            raise ValueError(f"{n}: {x.shape[2]} columns do not hold {H} heads of 64")


def _check_batch(q, k, v, H):
    """q [B, Sq, .], k / v [B, Skv, .]: the kernels address all three with q's B and k's Skv"""
    if k.shape[0] != q.shape[0] or v.shape[0] != q.shape[0] or v.shape[1] != k.shape[1]:
        raise ValueError(f"q {list(q.shape)}, k {list(k.shape)}, v {list(v.shape)}: k and v need q's batch and one common length")
    if not (q.device == k.device == v.device):
        raise ValueError("q, k and v must be on one device")


def _check_out(t, name, B, Sq, H, dtypes, device):
    if (t.dtype not in dtypes or t.device != device or t.dim() != 3 or t.shape[0] != B or t.shape[1] != Sq or t.shape[2] < H * 64
            or t.stride(2) != 1 or t.stride(0) != Sq * t.stride(1)):
        raise ValueError(f"{name}: a {' / '.join(str(d) for d in dtypes)} [{B}, {Sq}, >= {H * 64}] tensor with unit column stride on "
                         f"{device} is needed, got {t.dtype} {list(t.shape)} on {t.device}")


def _attention(q, k, v, H, q_len, kv_len, out=None, resid=None, resid_in=None):
    """attention (resid None: into `out`, allocated when None) and attention_resid (into `resid`): one entry each"""
    _check_qkv(q, k, v, H)
    _check_batch(q, k, v, H)
    B, Sq, Skv = q.shape[0], q.shape[1], k.shape[1]
    if q_len is None and kv_len is None:
        raise ValueError("q_len and kv_len are both None: the dense attention serves that")
    if resid is None:
        if out is None:
            out = torch.zeros(B, Sq, H * 64, dtype=torch.bfloat16, device=q.device)
        _check_out(out, "out", B, Sq, H, (torch.bfloat16,), q.device)
        entry, outs = hip.lib().ditto_attention_varlen_bf16, (out.data_ptr(), out.stride(1))
    else:
        src = resid if resid_in is None else resid_in
        _check_out(resid, "resid", B, Sq, H, (torch.float32, torch.bfloat16), q.device)
        _check_out(src, "resid_in", B, Sq, H, (resid.dtype,), q.device)
        if src.stride() != resid.stride():
            raise ValueError("resid / resid_in: fp32 or bf16 with the same dtype and row stride")
        entry = hip.lib().ditto_attention_resid_varlen_bf16
        outs = (src.data_ptr(), resid.data_ptr(), resid.stride(1), int(resid.dtype == torch.bfloat16))
    ql = _dev_lengths(q_len, B, Sq, "q_len", q.device)
    kl = _dev_lengths(kv_len, B, Skv, "kv_len", q.device)
    hip.check(entry(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), v.data_ptr(), v.stride(1), *outs,
                    ql.data_ptr() if ql is not None else None, kl.data_ptr() if kl is not None else None, B, H, Sq, Skv, 64,
                    torch.cuda.current_stream(q.device).cuda_stream))
    return out if resid is None else resid


def attention(q, k, v, H: int, q_len=None, kv_len=None, out=None):
    """softmax(q k^T) v per (utterance, head) over each utterance's own rows (q carries scale * log2(e)); q / out [B, Sq, >= H*64],
    k / v [B, Skv, >= H*64], bf16.  Rows of `out` past q_len are left as they were.  Returns `out`."""
    return _attention(q, k, v, H, q_len, kv_len, out=out)


def attention_resid(q, k, v, H: int, resid, q_len=None, kv_len=None, resid_in=None):
    """The residual form: resid[b, i, h*64 + c] = resid_in[...] + attention, for i < q_len[b] (resid_in None: in place); resid
    is fp32 or bf16 [B, Sq, >= H*64].  Rows past q_len are left untouched.  Returns `resid`."""
    return _attention(q, k, v, H, q_len, kv_len, resid=resid, resid_in=resid_in)


# ---------------------------------------------------------------------------------------------------------------------------------
# Packed batches (include/ditto_hip.h, the *_packed_* entries): utterances concatenated along the row axis, utterance b owning rows
# [cu[b], cu[b+1]) — flash-attention's varlen layout.  No padding is allocated, moved or computed.

def validate_cu_seqlens(cu, B: int, total: int, max_len: int, name: str = "cu_seqlens") -> torch.Tensor:
    """`cu` (list / tuple of ints, or an integer tensor on any device) as a CPU int32 tensor of shape [B + 1]: starting at 0, strictly
    increasing (no empty utterance), no utterance longer than `max_len`, ending at `total` (the packed rows).  Anything else raises
    ValueError."""
    if isinstance(cu, torch.Tensor):
        if cu.dtype.is_floating_point or cu.dtype.is_complex or cu.dtype == torch.bool:
            raise ValueError(f"{name}: an integer tensor is needed, got {cu.dtype}")
        t = cu.detach().to("cpu", torch.int64)
    elif isinstance(cu, (list, tuple)):
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in cu):
            raise ValueError(f"{name}: a list / tuple of ints is needed")
        t = torch.tensor(list(cu), dtype=torch.int64)
    else:
        raise ValueError(f"{name}: a list, tuple or integer tensor is needed, got {type(cu).__name__}")
    if t.dim() != 1 or t.shape[0] != B + 1:
        raise ValueError(f"{name}: shape [{B + 1}] expected, got {list(t.shape)}")
    if int(t[0]) != 0:
        raise ValueError(f"{name}: the offsets must start at 0, got {int(t[0])}")
    lens = t[1:] - t[:-1]
    if B and int(lens.min()) < 1:
        raise ValueError(f"{name}: the offsets must increase strictly (an utterance of {int(lens.min())} rows)")
    if B and int(lens.max()) > max_len:
        raise ValueError(f"{name}: an utterance of {int(lens.max())} rows exceeds the maximum length {max_len}")
    if int(t[-1]) != total:
        raise ValueError(f"{name}: the last offset {int(t[-1])} differs from the {total} packed rows")
    if total >= 2 ** 31:
        raise ValueError(f"{name}: {total} rows exceed int32 offsets")
    return t.to(torch.int32)


def cu_from_lengths(lengths) -> torch.Tensor:
    """[0, l0, l0 + l1, ...] as a CPU int32 tensor"""
    lens = torch.as_tensor(lengths, dtype=torch.int64).cpu()
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)]).to(torch.int32)


def validate_drop(drop, B: int, name: str = "drop") -> torch.Tensor:
    """`drop` (a list / tuple of bools or 0 / 1 ints, or a CPU bool / integer tensor) as a CPU bool tensor [B].  Anything else raises
    ValueError — a tensor on a device included: who is dropped decides the batch's layout, on the host, before anything is allocated."""
    if isinstance(drop, torch.Tensor):
        if drop.device.type != "cpu":
            raise ValueError(f"{name}: a CPU tensor is needed (the host lays the batch out), got one on {drop.device}")
        if drop.dtype.is_floating_point or drop.dtype.is_complex:
            raise ValueError(f"{name}: a bool or integer tensor is needed, got {drop.dtype}")
        t = drop.detach().to(torch.int64)
    elif isinstance(drop, (list, tuple)):
        if not all(isinstance(v, (bool, int)) for v in drop):
            raise ValueError(f"{name}: a list / tuple of bools is needed")
        t = torch.tensor([int(v) for v in drop], dtype=torch.int64)
    else:
        raise ValueError(f"{name}: a list, tuple or CPU bool tensor is needed, got {type(drop).__name__}")
    if t.dim() != 1 or t.shape[0] != B:
        raise ValueError(f"{name}: shape [{B}] expected, got {list(t.shape)}")
    if B and (int(t.min()) < 0 or int(t.max()) > 1):
        raise ValueError(f"{name}: every entry must be False / True (0 / 1)")
    return t.to(torch.bool)


def cond_dropout_layout(text_cu_seqlens, drop, T0: int):
    """Condition dropout's layout, on the host: utterance b of a packed text batch (offsets `text_cu_seqlens` [B + 1]) keeps its own
    rows, or — drop[b] — runs with the T0 rows of the null embedding as its text.  Returns (cu_out, table, max_T'):
    cu_out  CPU int32 [B + 1], the offsets of the effective text (its rows: S_T' = cu_out[-1]);
    table   CPU int32 [3B + 2] = [cu_out | text_cu_seqlens | drop], what ditto_text_select_packed and its backward read;
    max_T'  the longest effective text.
    A pure function of its arguments: no device, no library call."""
    if isinstance(T0, bool) or not isinstance(T0, int) or T0 < 1:
        raise ValueError(f"T0: the null embedding needs at least one row, got {T0!r}")
    n = len(text_cu_seqlens) - 1
    total = int(text_cu_seqlens[-1]) if n >= 0 and len(text_cu_seqlens) else 0
    ct = validate_cu_seqlens(text_cu_seqlens, n, total, max(total, 1), "text_cu_seqlens").to(torch.int64)
    if n < 1:
        raise ValueError("text_cu_seqlens: at least one utterance is needed")
    d = validate_drop(drop, n)
    lens = torch.where(d, torch.full((n,), T0, dtype=torch.int64), ct[1:] - ct[:-1])
    cu_out = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
    if int(cu_out[-1]) >= 2 ** 31:
        raise ValueError(f"cond_dropout_layout: {int(cu_out[-1])} effective text rows exceed int32 offsets")
    table = torch.cat([cu_out, ct, d.to(torch.int64)]).to(torch.int32).contiguous()
    return cu_out.to(torch.int32), table, int(lens.max())


def doubled_cu_seqlens(cu) -> torch.Tensor:
    """The offsets of [x; x] (classifier-free guidance: the batch followed by itself): [cu; S + cu[1:]]"""
    c = torch.as_tensor(cu).to(torch.int64)
    return torch.cat([c, c[-1] + c[1:]]).to(torch.int32)


def pack(x: torch.Tensor, lengths):
    """x [B, N, ...] padded, utterance b valid in x[b, :lengths[b]] -> (packed [S, ...] on x's device, cu int32 [B + 1] on x's
    device)."""
    B, N = int(x.shape[0]), int(x.shape[1])
    lens = validate_lengths(lengths, B, N, "lengths").to(torch.int64)
    cu = cu_from_lengths(lens)
    mask = torch.arange(N).unsqueeze(0) < lens.unsqueeze(1)                     # [B, N]
    packed = x[mask.to(x.device)]
    return packed.contiguous(), cu.to(x.device)


def unpack(packed: torch.Tensor, cu, N: int, fill: float = 0.0) -> torch.Tensor:
    """packed [S, ...] with offsets cu [B + 1] -> padded [B, N, ...] (rows past an utterance's length hold `fill`)."""
    c = torch.as_tensor(cu).detach().to("cpu", torch.int64)
    B = int(c.shape[0]) - 1
    c = validate_cu_seqlens(c, B, int(packed.shape[0]), N, "cu").to(torch.int64)
    out = torch.full((B, N, *packed.shape[1:]), fill, dtype=packed.dtype, device=packed.device)
    lens = c[1:] - c[:-1]
    mask = torch.arange(N).unsqueeze(0) < lens.unsqueeze(1)
    out[mask.to(packed.device)] = packed
    return out


def _dev_cu(cu, B, total, max_len, name, device):
    return validate_cu_seqlens(cu, B, total, max_len, name).to(device)


def _check_packed(t, name, H, dtypes=(torch.bfloat16,)):
    if t.dtype not in dtypes or t.dim() != 2 or not t.is_cuda or t.stride(1) != 1 or t.shape[1] < H * 64:
        raise ValueError(f"{name}: a {' / '.join(str(d) for d in dtypes)} [rows, >= {H * 64}] tensor on the GPU with unit column stride "
                         f"is needed, got {t.dtype} {list(t.shape)}")


def _attention_packed(q, k, v, H, cu_q, cu_kv, max_q, max_kv, out=None, resid=None, resid_in=None):
    """attention_packed (resid None: into `out`, allocated when None) and attention_resid_packed (into `resid`): one entry each"""
    for n, x in (("q", q), ("k", k), ("v", v)):
        _check_packed(x, n, H)
    if v.shape[0] != k.shape[0] or not (q.device == k.device == v.device):
        raise ValueError("k and v need one row count, q / k / v one device")
    Sq, Skv = int(q.shape[0]), int(k.shape[0])
    if resid is None:
        if out is None:
            out = torch.zeros(Sq, H * 64, dtype=torch.bfloat16, device=q.device)
        _check_packed(out, "out", H)
        if out.shape[0] != Sq:
            raise ValueError(f"out: {Sq} rows expected")
        entry, outs = hip.lib().ditto_attention_packed_bf16, (out.data_ptr(), out.stride(0))
    else:
        src = resid if resid_in is None else resid_in
        _check_packed(resid, "resid", H, (torch.float32, torch.bfloat16))
        if src.dtype != resid.dtype or src.stride() != resid.stride() or src.shape != resid.shape or resid.shape[0] != Sq:
            raise ValueError("resid / resid_in: one dtype, shape and row stride, q's rows")
        entry = hip.lib().ditto_attention_resid_packed_bf16
        outs = (src.data_ptr(), resid.data_ptr(), resid.stride(0), int(resid.dtype == torch.bfloat16))
    B = len(cu_q) - 1
    max_q = Sq if max_q is None else int(max_q)
    max_kv = Skv if max_kv is None else int(max_kv)
    cq = _dev_cu(cu_q, B, Sq, max_q, "cu_q", q.device)
    ck = _dev_cu(cu_kv, B, Skv, max_kv, "cu_kv", q.device)
    hip.check(entry(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), *outs, cq.data_ptr(), ck.data_ptr(),
                    B, H, Sq, Skv, max_q, max_kv, 64, torch.cuda.current_stream(q.device).cuda_stream))
    return out if resid is None else resid


def attention_packed(q, k, v, H: int, cu_q, cu_kv, max_q=None, max_kv=None, out=None):
    """softmax(q k^T) v per (utterance, head) of a packed batch (q carries scale * log2(e)): q / out [Sq, >= H*64] with utterance
    b in rows [cu_q[b], cu_q[b+1]), k / v [Skv, >= H*64] with rows [cu_kv[b], cu_kv[b+1]); bf16.  Returns `out`."""
    return _attention_packed(q, k, v, H, cu_q, cu_kv, max_q, max_kv, out=out)


def attention_resid_packed(q, k, v, H: int, resid, cu_q, cu_kv, max_q=None, max_kv=None, resid_in=None):
    """The residual form of attention_packed: resid[i, h*64 + c] = resid_in[...] + attention (resid_in None: in place); resid fp32 or
    bf16 [Sq, >= H*64].  Returns `resid`."""
    return _attention_packed(q, k, v, H, cu_q, cu_kv, max_q, max_kv, resid=resid, resid_in=resid_in)
