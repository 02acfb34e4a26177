"""The DDPM sampling loop over the HIP denoise path.

Mirrors the sampling surface of the reference's `SpeechGenerator`
(reference src/model/SpeechGenerator.py): constructor arguments `:18-27`, attributes `ditto_model`, `betas`,
`alphas`, `alphas_cumprod`, `device` `:70-72`, and the two (name-mangled) methods the notebooks reach,
`_SpeechGenerator__p_sample` `:130-147` and `_SpeechGenerator__sample_latents` `:149-164`.

Out of scope: the EnCodec / GPT-2 / BigVGAN pieces around the loop and the SLP's encoders (its decoder
stack is ditto_tts_amd/slp.py).  They are taken from
`ditto_model.nac` and from injected `vocoder` / `text_tokenizer` / `audio_processor` objects when present and
raise a clear error otherwise; nothing here re-implements them.

Differences from the reference, both deliberate and documented in SURVEY.md App. B:
  * B-8: the loop length is the caller's `utils.Config.ConfigDiTTO.DIFFUSION_STEPS` read at call time, as in the
    reference, when that module is imported (bounds-checked against the frozen tables instead of overrunning them);
    with `diffusion_steps=` or stand-alone it is this object's own table length;
  * B-9: RoPE tables and the cross-attention K/V of the unchanging text are computed once per call to
    `__sample_latents`, not once per step.
RNG: `torch.randn_like` on the state's device, in the reference's call order (one draw for x_T unless
`cond_by_audio`, then one draw per step).
"""
from __future__ import annotations

import functools
import math
from typing import Callable, Optional

import torch

from .engine import require_fused_attention
from .modules import DiTTO


def strided_schedule(alphas_cumprod: torch.Tensor, n_steps: int, eta: float = 0.0):
    """The strided (DDIM) schedule of `n_steps` evenly spaced timesteps over the table `alphas_cumprod`: a list of
    (tau_i, a, ce, sigma), x' = a x + ce eps + sigma z at step i (Song et al. 2021 eq. 12; the last step ends at abar = 1).
    The coefficients are computed in float64 and returned as Python floats."""
    T = int(alphas_cumprod.shape[0])
    if not 1 <= n_steps <= T:
        raise ValueError("n_steps must be in [1, diffusion_steps]")
    stride = T / n_steps
    taus = [int(round(T - 1 - i * stride)) for i in range(n_steps)]
    ac = alphas_cumprod.double().cpu()
    out = []
    for i, t_val in enumerate(taus):
        ab_t = ac[t_val]
        ab_p = ac[taus[i + 1]] if i + 1 < n_steps else torch.tensor(1.0, dtype=torch.float64)
        sigma = eta * torch.sqrt((1 - ab_p) / (1 - ab_t)) * torch.sqrt(1 - ab_t / ab_p)
        a = torch.sqrt(ab_p / ab_t)
        ce = torch.sqrt(torch.clamp(1 - ab_p - sigma ** 2, min=0.0)) - torch.sqrt(ab_p * (1 - ab_t) / ab_t)
        out.append((t_val, float(a), float(ce), float(sigma)))
    return out


def strided_schedule_v(alphas_cumprod: torch.Tensor, n_steps: int, eta: float = 0.0):
    """strided_schedule for a network that predicts v = alpha z - sigma x0 (Salimans & Ho 2022; Lin et al. 2024 section 3.2) instead of
    the noise: a list of (tau_i, a_v, cv, sigma), x' = a_v x + cv v + sigma z at step i, over the same timesteps and with the same
    sigma.  With x0 = alpha x - sigma_t v and eps = sigma_t x + alpha v (alpha = sqrt(abar), sigma_t = sqrt(1 - abar) at tau_i),
    alpha' = sqrt(abar') and c' = sqrt(clamp(1 - abar' - sigma^2, 0)): a_v = alpha' alpha + c' sigma_t and cv = c' alpha - alpha'
    sigma_t — each a sum of two products of numbers in [0, 1], so |a_v|, |cv| <= sqrt(2) at every step.  It is NOT computed as
    a + ce sigma_t from the eps form: at tau_0 of the cosine table 1 / alpha is ~100 and that is a difference of two numbers of that
    size.  The row layout is strided_schedule's: the fused updates are linear in the network's output, so a v step is the eps
    step's launch with (a_v, cv) in place of (a, ce).  float64, returned as Python floats."""
    T = int(alphas_cumprod.shape[0])
    if not 1 <= n_steps <= T:
        raise ValueError("n_steps must be in [1, diffusion_steps]")
    stride = T / n_steps
    taus = [int(round(T - 1 - i * stride)) for i in range(n_steps)]
    ac = alphas_cumprod.double().cpu()
    out = []
    for i, t_val in enumerate(taus):
        ab_t = ac[t_val]
        ab_p = ac[taus[i + 1]] if i + 1 < n_steps else torch.tensor(1.0, dtype=torch.float64)
        sigma = eta * torch.sqrt((1 - ab_p) / (1 - ab_t)) * torch.sqrt(1 - ab_t / ab_p)       # strided_schedule's, to the bit
        al_t, sg_t, al_p = torch.sqrt(ab_t), torch.sqrt(1 - ab_t), torch.sqrt(ab_p)
        c_p = torch.sqrt(torch.clamp(1 - ab_p - sigma ** 2, min=0.0))
        out.append((t_val, float(al_p * al_t + c_p * sg_t), float(c_p * al_t - al_p * sg_t), float(sigma)))
    return out


SOLVERS = ("ddim", "dpmpp2m")
PREDICTIONS = ("eps", "v")


def multistep_schedule(alphas_cumprod: torch.Tensor, n_steps: int):
    """The second-order multistep data-prediction solver, DPM-Solver++(2M) (Lu et al. 2022), over the timesteps of
    `strided_schedule`: a list of (tau_i, a, kx, ke, b, g, use_prev).  Step i predicts x0 = kx x + ke eps (kx = 1 / alpha_i, ke =
    -sigma_i / alpha_i) and moves to x' = a x + b x0 + g q with q the x0 of step i - 1; g = 0 where use_prev is False (step 0 and the
    last step, which ends at abar = 1 and is first order: x' = x0).  With lambda = log(alpha / sigma), h_i = lambda_{i+1} - lambda_i
    and r_i = h_{i-1} / h_i: a = sigma_{i+1} / sigma_i and x' = a x - alpha_{i+1} expm1(-h_i) D, D = (1 + 1 / (2 r_i)) x0 - (1 / (2
    r_i)) q.  Deterministic: one forward per step, no noise.  Computed in float64, returned as Python floats."""
    T = int(alphas_cumprod.shape[0])
    if not 1 <= n_steps <= T:
        raise ValueError("n_steps must be in [1, diffusion_steps]")
    stride = T / n_steps
    taus = [int(round(T - 1 - i * stride)) for i in range(n_steps)]
    ac = alphas_cumprod.double().cpu()
    alpha = [math.sqrt(float(ac[t])) for t in taus]
    sigma = [math.sqrt(1.0 - float(ac[t])) for t in taus]
    lam = [math.log(al / sg) for al, sg in zip(alpha, sigma)]
    out = []
    for i, t_val in enumerate(taus):
        kx, ke = 1.0 / alpha[i], -sigma[i] / alpha[i]
        if i == n_steps - 1:                                   # sigma_next = 0: the lower-order final step lands on x0
            out.append((t_val, 0.0, kx, ke, 1.0, 0.0, False))
            continue
        h = lam[i + 1] - lam[i]
        c = -alpha[i + 1] * math.expm1(-h)
        if i == 0:
            b, g = c, 0.0
        else:
            r = (lam[i] - lam[i - 1]) / h
            b, g = c * (1.0 + 0.5 / r), -c * 0.5 / r
        out.append((t_val, sigma[i + 1] / sigma[i], kx, ke, b, g, i > 0))
    return out


def multistep_schedule_v(alphas_cumprod: torch.Tensor, n_steps: int):
    """multistep_schedule for a network that predicts v (strided_schedule_v): the same rows except the data prediction, x0 = kx x +
    ke v with kx = alpha_i and ke = -sigma_i — no division by alpha.  a, b, g and use_prev act on x, x0 and the history and do not
    depend on the parameterisation."""
    ac = alphas_cumprod.double().cpu()
    return [(t_val, a, math.sqrt(float(ac[t_val])), -math.sqrt(1.0 - float(ac[t_val])), b, g, use_prev)
            for t_val, a, _, _, b, g, use_prev in multistep_schedule(alphas_cumprod, n_steps)]


def validate_prediction(prediction):
    """`prediction`: what the network's output is — "eps" (the noise, the reference's objective) or "v" (v = alpha z - sigma x0)"""
    if prediction not in PREDICTIONS:
        raise ValueError(f"prediction: one of {PREDICTIONS} is needed, got {prediction!r}")
    return prediction


def _padded_prediction(prediction):
    """the padded layouts sample eps-predicting networks only"""
    if validate_prediction(prediction) != "eps":
        raise NotImplementedError(f"prediction={prediction!r} is served over packed batches: pack the batch and call "
                                  "sample_guided_packed(prediction=)")


def validate_guidance_interval(interval, diffusion_steps: int):
    """`guidance_interval` — None, or a pair (t_lo, t_hi) of integer diffusion timesteps with 0 <= t_lo <= t_hi <= diffusion_steps - 1
    — as None or a tuple of two ints."""
    if interval is None:
        return None
    ok = isinstance(interval, (tuple, list)) and len(interval) == 2 and all(
        isinstance(v, int) and not isinstance(v, bool) for v in interval)
    if not ok:
        raise ValueError(f"guidance_interval: None or a pair (t_lo, t_hi) of ints is needed, got {interval!r}")
    lo, hi = interval
    if lo > hi or lo < 0 or hi > diffusion_steps - 1:
        raise ValueError(f"guidance_interval: 0 <= t_lo <= t_hi <= {diffusion_steps - 1} is needed, got {interval!r}")
    return lo, hi


def guided_steps(schedule, interval):
    """Which steps of a strided_schedule / multistep_schedule apply classifier-free guidance under `guidance_interval` (guidance in
    a limited interval, Kynkaanniemi et al. 2024): step i, at timestep tau_i, if and only if t_lo <= tau_i <= t_hi; every step
    without an interval.  The other steps use the conditional prediction alone and cost the unguided step."""
    if interval is None:
        return [True] * len(schedule)
    return [interval[0] <= row[0] <= interval[1] for row in schedule]


def validate_guidance_refresh(guidance_refresh):
    """`guidance_refresh` — None, or an int k >= 1: the unconditional forward runs at every k-th guided step — as None or an int."""
    if guidance_refresh is None:
        return None
    if isinstance(guidance_refresh, bool) or not isinstance(guidance_refresh, int) or guidance_refresh < 1:
        raise ValueError(f"guidance_refresh: None or an int >= 1 is needed, got {guidance_refresh!r}")
    return guidance_refresh


def refresh_plan(guided, k: int):
    """The schedule of a loop that reuses the guidance direction between refresh steps (the "CFG cache" of FasterCache, Lv et al.
    2024, without its frequency reweighting): `guided` is guided_steps' list, k >= 1 the refresh period.  Returns (kinds, mirror),
    one entry per step.  A counter j runs over the guided steps and is reset to 0 by every unguided one: a guided step is "refresh"
    (the forward over [x; x] x [text; null]; it keeps delta = c - u) where j % k == 0 and "reuse" (the conditional forward alone,
    e = c + (w - 1) delta) otherwise; an unguided step is "plain".  So the first guided step of the call is a refresh, and so is the
    first one behind any unguided run: a direction is never carried across steps that did not use it.  mirror[i]: step i is a reuse
    step and step i + 1 a refresh — its update writes the unconditional half of the state too, which that refresh reads.
    Pure host arithmetic."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"refresh_plan: k must be an int >= 1, got {k!r}")
    kinds, j = [], 0
    for g in guided:
        if not g:
            kinds.append("plain")
            j = 0
            continue
        kinds.append("refresh" if j % k == 0 else "reuse")
        j += 1
    mirror = [kinds[i] == "reuse" and i + 1 < len(kinds) and kinds[i + 1] == "refresh" for i in range(len(kinds))]
    return kinds, mirror


def guidance_vector(guidance, B: int) -> Optional[torch.Tensor]:
    """`guidance` (None, a number, or a sequence / tensor of B numbers) as a CPU fp32 tensor [B], or None (no guidance)."""
    if guidance is None:
        return None
    if isinstance(guidance, bool):
        raise ValueError("guidance: a number or a sequence of numbers is needed, got a bool")
    if isinstance(guidance, (int, float)):
        return torch.full((B,), float(guidance), dtype=torch.float32)
    if isinstance(guidance, torch.Tensor):
        if guidance.dtype == torch.bool or guidance.is_complex():
            raise ValueError(f"guidance: a real tensor is needed, got {guidance.dtype}")
        g = guidance.detach().to("cpu", torch.float32)
    elif isinstance(guidance, (list, tuple)):
        if not all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in guidance):
            raise ValueError("guidance: a list / tuple of numbers is needed")
        g = torch.tensor([float(v) for v in guidance], dtype=torch.float32)
    else:
        raise ValueError(f"guidance: None, a number, a sequence or a tensor is needed, got {type(guidance).__name__}")
    if g.dim() != 1 or g.shape[0] != B:
        raise ValueError(f"guidance: shape [{B}] expected, got {list(g.shape)}")
    if not torch.isfinite(g).all():
        raise ValueError("guidance: every scale must be finite")
    return g.contiguous()


def rescale_vector(guidance_rescale, B: int) -> Optional[torch.Tensor]:
    """`guidance_rescale` (None, a number in [0, 1], or a sequence of B of them) as a CPU fp32 tensor [B] of blend factors phi, or
    None (no rescale): guidance rescale, Lin et al. 2024 section 3.4."""
    if guidance_rescale is None:
        return None
    v = guidance_rescale
    if isinstance(v, torch.Tensor) and v.dtype != torch.bool and not v.is_complex() and v.dim() == 1:
        v = v.detach().cpu().tolist()
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        v = [v] * B
    if not isinstance(v, (list, tuple)) or not all(isinstance(x, (int, float)) and not isinstance(x, bool) for x in v):
        raise ValueError(f"guidance_rescale: None, a number or a sequence of {B} numbers is needed, got {guidance_rescale!r}")
    if len(v) != B:
        raise ValueError(f"guidance_rescale: {B} values expected (one per utterance), got {len(v)}")
    if not all(math.isfinite(x) and 0.0 <= x <= 1.0 for x in v):
        raise ValueError(f"guidance_rescale: every value must lie in [0, 1], got {guidance_rescale!r}")
    return torch.tensor([float(x) for x in v], dtype=torch.float32)


def _per_utterance(name, value, B: int, ok, rule: str) -> torch.Tensor:
    """`value` (a number, or a sequence / 1-d tensor of B numbers, each passing `ok`) as a CPU fp32 tensor [B]"""
    v = value
    if isinstance(v, torch.Tensor) and v.dtype != torch.bool and not v.is_complex() and v.dim() == 1:
        v = v.detach().cpu().tolist()
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        v = [v] * B
    if not isinstance(v, (list, tuple)) or not all(isinstance(x, (int, float)) and not isinstance(x, bool) for x in v):
        raise ValueError(f"{name}: None, a number or a sequence of {B} numbers is needed, got {value!r}")
    if len(v) != B:
        raise ValueError(f"{name}: {B} values expected (one per utterance), got {len(v)}")
    if not all(math.isfinite(x) and ok(x) for x in v):
        raise ValueError(f"{name}: every value must {rule}, got {value!r}")
    return torch.tensor([float(x) for x in v], dtype=torch.float32)


def projection_vectors(guidance_projection, guidance_norm_threshold, guidance_momentum, B: int):
    """The three keywords of projected guidance (APG, Sadat et al. 2024) as CPU fp32 tensors [B] (eta, r, beta), or None when
    `guidance_projection` is None: eta in [0, 1] the weight of the part of the direction parallel to the conditional x0 prediction;
    r > 0 the RMS threshold of the direction (None: 0, off); beta in (-1, 1) its momentum (None: 0).  The last two need the first."""
    if guidance_projection is None:
        for name, v in (("guidance_norm_threshold", guidance_norm_threshold), ("guidance_momentum", guidance_momentum)):
            if v is not None:
                raise ValueError(f"{name} needs guidance_projection=")
        return None
    eta = _per_utterance("guidance_projection", guidance_projection, B, lambda x: 0.0 <= x <= 1.0, "lie in [0, 1]")
    r = torch.zeros(B) if guidance_norm_threshold is None else _per_utterance(
        "guidance_norm_threshold", guidance_norm_threshold, B, lambda x: x > 0.0, "be positive")
    beta = torch.zeros(B) if guidance_momentum is None else _per_utterance(
        "guidance_momentum", guidance_momentum, B, lambda x: -1.0 < x < 1.0, "lie in (-1, 1)")
    return eta, r, beta


def project_table(projection, gv, x0_rows, guided):
    """The device table of a projected call, fp32 [n_steps, B, 8]: one ditto_project_coef per step and utterance.  `projection`:
    projection_vectors' (eta, r, beta); `gv`: guidance_vector's scales; `x0_rows`: the multistep schedule's rows over the call's
    timesteps, whose (kx, ke) map the network's output to x0 at step i; `guided`: guided_steps' list.  use_prev is 1 from the second
    guided step on, whatever lies in between: an unguided step leaves the direction alone.  Pure host arithmetic."""
    eta, r, beta = projection
    B = int(gv.shape[0])
    table = torch.zeros(len(x0_rows), B, 8, dtype=torch.float32)
    seen = False
    for i, row in enumerate(x0_rows):
        table[i, :, 0], table[i, :, 1] = row[2], row[3]
        table[i, :, 2], table[i, :, 3], table[i, :, 4], table[i, :, 5] = gv, eta, r, beta
        table.view(torch.int32)[i, :, 6] = int(seen and guided[i])
        seen = seen or guided[i]
    return table


def _padded_projection(guidance_projection, guidance_norm_threshold=None, guidance_momentum=None):
    """the padded layouts have no projected guidance"""
    if guidance_projection is not None or guidance_norm_threshold is not None or guidance_momentum is not None:
        raise NotImplementedError("guidance_projection= is served over packed batches: pack the batch and call "
                                  "sample_guided_packed(guidance_projection=)")


def _padded_rescale(guidance_rescale):
    """the padded layouts have no guidance rescale"""
    if guidance_rescale is not None:
        raise NotImplementedError("guidance_rescale= is served over packed batches: pack the batch and call "
                                  "sample_guided_packed(guidance_rescale=)")


def _padded_suffix(suffix_lengths):
    """the padded layouts have no speech infilling"""
    if suffix_lengths is not None:
        raise NotImplementedError("speech infilling is served over packed batches: pack the batch and call "
                                  "sample_guided_packed(suffix_lengths=)")


def _padded_solver(solver):
    """the padded layouts run the strided (DDIM) solver only"""
    if solver not in SOLVERS:
        raise ValueError(f"solver: one of {SOLVERS} is needed, got {solver!r}")
    if solver != "ddim":
        raise NotImplementedError(f"solver={solver!r} is served over packed batches: pack the batch and call "
                                  "sample_guided_packed(solver=)")


class SpeechGenerator:
    def __init__(self, lambda_factor=0.1, nac_model_path=None, ditto_model_path=None, slp_path=None,
                 sample_rate=24000, device="cuda", *, ditto_model: Optional[DiTTO] = None, config=None,
                 diffusion_steps: Optional[int] = None, vocoder=None, mel_fn: Optional[Callable] = None,
                 text_tokenizer=None, audio_processor=None, slp=None):
        self.device = device
        if ditto_model is None:
            if config is None:
                # the CALLER's utils.Config.ConfigDiTTO when its tree is importable (so a notebook's mutation of the
                # class attributes is what gets read, reference src/Experiments.ipynb cell 6), else the shipped values
                from .shipped_config import config_classes
                config = config_classes()[0]
            ditto_model = DiTTO(hidden_dim=config.HIDDEN_DIM, num_layers=config.NUM_LAYERS,
                                num_heads=config.NUM_HEADS, time_dim=config.TIME_DIM,
                                text_dim=config.TEXT_EMBED_DIM, diffusion_steps=config.DIFFUSION_STEPS,
                                lambda_factor=lambda_factor, nac_model_path=nac_model_path)
            if ditto_model_path is not None:
                info = torch.load(ditto_model_path, map_location="cpu")
                ditto_model.load_state_dict(info["model_state_dict"], strict=ditto_model.nac is not None)
        self.ditto_model = ditto_model.to(self.device).eval()
        if slp is None and slp_path is not None:
            # reference :54-62: SLP(ConfigSLP.NB_CLASSES, NUM_HEADS, NUM_LAYERS) + its checkpoint.  Only the decoder
            # stack and the head are built here (ditto_tts_amd/slp.py); the checkpoint's text_encoder.* /
            # audio_encoder.* entries belong to the pretrained encoders and are skipped.
            from .shipped_config import config_classes
            ConfigSLP = config_classes()[1]
            from .slp import SLP
            slp = SLP(ConfigSLP.NB_CLASSES, ConfigSLP.NUM_HEADS, ConfigSLP.NUM_LAYERS,
                      hidden_size=ConfigSLP.EMBEDDING_DIM)
            info = torch.load(slp_path, map_location="cpu")
            res = slp.load_state_dict(info["model_state_dict"], strict=False)
            if res.missing_keys:
                raise KeyError(f"SLP checkpoint {slp_path} lacks {res.missing_keys[:3]}...")
            slp = slp.to(self.device).eval()
        self.sample_rate = sample_rate
        self.vocoder, self.mel_fn, self.slp = vocoder, mel_fn, slp
        self.text_tokenizer, self.audio_processor = text_tokenizer, audio_processor
        # `diffusion_steps=` (an extension) pins the loop length; without it the reference's rule applies: the tables
        # are frozen here from the model's step count (reference :70 reads ConfigDiTTO.DIFFUSION_STEPS, which is also
        # what the model was built from, :32-36) and the LOOP length is read from the caller's mutable
        # ConfigDiTTO.DIFFUSION_STEPS at call time (reference :161), see `_loop_steps`.
        self._pinned_steps = diffusion_steps is not None
        steps = diffusion_steps if diffusion_steps is not None else self.ditto_model.cfg.diffusion_steps
        if steps > self.ditto_model.cfg.diffusion_steps:
            raise ValueError("diffusion_steps exceeds the rows of the model's t_embedding")
        # reference src/model/SpeechGenerator.py:70-72
        self.betas = self.ditto_model.cosine_beta_schedule(steps).to(self.device)
        self.alphas = (1.0 - self.betas).to(self.device)
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0).to(self.device)

    @property
    def diffusion_steps(self) -> int:
        return int(self.betas.shape[0])

    def _loop_steps(self) -> int:
        """Number of reverse steps of one call to __sample_latents.  Reference src/model/SpeechGenerator.py:161 reads
        the global `ConfigDiTTO.DIFFUSION_STEPS` at CALL time while the tables were frozen at construction (SURVEY
        App. B-8).  When the caller's `utils.Config` module is imported and this object was not pinned with
        `diffusion_steps=`, that read is reproduced (a shorter count starts the loop at that t, as the reference does;
        a longer one would index past the tables there — here it raises with a message).  Otherwise the loop length is
        the table length."""
        if not self._pinned_steps:
            from .shipped_config import caller_config
            mod = caller_config(import_it=False)
            if mod is not None:
                n = int(mod.ConfigDiTTO.DIFFUSION_STEPS)
                if n > self.diffusion_steps:
                    raise IndexError(f"ConfigDiTTO.DIFFUSION_STEPS = {n} exceeds the {self.diffusion_steps}-entry "
                                     "schedule tables frozen when this SpeechGenerator was built")
                return n
        return self.diffusion_steps

    # ---------------------------------------------------------------- the hot loop
    @torch.no_grad()
    def __p_sample(self, x, t, text_emb, noise=None):
        """Reverse diffusion step (reference :130-147).  Returns a new tensor, like the reference."""
        m = self.ditto_model
        cond = m.text_cond(text_emb, x.shape[1])
        if noise is None:
            noise = torch.randn_like(x)
        x_prev = x.detach().float().contiguous().clone()
        m.engine().p_sample_(x_prev, cond, t, noise, self.betas, self.alphas, self.alphas_cumprod)
        return x_prev

    @torch.no_grad()
    def __sample_latents(self, text_emb, audio_emb, text_prompt=None, audio=None, is_slp=False, cond_by_audio=False,
                         noises=None, keep=None, use_graph=None, seeds=None, batch_class=None, speech_lengths=None,
                         text_lengths=None):
        """All reverse diffusion steps (reference :149-164).

        `noises` (optional): a sequence / callable giving the z of executed step i, for parity tests;
        `keep` (optional): dict filled with {i: state after step i} for the i it already has as keys;
        `seeds` (optional, int64 [B]): per-utterance seeds.  x_T and every step's z then come from the library's
        counter-based generator (Philox4x32-10 keyed by the utterance's seed, engine.noise_normal_), generated inside
        the update kernel: an utterance's trajectory is a function of (seed, text, weights) and of the KERNEL CLASS its
        launches take (batches of 11 .. 15 and >= 17 utterances of 1024 frames — csrc/kernels.h fr_rule_rows — run two GEMM + LayerNorm pairs per block on a full-row kernel,
        which sums over k in another order).  Default None = the reference's behaviour, torch.randn_like from the global
        generator;
        `batch_class` (optional int): the number of utterances of the UNSPLIT batch this call is a piece of.  The loop
        then passes hip.CallOpts(class_rows = batch_class * N) to every step's call, every launch picks the class that batch would pick, and an
        utterance's latents are the same bits whatever piece or GPU it is sampled on (dist.sample_sharded pins the
        class itself: do not pass it there);
        `use_graph`: replay the step from a HIP graph (default off: measured no gain even at B = 1, the step is
        bound by per-kernel latency, not by its 122 launches; bit-identical to eager either way)."""
        if is_slp:
            raise NotImplementedError("the is_slp branch is broken in the reference (it passes the predictor's logits "
                                      "as a tensor shape, SURVEY.md App. B-6); length logits are available from "
                                      "self.slp.decode(z_text, z_audio)")
        m = self.ditto_model
        if seeds is not None and (noises is not None or use_graph):
            raise ValueError("seeds= excludes noises= and use_graph=")
        varlen = speech_lengths is not None or text_lengths is not None
        if varlen and use_graph:
            raise NotImplementedError("variable-length batches are not captured into a step graph (use_graph=False)")
        if varlen and cond_by_audio:
            raise NotImplementedError("variable-length batches start from noise (cond_by_audio=False)")
        if seeds is not None and not cond_by_audio:
            x = torch.empty(audio_emb.shape, dtype=torch.float32, device=self.device)
            seeds = seeds.to(self.device).long().contiguous()
            m.engine(x.device).noise_normal_(x, seeds, 0xFFFFFFFF)        # x_T: step index no loop step uses
        else:
            x = torch.randn_like(audio_emb) if not cond_by_audio else audio_emb.clone()
            x = x.to(self.device).float().contiguous()
            if seeds is not None:
                seeds = seeds.to(self.device).long().contiguous()
        eng = m.engine(x.device)
        cond = m.text_cond(text_emb.to(x.device), x.shape[1], text_lengths=text_lengths)
        B = x.shape[0]
        if varlen:   # (validated once here; every step passes the same device lengths)
            from .varlen import validate_lengths
            speech_lengths = validate_lengths(speech_lengths if speech_lengths is not None else [x.shape[1]] * B, B, x.shape[1],
                                              "speech_lengths").to(x.device)
        t_tensor = torch.empty(B, device=x.device, dtype=torch.long)
        use_graph = bool(use_graph)
        z = torch.empty_like(x)
        n_loop = self._loop_steps()
        opts = None
        if batch_class is not None:                 # every step of the loop is CALLED with the unsplit batch's kernel class: a
            from .hip import CallOpts               # per-call argument (ditto_call_opts), nothing process-wide changes
            opts = CallOpts(class_rows=int(batch_class) * x.shape[1])
        return self.__loop(x, cond, t_tensor, z, use_graph, n_loop, seeds, noises, keep, eng, opts, speech_lengths)

    def __loop(self, x, cond, t_tensor, z, use_graph, n_loop, seeds, noises, keep, eng, opts=None, speech_lengths=None):
        graph = None
        if use_graph:
            t_tensor.fill_(n_loop - 1)
            keep_x = x.clone()                      # capture runs one warm-up step on x: restore it afterwards
            z.zero_()
            graph = eng.capture_p_sample(x, cond, t_tensor, z, self.betas, self.alphas, self.alphas_cumprod, opts=opts)
            x.copy_(keep_x)
        for i, t_val in enumerate(reversed(range(n_loop))):
            t_tensor.fill_(t_val)
            if seeds is not None:
                eng.p_sample_seeded_(x, cond, t_tensor, seeds, t_val, self.betas, self.alphas, self.alphas_cumprod, opts=opts,
                                     speech_lengths=speech_lengths)
                if keep is not None and i in keep:
                    keep[i] = x.clone()
                continue
            if noises is None:
                z.normal_()                          # same generator stream as randn_like(x)
            else:
                z.copy_((noises(i) if callable(noises) else noises[i]).to(x.device))
            if graph is not None:
                graph.replay()
            else:
                eng.p_sample_(x, cond, t_tensor, z, self.betas, self.alphas, self.alphas_cumprod, opts=opts,
                              speech_lengths=speech_lengths)
            if keep is not None and i in keep:
                keep[i] = x.clone()
        return x

    # ---------------------------------------------------------------- strided (DDIM) loop + CFG  
    @torch.no_grad()
    def sample_latents_strided(self, text_emb, audio_emb, n_steps=25, eta=0.0, cfg_scale=None, null_text_emb=None,
                               cond_by_audio=False, noises=None, speech_lengths=None, text_lengths=None, prompt_lengths=None,
                               solver="ddim", guidance_rescale=None, suffix_lengths=None, prediction="eps",
                               guidance_projection=None, guidance_norm_threshold=None, guidance_momentum=None):
        """The serving configuration of the paper (App. A: 25 steps, guidance 5.0), which the reference lacks: a
        DDIM-style loop over `n_steps` evenly spaced timesteps, x' = a x + ce eps + cz z per step, with optional
        classifier-free guidance: the step runs ONE forward on the doubled batch [x; x] x [text; null_text] and combines
        eps_u + w (eps_c - eps_u).  sample_guided with one uniform `cfg_scale` over a dense batch: one library call per step."""
        _padded_solver(solver)
        _padded_rescale(guidance_rescale)
        _padded_projection(guidance_projection, guidance_norm_threshold, guidance_momentum)
        _padded_suffix(suffix_lengths)
        if prompt_lengths is not None:
            raise NotImplementedError("speech prompts are served over packed batches: sample_guided_packed(prompt_lengths=)")
        _padded_prediction(prediction)
        if speech_lengths is not None or text_lengths is not None:
            raise NotImplementedError("sample_latents_strided has no varlen form: a variable-length batch runs sample_guided "
                                      "(guided strided loop) or the ancestral sample_latents")
        return self.sample_guided(text_emb, audio_emb, n_steps=n_steps, eta=eta,
                                  guidance=None if cfg_scale is None else float(cfg_scale), null_text_emb=null_text_emb,
                                  noises=noises, cond_by_audio=cond_by_audio)

    # ---------------------------------------------------------------- guided strided loop over a variable-length batch
    def _step_loop(self, B, guidance, null_text_emb, seeds, batch_class, begin, interval, begin_plain, rescale, refresh, begin_reuse,
                   make_schedule, solver):
        """The loop of sample_guided and sample_guided_packed, whatever the solver.  `begin(eng, cfg, seeds)` is the layout's own
        prologue: it builds the conditioning and the state x2 (rows [x_T; room for the unconditional half] under guidance, else
        x_T) and returns (x2, max length, step) with `step(t=, opts=, ...)` the layout's library call bound to x2, its conditioning
        and its lengths or offsets.
        `make_schedule()` gives the solver's rows, the timestep first; `solver(eng, schedule, x, N, w, phi, seeds)` runs once behind
        the prologue — x the conditional half of x2, w the guidance scales and phi the rescale factors on the device, each None
        when unused —, allocates what the solver keeps over the call and returns `kwargs(i, kind)`: the solver's keyword arguments
        of step i for kind "plain", "reuse" or "step", asked for once per step and in step order.
        `interval` (a guidance interval, packed batches): step i is guided where guided_steps says so; the others run
        `begin_plain(eng, x2)`'s step — the layout's non-CFG call on the conditional half of x2, built only when a step needs it.
        The unconditional half is filled from the conditional one before the first guided step, and again before the first one
        behind unguided steps; in between every guided update writes both halves itself.  With no guided step at all the call is
        the one without guidance.
        `rescale` (rescale_vector's phi [B], packed batches): guided steps rescale (the solver's "step" arguments), the others not.
        `refresh` (an int k >= 2, packed batches; None: the loop as it was): refresh_plan's schedule over the guided steps.
        `begin_reuse(eng, x2, step, delta)` returns (refresh step, reuse step, plain step): the layout's STORE call on x2 with the
        guided conditioning, its LOAD call on the conditional half with begin_plain's text-only conditioning, and begin_plain's
        step itself.  delta [rows, d] is allocated once here.  A reuse step leaves the unconditional half behind unless it
        mirrors, so the copy runs before a refresh whose preceding step did not mirror."""
        gv = guidance_vector(guidance, B)
        if gv is not None and null_text_emb is None:
            raise ValueError("classifier-free guidance needs null_text_emb (the unconditional text embedding)")
        schedule = make_schedule()
        guided = guided_steps(schedule, interval)
        cfg = gv is not None and any(guided)
        eng = self.ditto_model.engine(torch.empty(0, device=self.device).device)   # "cuda" -> cuda:0: the engine the other loops use
        if seeds is not None:
            seeds = seeds.to(eng.device).long().contiguous()
            if seeds.shape != (B,):
                raise ValueError(f"seeds must have shape [{B}]")
        x2, N, step = begin(eng, cfg, seeds)
        rows = x2.shape[0] // 2 if cfg else x2.shape[0]
        kinds = mirror = reuse = None
        if refresh is not None and cfg:
            kinds, mirror = refresh_plan(guided, refresh)
            step, reuse, plain = begin_reuse(eng, x2, step, torch.empty_like(x2[:rows]))
        else:
            plain = begin_plain(eng, x2) if cfg and not all(guided) else None
        kwargs = solver(eng, schedule, x2[:rows], N, gv.to(eng.device) if cfg else None,
                        rescale.to(eng.device) if rescale is not None and cfg else None, seeds)
        t_tensor = torch.empty(2 * B if cfg else B, device=eng.device, dtype=torch.long)
        opts = plain_opts = None
        if batch_class is not None:
            from .hip import CallOpts
            opts = CallOpts(class_rows=(2 if cfg else 1) * int(batch_class) * N)
            plain_opts = CallOpts(class_rows=int(batch_class) * N)             # what the call without guidance pins
        stale = cfg                                          # the unconditional half is behind the conditional one
        for i, row in enumerate(schedule):
            t_tensor.fill_(row[0])
            if cfg and not guided[i]:                        # outside the interval: the non-CFG step on the conditional half
                plain(t=t_tensor[:B], opts=plain_opts, **kwargs(i, "plain"))
                stale = True
            elif kinds is not None and kinds[i] == "reuse":  # the conditional forward alone, e = c + (w - 1) delta
                reuse(t=t_tensor[:B], opts=plain_opts, mirror=mirror[i], **kwargs(i, "reuse"))
                stale = not mirror[i]
            else:
                if stale:                                    # [x; x], once; then every guided update writes both halves itself
                    x2[rows:].copy_(x2[:rows])
                    stale = False
                step(t=t_tensor, opts=opts, **kwargs(i, "step"))
        return x2[:rows].clone() if cfg else x2

    def _guided_loop(self, B, guidance, null_text_emb, n_steps, eta, seeds, noises, batch_class, begin, interval=None,
                     begin_plain=None, rescale=None, prediction="eps", refresh=None, begin_reuse=None, projection=None):
        """_step_loop for the strided (DDIM) update: `step(t=, a=, ce=, cz=, w=, noise=, seeds=, step=, opts=)`.  Every step's
        coefficients go up in one upload; step i's z (when sigma != 0) is Philox of `seeds` inside the kernel, `noises[i]`, else
        z.normal_() from torch's generator, one draw per noisy step in step order.
        `rescale`: every guided step computes each utterance's guidance-rescale factor from its eps and updates with ce s32 (the
        step's phi= argument).
        `prediction` "v" (packed batches): the rows of strided_schedule_v — (a_v, cv) travel where (a, ce) do, to the same launches.
        `projection` (projection_vectors' (eta, r, beta)): `begin`'s step is engine.guided_step_packed_project_; the guided steps get
        the direction buffer, the scratch — both allocated once here — and their row of project_table instead of w."""
        if seeds is not None and noises is not None:
            raise ValueError("seeds= excludes noises=")
        x0_rows = (multistep_schedule_v if prediction == "v" else multistep_schedule)(self.alphas_cumprod, n_steps) \
            if projection is not None else None

        def solver(eng, schedule, x, N, w, phi, seeds):
            # coef[i] = (a, ce, sigma) x B
            coef = torch.tensor([[[a] * B, [ce] * B, [sg] * B] for _, a, ce, sg in schedule], dtype=torch.float32).to(eng.device)
            rs = {} if phi is None else dict(phi=phi, rescale_scratch=eng.rescale_scratch(B, N))
            z = torch.empty_like(x) if seeds is None else None
            if projection is not None and w is not None:
                proj = project_table(projection, w.cpu(), x0_rows, guided_steps(schedule, interval)).to(eng.device)
                pj = dict(direction=torch.empty_like(x), project_scratch=eng.project_scratch(B, N))

            def kwargs(i, kind):
                noise = sd = None
                if schedule[i][3] != 0.0:
                    if seeds is not None:
                        sd = seeds
                    elif noises is None:
                        noise = z.normal_()
                    else:
                        noise = z.copy_((noises(i) if callable(noises) else noises[i]).to(eng.device))
                if kind == "step" and projection is not None and w is not None:
                    return dict(a=coef[i, 0], ce=coef[i, 1], cz=coef[i, 2], noise=noise, seeds=sd, step=schedule[i][0], proj=proj[i], **pj)
                return dict(a=coef[i, 0], ce=coef[i, 1], cz=coef[i, 2], w=None if kind == "plain" else w, noise=noise, seeds=sd,
                            step=schedule[i][0], **(rs if kind == "step" else {}))
            return kwargs

        return self._step_loop(B, guidance, null_text_emb, seeds, batch_class, begin, interval, begin_plain, rescale, refresh, begin_reuse,
                               lambda: (strided_schedule_v if prediction == "v" else strided_schedule)(self.alphas_cumprod, n_steps, eta),
                               solver)

    def _multistep_loop(self, B, guidance, null_text_emb, n_steps, seeds, batch_class, begin, interval=None, begin_plain=None,
                        rescale=None, prediction="eps", refresh=None, begin_reuse=None, projection=None):
        """_step_loop for solver="dpmpp2m": `begin`'s step is engine.guided_step_packed_multistep_ bound to x2, its conditioning and
        offsets; one library call per step of multistep_schedule over x2 and the history q — one buffer [S, d] per call, written
        by step 0 before any step reads it, the x0 of whichever step wrote it (conditional, guided or reuse: no special case).
        Each step's coefficients travel as a host struct.
        `rescale` (rescale_vector's phi [B]): the guided steps read their coefficients from DEVICE memory instead — one
        ditto_multistep_coef per utterance and step, uploaded once, the guidance scale inside — so that the rescale can patch each
        utterance's ke before the per-utterance update runs.
        `prediction` "v": the rows of multistep_schedule_v, (kx, ke) = (alpha, -sigma), to the same launches.
        `projection`: as in _guided_loop, with engine.guided_step_packed_multistep_project_."""
        from .hip import MultistepCoef

        def solver(eng, schedule, x, N, w, phi, seeds):
            q = torch.empty_like(x)
            coefs = rs = None
            if phi is not None:
                table = torch.zeros(len(schedule), B, 8, dtype=torch.float32)
                for i, row in enumerate(schedule):
                    table[i, :, :5] = torch.tensor(row[1:6], dtype=torch.float32)
                    table[i, :, 5] = guidance_vector(guidance, B)
                    table.view(torch.int32)[i, :, 6] = int(row[6])                      # use_prev
                coefs, rs = table.to(eng.device), eng.rescale_scratch(B, N)
            if projection is not None and w is not None:
                proj = project_table(projection, w.cpu(), schedule, guided_steps(schedule, interval)).to(eng.device)
                pj = dict(direction=torch.empty_like(x), project_scratch=eng.project_scratch(B, N))

            def kwargs(i, kind):
                if kind == "step" and coefs is not None:
                    return dict(q=q, coef=None, coefs=coefs[i], phi=phi, rescale_scratch=rs)
                _, a, kx, ke, b, g, use_prev = schedule[i]
                if kind == "step" and projection is not None and w is not None:
                    return dict(q=q, coef=MultistepCoef(a, kx, ke, b, g, 0.0, int(use_prev), 0), proj=proj[i], **pj)
                return dict(q=q, coef=MultistepCoef(a, kx, ke, b, g, 0.0, int(use_prev), 0), w=None if kind == "plain" else w)
            return kwargs

        return self._step_loop(B, guidance, null_text_emb, seeds, batch_class, begin, interval, begin_plain, rescale, refresh, begin_reuse,
                               lambda: (multistep_schedule_v if prediction == "v" else multistep_schedule)(self.alphas_cumprod, n_steps),
                               solver)

    @torch.no_grad()
    def sample_guided(self, text_emb, audio_emb, *, n_steps=25, eta=0.0, guidance=None, null_text_emb=None,
                      null_text_lengths=None, speech_lengths=None, text_lengths=None, seeds=None, noises=None,
                      cond_by_audio=False, batch_class=None, prompt_lengths=None, solver="ddim", guidance_rescale=None,
                      suffix_lengths=None, prediction="eps", guidance_projection=None, guidance_norm_threshold=None,
                      guidance_momentum=None):
        """The strided (DDIM) loop of sample_latents_strided with what serving needs: per-utterance `speech_lengths` /
        `text_lengths` (a padded batch; rows past an utterance's length are exactly 0 in the result and padding never reaches a
        valid row), per-utterance `guidance` (None: no CFG; a number; or [B] numbers), and per-utterance `seeds`.  One library
        call per step (ditto_guided_step_opts): the forward over [x; x] x [text; null] and one fused update kernel
        (csrc/guided.hip) that combines the guidance, adds the step's noise, writes both halves of the next doubled input and
        zeroes the padding.

        `null_text_emb` (required with guidance) broadcasts to text_emb; `null_text_lengths` default to `text_lengths`.
        x_T: `seeds` -> ditto_noise_normal(seeds, 0xFFFFFFFF) (the x_T of sample_latents(seeds=)); `cond_by_audio` -> audio_emb;
        else torch.randn_like.  Step i's z (when sigma != 0): Philox of `seeds` at tag tau_i, `noises[i]` (a sequence or
        callable, for parity tests), else z.normal_() from torch's generator.  `batch_class`: the unsplit batch's utterance
        count; every step is called with class_rows = (2 with guidance, else 1) * batch_class * N.
        The padded layout has no speech prompts (`prompt_lengths` raises NotImplementedError): pack the batch and call
        sample_guided_packed; so do solver="dpmpp2m", `guidance_rescale`, `suffix_lengths`, prediction="v" and `guidance_projection`
        (with `guidance_norm_threshold`, `guidance_momentum`).  Returns fp32 [B, N, d]."""
        _padded_solver(solver)
        _padded_rescale(guidance_rescale)
        _padded_projection(guidance_projection, guidance_norm_threshold, guidance_momentum)
        _padded_suffix(suffix_lengths)
        if prompt_lengths is not None:
            raise NotImplementedError("speech prompts are served over packed batches: sample_guided_packed(prompt_lengths=)")
        _padded_prediction(prediction)
        B, N = int(audio_emb.shape[0]), int(audio_emb.shape[1])

        def begin(eng, cfg, seeds):
            text = text_emb.to(eng.device).float()
            T = int(text.shape[1])
            if null_text_lengths is not None and not cfg:
                raise ValueError("null_text_lengths without guidance")
            varlen = speech_lengths is not None or text_lengths is not None or null_text_lengths is not None
            if varlen:
                require_fused_attention(eng.cfg, "variable-length batches")
                from .varlen import validate_lengths
                sl = validate_lengths(speech_lengths if speech_lengths is not None else [N] * B, B, N, "speech_lengths")
                tl = validate_lengths(text_lengths if text_lengths is not None else [T] * B, B, T, "text_lengths")
                if cfg:
                    ntl = validate_lengths(null_text_lengths, B, T, "null_text_lengths") if null_text_lengths is not None else tl
                    tl = torch.cat([tl, ntl])
            if cfg:
                text = torch.cat([text, null_text_emb.to(eng.device).float().expand_as(text)], dim=0).contiguous()
            cond = eng.prepare_text(text, N, text_lengths=tl if varlen else None)
            lens = eng.guided_lengths(sl if varlen else None, cond, B, N, cfg)
            x2 = torch.empty(2 * B if cfg else B, N, int(audio_emb.shape[2]), dtype=torch.float32, device=eng.device)
            if seeds is not None and not cond_by_audio:
                eng.noise_normal_(x2[:B], seeds, 0xFFFFFFFF)   # x_T: the step tag no loop step uses (sample_latents(seeds=))
            else:
                x2[:B].copy_(torch.randn_like(audio_emb) if not cond_by_audio else audio_emb)
            return x2, N, functools.partial(eng.guided_step_, x2, cond, B=B, lengths=lens)

        return self._guided_loop(B, guidance, null_text_emb, n_steps, eta, seeds, noises, batch_class, begin)

    @torch.no_grad()
    def sample_guided_packed(self, text_emb, text_cu_seqlens, audio_emb, cu_seqlens, *, n_steps=25, eta=0.0, guidance=None,
                             null_text_emb=None, null_text_cu_seqlens=None, seeds=None, noises=None, cond_by_audio=False,
                             batch_class=None, prompt_lengths=None, solver="ddim", guidance_interval=None, guidance_rescale=None,
                             suffix_lengths=None, prediction="eps", guidance_refresh=None, guidance_projection=None,
                             guidance_norm_threshold=None, guidance_momentum=None):
        """sample_guided over a PACKED batch: audio_emb [S, d] with utterance b in rows [cu_seqlens[b], cu_seqlens[b+1]), text_emb
        [S_T, text_dim] with its text in rows [text_cu_seqlens[b], text_cu_seqlens[b+1]).  The same loop and semantics as
        sample_guided; no padding is allocated, moved or computed.  Each step is one call of ditto_guided_step_packed_opts over
        [x; x] (offsets [cu; S + cu[1:]]) x [text; null].
        `null_text_emb` (required with guidance) is packed like the text — the same rows and offsets — unless `null_text_cu_seqlens`
        gives its own offsets.  `seeds`: x_T = ditto_noise_normal(seeds, 0xFFFFFFFF) per utterance and Philox z at each step's tag,
        the bits sample_guided(seeds=) draws for the same utterance.  `noises[i]` (a sequence or callable): packed [S, d].
        `batch_class`: class_rows = (2 with guidance, else 1) * batch_class * max length, what sample_guided pins for the padded
        batch of batch_class utterances.
        `prompt_lengths` (list / tuple / int tensor [B], 0 <= P_b < N_b): a SPEECH PROMPT per utterance — the first P_b rows of
        utterance b in `audio_emb` are the target speaker's clean latents; they stand in front of the frames to generate at every
        step (the forward attends to them like to any rows) and come back bit-equal.  The other G_b = N_b - P_b rows start from x_T —
        with `seeds`, ditto_noise_normal(seed_b, 0xFFFFFFFF) over G_b rows, what an unprompted utterance of G_b frames starts from —
        and every step is one ditto_guided_step_packed_prompt_opts call whose update skips the prompt rows.  A model uses a prompt
        only if it was trained with one (DiTTO.span_noise_packed / span_loss_packed).
        `solver`: "ddim" (the strided update above) or "dpmpp2m" — the second-order multistep solver of multistep_schedule over the
        same timesteps: one ditto_guided_step_packed_multistep_opts call per step, the same forward, and an update that keeps the
        previous step's x0 prediction in a history buffer [S, d].  It is deterministic: `eta` != 0 and `noises` raise ValueError,
        `seeds` give x_T only; every other argument works as above.
        `guidance_interval` (None, or a pair (t_lo, t_hi) of integer diffusion timesteps in [0, diffusion_steps - 1]): guidance in a
        limited interval (Kynkaanniemi et al. 2024) — step i is guided if and only if t_lo <= tau_i <= t_hi (guided_steps); the
        other steps use the conditional prediction alone, run the forward over the B conditional utterances only and cost the
        unguided step.  One interval per call, either solver; it needs `guidance` and `null_text_emb`.  Seeds, tags and noise are
        those of the call without it.
        `guidance_rescale` (None, a number in [0, 1], or one per utterance): guidance rescale (Lin et al. 2024, section 3.4) — at
        every guided step the guided prediction e = u + w (c - u) of utterance b is multiplied by s_b = 1 + phi_b (sigma_c / sigma_e -
        1), the standard deviations taken over the utterance's generated rows of this step's eps (csrc/guided_rescale.hip; fp64
        sums, an utterance's factor depends on its own rows only).  The step is ditto_guided_step_packed_rescale_opts (2M:
        ..._multistep_rescale_opts): the same forward, two small launches, and the same update with ce s_b (ke s_b).  It needs
        `guidance` and `null_text_emb`; phi_b = 0 gives utterance b the bits of the call without the argument; steps outside a
        `guidance_interval` rescale nothing.  None: the call as it was.
        `suffix_lengths` (list / tuple / int tensor [B], Q_b >= 0, P_b + Q_b <= N_b - 1): SPEECH INFILLING — the last Q_b rows of
        utterance b in `audio_emb` are clean latents too (the audio behind the part to re-synthesise); both contexts are written to
        both halves of x2 before the loop and come back bit-equal.  The G_b = N_b - P_b - Q_b rows in between start from x_T — with
        `seeds`, ditto_noise_normal(seed_b, 0xFFFFFFFF) over G_b rows; with `cond_by_audio`, those rows of `audio_emb` — and every
        step is one ditto_guided_step_packed_window_opts call (2M: ..._multistep_window_opts) whose update runs over the window
        alone.  Works without `prompt_lengths` (P = 0) and with guidance, seeds, noises, batch_class, both solvers and a
        `guidance_interval`; `guidance_rescale` with it raises NotImplementedError (the statistics run over prompt-to-end rows).  A
        model fills a window only if it was trained with spans anywhere (DiTTO.span_noise_packed(suffix_lengths=)); the effect on
        speech quality has not been measured.  None: the call as it was, whatever `prompt_lengths` is.
        `prediction`: "eps" (default: the call as it was) or "v" — the network's output is v = alpha z - sigma x0 (Salimans & Ho
        2022), the parameterisation a near-zero terminal SNR needs (Lin et al. 2024 section 3.2: x0 = alpha x - sigma v divides by
        nothing, where the eps form's 1 / alpha is ~100 at the cosine table's last timestep).  The loops, launches and kernels are
        the same: the updates are linear in the network's output and so is CFG, so a v step is the eps step with the coefficients
        of strided_schedule_v / multistep_schedule_v.  Every other argument works as above; `guidance_rescale` matches the standard
        deviations of the network's outputs as they are (v).  The model must have been trained on v (DiTTO.span_loss_packed(
        prediction="v")) and on this object's alphas_cumprod table; nothing here has been run with a trained model.
        `guidance_refresh` (None, or an int k >= 1): REUSE OF THE GUIDANCE DIRECTION — the unconditional forward runs at every k-th
        guided step only (the "CFG cache" of FasterCache, Lv et al. 2024, without its frequency reweighting).  refresh_plan gives
        the schedule: a refresh step is the guided step above, through ditto_guided_step_packed_reuse_opts (2M:
        ..._multistep_reuse_opts) in its STORE mode, which also keeps delta = c - u in one more buffer [S, d]; a reuse step runs the
        forward over the B conditional utterances alone — the forward of a step outside a `guidance_interval` — and updates with
        e = c + (w - 1) delta (LOAD mode); the first guided step of the call, and the first one behind unguided steps, is a refresh.
        By row counts the forward work of a fully guided loop falls to (k + 1) / (2 k).  It needs `guidance` and `null_text_emb`;
        None and 1 are the call as it was (the same entries, the same bits); with `guidance_rescale` it raises NotImplementedError
        (the statistics need u at every step: a follow-up).  Works with both solvers, prompts, suffixes, an interval,
        prediction="v", seeds / noises, cond_by_audio and batch_class.  This is an approximation of the guided trajectory, not
        another route to the same bits: what it costs in speech quality has not been measured with a trained model.
        `guidance_projection` (None, a number eta in [0, 1], or one per utterance): PROJECTED GUIDANCE — Adaptive Projected Guidance,
        Sadat, Hilliges & Weber 2024, Algorithm 1 (include/ditto_project.h states the arithmetic).  At every guided step the guidance
        direction is taken in x0 space, dd = ke (c - u), split into the part parallel to the conditional x0 prediction D_c = kx x + ke c
        and the part orthogonal to it, and the parallel part — what over-drives amplitude at a strong scale — is weighted by eta:
        eta = 1 is plain classifier-free guidance, eta = 0 keeps the orthogonal part alone.  `guidance_norm_threshold` (None, r > 0,
        or one per utterance) caps the direction: it is scaled by min(1, r / rms) with the RMS over the utterance's generated window
        — not the paper's whole-sample norm, which would make r depend on the utterance's length.  `guidance_momentum` (None, beta
        in (-1, 1), or one per utterance; the paper uses negative values) keeps a running direction m' = dd + beta m across the guided
        steps in one more buffer [S, d]; the first guided step starts it.  The last two need the first; all three need `guidance` and
        `null_text_emb`.  Every guided step is one ditto_guided_step_packed_project_opts call (2M: ..._multistep_project_opts): the
        same forward, one launch for the direction and its per-utterance fp64 sums, a small finish, and an update that reads x, c and
        the direction (csrc/guided_project.hip); an utterance's result depends on its own window only.  Works with both solvers,
        prediction "eps" and "v", prompts, suffixes, seeds / noises, per-utterance guidance and a `guidance_interval` (the steps
        outside run the unguided entry and leave the direction alone).  With `guidance_rescale` or `guidance_refresh` it raises
        NotImplementedError (follow-ups: a rescale of the projected prediction, a projection of the kept direction).  None: the call
        as it was — the same entries, the same bits.  Its effect on speech quality has not been measured with a trained model.
        Returns fp32 [S, d]."""
        if solver not in SOLVERS:
            raise ValueError(f"solver: one of {SOLVERS} is needed, got {solver!r}")
        validate_prediction(prediction)
        projection = projection_vectors(guidance_projection, guidance_norm_threshold, guidance_momentum, len(cu_seqlens) - 1)
        if projection is not None and (guidance is None or null_text_emb is None):
            raise ValueError("guidance_projection needs guidance= and null_text_emb=")
        if projection is not None and guidance_rescale is not None:
            raise NotImplementedError("guidance_projection= with guidance_rescale=: a rescale of the projected prediction is a follow-up")
        if projection is not None and guidance_refresh is not None:
            raise NotImplementedError("guidance_projection= with guidance_refresh=: a projection of the kept direction is a follow-up")
        interval = None if guidance_interval is None else validate_guidance_interval(guidance_interval, self.diffusion_steps)
        if interval is not None and (guidance is None or null_text_emb is None):
            raise ValueError("guidance_interval needs guidance= and null_text_emb=")
        if guidance_rescale is not None and (guidance is None or null_text_emb is None):
            raise ValueError("guidance_rescale needs guidance= and null_text_emb=")
        if guidance_rescale is not None and suffix_lengths is not None:
            raise NotImplementedError("guidance_rescale= with suffix_lengths=: the rescale statistics have no windowed form")
        refresh = validate_guidance_refresh(guidance_refresh)
        if refresh is not None and (guidance is None or null_text_emb is None):
            raise ValueError("guidance_refresh needs guidance= and null_text_emb=")
        if refresh is not None and guidance_rescale is not None:
            raise NotImplementedError("guidance_refresh= with guidance_rescale=: the rescale statistics need the unconditional "
                                      "prediction at every step; a rescale that reuses the kept direction is a follow-up")
        if refresh == 1:
            refresh = None                                       # every guided step refreshes: the loop as it was
        rescale = rescale_vector(guidance_rescale, len(cu_seqlens) - 1)
        multistep = solver == "dpmpp2m"
        if multistep and (eta != 0 or noises is not None):
            raise ValueError('solver="dpmpp2m" is deterministic: eta must be 0 and noises= cannot be given')
        require_fused_attention(self.ditto_model.cfg, "packed batches")
        from .varlen import pack, validate_cu_seqlens, validate_prompt_lengths, validate_suffix_lengths
        S, d = int(audio_emb.shape[0]), int(audio_emb.shape[1])
        B = len(cu_seqlens) - 1
        cu = validate_cu_seqlens(cu_seqlens, B, S, S, "cu_seqlens")
        N = int((cu[1:] - cu[:-1]).max())
        pl = None if prompt_lengths is None else validate_prompt_lengths(prompt_lengths, cu)
        ql = None if suffix_lengths is None else validate_suffix_lengths(suffix_lengths, cu, prompt_lengths)

        def context_kw(eng):
            """the step's prompt_len / suffix_len arguments"""
            kw = {} if pl is None else dict(prompt_len=pl.to(eng.device))
            if ql is not None:
                kw["suffix_len"] = ql.to(eng.device)
            return kw

        def entry_of(eng):
            return eng.guided_step_packed_multistep_ if multistep else eng.guided_step_packed_

        def begin_plain(eng, x2):
            """the step outside a guidance interval: the non-CFG entry on the conditional half of x2, with a conditioning image of
            the texts alone — what the call without guidance runs"""
            text = text_emb.to(eng.device).float().contiguous()
            ct = validate_cu_seqlens(text_cu_seqlens, B, int(text.shape[0]), int(text.shape[0]), "text_cu_seqlens")
            return functools.partial(entry_of(eng), x2[:S], eng.prepare_text_packed(text, ct), B=B,
                                     offsets=eng.guided_offsets_packed(cu, S, N, False), **context_kw(eng))

        def begin_reuse(eng, x2, step, delta):
            """the steps of a loop with guidance_refresh: the STORE entry bound to what `step` (begin's) is bound to, the LOAD
            entry bound to what begin_plain's step is bound to, and that step itself"""
            from .hip import REUSE_LOAD, REUSE_STORE
            entry = eng.guided_step_packed_multistep_reuse_ if multistep else eng.guided_step_packed_reuse_
            plain = begin_plain(eng, x2)
            return (functools.partial(entry, *step.args, delta=delta, mode=REUSE_STORE, **step.keywords),
                    functools.partial(entry, *plain.args, delta=delta, mode=REUSE_LOAD, **plain.keywords), plain)

        def begin(eng, cfg, seeds):
            entry = entry_of(eng)
            if projection is not None and cfg:                   # (no guided step at all: the call without guidance)
                entry = eng.guided_step_packed_multistep_project_ if multistep else eng.guided_step_packed_project_
            if null_text_cu_seqlens is not None and guidance is None:
                raise ValueError("null_text_cu_seqlens without guidance")
            text = text_emb.to(eng.device).float()
            S_T = int(text.shape[0])
            ct = validate_cu_seqlens(text_cu_seqlens, B, S_T, S_T, "text_cu_seqlens")
            if cfg:
                null = null_text_emb.to(eng.device).float()
                if null_text_cu_seqlens is None:
                    null, cn = null.expand_as(text), ct
                else:
                    cn = validate_cu_seqlens(null_text_cu_seqlens, B, int(null.shape[0]), int(null.shape[0]), "null_text_cu_seqlens")
                text = torch.cat([text, null], dim=0).contiguous()
                ct = torch.cat([ct, ct[-1] + cn[1:]])
            cond = eng.prepare_text_packed(text, ct)
            offsets = eng.guided_offsets_packed(cu, S, N, cfg)
            x2 = torch.empty(2 * S if cfg else S, d, dtype=torch.float32, device=eng.device)
            if pl is not None or ql is not None:
                x2[:S].copy_(audio_emb)                          # the contexts (and, with cond_by_audio, the start of the rest)
                if not cond_by_audio:
                    p0 = pl if pl is not None else torch.zeros(B, dtype=torch.int32)
                    q0 = ql if ql is not None else torch.zeros(B, dtype=torch.int32)
                    gl = (cu[1:] - cu[:-1] - p0 - q0).tolist()   # generated rows per utterance, and where they sit in the batch
                    at = torch.cat([torch.arange(int(cu[b]) + int(p0[b]), int(cu[b + 1]) - int(q0[b]))
                                    for b in range(B)]).to(eng.device)
                    if seeds is not None:                        # x_T of an unprompted utterance of G_b rows with that seed
                        xt = torch.empty(B, max(gl), d, dtype=torch.float32, device=eng.device)
                        eng.noise_normal_(xt, seeds, 0xFFFFFFFF)
                        xt = pack(xt, gl)[0]
                    else:
                        xt = torch.randn(len(at), d, dtype=torch.float32, device=eng.device)
                    x2[:S].index_copy_(0, at, xt)
                return x2, N, functools.partial(entry, x2, cond, B=B, offsets=offsets, **context_kw(eng))
            if seeds is not None and not cond_by_audio:
                # x_T: ditto_noise_normal over the padded [B, N, d] (the numbers of sample_guided(seeds=)), packed row by row
                xt = torch.empty(B, N, d, dtype=torch.float32, device=eng.device)
                eng.noise_normal_(xt, seeds, 0xFFFFFFFF)
                x2[:S].copy_(pack(xt, (cu[1:] - cu[:-1]).tolist())[0])
            else:
                x2[:S].copy_(torch.randn_like(audio_emb.float()) if not cond_by_audio else audio_emb)
            return x2, N, functools.partial(entry, x2, cond, B=B, offsets=offsets)

        pj = {} if projection is None else dict(projection=projection)   # None: the loops are called as they were
        if multistep:
            return self._multistep_loop(B, guidance, null_text_emb, n_steps, seeds, batch_class, begin, interval, begin_plain, rescale,
                                        prediction, refresh, begin_reuse, **pj)
        return self._guided_loop(B, guidance, null_text_emb, n_steps, eta, seeds, noises, batch_class, begin, interval, begin_plain,
                                 rescale, prediction, refresh, begin_reuse, **pj)

    def guided_stream(self, *, max_rows, max_utterances, max_text_rows, guided=True, class_rows=None, solver="ddim", infill=False,
                      prediction="eps", refresh=False, project=False):
        """A request stream over this model (ditto_tts_amd/serving.py GuidedStream): submit(text_emb, n_frames, ...) queues an
        utterance, step() admits what fits, runs one guided strided step over everything in flight — each utterance at its own
        index of its own strided_schedule — and returns the finished ones.  `max_rows` / `max_utterances` / `max_text_rows`: the
        speech rows, utterances and conditioning rows (text, plus null text under guidance) in flight at once; every buffer is
        sized from them here.  `class_rows`: hip.CallOpts(class_rows=) of every step (else the thread's hip.batch_class scope).
        `solver`: "ddim", or "dpmpp2m" — every request of the stream then runs multistep_schedule (sample_guided_packed(solver=));
        one solver per stream.
        `infill`: the stream accepts submit(..., suffix=[Q, d]) — speech infilling, clean rows behind the generated frames as
        `prompt` puts them in front (sample_guided_packed(suffix_lengths=)) — and refuses guidance_interval= / guidance_rescale=.
        False: the stream as it was.
        `prediction`: "eps", or "v" — every request's per-step coefficients come from strided_schedule_v / multistep_schedule_v
        (sample_guided_packed(prediction=)); one parameterisation per stream, as a stream serves one model.  Admission, tags and
        launches are unchanged.
        `refresh`: the stream accepts submit(..., guidance_refresh=k) — reuse of the guidance direction between refresh steps, each
        request on refresh_plan's schedule of its own guided steps (sample_guided_packed(guidance_refresh=)) — and holds the kept
        directions beside the state.  A guided "ddim" stream without infill only: guided=False is a ValueError, solver="dpmpp2m"
        and infill=True are NotImplementedError (follow-ups, like guidance_rescale with it).  False: the stream as it was.  What
        the approximation costs in speech quality has not been measured with a trained model.
        `project`: the stream accepts submit(..., guidance_projection=, guidance_norm_threshold=, guidance_momentum=) — projected
        guidance, each request with its own eta, r and beta (sample_guided_packed(guidance_projection=)) — and holds the directions
        m' beside the state.  A guided "ddim" stream without infill and without refresh only: guided=False is a ValueError, the
        others are NotImplementedError (follow-ups, like guidance_rescale with it).  False: the stream as it was.  Its effect on
        speech quality has not been measured with a trained model."""
        if solver not in SOLVERS:
            raise ValueError(f"solver: one of {SOLVERS} is needed, got {solver!r}")
        validate_prediction(prediction)
        from .serving import DeviceBatch, GuidedStream, validate_project_stream, validate_refresh_stream
        refresh = validate_refresh_stream(refresh, bool(guided), solver, bool(infill))
        project = validate_project_stream(project, bool(guided), solver, bool(infill), refresh)
        require_fused_attention(self.ditto_model.cfg, "request streams (packed batches)")
        eng = self.ditto_model.engine(torch.empty(0, device=self.device).device)
        batch = DeviceBatch(eng, max_rows=max_rows, max_utterances=max_utterances, max_text_rows=max_text_rows, guided=guided,
                            class_rows=class_rows, solver=solver, infill=infill, refresh=refresh,
                            project=project)
        return GuidedStream(batch, self.alphas_cumprod, max_rows=max_rows, max_utterances=max_utterances,
                            max_text_rows=max_text_rows, guided=guided, text_dim=eng.cfg.text_dim, hidden_dim=eng.cfg.hidden_dim,
                            solver=solver, infill=infill, prediction=prediction, refresh=refresh, project=project)

    # public aliases (the mangled names above are what the reference's own code reaches)
    def p_sample(self, x, t, text_emb, noise=None):
        return self.__p_sample(x, t, text_emb, noise)

    def sample_latents(self, text_emb, audio_emb, **kw):
        return self.__sample_latents(text_emb, audio_emb, **kw)

    # ---------------------------------------------------------------- around the loop (out of scope: delegated)
    def _need(self, what, obj):
        if obj is None:
            raise RuntimeError(f"SpeechGenerator.{what} is not available: the codec / vocoder / tokenizer stack is "
                               "outside the MI355X denoise path (SURVEY.md §2) and was not injected")
        return obj

    @torch.no_grad()
    def predict_frames(self, z_text, z_audio, *, frame_rate, audio_lengths=None, text_lengths=None,
                       seconds_of_class=None):
        """Frames to generate for every utterance of a (variable-length) batch, from the speech-length predictor: a list of B
        ints, ready for `stream.submit(text_emb, n_frames, ...)` and `sample_guided_packed`.

        z_text [B,T,d] / z_audio [B,S,d] are the encoder outputs `SLP.decode` takes, `audio_lengths` / `text_lengths` its
        per-utterance lengths (see there, also for what `text_lengths=None` means to a reference-trained checkpoint).
        class -> seconds is `seconds_of_class(c)` when given, else MIN_AUDIO_DURATION + c: the inverse of the reference's label
        `int(duration - 10)` (src/utils/MLS.py:77).  n_frames = round(seconds * frame_rate); `frame_rate` (latent frames per
        second of the codec in use) has no default: nothing here knows the codec."""
        slp = self._need("slp", self.slp)
        if isinstance(frame_rate, bool) or not isinstance(frame_rate, (int, float)) or not frame_rate > 0:
            raise ValueError(f"frame_rate must be a positive number of latent frames per second, got {frame_rate!r}")
        classes = slp.predict_class(z_text, z_audio, audio_lengths=audio_lengths, text_lengths=text_lengths)
        if seconds_of_class is None:
            from .shipped_config import config_classes
            t0 = config_classes()[1].MIN_AUDIO_DURATION
            seconds_of_class = lambda c: t0 + c   # noqa: E731
        return [int(round(float(seconds_of_class(int(c))) * frame_rate)) for c in classes.tolist()]

    @torch.no_grad()
    def generate_speech_from_audio_tensor(self, audio_tensor, padding_mask_audio, text_prompt, is_tokenized=False,
                                          is_slp=False, cond_by_audio=False):
        """Reference :93-111, using the caller-provided codec (`ditto_model.nac`) and vocoder."""
        nac = self._need("ditto_model.nac", self.ditto_model.nac)
        audio_latents, audio_scales = nac.audio_encoder(audio_tensor, padding_mask_audio)
        max_length = nac.language_model.config.n_positions
        audio_latents = audio_latents[:, :, :max_length].mean(dim=1)
        if not is_tokenized:
            tok = self._need("text_tokenizer", self.text_tokenizer)
            text_tokens = tok(text_prompt, return_tensors="pt").input_ids.to(self.device)
        else:
            text_tokens = text_prompt
        text_tokens = text_tokens[:, :max_length]
        text_embeddings = nac.language_model.transformer.wte(text_tokens)
        t = torch.full((audio_latents.size(0),), self._loop_steps() - 1, device=self.device, dtype=torch.long)  # :105
        audio_latents = self.ditto_model.q_sample(audio_latents, t)
        refined = self.__sample_latents(text_embeddings, audio_latents, text_tokens, audio_tensor, is_slp, cond_by_audio)
        return self.__generate_speech_from_latents(refined, audio_scales, padding_mask_audio)

    @torch.no_grad()
    def __generate_speech_from_latents(self, audio_latents, audio_scales, padding_mask_audio):
        """Reference :114-128 (VQ -> EnCodec decode -> mel -> vocoder), all delegated."""
        nac = self._need("ditto_model.nac", self.ditto_model.nac)
        vocoder, mel_fn = self._need("vocoder", self.vocoder), self._need("mel_fn", self.mel_fn)
        audio_latents = audio_latents.unsqueeze(1).repeat(1, 2, 1, 1)
        q = nac.vector_quantizer(audio_latents)
        waveform = nac.audio_decoder.decode(q.unsqueeze(0).detach(), audio_scales=audio_scales,
                                            padding_mask=padding_mask_audio)[0].squeeze(1)
        return vocoder(mel_fn(waveform, vocoder.h).to(self.device)).squeeze(0)

    def generate_speech_from_file(self, file_path, text_prompt, cond_by_audio=False):
        raise RuntimeError("generate_speech_from_file needs torchaudio + the EnCodec processor, which are outside the "
                           "denoise path; load the audio yourself and call generate_speech_from_audio_tensor")
