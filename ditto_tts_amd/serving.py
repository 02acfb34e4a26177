"""Continuous batching for guided strided sampling: utterances join and leave a packed batch between steps.

`sample_guided_packed` serves a closed batch: every utterance starts at step 0, runs the same `n_steps` and `eta`, and the call
returns when the last one is done.  A `GuidedStream` holds a queue of requests and a packed batch in flight; each `step()` admits
what fits (strictly FIFO), runs ONE library call over everything in flight — every utterance at its own index of its own
`strided_schedule` — and hands back the utterances that have run all their steps.  Under a pinned kernel class an utterance's bits
depend on its own rows and lengths only, so it comes out exactly as `sample_guided_packed` samples it alone.

Two layers:
  * `GuidedStream`: the scheduler.  Host arithmetic only (queue, capacities, schedules, offsets); it drives a batch object through
    three calls (`regroup`, `step`, `retire`) and never touches the device itself.
  * `DeviceBatch`: the packed batch on one GPU.  State, conditioning, offsets and the per-step arguments live in buffers sized once
    from the capacities; membership changes run in ONE launch of ditto_regroup_packed driven by a segment table, the step is
    ditto_guided_step_packed_tags_opts.  Nothing synchronises the device; steady-state steps allocate nothing.
Guidance intervals (submit(guidance_interval=)): a request is guided only at the steps whose timestep lies in its interval, so a
step's guided set G may be a part of the batch.  The unconditional copies of G are compacted behind the S speech rows, a change of G
is a regroup like any membership change, and the step is ditto_guided_step_packed_mixed_opts (G everyone / nobody: the entries above
with cfg 1 / 0).
Guidance rescale (submit(guidance_rescale=)): each request's blend factor phi rides in the step block; a step in which a guided
request has phi > 0 runs the ..._rescale_opts form of its entry — the same forward and update, with the two statistics launches of
csrc/guided_rescale.hip in between — over a scratch sized once from the capacities.
Speech infilling (guided_stream(infill=True), submit(suffix=)): a request may carry clean rows BEHIND its generated frames as well;
each request's suffix length rides in the step block and a step with a suffixed request in flight runs the ..._window_opts form of
its entry (csrc/guided_packed.hip, csrc/guided_multistep.hip).  Such a stream has no guidance intervals and no guidance rescale.
Guidance reuse (guided_stream(refresh=True), submit(guidance_refresh=k)): a request runs the unconditional forward at every k-th of
its guided steps only and reuses the kept direction delta = c - u in between (sampler.refresh_plan, computed per request at submit).
A step's set G is then the REFRESHING requests; the batch holds the directions in two more buffers that a regroup carries along, and
a step with a k > 1 request in flight is ditto_guided_step_packed_refresh_opts (csrc/guided_refresh.hip): refreshing, reusing and
plain utterances in one forward and one update.  "ddim" streams without infill; what the approximation costs in speech quality is
not measured by anything here.
Projected guidance (guided_stream(project=True), submit(guidance_projection=, guidance_norm_threshold=, guidance_momentum=)): a request
carries its own eta, r and beta, and its ditto_project_coef row of every step (sampler.project_table for that utterance alone,
computed at submit).  A step's kinds are 3 projected, 1 guided without projection, 0 plain; G is the guided ones of either kind; the
batch holds the directions m' in two more buffers — a regroup carries the one of every projected survivor between two of its guided
steps — and a step at which a request is projected is ditto_guided_step_packed_project_mixed_opts (csrc/guided_project_mixed.hip).
"ddim" streams without infill, refresh and guidance rescale.  Measured on one MI355X at C2 in a steady-state stream kept at B = 32
(profiles/stream_project_bench.json): 17.05 ms per step (16.97 - 17.36) without project=True, 17.02 ms (16.86 - 17.31) with it and
nobody projected, 17.08 ms (16.97 - 17.32) with every request projected: differences inside the round-to-round range.  Its effect
on speech quality is not measured by anything here; "dpmpp2m" streams, infill streams, rescale, reuse and the padded entries remain
follow-ups.
They serve the reference's sampling loop (reference src/model/SpeechGenerator.py:130-164) to a request stream.
"""
from __future__ import annotations

import collections
import ctypes as C
import math
from typing import List, Optional

import numpy as np
import torch

from . import hip
from .engine import _stream


class StreamHandle:
    """What `submit` returns and `step` hands back with the result."""
    __slots__ = ("id",)

    def __init__(self, id_: int):
        self.id = id_

    def __repr__(self):
        return f"StreamHandle({self.id})"


class Request:
    """One utterance of a stream: what was submitted, and where it stands (index `i` of its schedule; its slot `b`, speech row
    `row` and conditioning rows `trow` / `nrow` in the batch's CURRENT buffers once admitted).  `prompt` ([P, d] or None): the
    speech prompt that stands in front of the `n_frames` generated rows, `suffix` ([Q, d] or None) the clean rows behind them (speech
    infilling); the utterance occupies `rows` = P + n_frames + Q rows."""
    __slots__ = ("handle", "text", "null", "T", "T_null", "n_frames", "seed", "w", "n_steps", "eta", "x_T", "schedule", "i", "b",
                 "row", "trow", "nrow", "prompt", "P", "interval", "in_g", "ntm", "phi", "suffix", "Q", "kinds", "period", "pcoef")

    def __init__(self, handle, text, null, n_frames, seed, w, n_steps, eta, x_T, schedule, prompt=None, interval=None, phi=0.0,
                 suffix=None, kinds=None, period=1, pcoef=None):
        self.handle, self.text, self.null = handle, text, null
        # projected guidance: `pcoef` — fp32 [n_steps, 8], the request's ditto_project_coef of every step of its schedule
        # (sampler.project_table's rows for this utterance alone); None: the request is not projected
        self.pcoef = pcoef
        # guidance reuse: `kinds` — hip.KIND_* of every step of its schedule (refresh_plan's list; None: from guided_now()) —
        # and the refresh `period` k it was made with (1: every guided step refreshes)
        self.kinds, self.period = kinds, int(period)
        self.suffix, self.Q = suffix, 0 if suffix is None else int(suffix.shape[0])
        self.phi = float(phi)                        # guidance rescale: the blend factor in [0, 1]; 0 = none
        # `interval`: None, or (t_lo, t_hi) — guided only at the steps whose timestep lies in it.  `in_g`: whether the batch's current
        # layout holds its unconditional copy (None before its first regroup); `ntm`: the tmod row of its null text there
        self.interval, self.in_g, self.ntm = interval, None, None
        self.prompt, self.P = prompt, 0 if prompt is None else int(prompt.shape[0])
        self.T, self.T_null = int(text.shape[0]), 0 if null is None else int(null.shape[0])
        self.n_frames, self.seed, self.w, self.n_steps, self.eta, self.x_T = n_frames, seed, w, n_steps, eta, x_T
        self.schedule, self.i = schedule, 0
        self.b = self.row = self.trow = self.nrow = None

    @property
    def text_rows(self) -> int:
        return self.T + self.T_null

    def guided_now(self) -> bool:
        """whether the step it stands at applies the guidance: always without an interval, else t_lo <= tau <= t_hi"""
        return self.interval is None or self.interval[0] <= self.schedule[self.i][0] <= self.interval[1]

    def kind_now(self) -> int:
        """hip.KIND_* of the step it stands at: plain where it is not guided, else refresh (it runs the unconditional forward and
        keeps the direction) or reuse (guidance reuse, between two refresh steps)"""
        if self.kinds is not None:
            return self.kinds[self.i]
        return hip.KIND_REFRESH if self.guided_now() else hip.KIND_PLAIN

    def project_kind_now(self) -> int:
        """the kind of the step it stands at in a stream made with project=True: hip.KIND_PROJECT where it is guided and carries a
        projection, hip.KIND_CFG where it is guided without one, else hip.KIND_PLAIN"""
        if self.kind_now() == hip.KIND_PLAIN:
            return hip.KIND_PLAIN
        return hip.KIND_PROJECT if self.pcoef is not None else hip.KIND_CFG

    def carries_direction(self) -> bool:
        """whether a regroup in front of the step it stands at has to take its direction m' along: it is projected, has had a
        guided step (which wrote m') and has one to come (which reads it, whatever lies in between)"""
        return self.pcoef is not None and any(self.kinds[:self.i]) and any(self.kinds[self.i:])

    @property
    def rows(self) -> int:
        return self.P + self.n_frames + self.Q


class Plan:
    """A membership change: `members` (Requests in their new order: the survivors in their old order, then the newcomers in
    admission order), which of them are `newcomers`, and the new layout — `cu` speech offsets [B + 1], `cu_text` / `cu_null` text
    offsets [B + 1] (cu_null None without guidance).
    Under guidance `in_g` [B] says which members are guided at the coming step (the set G; default: everyone).  Their unconditional
    copies are compacted behind the S rows in batch order: `partner` [B] (the copy's index in [0, |G|), or -1), `cu_g` [|G| + 1] the
    copies' offsets, `offsets` = [cu; S + cu_g[1:]] and `text_offsets` = [cu_text; T + cu_null_g[1:]] what the step's forward
    reads.  The null conditioning of a member outside G is parked behind G's: `null_row` / `null_tm` [B] are each member's null K/V
    row (counted from the T text rows) and tmod row (counted from the B text ones) — G's first, in order, then the parked ones.
    `kind` [B] (guidance reuse; else None): hip.KIND_* of each member's coming step — G is then the refreshing members, and a
    survivor about to reuse takes its kept direction along.
    `carry` [B] (projected guidance; else None): which members take their direction m' along (Request.carries_direction)."""
    __slots__ = ("members", "newcomers", "cu", "cu_text", "cu_null", "in_g", "partner", "cu_g", "offsets", "text_offsets", "null_row",
                 "null_tm", "kind", "carry")

    def __init__(self, members, newcomers, guided, in_g=None, kind=None, carry=None):
        self.members, self.newcomers = list(members), list(newcomers)
        self.kind = None if kind is None else list(kind)
        self.carry = None if carry is None else [bool(f) for f in carry]
        self.cu, self.cu_text = _cumulate(r.rows for r in members), _cumulate(r.T for r in members)
        self.cu_null = _cumulate(r.T_null for r in members) if guided else None
        self.in_g = self.partner = self.cu_g = self.null_row = self.null_tm = None
        self.offsets, self.text_offsets = self.cu, self.cu_text
        if guided:
            self.in_g = [True] * len(self.members) if in_g is None else [bool(f) for f in in_g]
            self.partner = partner_table(self.in_g)
            order = [j for j, f in enumerate(self.in_g) if f] + [j for j, f in enumerate(self.in_g) if not f]
            G = sum(self.in_g)
            self.cu_g = _cumulate(self.members[j].rows for j in order[:G])
            at = _cumulate(self.members[j].T_null for j in order)
            self.null_row, self.null_tm = [0] * len(order), [0] * len(order)
            for k, j in enumerate(order):
                self.null_row[j], self.null_tm[j] = at[k], k
            self.offsets = self.cu + [self.cu[-1] + c for c in self.cu_g[1:]]
            self.text_offsets = self.cu_text + [self.cu_text[-1] + c for c in at[1:G + 1]]


class StepArgs:
    """One step over the batch in flight: per-utterance lists in slot order.  `coef` (solver "dpmpp2m" only, else None): each
    utterance's (a, kx, ke, b, g, use_prev) of its own multistep_schedule; a, ce, cz and tags are then None.  Under guidance
    `in_g` [B] says who is guided at this step (each request's guided_now(), asked once), `partner` [B] is its partner_table,
    `G` the number of guided utterances and `S_G` their rows (None, None, 0, 0 unguided).  `phi` [B]: each utterance's guidance-rescale
    blend factor (0: none).  `suffix` [B]: each utterance's suffix rows (speech infilling; 0: none).
    `kind` [B] (None unguided): hip.KIND_* of each utterance's step — plain, refresh or reuse; `in_g` is kind == refresh, "has an
    unconditional copy in this step's forward".  `period` [B]: each utterance's refresh period k (1: it never reuses).
    A stream made with project=True: `kind` [B] is hip.KIND_PLAIN / KIND_CFG / KIND_PROJECT, `in_g` is kind != plain, and `proj` [B]
    holds each utterance's ditto_project_coef of this step as 8 fp32 words (None: it carries no projection)."""
    __slots__ = ("B", "S", "max_N", "S_T", "max_T", "t", "a", "ce", "cz", "w", "tags", "seeds", "handles", "prompt", "coef", "in_g",
                 "partner", "G", "S_G", "phi", "suffix", "kind", "period", "proj")


def _cumulate(lengths) -> List[int]:
    out = [0]
    for n in lengths:
        out.append(out[-1] + int(n))
    return out


def partner_table(in_g) -> List[int]:
    """partner[b]: the index of utterance b's unconditional copy among the guided ones, in batch order, or -1"""
    out, g = [], 0
    for f in in_g:
        out.append(g if f else -1)
        g += bool(f)
    return out


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def validate_refresh_stream(refresh, guided: bool, solver: str, infill: bool) -> bool:
    """`refresh` of a stream as a bool; a stream that cannot serve guidance reuse is refused here, before anything is made"""
    if not refresh:
        return False
    if not guided:
        raise ValueError("refresh=True needs a guided stream: guidance reuse keeps the direction of classifier-free guidance")
    if solver != "ddim":
        raise NotImplementedError(f"refresh=True is served by \"ddim\" streams; this stream's solver is {solver}: there is no mixed "
                                  "multistep update (a follow-up)")
    if infill:
        raise NotImplementedError("refresh=True with infill=True: there is no mixed multistep update and the three-kind update has "
                                  "no windowed form (a follow-up)")
    return True


def validate_project_stream(project, guided: bool, solver: str, infill: bool, refresh: bool) -> bool:
    """`project` of a stream as a bool; a stream that cannot serve projected guidance is refused here, before anything is made"""
    if not project:
        return False
    if not guided:
        raise ValueError("project=True needs a guided stream: projected guidance reshapes the direction of classifier-free guidance")
    if solver != "ddim":
        raise NotImplementedError(f"project=True is served by \"ddim\" streams; this stream's solver is {solver}: a regroup has no "
                                  "slot left for the direction beside the multistep history (a follow-up)")
    if infill:
        raise NotImplementedError("project=True with infill=True: the mixed projected update has no windowed form (a follow-up)")
    if refresh:
        raise NotImplementedError("project=True with refresh=True: a projection of the kept direction is a follow-up")
    return True


class GuidedStream:
    """stream = sg.guided_stream(max_rows=, max_utterances=, max_text_rows=, guided=True | False, class_rows=None, infill=False,
                              refresh=False, project=False)
    h = stream.submit(text_emb [T_b, text_dim], n_frames, seed=, guidance=, null_text_emb=, n_steps=25, eta=0.0, x_T=None,
                      prompt=None, guidance_interval=None, guidance_rescale=None, suffix=None, guidance_refresh=None,
                      guidance_projection=None, guidance_norm_threshold=None, guidance_momentum=None)
    done = stream.step()          # [(handle, latents fp32 [n_frames, d] on the GPU), ...]
    stream.pending, stream.active, stream.drain()

    Capacities: `max_rows` speech rows, `max_utterances` utterances and `max_text_rows` rows of the conditioning (text rows, plus
    the null-text rows under guidance) in flight at once.  `guided=True`: every request carries `guidance` and `null_text_emb`;
    `guided=False`: none does (a mix would waste the unconditional half of the doubled batch).
    x_T of a request: `x_T` when given, else Philox of its `seed` at tag 0xFFFFFFFF — ditto_noise_normal's numbers, what
    sample_guided_packed(seeds=) starts from.  Every step's z is Philox of the seed at the step's tag.  `seed=None` draws one from
    torch's default CPU generator at submit.
    `prompt` (floating [P, d], P >= 1): a speech prompt — the target speaker's clean latents, kept in front of the `n_frames`
    generated rows at every step (sample_guided_packed(prompt_lengths=)).  The request then occupies P + n_frames of `max_rows`;
    `x_T` stays [n_frames, d] and so does the result.
    `solver` (one per stream): "ddim" — each request at its own index of its own strided_schedule — or "dpmpp2m": of its own
    multistep_schedule (sample_guided_packed(solver="dpmpp2m")); requests then need eta = 0 and their seeds give x_T only.
    `guidance_interval` (a guided "ddim" stream; None or (t_lo, t_hi)): the request is guided only at the steps of its schedule
    whose timestep lies in the interval (sample_guided_packed(guidance_interval=)); at the others it takes no part in the
    unconditional forward.  It counts against the capacities like any guided request, at every step.
    `guidance_rescale` (a guided stream, either solver; None or a number in [0, 1]): the request's guidance-rescale blend factor
    (sample_guided_packed(guidance_rescale=)), applied at the steps at which it is guided.
    `suffix` (a stream made with infill=True only; floating [Q, d], Q >= 1): speech infilling — clean latents kept BEHIND the
    `n_frames` generated rows at every step, as `prompt` is kept in front (sample_guided_packed(suffix_lengths=)).  The request
    occupies P + n_frames + Q of `max_rows`; `x_T` and the result stay [n_frames, d].  An infill stream refuses
    `guidance_interval` and `guidance_rescale` (NotImplementedError: neither update has a windowed form); with no suffixed request in
    flight it runs the entries a plain stream runs.
    `prediction` (one per stream): "eps", or "v" — the requests' coefficients come from strided_schedule_v / multistep_schedule_v
    (sample_guided_packed(prediction="v")); nothing else changes.
    `guidance_refresh` (a stream made with refresh=True only — guided, "ddim", no infill; None or an int k >= 1): reuse of the
    guidance direction (sample_guided_packed(guidance_refresh=)) — the request takes part in the unconditional forward at every
    k-th of its guided steps only and reuses the direction it kept there in between.  Its step kinds are refresh_plan of its own
    guided steps, fixed at submit: interval-aware, the counter reset by an unguided step, the first guided step a refresh.  None
    and 1: every guided step refreshes, the request as it was.  k > 1 with guidance_rescale > 0 raises NotImplementedError, as in
    the closed call; so does any guidance_rescale > 0 in a refresh=True stream, where the request could share a step with a
    reusing one.  An approximation of the guided trajectory: its effect on speech quality has not been measured.
    `guidance_projection`, `guidance_norm_threshold`, `guidance_momentum` (a stream made with project=True only — guided, "ddim", no
    infill, no refresh; None, or eta in [0, 1], r > 0, beta in (-1, 1)): projected guidance (sample_guided_packed(guidance_projection=))
    — sampler.projection_vectors' ranges and errors; the last two need the first.  The request is projected at its guided steps,
    interval-aware, the momentum kept across unguided ones; requests without the arguments keep their bits.  Any guidance_rescale > 0
    in such a stream raises NotImplementedError.  Measured at C2, B = 32 in steady state: 17.08 ms per step with every request
    projected against 17.05 ms in a stream made without project=True (profiles/stream_project_bench.json), inside the round-to-round
    range.  Its effect on speech quality has not been measured; "dpmpp2m" streams, infill streams, rescale, reuse and the padded
    entries remain follow-ups."""

    def __init__(self, batch, alphas_cumprod: torch.Tensor, *, max_rows: int, max_utterances: int, max_text_rows: int, guided: bool,
                 text_dim: int, hidden_dim: int, solver: str = "ddim", infill: bool = False, prediction: str = "eps",
                 refresh: bool = False, project: bool = False):
        from .sampler import SOLVERS, validate_prediction
        if solver not in SOLVERS:
            raise ValueError(f"solver: one of {SOLVERS} is needed, got {solver!r}")
        self.refresh = validate_refresh_stream(refresh, bool(guided), solver, bool(infill))
        self.project = validate_project_stream(project, bool(guided), solver, bool(infill), self.refresh)
        self.solver, self.infill = solver, bool(infill)
        self.prediction = validate_prediction(prediction)
        for name, v in (("max_rows", max_rows), ("max_utterances", max_utterances), ("max_text_rows", max_text_rows)):
            if not _is_int(v) or v < 1:
                raise ValueError(f"{name}: a positive int is needed, got {v!r}")
        self.batch, self.guided = batch, bool(guided)
        self.max_rows, self.max_utterances, self.max_text_rows = max_rows, max_utterances, max_text_rows
        self.text_dim, self.hidden_dim = int(text_dim), int(hidden_dim)
        self._acp = alphas_cumprod.detach().double().cpu()
        self._schedules = {}                       # (n_steps, eta) -> strided_schedule
        self._x0_rows = {}                         # n_steps -> multistep_schedule: the (kx, ke) of projected guidance
        self._queue: collections.deque = collections.deque()
        self._active: List[Request] = []
        self._dirty = False                        # utterances left since the last regroup: the buffers have holes
        self._next_id = 0

    # ------------------------------------------------------------------ the public surface
    @property
    def pending(self) -> int:
        """requests submitted and not yet admitted"""
        return len(self._queue)

    @property
    def active(self) -> int:
        """utterances in flight"""
        return len(self._active)

    def _schedule(self, n_steps: int, eta: float):
        key = (n_steps, eta)
        if key not in self._schedules:
            from .sampler import multistep_schedule, multistep_schedule_v, strided_schedule, strided_schedule_v
            v = self.prediction == "v"                                 # the same row layouts: (a_v, cv) for (a, ce), v-form (kx, ke)
            self._schedules[key] = ((strided_schedule_v if v else strided_schedule)(self._acp, n_steps, eta) if self.solver == "ddim"
                                    else (multistep_schedule_v if v else multistep_schedule)(self._acp, n_steps))
        return self._schedules[key]

    def _x0_schedule(self, n_steps: int):
        """the multistep schedule over a request's timesteps, whose (kx, ke) map the network's output to x0: what the closed call
        hands project_table"""
        if n_steps not in self._x0_rows:
            from .sampler import multistep_schedule, multistep_schedule_v
            self._x0_rows[n_steps] = (multistep_schedule_v if self.prediction == "v" else multistep_schedule)(self._acp, n_steps)
        return self._x0_rows[n_steps]

    def _text(self, t, name):
        if not isinstance(t, torch.Tensor) or not t.dtype.is_floating_point:
            raise ValueError(f"{name}: a floating-point tensor [rows, {self.text_dim}] is needed")
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] != self.text_dim:
            raise ValueError(f"{name}: shape [rows >= 1, {self.text_dim}] expected, got {list(t.shape)}")
        return t.detach()

    def submit(self, text_emb, n_frames, *, seed=None, guidance=None, null_text_emb=None, n_steps=25, eta=0.0, x_T=None,
               prompt=None, guidance_interval=None, guidance_rescale=None, suffix=None, guidance_refresh=None,
               guidance_projection=None, guidance_norm_threshold=None, guidance_momentum=None) -> StreamHandle:
        """Queue one utterance.  Everything is validated here, on the host: a bad request raises ValueError and leaves the stream as
        it was; so does one that could never fit the capacities."""
        text = self._text(text_emb, "text_emb")
        if not _is_int(n_frames) or n_frames < 1:
            raise ValueError(f"n_frames: a positive int is needed, got {n_frames!r}")
        if not _is_int(n_steps):
            raise ValueError(f"n_steps: an int is needed, got {n_steps!r}")
        if isinstance(eta, bool) or not isinstance(eta, (int, float)) or not math.isfinite(eta) or eta < 0:
            raise ValueError(f"eta: a finite number >= 0 is needed, got {eta!r}")
        if self.solver != "ddim" and eta != 0:
            raise ValueError(f"this stream's solver ({self.solver}) is deterministic: eta must be 0, got {eta!r}")
        schedule = self._schedule(n_steps, float(eta))             # (ValueError unless 1 <= n_steps <= diffusion_steps)
        if self.guided:
            if guidance is None or null_text_emb is None:
                raise ValueError("this stream is guided: every request needs guidance= and null_text_emb=")
            if isinstance(guidance, bool) or not isinstance(guidance, (int, float)) or not math.isfinite(guidance):
                raise ValueError(f"guidance: a finite number is needed, got {guidance!r}")
            null = self._text(null_text_emb, "null_text_emb")
        else:
            if guidance is not None or null_text_emb is not None:
                raise ValueError("this stream is unguided: a request with guidance= or null_text_emb= belongs in a guided stream")
            null = None
        if suffix is not None and not self.infill:
            raise ValueError("suffix= needs a stream made with infill=True (guided_stream(infill=True))")
        if self.infill and (guidance_interval is not None or guidance_rescale is not None):
            raise NotImplementedError("an infill stream serves neither guidance_interval= nor guidance_rescale=: the mixed and the "
                                      "rescale kernels have no windowed form")
        interval = None
        if guidance_interval is not None:
            if not self.guided:
                raise ValueError("this stream is unguided: guidance_interval= belongs in a guided stream")
            if self.solver != "ddim":
                raise NotImplementedError(f"guidance_interval= is served by \"ddim\" streams; this stream's solver is {self.solver}")
            from .sampler import validate_guidance_interval
            interval = validate_guidance_interval(guidance_interval, int(self._acp.shape[0]))
        phi = 0.0
        if guidance_rescale is not None:
            if not self.guided:
                raise ValueError("this stream is unguided: guidance_rescale= belongs in a guided stream")
            if (isinstance(guidance_rescale, bool) or not isinstance(guidance_rescale, (int, float)) or not math.isfinite(guidance_rescale)
                    or not 0.0 <= guidance_rescale <= 1.0):
                raise ValueError(f"guidance_rescale: a number in [0, 1] is needed, got {guidance_rescale!r}")
            phi = float(guidance_rescale)
        period = 1
        if guidance_refresh is not None:
            if not self.refresh:
                raise ValueError("guidance_refresh= needs a stream made with refresh=True (guided_stream(refresh=True))")
            from .sampler import validate_guidance_refresh
            period = validate_guidance_refresh(guidance_refresh)
            if period > 1 and phi > 0:
                raise NotImplementedError("guidance_refresh= with guidance_rescale=: the rescale statistics need the unconditional "
                                          "prediction at every step; a rescale that reuses the kept direction is a follow-up")
        if self.refresh and phi > 0:                               # it could share a step with a reusing request
            raise NotImplementedError("a stream made with refresh=True serves no guidance_rescale= > 0: the three-kind update of a step "
                                      "with a reusing request in flight has no rescale form (a follow-up)")
        if not self.project and not (guidance_projection is None and guidance_norm_threshold is None and guidance_momentum is None):
            raise ValueError("guidance_projection=, guidance_norm_threshold= and guidance_momentum= need a stream made with "
                             "project=True (guided_stream(project=True))")
        from .sampler import projection_vectors
        projection = projection_vectors(guidance_projection, guidance_norm_threshold, guidance_momentum, 1)
        if self.project and phi > 0:                               # it could share a step with a projected request
            raise NotImplementedError("a stream made with project=True serves no guidance_rescale= > 0: the three-kind update of a step "
                                      "with a projected request in flight has no rescale form (a follow-up)")
        kinds = None
        if self.guided:                                            # the list the closed call runs: refresh_plan of its own guided steps
            from .sampler import guided_steps, refresh_plan
            code = {"plain": hip.KIND_PLAIN, "refresh": hip.KIND_REFRESH, "reuse": hip.KIND_REUSE}
            kinds = [code[k] for k in refresh_plan(guided_steps(schedule, interval), period)[0]]
        pcoef = None
        if projection is not None:                                 # the rows the closed call uploads, for this utterance alone
            from .sampler import guided_steps, project_table
            pcoef = project_table(projection, torch.tensor([float(guidance)], dtype=torch.float32), self._x0_schedule(n_steps),
                                  guided_steps(schedule, interval))[:, 0].contiguous().numpy()
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)))
        elif not _is_int(seed) or not -2 ** 63 <= seed < 2 ** 63:
            raise ValueError(f"seed: an int64 is needed, got {seed!r}")
        if x_T is not None:
            if not isinstance(x_T, torch.Tensor) or not x_T.dtype.is_floating_point or tuple(x_T.shape) != (n_frames, self.hidden_dim):
                raise ValueError(f"x_T: a floating-point tensor [{n_frames}, {self.hidden_dim}] is needed")
            x_T = x_T.detach()
        if prompt is not None:
            if (not isinstance(prompt, torch.Tensor) or not prompt.dtype.is_floating_point or prompt.dim() != 2 or prompt.shape[0] < 1
                    or prompt.shape[1] != self.hidden_dim):
                raise ValueError(f"prompt: a floating-point tensor [P >= 1, {self.hidden_dim}] is needed")
            prompt = prompt.detach()
        if suffix is not None:
            if (not isinstance(suffix, torch.Tensor) or not suffix.dtype.is_floating_point or suffix.dim() != 2 or suffix.shape[0] < 1
                    or suffix.shape[1] != self.hidden_dim):
                raise ValueError(f"suffix: a floating-point tensor [Q >= 1, {self.hidden_dim}] is needed")
            suffix = suffix.detach()
        req = Request(StreamHandle(self._next_id), text, null, n_frames, seed, None if guidance is None else float(guidance), n_steps,
                      float(eta), x_T, schedule, prompt, interval, phi, suffix, kinds, period, pcoef)
        if req.rows > self.max_rows:
            raise ValueError(f"a request of {req.rows} rows ({req.P} prompt + {req.n_frames} frames"
                             + (f" + {req.Q} suffix" if req.Q else "") + f") can never fit max_rows = {self.max_rows}")
        if req.text_rows > self.max_text_rows:
            raise ValueError(f"a request of {req.text_rows} conditioning rows can never fit max_text_rows = {self.max_text_rows}")
        self._next_id += 1
        self._queue.append(req)
        return req.handle

    def _fits(self, req: Request, members: List[Request]) -> bool:
        return (len(members) + 1 <= self.max_utterances
                and sum(r.rows for r in members) + req.rows <= self.max_rows
                and sum(r.text_rows for r in members) + req.text_rows <= self.max_text_rows)

    def step(self):
        """Admit (FIFO, stopping at the first request that does not fit: nothing is overtaken), regroup if the membership changed,
        run one step over everything in flight, retire the utterances that have run their own n_steps.  Returns the retired
        [(handle, latents fp32 [N_b, d] on the GPU), ...] in slot order; [] when nothing is in flight."""
        members, newcomers = list(self._active), []
        while self._queue and self._fits(self._queue[0], members):
            req = self._queue.popleft()
            members.append(req)
            newcomers.append(req)
        if not members:
            return []
        args = self._step_args(members)
        in_g = args.in_g
        # a change of the guided set is a membership change of the unconditional region: the same one regroup serves it
        if newcomers or self._dirty or any(r.in_g != f for r, f in zip(members, in_g or ())):
            carry = [r not in newcomers and r.carries_direction() for r in members] if self.project else None
            self.batch.regroup(Plan(members, newcomers, self.guided, in_g, args.kind if self.refresh else None, carry), args)
            for r, f in zip(members, in_g or ()):
                r.in_g = f
            self._dirty = False
        self._active = members
        self.batch.step(args)
        done = []
        for r in members:
            r.i += 1
            if r.i == r.n_steps:
                done.append(r)
        if not done:
            return []
        outs = self.batch.retire(done)
        self._active = [r for r in members if r.i < r.n_steps]
        self._dirty = True
        return [(r.handle, o) for r, o in zip(done, outs)]

    def drain(self):
        """step() until nothing is pending or in flight; every result, in the order it came back."""
        out = []
        while self._queue or self._active:
            out.extend(self.step())
        return out

    def _step_args(self, members: List[Request]) -> StepArgs:
        s = StepArgs()
        s.B, s.S = len(members), sum(r.rows for r in members)
        s.max_N = max(r.rows for r in members)
        s.S_T = sum(r.text_rows for r in members)
        s.max_T = max(max(r.T, r.T_null) for r in members)
        rows = [r.schedule[r.i] for r in members]                   # (tau, a, ce, sigma) of each utterance's own step
        s.t = [int(q[0]) for q in rows]
        if self.solver == "ddim":
            s.a, s.ce, s.cz = [q[1] for q in rows], [q[2] for q in rows], [q[3] for q in rows]
            s.tags = [int(q[0]) & 0xFFFFFFFF for q in rows]         # the step's Philox tag: its timestep, as in the closed loops
            s.coef = None
        else:                                                       # (tau, a, kx, ke, b, g, use_prev): use_prev is False at r.i == 0
            s.a = s.ce = s.cz = s.tags = None
            s.coef = [tuple(q[1:]) for q in rows]
        s.w = [r.w for r in members] if self.guided else None
        s.kind = [r.kind_now() for r in members] if self.guided else None
        s.period = [r.period for r in members]
        s.in_g = [k == hip.KIND_REFRESH for k in s.kind] if self.guided else None
        s.proj = None
        if self.project:                                           # in_g = kind != plain: the guided ones, projected or not
            s.kind = [r.project_kind_now() for r in members]
            s.proj = [None if r.pcoef is None else r.pcoef[r.i] for r in members]
        s.partner = partner_table(s.in_g) if self.guided else None
        s.G = sum(s.in_g) if self.guided else 0
        s.S_G = sum(r.rows for r, f in zip(members, s.in_g) if f) if self.guided else 0
        s.seeds = [r.seed for r in members]
        s.handles = [r.handle for r in members]
        s.prompt = [r.P for r in members]
        s.phi = [r.phi for r in members]
        s.suffix = [r.Q for r in members]
        return s


def _pad(n: int, m: int) -> int:
    return (n + m - 1) // m * m


class _Upload:
    """One device buffer fed from a ring of pinned host buffers by asynchronous copies.  A slot is rewritten only after the copy that
    last read it has finished (its event — `slots` sends old; the wait is on that one copy, not on the device)."""

    def __init__(self, nbytes: int, device, slots: int = 8):
        self.dev = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self._host = [torch.zeros(nbytes, dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self._np = [h.numpy() for h in self._host]
        self._events = [None] * slots
        self._k = 0

    def send(self, data: np.ndarray):
        k, n = self._k, int(data.nbytes)
        self._k = (k + 1) % len(self._host)
        if self._events[k] is not None:
            self._events[k].synchronize()
        self._np[k][:n] = data.view(np.uint8).reshape(-1)
        self.dev[:n].copy_(self._host[k][:n], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev.device))
        self._events[k] = ev


# the buffers a regroup's segments name (ditto_regroup_packed): sources and destinations
_SRC_X, _SRC_XT, _SRC_COND, _SRC_NEW_COND, _SRC_TABLE, _SRC_Q = range(6)
_DST_X, _DST_OUT, _DST_COND, _DST_OFFSETS, _DST_Q = range(5)


def _suffix_rows(r) -> int:
    """Q of a request; a record without the field (host arithmetic on a bare record) has no suffix"""
    return getattr(r, "Q", 0)


def speech_segments(r: Request, new: bool, j: int, dst_row: int, xt_row: int, d4: int, dup: int) -> List[List[int]]:
    """The segments that put utterance `r` (slot j) at row `dst_row` of the next state, in 16-byte units (d4 per row).  A survivor
    moves as one range, prompt included.  A newcomer: its prompt, staged at row `xt_row` of the x_T buffer, is copied in front;
    behind it its own x_T (staged after the prompt) is copied, or drawn from its seed — the draw counts its units from 0, so the
    generated rows get ditto_noise_normal's numbers for an utterance of n_frames rows.  Its suffix (speech infilling), staged behind
    those two, is one more copy behind the generated rows.  `dup`: the unconditional half's offset."""
    if not new:
        return [[hip.REGROUP_COPY, _SRC_X, _DST_X, 0, r.row * d4, dst_row * d4, r.rows * d4, dup]]
    segs = []
    if r.P:
        segs.append([hip.REGROUP_COPY, _SRC_XT, _DST_X, 0, xt_row * d4, dst_row * d4, r.P * d4, dup])
    if r.x_T is not None:
        segs.append([hip.REGROUP_COPY, _SRC_XT, _DST_X, 0, (xt_row + r.P) * d4, (dst_row + r.P) * d4, r.n_frames * d4, dup])
    else:
        segs.append([hip.REGROUP_DRAW, 0, _DST_X, j, 0, (dst_row + r.P) * d4, r.n_frames * d4, dup])
    Q = _suffix_rows(r)
    if Q:
        segs.append([hip.REGROUP_COPY, _SRC_XT, _DST_X, 0, (xt_row + staged_rows(r) - Q) * d4, (dst_row + r.P + r.n_frames) * d4,
                     Q * d4, dup])
    return segs


def history_segment(r: Request, dst_row: int, d4: int) -> List[int]:
    """The segment that carries a survivor's multistep history — the x0 prediction of its last step, on its generated rows — from
    the current history buffer to row `dst_row` of the next one.  A newcomer has none: its first step does not read the history."""
    return [hip.REGROUP_COPY, _SRC_Q, _DST_Q, 0, (r.row + r.P) * d4, (dst_row + r.P) * d4, r.n_frames * d4, 0]


def direction_segment(r: Request, dst_row: int, d4: int) -> List[int]:
    """The segment that carries a survivor's kept guidance direction — delta = c - u of its last refresh step, on its generated rows
    — from the current direction buffer to row `dst_row` of the next one: for a survivor whose coming step is a reuse step.  One
    that refreshes writes its direction anew, a plain one and a newcomer have none.  A refresh stream has no multistep history,
    so the direction buffers take the history's source and destination slots."""
    return [hip.REGROUP_COPY, _SRC_Q, _DST_Q, 0, (r.row + r.P) * d4, (dst_row + r.P) * d4, r.n_frames * d4, 0]


def staged_rows(r: Request) -> int:
    """rows of the x_T staging buffer a newcomer takes: its prompt, then its own x_T, then its suffix"""
    return r.P + (r.n_frames if r.x_T is not None else 0) + _suffix_rows(r)


def retire_segments(done: List[Request], d4: int) -> List[List[int]]:
    """the generated rows of the utterances that leave (their prompts and suffixes stay behind), one behind the other in the output"""
    cu = _cumulate(r.n_frames for r in done)
    return [[hip.REGROUP_COPY, _SRC_X, _DST_OUT, 0, (r.row + r.P) * d4, cu[k] * d4, r.n_frames * d4, 0] for k, r in enumerate(done)]


def regroup_table(plan: Plan, *, d4: int, kv16: int, tm16: int, tmod_old16: int, tmod_new16: int, new_image: dict, multistep: bool,
                  cu_pad: int):
    """(segments, offsets tail) of the ONE launch that builds `plan`'s batch: host arithmetic only.  Units of 16 bytes: d4 per speech
    row, kv16 per K/V row, tm16 per tmod row; tmod_old16 / tmod_new16: where tmod starts in the current / next conditioning image;
    new_image[id] = (first unit of a newcomer's own image [text K/V | null K/V | tmod text, null] in the staging buffer, first unit
    of its tmod).
    Speech: every member's rows go to [cu[j], cu[j+1]) and, for a member of the guided set G, also to its unconditional copy at row
    S + cu_g[partner[j]] through the segment's dup_off — a member entering G gets its copy from its conditional rows (the two are
    equal after any update), one leaving G just has none.  Conditioning: text K/V and tmod in batch order; null K/V and tmod at
    plan.null_row / plan.null_tm — G's rows compacted behind the texts where the forward reads them, the others parked behind G's.
    The offsets [offsets | text_offsets] ride behind the segments in the same upload.
    Guidance reuse (plan.kind given): G is the refreshing members, and a survivor whose coming step is a reuse step gets one more
    segment, direction_segment.  Projected guidance (plan.carry given): so does every survivor plan.carry names — the buffers flip,
    so the direction m' moves with its utterance whatever its coming step's kind."""
    guided = plan.in_g is not None
    B, S, Tt = len(plan.members), plan.cu[-1], plan.cu_text[-1]
    segs, xt_row = [], 0
    for j, r in enumerate(plan.members):
        new = r.handle.id in new_image
        dup = (S + plan.cu_g[plan.partner[j]] - plan.cu[j]) * d4 if guided and plan.in_g[j] else 0
        segs.extend(speech_segments(r, new, j, plan.cu[j], xt_row, d4, dup))
        if new:
            xt_row += staged_rows(r)
        elif multistep:
            segs.append(history_segment(r, plan.cu[j], d4))
        elif plan.kind is not None and plan.kind[j] == hip.KIND_REUSE:
            segs.append(direction_segment(r, plan.cu[j], d4))
        elif plan.carry is not None and plan.carry[j]:
            segs.append(direction_segment(r, plan.cu[j], d4))
        if new:
            base, own_tmod = new_image[r.handle.id]
            source, kv_t, kv_n, tm_t, tm_n = _SRC_NEW_COND, base, base + r.T * kv16, own_tmod, own_tmod + tm16
        else:
            source, kv_t, kv_n = _SRC_COND, r.trow * kv16, r.nrow * kv16 if guided else 0
            tm_t, tm_n = tmod_old16 + r.b * tm16, tmod_old16 + (r.ntm if guided else 0) * tm16
        segs.append([hip.REGROUP_COPY, source, _DST_COND, 0, kv_t, plan.cu_text[j] * kv16, r.T * kv16, 0])
        segs.append([hip.REGROUP_COPY, source, _DST_COND, 0, tm_t, tmod_new16 + j * tm16, tm16, 0])
        if guided:
            segs.append([hip.REGROUP_COPY, source, _DST_COND, 0, kv_n, (Tt + plan.null_row[j]) * kv16, r.T_null * kv16, 0])
            segs.append([hip.REGROUP_COPY, source, _DST_COND, 0, tm_n, tmod_new16 + (B + plan.null_tm[j]) * tm16, tm16, 0])
    tail = np.zeros(2 * cu_pad, dtype=np.int32)
    tail[:len(plan.offsets)] = plan.offsets
    tail[cu_pad:cu_pad + len(plan.text_offsets)] = plan.text_offsets
    segs.append([hip.REGROUP_COPY, _SRC_TABLE, _DST_OFFSETS, 0, (len(segs) + 1) * 2, 0, 2 * cu_pad // 4, 0])
    return segs, tail


def step_block_layout(max_utterances: int, guided: bool, multistep: bool, infill: bool = False, refresh: bool = False,
                      project: bool = False) -> dict:
    """Byte offsets of the per-step argument block (host arithmetic): t int64 [halves * maxB] | seeds int64 [maxB] | a | ce | cz | w
    fp32 [maxB] | tags uint32 [maxB] | prompt_len int32 [maxB] | partner int32 [maxB] | (multistep) ditto_multistep_coef [maxB] |
    phi fp32 [maxB] — the guidance-rescale blend factors, appended behind everything else: the fields in front keep the offsets
    they had before it existed.  `infill`: suffix_len int32 [maxB] ("suffix") is appended behind phi in the same way; off (the
    default), the layout is the one without it.  `refresh`: kind int32 [maxB] ("kind", guidance reuse) is appended behind everything
    else in the same way.  `project`: kind int32 [maxB] ("kind", projected guidance's) and then ditto_project_coef [maxB] ("proj",
    16-byte aligned) are appended behind everything else in the same way.  "f_stride": bytes of one fp32 / int32 field; "bytes": the
    whole block."""
    maxB, nbB = int(max_utterances), (2 if guided else 1) * int(max_utterances)
    lay = {"t": 0, "seeds": _pad(nbB * 8, 16)}
    o_f = lay["seeds"] + _pad(maxB * 8, 16)
    lay["f_stride"] = _pad(maxB * 4, 16)
    for k, name in enumerate(("a", "ce", "cz", "w", "tags", "prompt", "partner", "coef")):
        lay[name] = o_f + k * lay["f_stride"]
    lay["phi"] = _pad(lay["coef"] + (C.sizeof(hip.MultistepCoef) * maxB if multistep else 0), 16)
    lay["bytes"] = lay["phi"] + lay["f_stride"]
    if infill:
        lay["suffix"] = lay["bytes"]
        lay["bytes"] += lay["f_stride"]
    if refresh:
        lay["kind"] = lay["bytes"]
        lay["bytes"] += lay["f_stride"]
    if project:
        lay["kind"] = lay["bytes"]
        lay["proj"] = _pad(lay["kind"] + lay["f_stride"], 16)
        lay["bytes"] = lay["proj"] + _pad(C.sizeof(hip.ProjectCoef) * maxB, 16)
    return lay


class DeviceBatch:
    """The packed batch of a GuidedStream on one GPU.  Buffers (sized once from the capacities): two state buffers [2 max_rows, d]
    ([max_rows, d] unguided) and two conditioning images (a regroup reads one and writes the other), a staging image for the
    newcomers' conditioning and one for callers' x_T, the device offsets, the per-step argument block and the segment table.
    `solver` "dpmpp2m": two history buffers [max_rows, d] beside the state (double-buffered like it: a regroup moves the
    survivors' rows of both in its one launch), and the step block carries one ditto_multistep_coef per utterance.
    `infill`: the step block carries each utterance's suffix length as well.
    `refresh` (guidance reuse): two direction buffers [max_rows, d] beside the state, double-buffered like it — a regroup moves the
    reusing survivors' rows in its one launch, through the slots the history takes in a "dpmpp2m" stream —, and the step block
    carries each utterance's kind.
    `project` (projected guidance): two direction buffers [max_rows, d] beside the state, double-buffered like it and moved through the
    same slots, one scratch (ditto_guidance_project_bytes) sized once from the capacities, and the step block carries each
    utterance's kind and ditto_project_coef."""

    def __init__(self, engine, *, max_rows: int, max_utterances: int, max_text_rows: int, guided: bool, class_rows=None,
                 solver: str = "ddim", infill: bool = False, refresh: bool = False, project: bool = False):
        from .engine import require_fused_attention
        self.refresh = validate_refresh_stream(refresh, bool(guided), solver, bool(infill))
        self.project = validate_project_stream(project, bool(guided), solver, bool(infill), self.refresh)
        require_fused_attention(engine.cfg, "request streams (packed batches)")
        self.multistep, self.infill = solver != "ddim", bool(infill)
        self.eng, self.lib, self.guided = engine, engine.lib, bool(guided)
        self.halves = 2 if guided else 1
        self.maxB, self.maxS, self.maxT = int(max_utterances), int(max_rows), int(max_text_rows)
        self.opts = None if class_rows is None else hip.CallOpts(class_rows=int(class_rows))
        dev, d = engine.device, engine.cfg.hidden_dim
        self.d = d
        row, off = C.c_size_t(0), C.c_size_t(0)
        hip.check(self.lib.ditto_regroup_cond_layout(C.byref(engine._ccfg), self.maxT, C.byref(row), C.byref(off)))
        self.kv_row = int(row.value)                                       # bytes of one K/V row of the conditioning image
        self.tmod_row = 2 * d * 4
        nbB = self.halves * self.maxB
        cond_bytes = int(self.lib.ditto_packed_cond_bytes(C.byref(engine._ccfg), nbB, self.maxT))
        with torch.cuda.device(dev):
            self.x = [torch.zeros(self.halves * self.maxS, d, dtype=torch.float32, device=dev) for _ in range(2)]
            self.q = [torch.zeros(self.maxS, d, dtype=torch.float32, device=dev) for _ in range(2)] if self.multistep else None
            self.delta = [torch.zeros(self.maxS, d, dtype=torch.float32, device=dev) for _ in range(2)] if self.refresh else None
            self.dir = [torch.zeros(self.maxS, d, dtype=torch.float32, device=dev) for _ in range(2)] if self.project else None
            self.cond = [torch.zeros(cond_bytes, dtype=torch.uint8, device=dev) for _ in range(2)]
            # every newcomer's own image [K/V rows | tmod], 256-byte aligned, one behind the other
            self.new_cond = torch.zeros(self.maxT * self.kv_row + self.maxB * (_pad(self.halves * self.tmod_row, 256) + 256),
                                        dtype=torch.uint8, device=dev)
            self.x_T = torch.zeros(self.maxS, d, dtype=torch.float32, device=dev)
            self.cu_pad = _pad(nbB + 1, 4)                                 # int32 words of one offsets section
            self.offsets = torch.zeros(2 * self.cu_pad, dtype=torch.int32, device=dev)     # [cu (doubled under CFG) | cu_text]
            lay = step_block_layout(self.maxB, self.guided, self.multistep, self.infill, self.refresh, self.project)
            self.o_suffix, self.o_kind, self.o_proj = lay.get("suffix"), lay.get("kind"), lay.get("proj")
            self.f_stride, self.block_bytes = lay["f_stride"], lay["bytes"]
            (self.o_t, self.o_seeds, self.o_a, self.o_ce, self.o_cz, self.o_w, self.o_tags, self.o_prompt, self.o_partner, self.o_coef,
             self.o_phi) = (lay[k] for k in ("t", "seeds", "a", "ce", "cz", "w", "tags", "prompt", "partner", "coef", "phi"))
            self.block = _Upload(self.block_bytes, dev)
            # the guidance-rescale scratch, once, for maxB utterances of at most maxS generated rows
            self.rescale = engine.rescale_scratch(self.maxB, self.maxS) if self.guided else None
            # the projected-guidance scratch [pcoef | partials], once, for the same capacities
            self.project_scratch = engine.project_scratch(self.maxB, self.maxS) if self.project else None
            self.max_seg = 8 * self.maxB + 8
            self.table = _Upload(self.max_seg * 4 * hip.REGROUP_SEG_WORDS + 2 * self.cu_pad * 4, dev)
            engine.workspace_packed(nbB, self.halves * self.maxS, self.maxT)
            self.rope = engine.rope_tables(self.maxS)                      # rows [0, max_N) of it are ditto_rope_tables(max_N)
        self.cur = 0                 # which of x / cond holds the batch in flight
        self.B = self.S = self.T_text = 0
        self._tmod_off = 0           # of the current conditioning image
        self._block_sent = False     # the step block of the coming step went up with its regroup

    # ------------------------------------------------------------------ uploads
    def _send_block(self, a: StepArgs):
        B = a.B
        buf = np.zeros(self.block_bytes, dtype=np.uint8)
        # t of the forward's utterances: the B in flight, then (under guidance) the guided ones' unconditional copies
        tt = a.t + [a.t[j] for j, p in enumerate(a.partner) if p >= 0] if self.guided else a.t
        buf[self.o_t:self.o_t + len(tt) * 8].view(np.int64)[:] = tt
        buf[self.o_seeds:self.o_seeds + B * 8].view(np.int64)[:] = a.seeds
        if self.multistep:             # ditto_multistep_coef: a, kx, ke, b, g, w fp32 | use_prev int32 | reserved
            co = buf[self.o_coef:self.o_coef + 32 * B].view(np.float32).reshape(B, 8)
            co[:, :5] = [c[:5] for c in a.coef]
            co[:, 5] = a.w if a.w is not None else 0.0
            co.view(np.int32)[:, 6] = [int(c[5]) for c in a.coef]
        else:
            for o, v in ((self.o_a, a.a), (self.o_ce, a.ce), (self.o_cz, a.cz), (self.o_w, a.w if a.w is not None else [0.0] * B)):
                buf[o:o + B * 4].view(np.float32)[:] = v
            buf[self.o_tags:self.o_tags + B * 4].view(np.uint32)[:] = a.tags
        buf[self.o_prompt:self.o_prompt + B * 4].view(np.int32)[:] = a.prompt
        if self.guided:
            buf[self.o_partner:self.o_partner + B * 4].view(np.int32)[:] = a.partner
            buf[self.o_phi:self.o_phi + B * 4].view(np.float32)[:] = a.phi
        if self.infill:
            buf[self.o_suffix:self.o_suffix + B * 4].view(np.int32)[:] = a.suffix
        if self.refresh:
            buf[self.o_kind:self.o_kind + B * 4].view(np.int32)[:] = a.kind
        if self.project:               # ditto_project_coef: kx, ke, w, eta, r, beta fp32 | use_prev int32 | reserved; zeros where there is none
            buf[self.o_kind:self.o_kind + B * 4].view(np.int32)[:] = a.kind
            pj = buf[self.o_proj:self.o_proj + 32 * B].view(np.float32).reshape(B, 8)
            for j, row in enumerate(a.proj):
                if row is not None:
                    pj[j] = row
        self.block.send(buf)

    def _block_ptr(self, off: int) -> int:
        return self.block.dev.data_ptr() + off

    def _tmod_offset(self, S_T: int) -> int:
        row, off = C.c_size_t(0), C.c_size_t(0)
        hip.check(self.lib.ditto_regroup_cond_layout(C.byref(self.eng._ccfg), S_T, C.byref(row), C.byref(off)))
        return int(off.value)

    def _run_table(self, segs: List[List[int]], tail: Optional[np.ndarray], out: Optional[torch.Tensor]):
        """upload the segments (+ `tail`: int32 words appended for the offsets segment) and run ditto_regroup_packed"""
        if len(segs) > self.max_seg:
            raise RuntimeError("regroup: more segments than the table holds")
        tab = np.asarray(segs, dtype=np.int64).astype(np.uint32).view(np.uint8).reshape(-1)
        data = tab if tail is None else np.concatenate([tab, tail.view(np.uint8).reshape(-1)])
        self.table.send(data)
        nxt = 1 - self.cur
        src = [self.x[self.cur], self.x_T, self.cond[self.cur], self.new_cond, self.table.dev]
        dst = [self.x[nxt], out, self.cond[nxt], self.offsets]
        if self.multistep:             # the history moves with the state: _SRC_Q, _DST_Q
            src.append(self.q[self.cur])
            dst.append(self.q[nxt])
        elif self.refresh:             # so do the kept directions, in the same slots (a refresh stream has no history)
            src.append(self.delta[self.cur])
            dst.append(self.delta[nxt])
        elif self.project:             # and the projected directions m' (a "ddim" stream without refresh: the slots are free)
            src.append(self.dir[self.cur])
            dst.append(self.dir[nxt])
        n = hip.REGROUP_BUFS
        sp, sb, dp, db = (C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_void_p * n)(), (C.c_size_t * n)()
        for k, t in enumerate(src):
            sp[k], sb[k] = t.data_ptr(), t.numel() * t.element_size()
        for k, t in enumerate(dst):
            if t is not None:
                dp[k], db[k] = t.data_ptr(), t.numel() * t.element_size()
        hip.check(self.lib.ditto_regroup_packed(self.table.dev.data_ptr(), len(segs), sp, sb, dp, db, n, self._block_ptr(self.o_seeds),
                                                self.maxB, 16 * max(s[6] for s in segs), _stream()))

    # ------------------------------------------------------------------ what the scheduler calls
    def _condition(self, r: Request, at: int) -> int:
        """the conditioning of newcomer `r`, computed exactly as a solo sample_guided_packed computes it — one
        ditto_text_precompute_packed over that utterance's [text; null] — into the staging image at byte `at`; returns its size"""
        dev = self.eng.device
        text = r.text.to(dev, torch.float32)
        ct = [0, r.T]
        if self.guided:
            text = torch.cat([text, r.null.to(dev, torch.float32)], dim=0)
            ct.append(r.T + r.T_null)
        nb = self.eng.prepare_text_packed_into(text.contiguous(), ct, self.new_cond, at)
        return nb

    def regroup(self, plan: Plan, args: StepArgs):
        """Build the next batch in the other pair of buffers: survivors' rows from the current ones, newcomers' x_T (drawn from the
        seed, or the caller's) and freshly computed conditioning, the new offsets.  One launch."""
        self._send_block(args)                                     # first: "draw x_T" reads the newcomers' seeds from it
        d4, kv16, tm16 = self.d // 4, self.kv_row // 16, self.tmod_row // 16
        B, S, Tt = len(plan.members), plan.cu[-1], plan.cu_text[-1]
        S_T = Tt + (plan.cu_null[-1] if self.guided else 0)
        tmod_new = self._tmod_offset(S_T)
        at, xt_row = 0, 0
        new_image = {}
        for r in plan.newcomers:
            new_image[r.handle.id] = (at // 16, (at + self._tmod_offset(r.text_rows)) // 16)
            at += self._condition(r, at)
        for r in plan.members:             # the newcomers' prompts, own x_T and suffixes, staged in the order speech_segments reads them
            if r.handle.id not in new_image:
                continue
            if r.P:
                self.x_T[xt_row:xt_row + r.P].copy_(r.prompt, non_blocking=True)
            if r.x_T is not None:
                self.x_T[xt_row + r.P:xt_row + r.P + r.n_frames].copy_(r.x_T, non_blocking=True)
            if r.Q:
                self.x_T[xt_row + staged_rows(r) - r.Q:xt_row + staged_rows(r)].copy_(r.suffix, non_blocking=True)
            xt_row += staged_rows(r)
        segs, tail = regroup_table(plan, d4=d4, kv16=kv16, tm16=tm16, tmod_old16=self._tmod_off // 16, tmod_new16=tmod_new // 16,
                                   new_image=new_image, multistep=self.multistep, cu_pad=self.cu_pad)
        self._run_table(segs, tail, None)
        self.cur = 1 - self.cur
        self.B, self.S, self.T_text, self._tmod_off = B, S, Tt, tmod_new
        for j, r in enumerate(plan.members):
            r.b, r.row, r.trow = j, plan.cu[j], plan.cu_text[j]
            r.nrow = Tt + plan.null_row[j] if self.guided else None
            r.ntm = B + plan.null_tm[j] if self.guided else None
        self._block_sent = True

    def step(self, a: StepArgs):
        """One library call over the batch in flight, in place on the current state; every per-utterance argument comes from the
        step block.
          * solver "dpmpp2m": ditto_guided_step_packed_multistep_opts on the state and the history, each utterance at its own
            coefficient entry;
          * some utterances guided, some not (guidance intervals): ditto_guided_step_packed_mixed_opts over the B utterances and
            the G copies, with the partner table;
          * else ditto_guided_step_packed_tags_opts (a prompted utterance in flight: ..._tags_prompt_opts) — with cfg 1 over
            [x; x] when everyone is guided, with cfg 0 over the conditional rows when nobody is (or the stream is unguided).
        A step in which a guided utterance has phi > 0 runs the guidance-rescale form of its entry
        (ditto_guided_step_packed_multistep_rescale_opts; ditto_guided_step_packed_rescale_opts with the partner table when only
        some are guided, without it when everyone is): phi from the step block, the scratch built once.
        A step with a suffixed utterance in flight (an infill stream: no intervals, no rescale) runs the window form of its entry,
        ditto_guided_step_packed_tags_window_opts or ditto_guided_step_packed_multistep_window_opts, the suffix lengths from the
        step block; with none in flight, the entries above.
        A step with a request of refresh period k > 1 in flight (a refresh stream: "ddim", no infill, no rescale beside k > 1) runs
        ditto_guided_step_packed_refresh_opts over the B utterances and the G copies of the refreshing ones — G = 0 and G = B
        included — with the kinds from the step block and the current direction buffer; with none in flight, the entries above.
        A step in which a request is projected (a project stream: "ddim", no infill, no refresh, no rescale) runs
        ditto_guided_step_packed_project_mixed_opts over the B utterances and the G copies of the guided ones, projected or not, with
        the kinds and the ditto_project_coef rows from the step block, the current direction buffer and the scratch built once;
        every other step runs the entries above."""
        if not self._block_sent:
            self._send_block(a)
        self._block_sent = False
        eng, at = self.eng, self._block_ptr
        cfg = self.guided and a.G > 0
        ws = eng.workspace_packed(a.B + a.G, a.S + a.S_G, a.S_T)         # the forward: the B utterances and the G copies
        # by the names include/ditto_hip.h gives them (hip.call).  What every entry shares: the model, the state, the conditioning, t,
        # the speech and text offsets, the rope tables, the workspace, the stream and the options
        args = dict(m=eng.handle, x2=self.x[self.cur].data_ptr(), cond=self.cond[self.cur].data_ptr(), t=at(self.o_t),
                    cu_speech=self.offsets.data_ptr(), cu_text=self.offsets.data_ptr() + 4 * self.cu_pad, max_N=a.max_N, S_T=a.S_T,
                    max_T=a.max_T, rope_cos=self.rope[0].data_ptr(), rope_sin=self.rope[1].data_ptr(), workspace=ws.data_ptr(),
                    workspace_bytes=ws.numel(), stream=_stream(), opts=None if self.opts is None else C.byref(self.opts))
        prompt = at(self.o_prompt) if any(a.prompt) else None
        noise = dict(noise=None, seeds=at(self.o_seeds), tags=at(self.o_tags))   # no buffer: Philox of the seeds at each utterance's tag
        coef = dict(a=at(self.o_a), ce=at(self.o_ce), cz=at(self.o_cz))
        history = dict(q=self.q[self.cur].data_ptr(), coefs=at(self.o_coef)) if self.multistep else None
        if self.infill and any(a.suffix):
            if self.multistep:
                hip.check(hip.call("ditto_guided_step_packed_multistep_window_opts", **args, prompt_len=prompt, suffix_len=at(self.o_suffix),
                                   **history, step=None, w=None, B=a.B, S=a.S, cfg=int(self.guided)))
            else:
                hip.check(hip.call("ditto_guided_step_packed_tags_window_opts", **args, prompt_len=prompt, suffix_len=at(self.o_suffix),
                                   **noise, w=at(self.o_w) if cfg else None, **coef, B=a.B, S=a.S, cfg=int(cfg)))
            return
        if self.refresh and any(k > 1 for k in a.period):
            hip.check(hip.call("ditto_guided_step_packed_refresh_opts", **args, partner=at(self.o_partner), kind=at(self.o_kind),
                               prompt_len=prompt, delta=self.delta[self.cur].data_ptr(), **noise, w=at(self.o_w), **coef, B=a.B, G=a.G,
                               S=a.S, S_G=a.S_G))
            return
        if self.project and any(k == hip.KIND_PROJECT for k in a.kind):
            hip.check(hip.call("ditto_guided_step_packed_project_mixed_opts", **args, partner=at(self.o_partner), kind=at(self.o_kind),
                               prompt_len=prompt, dir=self.dir[self.cur].data_ptr(), proj=at(self.o_proj), **noise, w=at(self.o_w), **coef,
                               B=a.B, G=a.G, S=a.S, S_G=a.S_G, scratch=self.project_scratch.data_ptr(),
                               scratch_bytes=self.project_scratch.numel()))
            return
        if cfg and any(p > 0 and g for p, g in zip(a.phi, a.in_g)):
            rescale = dict(phi=at(self.o_phi), scratch=self.rescale.data_ptr(), scratch_bytes=self.rescale.numel())
            if self.multistep:
                hip.check(hip.call("ditto_guided_step_packed_multistep_rescale_opts", **args, prompt_len=prompt, **history, **rescale,
                                   B=a.B, S=a.S))
            else:
                mixed = a.G < a.B
                hip.check(hip.call("ditto_guided_step_packed_rescale_opts", **args, partner=at(self.o_partner) if mixed else None,
                                   prompt_len=prompt, **noise, step=0, w=at(self.o_w), **coef, **rescale, B=a.B, G=a.G if mixed else 0,
                                   S=a.S, S_G=a.S_G if mixed else 0))
            return
        if self.multistep:
            hip.check(hip.call("ditto_guided_step_packed_multistep_opts", **args, prompt_len=prompt, **history, step=None, w=None, B=a.B,
                               S=a.S, cfg=int(self.guided)))
        elif 0 < a.G < a.B:
            hip.check(hip.call("ditto_guided_step_packed_mixed_opts", **args, partner=at(self.o_partner), prompt_len=prompt, **noise,
                               w=at(self.o_w), **coef, B=a.B, G=a.G, S=a.S, S_G=a.S_G))
        else:
            entry, spans = ("ditto_guided_step_packed_tags_opts", {}) if prompt is None else \
                ("ditto_guided_step_packed_tags_prompt_opts", dict(prompt_len=prompt))
            hip.check(hip.call(entry, **args, **spans, **noise, w=at(self.o_w) if cfg else None, **coef, B=a.B, S=a.S, cfg=int(cfg)))

    def retire(self, done: List[Request]) -> List[torch.Tensor]:
        """the generated rows of the utterances that leave, copied out of the state in one launch; the batch keeps its layout (with
        holes) until the next regroup"""
        cu = _cumulate(r.n_frames for r in done)
        out = torch.empty(cu[-1], self.d, dtype=torch.float32, device=self.eng.device)
        self._run_table(retire_segments(done, self.d // 4), None, out)
        return [out[cu[k]:cu[k + 1]] for k in range(len(done))]
