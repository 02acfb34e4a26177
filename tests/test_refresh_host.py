"""Reuse of the guidance direction on the host (no GPU): sampler.refresh_plan on hand-written cases with its mirror flags, the
argument validation of sample_guided_packed(guidance_refresh=) before any device work, what the closed call hands to its loops (None
and 1: nothing new), the loops' walk over the plan with stand-in step functions — the halves of the state are equal at every refresh —
and the new symbols with their argument refusals."""
import types

import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.sampler import SpeechGenerator, refresh_plan, validate_guidance_refresh
from ditto_tts_amd.synth import cosine_betas
from test_cabi_symbols import declared_functions

R, U, P = "refresh", "reuse", "plain"


def _plan(mask, k):
    return refresh_plan([c == "g" for c in mask], k)


@pytest.mark.parametrize("mask, k, kinds, mirror", [
    ("gggggg", 1, [R] * 6, []),                                                        # every guided step refreshes
    ("gggggg", 2, [R, U, R, U, R, U], [1, 3]),
    ("ggggggg", 3, [R, U, U, R, U, U, R], [2, 5]),
    ("--ggg-", 2, [P, P, R, U, R, P], [3]),                                            # an interval in the middle
    ("--ggg-", 3, [P, P, R, U, U, P], []),
    ("gggg--", 2, [R, U, R, U, P, P], [1]),                                            # touching the first step
    ("--gggg", 3, [P, P, R, U, U, R], [4]),                                            # touching the last step
    ("g", 2, [R], []), ("--g---", 5, [P, P, R, P, P, P], []),                          # a single guided step
    ("ggg", 7, [R, U, U], []),                                                         # k larger than the run
    ("gg-gg", 2, [R, U, P, R, U], []),                                                 # the counter restarts behind unguided steps
    ("g-g-g", 2, [R, P, R, P, R], []),
    ("------", 2, [P] * 6, []), ("", 3, [], []),
])
def test_refresh_plan_and_its_mirror_flags(mask, k, kinds, mirror):
    got, flags = _plan(mask, k)
    assert got == kinds
    assert [i for i, m in enumerate(flags) if m] == mirror and len(flags) == len(kinds)
    for i, kind in enumerate(got):                                                     # the rules, restated
        guided_before = i > 0 and mask[i - 1] == "g"
        if kind == R:
            assert mask[i] == "g"
        if mask[i] == "g" and not guided_before:
            assert kind == R, "the first guided step, and the first one behind unguided steps, refreshes"
        assert flags[i] == (kind == U and i + 1 < len(got) and got[i + 1] == R)


def test_refresh_plan_refuses_a_bad_period():
    for bad in (0, -2, True, 2.0, None, "2"):
        with pytest.raises(ValueError, match="k must be"):
            refresh_plan([True, True], bad)


def test_guidance_refresh_validation():
    assert validate_guidance_refresh(None) is None and validate_guidance_refresh(1) == 1 and validate_guidance_refresh(7) == 7
    for bad in (0, -1, True, False, 2.0, 1.5, "2", [2], (2,)):
        with pytest.raises(ValueError, match="guidance_refresh"):
            validate_guidance_refresh(bad)


def _bare_generator(cfg=DiTTOConfig(256, 2, 4, 256, 256, 50)):
    sg = object.__new__(SpeechGenerator)                          # no device: only what runs before the first GPU call
    sg.ditto_model = types.SimpleNamespace(cfg=cfg)
    sg.betas = torch.zeros(cfg.diffusion_steps)
    return sg


AUDIO, TEXT = torch.zeros(15, 256), torch.zeros(9, 256)
PACKED = (TEXT, [0, 3, 6, 9], AUDIO, [0, 5, 6, 15])
OK = dict(guidance=2.0, null_text_emb=TEXT)


def test_closed_call_refusals_before_any_launch():
    sg = _bare_generator()
    for solver in ("ddim", "dpmpp2m"):
        for bad in (0, -3, True, 2.0, "2"):
            with pytest.raises(ValueError, match="guidance_refresh"):
                sg.sample_guided_packed(*PACKED, solver=solver, guidance_refresh=bad, **OK)
        for k in (1, 2):
            with pytest.raises(ValueError, match="guidance_refresh needs"):
                sg.sample_guided_packed(*PACKED, solver=solver, guidance_refresh=k)
            with pytest.raises(ValueError, match="guidance_refresh needs"):
                sg.sample_guided_packed(*PACKED, solver=solver, guidance_refresh=k, guidance=2.0)
            with pytest.raises(NotImplementedError, match="follow-up"):
                sg.sample_guided_packed(*PACKED, solver=solver, guidance_refresh=k, guidance_rescale=0.5, **OK)


@pytest.mark.parametrize("solver, loop", [("ddim", "_guided_loop"), ("dpmpp2m", "_multistep_loop")])
def test_closed_call_hands_none_to_its_loop_for_none_and_one(solver, loop):
    sg = _bare_generator()
    seen = []
    setattr(sg, loop, lambda *a, **kw: seen.append(a) or "out")
    for k in (None, 1, 2, 3):
        kw = {} if k is None else dict(guidance_refresh=k)
        assert sg.sample_guided_packed(*PACKED, solver=solver, **OK, **kw) == "out"
    assert [a[-2] for a in seen] == [None, None, 2, 3]            # the loop's `refresh`
    assert all(callable(a[-1]) for a in seen)                     # and its begin_reuse


# ---------------------------------------------------------------------------------------------------------------- the loops
B, S, D = 2, 6, 4


class _Steps:
    """stand-ins for the layout's step functions over a CPU state: every call is recorded, a refresh REQUIRES equal halves"""

    def __init__(self):
        self.log, self.made = [], []

    def begin(self, eng, cfg, seeds):
        self.x2 = torch.zeros(2 * S if cfg else S, D)
        self.x2[:S] = torch.arange(S * D, dtype=torch.float32).reshape(S, D)
        if cfg:
            self.x2[S:] = float("nan")
        return self.x2, S, self._fn("step")

    def begin_plain(self, eng, x2):
        self.made.append("begin_plain")
        return self._fn("plain")

    def begin_reuse(self, eng, x2, step, delta):
        self.made.append("begin_reuse")
        assert delta.shape == (S, D) and delta.dtype == torch.float32
        return self._fn("refresh"), self._fn("reuse"), self._fn("plain")

    def _fn(self, name):
        def call(**kw):
            x2, opts = self.x2, kw["opts"]
            self.log.append((name, kw.get("mirror"), int(kw["t"].shape[0]), None if opts is None else opts.class_rows))
            if name in ("step", "refresh"):
                assert torch.equal(x2[S:], x2[:S]), "a guided forward over [x; x] needs the unconditional half up to date"
                x2 += 1.0
            else:
                x2[:S] += 1.0
                if name == "reuse" and kw["mirror"]:              # x' goes to both halves
                    x2[S:] = x2[:S]
        return call


def _loop_generator():
    sg = _bare_generator()
    sg.device = "cpu"
    sg.alphas_cumprod = torch.cumprod(1.0 - cosine_betas(50), dim=0)
    sg.ditto_model.engine = lambda device: types.SimpleNamespace(device=torch.device("cpu"))
    return sg


def _run(sg, solver, st, interval, refresh):
    if solver == "ddim":
        return sg._guided_loop(B, 2.0, TEXT, 6, 0.0, None, None, 3, st.begin, interval, st.begin_plain, None, "eps", refresh, st.begin_reuse)
    return sg._multistep_loop(B, 2.0, TEXT, 6, None, 3, st.begin, interval, st.begin_plain, None, "eps", refresh, st.begin_reuse)


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_loops_without_refresh_never_build_the_reuse_steps(solver):
    sg = _loop_generator()
    for interval in (None, (10, 35)):
        st = _Steps()
        out = _run(sg, solver, st, interval, None)
        assert "begin_reuse" not in st.made and {e[0] for e in st.log} <= {"step", "plain"}
        assert torch.equal(out, torch.arange(S * D, dtype=torch.float32).reshape(S, D) + 6.0)


@pytest.mark.parametrize("interval", [None, (10, 35), (10, 49), (0, 35)], ids=["all", "middle", "from_start", "to_end"])
@pytest.mark.parametrize("k", [2, 3, 9])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_loops_walk_the_plan_and_keep_the_halves_equal_at_every_refresh(solver, k, interval):
    sg = _loop_generator()
    st = _Steps()
    out = _run(sg, solver, st, interval, k)
    taus = [49, 41, 32, 24, 16, 7]
    guided = [interval is None or interval[0] <= t <= interval[1] for t in taus]
    kinds, mirror = refresh_plan(guided, k)
    assert st.made == ["begin_reuse"]                             # built once; its plain step serves the unguided steps
    assert [e[0] for e in st.log] == kinds
    assert [bool(e[1]) for e in st.log] == mirror
    # a refresh runs over the 2B utterances under the guided class, the others over B under the unguided one (batch_class 3, N = S)
    assert [(e[2], e[3]) for e in st.log] == [(2 * B, 2 * 3 * S) if kind == R else (B, 3 * S) for kind in kinds]
    assert torch.equal(out, torch.arange(S * D, dtype=torch.float32).reshape(S, D) + 6.0)


# ---------------------------------------------------------------------------------------------------------------- the C ABI
NEW = ("ditto_guided_update_packed_reuse", "ditto_multistep_update_packed_reuse", "ditto_guided_step_packed_reuse_opts",
       "ditto_guided_step_packed_multistep_reuse_opts")


def test_new_symbols_and_their_refusals():
    lib, p = hip.lib(), 4096                                      # a non-NULL pointer value: every call fails before anything reads it
    names = declared_functions()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n in hip.SYMBOLS
    assert lib.ditto_abi_version() == 10                          # additive entries: the version stays
    assert (hip.REUSE_STORE, hip.REUSE_LOAD) == (1, 2)
    coef = hip.MultistepCoef(0.8, 1.9, -1.6, 0.4, -0.1, 0.0, 1, 0)
    upd = dict(x=p, eps=p, delta=p, noise=None, seeds=None, step=0, w=p, a=p, ce=p, cz=p, cu=p, pl=None, ql=None, B=2, S=128,
               max_N=64, d=256, mode=2, mirror=0, stream=None)
    ms = dict(x=p, eps=p, q=p, delta=p, step=coef, w=p, cu=p, pl=None, ql=None, B=2, S=128, max_N=64, d=256, mode=2, mirror=0,
              stream=None)
    step = dict(m=None, x=p, cond=p, t=p, cu=p, cut=p, pl=None, ql=None, delta=p, noise=None, seeds=None, step=0, w=p, a=p, ce=p, cz=p,
                B=2, S=128, max_N=64, S_T=16, max_T=8, mode=2, mirror=0, rc=p, rs=p, ws=p, wsb=1 << 20, stream=None, opts=None)
    for fn, ok in ((lib.ditto_guided_update_packed_reuse, upd), (lib.ditto_multistep_update_packed_reuse, ms)):
        call = lambda **k: fn(*{**ok, **k}.values())              # noqa: E731, B023
        for over, code in ((dict(delta=None), hip.ERR_ARG), (dict(mode=0), hip.ERR_ARG), (dict(mode=3), hip.ERR_ARG),
                           (dict(mode=1, mirror=1), hip.ERR_ARG), (dict(w=None), hip.ERR_ARG), (dict(cu=None), hip.ERR_ARG),
                           (dict(x=None), hip.ERR_ARG), (dict(eps=None), hip.ERR_ARG), (dict(d=96), hip.ERR_SHAPE),
                           (dict(B=0), hip.ERR_SHAPE), (dict(S=0), hip.ERR_SHAPE), (dict(max_N=129), hip.ERR_SHAPE),
                           (dict(B=65536, S=70000), hip.ERR_SHAPE)):
            assert call(**over) == code, (fn, over, lib.ditto_last_error())
    assert lib.ditto_guided_update_packed_reuse(*{**upd, "noise": p, "seeds": p}.values()) == hip.ERR_ARG
    assert lib.ditto_multistep_update_packed_reuse(*{**ms, "step": None}.values()) == hip.ERR_ARG
    assert lib.ditto_multistep_update_packed_reuse(*{**ms, "q": None}.values()) == hip.ERR_ARG
    assert lib.ditto_guided_step_packed_reuse_opts(*step.values()) == hip.ERR_ARG          # no model
