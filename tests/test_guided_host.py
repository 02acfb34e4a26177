"""The guided strided step on the host (no GPU): both C entry points are declared, exported and bound with the ABI still 10; each bad
argument returns its error code and message before any launch; the schedule helper is the oracle's strided DDIM schedule; guidance
normalisation refuses what the kernel must not see."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.sampler import guidance_vector, strided_schedule
from oracle import ditto_oracle as O
from test_cabi_symbols import declared_functions

ENTRIES = ("ditto_guided_update", "ditto_guided_step_opts")
P = 4096   # a non-NULL pointer value: every call below fails its argument checks before anything touches it


def test_guided_symbols_declared_exported_and_bound():
    lib = hip.lib()
    names = declared_functions()
    for n in ENTRIES:
        assert n in names and hasattr(lib, n) and n in hip.SYMBOLS
    assert lib.ditto_abi_version() == 10


def _update(lib, x2=P, eps2=P, noise=None, seeds=None, w=P, a=P, ce=P, cz=P, B=2, N=64, d=256, cfg=1):
    return lib.ditto_guided_update(x2, eps2, noise, seeds, 0, w, a, ce, cz, None, B, N, d, cfg, None)


UPDATE_CASES = [(dict(x2=None), hip.ERR_ARG, b"x2"), (dict(eps2=None), hip.ERR_ARG, b"eps2"),
                (dict(noise=P, seeds=P), hip.ERR_ARG, b"exclusive"), (dict(w=None), hip.ERR_ARG, b"needs w"),
                (dict(a=None), hip.ERR_ARG, b"null a"), (dict(cz=None, seeds=P), hip.ERR_ARG, b"cz"),
                (dict(B=0), hip.ERR_SHAPE, b"positive"), (dict(B=-1), hip.ERR_SHAPE, b"positive"),
                (dict(N=0), hip.ERR_SHAPE, b"positive"), (dict(d=0), hip.ERR_SHAPE, b"positive"),
                (dict(d=96), hip.ERR_SHAPE, b"% 64"), (dict(d=260), hip.ERR_SHAPE, b"% 64")]


@pytest.mark.parametrize("kw,code,word", UPDATE_CASES, ids=[",".join(k for k in c[0]) + f"_{i}" for i, c in enumerate(UPDATE_CASES)])
def test_guided_update_refuses_bad_arguments(kw, code, word):
    lib = hip.lib()
    assert _update(lib, **kw) == code, kw
    assert word in lib.ditto_last_error(), (kw, lib.ditto_last_error())


def _step(lib, m=P, x2=P, sl=None, tl=None, noise=None, seeds=None, w=P, B=2, N=64, T=64, cfg=1, ws=P):
    return lib.ditto_guided_step_opts(m, x2, P, P, sl, tl, noise, seeds, 0, w, P, P, P, B, N, T, cfg, P, P, ws, 1 << 30, None, None)


def test_guided_step_refuses_bad_arguments():
    lib = hip.lib()
    for kw, code, word in [(dict(m=None), hip.ERR_ARG, b"bad argument"), (dict(ws=None), hip.ERR_ARG, b"bad argument"),
                           (dict(sl=P), hip.ERR_ARG, b"both"), (dict(tl=P), hip.ERR_ARG, b"both"),
                           (dict(T=0), hip.ERR_SHAPE, b"T must be positive")]:
        assert _step(lib, **kw) == code, kw
        assert word in lib.ditto_last_error(), (kw, lib.ditto_last_error())


@pytest.mark.parametrize("T,n_steps", [(50, 25), (50, 50), (50, 1), (50, 7), (1000, 25)])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_schedule_is_the_oracles(T, n_steps, eta):
    ac = O.sampler_tables(T)[2]
    got = strided_schedule(ac, n_steps, eta)
    taus = O.strided_timesteps(T, n_steps)
    assert [g[0] for g in got] == taus
    for i, (t_val, a, ce, sigma) in enumerate(got):
        t_prev = taus[i + 1] if i + 1 < n_steps else -1
        assert (a, ce, sigma) == O.ddim_coefficients(ac.double(), t_val, t_prev, eta)
    with pytest.raises(ValueError):
        strided_schedule(ac, 0)
    with pytest.raises(ValueError):
        strided_schedule(ac, T + 1)


def test_guidance_normalisation():
    assert guidance_vector(None, 3) is None
    for g in (5.0, 5, [5.0, 5.0, 5.0], (5, 5.0, 5), torch.tensor([5.0, 5.0, 5.0]), torch.tensor([5, 5, 5])):
        v = guidance_vector(g, 3)
        assert v.dtype == torch.float32 and v.device.type == "cpu" and v.tolist() == [5.0, 5.0, 5.0]
    assert guidance_vector([5.0, 1.5, 0.0], 3).tolist() == [5.0, 1.5, 0.0]


@pytest.mark.parametrize("bad", [[1.0, 2.0], [[1.0, 2.0, 3.0]], torch.ones(3, 1), torch.ones(4), [1.0, "2", 3.0], True,
                                 [1.0, True, 3.0], "5", torch.tensor([1.0, float("nan"), 2.0]), [1.0, float("inf"), 2.0]],
                         ids=["short", "nested", "2d", "long_tensor", "string_item", "bool", "bool_item", "string", "nan", "inf"])
def test_guidance_normalisation_rejects(bad):
    with pytest.raises(ValueError):
        guidance_vector(bad, 3)
