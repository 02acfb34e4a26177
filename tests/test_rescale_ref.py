"""tests/rescale_ref.py on the CPU: an fp32 / fmaf emulation of the guidance-rescale kernels' arithmetic, summed in orders the
kernels do not use, lies inside the derived bound for every utterance; the n vs n - 1 convention does not move s; the degenerate
cases give exactly 1.  Inputs: N(0,1)-like values of ditto_tts_amd/synth.py, for which sigma_e stays well away from 0."""
import numpy as np
import pytest

import rescale_ref as R
from ditto_tts_amd.synth import hash_normal

WS = (0.0, 1.0, 2.5, 5.0)
SIZES = (64, 4 * R.CHUNK_QUADS, 4 * R.CHUNK_QUADS + 256, 3 * 4 * R.CHUNK_QUADS + 768)   # one row of d = 64 .. several chunks


def _utterance(n, k, offset=0.0):
    c = hash_normal((n,), "rescale_ref.c", k).numpy() + np.float32(offset)
    u = (0.8 * c + 0.6 * hash_normal((n,), "rescale_ref.u", k).numpy()).astype(np.float32) + np.float32(offset)   # correlated, as eps halves are
    return c, u


@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("n", SIZES)
def test_emulation_in_other_orders_lies_inside_the_bound(n, w):
    for k, (phi, offset) in enumerate(((1.0, 0.0), (0.7, 0.0), (0.3, 3.0))):      # the last: a mean far from 0 (the cancellation term)
        c, u = _utterance(n, 17 * k + n % 13, offset)
        ref = R.reference(c, u, w, phi)
        bs, bc = R.bound(c, u, w, phi)
        assert 0 < bs < 1e-5 and bs < bc < 2e-5, (bs, bc)             # a bound of a few fp32 roundings, not a loose tolerance
        for order in ("pairwise", "reverse", "chunks"):
            s32 = R.emulate(c, u, w, phi, order)
            assert abs(float(s32) - ref["s"]) <= bs, (n, w, phi, order, float(s32), ref["s"], bs)
            for coef in (-0.731, 1.9e-3):
                out = np.float32(coef) * s32
                assert abs(float(out) - float(np.float32(coef)) * ref["s"]) <= abs(float(np.float32(coef))) * bc


def test_the_guided_std_grows_with_w_and_the_rescale_undoes_it():
    c, u = _utterance(4096, 5)
    r = [R.reference(c, u, w, 1.0)["r"] for w in (1.0, 2.5, 5.0)]
    assert abs(r[0] - 1.0) < 1e-12 and r[0] > r[1] > r[2] and r[2] < 0.5      # w = 1: e = c; at w = 5 e is far wider than c
    e = R.guided_fp64(c, u, 5.0) * R.reference(c, u, 5.0, 1.0)["s"]
    assert abs(np.std(e) / np.std(np.float64(c)) - 1.0) < 1e-12               # phi = 1: the scaled e has sigma_c


@pytest.mark.parametrize("w", WS)
def test_n_or_n_minus_one_does_not_move_s(w):
    c, u = _utterance(640, 3)
    a, b = R.reference(c, u, w, 0.7, ddof=0), R.reference(c, u, w, 0.7, ddof=1)
    assert a["var_c"] != b["var_c"] and abs(a["s"] - b["s"]) <= 4 * 2.0 ** -53 * a["s"]


def test_degenerate_cases_give_exactly_one():
    c, u = _utterance(640, 4)
    z = np.zeros(640, np.float32)
    assert R.reference(c, u, 5.0, 0.0)["s"] == 1.0 and R.bound(c, u, 5.0, 0.0) == (0.0, 0.0)            # phi == 0
    assert R.reference(c, u, 5.0, 0.7, guided=False)["s"] == 1.0                                         # unguided
    assert R.reference(z, z, 5.0, 0.7)["s"] == 1.0 and R.emulate(z, z, 5.0, 0.7) == np.float32(1.0)      # sigma_e == 0
    assert R.reference(c, u, 5.0, -3.0)["s"] == 1.0 and R.emulate(c, u, 5.0, 0.0) == np.float32(1.0)     # phi clamps into [0, 1]
    assert R.reference(c, u, 5.0, 7.0)["s"] == R.reference(c, u, 5.0, 1.0)["s"]
