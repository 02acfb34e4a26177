"""tests/optim_ref.py checked on the host: its float64 chain against torch's own clip_grad_norm_ + AdamW(foreach=False) + lerp_ on
float64 tensors; its bounds against an fp32 imitation of the kernel's arithmetic on the GPU test's inputs (admitted) and against each
modelled defect (refused).  The worst admitted and the least refused ratio are printed; DESIGN.md section 4.5 records them."""
import numpy as np
import pytest
import torch

import optim_ref as R


def _zeros(tensors):
    return [torch.zeros_like(t) for t in tensors]


def test_chain_is_torchs_clip_adamw_lerp_in_float64():
    p0, e0 = R.case_params()
    params = [torch.nn.Parameter(t.double()) for t in p0]
    groups = [{"params": [q for i, q in enumerate(params) if i % 2 == k], "lr": R.CASE_GROUPS[k][0], "weight_decay": R.CASE_GROUPS[k][1]}
              for k in range(2)]
    opt = torch.optim.AdamW(groups, betas=R.CASE_BETAS, eps=R.CASE_EPS, foreach=False)
    ema_t = [t.double().clone() for t in e0]
    p, m, v, ema = [t.double() for t in p0], _zeros([t.double() for t in p0]), _zeros([t.double() for t in p0]), [t.double() for t in e0]
    for step in range(1, R.CASE_STEPS + 1):
        grads = R.case_grads(step)
        for q, g in zip(params, grads):
            q.grad = g.double().clone()
        total = torch.nn.utils.clip_grad_norm_(params, R.CASE_MAX_NORM, foreach=False)
        opt.step()
        with torch.no_grad():
            for e, q in zip(ema_t, params):
                e.lerp_(q, 1.0 - R.CASE_DECAY)
        norm = R.global_norm(grads)
        assert abs(norm - float(total)) <= 1e-13 * norm
        clip = R.clip_factor(norm, R.CASE_MAX_NORM)
        assert 0.2 < clip < 0.5                        # the case does clip
        for i in range(len(p)):
            lr, wd = R.case_lr_wd(i)
            out, _ = R.chain_fp64(p[i], grads[i], m[i], v[i], ema[i], step, lr, wd, clip=clip)
            p[i], m[i], v[i], ema[i] = out["p"], out["m"], out["v"], out["ema"]
            st = opt.state[params[i]]
            for got, want in ((p[i], params[i].detach()), (m[i], st["exp_avg"]), (v[i], st["exp_avg_sq"]), (ema[i], ema_t[i])):
                assert torch.allclose(got, want, rtol=1e-12, atol=1e-15), (step, i)


def _run(bug=None):
    """three clipped steps of the imitation (state carried in fp32, as on the GPU), each step held against the float64 chain from the
    SAME fp32 state -> the worst ratio of every tensor kind"""
    p0, e0 = R.case_params()
    n = len(p0)
    p = [t.numpy().copy() for t in p0]
    ema = [None if i == R.CASE_NO_EMA else e0[i].numpy().copy() for i in range(n)]
    m, v = [np.zeros_like(x) for x in p], [np.zeros_like(x) for x in p]
    worst = {"p": 0.0, "m": 0.0, "v": 0.0, "ema": 0.0}
    for step in range(1, R.CASE_STEPS + 1):
        grads = R.case_grads(step)
        clip = R.clip_factor(R.imitate_norm([g.numpy() for g in grads]), R.CASE_MAX_NORM)
        clip_ref = R.clip_factor(R.global_norm(grads), R.CASE_MAX_NORM)
        for i in range(n):
            lr, wd = R.case_lr_wd(i)
            T = lambda a: None if a is None else torch.from_numpy(a)      # noqa: E731
            want, bound = R.chain_fp64(T(p[i]), grads[i], T(m[i]), T(v[i]), T(ema[i]), step, lr, wd, clip=clip_ref)
            lr_k, wd_k = R.case_lr_wd(i + 1) if bug == "wrong_lr" else (lr, wd)
            got = R.imitate(p[i], grads[i].numpy(), m[i], v[i], ema[i], step, lr_k, wd_k, clip=clip,
                            bug=None if bug == "wrong_lr" else bug)
            for key in got:
                worst[key] = max(worst[key], R.worst_ratio(torch.from_numpy(got[key]), want[key], bound[key]))
            p[i], m[i], v[i] = got["p"], got["m"], got["v"]
            if ema[i] is not None:
                ema[i] = got["ema"]
    return worst


def test_bounds_admit_the_fp32_imitation():
    worst = _run()
    print("optim bounds: worst admitted ratio per tensor", worst)
    assert max(worst.values()) <= 1.0, worst
    assert min(worst.values()) > 0.02, worst          # and are not slack by orders of magnitude


@pytest.mark.parametrize("bug", R.BUGS)
def test_bounds_refuse_each_modelled_defect(bug):
    worst = _run(bug)
    print(f"optim bounds: defect {bug}: ratios {worst}")
    assert max(worst.values()) > 1.0, (bug, worst)


def test_norm_bound_admits_another_summation_order():
    grads = R.case_grads(1)
    n = sum(g.numel() for g in grads)
    a, b = R.global_norm(grads), R.imitate_norm([g.numpy() for g in grads])
    assert abs(a - b) <= R.norm_rtol(n) * a, (a, b)
    assert R.norm_rtol(n) < 1e-10
    g2 = [g.clone() for g in grads]
    g2[-1][-1] += 1e-3                                  # one tail element: far outside the bound
    assert abs(R.global_norm(g2) - a) > 100 * R.norm_rtol(n) * a
