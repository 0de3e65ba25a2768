"""CPU: the fp64 statement of clip + AdamW (tests/optim_ref.py) against torch, and its bound against torch's own fp32.

* the statement, iterated in float64, equals ``clip_grad_norm_`` + ``torch.optim.AdamW(foreach=False)`` on float64 tensors
  at float64 rounding level over several steps;
* torch's fp32 CPU clip + AdamW, teacher-forced from the same fp32 state as the kernels are, stays inside the asserted
  bounds of p, m and v on EVERY element of every case of the shared table -- the bound can be met by a correct fp32
  evaluation and the inputs are well conditioned;
* NaN and inf gradients: the statement and torch agree, including on which elements are not finite.

The worst fractions are printed (``pytest -s``)."""
import math

import numpy as np
import pytest
import torch

import optim_ref as R


def _torch_step(params, grads, ms, vs, hyper, t, max_norm, dtype):
    """One clip + AdamW step of torch from the given state.  Returns (new p, m, v lists, norm, coef) -- coef formed from
    torch's own norm by the expression clip_grad_norm_ uses, in ``dtype``."""
    lr, b1, b2, eps, wd = hyper
    ps = [torch.nn.Parameter(torch.as_tensor(p, dtype=dtype).clone()) for p in params]
    opt = torch.optim.AdamW(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    for p, g, m, v in zip(ps, grads, ms, vs):
        p.grad = torch.as_tensor(g, dtype=dtype).clone()
        opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.as_tensor(m, dtype=dtype).clone(),
                        "exp_avg_sq": torch.as_tensor(v, dtype=dtype).clone()}
    norm, coef = None, 1.0
    if max_norm is not None:
        norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        coef = float(torch.clamp(max_norm / (norm + 1e-6), max=1.0))
        norm = float(norm)
    opt.step()
    assert all(float(opt.state[p]["step"]) == t for p in ps)
    return ([p.detach() for p in ps], [opt.state[p]["exp_avg"] for p in ps], [opt.state[p]["exp_avg_sq"] for p in ps], norm, coef)


def test_statement_equals_torch_float64_over_several_steps():
    """Five steps carried in float64 (not teacher-forced): clip active at first, two parameter sizes, weight decay on."""
    rng = np.random.default_rng(3)
    hyper = (1e-2, 0.9, 0.999, 1e-8, 0.1)
    sizes = (1, 5, 1021, 8193)
    p = [torch.from_numpy(rng.standard_normal(n)) for n in sizes]
    m = [torch.zeros(n, dtype=torch.float64) for n in sizes]
    v = [torch.zeros(n, dtype=torch.float64) for n in sizes]
    tp, tm, tv = p, m, v
    worst = 0.0
    for t in range(1, 6):
        g = [torch.from_numpy(rng.standard_normal(n) * (5.0 if t < 3 else 1e-3)) for n in sizes]
        norm, coef = R.clip(g, 1.0)
        assert (coef < 1.0) == (t < 3)
        tp, tm, tv, tnorm, tcoef = _torch_step(tp, g, tm, tv, hyper, t, 1.0, torch.float64)
        assert abs(tnorm - norm) <= 1e-14 * norm and abs(tcoef - coef) <= 1e-14 * coef
        ref = [R.update(p[i], g[i], m[i], v[i], hyper, t, coef) for i in range(len(sizes))]
        p, m, v = [r["p"] for r in ref], [r["m"] for r in ref], [r["v"] for r in ref]
        for mine, theirs in ((p, tp), (m, tm), (v, tv)):
            for a, b in zip(mine, theirs):
                rel = float((a - b).abs().max() / b.abs().max())
                worst = max(worst, rel)
                assert rel <= 1e-13, (t, rel)
    print(f"statement against torch float64 over 5 steps: worst difference {worst:.2e} of the largest element")


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_torch_fp32_adamw_stays_inside_the_bounds(case):
    """torch's fp32 clip_grad_norm_ + single-tensor AdamW on the case's inputs, from the same fp32 state: p, m and v within
    the bounds on every element; the fp32 norm within 2e-6 of the float64 norm and the coefficient within 3 u of the
    float64 expression of torch's own norm."""
    x = R.case_inputs(case)
    hyper = R.case_hyper(case)
    tp, tm, tv, norm32, coef32 = _torch_step(x["p"], x["g"], x["m"], x["v"], hyper, case["t"], case["clip"], torch.float32)
    if case["clip"] is not None:
        norm, coef = R.clip(x["g"], case["clip"])
        assert abs(norm32 - norm) <= R.NORM_RTOL * norm
        want = R.coef_from_norm(norm32, case["clip"])
        assert abs(coef32 - want) <= R.COEF_RTOL * want
        assert (coef32 < 1.0) == (case["gscale"] > 1.0)
        print(f"{case['name']}: torch fp32 norm off by {abs(norm32 - norm) / norm / R.U:.2f} u")
    worst = [0.0, 0.0, 0.0]
    for i in range(len(x["p"])):
        ref = R.update(x["p"][i], x["g"][i], x["m"][i], x["v"][i], hyper, case["t"], coef32)
        fr = R.fractions(tp[i], tm[i], tv[i], ref)
        worst = [max(a, b) for a, b in zip(worst, fr)]
        assert not torch.equal(tp[i], torch.from_numpy(x["p"][i]))
    print(f"{case['name']}: torch fp32 worst fraction of the bound p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")
    assert max(worst) <= 1.0, worst


def test_bound_is_not_slack_against_value_errors():
    """The bound is small against what a wrong scalar does: a step count off by one (t = 2), eps and weight decay
    exchanged, or a dropped clip coefficient move the statement's p by far more than Ep on nearly every element."""
    case = R.CASES[6]
    assert case["t"] == 2 and case["clip"] is not None
    x = R.case_inputs(case, [4096])
    lr, b1, b2, eps, wd = R.case_hyper(case)
    _, coef = R.clip(x["g"], case["clip"])
    coef = R.f32(coef)
    a = (x["p"][0], x["g"][0], x["m"][0], x["v"][0])
    ref = R.update(*a, (lr, b1, b2, eps, wd), 2, coef)
    for name, other in (("step", R.update(*a, (lr, b1, b2, eps, wd), 1, coef)),
                        ("eps<->wd", R.update(*a, (lr, b1, b2, wd, eps), 2, coef)),
                        ("coef", R.update(*a, (lr, b1, b2, eps, wd), 2, 1.0))):
        ratio = (other["p"] - ref["p"]).abs() / ref["Ep"]
        assert float(ratio.median()) > 100.0, (name, float(ratio.median()))


@pytest.mark.parametrize("bad", ["nan", "inf", "-inf"])
def test_non_finite_gradients_as_torch(bad):
    """One non-finite gradient element.  NaN: norm and coefficient NaN, every stepped element NaN.  inf: norm inf,
    coefficient 0, NaN at that element and g' = 0 everywhere else (the moments decay, the parameter moves by the old first
    moment).  The statement matches torch's fp32 run in the pattern of non-finite elements, and on the finite ones torch
    is inside the bound."""
    case = R.CASES[3]
    sizes = [5, 1021, R.CHUNK + 1]
    x = R.case_inputs(case, sizes)
    x["g"][1][77] = float(bad)
    hyper = R.case_hyper(case)
    norm, coef = R.clip(x["g"], 1.0)
    tp, tm, tv, norm32, coef32 = _torch_step(x["p"], x["g"], x["m"], x["v"], hyper, case["t"], 1.0, torch.float32)
    if bad == "nan":
        assert math.isnan(norm) and math.isnan(coef) and math.isnan(norm32) and math.isnan(coef32)
    else:
        assert norm == math.inf and coef == 0.0 and norm32 == math.inf and coef32 == 0.0
    for i in range(len(sizes)):
        ref = R.update(x["p"][i], x["g"][i], x["m"][i], x["v"][i], hyper, case["t"], coef)
        for got, key in ((tp[i], "p"), (tm[i], "m"), (tv[i], "v")):
            assert torch.equal(torch.isfinite(got), torch.isfinite(ref[key])), (i, key)
            assert torch.equal(torch.isnan(got), torch.isnan(ref[key])), (i, key)
            n_bad = int((~torch.isfinite(got)).sum())
            assert n_bad == (got.numel() if bad == "nan" else (1 if i == 1 else 0)), (i, key, n_bad)
        if bad != "nan" and i == 1:
            assert bool(torch.isnan(tp[i][77]))
        assert max(R.fractions(tp[i], tm[i], tv[i], ref)) <= 1.0
