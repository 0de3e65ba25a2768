"""CPU: the host side of multistep (DPM-Solver++ 2M, capped weight) structure sampling -- utils.MultistepTables against
the numpy float64 statement (tests/multistep_ref.py) and against StridedTables at eta = 0, whose first four columns it
shares bit for bit; the solver error of the rule against DDIM's on a model with a closed-form solution, in float64;
argument checks that raise before any device is touched; and the C-ABI entry point's declaration."""
import os

import numpy as np
import pytest
import torch

import multistep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _order(T, step):
    return list(reversed(range(0, T, step)))


@pytest.mark.parametrize("T,order", [(1000, _order(1000, 20)), (1000, _order(1000, 50)), (1000, _order(1000, 100)),
                                     (10, [9, 4, 0]), (10, [7, 2]), (10, [3])])
def test_tables_equal_the_ref_rounded_to_fp32(pkg, T, order):
    from e3diff_amd.structure_model.utils import CosineTables, MultistepTables, StridedTables
    tab = CosineTables(T)
    mt = MultistepTables(tab, order)
    got, want = mt.coef.numpy(), R.table(tab.betas.numpy(), order)
    assert mt.coef.dtype == torch.float32 and got.shape == (T, 8)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    visited = np.zeros(T, dtype=bool)
    visited[order] = True
    assert np.isnan(got[~visited]).all() and np.isfinite(got[visited]).all()
    assert (got[visited][:, 5:] == 0).all()
    # the DDIM part of the row is the strided table's at eta = 0, bit for bit
    st = StridedTables(tab, order, 0.0).coef.numpy()
    assert np.array_equal(got[order][:, :4].view(np.uint32), st[order][:, :4].view(np.uint32))
    # the weights: none at either end, at most the cap between
    w = mt.weights
    assert w.dtype == torch.float64 and tuple(w.shape) == (len(order),)
    assert np.array_equal(w.numpy(), R.weights(tab.betas.numpy(), order))
    assert w[0] == 0.0 and w[-1] == 0.0 and (w >= 0.0).all() and (w <= 0.5).all()
    assert got[order[0], 4] == 0.0 and got[order[-1], 4] == 0.0
    if len(order) > 2:
        assert (w[1:-1] > 0.0).all() and (got[order[1:-1], 4] > 0.0).all()
    assert mt.order == order and mt.timesteps == T and mt.w_max == 0.5
    assert [mt.successor(t) for t in order] == order[1:] + [-1]


def test_the_cap_acts_on_the_step_that_lands_on_zero(pkg):
    from e3diff_amd.structure_model.utils import CosineTables, MultistepTables
    tab = CosineTables(1000)
    order = _order(1000, 100)
    capped, free = MultistepTables(tab, order), MultistepTables(tab, order, w_max=None)
    assert free.w_max is None and np.array_equal(free.weights.numpy(), R.weights(tab.betas.numpy(), order, None))
    # t = 100 lands on t = 0: beta_0 is clipped, the log-SNR step is several times its predecessor's
    assert order[-2] == 100 and 2.0 < float(free.weights[-2]) < 2.2 and float(capped.weights[-2]) == 0.5
    assert float(free.weights[1]) < 0.5 and float(capped.weights[1]) == float(free.weights[1])    # no cap where none is needed
    acted = capped.weights != free.weights
    assert acted[-2] and not acted[0] and not acted[-1]
    assert np.array_equal(free.coef.numpy().view(np.uint32), R.table(tab.betas.numpy(), order, None).view(np.uint32))
    assert torch.equal(capped.coef[order][:, :4], free.coef[order][:, :4])
    assert float(free.coef[100, 4]) > 4.0 * float(capped.coef[100, 4])


def test_argument_errors_of_the_tables(pkg):
    from e3diff_amd.structure_model.utils import CosineTables, MultistepTables
    tab = CosineTables(10)
    with pytest.raises(ValueError, match="empty"):
        MultistepTables(tab, [])
    for order in ([5, 5, 0], [0, 5], [9, 3, 4]):
        with pytest.raises(ValueError, match="descending"):
            MultistepTables(tab, order)
    for order in ([10, 5], [5, -1]):
        with pytest.raises(ValueError, match=r"\[0, 10\)"):
            MultistepTables(tab, order)
    with pytest.raises(ValueError, match="w_max"):
        MultistepTables(tab, [9, 4, 0], w_max=-0.5)
    # CosineTables is untouched by building multistep tables from it
    before = {k: v.clone() for k, v in tab.as_dict().items()}
    MultistepTables(tab, [9, 4, 0])
    assert all(torch.equal(v, before[k]) for k, v in tab.as_dict().items())


@pytest.mark.parametrize("steps", [10, 20, 50])
@pytest.mark.parametrize("v", [0.05, 0.25, 1.0])
def test_solver_error_is_at_most_half_of_ddims(pkg, v, steps):
    """Gaussian data N(0.3, v): the probability-flow ODE has a closed-form end point (multistep_ref).  At the same number
    of decoder forwards the multistep chain ends at most half as far from it as the DDIM chain.  float64, real line."""
    from e3diff_amd.structure_model.utils import CosineTables, MultistepTables
    tab = CosineTables(1000)
    betas = tab.betas.double().numpy()
    order = _order(1000, 1000 // steps)
    assert len(order) == steps
    x_T = np.random.default_rng(0).standard_normal(4096)
    ddim = R.gaussian_max_error(betas, order, x_T, 0.3, v, "ddim")
    multi = R.gaussian_max_error(betas, order, x_T, 0.3, v, "multistep")
    paper = R.gaussian_max_error(betas, order, x_T, 0.3, v, "multistep", w_max=None)
    print(f"v={v} steps={steps}: max error ddim {ddim:.3g}, multistep {multi:.3g} (x{ddim / multi:.1f}), uncapped {paper:.3g}")
    assert multi <= 0.5 * ddim
    # the chain of the package's own table (float64 from its fp32 rows) is that chain up to the rounding of the rows
    rows = MultistepTables(tab, order).coef.numpy()
    ab = R.alphas_cumprod(betas)
    x, prev = x_T, np.full_like(x_T, np.nan)
    for t in order:
        x, prev, _ = R.update(rows[t], x, R.gaussian_eps(x, ab[t], 0.3, v), prev)
    assert np.abs(x - R.gaussian_chain(betas, order, x_T, 0.3, v)).max() < 1e-4


def test_the_sampler_checks_its_arguments_before_it_touches_a_device(pkg):
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.utils import CosineTables, MultistepTables, StridedTables
    B, L, T = 2, 32, 3
    x, m, betas = torch.zeros(B, L, 8), torch.ones(B, L), torch.full((T,), 0.1)
    with pytest.raises(ValueError, match="eta"):
        S.p_sample_loop(None, m, x, None, m, None, T, betas, update="multistep", eta=0.5)
    with pytest.raises(ValueError, match="update"):
        S.p_sample_loop(None, m, x, None, m, None, T, betas, update="ddim")
    with pytest.raises(ValueError, match="strided"):
        S.p_sample_loop(None, m, x, None, m, None, T, betas, update="ancestral", eta=0.5)
    with pytest.raises(ValueError, match="strided"):
        S.p_sample_loop(None, m, x, None, m, None, T, betas, wrap_x0=True)
    tab = CosineTables(6)
    order = [5, 3, 2, 0]
    mt = MultistepTables(tab, order)
    with pytest.raises(ValueError, match="one of them"):
        S.step_plan(tab, "cpu", strided=StridedTables(tab, order), multistep=mt)
    with pytest.raises(TypeError, match="MultistepTables"):
        S.step_plan(tab, "cpu", multistep=mt.coef)
    with pytest.raises(TypeError, match="MultistepTables"):
        S.step_plan(tab, "cpu", multistep=StridedTables(tab, order))
    with pytest.raises(ValueError, match="strided"):
        S.step_plan(tab, "cpu", wrap_x0=True)
    with pytest.raises(ValueError, match="history"):
        S.p_sample(None, m, x, None, m, None, 3, tab, multistep=mt)
    with pytest.raises(ValueError, match="history"):
        S.p_sample(None, m, x, None, m, None, 3, tab, history=torch.zeros_like(x))
    assert S.UPDATE in ("ancestral", "strided", "multistep")


def test_a_multistep_plan(pkg):
    """The frozen record: the table's order and [T,8] rows, no draws at any timestep, wrap_x0 allowed, keyed or not; the
    history is the chain's and reaches the launch through ``update``."""
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.utils import CosineTables, MultistepTables
    tab = CosineTables(6)
    order = [5, 3, 2, 0]
    mt = MultistepTables(tab, order)
    keys = pkg.keyed.padded_keys([4, 9], 8, "cpu")
    for kw in ({}, {"wrap_x0": True}, {"row_keys": keys, "seed": 5}):
        plan = S.step_plan(tab, "cpu", multistep=mt, **kw)
        assert plan.multistep is mt and plan.strided is None and list(plan.order) == order
        assert plan.coef.shape == (6, 8) and plan.coef.dtype == torch.float32
        assert torch.equal(plan.coef[order], mt.coef[order]) and torch.equal(plan.coef.isnan(), mt.coef.isnan())
        assert plan.wrap_x0 is bool(kw.get("wrap_x0", False))
        assert not any(plan.update_draws(t) for t in order) and not any(plan.compose_draws(t) for t in order)
        assert not hasattr(plan, "history")
    x = torch.zeros(2, 8, 8)
    with pytest.raises(ValueError, match="history"):
        plan.update(x, x, torch.zeros(2, dtype=torch.long), None, None, True, 3)


def test_the_kernel_is_declared(pkg):
    header = open(os.path.join(ROOT, "include", "e3d_hip.h")).read()
    assert "e3d_multistep_step_wrap(" in header and "e3d_multistep_step_wrap" in pkg.hip.EXPORTS
    assert "e3d_keyed_multistep_step_wrap" not in pkg.hip.EXPORTS          # the rule draws nothing: no keyed form
    assert pkg.hip.ABI_VERSION == 5
    lib = pkg.hip.lib()
    # argument validation before any launch: callable without a GPU
    assert lib.e3d_multistep_step_wrap(None, None, None, None, None, 10, 1, 0, None, None, 8, None) < 0
    assert b"multistep_step_wrap" in lib.e3d_last_error()
    assert callable(pkg.ops.multistep_step_wrap)
