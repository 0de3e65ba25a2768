"""CPU: the host side of strided (DDIM / respaced) structure sampling -- utils.StridedTables against the numpy float64
statement (tests/strided_ref.py) and against the DDPM posterior it must reduce to at stride 1 and eta = 1; argument
checks; and the two C-ABI entry points, which validate their arguments before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import strided_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _order(T, step):
    return list(reversed(range(0, T, step)))


def test_stride_one_eta_one_is_the_ddpm_posterior(pkg):
    """order = T-1 .. 0, eta = 1: x0 form == posterior mean (1/sqrt(alpha_t)) (x - beta_t e / sqrt(1 - ab_t)) and
    sigma^2 == beta_t (1 - ab_{t-1}) / (1 - ab_t), in float64 from the same betas, within 1e-10."""
    from e3diff_amd.structure_model.utils import CosineTables
    betas = CosineTables(1000).betas.double().numpy()
    T = len(betas)
    c = R.coefficients(betas, _order(T, 1), 1.0)[::-1]          # row t
    s1m, rsa, a_s, c_dir, sigma = c.T
    ab = R.alphas_cumprod(betas)
    ab_prev = np.concatenate([[1.0], ab[:-1]])
    var = betas * (1.0 - ab_prev) / (1.0 - ab)
    assert np.abs(sigma ** 2 - var).max() <= 1e-10
    # mean = kx x + ke e on both sides; compare the two linear coefficients, and the mean on random inputs
    kx, ke = a_s * rsa, c_dir - a_s * rsa * s1m
    want_kx = 1.0 / np.sqrt(1.0 - betas)
    want_ke = -want_kx * betas / np.sqrt(1.0 - ab)
    rng = np.random.default_rng(0)
    x, e = rng.uniform(-np.pi, np.pi, (T, 64)), rng.standard_normal((T, 64))
    got = a_s[:, None] * ((x - s1m[:, None] * e) * rsa[:, None]) + c_dir[:, None] * e
    want = want_kx[:, None] * (x - betas[:, None] * e / np.sqrt(1.0 - ab)[:, None])
    err = np.abs(got - want).max()
    print(f"posterior mean: max |strided - ddpm| = {err:.2e}; coefficients {np.abs(kx / want_kx - 1).max():.2e}")
    assert err <= 1e-10
    assert np.abs(ke - want_ke).max() <= 1e-10
    assert np.abs(kx / want_kx - 1.0).max() <= 1e-10


@pytest.mark.parametrize("T,step,eta", [(1000, 20, 0.0), (1000, 1, 1.0), (50, 7, 0.5), (6, 4, 1.0)])
def test_tables_equal_the_ref_rounded_to_fp32(pkg, T, step, eta):
    from e3diff_amd.structure_model.utils import CosineTables, StridedTables
    tab = CosineTables(T)
    order = _order(T, step)
    st = StridedTables(tab, order, eta)
    want = R.table(tab.betas.numpy(), order, eta)
    got = st.coef.numpy()
    assert st.coef.dtype == torch.float32 and got.shape == (T, 8)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    visited = np.zeros(T, dtype=bool)
    visited[order] = True
    assert np.isnan(got[~visited]).all() and np.isfinite(got[visited]).all()
    assert (got[visited][:, 5:] == 0).all()
    last = got[order[-1]]
    assert last[2] == 1.0 and last[3] == 0.0 and last[4] == 0.0          # a_s = 1, c_dir = 0, sigma = 0
    assert st.order == order and st.eta == eta and st.timesteps == T
    if eta == 0.0:
        assert (got[visited][:, 4] == 0).all()
    else:
        assert (got[order[:-1], 4] > 0).all()


def test_eta_zero_has_no_sigma(pkg):
    from e3diff_amd.structure_model.utils import CosineTables, StridedTables
    for T, step in ((1000, 20), (1000, 1), (12, 3)):
        st = StridedTables(CosineTables(T), _order(T, step))
        assert st.eta == 0.0 and (st.coef[st.order, 4] == 0).all()


def test_argument_errors(pkg):
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.utils import CosineTables, StridedTables
    tab = CosineTables(10)
    for eta in (-0.1, 1.5):
        with pytest.raises(ValueError, match="eta"):
            StridedTables(tab, [9, 5, 0], eta)
    for order in ([5, 5, 0], [0, 5], [9, 3, 4]):
        with pytest.raises(ValueError, match="descending"):
            StridedTables(tab, order)
    for order in ([10, 5], [5, -1]):
        with pytest.raises(ValueError, match=r"\[0, 10\)"):
            StridedTables(tab, order)
    # CosineTables is untouched by building strided tables from it
    before = {k: v.clone() for k, v in tab.as_dict().items()}
    StridedTables(tab, [9, 4, 0], 1.0)
    assert all(torch.equal(v, before[k]) for k, v in tab.as_dict().items())
    # the sampler refuses strided arguments with the ancestral update before it touches a device
    B, L, T = 2, 32, 3
    x, m = torch.zeros(B, L, 8), torch.ones(B, L)
    with pytest.raises(ValueError, match="strided"):
        S.p_sample_loop(None, m, x, None, m, None, T, torch.full((T,), 0.1), update="ancestral", eta=0.5)
    with pytest.raises(ValueError, match="strided"):
        S.p_sample_loop(None, m, x, None, m, None, T, torch.full((T,), 0.1), wrap_x0=True)
    with pytest.raises(ValueError, match="update"):
        S.p_sample_loop(None, m, x, None, m, None, T, torch.full((T,), 0.1), update="ddim")
    with pytest.raises(ValueError, match="eta"):
        S.p_sample_loop(None, m, x, None, m, None, T, torch.full((T,), 0.1), update="strided", eta=2.0)
    assert S.UPDATE in ("ancestral", "strided") and 0.0 <= S.ETA <= 1.0 and isinstance(S.WRAP_X0, bool)


def test_strided_kernels_are_declared(pkg):
    header = open(os.path.join(ROOT, "include", "e3d_hip.h")).read()
    for name in ("e3d_strided_step_wrap", "e3d_keyed_strided_step_wrap"):
        assert name + "(" in header and name in pkg.hip.EXPORTS
    assert pkg.hip.ABI_VERSION == 5
    lib = pkg.hip.lib()
    # argument validation before any launch: callable without a GPU
    assert lib.e3d_strided_step_wrap(None, None, None, None, None, 10, 1, 0, None, 8, None) < 0
    assert b"strided_step_wrap" in lib.e3d_last_error()
    assert lib.e3d_keyed_strided_step_wrap(None, None, None, None, 10, None, 1, 1, 0, None, 4, 8, None) < 0
    assert b"keyed_strided_step_wrap" in lib.e3d_last_error()
    p = ctypes.c_void_p(4096)      # never dereferenced: F is checked before the launch
    assert lib.e3d_keyed_strided_step_wrap(p, p, p, p, 10, p, 1, 1, 0, p, 4, 6, None) < 0
    assert b"F=6" in lib.e3d_last_error()
    assert callable(pkg.ops.strided_step_wrap) and callable(pkg.ops.keyed_strided_step_wrap)
