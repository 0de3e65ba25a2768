"""numpy float64 statement of the second-order multistep update (DPM-Solver++ 2M, Lu et al. 2022, data-prediction form,
with the extrapolation weight capped), written from the formulas and not from the kernel: the weights and coefficient
rows of a descending order of timesteps, the per-element update with its x0 history, and a chain on a model whose
probability-flow ODE has a closed-form solution (Gaussian data).  Test infrastructure only."""
import numpy as np

from strided_ref import alphas_cumprod, circ, wrap_pi  # noqa: F401  (re-exported: the tests read them here)


def half_log_snr(ab):
    """lambda(a) = ln(a / (1 - a)) / 2."""
    ab = np.asarray(ab, dtype=np.float64)
    return 0.5 * np.log(ab / (1.0 - ab))


def weights(betas, order, w_max=0.5):
    """float64 [len(order)]: w_k = min(h_k / (2 h_{k-1}), w_max) with h_k = lambda(ab at order[k+1]) - lambda(ab at
    order[k]); 0 at the first visited timestep (no history) and at the last (the jump ends on the clean level, h is
    infinite).  ``w_max`` None: the paper's weight, not capped."""
    lam = half_log_snr(alphas_cumprod(betas)[np.asarray(order, dtype=np.int64)])
    n = len(order)
    w = np.zeros(n, dtype=np.float64)
    for k in range(1, n - 1):
        w[k] = (lam[k + 1] - lam[k]) / (2.0 * (lam[k] - lam[k - 1]))
        if w_max is not None:
            w[k] = min(w[k], w_max)
    return w


def coefficients(betas, order, w_max=0.5):
    """float64 [len(order), 5] = (s1m, rsa, a_s, c_dir, c_1) per visited t; the successor of order[k] is order[k + 1], the
    last entry's is "-1": ab_s = 1.  The DDIM jump a_s x0 + c_dir e, with e = (x - sqrt(ab_t) x0) / s1m, carries x0 with
    the factor a_s - sqrt(ab_t) c_dir / s1m; the rule puts x0 + w (x0 - prev) in x0's place, so c_1 is that factor times w."""
    ab = alphas_cumprod(betas)
    order = np.asarray(order, dtype=np.int64)
    ab_t = ab[order]
    ab_s = np.concatenate([ab[order[1:]], [1.0]])
    s1m = np.sqrt(1.0 - ab_t)
    rsa = 1.0 / np.sqrt(ab_t)
    a_s = np.sqrt(ab_s)
    c_dir = np.sqrt(np.maximum(0.0, 1.0 - ab_s))
    c_1 = (a_s - np.sqrt(ab_t) * c_dir / s1m) * weights(betas, order, w_max)
    return np.stack([s1m, rsa, a_s, c_dir, c_1], axis=1)


def table(betas, order, w_max=0.5):
    """fp32 [T, 8]: row t = (s1m, rsa, a_s, c_dir, c_1, 0, 0, 0), each rounded once; NaN rows where t is not visited."""
    out = np.full((len(betas), 8), np.nan, dtype=np.float32)
    rows = np.zeros((len(order), 8), dtype=np.float64)
    rows[:, :5] = coefficients(betas, order, w_max)
    out[np.asarray(order, dtype=np.int64)] = rows.astype(np.float32)
    return out


def update(row, x, e, prev, wrap=False, wrap_x0=False):
    """The update in float64 from one row (s1m, rsa, a_s, c_dir, c_1, ...).  ``prev``: the x0 estimate the previous step
    stored; not read where c_1 == 0.  Returns (out, hist, parts): ``hist`` is the x0 estimate this step stores; ``out`` is
    NOT wrapped whatever ``wrap`` says (``wrap`` decides whether the difference of the estimates is taken on the circle;
    the caller compares by circular distance); ``parts`` holds the values before each wrap and the magnitudes the fp32
    error bound is made of."""
    s1m, rsa, a_s, c_dir, c_1 = (float(v) for v in row[:5])
    x = np.asarray(x, dtype=np.float64)
    e = np.asarray(e, dtype=np.float64)
    x0_raw = (x - s1m * e) * rsa
    x0 = wrap_pi(x0_raw) if wrap_x0 else x0_raw
    v = a_s * x0 + c_dir * e
    zero = np.zeros_like(x)
    d_raw, d = zero, zero
    if c_1 != 0.0:
        d_raw = x0 - np.asarray(prev, dtype=np.float64)
        d = wrap_pi(d_raw) if wrap else d_raw
        v = v + c_1 * d
    parts = {"x0_raw": x0_raw, "x0": x0, "d_raw": d_raw, "d": d,
             "x0_mag": rsa * (np.abs(x) + np.abs(s1m * e)),        # what the roundings of the x0 estimate scale with
             "prev_mag": np.abs(np.asarray(prev, dtype=np.float64)) if c_1 != 0.0 else zero,
             "dir_mag": np.abs(c_dir * e)}
    return v, x0, parts


# ------------------------------------------------------------------------------------------------ an exactly solvable model
# Data x0 ~ N(m, v) on the real line: x_t ~ N(sqrt(ab_t) m, ab_t v + 1 - ab_t), so E[eps | x_t] is linear in x_t and the
# probability-flow ODE keeps every start at its quantile: the exact end point of x_T at level ab is
#   m + sqrt(v) (x_T - sqrt(ab) m) / sqrt(ab v + 1 - ab).
def gaussian_eps(x, ab_t, m, v):
    return np.sqrt(1.0 - ab_t) * (x - np.sqrt(ab_t) * m) / (ab_t * v + 1.0 - ab_t)


def gaussian_exact_end(x_T, ab_T, m, v):
    return m + np.sqrt(v) * (x_T - np.sqrt(ab_T) * m) / np.sqrt(ab_T * v + 1.0 - ab_T)


def gaussian_chain(betas, order, x_T, m, v, rule="multistep", w_max=0.5):
    """The chain over ``order`` from ``x_T`` in float64 with unrounded coefficients, no wrap.  ``rule``: "ddim" (the
    strided update at eta = 0) or "multistep" (``w_max`` None: the paper's weight).  Returns the end point."""
    ab = alphas_cumprod(betas)
    coef = coefficients(betas, order, w_max)
    if rule == "ddim":
        coef[:, 4] = 0.0
    x = np.asarray(x_T, dtype=np.float64)
    prev = np.full_like(x, np.nan)
    for k, t in enumerate(order):
        x, prev, _ = update(coef[k], x, gaussian_eps(x, ab[t], m, v), prev)
    return x


def gaussian_max_error(betas, order, x_T, m, v, rule="multistep", w_max=0.5):
    end = gaussian_chain(betas, order, x_T, m, v, rule, w_max)
    return float(np.abs(end - gaussian_exact_end(np.asarray(x_T, dtype=np.float64), alphas_cumprod(betas)[order[0]], m, v)).max())
