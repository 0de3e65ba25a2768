"""numpy float64 statement of the strided (generalised DDIM / respaced-ancestral) update, Song et al. 2021 eqs. 12 and
16, written from the formulas and not from the kernel: the coefficient rows of a descending order of timesteps, and the
per-element update.  Test infrastructure only."""
import numpy as np

TWO_PI = 2.0 * np.pi


def wrap_pi(v):
    """[-pi, pi) by the floored modulo of the shifted value."""
    return np.mod(np.asarray(v, dtype=np.float64) + np.pi, TWO_PI) - np.pi


def circ(a, b):
    """Circular distance |a - b| on the 2 pi circle."""
    return np.abs(wrap_pi(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)))


def alphas_cumprod(betas):
    return np.cumprod(1.0 - np.asarray(betas, dtype=np.float64))


def coefficients(betas, order, eta):
    """float64 [len(order), 5] = (s1m, rsa, a_s, c_dir, sigma) per visited t; the successor of order[k] is order[k + 1],
    the last entry's is "-1": ab_s = 1."""
    ab = alphas_cumprod(betas)
    order = np.asarray(order, dtype=np.int64)
    ab_t = ab[order]
    ab_s = np.concatenate([ab[order[1:]], [1.0]])
    sigma = eta * np.sqrt((1.0 - ab_s) / (1.0 - ab_t)) * np.sqrt(1.0 - ab_t / ab_s)
    s1m = np.sqrt(1.0 - ab_t)
    rsa = 1.0 / np.sqrt(ab_t)
    a_s = np.sqrt(ab_s)
    c_dir = np.sqrt(np.maximum(0.0, 1.0 - ab_s - sigma ** 2))
    return np.stack([s1m, rsa, a_s, c_dir, sigma], axis=1)


def table(betas, order, eta):
    """fp32 [T, 8]: row t = (s1m, rsa, a_s, c_dir, sigma, 0, 0, 0), each rounded once; NaN rows where t is not visited."""
    T = len(betas)
    out = np.full((T, 8), np.nan, dtype=np.float32)
    rows = np.zeros((len(order), 8), dtype=np.float64)
    rows[:, :5] = coefficients(betas, order, eta)
    out[np.asarray(order, dtype=np.int64)] = rows.astype(np.float32)
    return out


def update(row, x, e, z=None, wrap=False, wrap_x0=False):
    """The update in float64 from one table row (s1m, rsa, a_s, c_dir, sigma, ...).  Returns (out, parts): ``parts`` holds
    x0 before and after its wrap, the mean, and the magnitudes the fp32 error bound is made of."""
    s1m, rsa, a_s, c_dir, sigma = (float(v) for v in row[:5])
    x = np.asarray(x, dtype=np.float64)
    e = np.asarray(e, dtype=np.float64)
    x0_raw = (x - s1m * e) * rsa
    x0 = wrap_pi(x0_raw) if wrap_x0 else x0_raw
    mean = a_s * x0 + c_dir * e
    noisy = sigma != 0.0 and z is not None
    out = mean + sigma * np.asarray(z, dtype=np.float64) if noisy else mean
    x0_mag = rsa * (np.abs(x) + np.abs(s1m * e))                  # what the roundings of the x0 estimate scale with
    parts = {"x0_raw": x0_raw, "x0": x0, "mean": mean, "x0_mag": x0_mag,
             # G of the bound: a_s * (x0 term) + |c_dir e| + |sigma z|; with wrap_x0 the wrapped x0 stands in G
             "G": a_s * (np.abs(x0) if wrap_x0 else x0_mag) + np.abs(c_dir * e)
                  + (np.abs(sigma * np.asarray(z, dtype=np.float64)) if noisy else 0.0)}
    return (wrap_pi(out) if wrap else out), parts
