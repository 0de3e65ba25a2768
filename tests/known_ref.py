"""numpy float64 statement of the partial redesign's replacement conditioning (Song et al. 2021, section I.2; Lugmayr et
al. 2022), written from the formulas and not from the kernel: the noise level the state is on after each visited timestep
of a descending order, and the per-element overwrite of the held positions.  Test infrastructure only."""
import numpy as np

from strided_ref import alphas_cumprod, circ, wrap_pi  # noqa: F401  (circ: the tests compare by circular distance)


def levels(betas, order):
    """float64 [len(order), 2] = (sqrt(ab_s), sqrt(1 - ab_s)) per visited t, s the successor of t in ``order``; after the
    last visited timestep the state is the sample itself: (1, 0)."""
    ab = alphas_cumprod(betas)
    order = np.asarray(order, dtype=np.int64)
    ab_s = np.concatenate([ab[order[1:]], [1.0]])
    return np.stack([np.sqrt(ab_s), np.sqrt(1.0 - ab_s)], axis=1)


def table(betas, order):
    """fp32 [T, 2]: row order[k] = levels(...)[k], each entry rounded once; NaN rows where t is not visited."""
    out = np.full((len(betas), 2), np.nan, dtype=np.float32)
    out[np.asarray(order, dtype=np.int64)] = levels(betas, order).astype(np.float32)
    return out


def compose(row, x, x0, mask, z, scale=1.0):
    """The overwrite in float64 from one table row (a, s1m): where ``mask`` is set, x becomes x0 at the clean level
    (s1m == 0), wrap(a x0 + s1m wrap(scale z)) otherwise, NaN for a NaN row; elsewhere x stays.  Returns (out, parts):
    ``parts`` holds what the fp32 error bound is made of -- sz = scale z, n = wrap(sz), v = a x0 + s1m n before the outer
    wrap, G = |a x0| + |s1m n|."""
    a, s1m = float(row[0]), float(row[1])
    x = np.asarray(x, dtype=np.float64)
    x0 = np.asarray(x0, dtype=np.float64)
    held = np.asarray(mask) != 0
    if np.isnan(a) or np.isnan(s1m):
        return np.where(held, np.nan, x), None
    if s1m == 0.0:
        return np.where(held, x0, x), None
    sz = scale * np.asarray(z, dtype=np.float64)
    n = wrap_pi(sz)
    v = a * x0 + s1m * n
    parts = {"sz": sz, "n": n, "v": v, "G": np.abs(a * x0) + np.abs(s1m * n)}
    return np.where(held, wrap_pi(v), x), parts


U = 2.0 ** -24


def excluded(sz, extra=0.0):
    """Elements whose float64 sz = scale * z lies within 8 u |sz| (+ ``extra``) of an odd multiple of pi: there a
    legitimate fp32 rounding moves wrap(sz) by 2 pi."""
    sz = np.asarray(sz, dtype=np.float64)
    cut = np.pi + 2 * np.pi * np.round((sz - np.pi) / (2 * np.pi))
    return np.abs(sz - cut) < 8 * U * np.abs(sz) + extra


def kernel_inputs(n, seed=31):
    """The fixed inputs of the kernel test: state x, known x0, N(0,1) draws z (fp32) and a mask of density about 0.5."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-np.pi, np.pi, n).astype(np.float32)
    x0 = rng.uniform(-np.pi, np.pi, n).astype(np.float32)
    x0[x0 >= np.float32(np.pi)] = -np.float32(np.pi)
    z = rng.standard_normal(n).astype(np.float32)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    mask[:8] = (1, 0, 1, 1, 0, 0, 0, 0)         # the small sizes hold and free something; a group of four that is free
    return x, x0, z, mask
