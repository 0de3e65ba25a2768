"""Host-side tables and angle arithmetic of the continuous (cosine) diffusion.

Public names follow the reference's structure_model/utils.py (same call signatures and
results, checked bit-for-bit against reference-generated fixtures); the per-step device work
of the sampler does not go through here -- see sample.py, which runs the HIP
``e3d_ddpm_step_wrap`` kernel.
"""
import math

import numpy as np
import torch

TWO_PI = 2 * math.pi


class CosineTables:
    """All per-timestep scalars of the DDPM, built once on the host as fp32 tensors.

    reference: cosine_beta_schedule (utils.py:9-18) + compute_alphas (utils.py:42-59), which the
    reference re-derives on every reverse step (sample.py:74).
    """

    def __init__(self, timesteps: int, s: float = 8e-3):
        grid = torch.linspace(0, timesteps, timesteps + 1)
        f = torch.cos(((grid / timesteps) + s) / (1 + s) * torch.pi * 0.5) ** 2
        f = f / f[0]
        self.timesteps = timesteps
        self.betas = torch.clip(1 - (f[1:] / f[:-1]), 0.0001, 0.9999)
        self._derive()

    @classmethod
    def from_betas(cls, betas: torch.Tensor) -> "CosineTables":
        self = cls.__new__(cls)
        self.timesteps = betas.shape[0]
        self.betas = betas
        self._derive()
        return self

    def _derive(self):
        b = self.betas
        self.alphas = 1.0 - b
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        prev = torch.cat([torch.ones(1, dtype=b.dtype), self.alphas_cumprod[:-1]])
        self.posterior_variance = b * (1.0 - prev) / (1.0 - self.alphas_cumprod)
        self.sqrt_alphas_cumprod = torch.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = torch.sqrt(1.0 - self.alphas_cumprod)
        # reverse-step scalars (sample.py:75,97)
        self.sqrt_recip_alphas = 1.0 / torch.sqrt(self.alphas)
        self.sigma = torch.sqrt(self.posterior_variance)

    def as_dict(self):
        keys = ("betas", "alphas", "alphas_cumprod", "sqrt_alphas_cumprod",
                "sqrt_one_minus_alphas_cumprod", "posterior_variance")
        return {k: getattr(self, k) for k in keys}


class StridedTables:
    """Coefficients of the strided (generalised DDIM / respaced-ancestral) update over a subset of the timesteps
    (Song et al. 2021, eqs. 12 and 16): the schedule-consistent jump from ``t`` straight to its successor ``s < t``.

    ``order``: the visited timesteps, strictly descending (``reversed(range(0, T, step))``); the successor of
    ``order[k]`` is ``order[k + 1]``, the last entry's is "-1" (ab_s = 1: the step returns the x0 estimate).
    ``eta`` in [0, 1]: 0 is deterministic DDIM, 1 the ancestral posterior variance of the respaced chain.

    Derived in float64 from ``tab.betas`` with ab = cumprod(1 - betas), each coefficient rounded to fp32 once:

        sigma = eta sqrt((1 - ab_s) / (1 - ab_t)) sqrt(1 - ab_t / ab_s)
        s1m = sqrt(1 - ab_t)    rsa = 1 / sqrt(ab_t)    a_s = sqrt(ab_s)    c_dir = sqrt(max(0, 1 - ab_s - sigma^2))

    ``coef`` fp32 [T, 8]: row t = (s1m, rsa, a_s, c_dir, sigma, 0, 0, 0) -- the table ``e3d_strided_step_wrap`` reads by
    the device step index; rows of timesteps that are not visited are NaN, so a wrong index shows up as NaN.
    """

    def __init__(self, tab: CosineTables, order, eta: float = 0.0):
        T = int(tab.betas.shape[0])
        order = [int(t) for t in order]
        eta = float(eta)
        if not 0.0 <= eta <= 1.0:
            raise ValueError(f"StridedTables: eta must be in [0, 1], got {eta}")
        if not order:
            raise ValueError("StridedTables: the order of timesteps is empty")
        if any(t < 0 or t >= T for t in order):
            raise ValueError(f"StridedTables: timesteps must lie in [0, {T}), got {order}")
        if any(a <= b for a, b in zip(order, order[1:])):
            raise ValueError(f"StridedTables: the order must be strictly descending, got {order}")
        ab = torch.cumprod(1.0 - tab.betas.double(), dim=0)
        idx = torch.tensor(order, dtype=torch.long)
        ab_t = ab[idx]
        ab_s = torch.cat([ab[idx[1:]], torch.ones(1, dtype=torch.float64)])
        sigma = eta * torch.sqrt((1.0 - ab_s) / (1.0 - ab_t)) * torch.sqrt(1.0 - ab_t / ab_s)
        rows = torch.zeros((len(order), 8), dtype=torch.float64)
        rows[:, 0] = torch.sqrt(1.0 - ab_t)
        rows[:, 1] = 1.0 / torch.sqrt(ab_t)
        rows[:, 2] = torch.sqrt(ab_s)
        rows[:, 3] = torch.sqrt(torch.clamp(1.0 - ab_s - sigma ** 2, min=0.0))
        rows[:, 4] = sigma
        self.timesteps, self.order, self.eta = T, order, eta
        self.coef = torch.full((T, 8), float("nan"), dtype=torch.float32)
        self.coef[idx] = rows.float()

    def successor(self, t: int) -> int:
        """The timestep the update at ``t`` lands on; -1 after the last visited one."""
        k = self.order.index(int(t))
        return self.order[k + 1] if k + 1 < len(self.order) else -1


class MultistepTables:
    """Coefficients of the second-order multistep update over a subset of the timesteps: DPM-Solver++(2M) of Lu et al.
    2022 in its data-prediction form, with the extrapolation weight capped.  One decoder forward per step, like the
    strided update; it keeps the previous step's x0 estimate and draws nothing.

    ``order``: the visited timesteps, strictly descending, as for ``StridedTables``; same successors.

    With lambda(a) = ln(a / (1 - a)) / 2 (half the log-SNR) and h_k = lambda(ab_s) - lambda(ab_t) at order[k], the rule
    replaces the x0 estimate of the eta = 0 strided (DDIM) update by x0 + w_k (x0 - x0_prev):

        w_k = 0                                  at the first visited timestep (no history) and the last (h is infinite)
        w_k = min(h_k / (2 h_{k-1}), w_max)      otherwise

    ``w_max`` = 0.5 by default; None gives the paper's uncapped weight.  The cap is a deliberate difference from the
    paper: the visited timesteps are uniform in t and beta_0 is clipped, so the jump that lands on t = 0 spans a log-SNR
    step several times its predecessor's (w = 2.1 at T = 1000, step 100) and the uncapped rule can then be worse than
    DDIM; 0.5 is the weight of equal steps.  ``weights`` (float64 [len(order)]) holds the w_k, so a caller sees where the
    cap acted.

    Derived in float64 from ``tab.betas`` with ab = cumprod(1 - betas), each coefficient rounded to fp32 once.  In the
    DDIM update the x0 estimate carries the factor a_s - sqrt(ab_t) c_dir / s1m (the rest of it multiplies x), hence

        c_1 = (a_s - sqrt(ab_t) c_dir / s1m) w_k

    ``coef`` fp32 [T, 8]: row t = (s1m, rsa, a_s, c_dir, c_1, 0, 0, 0), the first four bit-identical to
    ``StridedTables(tab, order, 0.0).coef`` -- the table ``e3d_multistep_step_wrap`` reads by the device step index;
    rows of timesteps that are not visited are NaN.
    """

    def __init__(self, tab: CosineTables, order, w_max=0.5):
        T = int(tab.betas.shape[0])
        order = [int(t) for t in order]
        if w_max is not None and not float(w_max) >= 0.0:
            raise ValueError(f"MultistepTables: w_max must be None or at least 0, got {w_max}")
        if not order:
            raise ValueError("MultistepTables: the order of timesteps is empty")
        if any(t < 0 or t >= T for t in order):
            raise ValueError(f"MultistepTables: timesteps must lie in [0, {T}), got {order}")
        if any(a <= b for a, b in zip(order, order[1:])):
            raise ValueError(f"MultistepTables: the order must be strictly descending, got {order}")
        ab = torch.cumprod(1.0 - tab.betas.double(), dim=0)
        idx = torch.tensor(order, dtype=torch.long)
        ab_t = ab[idx]
        ab_s = torch.cat([ab[idx[1:]], torch.ones(1, dtype=torch.float64)])
        n = len(order)
        w = torch.zeros(n, dtype=torch.float64)
        if n > 2:
            lam = 0.5 * torch.log(ab_t / (1.0 - ab_t))
            h = lam[1:] - lam[:-1]                      # h[k] of order[k], k < n - 1
            w[1:n - 1] = h[1:] / (2.0 * h[:-1])
            if w_max is not None:
                w = torch.clamp(w, max=float(w_max))
        rows = torch.zeros((n, 8), dtype=torch.float64)
        rows[:, 0] = torch.sqrt(1.0 - ab_t)
        rows[:, 1] = 1.0 / torch.sqrt(ab_t)
        rows[:, 2] = torch.sqrt(ab_s)
        rows[:, 3] = torch.sqrt(torch.clamp(1.0 - ab_s, min=0.0))
        rows[:, 4] = (rows[:, 2] - torch.sqrt(ab_t) * rows[:, 3] / rows[:, 0]) * w
        self.timesteps, self.order, self.w_max = T, order, None if w_max is None else float(w_max)
        self.weights = w
        self.coef = torch.full((T, 8), float("nan"), dtype=torch.float32)
        self.coef[idx] = rows.float()

    def successor(self, t: int) -> int:
        """The timestep the update at ``t`` lands on; -1 after the last visited one."""
        k = self.order.index(int(t))
        return self.order[k + 1] if k + 1 < len(self.order) else -1


class KnownLevels:
    """Noise levels of the held positions of a partial redesign (replacement conditioning; sample.py, ``known=``): the
    level the state is on AFTER the step at each visited timestep, whatever the update rule and the stride are.

    ``order``: the visited timesteps, strictly descending, as for ``StridedTables``.  After the step at ``order[k]`` the
    state is a sample at level ``s = order[k + 1]``, so the held positions get a forward-noised copy of their known values
    at ``s``; after the step at the last visited timestep the state is the sample itself and they get the known values.

    Derived in float64 from ``tab.betas`` with ab = cumprod(1 - betas), each entry rounded to fp32 once:

    ``levels`` fp32 [T, 2]: row order[k] = (sqrt(ab_s), sqrt(1 - ab_s)); the last visited timestep's row is (1, 0); rows of
    timesteps that are not visited are NaN -- the table ``e3d_known_compose_wrap`` reads by the device step index.
    """

    def __init__(self, tab: CosineTables, order):
        T = int(tab.betas.shape[0])
        order = [int(t) for t in order]
        if not order:
            raise ValueError("KnownLevels: the order of timesteps is empty")
        if any(t < 0 or t >= T for t in order):
            raise ValueError(f"KnownLevels: timesteps must lie in [0, {T}), got {order}")
        if any(a <= b for a, b in zip(order, order[1:])):
            raise ValueError(f"KnownLevels: the order must be strictly descending, got {order}")
        ab = torch.cumprod(1.0 - tab.betas.double(), dim=0)
        idx = torch.tensor(order, dtype=torch.long)
        ab_s = ab[idx[1:]]
        rows = torch.empty((len(order), 2), dtype=torch.float64)
        rows[:-1, 0] = torch.sqrt(ab_s)
        rows[:-1, 1] = torch.sqrt(1.0 - ab_s)
        rows[-1, 0], rows[-1, 1] = 1.0, 0.0
        self.timesteps, self.order = T, order
        self.levels = torch.full((T, 2), float("nan"), dtype=torch.float32)
        self.levels[idx] = rows.float()


class ScoreTables:
    """Schedule scalars of the structure score (sample.py, ``score_structures``): what turns the model's noise error at
    timestep ``t`` into the per-element term of the bound.

    With the sampler's indexing (timestep t reads a state at level ab_t and lands on level t - 1) the sampler's mean and
    the forward posterior's mean, given the same x_t, differ by k_t (eps_hat - eps); both laws have the variance sigma_t^2
    = posterior_variance[t] when the noise has unit scale.  ``scale`` is the dataset's ``angular_var_scale``.

    Derived in float64 from ``tab.betas`` with ab = cumprod(1 - betas), each entry rounded to fp32 once:

        k_t = beta_t / (sqrt(1 - beta_t) sqrt(1 - ab_t))
        t > 0:  h_t = 1 / (2 sigma_t^2), sigma_t^2 = beta_t (1 - ab_{t-1}) / (1 - ab_t);  add_t = (scale^2 - 1) / 2 - ln(scale)
        t = 0:  h_0 = 1 / (2 beta_0);  add_0 = ln(2 pi beta_0) / 2      (a Gaussian decoder of variance beta_0: a density)

    ``coef`` fp32 [T, 4]: row t = (k_t, h_t, add_t, 0) -- the table ``e3d_angle_score_items`` reads by each item's step.
    ``prior_ab`` (float64): ab_{T-1}, the level of the prior term.
    """

    def __init__(self, tab: CosineTables, scale: float = 1.0):
        scale = float(scale)
        if not (0.0 < scale < float("inf")):
            raise ValueError(f"ScoreTables: scale must be positive and finite, got {scale}")
        betas = tab.betas.double()
        T = int(betas.shape[0])
        if T < 1:
            raise ValueError("ScoreTables: an empty schedule")
        ab = torch.cumprod(1.0 - betas, dim=0)
        prev = torch.cat([torch.ones(1, dtype=torch.float64), ab[:-1]])
        rows = torch.zeros((T, 4), dtype=torch.float64)
        rows[:, 0] = betas / (torch.sqrt(1.0 - betas) * torch.sqrt(1.0 - ab))
        var = betas * (1.0 - prev) / (1.0 - ab)
        var[0] = betas[0]
        rows[:, 1] = 1.0 / (2.0 * var)
        rows[:, 2] = (scale * scale - 1.0) / 2.0 - math.log(scale)
        rows[0, 2] = math.log(2.0 * math.pi * float(betas[0])) / 2.0
        if not bool(torch.isfinite(rows).all()):
            raise ValueError("ScoreTables: the schedule gives a non-finite coefficient (a beta of 0 or 1?)")
        self.timesteps, self.scale = T, scale
        self.coef64 = rows                       # before the one rounding, for checks against the closed forms
        self.coef = rows.float().contiguous()
        self.prior_ab = float(ab[-1])


def cosine_beta_schedule(timesteps: int, s: float = 8e-3) -> torch.Tensor:
    return CosineTables(timesteps, s).betas


def compute_alphas(betas: torch.Tensor):
    return CosineTables.from_betas(betas).as_dict()


def modulo_with_wrapped_range(vals, range_min: float = -np.pi, range_max: float = np.pi):
    """Map onto [range_min, range_max) by a floored modulo of the shifted value
    (reference utils.py:20-40; e.g. (3, -2, 2) -> -1)."""
    if not (range_min <= 0.0 and range_min < range_max):
        raise AssertionError("need range_min <= 0 < range_max")
    span = range_max - range_min
    return (vals - range_min) % span + range_min


def _wrapped_delta(prediction, truth):
    return modulo_with_wrapped_range(truth - prediction, -torch.pi, torch.pi)


def _radian_l1_elem(input, target):
    delta = (target % TWO_PI) - (input % TWO_PI)
    delta = (delta + torch.pi) % TWO_PI - torch.pi
    return delta.abs()


def radian_l1_loss(input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Mean absolute angular difference (reference utils.py:61-76); both arguments are first
    reduced mod 2*pi, exactly as the reference does."""
    return _radian_l1_elem(input, target).mean()


def radian_smooth_l1_loss(input: torch.Tensor, target: torch.Tensor, beta: float = 1.0,
                          circle_penalty: float = 0.0) -> torch.Tensor:
    """Huber-style loss on the wrapped difference (reference utils.py:78-109): quadratic inside
    ``beta``, linear outside; ``circle_penalty`` charges whole turns of ``input``."""
    return _radian_smooth_l1_elem(input, target, beta, circle_penalty).mean()


def _radian_smooth_l1_elem(input, target, beta=1.0, circle_penalty=0.0):
    if target.shape != input.shape:
        raise AssertionError(f"Mismatched shapes: {input.shape} != {target.shape}")
    if not beta > 0:
        raise AssertionError("beta must be positive")
    delta = _wrapped_delta(input, target)
    mag = delta.abs()
    loss = torch.where(mag < beta, 0.5 * (delta ** 2) / beta, mag - 0.5 * beta)
    if circle_penalty > 0:
        loss = loss + circle_penalty * torch.div(input.abs(), torch.pi, rounding_mode="trunc")
    return loss


def elementwise_form(fn):
    """The per-element form ``e`` of one of this module's loss functions (``fn(x, y) == e(x, y).mean()``), or None for a
    callable this module does not know: lets the training step take the mean over the un-padded positions as a masked
    sum -- no ``torch.where(mask)`` index lists, hence no device-to-host synchronisation inside the step."""
    import functools
    if fn is radian_l1_loss:
        return _radian_l1_elem
    if fn is radian_smooth_l1_loss:
        return _radian_smooth_l1_elem
    if isinstance(fn, functools.partial) and fn.func is radian_smooth_l1_loss and not fn.args:
        return functools.partial(_radian_smooth_l1_elem, **fn.keywords)
    return None


def tolerant_comparison_check(values, cmp, v):
    """``values`` all >= v (or <= v) up to 1e-5 (reference utils.py:111-130, unused there)."""
    if cmp not in (">=", "<="):
        raise ValueError(f"Illegal comparator: {cmp}")
    extreme = np.nanmin(values) if cmp == ">=" else np.nanmax(values)
    gap = extreme - v
    if np.isclose(gap, 0, atol=1e-5):
        return True
    return bool(gap > 0) if cmp == ">=" else bool(gap < 0)
