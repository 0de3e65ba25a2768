"""The fp64 statement of the weight EMA (training.ema_decay_at / training.WeightEMA) and its error bound.

The statement is the recurrence  e <- e + (p - e) * w  carried in float64, fed the run's OWN fp32 parameters after each step
and the fp32 d_n of that update, with w = 1 - d_n formed in double.  Feeding it the run's parameters keeps the optimizer's
error (and the atomics of the weight-gradient launches) out of the picture: what is checked is the average alone.

The bound: after n updates an element lies within  n * 4u * M  of the statement, u = 2^-24, M the largest |p| and |e| the
element has had so far.  Per update there is one rounding each of the difference, the product and the sum, plus that of w
itself when d < 0.5 (1.0f - d is exact for d >= 0.5); earlier errors shrink by d.
"""
import torch

U = 2.0 ** -24


def decay_fp32(n, decay, warmup=True):
    """d_n as the law states it, written out here independently of the package: double, rounded once to fp32."""
    d = min(float(decay), (1.0 + n) / (10.0 + n)) if warmup else float(decay)
    return float(torch.tensor(d, dtype=torch.float64).to(torch.float32))


class Statement:
    """One tensor's shadow in float64.  ``start``: the fp32 parameter the shadow was cloned from."""

    def __init__(self, start):
        self.e = start.detach().double().cpu().clone()
        self.M = self.e.abs()
        self.n = 0

    def update(self, p, d32):
        """``p``: the run's fp32 parameter after the step; ``d32``: the fp32 d_n of this update (a Python float)."""
        p = p.detach().double().cpu()
        self.e = self.e + (p - self.e) * (1.0 - float(d32))
        self.M = torch.maximum(self.M, torch.maximum(p.abs(), self.e.abs()))
        self.n += 1

    def fraction(self, shadow):
        """The worst |shadow - statement| over its bound n * 4u * M (0.0 where the bound is 0 and so is the error; inf where
        the bound is 0 and the error is not).  <= 1 is the requirement."""
        err = (shadow.detach().double().cpu().reshape(self.e.shape) - self.e).abs()
        bound = self.n * 4 * U * self.M
        frac = torch.where(err == 0, torch.zeros_like(err), err / bound)
        return float(frac.max()) if frac.numel() else 0.0
