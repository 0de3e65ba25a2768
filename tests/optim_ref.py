"""The fp64 statement of the gradient-norm clip + AdamW update of csrc/optim.hip, its error bound, and the inputs and case
table the CPU and GPU tests share.  Test infrastructure only: the product does not import it.

The statement.  ``norm = sqrt(sum g^2)`` over all gradients in float64, ``coef = min(max_norm / (norm + 1e-6), 1)``, NaN
propagating (``clip``).  One update of one element (``update``) starts from the run's OWN fp32 p, m, v before the step --
teacher-forced, so nothing accumulates over steps -- and is fed the fp32 gradient, the fp32 hyper-parameters as
``ClipAdamW._hyper`` produces them (``hyper32``), the step count t and the fp32 clip coefficient the device wrote, all taken
as exact; everything below is float64, in the order of ``adamw_one``:

    g' = g coef                      p1 = p - lr wd p
    m' = m + (g' - m) (1 - b1)       v' = b2 v + (1 - b2) g'^2
    bc1 = 1 - b1^t                   bc2 = sqrt(1 - b2^t)
    ss = lr / bc1                    den = sqrt(v') / bc2 + eps
    q  = ss m' / den                 p' = p1 - q

The bound, u = 2^-24.  Every fp32 rounding of a correct evaluation is counted once, to first order, as u times the
magnitude it acts on; the sum is multiplied by SECOND = 1.01 for the second-order terms (the largest relative first-order
term is 12 u = 7e-7, its products are below 1e-12) and for the float64 ``pow`` / ``sqrt`` of the bias corrections (1e-16
against 1 - b^t >= 1e-3).  A contracted multiply-add has one rounding where the count has two, so the count holds either way.
Where the kernel and torch's single-tensor AdamW write the same quantity in two ways, the count takes the larger of the
two, so that both are correct evaluations under it (tests/test_optim_ref_cpu.py holds torch's fp32 CPU AdamW to it).

  g'   1 rounding: u |g'|.
  m'   the difference g' - m carries g' 's error and its own rounding, fl(1 - b1) one (it is exact for b1 >= 0.5; counted
       anyway), the product one, the sum one:
           E_m = u ((1 - b1) |g'| + 3 (1 - b1) |g' - m| + |m'|).
       Nothing here is relative to |m'| but the last rounding: m' may cancel.
  v'   b2 v: one rounding.  (1 - b2) g' g': g' 's own error twice, fl(1 - b2), two products: 5.  The sum: one.
           E_v = u (b2 v + 5 (1 - b2) g'^2 + v').
       v >= 0, so every term is positive and E_v <= 6 u v': v' has a RELATIVE error of at most 6 u, whatever its size.
  p1   the kernel: fl(lr wd) and its product with p, 2 u |lr wd p|, and the subtraction, u |p1|.  torch: the scalar
       1 - lr wd rounded to fp32 and its product with p, 2 u |p1|.  Both are within
           E_p1 = 2 u (|lr wd p| + |p1|).
  ss   fl(bc1) and the division: 2 u relative.
  den  sqrt(v'): half of 6 u, and sqrtf's rounding: 4.  Division by bc2: fl(bc2) and the division (the kernel), or
       fl(bc2), its fp32 reciprocal and a product (torch's division by a host scalar): 3.  So sqrt(v') / bc2 is within 7 u
       relative, and with the rounding of the sum  E_den = u (7 sqrt(v') / bc2 + den) <= 8 u den  (eps >= 0): 8 u relative.
  q    ss m' / den: product and division, 2.  With ss (2) and den (8): 12 u |q|, and m' 's ABSOLUTE error through ss / den:
           E_q = 12 u |q| + (ss / den) E_m.
  p'   E_p = E_p1 + E_q + u |p'|
           = u (2 |lr wd p| + 2 |p1| + 12 |q| + |p'|) + (ss / den) E_m.

No element is excluded and every bound is a continuous function of the inputs (absolute values, sums, products and a
quotient by den >= eps > 0).  sqrtf and the fp32 division are the correctly rounded ones (the library is built without
fast-math).  The inputs of the case table keep every intermediate far above the fp32 subnormals.

EMA forms: the shadow is held to ``ema_ref.Statement`` with n = 1 (4 u M), fed the device's own new parameter and
``ema_ref.decay_fp32`` of the update's number.

The norm.  ``norm_tolerance_note`` is the count behind the 2e-6 the tests assert.
"""
import numpy as np
import torch

U = 2.0 ** -24
SECOND = 1.01
CHUNK = 8192                      # e3d_optim_chunk_elems(); the GPU test asserts it
NORM_RTOL = 2e-6                  # the project's figure for the device norm, here against float64
COEF_RTOL = 3 * U                 # fl(norm + 1e-6f), the fp32 constant 1e-6f itself, the division

norm_tolerance_note = """A chunk's 8192 squares: each of 256 threads adds at most 32 of them with fmaf, one rounding per
term, into two accumulators (vector path: 16 each) or one (scalar path: 32); s0 + s1 one more; the wave butterfly six; the
four wave sums three.  All terms are >= 0, so these are relative: at most (32 + 1 + 6 + 3) u = 42 u on a partial.  The
partials are summed in double (nothing at this scale), the square root halves the error, the rounding of the norm to fp32
adds one: 22 u = 1.3e-6 < 2e-6 = 33.5 u."""


def f32(x):
    """The fp32 value of a Python number, as a Python float."""
    return float(np.float32(x))


def hyper32(lr, beta1, beta2, eps, weight_decay):
    """(lr, beta1, beta2, eps, weight_decay) as fp32 values: what ClipAdamW._hyper hands the kernels."""
    return tuple(f32(x) for x in (lr, beta1, beta2, eps, weight_decay))


def _d(x):
    return x.detach().double().cpu() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------- the statement
def clip(grads, max_norm):
    """(norm, coef) in float64 as Python floats; NaN / inf propagate as in clip_grad_norm_(error_if_nonfinite=False)."""
    total = 0.0
    for g in grads:
        g = _d(g)
        total += float((g * g).sum())
    norm = float(np.sqrt(np.float64(total)))
    with np.errstate(all="ignore"):
        r = float(np.float64(max_norm) / (np.float64(norm) + 1e-6))
    coef = r if (r < 1.0 or r != r) else 1.0
    return norm, coef


def coef_from_norm(norm32, max_norm):
    """The coefficient in float64 from the device's OWN fp32 norm."""
    with np.errstate(all="ignore"):
        r = float(np.float64(f32(max_norm)) / (np.float64(norm32) + 1e-6))
    return r if (r < 1.0 or r != r) else 1.0


def update(p, g, m, v, hyper, t, coef=1.0):
    """One teacher-forced update in float64.  ``hyper``: fp32-valued (lr, b1, b2, eps, wd); ``coef``: the fp32 clip
    coefficient as a Python float (1.0: no clip).  Returns dict(p, m, v: the new values; Ep, Em, Ev: their bounds)."""
    lr, b1, b2, eps, wd = (float(x) for x in hyper)
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    g1 = g * float(coef)
    decay = lr * wd * p
    p1 = p - decay
    c1, c2 = 1.0 - b1, 1.0 - b2
    m1 = m + (g1 - m) * c1
    v1 = b2 * v + c2 * g1 * g1
    bc1 = 1.0 - b1 ** float(t)
    bc2 = float(np.sqrt(1.0 - b2 ** float(t)))
    ss = lr / bc1
    root = v1.sqrt() / bc2
    den = root + eps
    q = ss * m1 / den
    p2 = p1 - q
    Em = U * (c1 * g1.abs() + 3.0 * c1 * (g1 - m).abs() + m1.abs())
    Ev = U * (b2 * v + 5.0 * c2 * g1 * g1 + v1)
    Ep = U * (2.0 * decay.abs() + 2.0 * p1.abs() + 12.0 * q.abs() + p2.abs()) + (ss / den) * Em
    return {"p": p2, "m": m1, "v": v1, "Ep": SECOND * Ep, "Em": SECOND * Em, "Ev": SECOND * Ev}


def fraction(got, want, bound):
    """The worst |got - want| / bound over all elements: 0 where both are 0, inf where only the bound is (or where exactly
    one of got / want is not finite, or they are different non-finite values).  <= 1 is the requirement.  Elements where the
    statement is NaN must be NaN in ``got`` (and the reverse); they count as 0."""
    got, want, bound = _d(got).reshape(-1), _d(want).reshape(-1), _d(bound).reshape(-1)
    if got.numel() == 0:
        return 0.0
    both_nan = got.isnan() & want.isnan()
    err = (got - want).abs()
    frac = torch.where(err == 0, torch.zeros_like(err), err / bound)
    frac = torch.where(both_nan, torch.zeros_like(frac), frac)
    frac = torch.where(frac.isnan(), torch.full_like(frac, float("inf")), frac)
    return float(frac.max())


def fractions(got_p, got_m, got_v, ref):
    """(p, m, v) fractions of one update against ``update``'s result."""
    return (fraction(got_p, ref["p"], ref["Ep"]), fraction(got_m, ref["m"], ref["Em"]), fraction(got_v, ref["v"], ref["Ev"]))


# ---------------------------------------------------------------------------------------------------- shared inputs
# numel of every tensor of the zoo (the last one is the 64 x 768 matrix) and of the misaligned views
ZOO = (1, 3, 4, 5, 255 * 4 + 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, 64 * 768)
VIEW_NUMEL = CHUNK + 6            # two chunks: the second one starts at the same residue of the address
# which of the roles (p, g, m, v, e: the shadow) sit at data_ptr % 16 == 4, everything else 16-byte aligned.  With only
# the gradient misaligned the norm takes its scalar path and so does the update; with the parameter (first and last view)
# the norm runs vectorised and the update scalar.
VIEWS = (("p",), ("g",), ("m",), ("e",), ("p", "m", "v", "e"))


def tensors():
    """[(numel, roles at a misaligned address)] of the zoo followed by the misaligned views."""
    return [(n, ()) for n in ZOO] + [(VIEW_NUMEL, mis) for mis in VIEWS]


def gen_inputs(numels, seed, gscale, state):
    """fp32 numpy inputs of one case for tensors of the given sizes: lists p, g, m, v, e.  ``state``: "zero" (first step:
    m = v = 0) or a scale s (m ~ 0.3 s N(0, 1), v ~ s^2 U(0.2, 1.2): moments of gradients of size s)."""
    rng = np.random.default_rng(seed)
    out = {k: [] for k in "pgmve"}
    for n in numels:
        p = rng.standard_normal(n).astype(np.float32)
        out["p"].append(p)
        out["g"].append((gscale * rng.standard_normal(n)).astype(np.float32))
        if state == "zero":
            out["m"].append(np.zeros(n, np.float32))
            out["v"].append(np.zeros(n, np.float32))
        else:
            s = float(state)
            out["m"].append((0.3 * s * rng.standard_normal(n)).astype(np.float32))
            out["v"].append((s * s * rng.uniform(0.2, 1.2, n)).astype(np.float32))
        out["e"].append((p + 0.5 * rng.standard_normal(n)).astype(np.float32))
    return out


# One row per case.  clip: max_norm of the norm launch whose coefficient the update reads, None: a null clip pointer.
# state: see gen_inputs.  ema: (decay, warmup, EMA updates made before this one).  Every step count, beta1, beta2, eps,
# weight decay, clip and state value of the issue's table appears at least once, and every entry point runs every row.
CASES = (
    dict(name="first-step-clipped", t=1, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, gscale=50.0, clip=1.0, state="zero",
         ema=(0.9999, True, 0)),
    dict(name="second-step-noclip", t=2, lr=3e-3, b1=0.85, b2=0.95, eps=1e-3, wd=0.1, gscale=1e-3, clip=None, state=1e-3,
         ema=(0.9, False, 1)),
    dict(name="t1000-clip-inactive", t=1000, lr=1e-3, b1=0.95, b2=0.999, eps=1e-8, wd=0.1, gscale=1e-3, clip=1.0, state=1e-3,
         ema=(0.9999, True, 999)),
    dict(name="t100000-clipped", t=100000, lr=1e-2, b1=0.9, b2=0.95, eps=1e-3, wd=0.0, gscale=50.0, clip=1.0, state=0.15,
         ema=(0.9999, False, 99999)),
    dict(name="first-step-noclip", t=1, lr=3e-3, b1=0.85, b2=0.999, eps=1e-3, wd=0.1, gscale=1.0, clip=None, state="zero",
         ema=(0.0, False, 0)),
    dict(name="t1000-noclip", t=1000, lr=1e-2, b1=0.9, b2=0.95, eps=1e-8, wd=0.0, gscale=1.0, clip=None, state=1.0,
         ema=(0.5, True, 3)),
    dict(name="second-step-clipped", t=2, lr=1e-3, b1=0.95, b2=0.999, eps=1e-8, wd=0.1, gscale=50.0, clip=1.0, state=0.15,
         ema=(0.9, True, 1)),
    dict(name="t100000-noclip", t=100000, lr=3e-3, b1=0.85, b2=0.999, eps=1e-8, wd=0.1, gscale=1e-3, clip=None, state=1e-3,
         ema=(0.25, False, 7)),
)


def case_hyper(case):
    return hyper32(case["lr"], case["b1"], case["b2"], case["eps"], case["wd"])


def case_inputs(case, numels=None):
    """The case's fp32 inputs over ``tensors()`` (or the given sizes); the seed is the row's position in CASES."""
    numels = [n for n, _ in tensors()] if numels is None else numels
    seed = 1000 + [c["name"] for c in CASES].index(case["name"])
    return gen_inputs(numels, seed, case["gscale"], case["state"])
