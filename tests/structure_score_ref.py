"""numpy float64 statement of the structure score (structure_model/sample.py::score_structures; DESIGN.md, "Scoring
structures"), written from the formulas of the definition and built on tests/sampler_ref.py, tests/keyed_ref.py and
tests/strided_ref.py, not from the kernels: the schedule scalars k_t, h_t, add_t, the per-element error and term, the
prior, the level sets with their weight, the keyed forward noising at per-item levels, and -- a function of fp32 values
alone, which the kernel must match exactly -- the fixed-shape sums of an item.  Below them the error bounds of
tests/test_structure_score_gpu.py and the inputs of its cases.  Test infrastructure only.

Bounds (u = 2^-24).  The float64 reference is fed the same fp32 inputs eps_hat, eps and the same fp32 table row (k, h,
add), so only the kernel's own operations count.  PI_ERR = |fp32(pi) - pi| = 8.75e-8.  With s = eps_hat - eps, d = k s:

  the subtraction      s is rounded once: u |s|.
  its amplification    d = k * fl(s), rounded: k carries the subtraction's error, u |k s| = u |d|, and the product adds
                       u |d|:  2 u |d|.
  the wrap             torch's modulo_with_wrapped_range in fp32: sft = d + fp32(pi), rounded: u (|d| + pi); fmodf by
                       2 fp32(pi): exact; + 2 fp32(pi) where the remainder is negative: u 2 pi; - fp32(pi): u pi.  The
                       shift cancels, but every whole turn taken off is a turn of 2 fp32(pi) and not of 2 pi: with m <=
                       |d| / (2 pi) + 3 / 2 turns, 2 m PI_ERR = (|d| / pi + 3) PI_ERR.  On the circle therefore
                           e_delta = 3 u |d| + 4 u pi + (|d| / pi + 3) PI_ERR.
                       Next to a cut the fp32 delta and the reference may sit on opposite sides, 2 pi apart as numbers
                       and e_delta apart on the circle.
  the square           delta^2 is continuous across the cut: for two points c apart on the circle, |a^2 - b^2| =
                       ||a| - |b|| (|a| + |b|) <= c (2 |b| + c), same side or not.  The product is rounded: u delta^2.
  h * sq, + add        one rounding each: u h delta^2 and u |term|.

  |term - ref| <= h e_delta (2 |delta| + e_delta) + 2 u h delta^2 + u |term|,    times 1 + 2^-10 for second order,

with delta and term the reference's.  Where eps_hat == eps the kernel's s, d and delta are exact zeros and the term is
add, bit for bit.  err = wrap(eps - eps_hat) takes the same wrap without the amplification:
  |err - ref| on the circle <= 2 u |s| + 4 u pi + (|s| / pi + 3) PI_ERR.
Sums: at most L F - 1 additions, each at most u of a partial sum of absolute values: (L F) u sum |v| against the float64
sum of the same fp32 values; the fixed-shape fp32 restatement below is matched bit for bit."""
import numpy as np

import keyed_ref as K
import sampler_ref as R
from score_ref import item_sum_fp32, level_set  # noqa: F401  (the level sets are the sequence score's)

U = R.U
F32 = np.float32
SCORE_STREAM_STRUCT = 12
PI_ERR = abs(float(R.PI_F) - np.pi)


# ----------------------------------------------------------------------------------------------------- fp64 statements
def schedule(betas):
    """float64 (alpha, ab, ab_prev, sigma2) of a schedule: sigma2[t] = beta_t (1 - ab_{t-1}) / (1 - ab_t), sigma2[0] = 0."""
    b = np.asarray(betas, dtype=np.float64)
    alpha = 1.0 - b
    ab = np.cumprod(alpha)
    prev = np.concatenate([[1.0], ab[:-1]])
    return alpha, ab, prev, b * (1.0 - prev) / (1.0 - ab)


def coefficients(betas, scale=1.0):
    """float64 [T, 3] = (k_t, h_t, add_t) from the definition."""
    b = np.asarray(betas, dtype=np.float64)
    alpha, ab, _, sigma2 = schedule(b)
    k = b / (np.sqrt(alpha) * np.sqrt(1.0 - ab))
    h = np.empty_like(b)
    h[1:] = 1.0 / (2.0 * sigma2[1:])
    h[0] = 1.0 / (2.0 * b[0])
    add = np.full_like(b, (scale * scale - 1.0) / 2.0 - np.log(scale))
    add[0] = np.log(2.0 * np.pi * b[0]) / 2.0
    return np.stack([k, h, add], axis=1)


def posterior_coefficients(betas):
    """The textbook q(x_{t-1} | x_t, x_0) mean coefficients (Ho et al. 2020, eq. 7): mean = c1 x0 + c2 x_t."""
    b = np.asarray(betas, dtype=np.float64)
    alpha, ab, prev, _ = schedule(b)
    return np.sqrt(prev) * b / (1.0 - ab), np.sqrt(alpha) * (1.0 - prev) / (1.0 - ab)


def elem(row, eps_hat, eps):
    """(err, delta, term) float64 of elements under one table row (k, h, add, ..): err = wrap(eps - eps_hat), delta =
    wrap(k (eps_hat - eps)), term = h delta^2 + add."""
    k, h, add = (float(v) for v in row[:3])
    eh, e = np.asarray(eps_hat, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    delta = R.wrap_pi(k * (eh - e))
    return R.wrap_pi(e - eh), delta, h * delta * delta + add


def term_bound(row, eps_hat, eps):
    """The absolute bound on the fp32 term (this module's docstring)."""
    k, h, _ = (float(v) for v in row[:3])
    d = np.abs(k * (np.asarray(eps_hat, dtype=np.float64) - np.asarray(eps, dtype=np.float64)))
    _, delta, term = elem(row, eps_hat, eps)
    e_delta = 3 * U * d + 4 * U * np.pi + (d / np.pi + 3) * PI_ERR
    return (h * e_delta * (2 * np.abs(delta) + e_delta) + 2 * U * h * delta * delta + U * np.abs(term)) * (1 + 2.0 ** -10)


def err_bound(eps_hat, eps):
    s = np.abs(np.asarray(eps_hat, dtype=np.float64) - np.asarray(eps, dtype=np.float64))
    return 2 * U * s + 4 * U * np.pi + (s / np.pi + 3) * PI_ERR


def prior(x0, ab, scale=1.0):
    """Per element: ((1 - ab) + ab x0^2 / scale^2 - 1 - ln(1 - ab)) / 2."""
    x0 = np.asarray(x0, dtype=np.float64)
    return ((1.0 - ab) + ab * x0 * x0 / scale ** 2 - 1.0 - np.log(1.0 - ab)) / 2.0


def combine(prior_sum, terms, w):
    """bound = prior + term_0 + w * sum of the other levels; terms [S, ...]."""
    terms = np.asarray(terms, dtype=np.float64)
    return prior_sum + terms[0] + (w * terms[1:].sum(axis=0) if len(terms) > 1 else 0.0)


def forward_levels(x0, keys, seed, steps, sqrt_ab, sqrt_1mab, scale=1.0):
    """(noise, x_t) float64 [N, L, F] of the keyed forward noising: item n is item n % B of x0 [B, L, F] / keys [B * L, 2]
    at step steps[n]; noise = wrap(scale z), z the stream-12 normals; x_t = wrap(a x0 + s noise).  Rows of no item: 0."""
    x0 = np.asarray(x0, dtype=np.float64)
    B, L, F = x0.shape
    keys = np.asarray(keys).reshape(B, L, 2)
    noise, xt = np.zeros((len(steps), L, F)), np.zeros((len(steps), L, F))
    for n, t in enumerate(steps):
        b = n % B
        z = K.normals(keys[b], seed, SCORE_STREAM_STRUCT, int(t), F)
        live = keys[b, :, 1] >= 0
        noise[n] = np.where(live[:, None], R.wrap_pi(scale * z), 0.0)
        xt[n] = np.where(live[:, None], R.q_sample(float(sqrt_ab[t]), float(sqrt_1mab[t]), x0[b], noise[n])[0], 0.0)
    return noise, xt


# ----------------------------------------------------------------------------------------------------- exact fp32 rules
def _butterfly(acc):
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ off]
        assert acc.dtype == F32
    return acc[0]


def item_sums_fp32(values, mask):
    """(res fp32 [L], feat fp32 [F], total fp32, count) of one item's values [L, F] in the kernel's fixed shape: a residue
    is the sum of its masked elements in feature order, a masked-out element adding +0; lane j of 64 adds residues j,
    j + 64, .. in order; the xor butterfly 32, 16, .. 1 gives the total.  A feature's sum takes the same lane walk over
    its own elements.  Sequential fp32 additions of stored values: exact."""
    v = np.asarray(values)
    assert v.dtype == F32 and v.ndim == 2
    L, nF = v.shape
    m = np.asarray(mask).astype(bool)
    sel = np.where(m, v, F32(0)).astype(F32)
    res = np.zeros(L, dtype=F32)
    for f in range(nF):
        res = res + sel[:, f]
    acc = np.zeros(64, dtype=F32)
    facc = np.zeros((64, nF), dtype=F32)
    for l in range(L):
        acc[l % 64] = acc[l % 64] + res[l]
        facc[l % 64] = facc[l % 64] + sel[l]
    assert res.dtype == F32 and facc.dtype == F32
    feat = np.array([_butterfly(facc[:, f]) for f in range(nF)], dtype=F32)
    return res, feat, _butterfly(acc), int(m.sum())


# ----------------------------------------------------------------------------------------------------- inputs of the tests
def score_inputs(N, L, F, rows, steps, seed=71):
    """fp32 (eps_hat, eps) [N, L, F]: eps wrapped normals; eps_hat - eps takes the values of wrap_grid() divided by the
    item's k, so that k (eps_hat - eps) sits on and beside every cut of the wrap as far as the fp32 division and
    subtraction allow (the grid's first 273 values are the neighbours of k pi, |k| <= 7); an item's last element and,
    past those 273, every fifth are exact zeros (eps_hat == eps) and every seventh a normal draw.  ``rows``: the fp32
    table, ``steps`` [N] the items' steps (an out-of-range step takes k = 1)."""
    rng = np.random.default_rng(seed + 1000 * N + 10 * L + F)
    eps = R.wrap_pi(rng.standard_normal((N, L, F))).astype(F32)
    grid = R.wrap_grid()
    eh = np.empty_like(eps)
    p = np.arange(L * F)
    zero = (p == L * F - 1) | ((p >= 273) & (p % 5 == 4))
    drawn = (p >= 273) & (p % 7 == 3) & ~zero
    for n in range(N):
        k = F32(rows[steps[n], 0]) if 0 <= steps[n] < len(rows) else F32(1.0)
        diff = np.resize(np.roll(grid[:4096], -37 * n), L * F).astype(F32) / k
        diff = np.where(drawn, rng.standard_normal(L * F).astype(F32), diff).astype(F32)
        flat = eps[n].reshape(-1) + diff
        eh[n] = np.where(zero, eps[n].reshape(-1), flat).reshape(L, F)
    return eh.astype(F32), eps


def score_masks(B, L, F, seed=72):
    """The element masks of the GPU test, uint8 [B, L, F] each: all, none, one element, random."""
    rng = np.random.default_rng(seed + 100 * B + 10 * L + F)
    one = np.zeros((B, L, F), dtype=np.uint8)
    one[:, L // 2, F - 1] = 1
    rand = (rng.random((B, L, F)) < 0.6).astype(np.uint8)
    rand[:, 0, 0] = 1
    return {"all": np.ones((B, L, F), dtype=np.uint8), "none": np.zeros((B, L, F), dtype=np.uint8), "one": one, "random": rand}
