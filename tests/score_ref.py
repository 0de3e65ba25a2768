"""numpy float64 statement of the sequence score (sequence_model/sample.py::score_sequences; DESIGN.md, "Scoring
sequences"), built on tests/sampler_ref.py: the posterior p_theta, the posterior q_post given the true residue, their KL
under the conventions 0 log 0 = 0 and q > 0, p == 0 -> +inf, the denoising cross-entropy, the prior, the level sets with
their weight, the keyed forward noising at per-item levels, and -- a function of fp32 values alone, which the kernel must
match exactly -- the fixed-shape item sum.  Below them, the error bounds tests/test_score_gpu.py derives in its docstring
and the inputs of its cases.  Test infrastructure only."""
import numpy as np

import sampler_ref as R

U = R.U
F32 = np.float32
KNOWN_STREAM_SEQ = 11
SHAPES = ((2, 5, 3), (2, 37, 20), (1, 257, 20), (1, 600, 32))      # L = 257 crosses the 256-thread walk, C = 32 is CMAX
MAX_SPREAD = 60.0


# ----------------------------------------------------------------------------------------------------- fp64 statements
def onehot_logits(x0, C):
    """Logits whose float64 softmax is exactly the one-hot of x0: 0 there, -inf elsewhere.  x0 int [B, L] >= 0."""
    x0 = np.asarray(x0, dtype=np.int64)
    lg = np.full(x0.shape + (C,), -np.inf)
    np.put_along_axis(lg, x0[..., None], 0.0, axis=-1)
    return lg


def p_theta(xt, logits, Qsb, Qtb):
    """[N, C]: the law the sampler draws z_s from (sampler_ref.posterior)."""
    return R.posterior(xt, logits, Qsb, Qtb)


def p_theta_from_pred(xt, pred, Qsb, Qtb):
    """p_theta from a given x0 prediction pred [B, L, C] (rows summing to 1), e.g. the fp32 softmax with its underflows:
    softmax(log pred) = pred."""
    with np.errstate(divide="ignore"):
        return R.posterior(xt, np.log(np.asarray(pred, dtype=np.float64)), Qsb, Qtb)


def q_post(xt, x0, Qsb, Qtb):
    """[N, C]: the same expression with the x0 prediction replaced by the one-hot of x0; NaN rows where x0 < 0."""
    x0 = np.asarray(x0, dtype=np.int64)
    C = np.asarray(Qsb).shape[-1]
    q = R.posterior(xt, onehot_logits(np.maximum(x0, 0), C), Qsb, Qtb)
    q[x0.reshape(-1) < 0] = np.nan
    return q


def kl_terms(q, p):
    """[N, C]: q log(q / p), 0 where q == 0, +inf where q > 0 and p == 0."""
    q, p = np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = q * (np.log(q) - np.log(p))
    t = np.where(q > 0, t, 0.0)
    t = np.where((q > 0) & (p == 0), np.inf, t)
    return np.where(np.isnan(q), np.nan, t)


def kl(q, p):
    return kl_terms(q, p).sum(axis=-1)


def nll(logits, x0):
    """[N]: -log_softmax(logits)[x0] = lse - (logit[x0] - max); NaN where x0 < 0."""
    x0 = np.asarray(x0, dtype=np.int64).reshape(-1)
    lg = np.asarray(logits, dtype=np.float64).reshape(len(x0), -1)
    d = lg - lg.max(axis=-1, keepdims=True)
    out = np.log(np.exp(d).sum(axis=-1)) - d[np.arange(len(x0)), np.maximum(x0, 0)]
    return np.where(x0 < 0, np.nan, out)


def prior(q_top, x0):
    """KL(q(z_T | x0) || uniform) per position: sum_c p log(C p), p the normalised column x0 of q_top [C, C]; 0 for x0 < 0."""
    q = np.asarray(q_top, dtype=np.float64)
    C = q.shape[0]
    x0 = np.asarray(x0, dtype=np.int64)
    p = q[:, np.maximum(x0, 0)]                                   # [C, ...]
    p = p / p.sum(axis=0, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(p > 0, p * np.log(C * p), 0.0)
    return np.where(x0 < 0, 0.0, t.sum(axis=0))


def level_set(T, levels=None):
    """(S, w): every step index, or {0} and the multiples of ``levels`` below T; w = (T - 1) / |S \\ {0}| (0: none)."""
    k = 1 if levels is None else levels
    S = [0] + [s for s in range(1, T) if s % k == 0]
    return S, ((T - 1) / (len(S) - 1) if len(S) > 1 else 0.0)


def combine(prior_sum, terms, w):
    """bound = prior + term_0 + w * sum of the other levels; terms [S, ...]."""
    terms = np.asarray(terms, dtype=np.float64)
    return prior_sum + terms[0] + (w * terms[1:].sum(axis=0) if len(terms) > 1 else 0.0)


# ----------------------------------------------------------------------------------------------------- exact fp32 rules
def item_sum_fp32(values, mask):
    """(sum fp32, count) of one item in the kernel's fixed shape: lane j of 64 adds positions j, j + 64, .. in order, a
    masked-out position adding +0; then the xor butterfly 32, 16, .. 1.  Sequential fp32, no product: exact."""
    v = np.asarray(values)
    assert v.dtype == F32 and v.ndim == 1
    m = np.asarray(mask).astype(bool)
    acc = np.zeros(64, dtype=F32)
    for l in range(len(v)):
        acc[l % 64] = acc[l % 64] + (v[l] if m[l] else F32(0))
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ off]
        assert acc.dtype == F32
    return acc[0], int(m.sum())


def forward_levels(x0, Qtb, keys, seed, steps):
    """int64 [N, L]: the keyed forward noising at per-item steps -- pick_fp32 on the fp32 column x0 of Qtb[n] with the
    uniforms of stream 11 at step steps[n]; class 0 for padding rows (x0 < 0) and rows of no item."""
    x0 = np.asarray(x0)
    N, L = x0.shape
    keys = np.asarray(keys).reshape(N, L, 2)
    out = np.zeros((N, L), dtype=np.int64)
    for n in range(N):
        p32 = R.forward_column(np.asarray(Qtb, dtype=F32)[n:n + 1], x0[n:n + 1])
        u = R.keyed_uniforms(keys[n], seed, KNOWN_STREAM_SEQ, int(steps[n]))
        live = (x0[n] >= 0) & (keys[n, :, 1] >= 0)
        out[n] = np.where(live, R.pick_fp32(p32, u, 1), 0)
    return out


# ----------------------------------------------------------------------------------------------------- bounds
def spread(logits, C):
    lg = np.asarray(logits, dtype=np.float64).reshape(-1, C)
    return lg.max(axis=-1) - lg.min(axis=-1)


def prob_eps(logits, C):
    """[N]: (7 C + 20 + 4 D) u, the relative bound of a posterior probability (tests/test_sampler_forms_gpu.py)."""
    return (7 * C + 20 + 4 * spread(logits, C)) * U


def kl_bound(q, p, logits, C):
    """[N]: the absolute bound on the fp32 KL (tests/test_score_gpu.py's docstring), from the float64 q and p."""
    eq, ep = (7 * C + 20) * U, prob_eps(logits, C)
    on = q > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        lq, lp = np.abs(np.log(q)), np.abs(np.log(p))
        d = np.abs(np.log(q) - np.log(p))
        logs = np.where(on, q * ((eq + ep[:, None]) + 2 * U * (lq + lp) + U * d), 0.0).sum(axis=-1)
        terms = np.where(on, q * d, 0.0).sum(axis=-1)
        return logs + (eq + (C + 4) * U) * terms


def nll_bound(logits, ref, C):
    """[N]: (2 D + C + 5) u + 3 u ref."""
    return (2 * spread(logits, C) + C + 5) * U + 3 * U * np.abs(ref)


# ----------------------------------------------------------------------------------------------------- inputs of the GPU test
def score_x0(B, L, C, seed=61):
    """x0 int32 [B, L]: random classes, every seventh row equal to nothing (-1, a padding row), the last row too (where
    there is more than one)."""
    rng = np.random.default_rng(seed + 100 * B + L + C)
    x0 = rng.integers(0, C, (B, L)).astype(np.int32)
    flat = x0.reshape(-1)
    if flat.size > 1:
        flat[3::7] = -1
        flat[-1] = -1
    return x0


def final_flags(B):
    """is_final uint8 [B]: the last item of two or more."""
    f = np.zeros(B, dtype=np.uint8)
    if B > 1:
        f[-1] = 1
    return f
