"""numpy float64 statements of the diffusion-process kernels of csrc/sampler.hip that tests/strided_ref.py and
tests/known_ref.py do not hold: the DDPM ancestral update, forward noising, the discrete posterior and its forward
column -- written from the formulas of oracle/structure.py and oracle/sequence.py, not from the kernels -- and the two
rules that are functions of fp32 values alone and that a kernel must therefore match exactly: the inverse-CDF class
pick and the angular wrap.  Below them, the fixed inputs of tests/test_sampler_forms_gpu.py, which
tests/test_sampler_ref_cpu.py examines where no GPU is needed.  Test infrastructure only."""
import numpy as np

import keyed_ref as K
from strided_ref import circ, wrap_pi  # noqa: F401  (circ: the tests compare by circular distance)

U = 2.0 ** -24
F32 = np.float32


def _f64(v):
    return np.asarray(v, dtype=np.float64)


# ----------------------------------------------------------------------------------------------------- fp64 statements
def ddpm(row, x, e, z=None, wrap=False):
    """The ancestral update from the four coefficients (sra, beta, s1m, sigma): mean = sra (x - beta e / s1m), plus
    sigma z where sigma != 0 and z is given.  Returns (out, parts): ``parts`` holds v, the value before the wrap, and
    G = sra (|x| + |beta e / s1m|) + |sigma z|, what the fp32 roundings of the expression scale with."""
    sra, beta, s1m, sigma = (float(v) for v in row[:4])
    x, e = _f64(x), _f64(e)
    q = beta * e / s1m
    v = sra * (x - q)
    G = sra * (np.abs(x) + np.abs(q))
    if sigma != 0.0 and z is not None:
        v = v + sigma * _f64(z)
        G = G + np.abs(sigma * _f64(z))
    return (wrap_pi(v) if wrap else v), {"v": v, "G": G}


def q_sample(a, s, x0, noise):
    """q(x_t | x_0) on the circle: wrap(a x0 + s noise); a, s scalars or arrays that broadcast.  Returns (out, parts)
    with v before the wrap and G = |a x0| + |s noise|."""
    a, s, x0, noise = _f64(a), _f64(s), _f64(x0), _f64(noise)
    v = a * x0 + s * noise
    return wrap_pi(v), {"v": v, "G": np.abs(a * x0) + np.abs(s * noise)}


def softmax(logits):
    lg = _f64(logits)
    ex = np.exp(lg - lg.max(axis=-1, keepdims=True))
    return ex / ex.sum(axis=-1, keepdims=True)


def posterior_unnormalised(xt, logits, Qsb, Qtb):
    """[N, C]: sum_x0 pred[x0] Qt[c][xt] Qsb[x0][c] / Qtb[x0][xt] with Qt = (Qsb / Qtb) / rowsum and a zero denominator
    replaced by 1e-6.  xt int [B, L], logits [B, L, C], Qsb / Qtb [B, C, C]."""
    xt = np.asarray(xt, dtype=np.int64)
    B, L = xt.shape
    Qsb, Qtb = _f64(Qsb), _f64(Qtb)
    C = Qsb.shape[-1]
    ratio = Qsb / Qtb
    Qt = ratio / ratio.sum(axis=-1, keepdims=True)
    pred = softmax(_f64(logits).reshape(B * L, C))
    b = np.repeat(np.arange(B), L)
    j = xt.reshape(-1)
    left = Qt[b, :, j]                                  # [N, C]: Qt[b][c][xt]
    den = Qtb[b, :, j].copy()                           # [N, C]: Qtb[b][x0][xt]
    den[den == 0.0] = 1e-6
    post = left[:, None, :] * Qsb[b] / den[:, :, None]  # [N, x0, c]
    return (pred[:, :, None] * post).sum(axis=1)


def posterior(xt, logits, Qsb, Qtb):
    """prob [N, C] of the reverse step: the unnormalised posterior, an all-zero row set to 1e-5 per class, each row
    divided by its sum."""
    un = posterior_unnormalised(xt, logits, Qsb, Qtb)
    un[un.sum(axis=-1) == 0.0] = 1e-5
    return un / un.sum(axis=-1, keepdims=True)


def forward_column(Qtb, x0):
    """p[n][c] = Qtb[b][c][x0[n]], the forward law of a row of class x0; a padding row (x0 < 0) is all zero.
    Keeps the dtype of Qtb.  x0 int [B, L]."""
    x0 = np.asarray(x0, dtype=np.int64)
    B, L = x0.shape
    Qtb = np.asarray(Qtb)
    b = np.repeat(np.arange(B), L)
    j = x0.reshape(-1)
    p = Qtb[b, :, np.maximum(j, 0)].copy()
    p[j < 0] = 0
    return p


# ----------------------------------------------------------------------------------------------------- exact fp32 rules
def pick_fp32(p32, u32, mode):
    """The class pick in sequential fp32: ``total`` and ``cum`` added in class order, thr = u * total, index =
    #{c : cum[c] <= thr} clamped to C - 1; mode 0: the first maximum.  No product feeds a sum, so the result does not
    depend on whether multiply-adds are fused: a function of the fp32 inputs alone.  p32 [N, C], u32 [N] -> int64 [N]."""
    p = np.asarray(p32)
    assert p.dtype == F32 and p.ndim == 2
    N, C = p.shape
    if mode == 0:
        return np.argmax(p, axis=1).astype(np.int64)
    u = np.asarray(u32)
    assert u.dtype == F32 and u.shape == (N,)
    total = np.zeros(N, dtype=F32)
    for c in range(C):
        total = total + p[:, c]
    thr = u * total
    assert total.dtype == F32 and thr.dtype == F32
    cum = np.zeros(N, dtype=F32)
    cnt = np.zeros(N, dtype=np.int64)
    for c in range(C):
        cum = cum + p[:, c]
        cnt += cum <= thr
    return np.minimum(cnt, C - 1)


PI_F = F32(3.14159265358979323846)
TWO_PI_F = F32(6.28318530717958647692)


def wrap_pi_fp32(v):
    """modulo_with_wrapped_range(v, -pi, pi) in fp32 as torch evaluates it: shift by the fp32 pi, fmod by the fp32 2 pi,
    + 2 pi when the remainder is negative (and not zero), shift back.  For bit comparison."""
    v = np.asarray(v)
    assert v.dtype == F32
    r = np.fmod(v + PI_F, TWO_PI_F)
    r = np.where((r != 0) & (r < 0), r + TWO_PI_F, r)
    out = r - PI_F
    assert out.dtype == F32
    return out


# ----------------------------------------------------------------------------------------------------- inputs of the GPU test
N_BIG = 2048 * 256 * 4 + 5                 # more float4 groups than the capped grid has threads, plus a tail
SIZES = (1, 3, 4, 5, 1023, 8 * 37, N_BIG)
TIMESTEPS = (999, 500, 1, 0)
EDGE_U = (0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24)


def ddpm_inputs(n=N_BIG, seed=41):
    """State x in [-pi, pi), predicted noise e and draws z ~ N(0, 1), fp32; smaller sizes are prefixes."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-np.pi, np.pi, n).astype(F32)
    x[x >= PI_F] = -PI_F
    return x, rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)


def wrap_grid():
    """fp32 values around every cut and zero of the wrap: the +-8 neighbours of k pi for |k| <= 7, +-0, +-the smallest
    normal, +-1e6, the twelve values of test_kernels_gpu.py::test_wrap_kernel_edge_values, 4096 uniform in [-40, 40]."""
    vals = []
    for k in range(-7, 8):
        c = F32(k * np.pi)
        up = dn = c
        vals.append(c)
        for _ in range(8):
            up, dn = np.nextafter(up, F32(np.inf)), np.nextafter(dn, F32(-np.inf))
            vals += [up, dn]
    tiny = np.finfo(F32).tiny
    vals += [F32(0.0), F32(-0.0), tiny, -tiny, F32(1e6), F32(-1e6)]
    vals += [F32(v) for v in (3.0, -3.0, 0.0, np.pi, -np.pi, 7.5, -7.5, 100.0, -100.0, 3.1415927410125732,
                              -3.1415927410125732, 1e-8)]
    rng = np.random.default_rng(42)
    return np.concatenate([np.array(vals, dtype=F32), rng.uniform(-40.0, 40.0, 4096).astype(F32)])


Q_SAMPLE_CASES = ((1, 1), (6, 7), (6, 296), (3, 174763))     # (B, per); the last: n = 524289, one past the capped grid
Q_SAMPLE_T = {1: (999,), 3: (0, 999, 500), 6: (0, 999, 5, 700, 37, 998)}      # neighbours far apart in the table


def q_sample_inputs(B, per, seed=43):
    """x0 in [-pi, pi), wrapped N(0, 1) noise, fp32 [B, per], and the items' timesteps.  The first and the last element
    of every item hold 1 and -0.75: the neighbouring item's table row then misses the bound there by far."""
    rng = np.random.default_rng(seed + B * 1000 + per)
    x0 = rng.uniform(-np.pi, np.pi, (B, per)).astype(F32)
    x0[x0 >= PI_F] = -PI_F
    noise = wrap_pi(rng.standard_normal((B, per))).astype(F32)
    noise[noise >= PI_F] = -PI_F
    x0[:, 0] = x0[:, -1] = 1.0
    noise[:, 0] = noise[:, -1] = -0.75
    return x0, noise, np.array(Q_SAMPLE_T[B], dtype=np.int64)


def row_stochastic(B, C, seed):
    """Seeded fp32 [B, C, C], rows summing to 1 (to fp32 rounding), every entry >= 1e-3."""
    rng = np.random.default_rng(seed)
    m = rng.random((B, C, C)) + 0.1
    m = (m / m.sum(axis=-1, keepdims=True)).astype(F32)
    assert m.min() >= 1e-3
    return m


POSTERIOR_SHAPES = ((1, 1, 2), (4, 37, 3), (2, 5, 20), (2, 256, 20), (2, 257, 20), (1, 600, 32))


def uniform_sets(N, seed):
    """The fp32 uniforms a draw test runs: one random vector with the four edge values in its first rows, then one
    constant vector per edge value."""
    rng = np.random.default_rng(seed)
    u = rng.random(N).astype(F32)
    u[u >= 1.0] = 0.5
    k = min(N, len(EDGE_U))
    u[:k] = np.array(EDGE_U, dtype=F32)[:k]
    return [u] + [np.full(N, e, dtype=F32) for e in EDGE_U]


def posterior_inputs(B, L, C, Qsb=None, Qtb=None, seed=44):
    """xt int32 [B, L], logits fp32 [B, L, C] (every fifth row spread four times wider) and the two transitions: the given
    ones, or seeded row-stochastic matrices."""
    rng = np.random.default_rng(seed + 10000 * B + 100 * L + C)
    xt = rng.integers(0, C, (B, L)).astype(np.int32)
    logits = (2.0 * rng.standard_normal((B, L, C))).astype(F32)
    logits.reshape(B * L, C)[::5] *= 4.0
    if Qsb is None:
        Qsb, Qtb = row_stochastic(B, C, seed + C), row_stochastic(B, C, seed + C + 1)
    return xt, logits, np.ascontiguousarray(Qsb, dtype=F32), np.ascontiguousarray(Qtb, dtype=F32)


ZERO_COLUMN = 1


def zero_total_inputs(B, L, C, seed=45):
    """posterior_inputs with column ZERO_COLUMN of Qsb set to zero (the other entries of each row rescaled to sum 1):
    rows whose xt is that column get an all-zero unnormalised posterior.  Every third row is given that xt."""
    xt, logits, Qsb, Qtb = posterior_inputs(B, L, C, seed=seed)
    Qsb = Qsb.astype(np.float64)
    Qsb[:, :, ZERO_COLUMN] = 0.0
    Qsb = (Qsb / Qsb.sum(axis=-1, keepdims=True)).astype(F32)
    xt.reshape(-1)[::3] = ZERO_COLUMN
    return xt, logits, Qsb, Qtb


Q_ROWS = {1: (1, 1), 255: (3, 85), 256: (2, 128), 257: (1, 257), 900: (3, 300)}      # B * L -> (B, L)
Q_CLASSES = (2, 20, 32)


def with_exact_zeros(Qtb):
    """Exact zeros written into a [B, C, C] transition: item 0 loses, in column j, the classes {0, C // 2, C - 1} other
    than j % C (zero classes at the front, in the middle and at the end of a row's law; class j % C keeps it non-zero);
    the last item of two or more becomes the identity (the clean level)."""
    Q = np.array(Qtb, dtype=F32)
    B, C = Q.shape[0], Q.shape[-1]
    for j in range(C):
        for c in {0, C // 2, C - 1} - {j % C}:
            Q[0, c, j] = 0.0
    if B > 1:
        Q[-1] = np.eye(C, dtype=F32)
    return Q


def discrete_q_inputs(B, L, C, Qtb=None, seed=46):
    """x0 int32 [B, L] with padding rows (-1), the last row among them (where there is more than one row), and a
    transition with exact zeros."""
    rng = np.random.default_rng(seed + 100 * B * L + C)
    x0 = rng.integers(0, C, (B, L)).astype(np.int32)
    flat = x0.reshape(-1)
    if B * L > 1:                      # a single row is drawn, not padded
        flat[rng.random(B * L) < 0.2] = -1
        flat[-1] = -1
        flat[0] = C - 1
    if Qtb is None:
        Qtb = row_stochastic(B, C, seed + C)
    return x0, with_exact_zeros(Qtb)


IDS = (3, (1 << 32) + 5, (1 << 63) + 7, (1 << 64) - 1, 12345678901)      # above 2^32, above 2^63
SEEDS = (7, 0xDEADBEEFCAFEF00D)


def as_int64(ids):
    """[0, 2^64) -> the int64 of the same bits (the kernels read the word as unsigned)."""
    return np.array([i - (1 << 64) if i >= 1 << 63 else i for i in ids], dtype=np.int64)


def key_table(rows, seed=47):
    """int64 [rows, 2] = (item id, position): ids of IDS, positions in [0, 2^24) with 0, 255 and 2^24 - 1 among them, rows
    of no item (position -1) first, in the middle and last."""
    rng = np.random.default_rng(seed + rows)
    keys = np.empty((rows, 2), dtype=np.int64)
    keys[:, 0] = as_int64(IDS)[rng.integers(0, len(IDS), rows)]
    keys[:, 1] = rng.integers(0, 1 << 24, rows)
    for r, pos in zip((1, 2, 3, rows - 2), (0, 255, (1 << 24) - 1, (1 << 24) - 1)):
        if 0 < r < rows - 1:
            keys[r, 1] = pos
    for r in (0, rows // 2, rows - 1):
        keys[r] = (9, -1)
    return keys


def padded_keys(ids, L):
    """Key table of a padded [B, L] frame: row b * L + l = (ids[b], l)."""
    B = len(ids)
    keys = np.empty((B, L, 2), dtype=np.int64)
    keys[:, :, 0] = as_int64(ids)[:, None]
    keys[:, :, 1] = np.arange(L)[None]
    return keys.reshape(B * L, 2)


def keyed_uniforms(keys, seed, stream, step):
    return K.uniforms(keys, seed, stream, step).astype(F32)
