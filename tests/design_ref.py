"""numpy statements of the sequence design controls (csrc/sampler.hip, "design controls"): the effective logits in fp32
exactly as the kernels form them, and the last step's pick with its scores in float64.  The posterior under controls is
``sampler_ref.posterior`` fed the effective logits.  Below them, the fixed inputs of tests/test_design_gpu.py.  Test
infrastructure only."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24


def effective_logits(logits, bias, inv_temp):
    """z = (logits + bias) * inv_temp in fp32: one add, then one multiply, each rounded.  ``bias`` None: zero."""
    lg = np.asarray(logits)
    assert lg.dtype == F32
    b = np.zeros_like(lg) if bias is None else np.asarray(bias)
    assert b.dtype == F32 and b.shape == lg.shape
    with np.errstate(invalid="ignore", over="ignore"):
        s = lg + b
        z = s * F32(inv_temp)
    assert s.dtype == F32 and z.dtype == F32
    return z


def final_pick(z):
    """(index, logp, entropy) of rows of fp32 effective logits z [N, C]: the first maximum, and in float64
    log_softmax(z)[index] and -sum p log p with 0 log 0 = 0.  A row that is -inf everywhere: index 0, NaN, NaN."""
    z = np.asarray(z)
    assert z.dtype == F32 and z.ndim == 2
    idx = np.argmax(z, axis=1).astype(np.int64)                    # numpy's argmax: the first maximum
    z64 = z.astype(np.float64)
    mx = z64.max(axis=1, keepdims=True)
    dead = np.isneginf(mx[:, 0])
    with np.errstate(invalid="ignore", divide="ignore"):
        d = z64 - np.where(dead[:, None], 0.0, mx)
        e = np.exp(d)
        se = e.sum(axis=1, keepdims=True)
        logsm = d - np.log(se)
        p = e / se
        terms = np.where(p > 0, -p * logsm, 0.0)
    logp = logsm[np.arange(len(z)), idx]
    ent = terms.sum(axis=1)
    logp[dead] = np.nan
    ent[dead] = np.nan
    return idx, logp, ent


def spread(z):
    """[N]: D = max |z - max z| over the finite entries of each row (0 for a row with none)."""
    z64 = np.asarray(z, dtype=np.float64)
    fin = np.isfinite(z64)
    hi = np.where(fin, z64, -np.inf).max(axis=1)
    lo = np.where(fin, z64, np.inf).min(axis=1)
    return np.where(fin.any(axis=1), hi - lo, 0.0)


# ----------------------------------------------------------------------------------------------------- inputs of the GPU test
SHAPES = ((2, 37, 20), (1, 257, 20), (1, 600, 32), (2, 5, 3))      # L below, at and beyond one 256-thread pass; C <= CMAX
TEMPERATURES = (0.5, 1.0, 2.0)
PICK_ROWS = (1, 255, 257, 1000)
PICK_CLASSES = (3, 20, 32)


def inv_temp(temperature):
    return F32(1) / F32(temperature)


def bias_inputs(N, C, seed=51):
    """fp32 [N, C]: finite entries uniform in [-4, 4], -inf on roughly a third of the classes, never on a whole row (the
    class (3 n) % C of row n always stays open)."""
    rng = np.random.default_rng(seed + 100 * N + C)
    b = rng.uniform(-4.0, 4.0, (N, C)).astype(F32)
    closed = rng.random((N, C)) < 1.0 / 3.0
    closed[np.arange(N), (3 * np.arange(N)) % C] = False
    b[closed] = -np.inf
    assert not np.isneginf(b).all(axis=1).any()
    return b


def pick_inputs(rows, C, seed=52):
    """logits fp32 [rows, C] (every fifth row four times wider, every seventh row with its maximum twice: the first one
    must win) and a bias of ``bias_inputs``."""
    rng = np.random.default_rng(seed + 100 * rows + C)
    lg = (2.0 * rng.standard_normal((rows, C))).astype(F32)
    lg[::5] *= 4.0
    b = bias_inputs(rows, C, seed + 1)
    for n in range(0, rows, 7):
        z = lg[n] + b[n]
        k = int(np.argmax(z))
        j = (k + 1 + n % max(C - 1, 1)) % C
        if j != k:
            lg[n, j], b[n, j] = lg[n, k], b[n, k]
    return lg, b
