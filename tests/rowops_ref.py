"""Plain statements of the row, reduction and small-K operations (csrc/rowops.hip, csrc/train_ops.hip), the inputs the GPU
forms test feeds them, and the comparison both test modules use.

Every operation is written out once, for a working dtype ``dt``: float64 is the reference the kernels are held to; float32
is torch's own single-precision evaluation of the same statement, which tests/test_rowops_ref_cpu.py holds to the SAME bound
(an input that torch's fp32 cannot bring within the bound is too ill-conditioned for any fp32 kernel: the input is changed,
never the bound).  Backward formulas are closed forms, checked against torch.autograd in float64 by the CPU test.

Bounds (the project's own, tests/test_kernels_gpu.py and tests/test_backward_gpu.py): ``FWD`` = 2e-6 for forward row ops,
``GRAD`` = 1e-5 for gradients and reductions, both of max |ref|; in addition every output row within 4x the bound of its
own largest |ref|, floored at 1e-3 max |ref| (the per-block rule of tests/test_gemm_forms_gpu.py).
"""
import math

import torch

FWD, GRAD = 2e-6, 1e-5
HS = (256, 512, 768, 1024)
F64 = torch.float64


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------------------------------- comparison
def row_errors(got, ref):
    """(max |got - ref| / max |ref|,  worst row: max_row |got - ref| / max(max_row |ref|, 1e-3 max |ref|))."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.dim() < 2:
        got, ref = got.reshape(1, -1), ref.reshape(1, -1)
    got, ref = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    err = (got - ref).abs()
    scale = float(ref.abs().max())
    if scale == 0.0:
        return (0.0, 0.0) if float(err.max()) == 0.0 else (math.inf, math.inf)
    rows = err.amax(1) / ref.abs().amax(1).clamp_min(1e-3 * scale)
    return float(err.max()) / scale, float(rows.max())


def check_close(got, ref, tol, what):
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    whole, row = row_errors(got, ref)
    assert whole <= tol, f"{what}: rel err {whole:.3g} > {tol:g}"
    assert row <= 4 * tol, f"{what}: a row is off by {row:.3g} of its own magnitude (> {4 * tol:g})"
    return whole, row


# ----------------------------------------------------------------------------------------------------- statements
def normalize(x, eps):
    """(xhat, rstd): biased variance, as nn.LayerNorm."""
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mu) * rstd, rstd


def layernorm(x, gamma, beta, eps, dt=F64):
    xhat, _ = normalize(x.to(dt), eps)
    if gamma is not None:
        xhat = xhat * gamma.to(dt)
    return xhat if beta is None else xhat + beta.to(dt)


def residual_layernorm(x, res, gamma, beta, eps, dt=F64):
    s = x.to(dt) if res is None else x.to(dt) + res.to(dt)
    return layernorm(s, gamma, beta, eps, dt)


def ln_input_grad(g, xhat, rstd):
    return rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))


def layernorm_bwd(dy, s, gamma, eps, dt=F64):
    """(ds, dgamma, dbeta) of y = xhat(s) * gamma + beta."""
    dy = dy.to(dt)
    xhat, rstd = normalize(s.to(dt), eps)
    g = dy if gamma is None else dy * gamma.to(dt)
    return ln_input_grad(g, xhat, rstd), (dy * xhat).sum(0), dy.sum(0)


def _chunks(mod, branch, rows_per_cond, H, dt):
    m = mod.to(dt)[:, 3 * branch * H:3 * (branch + 1) * H].repeat_interleave(rows_per_cond, 0)
    return m[:, :H], m[:, H:2 * H], m[:, 2 * H:]


def adaln_gate(x, y, mod, branch, rows_per_cond, dt=F64):
    """out = x + gate * (LN(y) * (1 + scale) + shift), (shift, scale, gate) = chunks 3 branch .. 3 branch + 2 of the
    conditioning row ``row // rows_per_cond`` of mod [C, 6 H]; LN without affine, eps 1e-5."""
    H = x.shape[1]
    sh, sc, ga = _chunks(mod, branch, rows_per_cond, H, dt)
    yhat, _ = normalize(y.to(dt), 1e-5)
    return x.to(dt) + ga * (yhat * (1 + sc) + sh)


def adaln_gate_indexed(x, y, idx, table, mod, branch, dt=F64):
    """adaln_gate with rows_per_cond = 1 whose conditioning row is table[idx[r]] where 0 <= idx[r] < table rows, else mod[r]."""
    rows = [table[int(i)] if 0 <= int(i) < table.shape[0] else mod[r] for r, i in enumerate(idx.tolist())]
    return adaln_gate(x, y, torch.stack(rows), branch, 1, dt)


def adaln_gate_bwd(dout, y, mod, branch, rows_per_cond, dt=F64):
    """(dy, dmod [C, 6 H]); the other branch's chunks of dmod are zero."""
    M, H = y.shape
    sh, sc, ga = _chunks(mod, branch, rows_per_cond, H, dt)
    yhat, rstd = normalize(y.to(dt), 1e-5)
    go = dout.to(dt)
    dga = go * (yhat * (1 + sc) + sh)
    dsh = go * ga
    dsc = dsh * yhat
    dy = ln_input_grad(dsh * (1 + sc), yhat, rstd)
    dmod = torch.zeros(mod.shape, dtype=dt)
    for i, d in enumerate((dsh, dsc, dga)):
        dmod[:, (3 * branch + i) * H:(3 * branch + i + 1) * H] = d.reshape(M // rows_per_cond, rows_per_cond, H).sum(1)
    return dy, dmod


def linear(x, W, b, dt=F64):
    z = x.to(dt) @ W.to(dt).t()
    return z if b is None else z + b.to(dt)


def embed_layernorm(x, W, b, gamma, beta, eps, post_add=None, rows_per_add=1, dt=F64):
    """(z, out): z = x W^T + b, out = LN(z) * gamma + beta (+ post_add[row // rows_per_add])."""
    z = linear(x, W, b, dt)
    out = layernorm(z, gamma, beta, eps, dt)
    if post_add is not None:
        out = out + post_add.to(dt).repeat_interleave(rows_per_add, 0)[:x.shape[0]]
    return z, out


def head_linear_bwd_dx(dout, W, dt=F64):
    return dout.to(dt) @ W.to(dt)


def small_k_wgrad(g, x, transpose_out=False, dt=F64):
    """(dW [H, F] = g^T x  (or its transpose), db [H] = column sums of g)."""
    dW = g.to(dt).t() @ x.to(dt)
    return (dW.t().contiguous() if transpose_out else dW), g.to(dt).sum(0)


SQRT1_2, INV_SQRT_2PI = 0.70710678118654752440, 0.39894228040143267794


def _phi(z):     # Phi(z) = erfc(-z / sqrt 2) / 2: no cancellation on the negative side
    return 0.5 * torch.special.erfc(-z * SQRT1_2)


def act(z, kind, dt=F64):
    """0: identity, 1: erf GELU, 2: SiLU."""
    z = z.to(dt)
    return z if kind == 0 else (z * _phi(z) if kind == 1 else z * torch.sigmoid(z))


def act_grad(z, kind, dt=F64):
    z = z.to(dt)
    if kind == 0:
        return torch.ones_like(z)
    if kind == 1:
        return _phi(z) + z * torch.exp(-0.5 * z * z) * INV_SQRT_2PI
    sg = torch.sigmoid(z)
    return sg * (1 + z * (1 - sg))


def colsum(x, dt=F64):
    return x.to(dt).sum(0)


def group_sum(x, rows_per_group, dt=F64):
    return x.to(dt).reshape(-1, rows_per_group, x.shape[1]).sum(1)


def absmax(x):
    """max |x| as e3d_absmax_f32 defines it: the order of the bit patterns of |x| (inf above finite, NaN above inf)."""
    return x.float().abs().view(torch.int32).max().view(torch.float32)


# ----------------------------------------------------------------------------------------------------- inputs and cases
def affine(H, tag):
    return 1 + 0.1 * torch.randn(H, generator=gen(H, tag, 1)), torch.randn(H, generator=gen(H, tag, 2))


RESIDUAL_LN_CASES = [(H, M, kind) for H in HS for M in (1, 5) for kind in ("plain", "shifted")]


def residual_ln_inputs(H, M, kind):
    """(x, res, gamma, beta).  ``shifted``: rows with mean 4 and unit spread (a one-pass variance loses them)."""
    x = torch.randn(M, H, generator=gen(H, M, 3))
    x = 4 + x if kind == "shifted" else 3 * x
    return (x, torch.randn(M, H, generator=gen(H, M, 4))) + affine(H, 5)


def constant_rows(H, M=5):
    return torch.tensor([0.0, 1.0, -3.7, 1e-3, 1234.5])[:M, None].expand(M, H).contiguous()


ADALN_FWD_CASES = [(H, M, rpc, br) for H in HS for M, rpc in ((1, 1), (5, 1), (5, 5), (50, 5), (48, 16)) for br in (0, 1)]
ADALN_BWD_CASES = [(H, M, rpc, br) for H in (256, 768)
                   for M, rpc in ((48, 16), (64, 32), (96, 48), (50, 5), (5, 5), (5, 1)) for br in (0, 1)]
ADALN_INDEXED_CASES = [(H, br) for H in (256, 768) for br in (0, 1)]
ADALN_IDX = (-1, 0, 20, 21, 2 ** 30, 7, 20)      # M = 7 rows, 21 table rows: 21 == table_rows reads mod
ADALN_TABLE_ROWS = 21


def adaln_inputs(H, M, rpc, tag=0):
    """(x, y, mod [M / rpc, 6 H], dout)"""
    return (torch.randn(M, H, generator=gen(H, M, rpc, tag, 1)), 2 * torch.randn(M, H, generator=gen(H, M, rpc, tag, 2)),
            torch.randn(M // rpc, 6 * H, generator=gen(H, M, rpc, tag, 3)), torch.randn(M, H, generator=gen(H, M, rpc, tag, 4)))


def hide_other_branch(mod, branch, H):
    """mod with the three chunks of the OTHER branch set to NaN."""
    m = mod.clone()
    m[:, 3 * (1 - branch) * H:3 * (2 - branch) * H] = float("nan")
    return m


# (M, F, H, rows_per_add or None).  Few-rows form: M <= 512; staged form: M > 512 (513 leaves a 1-row tail in the 4-row trip)
_RPA = (None, 3, 16)
EMBED_FEW_CASES = [(M, F, 768, _RPA[(i + j) % 3]) for i, M in enumerate((1, 5, 512)) for j, F in enumerate((1, 3, 8, 20, 32))]
EMBED_FEW_CASES += [(5, 20, 256, 3), (5, 8, 1024, 16)]
EMBED_STAGED_CASES = [(513, 3, 768, 3), (513, 20, 768, 16), (515, 3, 768, 16), (515, 20, 768, 3), (513, 32, 1024, 3),
                      (515, 20, 256, None)]


def embed_inputs(M, F, H, rpa):
    """(x, W, b, gamma, beta, post_add or None): seeded by (F, H) and drawn row by row, so the first rows of a larger M are
    the rows of a smaller one."""
    x = torch.randn(515, F, generator=gen(F, H, 1))[:M].contiguous()
    W, b = torch.randn(H, F, generator=gen(F, H, 2)), torch.randn(H, generator=gen(F, H, 3))
    add = None if rpa is None else torch.randn(172, H, generator=gen(F, H, 4))[:(M + rpa - 1) // rpa].contiguous()
    return (x, W, b) + affine(H, 6) + (add,)


# (H, Nout, M): every H, every Nout and every M at least twice
HEAD_CASES = [(256, 1, 1), (256, 32, 77), (256, 20, 77), (512, 8, 5), (512, 20, 1), (768, 1, 77), (768, 32, 5), (768, 8, 1),
              (1024, 8, 77), (1024, 20, 5)]


def head_inputs(H, Nout, M):
    """(x, W, b, dout): the bias keeps every output row (a single number at Nout = 1) away from a cancelling zero."""
    return (torch.randn(M, H, generator=gen(H, Nout, M, 1)), torch.randn(Nout, H, generator=gen(H, Nout, M, 2)) / math.sqrt(H),
            4 + torch.randn(Nout, generator=gen(H, Nout, M, 3)), torch.randn(M, Nout, generator=gen(H, Nout, M, 4)))


LN_BWD_CASES = [(H, M) for H in (256, 768) for M in (1, 2, 3, 17)]
LN_BWD_ATOMIC_CASE = (512, 33)


def ln_bwd_inputs(H, M):
    """(dy, s, gamma)"""
    return (torch.randn(M, H, generator=gen(H, M, 11)), 3 * torch.randn(M, H, generator=gen(H, M, 12)), affine(H, 13)[0])


def biased(shape, *key):
    """0.5 + N(0, 1): sums over many rows grow with the row count instead of cancelling, so every output of a reduction
    stays comparable with the largest one (the per-row rule then tests the kernel, not the luck of a sum near zero)."""
    return 0.5 + torch.randn(shape, generator=gen(*key))


# (H, g offset in floats, M, F, transpose_out, with_db): float4 kernel when H % 64 == 0 and g is 16-byte aligned
WGRAD_CASES = [(64, 0, 1, 1, 0, 1), (64, 0, 15, 8, 1, 0), (64, 0, 257, 32, 0, 1), (768, 0, 256, 20, 0, 1), (768, 0, 257, 8, 1, 1),
               (768, 0, 300, 20, 1, 0), (768, 0, 1000, 32, 0, 0), (768, 0, 15, 1, 0, 1),
               (100, 0, 1, 8, 0, 1), (100, 0, 300, 20, 1, 1), (200, 0, 257, 1, 0, 0), (200, 0, 1000, 32, 1, 1),
               (768, 1, 300, 20, 0, 1), (768, 1, 256, 32, 1, 0), (64, 1, 257, 32, 0, 1)]
WGRAD_PAIRS = [((64, 0, 257, 32, 0, 1), (64, 1, 257, 32, 0, 1)), ((768, 0, 300, 20, 1, 0), (768, 1, 300, 20, 0, 1))]


def wgrad_inputs(H, M, F):
    """(g [M, H], x [M, F])"""
    return biased((M, H), H, M, F, 1), biased((M, F), H, M, F, 2)


COLSUM_CASES = [(1, 1, 1), (17, 8, 8), (77, 20, 20), (300, 257, 300), (1100, 700, 768), (20010, 8, 8)]     # (M, N, ld)
GROUP_SUM_CASES = [(1, 5, 768), (16, 3, 768), (7, 4, 100), (3, 2, 300), (128, 2, 1024)]     # (rows_per_group, groups, H)
TRANSPOSE_CASES = [(count, rows, cols) for count in (1, 3, 64) for rows, cols in ((1, 1), (31, 33), (64, 64), (100, 70))]


def colsum_input(M, N):
    return biased((M, N), M, N, 21)


def group_sum_input(rpg, groups, H):
    return torch.randn(rpg * groups, H, generator=gen(rpg, groups, H, 22))


ACT_SPECIALS = (0.0, -0.0, 1e-30, -1e-30, 1e-40, -1e-40, 20.0, -20.0, 50.0, -50.0, 88.0, -88.0, 100.0, -100.0, 1e4)
ACT_BIG_N = 4096 * 256 + 3      # one element past the grid of 4096 x 256 threads: the second grid-stride trip


def act_grid():
    """~4k points: a dense grid over [-12, 12] and the special values (fp32)."""
    return torch.cat([torch.linspace(-12.0, 12.0, 4001, dtype=torch.float64).float(), torch.tensor(ACT_SPECIALS)])


def gelu_error(got, z):
    """max |got - gelu(z)| / max(|z|, 1e-30): the figure the kernel's comment bounds by 0.75e-7 (+ fp32 rounding)."""
    z = z.double().cpu()
    return float(((got.double().cpu() - act(z, 1)).abs() / z.abs().clamp_min(1e-30)).max())
