"""The row-complete GEMM + LayerNorm kernel (csrc/gemm_rowln.hip) stated plainly: mirrors of its host arithmetic (which rows
a workgroup owns, in which tiles it walks them), the fp64 statement of the operation, the inputs the GPU forms test feeds it
and the per-row allowance both test modules use.

Host arithmetic.  ``launch_rowln`` gives each workgroup one contiguous group of ``ceil32(ceil(M / n_cu))`` rows, n_cu being
the device's multiprocessor count rounded down to a multiple of 8 (``e3d_cu_count``); ``next_tile_rows`` walks a group in
tiles of 96 / 64 / 32 rows, a 256-row group in one of four orders chosen by ``(blockIdx.x >> 3) & 3``.

Statement.  out = LN(out_scale * (a . w^T) + bias + residual) * gamma + beta, biased variance, eps inside the square root.

Allowance.  A pre-norm error of at most delta in every element of a row moves the row's mean by at most delta, a centred
element c by at most 2 delta and -- to first order -- the variance by 2 mean(c e) <= 2 delta sqrt(var), hence rstd by at
most rstd^2 delta, so a normalised element zhat = c rstd moves by at most (2 + |zhat|) delta rstd.  With delta_r = 4 TOL max_j |out_scale (a . w^T)_rj| (TOL: the bound
tests/test_gemm_forms_gpu.py asserts for the arithmetic, 4 TOL its rule for a part of the output against that part's own
magnitude) and the forward row-op bound 2e-6 of tests/test_rowops_forms_gpu.py for the LayerNorm arithmetic itself:

    allow_r = (2 + max_j |zhat_rj|) delta_r rstd_r max |gamma| + 2e-6 max_j |out_ref_rj|.

A row passes when max_j |got_rj - ref_rj| <= allow_r.  tests/test_rowln_ref_cpu.py shows for every input family that the
allowance is not vacuous (allow_r <= 1e-3 max_j |out_ref_rj| on every row) and not too tight (torch's own fp32 matmul and
layer_norm pass it).
"""
import math

import torch

RN = 768                                # the kernel's N
TOL = {19: 5e-6, 3: 3e-5}               # tests/test_gemm_forms_gpu.py: f16x3, bf16x3
LN_FWD = 2e-6                           # tests/test_rowops_forms_gpu.py (rowops_ref.FWD)
MODES = {"f16x3": 19, "bf16x3": 3}
GROUPS = (128, 160, 192, 224, 256, 288, 320, 352)
F64 = torch.float64


# ----------------------------------------------------------------------------------------------------- host arithmetic
def cu_count(multiprocessors):
    """e3d_cu_count: the multiprocessor count rounded down to a multiple of 8 (at least 8)."""
    n = multiprocessors - multiprocessors % 8
    return n if n > 0 else 8


def group_rows(M, n_cu):
    """launch_rowln: (rows_per_wg, grid, rows of the last workgroup)."""
    rows_per_wg = ((M + n_cu - 1) // n_cu + 31) // 32 * 32
    grid = (M + rows_per_wg - 1) // rows_per_wg
    return rows_per_wg, grid, M - (grid - 1) * rows_per_wg


def pattern_of(block):
    return (block >> 3) & 3


def next_tile_rows(left, pattern, group):
    if group == 256:
        if pattern == 1 and left == 256:
            return 64
        if pattern == 2 and left == 160:
            return 64
        if pattern == 3:
            return 64
    if left >= 160 or left == 96:
        return 96
    if left > 96:
        return 64
    return left


def walk(group, pattern=0):
    """The tiles (rows each) in which a workgroup with ``group`` rows (a multiple of 32) walks them."""
    assert group > 0 and group % 32 == 0
    tiles, left = [], group
    while left > 0:
        tiles.append(next_tile_rows(left, pattern, group))
        left -= tiles[-1]
    assert left == 0
    return tiles


def smallest_m(g, n_cu):
    """The smallest M whose workgroups own g rows each."""
    return (g - 32) * n_cu + 32


def block_rows(M, n_cu, block):
    """(first row, end row) of workgroup ``block``."""
    rpw, grid, _ = group_rows(M, n_cu)
    assert 0 <= block < grid
    return block * rpw, min(M, (block + 1) * rpw)


def checked_blocks(M, n_cu):
    """The workgroups whose whole groups the GPU test holds to fp64: the first of each walk order (blocks 0, 8, 16, 24), the
    two before the last and the last (short) one."""
    grid = group_rows(M, n_cu)[1]
    return sorted({b for b in (0, 8, 16, 24, grid - 3, grid - 2, grid - 1) if 0 <= b < grid})


# ----------------------------------------------------------------------------------------------------- inputs
def params(K, seed=0):
    """(w [768, K] ~ N(0, 1/K), bias ~ N(0, 1), gamma in [0.5, 1.5), beta ~ N(0, 1)) on the CPU."""
    gen = torch.Generator().manual_seed(1000003 * K + seed + 17)
    w = torch.randn(RN, K, generator=gen) / math.sqrt(K)
    return w, torch.randn(RN, generator=gen), torch.rand(RN, generator=gen) + 0.5, torch.randn(RN, generator=gen)


FAMILIES = ("spread", "large_mean")


def inputs(M, K, family="spread", device="cpu", seed=0):
    """(a [M, K], residual [M, 768]) generated on ``device``: a ~ N(0, 1) with every 97th row x 1e3 and every 101st (from 5)
    x 1e-3; residual = 3 N(0, 1) + 0.5 ("spread") or 40 + 0.5 N(0, 1) ("large_mean": a large mean over a small spread)."""
    gen = torch.Generator(device=device).manual_seed(7919 * M + 31 * K + seed)
    a = torch.randn(M, K, device=device, generator=gen)
    a[::97] *= 1e3
    a[5::101] *= 1e-3
    r = torch.randn(M, RN, device=device, generator=gen)
    res = r * 3 + 0.5 if family == "spread" else r * 0.5 + 40
    assert family in FAMILIES
    return a, res


# what tests/test_rowln_forms_gpu.py::test_abi_edges launches: (id, mode, family, bias present, log2 of the weight's
# pre-multiplier -- out_scale is its inverse --, eps).  Every case runs with its residual and without one.
ABI_CASES = [
    ("no_bias", "f16x3", "spread", False, 0, 1e-12),
    ("out_scale", "bf16x3", "spread", True, 3, 1e-12),
    ("eps_1e-12", "f16x3", "spread", True, 0, 1e-12),
    ("eps_1e-5", "f16x3", "spread", True, 0, 1e-5),
    ("eps_1e-2", "f16x3", "spread", True, 0, 1e-2),
    ("large_mean_f16x3", "f16x3", "large_mean", True, 0, 1e-12),
    ("large_mean_bf16x3", "bf16x3", "large_mean", True, 0, 1e-12),
]
WALK_KS = (64, 96, 768)                 # test_row_group_walks
SHORT_KS = (64, 96, 128, 1024)          # test_short_reductions_across_tiles
ABI_K = 96


def rows_differ(x):
    """Every row differs from the rows 32, 64 and 96 places after it: a tile that reads its predecessor's image cannot pass."""
    return all(bool((x[:-d] != x[d:]).any(1).all()) for d in (32, 64, 96) if x.shape[0] > d)


# ----------------------------------------------------------------------------------------------------- statement
def statement(a, w, bias, res, gamma, beta, eps, out_scale=1.0, dt=F64):
    """(out, product, zhat, rstd) in ``dt``; product = out_scale * (a . w^T)."""
    prod = (a.to(dt) @ w.to(dt).t()) * out_scale
    z = prod
    if bias is not None:
        z = z + bias.to(dt)
    if res is not None:
        z = z + res.to(dt)
    mu = z.mean(-1, keepdim=True)
    var = ((z - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    zhat = (z - mu) * rstd
    return zhat * gamma.to(dt) + beta.to(dt), prod, zhat, rstd.squeeze(-1)


def statement_f32(a, w, bias, res, gamma, beta, eps, out_scale=1.0):
    """The same statement by torch's own fp32 operators."""
    z = (a.float() @ w.float().t()) * out_scale
    if bias is not None:
        z = z + bias.float()
    if res is not None:
        z = z + res.float()
    return torch.nn.functional.layer_norm(z, (z.shape[-1],), gamma.float(), beta.float(), eps)


def allowance(out, prod, zhat, rstd, gamma, terms):
    """allow_r [M] (fp64) from the fp64 statement's parts."""
    delta = 4 * TOL[terms] * prod.abs().amax(1)
    return (2 + zhat.abs().amax(1)) * delta * rstd * float(gamma.abs().max()) + LN_FWD * out.abs().amax(1)


def row_excess(got, ref, allow):
    """(max_r err_r / allow_r, its row): at most 1 when every row passes."""
    err = (got.detach().double().cpu() - ref).abs().amax(1)
    ratio = err / allow
    r = int(ratio.argmax())
    return float(ratio[r]), r


def check_rows(got, a, w, bias, res, gamma, beta, eps, terms, what, out_scale=1.0):
    """Rows of ``got`` against the fp64 statement of the same rows with the per-row allowance; returns the largest
    err_r / allow_r."""
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    ref, prod, zhat, rstd = statement(a, w, bias, res, gamma, beta, eps, out_scale)
    allow = allowance(ref, prod, zhat, rstd, gamma, terms)
    worst, r = row_excess(got, ref, allow)
    assert worst <= 1.0, f"{what}: row {r} is off by {worst:.3g} of its allowance {float(allow[r]):.3g}"
    return worst
