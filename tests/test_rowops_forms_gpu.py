"""Every row, reduction and small-K kernel of csrc/rowops.hip and csrc/train_ops.hip at every launcher branch, against the
fp64 statements of tests/rowops_ref.py (whose inputs tests/test_rowops_ref_cpu.py shows to be well enough conditioned for
the bounds below).  The forms are forced by operand properties only -- M against 512, F % 4, pointer alignment, H % 64,
rows_per_cond % 16, adjacency of dgamma / dbeta -- through the C ABI.

One row per ``hipLaunchKernelGGL`` site (R = csrc/rowops.hip, T = csrc/train_ops.hip):

=====  ==========================================  ====================================  =================================================
line   kernel instantiation (V = H / 256: 1..4)    forced by                             test id
=====  ==========================================  ====================================  =================================================
R:320  residual_layernorm_kernel<V>                e3d_residual_layernorm_fwd, each H    test_residual_layernorm[*]
R:332  residual_layernorm_kernel<V, true>          e3d_residual_layernorm_drop_fwd       test_dropout_gpu.py::test_dropout_folded_into_the_residual_layernorm_kernels
R:346  residual_layernorm_kernel<V, true, true>    ..._drop_fwd_keyed                    test_keyed_dropout_gpu.py::test_keyed_residual_layernorm_pair_against_fp64_and_the_unfused_kernels
R:357  adaln_gate_kernel<V>                        e3d_adaln_gate_fwd, each H            test_adaln_gate_fwd[*]
R:372  embed_layernorm_rows_kernel<V>, 16-B loads  M <= 512, F % 4 == 0, x | W aligned   test_embed_layernorm_few_rows[*-8-*|*-20-*|*-32-*]
R:372  embed_layernorm_rows_kernel<V>, scalar      M <= 512, F % 4 != 0 or x at +4 B     test_embed_layernorm_few_rows[*-1-*|*-3-*], test_embed_layernorm_unaligned_x
R:388  embed_layernorm_kernel<V> (LDS-staged)      M > 512                               test_embed_layernorm_staged[*], test_embed_layernorm_forms_agree[*]
R:406  classify_onehot_kernel<true>                F % 4 == 0, x aligned                 test_onehot_modulation_gpu.py::test_classification[True]
R:408  classify_onehot_kernel<false>               otherwise                             test_onehot_modulation_gpu.py::test_classification[False]
R:417  adaln_gate_indexed_kernel<V>                e3d_adaln_gate_indexed_fwd            test_adaln_gate_indexed[*]
R:427  head_linear_kernel<V>                       e3d_head_linear_fwd, each H           test_head_linear[*]
R:445  absmax_kernel                               e3d_absmax_f32                        test_absmax_*
T:553  layernorm_bwd_kernel<V> (atomics)           e3d_layernorm_bwd; both zero-fills    test_layernorm_bwd_atomics_form[adjacent|separate]
T:576  layernorm_bwd_kernel<V, true, true>, ws     e3d_layernorm_bwd_ws_keyed            test_keyed_dropout_gpu.py::test_keyed_residual_layernorm_pair_against_fp64_and_the_unfused_kernels
T:579  layernorm_bwd_kernel<V, true>, ws           e3d_layernorm_bwd_ws, ds_dropped      test_dropout_gpu.py::test_dropout_folded_into_the_residual_layernorm_kernels
T:582  layernorm_bwd_kernel<V>, ws                 e3d_layernorm_bwd_ws, no ds_dropped   test_layernorm_bwd[*], test_layernorm_bwd_without_gamma[*]
T:586  ln_param_grad_sum_kernel                    dgamma or dbeta wanted                test_layernorm_bwd[*-True]  (not launched: [*-False])
T:621  layernorm_bwd_kernel<V, true, true>         e3d_layernorm_bwd_drop_keyed          test_layernorm_bwd_drop_atomics_forms[keyed]
T:624  layernorm_bwd_kernel<V, true>               e3d_layernorm_bwd_drop                test_layernorm_bwd_drop_atomics_forms[seeded]
T:650  adaln_gate_bwd_shared_kernel<V>             rows_per_cond % 16 == 0               test_adaln_gate_bwd[*-48-16-*|*-64-32-*|*-96-48-*]
T:654  adaln_gate_bwd_kernel<V>, atomics           rows_per_cond % 16 != 0, > 1          test_adaln_gate_bwd[*-50-5-*|*-5-5-*]
T:654  adaln_gate_bwd_kernel<V>, stores            rows_per_cond == 1                    test_adaln_gate_bwd[*-5-1-*]
T:661  act_fwd_kernel                              e3d_act_fwd                           test_act_*
T:667  act_bwd_kernel                              e3d_act_bwd                           test_act_*
T:680  colsum_kernel                               e3d_colsum                            test_colsum[*]
T:697  transpose_grouped_kernel                    e3d_transpose_grouped_f32             test_transpose_grouped[*]
T:705  group_sum_kernel                            e3d_group_sum                         test_group_sum[*]
T:719  small_k_wgrad4_kernel (float4)              H % 64 == 0 and g 16-B aligned        test_small_k_wgrad[64-0-*|768-0-*]
T:722  small_k_wgrad_kernel (fallback)             H % 64 != 0 or g at +4 B              test_small_k_wgrad[100-*|200-*|*-1-*], test_small_k_wgrad_kernels_agree[*]
T:730  head_linear_bwd_dx_kernel<V>                e3d_head_linear_bwd_dx, each H        test_head_linear[*]
=====  ==========================================  ====================================  =================================================

Conventions.  Every output the ABI lets the caller place is a block in the middle of a larger allocation filled with a
sentinel: >= 16 guard rows before and after, guard columns where a leading dimension exists; every guard word must be
bit-unchanged afterwards, and what the output held before (the sentinel) must not survive.  Inputs carry NaN rows after
row M - 1, NaN in the padding columns of strided inputs and NaN in every chunk or row the kernel must not read, so a consumed
over-read shows in the result.  The guards exist so that an overrun lands inside the allocation and fails an assertion; no
case is shaped to fault.  Kernels without atomics run twice and must be bit-identical.

Bounds (rowops_ref.check_close): 2e-6 of max |ref| for forward row ops, 1e-5 for gradients and reductions, and every
output row within 4x that of its own largest |ref| (floored at 1e-3 max |ref|, the GEMM forms test's per-block rule).

Measured on an MI355X over rowops_ref.act_grid() (asserted value in brackets):
  gelu_erf forward, max |got - ref| / max(|z|, 1e-30):  1.77e-7  [3.56e-7 = 2x; cap 5e-7].  Below 2.5e-7: the erfc fit's
                                                        0.75e-7 plus about an ulp of |z|, as the kernel's comment says.
  SiLU forward, max |got - ref|:                        1.09e-6  [2e-6: the cap; 4x would be 4.4e-6].  One to two ulp of |z| near 12.
  GELU derivative, max |got - ref|:                     1.09e-7  [4.4e-7 = 4x; cap 2e-6]
  SiLU derivative, max |got - ref|:                     6.7e-7   [2e-6: the cap; 4x would be 2.7e-6].  sg (1 + z (1 - sg)) loses
                                                        1 - sg to cancellation for z ~ 10 (sg rounds to 1 - 4.5e-5 +- 6e-8) and
                                                        multiplies that by z: inherent to the formula in fp32, within the cap.
"""
import ctypes

import pytest
import torch

import rowops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
G = 16                  # guard rows on each side of an output
SENTINEL = -7777.25

# max |got - ref| / max(|z|, 1e-30) of the hand-written erfc GELU over R.act_grid(), measured on an MI355X.  The kernel's
# comment derives 0.75e-7 from the fit; hardware rcp / exp2 and the fp32 roundings add about an ulp each of 0.5 |z| erfc.
GELU_FWD_MEASURED = 1.78e-7
GELU_FWD_BOUND = min(2 * GELU_FWD_MEASURED, 5e-7)
# max |got - ref| (absolute; the derivatives are O(1)), measured on an MI355X: libm expf / erff
ACT_ABS_MEASURED = {("fwd", 2): 1.10e-6, ("bwd", 1): 1.10e-7, ("bwd", 2): 6.8e-7}
ACT_ABS_BOUND = {k: min(4 * v, 2e-6) for k, v in ACT_ABS_MEASURED.items()}


# ----------------------------------------------------------------------------------------------------- plumbing
def _s():
    return torch.cuda.current_stream().cuda_stream


def call(pkg, name, *args):
    pkg.hip.check(getattr(pkg.hip.lib(), name)(*args, _s()), name)
    torch.cuda.synchronize()


def bits(t):
    return t.contiguous().view(torch.int32)


class Out:
    """A [rows, cols] output (row stride ``ld``) in the middle of a sentinel-filled [rows + 2 G, ld] allocation."""

    def __init__(self, rows, cols, ld=None, zero=False, fill=SENTINEL, flat=False):
        ld = cols if ld is None else ld
        self.rows, self.cols, self.flat = rows, cols, flat
        self.big = torch.full((rows + 2 * G, ld), fill, device=DEV)
        self.v = self.big[G:G + rows, :cols]
        if zero:
            self.v.zero_()
        self.before = self.big.clone()
        self.ptr = self.v.data_ptr()

    def row(self, i):
        return self.v[i].data_ptr()

    def guards_intact(self):
        same = bits(self.big) == bits(self.before)
        same[G:G + self.rows, :self.cols] = True
        return bool(same.all())

    def untouched(self):
        return torch.equal(bits(self.big), bits(self.before))

    def get(self, what):
        assert self.guards_intact(), f"{what}: a write outside the output"
        return self.v.clone().reshape(-1) if self.flat else self.v.clone()


def Vec(n, **kw):
    """A vector output of n floats with G guard floats on each side."""
    return Out(n, 1, flat=True, **kw)


def dev_in(x, offset=0, tail=None):
    """x on the device with NaN after its last element (``tail`` floats, default four rows) and ``offset`` NaN floats
    before its first: the returned view starts ``4 * offset`` bytes after a 16-byte boundary."""
    if x is None:
        return None
    if tail is None:
        tail = 4 * (x.shape[-1] if x.dim() > 1 else 1) + 64
    flat = torch.cat([torch.full((offset,), NAN), x.reshape(-1).float(), torch.full((tail,), NAN)]).to(DEV)
    return flat[offset:offset + x.numel()].view(x.shape)


def strided_in(x, ld):
    """x [M, N] as a column block of a NaN-filled [M + 4, ld] device buffer."""
    M, N = x.shape
    buf = torch.full((M + 4, ld), NAN)
    buf[:M, :N] = x
    return buf.to(DEV)[:M, :N]


def p(t):
    return None if t is None else t.data_ptr()


def twice(run, what):
    """run() -> tuple of tensors; two calls must agree bit for bit.  Returns the first."""
    a, b = run(), run()
    for u, v in zip(a, b):
        assert torch.equal(bits(u), bits(v)), f"{what}: repeated call differs"
    return a


# ----------------------------------------------------------------------------------------------------- residual LayerNorm
@pytest.mark.parametrize("H,M,kind", R.RESIDUAL_LN_CASES)
def test_residual_layernorm(pkg, hip, H, M, kind):
    x, res, ga, be = R.residual_ln_inputs(H, M, kind)
    xd, rd, gd, bd = dev_in(x), dev_in(res), dev_in(ga), dev_in(be)
    for r_cpu, r_dev in ((res, rd), (None, None)):
        what = f"residual_layernorm H={H} M={M} {kind} res={r_cpu is not None}"

        def run():
            s_out, out = Out(M, H), Out(M, H)
            call(pkg, "e3d_residual_layernorm_fwd", p(xd), p(r_dev), p(gd), p(bd), 1e-12, s_out.ptr, out.ptr, M, H)
            return s_out.get(what), out.get(what)
        s_got, got = twice(run, what)
        s32 = x if r_cpu is None else x + r_cpu          # fp32
        assert torch.equal(bits(s_got.cpu()), bits(s32)), f"{what}: s_out is not fp32 x + res"
        R.check_close(got, R.residual_layernorm(x, r_cpu, ga, be, 1e-12), R.FWD, what)


@pytest.mark.parametrize("H", R.HS)
def test_residual_layernorm_constant_rows_stay_finite(pkg, hip, H):
    x = R.constant_rows(H)
    ga, be = R.affine(H, 5)
    xd, gd, bd, out = dev_in(x), dev_in(ga), dev_in(be), Out(5, H)
    call(pkg, "e3d_residual_layernorm_fwd", p(xd), None, p(gd), p(bd), 1e-12, None, out.ptr, 5, H)
    assert torch.isfinite(out.get("constant rows")).all()


# ----------------------------------------------------------------------------------------------------- adaLN gate
@pytest.mark.parametrize("H,M,rpc,br", R.ADALN_FWD_CASES)
def test_adaln_gate_fwd(pkg, hip, H, M, rpc, br):
    x, y, mod, _ = R.adaln_inputs(H, M, rpc)
    xd, yd, md = dev_in(x), dev_in(y), dev_in(R.hide_other_branch(mod, br, H))
    what = f"adaln_gate H={H} M={M} rpc={rpc} branch={br}"

    def run():
        out = Out(M, H)
        call(pkg, "e3d_adaln_gate_fwd", p(xd), p(yd), p(md), br, rpc, out.ptr, M, H)
        return (out.get(what),)
    R.check_close(twice(run, what)[0], R.adaln_gate(x, y, mod, br, rpc), R.FWD, what)


@pytest.mark.parametrize("H,br", R.ADALN_INDEXED_CASES)
def test_adaln_gate_indexed(pkg, hip, H, br):
    M, T = len(R.ADALN_IDX), R.ADALN_TABLE_ROWS
    x, y, mod, _ = R.adaln_inputs(H, M, 1)
    table = torch.randn(T, 6 * H, generator=R.gen(H, 31))
    idx = torch.tensor(R.ADALN_IDX, dtype=torch.int32)
    ref = R.adaln_gate_indexed(x, y, idx, table, mod, br)
    # what must not be read holds NaN: the other branch, table rows nobody names, mod rows of rows that name a table row
    mod_h, table_h = R.hide_other_branch(mod, br, H), R.hide_other_branch(table, br, H)
    named = [i for i in R.ADALN_IDX if 0 <= i < T]
    for t in range(T):
        if t not in named:
            table_h[t] = NAN
    for r, i in enumerate(R.ADALN_IDX):
        if 0 <= i < T:
            mod_h[r] = NAN
    xd, yd, md, td = dev_in(x), dev_in(y), dev_in(mod_h), dev_in(table_h)
    idx_d = torch.cat([idx, torch.full((8,), -1, dtype=torch.int32)]).to(DEV)
    what = f"adaln_gate_indexed H={H} branch={br}"

    def run():
        out = Out(M, H)
        call(pkg, "e3d_adaln_gate_indexed_fwd", p(xd), p(yd), p(idx_d), p(td), T, p(md), br, out.ptr, M, H)
        return (out.get(what),)
    got = twice(run, what)[0]
    R.check_close(got, ref, R.FWD, what)
    # and the dense gate on the gathered rows gives the same bits (same arithmetic per row)
    rows = torch.stack([table[i] if 0 <= i < T else mod[r] for r, i in enumerate(R.ADALN_IDX)])
    dense, rows_d = Out(M, H), dev_in(rows)
    call(pkg, "e3d_adaln_gate_fwd", p(xd), p(yd), p(rows_d), br, 1, dense.ptr, M, H)
    assert torch.equal(bits(dense.get(what)), bits(got))


@pytest.mark.parametrize("H,M,rpc,br", R.ADALN_BWD_CASES)
def test_adaln_gate_bwd(pkg, hip, H, M, rpc, br):
    _, y, mod, dout = R.adaln_inputs(H, M, rpc)
    yd, md, dd = dev_in(y), dev_in(R.hide_other_branch(mod, br, H)), dev_in(dout)
    what = f"adaln_gate_bwd H={H} M={M} rpc={rpc} branch={br}"

    def run():
        dy, dmod = Out(M, H), Out(M // rpc, 6 * H, zero=True)       # the caller zeroes dmod
        call(pkg, "e3d_adaln_gate_bwd", p(dd), p(yd), p(md), br, rpc, dy.ptr, dmod.ptr, M, H)
        return dy.get(what), dmod.get(what)
    dy, dmod = twice(run, what) if rpc == 1 else run()
    ref_dy, ref_dmod = R.adaln_gate_bwd(dout, y, mod, br, rpc)
    R.check_close(dy, ref_dy, R.GRAD, what + " dy")
    R.check_close(dmod, ref_dmod, R.GRAD, what + " dmod")
    other = dmod[:, 3 * (1 - br) * H:3 * (2 - br) * H]
    assert int(bits(other).abs().max()) == 0, f"{what}: the other branch's chunks of dmod were written"


# ----------------------------------------------------------------------------------------------------- feature embedding
def run_embed(pkg, ins, M, F, H, rpa, what, x_offset=0):
    x, W, b, ga, be, add = ins
    xd, Wd, bd, gd, bed, ad = dev_in(x, x_offset), dev_in(W), dev_in(b), dev_in(ga), dev_in(be), dev_in(add)
    assert xd.data_ptr() % 16 == 4 * x_offset and Wd.data_ptr() % 16 == 0

    def run():
        z, out = Out(M, H), Out(M, H)
        call(pkg, "e3d_embed_layernorm_fwd", p(xd), F, p(Wd), p(bd), p(gd), p(bed), 1e-12, p(ad), rpa or 0, z.ptr, out.ptr, M, H)
        return z.get(what), out.get(what)
    return twice(run, what)


def check_embed(pkg, M, F, H, rpa, what):
    ins = R.embed_inputs(M, F, H, rpa)
    z, out = run_embed(pkg, ins, M, F, H, rpa, what)
    x, W, b, ga, be, add = ins
    ref_z, ref = R.embed_layernorm(x, W, b, ga, be, 1e-12, add, rpa or 1)
    R.check_close(z, ref_z, R.FWD, what + " z_out")
    R.check_close(out, ref, R.FWD, what + " out")


@pytest.mark.parametrize("M,F,H,rpa", R.EMBED_FEW_CASES)
def test_embed_layernorm_few_rows(pkg, hip, M, F, H, rpa):
    check_embed(pkg, M, F, H, rpa, f"embed_layernorm (few rows) M={M} F={F} H={H} rows_per_add={rpa}")


@pytest.mark.parametrize("M,F,H,rpa", R.EMBED_STAGED_CASES)
def test_embed_layernorm_staged(pkg, hip, M, F, H, rpa):
    check_embed(pkg, M, F, H, rpa, f"embed_layernorm (staged) M={M} F={F} H={H} rows_per_add={rpa}")


@pytest.mark.parametrize("M", [5, 512])
def test_embed_layernorm_unaligned_x(pkg, hip, M):
    """F = 8 with x 4 bytes off a 16-byte boundary: the scalar path, the same per-element order -- the same bits."""
    ins = R.embed_inputs(M, 8, 768, 3)
    aligned = run_embed(pkg, ins, M, 8, 768, 3, "aligned")
    shifted = run_embed(pkg, ins, M, 8, 768, 3, "x at +4 bytes", x_offset=1)
    for a, b in zip(aligned, shifted):
        assert torch.equal(bits(a), bits(b))
    R.check_close(shifted[1], R.embed_layernorm(*ins[:5], 1e-12, ins[5], 3)[1], R.FWD, "embed_layernorm, x at +4 bytes")


@pytest.mark.parametrize("F", [3, 20])
def test_embed_layernorm_forms_agree(pkg, hip, F):
    """The staged form (M = 513) and the few-rows form (its first 512 rows): bit-equal on the shared rows."""
    staged = run_embed(pkg, R.embed_inputs(513, F, 768, 3), 513, F, 768, 3, "staged")
    few = run_embed(pkg, R.embed_inputs(512, F, 768, 3), 512, F, 768, 3, "few rows")
    for a, b in zip(staged, few):
        assert torch.equal(bits(a[:512]), bits(b))


# ----------------------------------------------------------------------------------------------------- output head
@pytest.mark.parametrize("H,Nout,M", R.HEAD_CASES)
def test_head_linear(pkg, hip, H, Nout, M):
    x, W, b, dout = R.head_inputs(H, Nout, M)
    xd, Wd, bd, dd = dev_in(x), dev_in(W), dev_in(b), dev_in(dout)
    what = f"head_linear H={H} Nout={Nout} M={M}"

    def fwd():
        out = Out(M, Nout)
        call(pkg, "e3d_head_linear_fwd", p(xd), p(Wd), p(bd), out.ptr, M, H, Nout)
        return (out.get(what),)

    def bwd():
        dx = Out(M, H)
        call(pkg, "e3d_head_linear_bwd_dx", p(dd), p(Wd), dx.ptr, M, H, Nout)
        return (dx.get(what),)
    R.check_close(twice(fwd, what)[0], R.linear(x, W, b), R.FWD, what + " fwd")
    R.check_close(twice(bwd, what)[0], R.head_linear_bwd_dx(dout, W), R.GRAD, what + " dx")


# ----------------------------------------------------------------------------------------------------- |x| maximum
ABSMAX_BIG = 256 * 8 * 1024 + 5      # 1024 blocks x 256 threads walk it: eight full trips and a ninth of five elements


def run_absmax(pkg, x, start=0.0):
    xd = dev_in(x, tail=64)
    target = Vec(1, fill=7.0)
    target.v.fill_(start)
    target.before = target.big.clone()
    call(pkg, "e3d_absmax_f32", p(xd), x.numel(), target.ptr)
    return target.get("absmax").cpu().reshape(())


@pytest.mark.parametrize("n", [1, 3, 2049, ABSMAX_BIG])
def test_absmax_sizes_and_positions(pkg, hip, n):
    base = torch.randn(n, generator=R.gen(n, 41))
    positions = sorted({0, n - 1, n // 2, min(n - 1, 1024 * 256 + 77)})     # the last one: beyond gridDim x 256
    for pos in positions:
        for extreme in (-9.5, 9.25):       # a negative extreme too
            x = base.clone()
            x[pos] = extreme
            got = run_absmax(pkg, x)
            assert float(got) == abs(extreme) and torch.equal(bits(got), bits(R.absmax(x))), (n, pos, extreme, float(got))
    assert float(run_absmax(pkg, base)) == float(base.abs().max())


def test_absmax_special_values(pkg, hip):
    n = 2049
    base = torch.randn(n, generator=R.gen(n, 42))
    zeros = torch.full((n,), -0.0)
    assert int(bits(run_absmax(pkg, zeros))) == 0                                   # all -0.0: +0.0
    den = zeros.clone()
    den[n - 1] = -1e-40                                                             # a denormal maximum
    assert torch.equal(bits(run_absmax(pkg, den)), bits(torch.tensor(1e-40))) and float(torch.tensor(1e-40)) > 0
    assert float(run_absmax(pkg, base, start=100.0)) == 100.0                       # a target above the data stays
    assert float(run_absmax(pkg, base, start=0.5)) == float(base.abs().max())      # one below it is raised
    for v in (float("inf"), float("-inf")):
        for pos in (0, n - 1):
            x = base.clone()
            x[pos] = v
            assert float(run_absmax(pkg, x)) == float("inf")
    for pos in (0, 1000, n - 1):                                                    # a NaN anywhere: NaN, also next to inf
        x = base.clone()
        x[5] = float("inf")
        x[pos] = NAN
        assert torch.isnan(run_absmax(pkg, x))
    big = torch.zeros(ABSMAX_BIG)
    big[ABSMAX_BIG - 1] = NAN
    assert torch.isnan(run_absmax(pkg, big))


# ----------------------------------------------------------------------------------------------------- LayerNorm backward
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("H,M", R.LN_BWD_CASES)
def test_layernorm_bwd(pkg, hip, H, M, affine):
    """Through autograd.layernorm_bwd (the workspace form): rows 1, 2, 3 leave waves without rows, an odd count leaves
    the second row of a trip missing.  want_affine_grads=False asks for no workspace and launches no column sum."""
    dy, s, gamma = R.ln_bwd_inputs(H, M)
    dyd, sd, gd = dev_in(dy), dev_in(s), dev_in(gamma)
    what = f"layernorm_bwd H={H} M={M} affine={affine}"
    got = twice(lambda: tuple(t for t in pkg.autograd.layernorm_bwd(dyd, sd, gd, 1e-12, want_affine_grads=affine) if t is not None),
                what)
    ref = R.layernorm_bwd(dy, s, gamma, 1e-12)
    assert len(got) == (3 if affine else 1)
    for name, a, b in zip(("ds", "dgamma", "dbeta"), got, ref):
        R.check_close(a, b, R.GRAD, f"{what} {name}")


@pytest.mark.parametrize("H,M", [(256, 3), (768, 17)])
def test_layernorm_bwd_without_gamma(pkg, hip, H, M):
    dy, s, _ = R.ln_bwd_inputs(H, M)
    dyd, sd = dev_in(dy), dev_in(s)
    n_ws = hip.e3d_layernorm_bwd_workspace_floats(M, H)
    assert n_ws == ((M + 15) // 16) * 2 * H
    what = f"layernorm_bwd_ws gamma=None H={H} M={M}"

    def run():
        ds, both, ws = Out(M, H), Out(2, H), Vec(n_ws)
        call(pkg, "e3d_layernorm_bwd_ws", p(dyd), p(sd), None, 1e-12, ds.ptr, None, both.row(0), both.row(1), M, H, 0.0, 0,
             ws.ptr, n_ws)
        assert ws.guards_intact(), f"{what}: a write outside the workspace"
        return ds.get(what), both.get(what)
    ds, both = twice(run, what)
    ref = R.layernorm_bwd(dy, s, None, 1e-12)
    R.check_close(ds, ref[0], R.GRAD, what + " ds")
    R.check_close(both[0], ref[1], R.GRAD, what + " dgamma")
    R.check_close(both[1], ref[2], R.GRAD, what + " dbeta")
    # no affine gradients wanted: no workspace needed; dgamma alone wanted: dbeta's place stays as it was
    ds2, alone = Out(M, H), Vec(H)
    call(pkg, "e3d_layernorm_bwd_ws", p(dyd), p(sd), None, 1e-12, ds2.ptr, None, None, None, M, H, 0.0, 0, None, 0)
    assert torch.equal(bits(ds2.get(what)), bits(ds))
    ws = Vec(n_ws)
    call(pkg, "e3d_layernorm_bwd_ws", p(dyd), p(sd), None, 1e-12, ds2.ptr, None, alone.ptr, None, M, H, 0.0, 0, ws.ptr, n_ws)
    assert torch.equal(bits(alone.get(what)), bits(both[0])) and ws.guards_intact()


@pytest.mark.parametrize("layout", ["adjacent", "separate"])
def test_layernorm_bwd_atomics_form(pkg, hip, layout):
    """The exported atomics form at M = 33 (three blocks add into dgamma / dbeta): dbeta == dgamma + H takes the single
    zero-fill, two buffers the separate ones; what the buffers held before must not survive either way."""
    H, M = R.LN_BWD_ATOMIC_CASE
    dy, s, gamma = R.ln_bwd_inputs(H, M)
    ds = Out(M, H)
    if layout == "adjacent":
        both = Out(2, H)
        dg_ptr, db_ptr = both.row(0), both.row(1)
        assert db_ptr == dg_ptr + 4 * H
    else:
        dg, db = Vec(H), Vec(H)
        dg_ptr, db_ptr = dg.ptr, db.ptr
        assert db_ptr != dg_ptr + 4 * H
    dyd, sd, gd = dev_in(dy), dev_in(s), dev_in(gamma)
    call(pkg, "e3d_layernorm_bwd", p(dyd), p(sd), p(gd), 1e-12, ds.ptr, dg_ptr, db_ptr, M, H)
    what = f"layernorm_bwd (atomics, {layout})"
    got_g, got_b = (both.get(what)[0], both.get(what)[1]) if layout == "adjacent" else (dg.get(what), db.get(what))
    ref = R.layernorm_bwd(dy, s, gamma, 1e-12)
    R.check_close(ds.get(what), ref[0], R.GRAD, what + " ds")
    R.check_close(got_g, ref[1], R.GRAD, what + " dgamma")
    R.check_close(got_b, ref[2], R.GRAD, what + " dbeta")


@pytest.mark.parametrize("kind", ["seeded", "keyed"])
def test_layernorm_bwd_drop_atomics_forms(pkg, hip, kind):
    """The atomics entry points with the forward's dropout folded in, against the workspace form of the same decisions
    (itself held to fp64 by the dropout tests): ds and ds_dropped the same bits, dgamma / dbeta within the bound."""
    H, M = R.LN_BWD_ATOMIC_CASE
    dy, s, gamma = R.ln_bwd_inputs(H, M)
    dyd, sd, gd = dev_in(dy), dev_in(s), dev_in(gamma)
    if kind == "keyed":
        keys = torch.randint(-2 ** 62, 2 ** 62, (M,), generator=R.gen(51), dtype=torch.int64).to(DEV)
        drop, tail, name = (0.25, 7, keys), (0.25, 7, p(keys)), "e3d_layernorm_bwd_drop_keyed"
    else:
        drop, tail, name = (0.25, 1234), (0.25, 1234), "e3d_layernorm_bwd_drop"
    ref_ds, ref_dg, ref_db, ref_dsd = pkg.autograd.layernorm_bwd(dyd, sd, gd, 1e-12, drop=drop)
    ds, dsd, both = Out(M, H), Out(M, H), Out(2, H)
    call(pkg, name, p(dyd), p(sd), p(gd), 1e-12, ds.ptr, dsd.ptr, both.row(0), both.row(1), M, H, *tail)
    what = f"layernorm_bwd_drop ({kind})"
    assert torch.equal(bits(ds.get(what)), bits(ref_ds)) and torch.equal(bits(dsd.get(what)), bits(ref_dsd))
    frac = float((ref_dsd == 0).float().mean())
    assert 0.2 < frac < 0.3, frac
    R.check_close(both.get(what)[0], ref_dg.double(), R.GRAD, what + " dgamma")
    R.check_close(both.get(what)[1], ref_db.double(), R.GRAD, what + " dbeta")
    R.check_close(ref_dg, R.layernorm_bwd(dy, s, gamma, 1e-12)[1], R.GRAD, what + " dgamma (workspace form)")


# ----------------------------------------------------------------------------------------------------- activations
def run_act(pkg, z, kind, dh=1.0):
    n = z.numel()
    zd = dev_in(z, tail=64)
    dhd = dev_in(torch.full((n,), dh), tail=64)

    def run():
        out, dz = Vec(n), Vec(n)
        call(pkg, "e3d_act_fwd", p(zd), kind, out.ptr, n)
        call(pkg, "e3d_act_bwd", p(dhd), p(zd), kind, dz.ptr, n)
        return out.get("act_fwd").cpu(), dz.get("act_bwd").cpu()
    return twice(run, f"act {kind} n={n}")


def act_figures(got, dgot, z, kind):
    """(forward figure, derivative figure) as the module docstring defines them."""
    fwd = R.gelu_error(got, z) if kind == 1 else float((got.double() - R.act(z, kind)).abs().max())
    return fwd, float((dgot.double() - R.act_grad(z, kind)).abs().max())


def check_act(got, dgot, z, kind, what):
    assert torch.isfinite(got).all() and torch.isfinite(dgot).all(), f"{what}: a finite z gave a non-finite result"
    fwd, bwd = act_figures(got, dgot, z, kind)
    print(f"{what}: forward {fwd:.3e}, derivative {bwd:.3e}")
    if kind == 0:
        assert torch.equal(bits(got), bits(z)) and bool((dgot == 1).all())
        return
    assert fwd <= (GELU_FWD_BOUND if kind == 1 else ACT_ABS_BOUND[("fwd", 2)]), f"{what}: forward error {fwd:.3e}"
    assert bwd <= ACT_ABS_BOUND[("bwd", kind)], f"{what}: derivative error {bwd:.3e}"


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_act_grid(pkg, hip, kind):
    z = R.act_grid()
    got, dgot = run_act(pkg, z, kind)
    check_act(got, dgot, z, kind, f"act {kind} over the grid")
    if kind:
        at = {float(v): i for i, v in enumerate(z.tolist())}
        i = at[-100.0]
        assert abs(float(got[i])) <= 1e-30 and abs(float(dgot[i])) <= 1e-30, (float(got[i]), float(dgot[i]))
        assert float(got[at[1e4]]) == 1e4 and float(dgot[at[1e4]]) == 1.0
    # dh scales the derivative: a power of two scales it exactly
    got2, dgot2 = run_act(pkg, z, kind, dh=-2.0)
    assert torch.equal(bits(got2), bits(got)) and torch.equal(bits(dgot2), bits(-2.0 * dgot))


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_act_sizes(pkg, hip, kind):
    grid = R.act_grid()
    full, dfull = run_act(pkg, grid, kind)
    for n in (1, 1000, R.ACT_BIG_N):
        # n = 1: z = -0.75; n = 1000: the special values and every fourth grid point; the largest: the grid, tiled
        z = grid[1875:1876] if n == 1 else (torch.cat([grid[4001:], grid[:4001:4]])[:n] if n == 1000
                                           else grid.repeat(n // grid.numel() + 1)[:n])
        assert z.numel() == n
        got, dgot = run_act(pkg, z, kind)
        check_act(got, dgot, z, kind, f"act {kind} n={n}")
        if n == R.ACT_BIG_N:      # the same value gives the same result wherever it sits (the last 3 are the second trip)
            m = grid.numel()
            assert torch.equal(bits(got[-m:]), bits(full.repeat(3)[(n - m) % m:(n - m) % m + m]))
            assert torch.equal(bits(dgot[-m:]), bits(dfull.repeat(3)[(n - m) % m:(n - m) % m + m]))


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_act_nan_in_nan_out(pkg, hip, kind):
    z = torch.tensor([1.0, NAN, -2.0, NAN])
    got, dgot = run_act(pkg, z, kind)
    assert got.isnan().tolist() == [False, True, False, True]
    assert dgot.isnan().tolist() == ([False] * 4 if kind == 0 else [False, True, False, True])


# ----------------------------------------------------------------------------------------------------- reductions
@pytest.mark.parametrize("M,N,ld", R.COLSUM_CASES)
def test_colsum(pkg, hip, M, N, ld):
    x = R.colsum_input(M, N)
    xd = strided_in(x, ld)
    out = Vec(N)          # holds the sentinel: stale contents must not survive
    call(pkg, "e3d_colsum", p(xd), ld, out.ptr, M, N)
    R.check_close(out.get("colsum"), R.colsum(x), R.GRAD, f"colsum M={M} N={N} ld={ld}")


@pytest.mark.parametrize("rpg,groups,H", R.GROUP_SUM_CASES)
def test_group_sum(pkg, hip, rpg, groups, H):
    x = R.group_sum_input(rpg, groups, H)
    xd = dev_in(x)
    what = f"group_sum {rpg} x {groups} x {H}"

    def run():
        out = Out(groups, H)
        call(pkg, "e3d_group_sum", p(xd), rpg, out.ptr, rpg * groups, H)
        return (out.get(what),)
    R.check_close(twice(run, what)[0], R.group_sum(x, rpg), R.GRAD, what)


def run_wgrad(pkg, case):
    H, off, M, F, tr, with_db = case
    g, x = R.wgrad_inputs(H, M, F)
    gd, xd = dev_in(g, off), dev_in(x)
    assert gd.data_ptr() % 16 == 4 * off
    dW, db = (Out(F, H) if tr else Out(H, F)), Vec(H)
    call(pkg, "e3d_small_k_wgrad", p(gd), p(xd), dW.ptr, db.ptr if with_db else None, M, H, F, tr)
    what = f"small_k_wgrad {case}"
    if not with_db:
        assert db.untouched(), f"{what}: db is null, yet its neighbourhood was written"
    return dW.get(what), (db.get(what) if with_db else None)


@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=lambda c: "-".join(map(str, c)))
def test_small_k_wgrad(pkg, hip, case):
    H, off, M, F, tr, with_db = case
    dW, db = run_wgrad(pkg, case)
    ref_dW, ref_db = R.small_k_wgrad(*R.wgrad_inputs(H, M, F), tr)
    R.check_close(dW, ref_dW, R.GRAD, f"small_k_wgrad {case} dW")
    if with_db:
        R.check_close(db, ref_db, R.GRAD, f"small_k_wgrad {case} db")


@pytest.mark.parametrize("pair", R.WGRAD_PAIRS, ids=lambda c: "-".join(map(str, c[0])))
def test_small_k_wgrad_kernels_agree(pkg, hip, pair):
    """The float4 kernel and the fallback on the same data (atomics: within the bound, not bit-equal)."""
    a, b = pair
    dWa, dba = run_wgrad(pkg, a)
    dWb, dbb = run_wgrad(pkg, b)
    R.check_close(dWb if a[4] == b[4] else dWb.t(), dWa.double(), R.GRAD, f"small_k_wgrad {a} against {b}")
    if dba is not None and dbb is not None:
        R.check_close(dbb, dba.double(), R.GRAD, f"small_k_wgrad db {a} against {b}")


@pytest.mark.parametrize("count,rows,cols", R.TRANSPOSE_CASES)
def test_transpose_grouped(pkg, hip, count, rows, cols):
    ld_src, ld_dst = cols + 5, rows + 3
    srcs = [torch.randn(rows, cols, generator=R.gen(count, rows, cols, i)) for i in range(count)]
    srcs_d = [strided_in(s, ld_src) for s in srcs]
    what = f"transpose_grouped {count} x {rows} x {cols}"

    def run():
        dsts = [Out(cols, rows, ld=ld_dst) for _ in range(count)]
        a_src = (ctypes.c_void_p * count)(*[s.data_ptr() for s in srcs_d])
        a_dst = (ctypes.c_void_p * count)(*[d.ptr for d in dsts])
        call(pkg, "e3d_transpose_grouped_f32", a_src, a_dst, count, rows, cols, ld_src, ld_dst)
        return tuple(d.get(what) for d in dsts)
    for got, src in zip(twice(run, what), srcs):
        assert torch.equal(bits(got.cpu()), bits(src.t())), what


# ----------------------------------------------------------------------------------------------------- argument checks
def test_bad_arguments_are_refused_before_any_launch(pkg, hip):
    """One per launcher family: a non-zero status, a message, and outputs bit-untouched."""
    x = dev_in(torch.randn(8, 1024, generator=R.gen(61)))
    v = dev_in(torch.randn(1024, generator=R.gen(62)))
    small = dev_in(torch.randn(8, 33, generator=R.gen(63)))
    out, out2 = Out(8, 1024), Out(8, 1024)
    ptrs = (ctypes.c_void_p * 65)(*[p(x)] * 65)
    dsts = (ctypes.c_void_p * 65)(*[out.ptr] * 65)
    cases = [
        ("e3d_residual_layernorm_fwd", (p(x), None, p(v), p(v), 1e-12, out2.ptr, out.ptr, 4, 300), "H"),             # H = 300
        ("e3d_embed_layernorm_fwd", (p(small), 33, p(x), p(v), p(v), p(v), 1e-12, None, 0, out2.ptr, out.ptr, 8, 256), "F"),
        ("e3d_head_linear_fwd", (p(x), p(x), p(v), out.ptr, 1, 256, 33), "Nout"),                                    # Nout = 33
        ("e3d_head_linear_bwd_dx", (p(small), p(x), out.ptr, 1, 256, 33), ""),
        ("e3d_adaln_gate_fwd", (p(x), p(x), p(x), 0, 1, out.ptr, 0, 256), ""),                                        # M = 0
        ("e3d_adaln_gate_bwd", (p(x), p(x), p(x), 0, 1, out.ptr, out2.ptr, 0, 256), ""),
        ("e3d_act_fwd", (p(x), 3, out.ptr, 8), ""),                                                                   # act = 3
        ("e3d_transpose_grouped_f32", (ptrs, dsts, 65, 8, 8, 1024, 1024), "count"),                                   # count = 65
        ("e3d_colsum", (p(x), 7, out.ptr, 8, 8), ""),                                                                 # ld < N
        ("e3d_group_sum", (p(x), 3, out.ptr, 8, 1024), "rows_per_group"),                                             # M % rpg
        ("e3d_small_k_wgrad", (p(x), p(small), out.ptr, out2.ptr, 8, 1024, 33, 0), "F"),                              # F = 33
        ("e3d_absmax_f32", (p(x), 0, out.ptr), ""),                                                                   # n = 0
    ]
    for name, args, word in cases:
        rc = getattr(hip, name)(*args, _s())
        torch.cuda.synchronize()
        msg = hip.e3d_last_error().decode(errors="replace")
        assert rc != 0 and msg and word in msg, (name, rc, msg)
        assert out.untouched() and out2.untouched(), f"{name}: refused, yet an output was written"
