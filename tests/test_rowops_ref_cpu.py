"""tests/rowops_ref.py checked without a GPU.

1. Every closed form against torch's own operators and torch.autograd in float64, on the smallest instances of the shapes:
   a wrong reference cannot then pass a wrong kernel.
2. Input conditioning: for every input generator and case list of tests/test_rowops_forms_gpu.py, the SAME statement
   evaluated by torch in float32 on the CPU lies within the bound the GPU test asserts (whole tensor and per row).  An
   input that fails here is too ill-conditioned for any fp32 kernel; the input is changed, not the bound.  Rows of
   constant value (variance 0 under eps = 1e-12) are asserted finite only.
"""
import pytest
import torch
import torch.nn.functional as F

import rowops_ref as R

F32, F64 = torch.float32, torch.float64


def close64(a, b, what):
    scale = float(b.abs().max()) or 1.0
    assert float((a - b).abs().max()) <= 1e-12 * scale, what


def leaf(t):
    return t.double().clone().requires_grad_(True)


# ----------------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("H,M", [(256, 1), (256, 3)])
def test_layernorm_forms_match_autograd(H, M):
    dy, s, gamma = R.ln_bwd_inputs(H, M)
    beta = R.affine(H, 13)[1]
    s_, g_, b_ = leaf(s), leaf(gamma), leaf(beta)
    out = F.layer_norm(s_, (H,), g_, b_, 1e-12)
    close64(R.layernorm(s, gamma, beta, 1e-12), out.detach(), "layernorm")
    out.backward(dy.double())
    ds, dg, db = R.layernorm_bwd(dy, s, gamma, 1e-12)
    close64(ds, s_.grad, "ds"), close64(dg, g_.grad, "dgamma"), close64(db, b_.grad, "dbeta")
    s2 = leaf(s)      # gamma = None
    F.layer_norm(s2, (H,), None, None, 1e-12).backward(dy.double())
    close64(R.layernorm_bwd(dy, s, None, 1e-12)[0], s2.grad, "ds without gamma")
    x, res, ga, be = R.residual_ln_inputs(H, M, "shifted")
    close64(R.residual_layernorm(x, res, ga, be, 1e-12), F.layer_norm(x.double() + res.double(), (H,), ga.double(), be.double(), 1e-12),
            "residual_layernorm")


@pytest.mark.parametrize("M,rpc", [(5, 1), (5, 5), (32, 16)])
@pytest.mark.parametrize("branch", [0, 1])
def test_adaln_gate_forms_match_autograd(M, rpc, branch):
    H = 256
    x, y, mod, dout = R.adaln_inputs(H, M, rpc)
    y_, m_ = leaf(y), leaf(mod)
    sh, sc, ga = [m_[:, (3 * branch + i) * H:(3 * branch + i + 1) * H].repeat_interleave(rpc, 0) for i in range(3)]
    out = x.double() + ga * (F.layer_norm(y_, (H,), eps=1e-5) * (1 + sc) + sh)
    close64(R.adaln_gate(x, y, mod, branch, rpc), out.detach(), "adaln_gate")
    close64(R.adaln_gate(x, y, R.hide_other_branch(mod, branch, H), branch, rpc), out.detach(), "adaln_gate, other branch NaN")
    out.backward(dout.double())
    dy, dmod = R.adaln_gate_bwd(dout, y, mod, branch, rpc)
    close64(dy, y_.grad, "dy"), close64(dmod, m_.grad, "dmod")
    other = dmod[:, 3 * (1 - branch) * H:3 * (2 - branch) * H]
    assert (other == 0).all()


def test_adaln_gate_indexed_form():
    H, M = 256, len(R.ADALN_IDX)
    x, y, mod, _ = R.adaln_inputs(H, M, 1)
    table = torch.randn(R.ADALN_TABLE_ROWS, 6 * H, generator=R.gen(H, 31))
    idx = torch.tensor(R.ADALN_IDX)
    got = R.adaln_gate_indexed(x, y, idx, table, mod, 1)
    for r, i in enumerate(R.ADALN_IDX):
        row = table[i] if 0 <= i < R.ADALN_TABLE_ROWS else mod[r]
        close64(got[r:r + 1], R.adaln_gate(x[r:r + 1], y[r:r + 1], row[None], 1, 1), f"row {r}")
    assert [0 <= i < R.ADALN_TABLE_ROWS for i in R.ADALN_IDX] == [False, True, True, False, False, True, True]


def test_linear_forms_match_autograd():
    H, Nout, M = 256, 8, 5
    x, W, b, dout = R.head_inputs(H, Nout, M)
    x_, W_, b_ = leaf(x), leaf(W), leaf(b)
    out = F.linear(x_, W_, b_)
    close64(R.linear(x, W, b), out.detach(), "head_linear")
    out.backward(dout.double())
    close64(R.head_linear_bwd_dx(dout, W), x_.grad, "dx")
    dW, db = R.small_k_wgrad(dout, x)          # dW = g^T x with g = dout [M, Nout], x [M, H]
    close64(dW, W_.grad, "dW"), close64(db, b_.grad, "db")
    close64(R.small_k_wgrad(dout, x, True)[0], W_.grad.t(), "dW^T")
    M, Fin, H = 5, 3, 256
    x, W, b, ga, be, add = R.embed_inputs(M, Fin, H, 3)
    z, out = R.embed_layernorm(x, W, b, ga, be, 1e-12, add, 3)
    zr = F.linear(x.double(), W.double(), b.double())
    close64(z, zr, "embed z")
    close64(out, F.layer_norm(zr, (H,), ga.double(), be.double(), 1e-12) + add.double()[[0, 0, 0, 1, 1]], "embed out")


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_activation_forms_match_autograd(kind):
    z = R.act_grid()
    z = z[(z.abs() <= 20)]
    z_ = leaf(z)
    out = (z_, F.gelu(z_), F.silu(z_))[kind] * 1.0
    # torch's fp64 GELU is 0.5 z (1 + erf): absolute agreement (it cancels on the far negative side, the erfc form does not)
    assert float((R.act(z, kind) - out.detach()).abs().max()) <= 1e-14
    out.sum().backward()
    assert float((R.act_grad(z, kind) - z_.grad).abs().max()) <= 1e-14
    far = torch.tensor([-100.0, -50.0, 50.0, 100.0, 1e4], dtype=F64)
    assert torch.isfinite(R.act(far, kind)).all() and torch.isfinite(R.act_grad(far, kind)).all()
    if kind:
        assert abs(float(R.act(far, kind)[0])) <= 1e-30 and abs(float(R.act_grad(far, kind)[0])) <= 1e-30
        assert float(R.act(far, kind)[-1]) == 1e4 and float(R.act_grad(far, kind)[-1]) == 1.0


def test_reduction_forms():
    x = R.colsum_input(17, 8)
    close64(R.colsum(x), x.double().t() @ torch.ones(17, dtype=F64), "colsum")
    x = R.group_sum_input(7, 4, 100)
    ref = torch.stack([x[7 * g:7 * g + 7].double().sum(0) for g in range(4)])
    close64(R.group_sum(x, 7), ref, "group_sum")
    v = torch.tensor([1.0, -3.0, 2.0])
    assert float(R.absmax(v)) == 3.0
    assert float(R.absmax(torch.tensor([-0.0, -0.0]))) == 0.0 and R.absmax(torch.tensor([-0.0])).view(torch.int32) == 0
    assert float(R.absmax(torch.tensor([1.0, float("-inf")]))) == float("inf")
    assert torch.isnan(R.absmax(torch.tensor([float("inf"), float("nan"), 1.0])))
    assert float(R.absmax(torch.tensor([0.0, -1e-40]))) == float(torch.tensor(1e-40))


# ----------------------------------------------------------------------------------------------------- conditioning
def within(got32, ref64, tol, what):
    whole, row = R.check_close(got32, ref64, tol, what)
    print(f"{what}: fp32 torch {whole:.2e} of {tol:g}, worst row {row:.2e} of {4 * tol:g}")


@pytest.mark.parametrize("H,M,kind", R.RESIDUAL_LN_CASES)
def test_conditioning_residual_layernorm(H, M, kind):
    x, res, ga, be = R.residual_ln_inputs(H, M, kind)
    for r in (res, None):
        within(R.residual_layernorm(x, r, ga, be, 1e-12, F32), R.residual_layernorm(x, r, ga, be, 1e-12), R.FWD, f"ln {H} {M} {kind}")


@pytest.mark.parametrize("H", R.HS)
def test_conditioning_constant_rows_finite_only(H):
    ga, be = R.affine(H, 5)
    assert torch.isfinite(R.residual_layernorm(R.constant_rows(H), None, ga, be, 1e-12, F32)).all()
    assert torch.isfinite(R.residual_layernorm(R.constant_rows(H), None, ga, be, 1e-12)).all()


@pytest.mark.parametrize("H,M,rpc,br", R.ADALN_FWD_CASES)
def test_conditioning_adaln_gate_fwd(H, M, rpc, br):
    x, y, mod, _ = R.adaln_inputs(H, M, rpc)
    within(R.adaln_gate(x, y, mod, br, rpc, F32), R.adaln_gate(x, y, mod, br, rpc), R.FWD, "adaln_gate")


@pytest.mark.parametrize("H,M,rpc,br", R.ADALN_BWD_CASES)
def test_conditioning_adaln_gate_bwd(H, M, rpc, br):
    x, y, mod, dout = R.adaln_inputs(H, M, rpc)
    for name, a, b in zip(("dy", "dmod"), R.adaln_gate_bwd(dout, y, mod, br, rpc, F32), R.adaln_gate_bwd(dout, y, mod, br, rpc)):
        within(a, b, R.GRAD, name)


@pytest.mark.parametrize("M,Fin,H,rpa", R.EMBED_FEW_CASES + R.EMBED_STAGED_CASES)
def test_conditioning_embed_layernorm(M, Fin, H, rpa):
    x, W, b, ga, be, add = R.embed_inputs(M, Fin, H, rpa)
    got, ref = R.embed_layernorm(x, W, b, ga, be, 1e-12, add, rpa or 1, F32), R.embed_layernorm(x, W, b, ga, be, 1e-12, add, rpa or 1)
    within(got[0], ref[0], R.FWD, "embed z"), within(got[1], ref[1], R.FWD, "embed out")


def test_embed_inputs_share_their_first_rows():
    a, b = R.embed_inputs(513, 3, 768, 3), R.embed_inputs(512, 3, 768, 3)
    assert torch.equal(a[0][:512], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[5][:171], b[5])
    assert a[5].shape[0] == 171 and R.embed_inputs(515, 3, 768, 3)[5].shape[0] == 172


@pytest.mark.parametrize("H,Nout,M", R.HEAD_CASES)
def test_conditioning_head_linear(H, Nout, M):
    x, W, b, dout = R.head_inputs(H, Nout, M)
    within(R.linear(x, W, b, F32), R.linear(x, W, b), R.FWD, "head fwd")
    within(R.head_linear_bwd_dx(dout, W, F32), R.head_linear_bwd_dx(dout, W), R.GRAD, "head dx")


@pytest.mark.parametrize("H,M", R.LN_BWD_CASES + [R.LN_BWD_ATOMIC_CASE])
def test_conditioning_layernorm_bwd(H, M):
    dy, s, gamma = R.ln_bwd_inputs(H, M)
    for g in (gamma, None):
        for name, a, b in zip(("ds", "dgamma", "dbeta"), R.layernorm_bwd(dy, s, g, 1e-12, F32), R.layernorm_bwd(dy, s, g, 1e-12)):
            within(a, b, R.GRAD, name)


@pytest.mark.parametrize("H,off,M,Fin,tr,with_db", R.WGRAD_CASES)
def test_conditioning_small_k_wgrad(H, off, M, Fin, tr, with_db):
    g, x = R.wgrad_inputs(H, M, Fin)
    for name, a, b in zip(("dW", "db"), R.small_k_wgrad(g, x, tr, F32), R.small_k_wgrad(g, x, tr)):
        within(a, b, R.GRAD, f"{name} M={M}")


def test_wgrad_pairs_share_their_data():
    for a, b in R.WGRAD_PAIRS:
        assert a in R.WGRAD_CASES and b in R.WGRAD_CASES and (a[0], a[2], a[3]) == (b[0], b[2], b[3]) and a[1] != b[1]


@pytest.mark.parametrize("M,N,ld", R.COLSUM_CASES)
def test_conditioning_colsum(M, N, ld):
    x = R.colsum_input(M, N)
    within(R.colsum(x, F32), R.colsum(x), R.GRAD, f"colsum M={M}")


@pytest.mark.parametrize("rpg,groups,H", R.GROUP_SUM_CASES)
def test_conditioning_group_sum(rpg, groups, H):
    x = R.group_sum_input(rpg, groups, H)
    within(R.group_sum(x, rpg, F32), R.group_sum(x, rpg), R.GRAD, "group_sum")


@pytest.mark.parametrize("kind", [1, 2])
def test_conditioning_activations(kind):
    """torch's fp32 evaluation stays within the CAPS the GPU test may not exceed (its asserted bounds are measured ones)."""
    z = R.act_grid()
    got = (F.gelu(z) if kind == 1 else F.silu(z))
    if kind == 1:
        assert R.gelu_error(got, z) <= 5e-7
    else:
        assert float((got.double() - R.act(z, 2)).abs().max()) <= 2e-6
    assert float((R.act_grad(z, kind, F32).double() - R.act_grad(z, kind)).abs().max()) <= 2e-6
    assert torch.isfinite(R.act(z, kind)).all() and torch.isfinite(R.act_grad(z, kind)).all()
