"""Every diffusion-process kernel of csrc/sampler.hip at every launcher branch, through the C ABI, against the float64
statements and the exact fp32 rules of tests/sampler_ref.py (which tests/test_sampler_ref_cpu.py holds to the oracle, and
whose inputs it examines).  The branches are forced by operand properties only: n against 4 and against the 2048-block
grid cap, L against the 256 threads of a block, C against the 32 classes the LDS arrays hold, null pointers, sigma == 0.

One row per ``hipLaunchKernelGGL`` site of csrc/sampler.hip, by entry point and the instantiation it launches:

=======================================  =======================================  ===========================================  ==========================================
entry point                              kernel                                   forced by                                    test id
=======================================  =======================================  ===========================================  ==========================================
e3d_ddpm_step_wrap                       ddpm_step_wrap_kernel<false>, scalars    n % 4, n < 4, n4 > 2048 * 256, noise NULL,   test_ddpm_update[*], test_ddpm_without_noise,
                                                                                  sigma == 0, out == x, a pointer at +4 bytes  test_ddpm_out_may_alias_x, test_wrap_pi_bit_exact,
                                                                                                                               test_ddpm_refuses_misaligned_pointers
e3d_ddpm_step_wrap_table                 ddpm_step_wrap_kernel<false>, table row  the same sizes                               test_ddpm_update[*], test_ddpm_out_may_alias_x,
                                                                                                                               test_ddpm_refuses_misaligned_pointers
e3d_strided_step_wrap                    strided_step_wrap_kernel<false>          --                                           test_strided_gpu.py::test_kernel_against_the_float64_ref
e3d_q_sample_wrap                        q_sample_wrap_kernel                     n against 2048 * 256, i / per                test_q_sample_wrap[*]
e3d_discrete_posterior_sample            discrete_posterior_kernel<false, false>  L against 256, C = 2 .. 32, tot == 0,        test_discrete_posterior[*],
                                                                                  prob_out NULL, both modes                    test_discrete_posterior_zero_total[*]
e3d_discrete_q_sample                    discrete_q_sample_kernel<false>          B L against 256, C, padding rows             test_discrete_q_sample[*]
e3d_keyed_ddpm_step_wrap                 ddpm_step_wrap_kernel<true>              F = 4 | 1024, n4 > 2048 * 256                test_keyed_ddpm_step[*]
e3d_keyed_strided_step_wrap              strided_step_wrap_kernel<true>           --                                           test_strided_gpu.py::test_keyed_form_equals_the_unkeyed_form_with_the_keyed_draws
e3d_keyed_discrete_posterior_sample      discrete_posterior_kernel<true, false>   L > 256, C = 32, rows of no item             test_keyed_discrete_posterior[*]
e3d_keyed_draws                          keyed_draws_kernel                       kind 0 .. 3, F, n > 2048 * 256, step 65535   test_keyed_draws[*]
e3d_keyed_timesteps                      keyed_timesteps_kernel                   B against 256, C = 1                         test_keyed_timesteps[*]
e3d_keyed_q_sample_wrap                  keyed_q_sample_wrap_kernel               F = 1024, n4 > 2048 * 256, t outside [0,T)   test_keyed_q_sample_wrap[*]
e3d_keyed_discrete_q_sample              discrete_q_sample_kernel<true>           B L = 257 | 900, ids above 2^63              test_discrete_q_sample[257-*|900-*]
e3d_known_compose_wrap                   known_compose_wrap_kernel<false>         --                                           test_known_gpu.py::test_compose_against_the_float64_ref
e3d_keyed_known_compose_wrap             known_compose_wrap_kernel<true>          --                                           test_known_gpu.py::test_keyed_compose_equals_the_buffer_form_with_the_keyed_draws
e3d_discrete_known_compose               discrete_known_compose_kernel<false>     --                                           test_known_gpu.py::test_discrete_compose_equals_q_sample_and_where
e3d_keyed_discrete_known_compose         discrete_known_compose_kernel<true>      --                                           test_known_gpu.py::test_discrete_compose_equals_q_sample_and_where
e3d_discrete_posterior_sample_ctl        discrete_posterior_kernel<false, true>   --                                           test_design_gpu.py::test_posterior_under_controls_against_float64
e3d_keyed_discrete_posterior_sample_ctl  discrete_posterior_kernel<true, true>    --                                           test_design_gpu.py::test_keyed_ctl_form_equals_the_buffer_ctl_form_with_the_keyed_uniforms
e3d_discrete_final_pick                  discrete_final_pick_kernel               --                                           test_design_gpu.py::test_final_pick
=======================================  =======================================  ===========================================  ==========================================

Conventions (those of tests/test_rowops_forms_gpu.py, whose plumbing this module uses).  Every output is a block in the
middle of a sentinel-filled allocation, 16 guard words on each side, 16-byte aligned where the kernel stores float4; the
guards must be bit-unchanged afterwards and the sentinel must not survive inside the output.  Float inputs carry NaN after
their last element; a NaN-filled ``noise`` is passed wherever the kernel must not read it.  No kernel here uses atomics:
every case runs twice and must be bit-identical.  No case passes an index outside a table or a class outside [0, C).

Bounds (u = 2^-24, the unit roundoff of fp32).
  * DDPM update  sra (x - beta e / s1m) + sigma z:  six fp32 roundings, each at most u of
    G = sra (|x| + |beta e / s1m|) + |sigma z|; |got - ref| <= 8 u G (two added for second order), on every element.  With
    ``wrap``: circular distance, plus 4 u (|v| + pi) for wrap_pi's two additions and the fp32 value of 2 pi.
  * q_sample_wrap  wrap(a x0 + s noise):  three roundings, 5 u G with G = |a x0| + |s noise|, plus 4 u (|v| + pi).
  * Discrete posterior, element by element.  Every term of every sum is non-negative, so relative errors add and none is
    amplified.  With D = max |logit - max logit| of the row:
      Qt[c][xt] = (Qsb / Qtb) / rowsum: the ratio 1, the C-term sum C - 1 on top of its terms' 1, the division 1 ->  C + 2
      pred[x0] = exp(l - mx) / se: the difference rounds to u D of the exponent's argument, hence u D of the
        exponential, expf itself 2 (it is good to an ulp); se adds C - 1 on top of that; the division 1          ->  2 D + C + 4
      w * ((Qt * Qsb) / den): three roundings; the sum over x0: C - 1                                            ->  C + 2
      so an unnormalised prob[c] carries (3 C + 8 + 2 D) u; tot: C - 1 more; prob / tot: 1 more                  ->  7 C + 16 + 4 D
    and |got - ref| <= (7 C + 20 + 4 D) u ref, four added for second order.  Each row sums to 1 within C u (tot's C - 1
    roundings and the division).  The project's older figure, max |got - ref| / max |ref| < 1e-5, is asserted as well.
  * The class pick, the wrap and the uniforms and classes of the keyed streams are exact: bit for bit.  Keyed normals:
    2e-6 max(1, |z|) against the float64 Box-Muller of tests/keyed_ref.py (the bound of test_keyed_sampling_gpu.py).

Measured on an MI355X, worst |got - ref| / bound over all cases of a test (each test prints its own):
  DDPM update, both forms          0.419 without wrap, 0.344 with; 0.301 with noise == NULL
  q_sample_wrap                    0.277  (3 x 174763; 0.075 / 0.184 / 0.245 at the smaller shapes)
  discrete posterior, elementwise  0.072  (4 x 37 x 3; 0.065 at C = 20, 0.037 at 1 x 600 x 32): the count is a worst case over
                                   70 to 250 roundings that a real row averages out.  Row sums: 6.5 u at C = 20 (bound 20),
                                   4.7 u at C = 32, 1.25 u at C = 3, 0.5 u at C = 2.
  keyed normals                    0.211  (2049 x 1024, with and without wrap; 0.148 at F = 4, 0.171 at F = 8)
  keyed_q_sample_wrap noise        9.1e-7 on the circle at 3 x 683 x 1024 (bound 2e-6); 4.0e-7 at 3 x 5 x 8
Everything else in this module is compared bit for bit.
"""
import numpy as np
import pytest
import torch

import keyed_ref as K
import sampler_ref as R
from helpers import rel_err
from test_rowops_forms_gpu import DEV, G, NAN, SENTINEL, Out, Vec, _s, bits, call, dev_in, p, twice
from test_sampler_ref_cpu import POSTERIOR_CASES, discrete_q_case, posterior_case

pytestmark = pytest.mark.gpu

U = R.U
ISENTINEL = -7777
BLOCKS = 2048 * 256                       # threads of the capped grid


# ----------------------------------------------------------------------------------------------------- plumbing
class IVec:
    """n integers in the middle of a sentinel-filled allocation, G guard words on each side."""

    def __init__(self, n, dtype=torch.int32):
        self.n = n
        self.big = torch.full((n + 2 * G,), ISENTINEL, dtype=dtype, device=DEV)
        self.v = self.big[G:G + n]
        self.before = self.big.clone()
        self.ptr = self.v.data_ptr()

    def get(self, what):
        same = self.big == self.before
        same[G:G + self.n] = True
        assert bool(same.all()), f"{what}: a write outside the output"
        assert not bool((self.v == ISENTINEL).any()), f"{what}: a row was not written"
        return self.v.clone()


def take(out, what):
    """The output of a float block: guards checked, and nothing of the sentinel left inside."""
    got = out.get(what)
    assert not bool((got == SENTINEL).any()), f"{what}: an element was not written"
    return got


def fvec(n):
    v = Vec(n)
    assert v.ptr % 16 == 0
    return v


def dev_f(a, offset=0):
    """A numpy float array on the device, NaN after its last element."""
    return dev_in(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)), offset, tail=64)


def dev_i(a, pad, dtype=torch.int32, n_pad=8):
    """A numpy integer array on the device, followed by ``n_pad`` elements of the (harmless) value ``pad``."""
    a = np.asarray(a)
    flat = torch.cat([torch.from_numpy(a.reshape(-1).astype(np.int64)), torch.full((n_pad,), pad, dtype=torch.int64)])
    return flat.to(dtype).to(DEV)[:a.size]


def dev_keys(keys):
    """A key table on the device, followed by rows of no item."""
    t = torch.cat([torch.from_numpy(keys), torch.tensor([[9, -1]] * 4, dtype=torch.int64)]).to(DEV)
    return t[:len(keys)]


def nan_buf(n):
    return torch.full((n + 64,), NAN, device=DEV)[:n]


def word(v):
    return torch.full((1,), v, dtype=torch.int64, device=DEV)


def np_(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def data(pkg, hip):
    """The DDPM inputs (smaller sizes are prefixes of the largest), each size with its own NaN tail, and the tables."""
    from e3diff_amd.structure_model.utils import CosineTables
    tab = CosineTables(1000)
    coef = torch.stack([tab.sqrt_recip_alphas, tab.betas, tab.sqrt_one_minus_alphas_cumprod, tab.sigma], dim=1).contiguous()
    assert coef.shape == (1000, 4) and coef.dtype == torch.float32
    x, e, z = R.ddpm_inputs()
    return {"x": x, "e": e, "z": z, "rows": coef.numpy(), "coef": dev_f(coef.numpy()),
            "dev": {n: tuple(dev_f(v[:n]) for v in (x, e, z)) for n in R.SIZES},
            "sa": tab.sqrt_alphas_cumprod.numpy(), "s1": tab.sqrt_one_minus_alphas_cumprod.numpy(),
            "sa_d": dev_f(tab.sqrt_alphas_cumprod.numpy()), "s1_d": dev_f(tab.sqrt_one_minus_alphas_cumprod.numpy())}


# ----------------------------------------------------------------------------------------------------- DDPM update
def ddpm_scalar(pkg, xd, ed, nd, row, wrap, n, what, out=None):
    o = fvec(n) if out is None else out
    call(pkg, "e3d_ddpm_step_wrap", p(xd), p(ed), p(nd), *(float(v) for v in row), int(wrap), o.ptr, n)
    return take(o, what)


def ddpm_table(pkg, xd, ed, nd, coef, t, wrap, n, what, out=None):
    o = fvec(n) if out is None else out
    call(pkg, "e3d_ddpm_step_wrap_table", p(xd), p(ed), p(nd), p(coef), p(word(t)), int(wrap), o.ptr, n)
    return take(o, what)


def check_ddpm(row, got, x, e, z, wrap, what):
    """Assert the bound of the module docstring on every element; returns the worst error / bound."""
    ref, parts = R.ddpm(row, x, e, z)                       # before the wrap
    got = got.astype(np.float64)
    bound = 8 * U * parts["G"]
    if wrap:
        err, bound = R.circ(got, ref), bound + 4 * U * (np.abs(ref) + np.pi)
        assert np.abs(got).max() <= np.pi + 1e-6, what
    else:
        err = np.abs(got - ref)
    ratio = float((err / bound).max())
    assert (err <= bound).all(), (what, "worst |got - ref| / bound", ratio)
    return ratio


@pytest.mark.parametrize("wrap", [False, True])
def test_ddpm_update(pkg, hip, data, wrap):
    """Scalar form against float64 from the same four fp32 coefficients; the table form bit-identical to it; at t = 0
    (sigma == 0) both bit-identical with a NaN-filled noise buffer."""
    worst = 0.0
    for t in R.TIMESTEPS:
        row = data["rows"][t]
        assert (row[3] == 0) == (t == 0)
        for n in R.SIZES:
            xd, ed, zd = data["dev"][n]
            what = f"ddpm t={t} n={n} wrap={wrap}"
            got = twice(lambda: (ddpm_scalar(pkg, xd, ed, zd, row, wrap, n, what),), what)[0]
            tab = twice(lambda: (ddpm_table(pkg, xd, ed, zd, data["coef"], t, wrap, n, what),), what)[0]
            assert same_bits(tab, got), f"{what}: the table form differs from the scalar form"
            worst = max(worst, check_ddpm(row, np_(got), data["x"][:n], data["e"][:n], data["z"][:n], wrap, what))
            if t == 0:
                poison = nan_buf(n)
                assert same_bits(ddpm_scalar(pkg, xd, ed, poison, row, wrap, n, what), got), f"{what}: noise was read"
                assert same_bits(ddpm_table(pkg, xd, ed, poison, data["coef"], t, wrap, n, what), got), f"{what}: noise was read"
    print(f"ddpm update wrap={wrap}: worst |got - ref| / bound = {worst:.3f}")


def test_ddpm_without_noise(pkg, hip, data):
    """noise == NULL with sigma != 0: the mean, the bits of the sigma == 0 call."""
    worst = 0.0
    for t in (999, 500):
        row = data["rows"][t]
        mean_row = (row[0], row[1], row[2], 0.0)
        for n in R.SIZES:
            xd, ed, _ = data["dev"][n]
            what = f"ddpm noise=NULL t={t} n={n}"
            got = twice(lambda: (ddpm_scalar(pkg, xd, ed, None, row, True, n, what),), what)[0]
            assert same_bits(got, ddpm_scalar(pkg, xd, ed, nan_buf(n), mean_row, True, n, what))
            worst = max(worst, check_ddpm(row, np_(got), data["x"][:n], data["e"][:n], None, True, what))
    print(f"ddpm without noise: worst |got - ref| / bound = {worst:.3f}")


def test_ddpm_out_may_alias_x(pkg, hip, data):
    for n in (5, R.N_BIG):
        xd, ed, zd = data["dev"][n]
        row = data["rows"][500]
        for form in ("scalar", "table"):
            what = f"ddpm out == x, {form}, n={n}"
            run = ((lambda x, o: ddpm_scalar(pkg, x, ed, zd, row, True, n, what, o)) if form == "scalar" else
                   (lambda x, o: ddpm_table(pkg, x, ed, zd, data["coef"], 500, True, n, what, o)))
            want = run(xd, None)
            o = fvec(n)
            o.v.copy_(xd.reshape(n, 1))
            o.before = o.big.clone()
            assert same_bits(run(o.v, o), want), what


def test_ddpm_refuses_misaligned_pointers(pkg, hip, data):
    n = 8 * 37
    x, e, z = data["x"][:n], data["e"][:n], data["z"][:n]
    row = [float(v) for v in data["rows"][500]]
    t = word(500)
    for which in range(4):
        xd, ed, zd = (dev_f(v, offset=int(which == i)) for i, v in enumerate((x, e, z)))
        out = fvec(n + 4)
        optr = out.ptr + (4 if which == 3 else 0)
        assert [xd.data_ptr() % 16, ed.data_ptr() % 16, zd.data_ptr() % 16, optr % 16][which] == 4
        for name, args in (("e3d_ddpm_step_wrap", (p(xd), p(ed), p(zd), *row, 1, optr, n)),
                           ("e3d_ddpm_step_wrap_table", (p(xd), p(ed), p(zd), p(data["coef"]), p(t), 1, optr, n))):
            rc = getattr(hip, name)(*args, _s())
            torch.cuda.synchronize()
            msg = hip.e3d_last_error().decode(errors="replace")
            assert rc != 0 and "16B aligned" in msg and name[4:] in msg, (name, which, rc, msg)
            assert out.untouched(), f"{name}: refused, yet the output was written"


def test_wrap_pi_bit_exact(pkg, hip):
    """sra = 1, beta = 0, s1m = 1, sigma = 0 passes x through exactly, so the result is wrap_pi(x): the fp32 rule."""
    v = R.wrap_grid()
    n = len(v)
    xd, ed = dev_f(v), dev_f(np.zeros(n, dtype=np.float32))
    got = np_(twice(lambda: (ddpm_scalar(pkg, xd, ed, None, (1.0, 0.0, 1.0, 0.0), True, n, "wrap_pi"),), "wrap_pi")[0])
    want = R.wrap_pi_fp32(v)
    bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, [(float(v[i]), float(got[i]), float(want[i])) for i in bad[:8]]
    plain = np_(ddpm_scalar(pkg, xd, ed, None, (1.0, 0.0, 1.0, 0.0), False, n, "pass through"))
    assert np.array_equal(plain.view(np.int32), v.view(np.int32))


# ----------------------------------------------------------------------------------------------------- forward noising
@pytest.mark.parametrize("B,per", R.Q_SAMPLE_CASES)
def test_q_sample_wrap(pkg, hip, data, B, per):
    x0, noise, t = R.q_sample_inputs(B, per)
    n = B * per
    xd, nd, td = dev_f(x0), dev_f(noise), dev_i(t, 0, torch.int64)
    what = f"q_sample_wrap B={B} per={per}"

    def run():
        o = fvec(n)
        call(pkg, "e3d_q_sample_wrap", p(xd), p(nd), p(td), p(data["sa_d"]), p(data["s1_d"]), o.ptr, B, per)
        return (take(o, what),)
    got = np_(twice(run, what)[0]).astype(np.float64).reshape(B, per)
    ref, parts = R.q_sample(data["sa"][t][:, None], data["s1"][t][:, None], x0, noise)
    err = R.circ(got, ref)
    bound = 5 * U * parts["G"] + 4 * U * (np.abs(parts["v"]) + np.pi)
    ratio = float((err / bound).max())
    print(f"{what}: worst |got - ref| / bound = {ratio:.3f}")
    assert np.abs(got).max() <= np.pi + 1e-6
    assert (err <= bound).all(), (what, "worst |got - ref| / bound", ratio, np.argwhere(err > bound)[:4].tolist())


# ----------------------------------------------------------------------------------------------------- discrete posterior
class Posterior:
    """The inputs of one posterior case on the device, and the two entry points."""

    def __init__(self, pkg, xt, logits, Qsb, Qtb):
        self.pkg, (self.B, self.L), self.C = pkg, xt.shape, Qsb.shape[-1]
        self.N = self.B * self.L
        self.xt, self.lg, self.qs, self.qt = dev_i(xt, 0), dev_f(logits), dev_f(Qsb), dev_f(Qtb)

    def run(self, mode, u, with_prob, what):
        idx, prob = IVec(self.N), (Out(self.N, self.C) if with_prob else None)
        ud = None if u is None else dev_f(u)
        call(self.pkg, "e3d_discrete_posterior_sample", p(self.xt), p(self.lg), p(self.qs), p(self.qt), p(ud), mode, idx.ptr,
             prob.ptr if with_prob else None, self.B, self.L, self.C)
        return (idx.get(what),) + ((take(prob, what),) if with_prob else ())

    def keyed(self, keys_d, seed, s, what):
        idx = IVec(self.N)
        call(self.pkg, "e3d_keyed_discrete_posterior_sample", p(self.xt), p(self.lg), p(self.qs), p(self.qt), p(keys_d), seed,
             p(word(s)), idx.ptr, self.B, self.L, self.C)
        return (idx.get(what),)


def posterior_bound(logits, C):
    """[N, 1]: (7 C + 20 + 4 D) u, D = max |logit - max logit| of the row (module docstring)."""
    lg = logits.reshape(-1, C).astype(np.float64)
    D = (lg.max(-1) - lg.min(-1))[:, None]
    return (7 * C + 20 + 4 * D) * U


def check_draws(P, prob_t, what):
    """Both modes on every row against the exact rule applied to the kernel's own probabilities; the drawn class has
    probability > 0; prob_out == NULL draws the same."""
    prob = np_(prob_t)
    rows = np.arange(P.N)
    for k, u in enumerate([None] + R.uniform_sets(P.N, 7 * P.N + P.C)):
        mode = 0 if u is None else 1
        idx, again = P.run(mode, u, True, what)
        assert same_bits(again, prob_t), f"{what}: prob_out changed between calls"
        idx = np_(idx).astype(np.int64)
        want = R.pick_fp32(prob, u, mode)
        assert np.array_equal(idx, want), (what, "mode", mode, "u set", k, np.flatnonzero(idx != want)[:8].tolist())
        assert (prob[rows, idx] > 0).all(), f"{what}: a class of probability zero was drawn"
        assert np.array_equal(np_(P.run(mode, u, False, what)[0]), idx), f"{what}: prob_out == NULL draws differ"


@pytest.mark.parametrize("B,L,C,name", POSTERIOR_CASES)
def test_discrete_posterior(pkg, hip, B, L, C, name):
    xt, logits, Qsb, Qtb = posterior_case(B, L, C, name)
    P = Posterior(pkg, xt, logits, Qsb, Qtb)
    what = f"discrete posterior {B}x{L}x{C} {name}"
    _, prob_t = twice(lambda: P.run(0, None, True, what), what)
    got = np_(prob_t).astype(np.float64)
    ref = R.posterior(xt, logits, Qsb, Qtb)
    assert rel_err(prob_t, torch.from_numpy(ref)) < 1e-5
    err, bound = np.abs(got - ref), posterior_bound(logits, C) * ref
    ratio = float((err / bound).max())
    print(f"{what}: worst |got - ref| / bound = {ratio:.3f}; worst |row sum - 1| = {np.abs(got.sum(-1) - 1).max() / U:.2f} u "
          f"(bound {C})")
    assert (err <= bound).all(), (what, "worst |got - ref| / bound", ratio)
    assert (np.abs(got.sum(-1) - 1) <= C * U).all(), what
    check_draws(P, prob_t, what)


@pytest.mark.parametrize("C", [3, 32])
def test_discrete_posterior_zero_total(pkg, hip, C):
    """A zero column of Qsb under some rows' xt: their unnormalised posterior is all zero, the result 1 / C in every
    class -- one float, the reference's to the rounding of a C-term sum and a division."""
    B, L = 2, 37
    xt, logits, Qsb, Qtb = R.zero_total_inputs(B, L, C)
    P = Posterior(pkg, xt, logits, Qsb, Qtb)
    what = f"discrete posterior, zero total, C={C}"
    idx, prob_t = twice(lambda: P.run(0, None, True, what), what)
    got = np_(prob_t)
    hit = xt.reshape(-1) == R.ZERO_COLUMN
    ref = R.posterior(xt, logits, Qsb, Qtb)
    assert (got[hit].view(np.int32) == got[hit][:, :1].view(np.int32)).all(), f"{what}: classes differ"
    assert (np.abs(got[hit].astype(np.float64) - ref[hit]) <= (C + 1) * U * ref[hit]).all()
    assert (np_(idx)[hit] == 0).all()                                       # all equal: the first maximum
    err, bound = np.abs(got.astype(np.float64) - ref), posterior_bound(logits, C) * ref
    assert (err <= bound).all(), (what, float((err / bound).max()))
    check_draws(P, prob_t, what)


@pytest.mark.parametrize("B,L,C,name", [(2, 257, 20, "blosum"), (1, 600, 32, "random")])
def test_keyed_discrete_posterior(pkg, hip, B, L, C, name):
    """The keyed form = the buffer form fed the restated uniforms of stream 3 at step s_dev[0]; rows of no item: u = 0."""
    P = Posterior(pkg, *posterior_case(B, L, C, name))
    keys = R.key_table(P.N)
    kd = dev_keys(keys)
    for seed in R.SEEDS:
        for s in (0, 999, 65535):
            what = f"keyed posterior {B}x{L}x{C} seed={seed} s={s}"
            got = twice(lambda: P.keyed(kd, seed, s, what), what)[0]
            u = R.keyed_uniforms(keys, seed, 3, s)
            assert (u[keys[:, 1] < 0] == 0).all() and len(np.unique(u)) > P.N // 2
            assert torch.equal(got, P.run(1, u, False, what)[0]), what


# ----------------------------------------------------------------------------------------------------- discrete forward noising
@pytest.mark.parametrize("C", R.Q_CLASSES)
@pytest.mark.parametrize("BL", sorted(R.Q_ROWS))
def test_discrete_q_sample(pkg, hip, BL, C):
    x0, Qtb = discrete_q_case(BL, C)
    B, L = x0.shape
    xd, qd = dev_i(x0, -1), dev_f(Qtb)
    p32 = R.forward_column(Qtb, x0)
    drawn = x0.reshape(-1) >= 0
    rows = np.arange(BL)
    what = f"discrete_q_sample {B}x{L}x{C}"

    def run(mode, u):
        idx = IVec(BL)
        call(pkg, "e3d_discrete_q_sample", p(xd), p(qd), p(None if u is None else dev_f(u)), mode, idx.ptr, B, L, C)
        return (idx.get(what),)
    for k, u in enumerate([None] + R.uniform_sets(BL, 11 * BL + C)):
        mode = 0 if u is None else 1
        idx = np_(twice(lambda: run(mode, u), what)[0]).astype(np.int64)
        want = np.where(drawn, R.pick_fp32(p32, u, mode), 0)
        assert np.array_equal(idx, want), (what, "mode", mode, "u set", k, np.flatnonzero(idx != want)[:8].tolist())
        assert (p32[rows, idx][drawn] > 0).all(), f"{what}: a class of probability zero was drawn"
    if BL not in (257, 900):
        return
    ids = R.IDS[2:3] if B == 1 else (R.IDS[2], R.IDS[3], R.IDS[1])
    ids_d = dev_i(R.as_int64(ids), 0, torch.int64)
    keys = R.padded_keys(ids, L)
    for seed in R.SEEDS:
        for epoch in (0, 65535):                                            # 65535: the validation word
            def keyed():
                idx = IVec(BL)
                call(pkg, "e3d_keyed_discrete_q_sample", p(xd), p(qd), p(ids_d), p(word(epoch)), seed, idx.ptr, B, L, C)
                return (idx.get(what),)
            got = twice(keyed, what)[0]
            u = R.keyed_uniforms(keys, seed, 7, epoch)
            assert torch.equal(got, run(1, u)[0]), (what, seed, epoch)
            assert np.array_equal(np_(got).astype(np.int64), np.where(drawn, R.pick_fp32(p32, u, 1), 0))


# ----------------------------------------------------------------------------------------------------- keyed draws
def keyed_normals(pkg, kd, seed, stream, t, F, rows, wrap=0, scale=1.0, what="keyed_draws"):
    o = fvec(rows * F)
    call(pkg, "e3d_keyed_draws", p(kd), seed, stream, t, 0, F, wrap, scale, o.ptr, rows)
    return take(o, what)


@pytest.mark.parametrize("rows,F", [(37, 4), (37, 8), (2049, 1024)])
def test_keyed_draws(pkg, hip, rows, F):
    """All four kinds against the restatement; rows of no item are zero.  2049 x 1024: 524 544 float4 groups, more than
    the capped grid has threads, block indices up to 255."""
    keys = R.key_table(rows)
    kd = dev_keys(keys)
    none = keys[:, 1] < 0
    big = rows * F // 4 > BLOCKS
    worst = 0.0
    for seed in (R.SEEDS[1:] if big else R.SEEDS):
        for t in ((65535,) if big else (0, 999, 65535)):
            what = f"keyed_draws rows={rows} F={F} seed={seed} t={t}"
            z = K.normals(keys, seed, 1, t, F)
            tol = 2e-6 * np.maximum(1.0, np.abs(z))
            got = np_(twice(lambda: (keyed_normals(pkg, kd, seed, 1, t, F, rows, what=what),), what)[0]).reshape(rows, F)
            err = np.abs(got - z)
            worst = max(worst, float((err / tol).max()))
            assert (err <= tol).all(), (what, float((err / tol).max()))
            assert (got[none].view(np.int32) == 0).all() and 0.9 < got[~none].std() < 1.1
            z0 = z if big else K.normals(keys, seed, 0, t, F)              # the big shape: one Box-Muller pass
            for scale in (1.0, 1.5):
                w = np_(keyed_normals(pkg, kd, seed, 1 if big else 0, t, F, rows, 1, scale, what)).reshape(rows, F)
                err, wtol = R.circ(w, scale * z0), scale * 2e-6 * np.maximum(1.0, np.abs(z0))
                worst = max(worst, float((err / wtol).max()))
                assert (err <= wtol).all(), (what, "wrap", scale, float((err / wtol).max()))
                assert np.abs(w).max() <= np.pi + 1e-6 and (w[none].view(np.int32) == 0).all()
            if F != 4 and not big:
                continue
            # kinds 1 - 3 (one draw per row): bit for bit
            o = fvec(rows)
            call(pkg, "e3d_keyed_draws", p(kd), seed, 3, t, 1, 0, 0, 1.0, o.ptr, rows)
            assert np.array_equal(np_(take(o, what)).view(np.int32), K.uniforms(keys, seed, 3, t).astype(np.float32).view(np.int32))
            for C in (2, 20):
                cls = K.classes(keys, seed, 2, t, C)
                oh = Out(rows, C)
                call(pkg, "e3d_keyed_draws", p(kd), seed, 2, t, 2, C, 0, 1.0, oh.ptr, rows)
                want = np.zeros((rows, C), dtype=np.float32)
                want[np.arange(rows)[~none], cls[~none]] = 1.0
                assert np.array_equal(np_(take(oh, what)).view(np.int32), want.view(np.int32)), what
                oi = IVec(rows)
                call(pkg, "e3d_keyed_draws", p(kd), seed, 2, t, 3, C, 0, 1.0, oi.ptr, rows)
                assert np.array_equal(np_(oi.get(what)).astype(np.int64), cls), what
    print(f"keyed_draws rows={rows} F={F}: worst |z - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("rows,F", [(37, 4), (2049, 1024)])
def test_keyed_ddpm_step(pkg, hip, data, rows, F):
    """= the table form fed the keyed draws of stream 1 at step t, bit for bit; rows of no item get the mean; in place."""
    n = rows * F
    x, e, _ = R.ddpm_inputs(n, seed=48)
    xd, ed = dev_f(x), dev_f(e)
    keys = R.key_table(rows)
    kd = dev_keys(keys)
    none = torch.from_numpy(np.repeat(keys[:, 1] < 0, F)).to(DEV)
    seed = R.SEEDS[1]
    for t in (500, 0):
        for wrap in ((1,) if n > R.N_BIG else (1, 0)):
            what = f"keyed_ddpm_step rows={rows} F={F} t={t} wrap={wrap}"

            def run(x_in, o):
                call(pkg, "e3d_keyed_ddpm_step_wrap", p(x_in), p(ed), p(data["coef"]), p(word(t)), p(kd), seed, wrap, o.ptr, rows, F)
                return (take(o, what),)
            got = twice(lambda: run(xd, fvec(n)), what)[0]
            z = keyed_normals(pkg, kd, seed, 1, t, F, rows)
            want = ddpm_table(pkg, xd, ed, z, data["coef"], t, wrap, n, what)
            assert same_bits(got, want), what
            mean = ddpm_scalar(pkg, xd, ed, None, data["rows"][t], wrap, n, what)
            assert same_bits(got[none], mean[none]), f"{what}: a row of no item is not the mean"
            assert same_bits(got, mean) == (t == 0)
            o = fvec(n)
            o.v.copy_(xd.reshape(n, 1))
            o.before = o.big.clone()
            assert same_bits(run(o.v, o)[0], got), f"{what}: out == x differs"


# ----------------------------------------------------------------------------------------------------- keyed training draws
@pytest.mark.parametrize("B,L,F", [(3, 5, 8), (3, 683, 1024)])
def test_keyed_q_sample_wrap(pkg, hip, data, B, L, F):
    """noise = wrap(scale z) of stream 5 against the restatement (2e-6 on the circle, the bound of
    test_keyed_training_gpu.py); x_t bit-identical to e3d_q_sample_wrap fed that noise; t outside [0, T) reads the end
    rows.  3 x 683 x 1024: 524 544 float4 groups, past the capped grid."""
    n = B * L * F
    x0 = R.ddpm_inputs(n, seed=49)[0]
    xd = dev_f(x0)
    ids = (R.IDS[2], R.IDS[3], R.IDS[1])
    ids_d = dev_i(R.as_int64(ids), 0, torch.int64)
    keys = R.padded_keys(ids, L)
    seed = R.SEEDS[1]
    inside, outside = dev_i(np.array([0, 999, 500]), 0, torch.int64), dev_i(np.array([-5, 1200, 500]), 0, torch.int64)
    big = n // 4 > BLOCKS
    for epoch, scale in (((65535, 1.0),) if big else ((0, 1.0), (1, 0.5), (65535, 1.0))):
        what = f"keyed_q_sample_wrap {B}x{L}x{F} epoch={epoch} scale={scale}"

        def run(td):
            noise, xt = fvec(n), fvec(n)
            call(pkg, "e3d_keyed_q_sample_wrap", p(xd), p(td), p(data["sa_d"]), p(data["s1_d"]), 1000, scale, p(ids_d),
                 p(word(epoch)), seed, noise.ptr, xt.ptr, B, L, F)
            return take(noise, what), take(xt, what)
        noise, xt = twice(lambda: run(inside), what)
        want = scale * K.normals(keys, seed, 5, epoch, F).reshape(-1)
        d = float(R.circ(np_(noise), want).max())
        print(f"{what}: max wrapped |noise - restatement| = {d:.3e} (2e-6)")
        assert d <= 2e-6 and float(noise.abs().max()) <= np.pi + 1e-6
        o = fvec(n)
        call(pkg, "e3d_q_sample_wrap", p(xd), p(noise), p(inside), p(data["sa_d"]), p(data["s1_d"]), o.ptr, B, L * F)
        assert same_bits(xt, take(o, what)), f"{what}: x_t differs from q_sample_wrap fed the noise"
        clamped = run(outside)
        assert same_bits(clamped[0], noise) and same_bits(clamped[1], xt), f"{what}: t outside [0, T) is not clamped"


@pytest.mark.parametrize("B", [1, 256, 257])
def test_keyed_timesteps(pkg, hip, B):
    ids = [(R.IDS[b % len(R.IDS)] + 1000 * b) % (1 << 64) for b in range(B)]
    ids_d = dev_i(R.as_int64(ids), 0, torch.int64)
    keys = R.padded_keys(ids, 1)
    for seed in R.SEEDS:
        for epoch in (0, 65535):
            for stream, C in ((4, 1000), (6, 51), (4, 1), (6, 1 << 24)):
                what = f"keyed_timesteps B={B} seed={seed} epoch={epoch} stream={stream} C={C}"

                def run():
                    o = IVec(B, torch.int64)
                    call(pkg, "e3d_keyed_timesteps", p(ids_d), p(word(epoch)), seed, stream, C, o.ptr, B)
                    return (o.get(what),)
                got = np_(twice(run, what)[0])
                assert np.array_equal(got, K.classes(keys, seed, stream, epoch, C)), what
                assert C > 1 or (got == 0).all()
