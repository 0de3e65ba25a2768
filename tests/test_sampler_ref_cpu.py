"""tests/sampler_ref.py checked without a GPU.

1. Every float64 statement against the oracle (oracle/structure.py, oracle/sequence.py) evaluated in float64, to 1e-12: a
   wrong reference cannot then pass a wrong kernel.  The two fp32 rules against what they restate: ``wrap_pi_fp32`` bit for
   bit against ``modulo_with_wrapped_range`` on fp32 tensors, ``pick_fp32`` against the float64 ``categorical_from_uniform``
   wherever the float64 cdf is further than 1e-5 from the threshold.
2. The inputs of tests/test_sampler_forms_gpu.py: the synthetic transitions are row-stochastic where they claim to be, the
   zero-column case gives an all-zero unnormalised posterior in float64, the pick never lands on a class of probability
   zero, the key tables hold what the kernels' index arithmetic must survive, and at an item boundary of the forward
   noising the neighbouring item's table row misses the bound by far.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sampler_ref as R
from helpers import GOLDEN
from oracle import sequence as oseq
from oracle import structure as ostr

U = R.U
S_INTS = (1, 48, 24, 10)      # the items' steps s of the C = 20 transitions (t = s + 1), of a 50-step schedule
T_SEQ = 50


def transitions(name, B):
    """(Qsb, Qtb) fp32 numpy [B, 20, 20] of the BLOSUM or the uniform transition at the steps S_INTS[:B]."""
    sched = oseq.NoiseScheduleDiscrete(T_SEQ)
    blosum = torch.load(os.path.join(GOLDEN, "blosum_substitute.pt"), weights_only=True)
    trans = oseq.BlosumTransition(blosum) if name == "blosum" else oseq.UniformTransition(20)
    s = torch.tensor(S_INTS[:B], dtype=torch.float32).reshape(B, 1)
    qsb = trans.get_Qt_bar(sched.get_alpha_bar(s / T_SEQ))
    qtb = trans.get_Qt_bar(sched.get_alpha_bar((s + 1) / T_SEQ))
    return qsb.numpy().copy(), qtb.numpy().copy()


POSTERIOR_CASES = [(B, L, C, name) for (B, L, C) in R.POSTERIOR_SHAPES
                   for name in (("blosum", "uniform") if C == 20 else ("random",))]


def posterior_case(B, L, C, name):
    Qsb, Qtb = transitions(name, B) if C == 20 else (None, None)
    return R.posterior_inputs(B, L, C, Qsb, Qtb)


def discrete_q_case(BL, C):
    B, L = R.Q_ROWS[BL]
    return R.discrete_q_inputs(B, L, C, transitions("blosum", B)[1] if C == 20 else None)


class _Schedule:
    """get_alpha_bar hands its argument on: the transition below tells t from s by identity."""
    timesteps = 1

    def get_alpha_bar(self, x):
        return x


class _Transition:
    def __init__(self, by_key):
        self.by_key = by_key

    def get_Qt_bar(self, key):
        for k, v in self.by_key:
            if k is key:
                return v.clone()
        return self.by_key[-1][1].clone()


def oracle_reverse_prob(xt, logits, Qsb, Qtb):
    B, L = xt.shape
    C = Qsb.shape[-1]
    t, s = torch.ones(B, 1), torch.zeros(B, 1)
    trans = _Transition([(t, torch.from_numpy(Qtb).double()), (s, torch.from_numpy(Qsb).double())])
    x_t = F.one_hot(torch.from_numpy(xt).long(), C).double()
    return oseq.reverse_prob(t, s, x_t, torch.from_numpy(logits).double(), _Schedule(), trans).numpy()


def close(got, want, what, tol=1e-12):
    scale = max(float(np.abs(want).max()), 1e-300)
    assert float(np.abs(got - want).max()) <= tol * scale, what


# ----------------------------------------------------------------------------------------------------- fp64 statements
def test_ddpm_matches_p_sample():
    betas = ostr.cosine_beta_schedule(1000).double()
    ab = ostr.compute_alphas(betas)
    x, e, z = (v[:296] for v in R.ddpm_inputs(296))
    tx, te, tz = (torch.from_numpy(v).double() for v in (x, e, z))
    for t in R.TIMESTEPS:
        want = ostr.p_sample(lambda *a: te, None, tx, None, None, None, torch.full((1,), t), betas, tz)
        row = (1.0 / torch.sqrt(ab["alphas"][t]), betas[t], ab["sqrt_one_minus_alphas_cumprod"][t],
               torch.sqrt(ab["posterior_variance"][t]))
        assert (float(row[3]) == 0.0) == (t == 0)
        got, parts = R.ddpm(row, x, e, z)
        close(got, want.numpy(), f"ddpm t={t}")
        assert (parts["G"] >= np.abs(parts["v"]) * (1 - 1e-12)).all()
        wrapped = ostr.modulo_with_wrapped_range(want, -torch.pi, torch.pi).numpy()
        assert R.circ(R.ddpm(row, x, e, z, wrap=True)[0], wrapped).max() < 1e-12
        mean = ostr.p_sample(lambda *a: te, None, tx, None, None, None, torch.full((1,), t), betas, torch.zeros_like(tz))
        close(R.ddpm(row, x, e, None)[0], mean.numpy(), f"ddpm mean t={t}")


def test_q_sample_matches_add_noise_by_timestep():
    terms = ostr.compute_alphas(ostr.cosine_beta_schedule(1000).double())
    x0, noise, t = R.q_sample_inputs(6, 7)
    for b in range(6):
        want = ostr.add_noise_by_timestep(torch.from_numpy(x0[b]).double(), int(t[b]), terms,
                                          torch.from_numpy(noise[b]).double()).numpy()
        got, parts = R.q_sample(float(terms["sqrt_alphas_cumprod"][t[b]]),
                                float(terms["sqrt_one_minus_alphas_cumprod"][t[b]]), x0[b], noise[b])
        assert R.circ(got, want).max() < 1e-12 and (parts["G"] >= np.abs(parts["v"]) * (1 - 1e-12)).all()


def test_wrap_pi_fp32_is_the_fp32_modulo_bit_for_bit():
    v = R.wrap_grid()
    assert v.dtype == np.float32 and len(v) > 4096 + 15 * 17
    want = ostr.modulo_with_wrapped_range(torch.from_numpy(v)).numpy()
    got = R.wrap_pi_fp32(v)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.abs(got).max() <= np.pi + 1e-6
    # and it is the float64 wrap to fp32 rounding: two additions and the fp32 value of 2 pi
    small = np.abs(v) <= 100
    assert (R.circ(got[small], R.wrap_pi(v[small])) <= 4 * U * (np.abs(v[small]) + np.pi)).all()


@pytest.mark.parametrize("B,L,C,name", POSTERIOR_CASES)
def test_posterior_matches_reverse_prob(B, L, C, name):
    xt, logits, Qsb, Qtb = posterior_case(B, L, C, name)
    got = R.posterior(xt, logits, Qsb, Qtb)
    close(got, oracle_reverse_prob(xt, logits, Qsb, Qtb), (B, L, C, name))
    assert got.shape == (B * L, C) and (got > 0).all() and np.abs(got.sum(-1) - 1).max() < 1e-12
    # the transitions are row-stochastic: the synthetic ones to fp32 rounding of C terms, every entry >= 1e-3
    for Q in (Qsb, Qtb):
        assert np.abs(Q.astype(np.float64).sum(-1) - 1).max() <= (C * U if name == "random" else 1e-4)
        assert name != "random" or Q.min() >= 1e-3


@pytest.mark.parametrize("C", [3, 20, 32])
def test_zero_column_gives_a_zero_total_in_float64(C):
    xt, logits, Qsb, Qtb = R.zero_total_inputs(2, 37, C)
    assert (Qsb[:, :, R.ZERO_COLUMN] == 0).all() and (Qtb > 0).all()
    assert np.abs(Qsb.astype(np.float64).sum(-1) - 1).max() <= C * U
    hit = xt.reshape(-1) == R.ZERO_COLUMN
    assert 10 < hit.sum() < hit.size - 10
    un = R.posterior_unnormalised(xt, logits, Qsb, Qtb)
    assert (un[hit] == 0).all() and (un[~hit].sum(-1) > 0).all()
    got = R.posterior(xt, logits, Qsb, Qtb)
    assert (got[hit] == 1.0 / C).all() or np.abs(got[hit] - 1.0 / C).max() < 1e-15
    close(got, oracle_reverse_prob(xt, logits, Qsb, Qtb), ("zero column", C))


@pytest.mark.parametrize("BL", sorted(R.Q_ROWS))
@pytest.mark.parametrize("C", R.Q_CLASSES)
def test_forward_column_matches_aa_noise_prob(BL, C):
    x0, Qtb = discrete_q_case(BL, C)
    B, L = x0.shape
    onehot = F.one_hot(torch.from_numpy(x0).long().clamp_min(0), C).double() * torch.from_numpy(x0 >= 0)[..., None]
    trans = _Transition([(None, torch.from_numpy(Qtb).double())])
    want = oseq.aa_noise_prob(onehot, torch.ones(B, 1), _Schedule(), trans).numpy()
    got = R.forward_column(Qtb, x0)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
    pad = x0.reshape(-1) < 0
    assert (pad[-1] or BL == 1) and not pad[0] and (got[pad] == 0).all() and (got[~pad].sum(-1) > 0).all()
    assert (got[~pad] == 0).any(), "no exact zero among the probabilities"


# ----------------------------------------------------------------------------------------------------- the class pick
def _rows_of_every_draw_test():
    """(name, p32 [N, C], rows that are drawn) of every probability table the GPU test picks from, the reference's
    probabilities rounded to fp32 standing in for the kernel's."""
    for B, L, C, name in POSTERIOR_CASES:
        p = R.posterior(*posterior_case(B, L, C, name)).astype(np.float32)
        yield f"posterior {B}x{L}x{C} {name}", p, np.ones(len(p), dtype=bool)
    for C in (3, 32):
        p = R.posterior(*R.zero_total_inputs(2, 37, C)).astype(np.float32)
        yield f"zero total C={C}", p, np.ones(len(p), dtype=bool)
    for BL in sorted(R.Q_ROWS):
        for C in R.Q_CLASSES:
            x0, Qtb = discrete_q_case(BL, C)
            yield f"forward {BL}x{C}", R.forward_column(Qtb, x0), x0.reshape(-1) >= 0


def test_pick_agrees_with_the_float64_draw_where_it_is_clear():
    seen = 0
    for n, (name, p, drawn) in enumerate(_rows_of_every_draw_test()):
        for u in R.uniform_sets(len(p), 100 + n):
            got = R.pick_fp32(p, u, 1)
            p64, u64 = torch.from_numpy(p).double(), torch.from_numpy(u).double()
            want = oseq.categorical_from_uniform(p64, u64).numpy()
            cdf = p64.cumsum(-1)
            clear = ((cdf - (u64 * cdf[:, -1]).unsqueeze(-1)).abs().min(-1).values > 1e-5).numpy() & drawn
            assert np.array_equal(got[clear], want[clear]), name
            seen += int(clear.sum())
        assert np.array_equal(R.pick_fp32(p, None, 0)[drawn], p.astype(np.float64).argmax(-1)[drawn]), name
    assert seen > 10000


def test_pick_never_lands_on_a_class_of_probability_zero():
    for n, (name, p, drawn) in enumerate(_rows_of_every_draw_test()):
        rows = np.arange(len(p))
        for u in R.uniform_sets(len(p), 100 + n):
            for mode in (0, 1):
                idx = R.pick_fp32(p, u, mode)
                assert (p[rows, idx][drawn] > 0).all(), (name, mode)
    # the rule itself, on random rows with zero classes at the front, in the middle and at the end
    rng = np.random.default_rng(3)
    for C in (2, 3, 20, 32):
        p = rng.random((20000, C)).astype(np.float32)
        p[rng.random((20000, C)) < 0.4] = 0
        p[:, 0][rng.random(20000) < 0.5] = 0
        p[:, -1][rng.random(20000) < 0.5] = 0
        keep = p.sum(-1) > 0
        p = p[keep]
        for e in R.EDGE_U:
            idx = R.pick_fp32(p, np.full(len(p), e, dtype=np.float32), 1)
            assert (p[np.arange(len(p)), idx] > 0).all(), (C, e)


# ----------------------------------------------------------------------------------------------------- other inputs
def test_neighbouring_item_row_misses_the_bound_at_item_boundaries():
    tab = ostr.compute_alphas(ostr.cosine_beta_schedule(1000))
    sa, s1 = tab["sqrt_alphas_cumprod"].numpy(), tab["sqrt_one_minus_alphas_cumprod"].numpy()
    for B, per in R.Q_SAMPLE_CASES:
        x0, noise, t = R.q_sample_inputs(B, per)
        assert len(t) == B and len(set(t.tolist())) == B and t.min() >= 0 and t.max() <= 999
        assert B == 1 or (0 in t and 999 in t)
        ref, parts = R.q_sample(sa[t][:, None], s1[t][:, None], x0, noise)
        bound = 5 * U * parts["G"] + 4 * U * (np.abs(parts["v"]) + np.pi)
        for shift in (1, -1):
            tn = np.roll(t, shift)
            other, _ = R.q_sample(sa[tn][:, None], s1[tn][:, None], x0, noise)
            edge = (slice(1, None), 0) if shift == 1 else (slice(0, -1), -1)
            if B > 1:
                assert (R.circ(other, ref)[edge] > 1000 * bound[edge]).all(), (B, per, shift)


def test_key_tables_hold_the_edges():
    for rows in (37, 257, 600, 2049):
        keys = R.key_table(rows)
        none = keys[:, 1] < 0
        assert none[0] and none[rows // 2] and none[-1] and none.sum() == 3
        pos = keys[~none, 1]
        assert {0, 255, (1 << 24) - 1} <= set(pos.tolist()) and pos.max() < 1 << 24 and pos.min() >= 0
        ids = keys[~none, 0].astype(np.uint64)
        assert (ids > np.uint64(1 << 63)).any() and ((ids > np.uint64(1 << 32)) & (ids < np.uint64(1 << 63))).any()
    keys = R.padded_keys(R.IDS[:3], 5)
    assert keys.shape == (15, 2) and keys[7].tolist() == [int(R.as_int64(R.IDS)[1]), 2]
    z = R.ddpm_inputs(1023)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in z) and np.abs(z[0]).max() <= np.pi
