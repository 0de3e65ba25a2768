"""GPU: sequence design controls -- temperature, residue bias and design scores (csrc/sampler.hip, "design controls").
The posterior under controls through the C ABI against the existing kernel (no controls: bit for bit), against float64
(tests/sampler_ref.py fed the fp32 effective logits of tests/design_ref.py) and against its keyed form; the last step's
pick against float64; then chains and the entry point.  Plumbing and conventions are those of
tests/test_sampler_forms_gpu.py: outputs between guard words, NaN after every input, every case run twice.

Bounds (u = 2^-24).
  * Effective logits z = (logit + bias) * inv_temp: one add, one multiply, each correctly rounded and never fused, so z is
    an exact function of the three fp32 inputs, and tests/design_ref.py computes the same fp32 numbers.  Nothing is
    allowed for them.
  * Posterior: the bound test_sampler_forms_gpu.py derives, |got - ref| <= (7 C + 20 + 4 D) u ref, carries over as it is.
    Its derivation starts from the fp32 logits the softmax reads and counts the roundings after them; here the softmax
    reads z, the reference is given the same z, and every later operation is the same.  D = max |z - max z| over the
    FINITE effective logits of the row: a forbidden class has exp(-inf - mx) = 0 exactly, in fp32 and in float64 alike,
    and adds a zero to every sum it enters, which rounds nothing.  Row sums: within C u of 1, as there.
  * Final pick.  The index is exact: the first maximum of z.  With d[c] = z[c] - mx (one subtraction: relative u, hence
    at most u D absolute, D as above), e[c] = expf(d[c]) and se the C-term sequential sum:
      e[c]:  u |d[c]| from the argument (the exponential turns an absolute error of its argument into a relative one of
             its value) + 2 u for expf, which HIP documents as good to 1 ulp = 2 u relative at worst     ->  (D + 2) u
      se:    its terms are non-negative, so their relative errors do not grow; C - 1 additions           ->  (D + C + 1) u
      lse = logf(se): a relative error of se is an absolute one of its logarithm; logf, documented as good to 1 ulp,
             adds 2 u |lse|                                                                    ->  (D + C + 1) u + 2 u |lse|
    logp = 0 - lse exactly (the pick is the maximum, d = 0 there), so
      |logp - ref| <= (D + C + 5) u + 2 u |ref|                           (four added for second order).
    entropy = sum_c p[c] g[c], p[c] = e[c] / se, g[c] = lse - d[c]; every p and g is non-negative, so relative errors add
    and nothing cancels:
      p[c]:  (D + 2) + (D + C + 1) + 1 for the division                                                  ->  (2 D + C + 4) u
      g[c]:  the error of lse, u |d[c]| from d, u g for the subtraction; lse, |d[c]| <= g[c]  ->  (D + C + 1) u + 3 u g[c]
      the product 1, the C-term sum C - 1
    so |entropy - ref| <= sum_c p[c] ((2 D + 2 C + 7) u g[c] + (D + C + 1) u) = (2 D + 2 C + 7) u H + (D + C + 1) u, and
      |entropy - ref| <= (2 D + 2 C + 11) u ref + (D + C + 5) u            (four added to each part for second order).
    A class whose exponential underflows (d < -87) is off by at most its own size, below 2^-126: nothing next to u.

Measured on an MI355X, worst |got - ref| / bound over all cases of a test (each test prints its own; DESIGN.md,
"Sequence design controls", records them too):
  posterior under controls   0.070  (2 x 5 x 3; 0.059 at 2 x 37 x 20, 0.044 at 1 x 257 x 20, 0.039 at 1 x 600 x 32).
                             Row sums: 5.6 u at C = 32 (bound 32), 4.6 u at C = 20, 1.5 u at C = 3.
  final pick, logp           0.289  (1000 x 3; 0.204 at 1000 x 20, 0.176 at 1000 x 32)
  final pick, entropy        0.128  (1000 x 20; 0.126 at 1000 x 32, 0.125 at 257 x 3)
Everything else in this module is compared bit for bit, or is a statement about strings.
"""
import warnings

import numpy as np
import pytest
import torch

import design_ref as DR
import sampler_ref as R
from helpers import seeded_state_dict, synthetic_pockets
from test_rowops_forms_gpu import DEV, Out, Vec, call, p, twice
from test_sampler_forms_gpu import IVec, dev_f, dev_i, dev_keys, np_, same_bits, take, word
from test_sampler_ref_cpu import posterior_case

pytestmark = pytest.mark.gpu

U = R.U
VOCAB = "ACDEFGHIKLMNPQRSTVWY"
CASES = [(B, L, C, "blosum" if C == 20 else "random") for B, L, C in DR.SHAPES]


# ----------------------------------------------------------------------------------------------------- plumbing
class Ctl:
    """The inputs of one posterior case on the device and the three entry points: without controls, with them, keyed."""

    def __init__(self, pkg, xt, logits, Qsb, Qtb):
        self.pkg, (self.B, self.L), self.C = pkg, xt.shape, Qsb.shape[-1]
        self.N = self.B * self.L
        self.xt, self.qs, self.qt = dev_i(xt, 0), dev_f(Qsb), dev_f(Qtb)
        self.lg = dev_f(logits)

    def _outs(self, with_prob):
        return IVec(self.N), (Out(self.N, self.C) if with_prob else None)

    def plain(self, mode, u, what, with_prob=True):
        idx, prob = self._outs(with_prob)
        call(self.pkg, "e3d_discrete_posterior_sample", p(self.xt), p(self.lg), p(self.qs), p(self.qt),
             p(None if u is None else dev_f(u)), mode, idx.ptr, prob.ptr if with_prob else None, self.B, self.L, self.C)
        return (idx.get(what),) + ((take(prob, what),) if with_prob else ())

    def ctl(self, bias_d, inv_temp, mode, u, what, with_prob=True, lg=None):
        idx, prob = self._outs(with_prob)
        call(self.pkg, "e3d_discrete_posterior_sample_ctl", p(self.xt), p(self.lg if lg is None else lg), p(bias_d),
             float(inv_temp), p(self.qs), p(self.qt), p(None if u is None else dev_f(u)), mode, idx.ptr,
             prob.ptr if with_prob else None, self.B, self.L, self.C)
        return (idx.get(what),) + ((take(prob, what),) if with_prob else ())

    def keyed(self, bias_d, inv_temp, keys_d, seed, s, what):
        idx = IVec(self.N)
        call(self.pkg, "e3d_keyed_discrete_posterior_sample_ctl", p(self.xt), p(self.lg), p(bias_d), float(inv_temp), p(self.qs),
             p(self.qt), p(keys_d), seed, p(word(s)), idx.ptr, self.B, self.L, self.C)
        return (idx.get(what),)


def final_pick(pkg, lg_d, bias_d, inv_temp, rows, C, what, scores=True):
    idx = IVec(rows)
    logp, ent = (Vec(rows), Vec(rows)) if scores else (None, None)
    call(pkg, "e3d_discrete_final_pick", p(lg_d), p(bias_d), float(inv_temp), idx.ptr, logp.ptr if scores else None,
         ent.ptr if scores else None, rows, C)
    return (idx.get(what),) + ((take(logp, what), take(ent, what)) if scores else ())


def bound_factor(z, C):
    """[N, 1]: (7 C + 20 + 4 D) u with D over the finite effective logits of the row (module docstring)."""
    return ((7 * C + 20 + 4 * DR.spread(z.reshape(-1, C))) * U)[:, None]


# ----------------------------------------------------------------------------------------------------- 1. no controls
@pytest.mark.parametrize("B,L,C,name", CASES)
def test_no_controls_in_the_ctl_form_is_the_existing_kernel_bit_for_bit(pkg, hip, B, L, C, name):
    P = Ctl(pkg, *posterior_case(B, L, C, name))
    zero = dev_f(np.zeros((B, L, C), dtype=np.float32))
    us = R.uniform_sets(P.N, 7 * P.N + C)
    for mode, u in ((0, None), (1, us[0]), (1, us[3])):
        what = f"ctl without controls {B}x{L}x{C} mode={mode}"
        idx, prob = twice(lambda: P.plain(mode, u, what), what)
        for bias_d, tag in ((None, "bias NULL"), (zero, "zero bias")):
            got_idx, got_prob = twice(lambda: P.ctl(bias_d, 1.0, mode, u, what), what)
            assert same_bits(got_prob, prob), f"{what}, {tag}: prob_out differs"
            assert torch.equal(got_idx, idx), f"{what}, {tag}: draws differ"
            assert torch.equal(P.ctl(bias_d, 1.0, mode, u, what, with_prob=False)[0], idx), f"{what}, {tag}: prob_out == NULL"


# ----------------------------------------------------------------------------------------------------- 2. against float64
@pytest.mark.parametrize("B,L,C,name", CASES)
def test_posterior_under_controls_against_float64(pkg, hip, B, L, C, name):
    xt, logits, Qsb, Qtb = posterior_case(B, L, C, name)
    P = Ctl(pkg, xt, logits, Qsb, Qtb)
    bias = DR.bias_inputs(P.N, C).reshape(B, L, C)
    closed = np.isneginf(bias)
    assert closed.any() and not closed.all(-1).any()               # test_design_cpu.py checks the share on a large table
    bias_d = dev_f(bias)
    rng = np.random.default_rng(5)
    other_d = dev_f(np.where(closed, rng.uniform(-300.0, 300.0, logits.shape).astype(np.float32), logits))
    rows = np.arange(P.N)
    worst = worst_sum = 0.0
    for T in DR.TEMPERATURES:
        it = DR.inv_temp(T)
        what = f"posterior under controls {B}x{L}x{C} {name} T={T}"
        _, prob_t = twice(lambda: P.ctl(bias_d, it, 0, None, what), what)
        got = np_(prob_t).astype(np.float64)
        z = DR.effective_logits(logits, bias, it)
        ref = R.posterior(xt, z, Qsb, Qtb)
        assert np.isfinite(got).all() and (ref > 0).all()
        err, bound = np.abs(got - ref), bound_factor(z, C) * ref
        ratio = float((err / bound).max())
        sums = float(np.abs(got.sum(-1) - 1).max() / U)
        worst, worst_sum = max(worst, ratio), max(worst_sum, sums)
        print(f"{what}: worst |got - ref| / bound = {ratio:.3f}; worst |row sum - 1| = {sums:.2f} u (bound {C})")
        assert (err <= bound).all(), (what, "worst |got - ref| / bound", ratio)
        assert (np.abs(got.sum(-1) - 1) <= C * U).all(), what
        # the draws: the exact rule on the kernel's own probabilities, both modes
        prob32 = np_(prob_t)
        for k, u in enumerate([None] + R.uniform_sets(P.N, 7 * P.N + C)[:2]):
            mode = 0 if u is None else 1
            idx, again = P.ctl(bias_d, it, mode, u, what)
            assert same_bits(again, prob_t), f"{what}: prob_out changed between calls"
            idx = np_(idx).astype(np.int64)
            want = R.pick_fp32(prob32, u, mode)
            assert np.array_equal(idx, want), (what, "mode", mode, "u set", k, np.flatnonzero(idx != want)[:8].tolist())
            assert (prob32[rows, idx] > 0).all()
        # a forbidden class contributes exactly nothing: any finite logit under it, the same bits
        assert same_bits(P.ctl(bias_d, it, 0, None, what, lg=other_d)[1], prob_t), f"{what}: a forbidden class's logit was read"
    print(f"posterior under controls {B}x{L}x{C} {name}: worst |got - ref| / bound = {worst:.3f}, row sums {worst_sum:.2f} u")


# ----------------------------------------------------------------------------------------------------- 3. all forbidden
@pytest.mark.parametrize("C", [3, 20])
def test_a_row_with_every_class_forbidden(pkg, hip, C):
    B, L = 2, 37
    xt, logits, Qsb, Qtb = posterior_case(B, L, C, "blosum" if C == 20 else "random")
    P = Ctl(pkg, xt, logits, Qsb, Qtb)
    open_bias = DR.bias_inputs(P.N, C).reshape(B, L, C)
    bias = open_bias.copy()
    bias[0, 0] = -np.inf
    it = DR.inv_temp(0.5)
    what = f"all-forbidden row C={C}"
    for mode, u in ((0, None), (1, R.uniform_sets(P.N, 3)[0])):
        idx, prob_t = twice(lambda: P.ctl(dev_f(bias), it, mode, u, what), what)
        base_idx, base_prob = P.ctl(dev_f(open_bias), it, mode, u, what)
        got = np_(prob_t)
        assert np.isfinite(got).all()
        assert (got[0].view(np.int32) == got[0, :1].view(np.int32)).all(), f"{what}: classes differ"
        assert (np.abs(got[0].astype(np.float64) - 1.0 / C) <= (C + 1) * U / C).all()       # a C-term sum and a division
        assert same_bits(prob_t[1:], base_prob[1:]) and torch.equal(idx[1:], base_idx[1:]), f"{what}: a neighbour changed"
        assert int(idx[0]) == (0 if mode == 0 else int(R.pick_fp32(got[:1], u[:1], 1)[0]))
    # the last step's pick: index 0 and NaN scores for that row, and for that row only
    lg_d, rows = dev_f(logits), P.N
    idx, logp, ent = twice(lambda: final_pick(pkg, lg_d, dev_f(bias), it, rows, C, what), what)
    base = final_pick(pkg, lg_d, dev_f(open_bias), it, rows, C, what)
    assert int(idx[0]) == 0 and bool(torch.isnan(logp[0])) and bool(torch.isnan(ent[0]))
    assert torch.isfinite(logp[1:]).all() and torch.isfinite(ent[1:]).all()
    assert torch.equal(idx[1:], base[0][1:]) and same_bits(logp[1:], base[1][1:]) and same_bits(ent[1:], base[2][1:])
    assert torch.equal(final_pick(pkg, lg_d, dev_f(bias), it, rows, C, what, scores=False)[0], idx)


# ----------------------------------------------------------------------------------------------------- 4. keyed form
@pytest.mark.parametrize("B,L,C,name", [(2, 37, 20, "blosum"), (1, 600, 32, "random")])
def test_keyed_ctl_form_equals_the_buffer_ctl_form_with_the_keyed_uniforms(pkg, hip, B, L, C, name):
    P = Ctl(pkg, *posterior_case(B, L, C, name))
    bias_d = dev_f(DR.bias_inputs(P.N, C).reshape(B, L, C))
    keys = R.key_table(P.N)
    kd = dev_keys(keys)
    it = DR.inv_temp(2.0)
    for seed in R.SEEDS:
        for s in (0, 999):
            what = f"keyed ctl posterior {B}x{L}x{C} seed={seed} s={s}"
            u = R.keyed_uniforms(keys, seed, 3, s)
            assert (u[keys[:, 1] < 0] == 0).all() and len(np.unique(u)) > P.N // 2
            for b_d in (bias_d, None):
                got = twice(lambda: P.keyed(b_d, it, kd, seed, s, what), what)[0]
                assert torch.equal(got, P.ctl(b_d, it, 1, u, what, with_prob=False)[0]), what
    # and without controls it is the keyed entry point that was there
    idx = IVec(P.N)
    call(pkg, "e3d_keyed_discrete_posterior_sample", p(P.xt), p(P.lg), p(P.qs), p(P.qt), p(kd), 7, p(word(999)), idx.ptr, B, L, C)
    assert torch.equal(P.keyed(None, 1.0, kd, 7, 999, "keyed, no controls")[0], idx.get("keyed, no controls"))


# ----------------------------------------------------------------------------------------------------- 5. final pick
@pytest.mark.parametrize("C", DR.PICK_CLASSES)
@pytest.mark.parametrize("rows", DR.PICK_ROWS)
def test_final_pick(pkg, hip, rows, C):
    lg, bias = DR.pick_inputs(rows, C)
    lg_d, bias_d = dev_f(lg), dev_f(bias)
    worst_lp = worst_h = 0.0
    for T in DR.TEMPERATURES:
        it = DR.inv_temp(T)
        for b, b_d in ((bias, bias_d), (None, None)):
            what = f"final pick rows={rows} C={C} T={T} bias={b is not None}"
            idx, logp, ent = twice(lambda: final_pick(pkg, lg_d, b_d, it, rows, C, what), what)
            z = DR.effective_logits(lg, b, it)
            ref_idx, ref_lp, ref_h = DR.final_pick(z)
            assert np.array_equal(np_(idx).astype(np.int64), ref_idx), (what, "not the first maximum of z")
            D = DR.spread(z)
            lp_err, lp_bound = np.abs(np_(logp).astype(np.float64) - ref_lp), (D + C + 5) * U + 2 * U * np.abs(ref_lp)
            h_err, h_bound = np.abs(np_(ent).astype(np.float64) - ref_h), (2 * D + 2 * C + 11) * U * ref_h + (D + C + 5) * U
            r_lp, r_h = float((lp_err / lp_bound).max()), float((h_err / h_bound).max())
            worst_lp, worst_h = max(worst_lp, r_lp), max(worst_h, r_h)
            assert (lp_err <= lp_bound).all(), (what, "logp: worst |got - ref| / bound", r_lp)
            assert (h_err <= h_bound).all(), (what, "entropy: worst |got - ref| / bound", r_h)
            assert torch.equal(final_pick(pkg, lg_d, b_d, it, rows, C, what, scores=False)[0], idx), f"{what}: NULL scores"
    print(f"final pick rows={rows} C={C}: worst |got - ref| / bound = {worst_lp:.3f} (logp), {worst_h:.3f} (entropy)")


# ----------------------------------------------------------------------------------------------------- 6. chains
T_CHAIN, B_CHAIN, L_CHAIN = 8, 4, 128                              # eight steps: long enough for denoise's own capture
IDS = [11, (1 << 35) + 2, 7, 123456]
SEED = 5


@pytest.fixture(scope="module")
def seq(pkg, hip):
    """The tiny sequence model, four synthetic pockets and the uniform transition: the setup of test_known_gpu.py's
    ``seq`` fixture."""
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.sequence_model.model import PeptideDiff
    from e3diff_amd.sequence_model.utils import DiscreteUniformTransition, PredefinedNoiseScheduleDiscrete
    common = dict(hidden_size=256, num_attention_heads=4, intermediate_size=1024, num_hidden_layers=2,
                  max_position_embeddings=L_CHAIN)
    model = PeptideDiff(BertConfig(**common), BertConfig(**common, is_decoder=True, add_cross_attention=True),
                        feature_names=list(VOCAB), loss_func=torch.nn.CrossEntropyLoss(), noise_schedule="cosine",
                        timesteps=T_CHAIN)
    model.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=2))
    pk = dict(synthetic_pockets(B_CHAIN, L_CHAIN, seed=8, with_ligand_seq=True, rec_range=(20, 60)), structure_ids=None)
    valid = pk["ligand_attn_mask"].bool()
    lengths = [int(n) for n in valid.sum(dim=1)]
    assert min(lengths) >= 5 and min(lengths) < max(lengths)
    mask = torch.zeros(B_CHAIN, L_CHAIN, dtype=torch.bool)
    mask[:, 1:4] = True
    mask[:, 100] = True                                              # padding: ignored
    mask[3] = valid[3]                                               # an item with no free position
    return {"model": model.eval().to(DEV), "pk": pk, "sched": PredefinedNoiseScheduleDiscrete("cosine", T_CHAIN).to(DEV),
            "tr": DiscreteUniformTransition(20), "valid": valid, "lengths": lengths, "mask": mask,
            "allow": {2: "LIV", min(lengths): "DE"}}                 # the second position: beyond the shortest ligand


def chain(q, pk=None, **kw):
    from e3diff_amd.sequence_model.sample import denoise
    kw.setdefault("seed", SEED)
    kw.setdefault("item_ids", IDS)
    return denoise(q["pk"] if pk is None else pk, q["model"], q["sched"], q["tr"], True, timesteps=T_CHAIN, **kw)


def same_results(a, b):
    return a[:3] == b[:3] and [repr(r) for r in a[3]] == [repr(r) for r in b[3]]


def test_chain_respects_the_controls_in_every_frame(pkg, hip, seq):
    from e3diff_amd.design import DesignControls
    q = seq
    controls = DesignControls.build(q["pk"], temperature=0.7, omit="CM", allow=q["allow"])
    base = chain(q, use_graph=False)
    got = chain(q, controls=controls, use_graph=False)
    assert len(got) == 4 and got[0] == base[0] and got[1] == base[1] and got[2] != base[2]
    p2 = min(q["lengths"])
    for b, s in enumerate(got[2]):
        assert len(s) == q["lengths"][b] and not set(s) & set("CM"), (b, s)
        assert s[2] in "LIV" and (len(s) <= p2 or s[p2] in "DE"), (b, s)
    assert sum(len(s) > p2 for s in got[2]) >= 1 and sum(len(s) <= p2 for s in got[2]) >= 1
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        graph = chain(q, controls=controls, use_graph=True)
    assert not [str(w.message) for w in caught if "HIP-graph capture" in str(w.message)]
    assert same_results(graph, got)
    assert same_results(chain(q, controls=controls, trim_padding=True), got)
    assert same_results(chain(q, controls=controls, pack=True), got)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert same_results(chain(q, controls=controls, pack=True, use_graph=True), got)
    rev_pk = {k: (v.flip(0) if torch.is_tensor(v) else v) for k, v in q["pk"].items()}
    rev = chain(q, rev_pk, controls=DesignControls.build(rev_pk, temperature=0.7, omit="CM", allow=q["allow"]), item_ids=IDS[::-1])
    assert rev[2][::-1] == got[2] and rev[1][::-1] == got[1]
    # an item's design depends on its own controls only: another item's allow list leaves the others alone
    own = DesignControls.build(q["pk"], temperature=0.7, omit="CM", allow=lambda i: {**q["allow"], **({0: "W"} if i == 1 else {})})
    per_item = chain(q, controls=own)
    assert per_item[2][1][0] == "W" and [s for b, s in enumerate(per_item[2]) if b != 1] == [s for b, s in enumerate(got[2]) if b != 1]
    # the temperature reaches the steps s > 0
    assert chain(q, controls=DesignControls.build(q["pk"], temperature=0.25))[2] != base[2]
    # whatever the chain without controls likes best, forbidden: none of it comes back
    used = "".join(base[2])
    liked = "".join(sorted(set(used), key=lambda a: (-used.count(a), a))[:10])
    none_liked = chain(q, controls=DesignControls.build(q["pk"], omit=liked))
    assert liked and not set("".join(none_liked[2])) & set(liked), (liked, none_liked[2])


def test_no_controls_and_inactive_controls_are_the_chain_without_the_argument(pkg, hip, seq):
    from e3diff_amd.design import DesignControls
    q = seq
    for frame in ({}, {"use_graph": True}, {"pack": True}):
        base = chain(q, **frame)
        assert same_results(chain(q, controls=None, **frame), base)
        assert same_results(chain(q, controls=DesignControls.build(q["pk"]), **frame), base)
        assert same_results(chain(q, controls=DesignControls.build(q["pk"], allow={127: "A"}), **frame), base)
    # unseeded too: the same torch seed, the same chain and the same generator state afterwards
    torch.manual_seed(3)
    base = chain(q, seed=None, item_ids=None, use_graph=False)
    state = torch.cuda.get_rng_state(DEV)
    torch.manual_seed(3)
    assert same_results(chain(q, seed=None, item_ids=None, use_graph=False, controls=DesignControls.build(q["pk"])), base)
    assert torch.equal(torch.cuda.get_rng_state(DEV), state)


def test_held_positions_win_over_the_controls(pkg, hip, seq):
    from e3diff_amd.design import DesignControls
    q = seq
    native = chain(q, use_graph=False)[1]
    omit = "".join(sorted({native[0][c] for c in (1, 2, 3)}))        # the held residues of item 0 are forbidden everywhere
    controls = DesignControls.build(q["pk"], temperature=0.7, omit=omit)
    got = chain(q, controls=controls, known_mask=q["mask"], use_graph=False)
    for b, (true, pred) in enumerate(zip(got[1], got[2])):
        n = q["lengths"][b]
        held = list(range(n)) if b == 3 else [1, 2, 3]
        assert all(pred[c] == true[c] for c in held), b
        assert not any(pred[c] in omit for c in range(n) if c not in held), (b, pred)
    assert all(got[2][0][c] in omit for c in (1, 2, 3)) and np.isnan(got[3][3])
    assert same_results(chain(q, controls=controls, known_mask=q["mask"], use_graph=True), got)
    assert same_results(chain(q, controls=controls, known_mask=q["mask"], pack=True), got)


def test_details_hold_the_scores(pkg, hip, seq):
    from e3diff_amd.design import DesignControls
    q = seq
    controls = DesignControls.build(q["pk"], temperature=0.7, omit="CM", allow=q["allow"])
    for kw in (dict(controls=controls, known_mask=q["mask"]), dict(known_mask=q["mask"]), dict(controls=controls, pack=True)):
        d = {}
        got = chain(q, details=d, **kw)
        assert same_results(got, chain(q, **kw)), "details changed the design"
        assert set(d) == {"logp", "entropy", "score"}
        logp, ent, score = d["logp"], d["entropy"], d["score"]
        assert logp.shape == ent.shape == (B_CHAIN, L_CHAIN) and score.shape == (B_CHAIN,)
        assert torch.isnan(logp[~q["valid"]]).all() and torch.isnan(ent[~q["valid"]]).all()
        assert torch.isfinite(logp[q["valid"]]).all() and (logp[q["valid"]] <= 0).all()
        assert torch.isfinite(ent[q["valid"]]).all() and (ent[q["valid"]] >= 0).all() and (ent[q["valid"]] <= np.log(20) + 1e-5).all()
        held = q["mask"] & q["valid"] if "known_mask" in kw else torch.zeros_like(q["valid"])
        for b in range(B_CHAIN):
            des = q["valid"][b] & ~held[b]
            if not bool(des.any()):
                assert b == 3 and bool(torch.isnan(score[b]))
                continue
            want = float((-logp[b][des].double()).mean())
            assert abs(float(score[b]) - want) <= 1e-6 * max(1.0, abs(want)), (b, float(score[b]), want)
        assert ("known_mask" in kw) == bool(torch.isnan(score[3]))
    # forbidden classes carry no probability: at an allowed position the entropy stays below log 3
    d = {}
    chain(q, details=d, controls=controls)
    assert (d["entropy"][:, 2] <= np.log(3) + 1e-5).all()


# ----------------------------------------------------------------------------------------------------- 7. entry point
def test_sequence_entry_point_takes_the_controls(pkg, hip, tmp_path, monkeypatch):
    import pandas as pd
    from torch.utils.data import DataLoader
    from e3diff_amd import biolip
    from e3diff_amd.sequence_model import sample as Q
    from e3diff_amd.sequence_model.dataset import LigandBindingSiteDataset
    from e3diff_amd.sequence_model.utils import DiscreteUniformTransition
    path = biolip.write_synthetic(str(tmp_path / "biolip.pt"), 2, seed=4)
    out = tmp_path / "output.pkl"
    for key, value in (("timesteps", 6), ("max_seq_len", 64), ("batch_size", 2), ("num_hidden_layers", 2), ("hidden_size", 256),
                       ("num_heads", 4)):
        monkeypatch.setitem(Q.CONFIG, key, value)
    monkeypatch.setattr(Q, "DATA_PATH", path)
    monkeypatch.setattr(Q, "OUTPUT_PATH", str(out))
    monkeypatch.setattr(Q, "MODEL_PATH", "")
    # both records, whatever the split would leave in "test", and no loader processes
    monkeypatch.setattr(Q, "get_dataloader", lambda file_path: DataLoader(
        LigandBindingSiteDataset(file_path, None, Q.CONFIG["max_seq_len"], Q.CONFIG["pocket_ext"]), batch_size=2, shuffle=False))

    def run(**kw):
        torch.manual_seed(3)                                        # the model's initial weights
        res = Q.run(DiscreteUniformTransition(20), seed=31, **kw)
        assert res.equals(pd.read_pickle(out))
        return res
    free = run()
    assert list(free.columns) == ["structure_ids", "true_sequence", "predict_sequence", "recovery_rate"] and len(free) == 2
    used = "".join(free["predict_sequence"])
    omit = "".join(sorted(set(used), key=lambda a: (-used.count(a), a))[:10])      # what the free run likes best
    monkeypatch.setenv("E3D_SAMPLE_OMIT", omit)
    monkeypatch.setattr(Q, "OMIT", omit)                            # the module reads the variable when it is imported
    kept = run()
    assert list(kept.columns) == list(free.columns), "no score column without scores=True"
    assert list(kept["true_sequence"]) == list(free["true_sequence"])
    for s in kept["predict_sequence"]:
        assert s and not set(s) & set(omit), (omit, s)
    scored = run(scores=True)
    assert list(scored.columns) == list(free.columns) + ["score"]
    assert list(scored["predict_sequence"]) == list(kept["predict_sequence"])
    assert np.isfinite(scored["score"]).all() and (scored["score"] >= 0).all()
    # the keywords win over the variable, and reach the chain
    by_kw = run(omit="W", allow={0: "WY", 1: "KR"}, temperature=0.5, scores=True)
    for s in by_kw["predict_sequence"]:
        assert s[0] == "Y" and s[1] in "KR" and "W" not in s
    with pytest.raises(ValueError, match="item 0, position 0"):
        run(omit="W", allow={0: "W"})
