"""GPU: scoring supplied sequences (csrc/sampler.hip, "scoring supplied sequences"; sequence_model/sample.py::
score_sequences).  The three entry points through the C ABI against tests/score_ref.py -- the keyed forward noising at
per-item levels and the fixed-shape item sums bit for bit, the score rows' p against the existing posterior kernel bit
for bit and their q, KL term and cross-entropy against float64 -- then ``score_sequences`` end to end on the tiny model of
tests/test_design_gpu.py, and the command-line tool.  Plumbing and conventions are those of
tests/test_sampler_forms_gpu.py: outputs between guard words, NaN after every input, every case run twice.

Bounds (u = 2^-24).  The float64 reference is fed the same fp32 inputs; logit spreads D = max - min of a row stay <= 60
in the bounded cases, so nothing underflows on either side.
  * Probabilities.  p: |got - ref| <= (7 C + 20 + 4 D) u ref =: e_p ref, the bound tests/test_sampler_forms_gpu.py derives
    for the posterior; it is the same arithmetic (p_out is compared with that kernel bit for bit as well).  q is the
    same expression under a one-hot prediction: the softmax roundings drop out (D = 0) and every other operation is
    counted as there (the kernel computes only the one non-zero term of the mixture, fewer roundings, not more):
    |got - ref| <= (7 C + 20) u ref =: e_q ref.  An exact zero of a table gives an exact zero on both sides.
  * Cross-entropy  nll = lse - d, d = logit[x0] - mx, lse = logf(se), se the C-term sequential sum of e[c] = expf(l[c] - mx):
      d:    one subtraction, relative u, at most u D absolute
      e[c]: u D from its argument (absolute there, relative on the value) + 2 u for expf (good to 1 ulp)  ->  (D + 2) u
      se:   non-negative terms, so relative errors do not grow; C - 1 additions                           ->  (D + C + 1) u
      lse:  a relative error of se is an absolute one of its logarithm; logf adds 2 u |lse|    ->  (D + C + 1) u + 2 u |lse|
      nll:  the subtraction u |nll|; 0 <= lse <= nll because d <= 0
    so |nll - ref| <= (2 D + C + 5) u + 3 u ref                                     (four added for second order).
  * KL term  sum_c t[c], t[c] = q[c] (logf(q[c]) - logf(p[c])) over q[c] > 0, added in class order.  Its terms change
    sign, so the bound is absolute.  With g[c] = ln q[c] - ln p[c]:
      logf(q[c]): e_q from its argument + 2 u |ln q[c]|;  logf(p[c]): e_p + 2 u |ln p[c]|;  their difference: u |g[c]|
                                                      ->  |dg[c]| <= e_q + e_p + 2 u (|ln q[c]| + |ln p[c]|) + u |g[c]|
      t[c]:  q[c] dg[c]  +  e_q |t[c]| from q  +  u |t[c]| for the product (none when it is fused into the sum)
      the sum: C - 1 additions, each at most u of a partial sum <= sum |t[c]|
    so |term - ref| <= sum_c q[c] (e_q + e_p + 2 u (|ln q[c]| + |ln p[c]|) + u |g[c]|)  +  (e_q + (C + 4) u) sum_c |t[c]|
    (four added for second order).  With p == q to the last bit the kernel returns exactly 0.
  * +inf.  A class with q > 0 and p == 0 makes the term +inf, on both sides or on neither when the reference is fed the
    kernel's fp32 softmax (zero there means expf underflowed, the same in numpy's fp32); never NaN.
  * Item sums: bit for bit against the fixed-shape fp32 restatement; against float64 within L u sum |v| (at most L - 1
    additions, each at most u of a partial sum of absolute values).
  * End to end: terms[s, b] against the float64 rows evaluated on the returned z_t and logits, summed over the scored
    positions: the sum of the rows' bounds above + L u sum |row value|.

Measured on an MI355X, worst |got - ref| / bound over all cases of a test (each test prints its own; DESIGN.md, "Scoring
sequences", records them too):
  score rows, q              0.052  (2 x 5 x 3; 0.040 at 2 x 37 x 20, 0.048 at 1 x 257 x 20, 0.036 at 1 x 600 x 32)
  score rows, KL term        0.021  (2 x 5 x 3; 0.011 at 2 x 37 x 20, 0.013 at 1 x 257 x 20, 0.012 at 1 x 600 x 32)
  score rows, cross-entropy  0.213  (1 x 600 x 32; 0.171 at 2 x 5 x 3, 0.179 at 2 x 37 x 20, 0.212 at 1 x 257 x 20)
  item sums against float64  0.007  (L = 63, 64, 65; 0.001 at L = 257): the count is a worst case over L roundings of one sign
  end to end                 0.035 (terms), 0.015 (nll), uniform transition; 0.009 and 0.015 with the BLOSUM transition
Everything else in this module is compared bit for bit, or is a statement about strings.
"""
import numpy as np
import pytest
import torch

import sampler_ref as R
import score_ref as SR
from helpers import seeded_state_dict, synthetic_pockets
from test_rowops_forms_gpu import DEV, Out, Vec, call, p, twice
from test_sampler_forms_gpu import IVec, dev_f, dev_i, dev_keys, np_, same_bits, take, word
from test_sampler_ref_cpu import posterior_case, transitions

pytestmark = pytest.mark.gpu

U = R.U
CASES = [(B, L, C, "blosum" if C == 20 else "random") for B, L, C in SR.SHAPES]


def dev_u8(a):
    return dev_i(np.asarray(a).astype(np.int64), 0, torch.uint8)


# ----------------------------------------------------------------------------------------------------- 1. forward levels
def forward_levels(pkg, x0_d, q_d, keys_d, steps, max_step, seed, N, L, C, what):
    idx = IVec(N * L)
    steps_d = dev_i(np.asarray(steps), 0, torch.int64)
    call(pkg, "e3d_keyed_discrete_forward_levels", p(x0_d), p(q_d), p(keys_d), p(steps_d), max_step, seed, idx.ptr, N, L, C)
    return (idx.get(what),)


@pytest.mark.parametrize("B,L,C,name", CASES)
def test_forward_levels(pkg, hip, B, L, C, name):
    x0, Qtb = R.discrete_q_inputs(B, L, C, transitions("blosum", B)[1] if C == 20 else None)
    N = B * L
    ids = R.IDS[2:2 + B]
    keys = R.padded_keys(ids, L)
    if N > 8:
        keys[2] = keys[N // 2] = (9, -1)                                   # rows of no item
    none = (keys[:, 1] < 0) | (x0.reshape(-1) < 0)
    assert (x0 < 0).any() and (Qtb == 0).any()
    x0_d, q_d, keys_d = dev_i(x0, -1), dev_f(Qtb), dev_keys(keys)
    ones = dev_u8(np.ones(N))
    for seed in R.SEEDS:
        # equal steps: the held-row compose with a full mask, bit for bit
        for s in (0, 999, 65535):
            what = f"forward levels {B}x{L}x{C} seed={seed} s={s}"
            got = twice(lambda: forward_levels(pkg, x0_d, q_d, keys_d, [s] * B, 65535, seed, B, L, C, what), what)[0]
            base, s_d = torch.zeros(N, dtype=torch.int32, device=DEV), word(s)
            call(pkg, "e3d_keyed_discrete_known_compose", p(base), p(x0_d), p(ones), p(q_d), p(keys_d), seed, p(s_d), B, L, C)
            assert torch.equal(got, base), f"{what}: differs from e3d_keyed_discrete_known_compose"
            assert (np_(got)[none] == 0).all(), f"{what}: a padding row or a row of no item is not class 0"
        # mixed steps: the reference's classes exactly
        steps = (7, 65535)[:B] if B > 1 else (31,)
        what = f"forward levels {B}x{L}x{C} seed={seed} steps={steps}"
        got = np_(twice(lambda: forward_levels(pkg, x0_d, q_d, keys_d, steps, 65535, seed, B, L, C, what), what)[0])
        want = SR.forward_levels(x0, Qtb, keys, seed, steps).reshape(-1)
        assert np.array_equal(got.astype(np.int64), want), (what, np.flatnonzero(got != want)[:8].tolist())
        assert (got[none] == 0).all() and len(np.unique(got[~none])) > 1
        # a step beyond the caller's bound: that item is rows of no item
        low = np_(forward_levels(pkg, x0_d, q_d, keys_d, steps, 7, seed, B, L, C, what)[0])
        assert (low == 0).all() if B == 1 else (np.array_equal(low[:L], got[:L]) and (low[L:] == 0).all())


# ----------------------------------------------------------------------------------------------------- 2. score rows
class Rows:
    """The inputs of one score case on the device and the entry point."""

    def __init__(self, pkg, xt, x0, logits, Qsb, Qtb, fin=None):
        self.pkg, (self.B, self.L), self.C = pkg, xt.shape, Qsb.shape[-1]
        self.N = self.B * self.L
        self.xt, self.x0, self.lg = dev_i(xt, 0), dev_i(x0, -1), dev_f(logits)
        self.qs, self.qt = dev_f(Qsb), dev_f(Qtb)
        self.fin = dev_u8(np.zeros(self.B) if fin is None else fin)

    def run(self, what, probs=True, qs=None, qt=None):
        term, nll = Vec(self.N), Vec(self.N)
        po, qo = (Out(self.N, self.C), Out(self.N, self.C)) if probs else (None, None)
        call(self.pkg, "e3d_discrete_score_rows", p(self.xt), p(self.x0), p(self.lg), p(self.qs if qs is None else qs),
             p(self.qt if qt is None else qt), p(self.fin), term.ptr, nll.ptr, po.ptr if probs else None,
             qo.ptr if probs else None, self.B, self.L, self.C)
        return (take(term, what), take(nll, what)) + ((take(po, what), take(qo, what)) if probs else ())


def posterior_prob(pkg, xt, logits, Qsb, Qtb, what):
    B, L = xt.shape
    C = Qsb.shape[-1]
    idx, prob = IVec(B * L), Out(B * L, C)
    ins = (dev_i(xt, 0), dev_f(logits), dev_f(Qsb), dev_f(Qtb))             # held until the call has run
    call(pkg, "e3d_discrete_posterior_sample", *(p(t) for t in ins), None, 0, idx.ptr, prob.ptr, B, L, C)
    idx.get(what)
    return take(prob, what)


def p_cases():
    for B, L, C, name in CASES:
        yield f"{B}x{L}x{C} {name}", posterior_case(B, L, C, name)
    for C in (3, 32):
        yield f"zero total C={C}", R.zero_total_inputs(2, 37, C)
        xt, logits, Qsb, Qtb = R.posterior_inputs(2, 37, C)
        yield f"exact zeros in Qtb C={C}", (xt, logits, Qsb, R.with_exact_zeros(Qtb))
        yield f"exact zeros in Qsb C={C}", (xt, logits, R.with_exact_zeros(Qsb), Qtb)


def test_p_out_is_the_posterior_kernels_prob_out_bit_for_bit(pkg, hip):
    for tag, (xt, logits, Qsb, Qtb) in p_cases():
        B, L = xt.shape
        C = Qsb.shape[-1]
        what = f"score rows p_out, {tag}"
        want = posterior_prob(pkg, xt, logits, Qsb, Qtb, what)
        x0 = SR.score_x0(B, L, C)
        got = twice(lambda: Rows(pkg, xt, np.maximum(x0, 0), logits, Qsb, Qtb).run(what), what)[2]
        assert same_bits(got, want), f"{what}: differs from e3d_discrete_posterior_sample's prob_out"
        part = Rows(pkg, xt, x0, logits, Qsb, Qtb).run(what)[2]
        live = torch.from_numpy(x0.reshape(-1) >= 0).to(DEV)
        assert same_bits(part[live], want[live]) and bool(torch.isnan(part[~live]).all()), what


@pytest.mark.parametrize("B,L,C,name", CASES)
def test_score_rows_against_float64(pkg, hip, B, L, C, name):
    xt, logits, Qsb, Qtb = posterior_case(B, L, C, name)
    x0 = SR.score_x0(B, L, C)
    fin = SR.final_flags(B)
    live = x0.reshape(-1) >= 0
    last = np.repeat(fin != 0, L)                                           # rows of an is_final item
    sure = np.zeros((B, L, C), dtype=np.float32)                            # the prediction = the true residue: KL about 0
    np.put_along_axis(sure, np.maximum(x0, 0)[..., None].astype(np.int64), np.float32(60.0), axis=-1)
    q = SR.q_post(xt, x0, Qsb, Qtb)
    worst = {"q": 0.0, "term": 0.0, "nll": 0.0}
    for tag, lg in (("random logits", logits), ("sure logits", sure)):
        assert SR.spread(lg, C).max() <= SR.MAX_SPREAD
        what = f"score rows {B}x{L}x{C} {name}, {tag}"
        P = Rows(pkg, xt, x0, lg, Qsb, Qtb, fin)
        term_t, nll_t, p_t, q_t = twice(lambda: P.run(what), what)
        term, nll, pg, qg = (np_(t).astype(np.float64) for t in (term_t, nll_t, p_t, q_t))
        # rows without a true residue
        assert np.isnan(term[~live]).all() and np.isnan(nll[~live]).all() and np.isnan(qg[~live]).all()
        assert np.isfinite(term[live]).all() and np.isfinite(nll[live]).all()
        # cross-entropy, every live row
        ref_nll = SR.nll(lg, x0)
        err, bound = np.abs(nll - ref_nll)[live], SR.nll_bound(lg, ref_nll, C)[live]
        worst["nll"] = max(worst["nll"], float((err / bound).max()))
        assert (err <= bound).all(), (what, "nll: worst |got - ref| / bound", float((err / bound).max()))
        # is_final items: term == nll bit for bit, no probabilities, the tables unread
        fl = torch.from_numpy(last).to(DEV)
        assert same_bits(term_t[fl], nll_t[fl]), f"{what}: an is_final item's term is not its nll"
        assert bool(torch.isnan(p_t[fl]).all()) and bool(torch.isnan(q_t[fl]).all())
        if last.any():
            poison_s, poison_t = P.qs.clone(), P.qt.clone()
            poison_s[torch.from_numpy(fin != 0)] = float("nan")
            poison_t[torch.from_numpy(fin != 0)] = float("nan")
            for a, b in zip(P.run(what, qs=poison_s, qt=poison_t), (term_t, nll_t, p_t, q_t)):
                assert same_bits(a, b), f"{what}: an is_final item read its tables"
        # q, p and the KL term on the other live rows
        rows = live & ~last
        p_ref = SR.p_theta(xt, lg, Qsb, Qtb)
        e_q = np.abs(qg - q)[rows]
        b_q = ((7 * C + 20) * U * q)[rows]
        assert (e_q <= b_q).all(), (what, "q: worst |got - ref| / bound", float((e_q / b_q).max()))
        worst["q"] = max(worst["q"], float((e_q / b_q).max()))
        assert (np.abs(pg - p_ref)[rows] <= (SR.prob_eps(lg, C)[:, None] * p_ref)[rows]).all(), what
        ref, bound = SR.kl(q, p_ref)[rows], SR.kl_bound(q, p_ref, lg, C)[rows]
        err = np.abs(term[rows] - ref)
        worst["term"] = max(worst["term"], float((err / bound).max()))
        assert (err <= bound).all(), (what, "term: worst |got - ref| / bound", float((err / bound).max()))
        assert (term[rows] >= -bound).all()
        # without the probabilities: the same terms
        for a, b in zip(P.run(what, probs=False), (term_t, nll_t)):
            assert same_bits(a, b), f"{what}: p_out == NULL changes the terms"
    print(f"score rows {B}x{L}x{C} {name}: worst |got - ref| / bound = {worst['q']:.3f} (q), {worst['term']:.3f} (KL term), "
          f"{worst['nll']:.3f} (cross-entropy)")


def test_kl_is_exactly_zero_where_p_equals_q(pkg, hip):
    """The true residue 200 above every other logit: the fp32 softmax is exactly its one-hot (expf(-200) == 0), the other
    classes add exact zeros to the mixture, so p == q bit for bit and the term is exactly 0."""
    B, L, C = 2, 37, 20
    xt, _, Qsb, Qtb = posterior_case(B, L, C, "blosum")
    x0 = np.maximum(SR.score_x0(B, L, C), 0)
    logits = np.zeros((B, L, C), dtype=np.float32)
    np.put_along_axis(logits, x0[..., None].astype(np.int64), np.float32(200.0), axis=-1)
    term, nll, p_t, q_t = Rows(pkg, xt, x0, logits, Qsb, Qtb).run("one-hot prediction")
    assert same_bits(p_t, q_t) and bool((term == 0).all()) and bool((nll == 0).all())


@pytest.mark.parametrize("tables", ["random", "identity"])
def test_a_true_residue_300_below_the_maximum_is_inf_or_finite_never_nan(pkg, hip, tables):
    B, L, C = 2, 37, 20
    xt, logits, Qsb, Qtb = R.posterior_inputs(B, L, C)
    x0 = np.maximum(SR.score_x0(B, L, C), 0)
    logits = np.clip(logits, -2.0, 2.0).astype(np.float32)
    np.put_along_axis(logits, x0[..., None].astype(np.int64), logits.max(-1, keepdims=True) - np.float32(300.0), axis=-1)
    if tables == "identity":                                               # the clean level: p and q are one-hots or uniform
        Qsb = np.broadcast_to(np.eye(C, dtype=np.float32), (B, C, C)).copy()
    what = f"x0 logit 300 below the maximum, {tables} Qsb"
    term_t, nll_t = twice(lambda: Rows(pkg, xt, x0, logits, Qsb, Qtb).run(what, probs=False), what)
    term, nll = np_(term_t).astype(np.float64), np_(nll_t).astype(np.float64)
    d = logits - logits.max(-1, keepdims=True)
    e32 = np.exp(d.astype(np.float32))                                      # the fp32 softmax: exp(-300) is 0 there
    assert e32.dtype == np.float32 and (np.take_along_axis(e32, x0[..., None].astype(np.int64), -1) == 0).all()
    pred = e32 / e32.sum(-1, keepdims=True, dtype=np.float32)
    q, p_ref = SR.q_post(xt, x0, Qsb, Qtb), SR.p_theta_from_pred(xt, pred, Qsb, Qtb)
    ref = SR.kl(q, p_ref)
    assert not np.isnan(term).any() and not np.isnan(ref).any()
    assert np.array_equal(np.isinf(term), np.isinf(ref)) and (term[np.isinf(term)] > 0).all(), what
    assert np.isinf(ref).any() == (tables == "identity")
    fin = np.isfinite(ref)
    assert fin.any() and (np.abs(term[fin] - ref[fin]) <= SR.kl_bound(q, p_ref, logits, C)[fin]).all(), what
    ref_nll = SR.nll(logits, x0)
    assert (np.abs(nll - ref_nll) <= SR.nll_bound(logits, ref_nll, C)).all() and (nll > 295).all()


# ----------------------------------------------------------------------------------------------------- 3. item sums
def item_sums(pkg, values, mask, what):
    N, L = values.shape
    sums, counts = Vec(N), IVec(N)
    v_d, m_d = dev_f(values), dev_u8(mask)
    call(pkg, "e3d_masked_item_sums", p(v_d), p(m_d), sums.ptr, counts.ptr, N, L)
    return take(sums, what), counts.get(what)


@pytest.mark.parametrize("L", [1, 63, 64, 65, 257])
def test_item_sums(pkg, hip, L):
    N = 5
    rng = np.random.default_rng(100 + L)
    v = (rng.standard_normal((N, L)) * 10 ** rng.uniform(-3, 3, (N, L))).astype(np.float32)
    m = rng.random((N, L)) < 0.7
    m[:, 0] = True
    m[1] = False                                                            # an empty mask
    what = f"item sums L={L}"
    sums_t, counts_t = twice(lambda: item_sums(pkg, v, m, what), what)
    sums, counts = np_(sums_t), np_(counts_t)
    worst = 0.0
    for n in range(N):
        want, cnt = SR.item_sum_fp32(v[n], m[n])
        assert sums[n].view(np.int32) == want.view(np.int32) and counts[n] == cnt, (what, n, float(sums[n]), float(want))
        exact, bound = v[n].astype(np.float64)[m[n]].sum(), L * U * np.abs(v[n].astype(np.float64))[m[n]].sum()
        assert abs(float(sums[n]) - exact) <= bound
        worst = max(worst, abs(float(sums[n]) - exact) / bound) if bound else worst
    assert sums[1].view(np.int32) == 0 and counts[1] == 0                   # +0, not -0
    # NaN in the masked-out places and in the padding, padded to 2 L, alone, reversed: the same bits
    wide = np.full((N, 2 * L), np.nan, dtype=np.float32)
    wide[:, :L] = np.where(m, v, np.float32(np.nan))
    wide_m = np.concatenate([m, np.zeros((N, L), dtype=bool)], axis=1)
    for vv, mm, order, tag in ((wide, wide_m, slice(None), "padded to 2 L"), (v[::-1].copy(), m[::-1].copy(), slice(None, None, -1), "reversed"),
                               (wide[::-1].copy(), wide_m[::-1].copy(), slice(None, None, -1), "padded and reversed")):
        s2, c2 = item_sums(pkg, vv, mm, f"{what}, {tag}")
        assert same_bits(s2.flip(0) if order != slice(None) else s2, sums_t), f"{what}: {tag} changes a sum"
        assert torch.equal(c2.flip(0) if order != slice(None) else c2, counts_t)
    for n in range(N):
        s1, c1 = item_sums(pkg, v[n:n + 1], m[n:n + 1], f"{what}, alone")
        assert same_bits(s1, sums_t[n:n + 1]) and int(c1[0]) == int(counts[n]), f"{what}: item {n} alone differs"
    print(f"{what}: worst |got - float64| / bound = {worst:.3f}")


# ----------------------------------------------------------------------------------------------------- 4. end to end
T_CHAIN, B_CHAIN, L_CHAIN = 8, 4, 128
IDS = [11, (1 << 35) + 2, 7, 123456]
SEED = 5


@pytest.fixture(scope="module")
def seq(pkg, hip):
    """The tiny sequence model and the four synthetic pockets of tests/test_design_gpu.py's ``seq`` fixture, both
    transitions, the native strings and a cache of the runs the tests below share."""
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.sequence_model.dataset import AA_VOCAB as VOCAB
    from e3diff_amd.sequence_model.model import PeptideDiff
    from e3diff_amd.sequence_model.utils import BlosumTransition, DiscreteUniformTransition, PredefinedNoiseScheduleDiscrete
    common = dict(hidden_size=256, num_attention_heads=4, intermediate_size=1024, num_hidden_layers=2,
                  max_position_embeddings=L_CHAIN)
    model = PeptideDiff(BertConfig(**common), BertConfig(**common, is_decoder=True, add_cross_attention=True),
                        feature_names=list(VOCAB), loss_func=torch.nn.CrossEntropyLoss(), noise_schedule="cosine",
                        timesteps=T_CHAIN)
    model.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=2))
    pk = dict(synthetic_pockets(B_CHAIN, L_CHAIN, seed=8, with_ligand_seq=True, rec_range=(20, 60)), structure_ids=None)
    valid = pk["ligand_attn_mask"].bool()
    x0 = torch.where(valid, pk["ligand_seq"].argmax(-1), torch.full((), -1)).numpy()
    native = ["".join(VOCAB[j] for j in row[row >= 0]) for row in x0]
    return {"model": model.eval().to(DEV), "pk": pk, "sched": PredefinedNoiseScheduleDiscrete("cosine", T_CHAIN).to(DEV),
            "uniform": DiscreteUniformTransition(20), "blosum": BlosumTransition(x_classes=20), "valid": valid, "x0": x0,
            "native": native, "lengths": [int(n) for n in valid.sum(dim=1)], "cache": {}}


def score(q, pk=None, transition="uniform", cached=None, **kw):
    """score_sequences on the fixture; ``cached``: a key under which the (result, details) pair is kept for other tests."""
    from e3diff_amd.sequence_model.sample import score_sequences
    if cached is not None and cached in q["cache"]:
        return q["cache"][cached]
    kw.setdefault("seed", SEED)
    if kw["seed"] is not None:
        kw.setdefault("item_ids", IDS)
    details = {} if kw.pop("want_details", False) else None
    out = score_sequences(q["pk"] if pk is None else pk, q["model"], q["sched"], q[transition], kw.pop("sequences", None),
                          timesteps=T_CHAIN, details=details, **kw)
    if cached is not None:
        q["cache"][cached] = (out, details)
    return out, details


def tables(q, transition, s):
    """fp32 (Qsb, Qtb) [B, C, C] of step index s, computed as the sampler computes them."""
    sa = torch.full((B_CHAIN, 1), float(s), device=DEV)
    tr, sched = q[transition], q["sched"]
    return (np_(tr.get_Qt_bar(sched.get_alpha_bar(t_normalized=sa / T_CHAIN), DEV)),
            np_(tr.get_Qt_bar(sched.get_alpha_bar(t_normalized=(sa + 1) / T_CHAIN), DEV)))


def check_against_reference(q, out, details, transition, what):
    """Every term and nll of ``out`` against float64 on the returned z_t and logits; returns the worst error / bound."""
    valid, x0, C = q["valid"].numpy(), q["x0"], 20
    z_t, logits = details["z_t"].numpy(), details["logits"].numpy()
    assert z_t.shape == (len(out["levels"]), B_CHAIN, L_CHAIN) and logits.shape == z_t.shape + (C,)
    assert (z_t[:, ~valid] == 0).all()
    worst = [0.0, 0.0]
    for i, s in enumerate(out["levels"]):
        lg = np.where(valid[..., None], logits[i], np.float32(0))
        assert SR.spread(lg, C).max() <= SR.MAX_SPREAD
        ref_nll = SR.nll(lg, x0)
        b_nll = SR.nll_bound(lg, ref_nll, C)
        if s == 0:
            ref, bound = ref_nll, b_nll
        else:
            Qsb, Qtb = tables(q, transition, s)
            qq, pp = SR.q_post(z_t[i], x0, Qsb, Qtb), SR.p_theta(z_t[i], lg, Qsb, Qtb)
            ref, bound = SR.kl(qq, pp), SR.kl_bound(qq, pp, lg, C)
        for k, (key, r, b) in enumerate((("terms", ref, bound), ("nll", ref_nll, b_nll))):
            r, b = (np.where(valid, v.reshape(B_CHAIN, L_CHAIN), 0.0) for v in (r, b))
            total, tb = r.sum(1), b.sum(1) + L_CHAIN * U * np.abs(r).sum(1)
            err = np.abs(out[key][i].numpy() - total)
            worst[k] = max(worst[k], float((err / tb).max()))
            assert (err <= tb).all(), (what, key, "step", s, "worst |got - ref| / bound", float((err / tb).max()))
    return worst


def test_terms_and_nll_against_the_reference_in_every_chunking_and_frame(pkg, hip, seq):
    q = seq
    z_first, worst = None, [0.0, 0.0]
    for lpl in (1, 3, 8):
        for trim in (False, True):
            what = f"score_sequences levels_per_launch={lpl} trim_padding={trim}"
            out, det = score(q, cached=("all", lpl, trim), levels_per_launch=lpl, trim_padding=trim, want_details=True)
            assert out["levels"] == list(range(T_CHAIN)) and set(det) == {"z_t", "logits"}
            w = check_against_reference(q, out, det, "uniform", what)
            worst = [max(a, b) for a, b in zip(worst, w)]
            z_first = det["z_t"] if z_first is None else z_first
            assert torch.equal(det["z_t"], z_first), f"{what}: z_t depends on the chunking or the frame"
    print(f"score_sequences, uniform transition: worst |got - ref| / bound = {worst[0]:.3f} (terms), {worst[1]:.3f} (nll)")
    out, det = score(q, transition="blosum", levels_per_launch=3, want_details=True)
    w = check_against_reference(q, out, det, "blosum", "score_sequences, BLOSUM transition")
    print(f"score_sequences, BLOSUM transition: worst |got - ref| / bound = {w[0]:.3f} (terms), {w[1]:.3f} (nll)")
    assert torch.isfinite(out["score"]).all() and not torch.equal(det["z_t"], z_first)


def test_an_items_score_does_not_depend_on_its_place_in_the_batch(pkg, hip, seq):
    q = seq
    out, det = score(q, cached=("all", 3, False), levels_per_launch=3, trim_padding=False, want_details=True)
    rev_pk = {k: (v.flip(0) if torch.is_tensor(v) else v) for k, v in q["pk"].items()}
    rev, rdet = score(q, rev_pk, levels_per_launch=3, item_ids=IDS[::-1], want_details=True)
    assert torch.equal(rdet["z_t"].flip(1), det["z_t"]), "z_t depends on the item's place"
    for key in ("bound", "score", "prior", "n"):
        assert torch.equal(rev[key].flip(0), out[key]), key
    for key in ("terms", "nll"):
        assert torch.equal(rev[key].flip(1), out[key]), key
    assert torch.equal(torch.nan_to_num(rev["per_residue"].flip(0), nan=-1.0), torch.nan_to_num(out["per_residue"], nan=-1.0))
    # other item ids: other draws
    assert not torch.equal(score(q, levels_per_launch=3, item_ids=[1, 2, 3, 4], want_details=True)[1]["z_t"], det["z_t"])


def test_level_sets_weights_and_the_returned_record(pkg, hip, seq):
    q = seq
    out, det = score(q, cached=("all", 3, False), levels_per_launch=3, trim_padding=False, want_details=True)
    valid, n = q["valid"], torch.tensor(q["lengths"], dtype=torch.int32)
    assert set(out) == {"bound", "score", "prior", "n", "stderr", "terms", "nll", "levels", "per_residue"}
    assert all(not out[k].is_cuda for k in out if k != "levels")
    assert out["terms"].shape == out["nll"].shape == (T_CHAIN, B_CHAIN) and out["per_residue"].shape == (B_CHAIN, L_CHAIN)
    assert torch.equal(out["n"], n) and torch.isnan(out["stderr"]).all() and torch.isfinite(out["score"]).all()
    # levels=None: w = 1, the bound is the prior and every term
    want = out["prior"] + out["terms"][0] + 1.0 * out["terms"][1:].sum(dim=0)
    assert (out["bound"] - want).abs().max() <= 1e-12 * want.abs().max()
    assert (out["score"] - out["bound"] / n).abs().max() <= 1e-12 * out["score"].abs().max()
    assert (out["terms"][1:] >= -1e-4).all() and (out["nll"] > 0).all() and (out["prior"] >= 0).all()
    want_prior = np.where(valid.numpy(), SR.prior(tables(q, "uniform", T_CHAIN - 1)[1][0], q["x0"]), 0.0).sum(1)
    assert np.abs(out["prior"].numpy() - want_prior).max() <= 1e-12
    # per residue: NaN off the ligand, and the positions add up to the bound (a float64 sum of fp32 values)
    per = out["per_residue"]
    assert torch.isnan(per[~valid]).all() and torch.isfinite(per[valid]).all()
    assert (torch.where(valid, per, torch.zeros(())).sum(1) - out["bound"]).abs().max() <= 1e-5 * out["bound"].abs().max()
    # levels=3: {0, 3, 6}, w = 7 / 2, the same draws at those levels
    sub, sdet = score(q, levels=3, want_details=True)
    assert sub["levels"] == [0, 3, 6] and sub["terms"].shape == (3, B_CHAIN)
    want = sub["prior"] + sub["terms"][0] + 3.5 * sub["terms"][1:].sum(dim=0)
    assert (sub["bound"] - want).abs().max() <= 1e-12 * want.abs().max()
    assert torch.equal(sdet["z_t"], det["z_t"][[0, 3, 6]]) and torch.equal(sub["prior"], out["prior"])
    # sequences=None is the native strings; another sequence scores differently
    named, ndet = score(q, sequences=q["native"], levels_per_launch=3, want_details=True)
    assert torch.equal(ndet["z_t"], det["z_t"]) and all(torch.equal(named[k], out[k]) for k in ("bound", "score", "terms", "nll"))
    other = [s[1:] + s[:1] for s in q["native"]]
    assert not torch.equal(score(q, sequences=other, levels_per_launch=3)[0]["score"], out["score"])


def test_seeds_masks_and_unseeded_draws(pkg, hip, seq):
    q = seq
    # two seeds: the mean of the single-seed runs, and a finite standard error
    a, _ = score(q, cached=("all", 3, False), levels_per_launch=3, trim_padding=False, want_details=True)
    state = torch.cuda.get_rng_state(DEV), torch.get_rng_state()
    b, _ = score(q, seed=6, levels_per_launch=3)
    both, _ = score(q, seed=[SEED, 6], levels_per_launch=3)
    assert torch.equal(torch.cuda.get_rng_state(DEV), state[0]) and torch.equal(torch.get_rng_state(), state[1]), \
        "a seeded call moved torch's generator"
    for key in ("bound", "score", "terms", "nll"):
        want = (a[key] + b[key]) / 2
        assert (both[key] - want).abs().max() <= 1e-12 * want.abs().max(), key
    spread = torch.stack([a["score"], b["score"]]).std(dim=0, unbiased=True) / 2 ** 0.5
    assert torch.isfinite(both["stderr"]).all() and (both["stderr"] - spread).abs().max() <= 1e-12 * spread.max()
    assert (both["stderr"] > 0).all() and not torch.equal(a["score"], b["score"])
    # score_mask: and-ed with the padding mask, n counts what is left, an item with nothing scored is NaN
    mask = torch.zeros(B_CHAIN, L_CHAIN, dtype=torch.bool)
    mask[:, 1:4] = True
    mask[:, 100] = True                                              # padding: ignored
    mask[3] = False
    part, _ = score(q, score_mask=mask, levels_per_launch=3)
    assert part["n"].tolist() == [3, 3, 3, 0] and bool(torch.isnan(part["score"][3])) and torch.isfinite(part["score"][:3]).all()
    assert float(part["bound"][3]) == 0.0 and (part["bound"][:3] < a["bound"][:3]).all()
    sel = mask & q["valid"]
    want = torch.where(sel, a["per_residue"], torch.zeros(())).sum(1)
    assert (part["bound"] - want).abs().max() <= 1e-5 * a["bound"].abs().max()
    # unseeded: injected uniforms reproduce the call; torch's generator serves the default
    g = torch.Generator().manual_seed(9)
    us = torch.rand(T_CHAIN, B_CHAIN, L_CHAIN, generator=g)
    u1, d1 = score(q, seed=None, us=us, levels_per_launch=3, want_details=True)
    u2, d2 = score(q, seed=None, us=us, levels_per_launch=3, want_details=True)
    assert torch.equal(d1["z_t"], d2["z_t"]) and all(torch.equal(u1[k], u2[k]) for k in ("bound", "score", "terms", "nll"))
    _, d3 = score(q, seed=None, us=us, levels_per_launch=8, trim_padding=True, want_details=True)
    assert torch.equal(d3["z_t"], d1["z_t"])
    assert not torch.equal(score(q, seed=None, us=us.flip(0), levels_per_launch=3, want_details=True)[1]["z_t"], d1["z_t"])
    torch.manual_seed(4)
    r1 = score(q, seed=None, levels_per_launch=3, want_details=True)[1]["z_t"]
    torch.manual_seed(4)
    assert torch.equal(score(q, seed=None, levels_per_launch=3, want_details=True)[1]["z_t"], r1)


# ----------------------------------------------------------------------------------------------------- 5. entry tool
def test_the_tool_scores_a_table_a_fasta_file_and_the_native_sequences(pkg, hip, tmp_path, monkeypatch):
    import json
    import pandas as pd
    from e3diff_amd import biolip
    from e3diff_amd.sequence_model import sample as Q
    from test_score_cpu import load_tool
    tool = load_tool()
    path = biolip.write_synthetic(str(tmp_path / "biolip.pt"), 2, seed=4)
    for key, value in (("timesteps", 6), ("max_seq_len", 64), ("batch_size", 2), ("num_hidden_layers", 2), ("hidden_size", 256),
                       ("num_heads", 4)):
        monkeypatch.setitem(Q.CONFIG, key, value)
    shapes = {k: tuple(v.shape) for k, v in Q.get_model(1, "").state_dict().items()}
    ckpt = str(tmp_path / "seq.ckpt")
    torch.save(seeded_state_dict(shapes, seed=3), ckpt)
    base = ["--data", path, "--model", ckpt, "--split", "all", "--transition", "uniform", "--seeds", "1,2"]
    native = tool.main(base + ["--native", "-o", str(tmp_path / "native.json")])
    rows = json.load(open(tmp_path / "native.json"))
    assert len(rows) == 2 and list(native.columns) == ["structure_ids", "sequence", "bound", "score", "stderr"]
    assert [r["structure_ids"] for r in rows] == ["syn00000_B", "syn00001_B"]
    assert all(np.isfinite(r[k]) for r in rows for k in ("bound", "score", "stderr")) and all(r["score"] > 0 for r in rows)
    assert [r["score"] for r in rows] == list(native["score"])
    # the table sample.run() writes, its rows in another order than the records and one row of no record among them: the
    # output is the table's own rows, every column kept, in the dataset's order
    table = pd.DataFrame({"structure_ids": ["9zzz_A"] + list(native["structure_ids"])[::-1],
                          "true_sequence": ["AC"] + list(native["sequence"])[::-1],
                          "predict_sequence": ["AC"] + list(native["sequence"])[::-1], "recovery_rate": [0.5, 1.0, 0.25]})
    table.to_pickle(tmp_path / "output.pkl")
    by_table = tool.main(base + ["--table", str(tmp_path / "output.pkl"), "-o", str(tmp_path / "scores.pkl")])
    assert by_table.equals(pd.read_pickle(tmp_path / "scores.pkl"))
    assert list(by_table.columns) == list(table.columns) + ["bound", "score", "stderr"] and len(by_table) == 2
    assert list(by_table["structure_ids"]) == list(native["structure_ids"]) and list(by_table["score"]) == list(native["score"])
    assert list(by_table["predict_sequence"]) == list(native["sequence"]) and list(by_table["recovery_rate"]) == [0.25, 1.0]
    in_order = table.iloc[:0:-1].reset_index(drop=True)
    in_order.to_pickle(tmp_path / "output.pkl")
    kept = tool.main(base + ["--table", str(tmp_path / "output.pkl"), "-o", str(tmp_path / "scores.pkl")])
    assert list(kept.columns) == list(table.columns) + ["bound", "score", "stderr"] and list(kept["score"]) == list(native["score"])
    # a FASTA file with another sequence for the first record; one seed: no standard error
    seqs = list(native["sequence"])
    changed = seqs[0][1:] + seqs[0][:1]
    (tmp_path / "d.fa").write_text(f">syn00000_B\n{changed}\n>syn00001_B\n{seqs[1]}\n")
    fa = tool.main(base[:-2] + ["--seeds", "1", "--levels", "2", "--fasta", str(tmp_path / "d.fa"), "-o", str(tmp_path / "fa.json")])
    assert list(fa["sequence"]) == [changed, seqs[1]] and np.isnan(fa["stderr"]).all() and np.isfinite(fa["score"]).all()
    (tmp_path / "d.fa").write_text(f">syn00000_B\n{changed}A\n>syn00001_B\n{seqs[1]}\n")
    with pytest.raises(ValueError, match="syn00000_B: the ligand has"):
        tool.main(base + ["--fasta", str(tmp_path / "d.fa"), "-o", str(tmp_path / "fa.json")])
