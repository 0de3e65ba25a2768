"""GPU: scoring supplied structures (csrc/sampler.hip, "scoring supplied structures"; structure_model/sample.py::
score_structures).  The two entry points through the C ABI -- the keyed forward noising at per-item levels bit for bit
against ``e3d_q_sample_wrap`` fed the stream-12 draws of ``e3d_keyed_draws``, the score items against
tests/structure_score_ref.py in float64 per element and their sums bit for bit against the fixed-shape fp32 restatement
and against ``e3d_masked_item_sums`` -- then ``score_structures`` end to end on the tiny structure model of
tests/test_known_gpu.py, and the command-line tool.  Plumbing and conventions are those of tests/test_score_gpu.py:
outputs between guard words, NaN after every input, every case run twice.

Bounds (u = 2^-24): tests/structure_score_ref.py's docstring derives them from the operations performed --
  term   |got - ref| <= (h e_delta (2 |delta| + e_delta) + 2 u h delta^2 + u |term|) (1 + 2^-10),
         e_delta = 3 u |d| + 4 u pi + (|d| / pi + 3) PI_ERR, d = k (eps_hat - eps)
  err    circular |got - ref| <= 2 u |s| + 4 u pi + (|s| / pi + 3) PI_ERR, s = eps_hat - eps
  sums   bit for bit against the fixed-shape fp32 restatement; against float64 within (L F) u sum |v|
  end to end   terms[s, b] against the float64 elements evaluated on the returned eps and eps_hat, summed over the scored
         elements: the sum of the elements' bounds + (L F) u sum |term|; eps_mse the same with err^2, whose element bound
         is e_err (2 |err| + e_err) + u err^2.
The forward noising's noise is also held to the numpy restatement of the stream within 2e-6 max(1, |z|) on the circle,
the bound tests/test_sampler_forms_gpu.py applies to every keyed normal.

Measured on an MI355X, worst |got - ref| / bound over all cases of a test (each test prints its own; DESIGN.md, "Scoring
structures", records them too):
  forward levels, noise against the restatement   0.193  (3 x 2 x 64 x 12; 0.126 at 1 x 1 x 1 x 4, 0.183 at the other two)
  score items, term                               0.605  (L = 257, F = 4; 0.31 - 0.40 at L = 1, 0.49 - 0.60 at L = 63 .. 257)
  score items, err                                0.754  (L = 257, F = 8; 0.41 - 0.48 at L = 1, 0.63 - 0.72 elsewhere)
  score items, sums against float64               0.215  (L = 1, F = 4: four values; 0.007 at L = 63 .. 65, 0.001 at L = 257)
  end to end                                      0.032 (terms), 0.004 (eps_mse)
The term and err ratios are large because the bounds are tight where it matters: beside a wrap cut the fp32 shift by pi
rounds at 2^-22, which the 4 u pi of e_delta counts at 3.14 / 4 of its worst case.
Everything else in this module is compared bit for bit, or is a statement about counts, shapes and strings.
"""
import numpy as np
import pytest
import torch

import keyed_ref as K
import sampler_ref as R
import structure_score_ref as SS
from helpers import rel_err
from test_rowops_forms_gpu import DEV, SENTINEL, Vec, call, p, twice
from test_sampler_forms_gpu import IVec, dev_f, dev_i, dev_keys, fvec, keyed_normals, np_, same_bits, take
from test_score_gpu import dev_u8

pytestmark = pytest.mark.gpu

U = R.U
T_BIG = 1000


@pytest.fixture(scope="module")
def sched(pkg, hip):
    """The T = 1000 tables: the forward law's two columns and the score table at scale 0.5 (add != 0), host and device."""
    from e3diff_amd.structure_model.utils import CosineTables, ScoreTables
    tab = CosineTables(T_BIG)
    out = {"sa": tab.sqrt_alphas_cumprod.numpy(), "s1": tab.sqrt_one_minus_alphas_cumprod.numpy()}
    out["sa_d"], out["s1_d"] = dev_f(out["sa"]), dev_f(out["s1"])
    for name, scale in (("coef", 0.5), ("coef1", 1.0)):
        out[name] = ScoreTables(tab, scale).coef.numpy()
        out[name + "_d"] = dev_f(out[name])
    return out


# ----------------------------------------------------------------------------------------------------- 1. forward levels
def forward_levels(pkg, sched, xd, kd, steps, max_step, scale, seed, N, B, L, F, what):
    noise, xt = fvec(N * L * F), fvec(N * L * F)
    steps_d = dev_i(np.asarray(steps), 0, torch.int64)
    call(pkg, "e3d_keyed_q_sample_levels_wrap", p(xd), p(kd), p(steps_d), max_step, p(sched["sa_d"]), p(sched["s1_d"]), T_BIG,
         scale, seed, noise.ptr, xt.ptr, N, B, L, F)
    return take(noise, what), take(xt, what)


@pytest.mark.parametrize("B,n,L,F", [(1, 1, 1, 4), (2, 3, 37, 8), (1, 2, 257, 8), (3, 2, 64, 12)])
def test_forward_levels(pkg, hip, sched, B, n, L, F):
    N, per = n * B, L * F
    x0 = R.ddpm_inputs(B * per, seed=51)[0].reshape(B, L, F)
    ids = R.IDS[1:1 + B]
    keys = R.padded_keys(ids, L)
    if B * L > 8:
        keys[2] = keys[B * L // 2] = (9, -1)                               # rows of no item
    live = np.repeat(keys[:, 1] >= 0, F).reshape(B, per)
    xd, kd = dev_f(x0), dev_keys(keys)
    x_tiled = dev_f(np.tile(x0.reshape(B, per), (n, 1)))
    live_n = torch.from_numpy(np.tile(live, (n, 1)).reshape(-1)).to(DEV)
    mixed = [(0, 1, T_BIG - 1, 500, 7, 998)[i % 6] for i in range(N)]
    worst = 0.0
    for seed, scale in zip(R.SEEDS, (1.0, 0.5)):
        for steps in ([0] * N, [1] * N, [T_BIG - 1] * N, mixed):
            what = f"forward levels {B}x{n}x{L}x{F} seed={seed} scale={scale} steps={steps[:4]}"
            noise, xt = twice(lambda: forward_levels(pkg, sched, xd, kd, steps, T_BIG - 1, scale, seed, N, B, L, F, what), what)
            # the stream-12 draws of each item's step, wrapped and scaled by e3d_keyed_draws, through e3d_q_sample_wrap
            want_noise = torch.cat([keyed_normals(pkg, kd, seed, 12, t, F, B * L, 1, scale, what).reshape(B, per)[i % B]
                                    for i, t in enumerate(steps)])
            assert same_bits(noise, want_noise), f"{what}: noise differs from e3d_keyed_draws(stream 12)"
            o = fvec(N * per)
            steps_d = dev_i(np.asarray(steps), 0, torch.int64)
            call(pkg, "e3d_q_sample_wrap", p(x_tiled), p(want_noise), p(steps_d), p(sched["sa_d"]), p(sched["s1_d"]), o.ptr, N, per)
            want_xt = take(o, what)
            assert same_bits(xt[live_n], want_xt[live_n]), f"{what}: x_t differs from e3d_q_sample_wrap fed the noise"
            assert bool((xt[~live_n].view(torch.int32) == 0).all()) and bool((noise[~live_n].view(torch.int32) == 0).all()), \
                f"{what}: a row of no item is not zero"
            # ... and the numpy restatement of the stream
            ref_noise, ref_xt = SS.forward_levels(x0, keys, seed, steps, sched["sa"], sched["s1"], scale)
            z = np.stack([K.normals(keys.reshape(B, L, 2)[i % B], seed, 12, t, F) for i, t in enumerate(steps)])
            tol = scale * 2e-6 * np.maximum(1.0, np.abs(z)).reshape(-1)
            err = R.circ(np_(noise), ref_noise.reshape(-1))
            worst = max(worst, float((err / tol).max()))
            assert (err <= tol).all(), (what, float((err / tol).max()))
            assert float(noise.abs().max()) <= np.pi + 1e-6 and float(xt.abs().max()) <= np.pi + 1e-6
            # x_t: the noise's tolerance (s <= 1) + the fp32 roundings of two products, their sum and the wrap, each at most
            # u of a value below 2 pi, and the wrap's PI_ERR: 16 u pi covers them
            assert (R.circ(np_(xt).astype(np.float64), ref_xt.reshape(-1)) <= tol + 16 * U * np.pi).all(), what
        # a step above the caller's bound: that item is NaN, its neighbours are unchanged
        what = f"forward levels {B}x{n}x{L}x{F} seed={seed}: max_step below an item's step"
        base_n, base_x = forward_levels(pkg, sched, xd, kd, mixed, T_BIG - 1, scale, seed, N, B, L, F, what)
        low_n, low_x = forward_levels(pkg, sched, xd, kd, mixed, 7, scale, seed, N, B, L, F, what)
        over = torch.from_numpy(np.repeat(np.asarray(mixed) > 7, per)).to(DEV)
        for a, b in ((low_n, base_n), (low_x, base_x)):
            assert bool(torch.isnan(a[over]).all()) and same_bits(a[~over], b[~over]), what
        for bad in (-1, T_BIG):                                             # outside the tables, whatever max_step says
            steps = list(mixed)
            steps[-1] = bad
            bn, bx = forward_levels(pkg, sched, xd, kd, steps, 65535, scale, seed, N, B, L, F, what)
            assert bool(torch.isnan(bn[-per:]).all()) and bool(torch.isnan(bx[-per:]).all())
            assert same_bits(bn[:-per], base_n[:-per]) and same_bits(bx[:-per], base_x[:-per]), what
        # tiling: item i of the n x B launch is the same (item, step) of a B = 1 launch
        for i in range(N):
            b = i % B
            one = forward_levels(pkg, sched, dev_f(x0[b:b + 1]), dev_keys(keys[b * L:(b + 1) * L].copy()), [mixed[i]], T_BIG - 1,
                                 scale, seed, 1, 1, L, F, what)
            assert same_bits(one[0], base_n[i * per:(i + 1) * per]) and same_bits(one[1], base_x[i * per:(i + 1) * per]), (what, i)
    print(f"forward levels {B}x{n}x{L}x{F}: worst |noise - restatement| / bound = {worst:.3f}")


# ----------------------------------------------------------------------------------------------------- 2. score items
class Items:
    """The inputs of one score case on the device and the entry point; every output between guard words."""

    def __init__(self, pkg, eps_hat, eps, mask, steps, coef_d, T=T_BIG):
        self.pkg, (self.N, self.L, self.F), self.B, self.T = pkg, eps.shape, mask.shape[0], T
        self.eh, self.e, self.m = dev_f(eps_hat), dev_f(eps), dev_u8(mask)
        self.steps, self.coef = dev_i(np.asarray(steps), 0, torch.int64), coef_d

    def run(self, what, elements=True, parts=True):
        N, L, F = self.N, self.L, self.F
        el = [Vec(N * L * F), Vec(N * L * F)] if elements else [None, None]
        pa = [Vec(N * L), Vec(N * L), Vec(N * F), Vec(N * F)] if parts else [None] * 4
        tot, cnt = [Vec(N), Vec(N)], IVec(N)
        call(self.pkg, "e3d_angle_score_items", p(self.eh), p(self.e), p(self.m), p(self.steps), p(self.coef), self.T,
             *(None if o is None else o.ptr for o in el + pa), tot[0].ptr, tot[1].ptr, cnt.ptr, N, self.B, L, F)
        got = {k: (None if o is None else o.get(what)) for k, o in zip(("term", "err", "res_term", "res_err2", "feat_term", "feat_err2",
                                                                         "tot_term", "tot_err2"), el + pa + tot)}
        for k, v in got.items():
            assert v is None or not bool((v == SENTINEL).any()), f"{what}: an element of {k} was not written"
        got["counts"] = cnt.get(what)
        return got


def masked_sums(pkg, values, mask, what):
    N, L = values.shape
    sums, counts = Vec(N), IVec(N)
    m_d = dev_u8(mask)
    call(pkg, "e3d_masked_item_sums", p(values), p(m_d), sums.ptr, counts.ptr, N, L)
    return take(sums, what), counts.get(what)


@pytest.mark.parametrize("F", [4, 8, 12])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 257])
def test_score_items_against_float64(pkg, hip, sched, L, F):
    steps = [0, 1, T_BIG - 1, T_BIG]                                        # the last one: outside the table
    N = len(steps)
    rows = sched["coef"]
    eps_hat, eps = SS.score_inputs(N, L, F, rows, steps)
    worst = {"term": 0.0, "err": 0.0, "sum": 0.0}
    for tag, mask in SS.score_masks(N, L, F).items():
        what = f"score items L={L} F={F} mask={tag}"
        on = mask.astype(bool)
        eh = eps_hat.copy()
        if tag == "random":
            eh[~on] = np.nan                                                # NaN under everything masked out
        P = Items(pkg, eh, eps, mask, steps, sched["coef_d"])
        got_t = twice(lambda: tuple(P.run(what).values()), what)
        got = dict(zip(("term", "err", "res_term", "res_err2", "feat_term", "feat_err2", "tot_term", "tot_err2", "counts"), got_t))
        g = {k: np_(v) for k, v in got.items()}
        term, err = g["term"].reshape(N, L, F), g["err"].reshape(N, L, F)
        assert np.array_equal(g["counts"], on.reshape(N, -1).sum(1))
        # the item with a step outside [0, T): NaN everywhere
        for k in ("term", "err", "res_term", "res_err2", "feat_term", "feat_err2", "tot_term", "tot_err2"):
            assert np.isnan(g[k].reshape(N, -1)[-1]).all(), (what, k)
        for n in range(N - 1):
            see = on[n] if tag == "random" else np.ones((L, F), dtype=bool)
            r_err, _, r_term = SS.elem(rows[steps[n]], eps_hat[n], eps[n])
            e_t, b_t = np.abs(term[n] - r_term)[see], SS.term_bound(rows[steps[n]], eps_hat[n], eps[n])[see]
            e_e, b_e = R.circ(err[n], r_err)[see], SS.err_bound(eps_hat[n], eps[n])[see]
            if see.any():
                worst["term"], worst["err"] = max(worst["term"], float((e_t / b_t).max())), max(worst["err"], float((e_e / b_e).max()))
                assert (e_t <= b_t).all(), (what, n, "term: worst |got - ref| / bound", float((e_t / b_t).max()))
                assert (e_e <= b_e).all(), (what, n, "err: worst |got - ref| / bound", float((e_e / b_e).max()))
            same = (eps_hat[n] == eps[n]) & see
            assert same.any() or tag == "random"
            assert (term[n][same].view(np.int32) == np.float32(rows[steps[n], 2]).view(np.int32)).all(), \
                f"{what}: term != add where eps_hat == eps"
            assert (err[n][same].view(np.int32) == 0).all()
            assert np.isnan(term[n][~see]).all() and (np.abs(err[n][see]) <= np.pi + 1e-6).all()
            # the sums: bit for bit against the fixed shape, and against float64
            for val, key in ((term[n], "term"), ((err[n] * err[n]).astype(np.float32), "err2")):
                res, feat, tot, cnt = SS.item_sums_fp32(val, on[n])
                assert np.array_equal(g["res_" + key].reshape(N, L)[n].view(np.int32), res.view(np.int32)), (what, n, key, "res")
                assert np.array_equal(g["feat_" + key].reshape(N, F)[n].view(np.int32), feat.view(np.int32)), (what, n, key, "feat")
                assert g["tot_" + key][n].view(np.int32) == tot.view(np.int32), (what, n, key, float(g["tot_" + key][n]), float(tot))
                exact, bound = val.astype(np.float64)[on[n]].sum(), L * F * U * np.abs(val.astype(np.float64))[on[n]].sum()
                assert abs(float(tot) - exact) <= bound
                worst["sum"] = max(worst["sum"], abs(float(tot) - exact) / bound) if bound else worst["sum"]
        if tag == "none":
            for k in ("res_term", "res_err2", "feat_term", "feat_err2", "tot_term", "tot_err2"):
                assert (g[k].reshape(N, -1)[:-1].view(np.int32) == 0).all(), f"{what}: {k} is not +0"
        # tot_* is e3d_masked_item_sums on res_* with the any-element-set residue mask
        any_set = on.any(axis=2)
        for key in ("term", "err2"):
            s, c = masked_sums(pkg, got["res_" + key].reshape(N, L), any_set, what)
            assert same_bits(s[:-1], got["tot_" + key][:-1]), f"{what}: tot_{key} differs from e3d_masked_item_sums(res_{key})"
            assert np.array_equal(np_(c), any_set.sum(1))
        # every optional output absent: the same totals
        bare = P.run(what, elements=False, parts=False)
        for k in ("tot_term", "tot_err2", "counts"):
            assert torch.equal(bare[k].view(torch.int32), got[k].view(torch.int32)), f"{what}: NULL outputs change {k}"
    print(f"score items L={L} F={F}: worst |got - ref| / bound = {worst['term']:.3f} (term), {worst['err']:.3f} (err), "
          f"{worst['sum']:.3f} (sums against float64)")


def test_an_items_sums_do_not_depend_on_padding_batch_or_mask_tiling(pkg, hip, sched):
    B, L, F = 3, 64, 8
    steps = [1, 500, T_BIG - 1]
    eps_hat, eps = SS.score_inputs(B, L, F, sched["coef"], steps, seed=90)
    mask = SS.score_masks(B, L, F, seed=91)["random"]
    mask[:, 40:] = 0                                                        # nothing set beyond position 39
    keys = ("res_term", "res_err2", "feat_term", "feat_err2", "tot_term", "tot_err2", "counts")
    what = "score items: L = 64"
    base = Items(pkg, eps_hat, eps, mask, steps, sched["coef_d"]).run(what)
    # L = 128 with NaN padding that is masked out
    wide_h, wide_e = (np.concatenate([a, np.full((B, L, F), np.nan, dtype=np.float32)], axis=1) for a in (eps_hat, eps))
    wide_m = np.concatenate([mask, np.zeros((B, L, F), dtype=np.uint8)], axis=1)
    wide = Items(pkg, wide_h, wide_e, wide_m, steps, sched["coef_d"]).run("score items: L = 128")
    for k in keys:
        a = wide[k].reshape(B, 2 * L)[:, :L].reshape(-1) if k.startswith("res_") else wide[k]
        assert same_bits(a, base[k]), f"padding to L = 128 changes {k}"
    assert bool((wide["res_term"].reshape(B, 2 * L)[:, L:].view(torch.int32) == 0).all())
    # alone, and reversed
    for b in range(B):
        one = Items(pkg, eps_hat[b:b + 1], eps[b:b + 1], mask[b:b + 1], steps[b:b + 1], sched["coef_d"]).run(f"item {b} alone")
        for k in keys:
            assert same_bits(one[k].reshape(1, -1), base[k].reshape(B, -1)[b:b + 1]), f"item {b} alone differs in {k}"
    rev = Items(pkg, eps_hat[::-1].copy(), eps[::-1].copy(), mask[::-1].copy(), steps[::-1], sched["coef_d"]).run("reversed")
    for k in keys:
        assert same_bits(rev[k].reshape(B, -1).flip(0), base[k].reshape(B, -1)), f"reversing the batch changes {k}"
    # the mask given once for B items, N = 3 B level-major: item i reads mask i % B
    steps3 = steps + [0, 0, 0] + [7, 7, 7]
    h3, e3 = SS.score_inputs(3 * B, L, F, sched["coef"], steps3, seed=92)
    tiled = Items(pkg, h3, e3, np.tile(mask, (3, 1, 1)), steps3, sched["coef_d"]).run("mask tiled by the caller")
    once = Items(pkg, h3, e3, mask, steps3, sched["coef_d"]).run("mask given for B items")
    assert once["counts"].tolist() == tiled["counts"].tolist() == np_(base["counts"]).tolist() * 3
    for k in keys + ("term", "err"):
        assert same_bits(once[k], tiled[k]), f"reading the mask as item i % B changes {k}"


# ----------------------------------------------------------------------------------------------------- 3. end to end
T_CHAIN, B_CHAIN, L_CHAIN, F_CHAIN = 8, 4, 64, 8
IDS = [11, (1 << 35) + 2, 7, 123456]
SEED = 5


@pytest.fixture(scope="module")
def chain(pkg, hip):
    """The tiny 2-layer structure model and the four synthetic pockets of tests/test_known_gpu.py's ``setup`` at L = 64,
    T = 8, the pockets' own ligand angles as x0, and a cache of the runs the tests below share."""
    from test_keyed_sampling_gpu import _structure_setup
    from helpers import synthetic_pockets
    model, pk, tab = _structure_setup(B=B_CHAIN, L=L_CHAIN, T=T_CHAIN)
    x0 = synthetic_pockets(B_CHAIN, L_CHAIN, seed=3, rec_range=(20, 70))["ligand_angles"]
    assert torch.equal(x0, pk["ligand_angles"].cpu())
    valid = pk["ligand_attn_mask"].cpu() != 0
    return {"model": model, "pk": pk, "tab": tab, "x0": x0, "valid": valid, "lengths": [int(v) for v in valid.sum(1)], "cache": {}}


def score(q, sel=None, cached=None, **kw):
    """score_structures on the fixture (``sel``: the items of the batch, default all); ``cached``: a key under which the
    (result, details) pair is kept for other tests."""
    from e3diff_amd.structure_model.sample import score_structures
    if cached is not None and cached in q["cache"]:
        return q["cache"][cached]
    sel = list(range(B_CHAIN)) if sel is None else sel
    kw.setdefault("seed", SEED)
    if kw["seed"] is not None:
        kw.setdefault("item_ids", [IDS[i] for i in sel])
    details = {} if kw.pop("want_details", False) else None
    pk = {k: v[sel].contiguous() for k, v in q["pk"].items()}
    out = score_structures(q["model"], pk["ligand_attn_mask"], q["x0"][sel], pk["receptor_seq"], pk["receptor_attn_mask"],
                           pk["receptor_angles"], T_CHAIN, q["tab"], details=details, **kw)
    if cached is not None:
        q["cache"][cached] = (out, details)
    return out, details


def restated_draws(q, scale=1.0, seed=SEED, levels=None):
    """(eps, x_t) [S, B, L, F] on the host from e3d_keyed_draws(stream 12) and e3d_q_sample_wrap, level by level."""
    from e3diff_amd import keyed, ops
    tab = q["tab"]
    keys = keyed.padded_keys(keyed.item_ids(IDS, B_CHAIN), L_CHAIN, DEV)
    sa, s1 = tab.sqrt_alphas_cumprod.to(DEV), tab.sqrt_one_minus_alphas_cumprod.to(DEV)
    x0 = q["x0"].to(DEV).contiguous()
    eps, xt = [], []
    for t in (range(T_CHAIN) if levels is None else levels):
        e = ops.keyed_draws(keys, seed, 12, t, ops.KEYED_NORMAL, F_CHAIN, wrap=True, scale=scale).reshape(B_CHAIN, L_CHAIN, F_CHAIN)
        eps.append(e)
        xt.append(ops.q_sample_wrap(x0, e.contiguous(), torch.full((B_CHAIN,), t, device=DEV, dtype=torch.long), sa, s1))
    return torch.stack(eps).cpu(), torch.stack(xt).cpu()


def check_against_reference(q, out, det, what, scale=1.0, scored=None):
    """Every terms[s, b] and eps_mse[s, b] against float64 on the returned eps and eps_hat; the worst error / bound."""
    from e3diff_amd.structure_model.utils import ScoreTables
    rows = ScoreTables(q["tab"], scale).coef.numpy()
    scored = q["valid"][..., None].expand(B_CHAIN, L_CHAIN, F_CHAIN).numpy() if scored is None else scored
    eps, eh = det["eps"].numpy(), det["eps_hat"].numpy()
    n = scored.reshape(B_CHAIN, -1).sum(1)
    worst = [0.0, 0.0]
    for i, t in enumerate(out["levels"]):
        r_err, _, r_term = SS.elem(rows[t], eh[i], eps[i])
        b_term = SS.term_bound(rows[t], eh[i], eps[i])
        e_err = SS.err_bound(eh[i], eps[i])
        r_e2, b_e2 = r_err ** 2, e_err * (2 * np.abs(r_err) + e_err) + U * r_err ** 2
        for k, (key, r, b, div) in enumerate((("terms", r_term, b_term, 1.0), ("eps_mse", r_e2, b_e2, n))):
            r, b = (np.where(scored, v, 0.0).reshape(B_CHAIN, -1) for v in (r, b))
            total, tb = r.sum(1), b.sum(1) + L_CHAIN * F_CHAIN * U * np.abs(r).sum(1)
            err = np.abs(out[key][i].numpy() * div - total)
            ratio = float(np.divide(err, tb, out=np.zeros_like(err), where=tb > 0).max())      # (an item with nothing scored: 0 / 0)
            worst[k] = max(worst[k], ratio)
            assert (err <= tb).all(), (what, key, "level", t, "worst |got - ref| / bound", ratio)
    return worst


def test_draws_terms_and_predictions_in_every_chunking_and_frame(pkg, hip, chain):
    q = chain
    valid = q["valid"]
    eps_want, xt_want = restated_draws(q)
    first, worst = None, [0.0, 0.0]
    for lpl in (1, 3, 8):
        for trim in (False, True):
            what = f"score_structures levels_per_launch={lpl} trim_padding={trim}"
            out, det = score(q, cached=("all", lpl, trim), levels_per_launch=lpl, trim_padding=trim, want_details=True)
            assert out["levels"] == list(range(T_CHAIN)) and set(det) == {"x_t", "eps", "eps_hat"}
            assert all(tuple(det[k].shape) == (T_CHAIN, B_CHAIN, L_CHAIN, F_CHAIN) and not det[k].is_cuda for k in det)
            # the frame's rows hold the restated keyed draws, bit for bit (a trimmed frame returns zeros beyond its rows)
            Ll = 32 if trim else L_CHAIN
            assert max(q["lengths"]) <= 32
            for k, want in (("eps", eps_want), ("x_t", xt_want)):
                assert torch.equal(det[k][:, :, :Ll].contiguous().view(torch.int32), want[:, :, :Ll].contiguous().view(torch.int32)), \
                    f"{what}: {k} is not the restated keyed draw"
                assert bool((det[k][:, :, Ll:] == 0).all())
            w = check_against_reference(q, out, det, what)
            worst = [max(a, b) for a, b in zip(worst, w)]
            if first is None:
                first = det
            # eps_hat between chunkings and frames: the bound tests/test_packed_gpu.py applies between frames
            v = valid[None].expand(T_CHAIN, B_CHAIN, L_CHAIN)
            assert rel_err(det["eps_hat"][v], first["eps_hat"][v]) < 2e-5, what
    print(f"score_structures: worst |got - ref| / bound = {worst[0]:.3f} (terms), {worst[1]:.3f} (eps_mse)")
    # ... and against a direct forward at the same per-item timesteps and x_t
    pk, model = q["pk"], q["model"]
    for i, t in enumerate(range(T_CHAIN)):
        direct = model.forward(torch.full((B_CHAIN,), t, device=DEV, dtype=torch.long), first["x_t"][i].to(DEV), pk["ligand_attn_mask"],
                               pk["receptor_seq"], pk["receptor_angles"], pk["receptor_attn_mask"]).cpu()
        assert rel_err(first["eps_hat"][i][valid], direct[valid]) < 2e-5, f"eps_hat differs from model.forward at t={t}"


def test_an_items_draws_do_not_depend_on_its_place_or_its_batch(pkg, hip, chain):
    q = chain
    out, det = score(q, cached=("all", 3, False), levels_per_launch=3, trim_padding=False, want_details=True)
    rev, rdet = score(q, sel=[3, 2, 1, 0], levels_per_launch=3, want_details=True)
    for k in ("eps", "x_t"):
        assert torch.equal(rdet[k].flip(1).view(torch.int32), det[k].view(torch.int32)), f"{k} depends on the item's place"
    assert torch.equal(rev["n"].flip(0), out["n"]) and torch.equal(rev["prior"].flip(0), out["prior"])
    check_against_reference({**q, "valid": q["valid"].flip(0)}, rev, rdet, "reversed batch")
    part, pdet = score(q, sel=[1, 2], levels_per_launch=2, want_details=True)
    for k in ("eps", "x_t"):
        assert torch.equal(pdet[k].view(torch.int32), det[k][:, 1:3].contiguous().view(torch.int32)), f"{k} depends on the batch"
    assert torch.equal(part["n"], out["n"][1:3])
    # other item ids: other draws; levels=3: the same draws at those levels
    assert not torch.equal(score(q, item_ids=[1, 2, 3, 4], want_details=True)[1]["eps"], det["eps"])
    sub, sdet = score(q, levels=3, want_details=True)
    assert sub["levels"] == [0, 3, 6] and torch.equal(sdet["eps"].view(torch.int32), det["eps"][[0, 3, 6]].view(torch.int32))
    want = sub["prior"] + sub["terms"][0] + 3.5 * sub["terms"][1:].sum(dim=0)
    assert (sub["bound"] - want).abs().max() <= 1e-12 * want.abs().max()


def test_the_encoder_runs_once_and_decode_gets_the_levels_timesteps(pkg, hip, chain, monkeypatch):
    q = chain
    model = q["model"]
    calls = {"encode": 0, "steps": []}
    encode, decode = model.encode_receptor, model.decode

    def counted_encode(*a, **kw):
        calls["encode"] += 1
        return encode(*a, **kw)

    def seen_decode(timestep, *a, **kw):
        calls["steps"].append(timestep.cpu().tolist())
        return decode(timestep, *a, **kw)
    monkeypatch.setattr(model, "encode_receptor", counted_encode)
    monkeypatch.setattr(model, "decode", seen_decode)
    for lpl, seeds in ((3, SEED), (8, [SEED, 6]), (1, None)):
        calls["encode"], calls["steps"] = 0, []
        score(q, levels_per_launch=lpl, seed=seeds)
        assert calls["encode"] == 1, f"encode_receptor ran {calls['encode']} times in one call"
        n_seeds = 2 if isinstance(seeds, list) else 1
        flat = [t for launch in calls["steps"] for t in launch]
        want = [t for first in range(0, T_CHAIN, lpl) for t in range(first, min(first + lpl, T_CHAIN)) for _ in range(B_CHAIN)]
        assert flat == want * n_seeds and len(calls["steps"]) == n_seeds * -(-T_CHAIN // lpl)


def test_the_returned_record_adds_up(pkg, hip, chain):
    q = chain
    out, det = score(q, cached=("all", 3, False), levels_per_launch=3, trim_padding=False, want_details=True)
    valid, lengths = q["valid"], torch.tensor(q["lengths"])
    assert set(out) == {"bound", "score", "prior", "n", "stderr", "terms", "eps_mse", "levels", "per_residue", "per_feature"}
    assert all(not out[k].is_cuda for k in out if k != "levels")
    assert out["terms"].shape == out["eps_mse"].shape == (T_CHAIN, B_CHAIN) and out["per_residue"].shape == (B_CHAIN, L_CHAIN)
    assert out["per_feature"].shape == (B_CHAIN, F_CHAIN) and out["n"].dtype == torch.int32
    assert torch.equal(out["n"], (lengths * F_CHAIN).int()) and torch.isnan(out["stderr"]).all() and torch.isfinite(out["score"]).all()
    # levels=None: w = 1, the bound is the prior and every term (float64 on the host: its own rounding)
    want = out["prior"] + out["terms"][0] + 1.0 * out["terms"][1:].sum(dim=0)
    assert (out["bound"] - want).abs().max() <= 1e-12 * want.abs().max()
    assert (out["score"] - out["bound"] / out["n"]).abs().max() <= 1e-12 * out["score"].abs().max()
    assert (out["eps_mse"] >= 0).all() and (out["eps_mse"] <= np.pi ** 2 + 1e-6).all()
    from e3diff_amd.structure_model.utils import ScoreTables
    st = ScoreTables(q["tab"])
    assert (out["terms"][1:] >= 0).all() and (out["terms"][0] >= float(st.coef[0, 2]) * out["n"] * (1 + 1e-6)).all()
    want_prior = np.where(valid[..., None].numpy(), SS.prior(q["x0"].numpy(), st.prior_ab), 0.0).sum((1, 2))
    assert np.abs(out["prior"].numpy() - want_prior).max() <= 1e-12 * max(1.0, np.abs(want_prior).max())
    # per residue and per feature: fp32 partial sums of the same elements in other orders, added up in float64 -- each
    # differs from the total by at most (L F) u sum |element term| per level, the bound of the sums themselves
    per = out["per_residue"]
    assert torch.isnan(per[~valid]).all() and torch.isfinite(per[valid]).all()
    rows = st.coef.numpy()
    mag = np.zeros(B_CHAIN)
    for i, t in enumerate(out["levels"]):
        mag += np.where(valid[..., None].numpy(), np.abs(SS.elem(rows[t], det["eps_hat"][i].numpy(), det["eps"][i].numpy())[2]), 0.0).sum((1, 2))
    slack = torch.from_numpy(2 * L_CHAIN * F_CHAIN * U * mag)
    assert ((torch.nan_to_num(per, nan=0.0).sum(1) - out["bound"]).abs() <= slack).all()
    assert ((out["prior"] + out["per_feature"].sum(1) - out["bound"]).abs() <= slack).all()
    # a score_mask of one residue: the draws are those of the full call, the bound is that residue's
    mask = torch.zeros(B_CHAIN, L_CHAIN, dtype=torch.bool)
    mask[:, 2] = True
    mask[:, 60] = True                                               # padding: ignored
    mask[3] = False                                                  # nothing scored
    part, pdet = score(q, score_mask=mask, levels_per_launch=3, want_details=True)
    for k in ("eps", "x_t", "eps_hat"):
        assert torch.equal(pdet[k].view(torch.int32), det[k].view(torch.int32)), f"a score_mask changes {k}"
    assert part["n"].tolist() == [F_CHAIN] * 3 + [0] and bool(torch.isnan(part["score"][3])) and torch.isfinite(part["score"][:3]).all()
    assert float(part["bound"][3]) == 0.0 and bool(torch.isnan(part["eps_mse"][:, 3]).all())
    assert ((part["bound"] - torch.nan_to_num(per[:, 2], nan=0.0) * torch.tensor([1.0, 1.0, 1.0, 0.0])).abs() <= slack).all()
    scored = (mask[..., None] & valid[..., None]).expand(B_CHAIN, L_CHAIN, F_CHAIN).numpy()
    check_against_reference(q, {**part, "eps_mse": torch.nan_to_num(part["eps_mse"], nan=0.0)}, pdet, "score_mask", scored=scored)
    # per element: one feature of one residue
    el = torch.zeros(B_CHAIN, L_CHAIN, F_CHAIN, dtype=torch.bool)
    el[:, 1, 5] = True
    one, _ = score(q, score_mask=el, levels_per_launch=3)
    assert one["n"].tolist() == [1] * 4 and (one["per_feature"][:, [0, 1, 2, 3, 4, 6, 7]] == 0).all()
    assert torch.equal(one["prior"] + one["per_feature"][:, 5], one["bound"])


def test_seeds_scale_and_injected_noises(pkg, hip, chain):
    from e3diff_amd import keyed, ops
    q = chain
    a, adet = score(q, cached=("all", 3, False), levels_per_launch=3, trim_padding=False, want_details=True)
    state = torch.cuda.get_rng_state(DEV), torch.get_rng_state()
    b, _ = score(q, seed=6, levels_per_launch=3)
    both, _ = score(q, seed=[SEED, 6], levels_per_launch=3)
    assert torch.equal(torch.cuda.get_rng_state(DEV), state[0]) and torch.equal(torch.get_rng_state(), state[1]), \
        "a seeded call moved torch's generator"
    for key in ("bound", "score", "terms", "eps_mse", "per_feature"):
        want = (a[key] + b[key]) / 2
        assert (both[key] - want).abs().max() <= 1e-12 * want.abs().max(), key
    spread = torch.stack([a["score"], b["score"]]).std(dim=0, unbiased=True) / 2 ** 0.5
    assert torch.isfinite(both["stderr"]).all() and (both["stderr"] - spread).abs().max() <= 1e-12 * spread.max()
    assert (both["stderr"] > 0).all() and not torch.equal(a["score"], b["score"])
    # injected noises equal to the keyed normals: the seeded result, bit for bit
    keys = keyed.padded_keys(keyed.item_ids(IDS, B_CHAIN), L_CHAIN, DEV)
    z = torch.stack([ops.keyed_draws(keys, SEED, 12, t, ops.KEYED_NORMAL, F_CHAIN).reshape(B_CHAIN, L_CHAIN, F_CHAIN)
                     for t in range(T_CHAIN)]).cpu()
    inj, idet = score(q, seed=None, noises=z, levels_per_launch=3, want_details=True)
    for k in ("eps", "x_t", "eps_hat"):
        assert torch.equal(idet[k].view(torch.int32), adet[k].view(torch.int32)), f"injected noises: {k} differs"
    for k in ("bound", "score", "terms", "eps_mse", "per_residue", "per_feature", "prior"):
        assert torch.equal(torch.nan_to_num(inj[k], nan=-1.0), torch.nan_to_num(a[k], nan=-1.0)), k
    _, tdet = score(q, seed=None, noises=z, levels_per_launch=8, trim_padding=True, want_details=True)
    assert torch.equal(tdet["eps"][:, :, :32].contiguous().view(torch.int32), adet["eps"][:, :, :32].contiguous().view(torch.int32))
    # scale 0.5: other draws (the restated ones), a constant added per element and level above 0
    half, hdet = score(q, scale=0.5, levels_per_launch=3, want_details=True)
    eps_want, xt_want = restated_draws(q, scale=0.5)
    assert torch.equal(hdet["eps"].view(torch.int32), eps_want.view(torch.int32)) and torch.equal(hdet["x_t"].view(torch.int32), xt_want.view(torch.int32))
    check_against_reference(q, half, hdet, "scale 0.5", scale=0.5)
    add = (0.25 - 1.0) / 2.0 - np.log(0.5)
    assert (half["terms"][1:] >= add * half["n"] * (1 - 1e-6)).all()
    # unseeded: torch's generator serves the default
    torch.manual_seed(4)
    r1 = score(q, seed=None, levels_per_launch=3, want_details=True)[1]["eps"]
    torch.manual_seed(4)
    assert torch.equal(score(q, seed=None, levels_per_launch=3, want_details=True)[1]["eps"], r1) and not torch.equal(r1, adet["eps"])


# ----------------------------------------------------------------------------------------------------- 4. entry tool
def test_the_tool_scores_sampled_replicates_and_the_native_backbones(pkg, hip, tmp_path, monkeypatch):
    import json
    import pickle
    from e3diff_amd import biolip, ops
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.dataset import LigandBindingSiteDataset, NoisedAnglesDataset
    from helpers import seeded_state_dict
    from test_structure_score_cpu import load_tool
    tool = load_tool()
    path = biolip.write_synthetic(str(tmp_path / "biolip.pt"), 2, seed=4)
    for key, value in (("timesteps", 6), ("max_seq_len", 64), ("batch_size", 4), ("num_hidden_layers", 2)):
        monkeypatch.setitem(S.CONFIG, key, value)
    ds = NoisedAnglesDataset(LigandBindingSiteDataset(path, None, 64, 0), timesteps=6)
    shapes = {k: tuple(v.shape) for k, v in S.load_model(ds, "").state_dict().items()}
    ckpt = str(tmp_path / "struct.ckpt")
    torch.save(seeded_state_dict(shapes, seed=3), ckpt)
    base = ["--data", path, "--model", ckpt, "--split", "all", "--seeds", "1,2"]
    native = tool.main(base + ["--native", "-o", str(tmp_path / "native.json")])
    rows = json.load(open(tmp_path / "native.json"))
    names = list(ds.feature_names)
    assert list(native.columns) == ["structure_ids", "replicate", "source", "bound", "score", "stderr", "n"] + names + ["rank"]
    assert len(rows) == 2 and sorted(r["structure_ids"] for r in rows) == ["syn00000_B", "syn00001_B"]
    assert all(np.isfinite(r[k]) for r in rows for k in ["bound", "score", "stderr"] + names) and [r["rank"] for r in rows] == [1, 1]
    assert [r["score"] for r in rows] == list(native["score"])
    # two replicates: the native angles as a [T, l, 8] trajectory, and a shifted copy as [l, 8] arrays
    items = [ds.dset[i] for i in range(2)]
    lengths = [int(it["ligand_attn_mask"].sum()) for it in items]
    rep0 = [np.stack([np.zeros((l, 8), dtype=np.float32), it["ligand_angles"][:l].numpy()]) for it, l in zip(items, lengths)]
    rep1 = [(it["ligand_angles"][:l].numpy() + np.float32(0.3)).astype(np.float32) for it, l in zip(items, lengths)]
    for name, rep in (("r0.pkl", rep0), ("r1.pkl", rep1)):
        with open(tmp_path / name, "wb") as f:
            pickle.dump(rep, f)
    files = [str(tmp_path / "r0.pkl"), str(tmp_path / "r1.pkl")]
    res = tool.main(base + ["--samples"] + files + ["-o", str(tmp_path / "scores.pkl")])
    import pandas as pd
    assert res.equals(pd.read_pickle(tmp_path / "scores.pkl")) and len(res) == 4          # one row per (record, replicate)
    assert list(res["replicate"]) == [0, 0, 1, 1] and list(res["source"]) == [files[0]] * 2 + [files[1]] * 2
    assert list(res["structure_ids"]) == list(native["structure_ids"]) * 2
    for sid in set(res["structure_ids"]):                                                 # ranks within a pocket: a permutation
        grp = res[res["structure_ids"] == sid]
        assert sorted(grp["rank"]) == [1, 2] and list(grp.sort_values("score")["rank"]) == [1, 2]
    # the same records through score_structures directly: the same numbers
    def stack(name):
        return torch.stack([items[i][name] for i in (0, 1, 0, 1)]).to(DEV)
    angles = torch.zeros(4, 64, 8)
    for j, (rep, i) in enumerate(((rep0, 0), (rep0, 1), (rep1, 0), (rep1, 1))):
        a = rep[i][-1] if rep[i].ndim == 3 else rep[i]
        angles[j, :a.shape[0]] = torch.from_numpy(a)
    model = S.load_model(ds, ckpt)
    with ops.arithmetic(S.ARITHMETIC):
        want = S.score_structures(model, stack("ligand_attn_mask"), angles, stack("receptor_seq"), stack("receptor_attn_mask"),
                                  stack("receptor_angles"), 6, ds.alpha_beta_terms["betas"], seed=[1, 2], item_ids=[0, 1, 0, 1])
    assert list(res["score"]) == want["score"].tolist() and list(res["bound"]) == want["bound"].tolist()
    assert list(res["stderr"]) == want["stderr"].tolist() and list(res["n"]) == want["n"].tolist()
    for f, name in enumerate(names):
        assert list(res[name]) == (want["per_feature"][:, f] / torch.tensor([lengths[0], lengths[1]] * 2, dtype=torch.float64)).tolist()
    with open(tmp_path / "bad.pkl", "wb") as f:
        pickle.dump([rep1[0][:-1], rep1[1]], f)
    with pytest.raises(ValueError, match="the ligand has"):
        tool.main(base + ["--samples", str(tmp_path / "bad.pkl"), "-o", str(tmp_path / "x.json")])
