"""CPU: scoring supplied structures -- ``ScoreTables`` against the closed forms in float64, tests/structure_score_ref.py
itself (the term's floor, cap and continuity across the wrap cut, the fixed-shape sums), the two new C-ABI symbols, the
argument checks of ``score_structures`` (made before any device work: the model is ``None``) and the command-line tool's
parsing.

Tolerances.  Everything here is float64.  A closed form and the table differ by the roundings of the handful of float64
operations that lead to each (a cumulative product of T factors among them: T 2^-53 relative), so the comparisons allow
1e-11 relative -- four orders above 1000 x 2^-53 = 1.1e-13 and seven below fp32's 2^-24.  ``coef`` itself is ``coef64``
rounded once: compared exactly."""
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import sampler_ref as R
import score_ref as SR
import structure_score_ref as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("e3d_keyed_q_sample_levels_wrap", "e3d_angle_score_items")
REL = 1e-11


def tables(T, scale=1.0):
    from e3diff_amd.structure_model.utils import CosineTables, ScoreTables
    tab = CosineTables(T)
    return tab, ScoreTables(tab, scale)


# ------------------------------------------------------------------------------------------------ ScoreTables
@pytest.mark.parametrize("T", [8, 50, 1000])
def test_score_tables_against_the_closed_forms(pkg, T):
    from e3diff_amd.structure_model.utils import CosineTables
    tab, st = tables(T)
    assert st.coef.dtype == torch.float32 and tuple(st.coef.shape) == (T, 4) and st.coef.is_contiguous()
    assert torch.equal(st.coef, st.coef64.float()) and bool((st.coef[:, 3] == 0).all())      # rounded once
    assert bool(torch.isfinite(st.coef).all()) and bool(torch.isfinite(st.coef64).all())      # no unvisited or non-finite entry
    c = st.coef64.numpy()
    betas = tab.betas.double().numpy()
    want = SS.coefficients(betas)
    assert np.abs(c[:, :3] - want).max() <= REL * np.abs(want).max() and (np.abs(c[:, :3] - want) <= REL * np.abs(want) + 1e-300).all()
    alpha, ab, prev, sigma2 = SS.schedule(betas)
    assert abs(st.prior_ab - ab[-1]) <= REL * ab[-1] and isinstance(st.prior_ab, float)
    # the sampler's own row, in float64 from the same betas
    t64 = CosineTables.from_betas(tab.betas.double())
    rows = np.stack([t64.sqrt_recip_alphas.numpy(), betas, t64.sqrt_one_minus_alphas_cumprod.numpy(), t64.sigma.numpy()], axis=1)
    assert rows.dtype == np.float64 and np.abs(rows[1:, 3] ** 2 - sigma2[1:]).max() <= REL * sigma2.max()
    c1, c2 = SS.posterior_coefficients(betas)
    rng = np.random.default_rng(T)
    x0, eps, eps_hat = (0.002 * rng.standard_normal(257) for _ in range(3))    # small: nothing wraps (k reaches 100)
    for t in sorted({1, 2, T // 2, T - 2, T - 1}):
        x_t = np.sqrt(ab[t]) * x0 + np.sqrt(1.0 - ab[t]) * eps
        mu_post = c1[t] * x0 + c2[t] * x_t
        mu_theta = R.ddpm(rows[t], x_t, eps_hat)[0]
        assert np.abs(x_t).max() < 1 and np.abs(c[t, 0] * (eps_hat - eps)).max() < np.pi
        kl = (mu_post - mu_theta) ** 2 / (2.0 * sigma2[t])          # KL(N(mu_post, s^2) || N(mu_theta, s^2))
        got = c[t, 1] * (c[t, 0] * (eps_hat - eps)) ** 2
        # the difference of two means cancels: each mean carries a handful of float64 roundings of size 2^-53 |mu| (its
        # coefficients' and its own: 32 allowed for the two), which the small difference then shows in full; forming
        # 1 - ab_t, which every coefficient divides by, turns one rounding of ab_t into ab_t / (1 - ab_t) of them
        slack = 32 * 2.0 ** -53 * (1.0 + ab[t] / (1.0 - ab[t])) * (np.abs(mu_post) + np.abs(mu_theta)) * 2 * np.abs(mu_post - mu_theta) / (2.0 * sigma2[t])
        assert (np.abs(got - kl) <= REL * kl + slack).all(), (T, t, float(np.abs(got - kl).max()))
        assert abs(c[t, 1] - 1.0 / (2.0 * float(t64.posterior_variance[t]))) <= REL * c[t, 1] and c[t, 2] == 0.0
    # t = 0: the sampler returns the x0 estimate, k_0 (eps_hat - eps) away from x0
    x_t = np.sqrt(ab[0]) * x0 + np.sqrt(1.0 - ab[0]) * eps
    est = R.ddpm(rows[0], x_t, eps_hat)[0]
    assert rows[0, 3] == 0.0
    d = c[0, 0] * (eps_hat - eps)
    assert (np.abs((est - x0) - (-d)) <= REL * np.abs(d) + 8 * 2.0 ** -53 * np.abs(x_t) / np.sqrt(alpha[0])).all()
    assert abs(c[0, 1] - 1.0 / (2.0 * betas[0])) <= REL * c[0, 1]
    assert abs(c[0, 2] - 0.5 * np.log(2.0 * np.pi * betas[0])) <= REL * abs(c[0, 2]) and c[0, 2] < 0      # a density
    # the Gaussian decoder's negative log-density at the clean angles
    nld = 0.5 * np.log(2 * np.pi * betas[0]) + (x0 - est) ** 2 / (2 * betas[0])
    assert (np.abs(c[0, 1] * d ** 2 + c[0, 2] - nld) <= REL * np.abs(nld) + 1e-9).all()


def test_score_tables_scale_and_its_checks(pkg):
    from e3diff_amd.structure_model.utils import CosineTables, ScoreTables
    tab, st = tables(50)
    half = ScoreTables(tab, 0.5)
    assert bool((st.coef64[1:, 2] == 0).all())
    want = (0.25 - 1.0) / 2.0 - np.log(0.5)
    assert np.abs(half.coef64[1:, 2].numpy() - want).max() <= REL * want and want > 0
    assert torch.equal(half.coef64[0], st.coef64[0]) and torch.equal(half.coef64[:, :2], st.coef64[:, :2])
    # KL(N(m, s^2 sigma^2) || N(m', sigma^2)) = ((s^2 - 1) / 2 - ln s) + (m - m')^2 / (2 sigma^2): add is its first part
    s, sig, dm = 0.5, 0.3, 0.2
    kl = np.log(sig / (s * sig)) + ((s * sig) ** 2 + dm ** 2) / (2 * sig ** 2) - 0.5
    assert abs(kl - (want + dm ** 2 / (2 * sig ** 2))) < 1e-15
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="scale must be positive and finite"):
            ScoreTables(tab, bad)
    # the figures the docstrings quote for T = 1000
    big = ScoreTables(CosineTables(1000))
    sigma = 1.0 / np.sqrt(2.0 * float(big.coef64[999, 1]))
    assert abs(sigma - 0.99995) < 1e-5 and 99.9 < float(big.coef64[:, 0].max()) < 100.0 and big.prior_ab < 1e-8
    print(f"T=1000: sigma_999 = {sigma:.6f}, max k_t = {float(big.coef64[:, 0].max()):.4f} at t = {int(big.coef64[:, 0].argmax())}, "
          f"ab_999 = {big.prior_ab:.3e}")


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("t", [0, 1, 500, 999])
def test_reference_terms_floor_cap_and_continuity(pkg, t):
    _, st = tables(1000, 0.5)
    row = st.coef.numpy()[t].astype(np.float64)
    k, h, add = row[:3]
    eps = R.wrap_pi(np.random.default_rng(t).standard_normal(4369)).astype(np.float32)
    grid = R.wrap_grid().astype(np.float64)
    eh = eps.astype(np.float64) + grid / k                      # k (eps_hat - eps) on and beside every cut
    err, delta, term = SS.elem(row, eh, eps)
    assert (term >= add).all() and (term <= np.pi ** 2 * h + add).all() and (np.abs(delta) <= np.pi).all()
    same = SS.elem(row, eps, eps)
    assert (same[2] == add).all() and (same[0] == 0).all() and (same[1] == 0).all()      # exactly add where eps_hat == eps
    # continuity of delta^2 across the cut: both sides of +-pi, 2 pi apart as numbers
    for cut in (np.pi, -np.pi, 3 * np.pi, -5 * np.pi):
        for gap in (1e-9, 1e-6, 1e-3):
            lo, hi = SS.elem(row, (cut - gap) / k, 0.0), SS.elem(row, (cut + gap) / k, 0.0)
            assert abs(abs(lo[1]) - abs(hi[1])) <= 2 * gap + 1e-12 and abs(lo[1] - hi[1]) > 6.0
            assert abs(lo[2] - hi[2]) <= h * 2 * np.pi * 2 * gap + 1e-9 * h
    s = eps.astype(np.float64) - eh
    assert (R.circ(err, s) <= 8 * 2.0 ** -53 * (np.abs(s) + np.pi)).all()                  # float64 rounding of the wrap
    assert (SS.term_bound(row, eh, eps) > 0).all() and (SS.err_bound(eh, eps) > 0).all()


@pytest.mark.parametrize("L,F", [(1, 4), (63, 8), (64, 8), (65, 12), (257, 8)])
def test_fixed_shape_sums_of_the_reference(L, F):
    rng = np.random.default_rng(10 * L + F)
    v = (rng.standard_normal((L, F)) * 10 ** rng.uniform(-3, 3, (L, F))).astype(np.float32)
    m = rng.random((L, F)) < 0.6
    m[0, 0] = True
    if L > 2:
        m[1] = False                                            # a residue with nothing set
    res, feat, tot, cnt = SS.item_sums_fp32(v, m)
    assert res.dtype == feat.dtype == np.float32 and res.shape == (L,) and feat.shape == (F,) and cnt == int(m.sum())
    # the total is the sequence score's item sum applied to the per-residue values with the any-element-set mask
    want, _ = SR.item_sum_fp32(res, m.any(axis=1))
    assert tot.view(np.int32) == want.view(np.int32)
    for f in range(F):
        assert feat[f].view(np.int32) == SR.item_sum_fp32(v[:, f], m[:, f])[0].view(np.int32)
    exact = v.astype(np.float64)[m].sum()
    bound = L * F * R.U * np.abs(v[m]).sum()
    assert abs(float(tot) - exact) <= bound and abs(float(feat.astype(np.float64).sum()) - exact) <= 2 * bound
    # padding to 2 L with NaN under everything masked out: the same bits
    wide = np.full((2 * L, F), np.nan, dtype=np.float32)
    wide[:L] = np.where(m, v, np.float32(np.nan))
    wm = np.concatenate([m, np.zeros((L, F), dtype=bool)])
    res2, feat2, tot2, cnt2 = SS.item_sums_fp32(wide, wm)
    assert tot2.view(np.int32) == tot.view(np.int32) and np.array_equal(feat2.view(np.int32), feat.view(np.int32)) and cnt2 == cnt
    assert np.array_equal(res2[:L].view(np.int32), res.view(np.int32)) and (res2[L:].view(np.int32) == 0).all()
    empty = SS.item_sums_fp32(wide, np.zeros_like(wm))
    assert empty[2].view(np.int32) == 0 and empty[3] == 0 and (empty[1].view(np.int32) == 0).all()      # +0, not -0


def test_forward_levels_reference_is_the_per_step_draw(pkg):
    tab, _ = tables(50)
    sa, s1 = tab.sqrt_alphas_cumprod.numpy(), tab.sqrt_one_minus_alphas_cumprod.numpy()
    B, L, F = 2, 5, 8
    x0 = R.ddpm_inputs(B * L * F, seed=3)[0].reshape(B, L, F)
    keys = R.padded_keys(R.IDS[:B], L)
    keys[3] = (9, -1)
    steps = (0, 49, 49, 7)
    noise, xt = SS.forward_levels(x0, keys, R.SEEDS[1], steps, sa, s1, 0.5)
    import keyed_ref as K
    for n, t in enumerate(steps):
        z = K.normals(keys.reshape(B, L, 2)[n % B], R.SEEDS[1], 12, t, F)
        live = keys.reshape(B, L, 2)[n % B, :, 1] >= 0
        assert np.abs(R.circ(noise[n][live], 0.5 * z[live])).max() < 1e-12 and (noise[n][~live] == 0).all()
        want = R.wrap_pi(float(sa[t]) * x0[n % B].astype(np.float64) + float(s1[t]) * noise[n])
        assert np.abs(R.circ(xt[n][live], want[live])).max() < 1e-12 and (xt[n][~live] == 0).all()
    assert not np.array_equal(noise[1], noise[2]) and np.array_equal(noise[0, 3], np.zeros(F))
    # stream 12 is its own: not stream 10's draw at the same step
    assert np.abs(K.normals(keys, 7, 12, 5, F) - K.normals(keys, 7, 10, 5, F)).max() > 0.1
    assert SS.level_set(8, 3) == ([0, 3, 6], 3.5)


# ------------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_are_declared_bound_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "e3d_hip.h")).read()
    declared = set(re.findall(r"\b(e3d_[a-z0-9_]+)\s*\(", header))
    lib = pkg.hip.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg.hip.EXPORTS, name
        assert getattr(lib, name) is not None
    for name in ("keyed_q_sample_levels_wrap", "angle_score_items"):
        assert callable(getattr(pkg.ops, name))
    assert pkg.hip.ABI_VERSION == 5 and lib.e3d_abi_version() == 5
    assert "Additions to ABI v5" in header[header.index("scoring supplied structures"):][:700]
    assert pkg.score_structures is __import__("e3diff_amd.structure_model.sample", fromlist=["x"]).score_structures
    assert "score_structures" in pkg.__all__ and pkg.keyed.SCORE_STRUCT == 12
    src = open(os.path.join(ROOT, "e3-invaraint-diffusion-model_amd", "csrc", "e3d_philox.h")).read()
    assert re.search(r"^#define\s+E3D_SCORE_STRUCT_NOISE\s+12\b", src, re.M)
    # argument validation happens before any launch: callable without a GPU
    x = 1024                                                        # a non-null, 16-byte aligned address that is never read

    def forward(*, ptrs=(x,) * 7, max_step=7, T=8, N=4, B=2, L=4, F=8):
        x0, keys, steps, sa, s1, noise, xt = ptrs
        return lib.e3d_keyed_q_sample_levels_wrap(x0, keys, steps, max_step, sa, s1, T, 1.0, 1, noise, xt, N, B, L, F, None)

    def items(*, ptrs=(x,) * 8, outs=(None,) * 6, T=8, N=4, B=2, L=4, F=8):
        eh, e, m, steps, coef, tt, te, cnt = ptrs
        return lib.e3d_angle_score_items(eh, e, m, steps, coef, T, *outs, tt, te, cnt, N, B, L, F, None)
    for i in range(7):
        assert forward(ptrs=tuple(None if j == i else x for j in range(7))) < 0
        assert b"keyed_q_sample_levels_wrap: bad arguments" in lib.e3d_last_error()
    for i in range(8):
        assert items(ptrs=tuple(None if j == i else x for j in range(8))) < 0
        assert b"angle_score_items: bad arguments" in lib.e3d_last_error()
    for F in (6, 0, 1028):
        assert forward(F=F) < 0 and b"F must be a multiple of 4 in [4, 1024]" in lib.e3d_last_error()
    for F in (6, 36, 0):
        assert items(F=F) < 0 and b"angle_score_items: F must be a multiple of 4 in [4, 32]" in lib.e3d_last_error()
    for step in (65536, -1):
        assert forward(max_step=step) < 0 and b"steps up to 65535" in lib.e3d_last_error()
    assert forward(N=3) < 0 and b"N must be a multiple of B" in lib.e3d_last_error()
    assert items(N=3) < 0 and b"N must be a multiple of B" in lib.e3d_last_error()
    for kw in ({"T": 0}, {"N": 0}, {"B": 0}, {"L": 0}):
        assert forward(**kw) < 0 and items(**kw) < 0, kw
    assert forward(L=(1 << 24) + 1) < 0 and b"below 2^24" in lib.e3d_last_error()
    assert forward(ptrs=(x + 4,) + (x,) * 6) < 0 and b"16B aligned" in lib.e3d_last_error()
    assert items(ptrs=(x + 4,) + (x,) * 7) < 0 and items(ptrs=(x, x, x + 2) + (x,) * 5) < 0
    assert items(outs=(x + 8, None, None, None, None, None)) < 0 and b"mask 4B aligned" in lib.e3d_last_error()


# ------------------------------------------------------------------------------------------------ score_structures: argument checks
def test_score_structures_checks_its_arguments_before_any_device_work(pkg):
    from e3diff_amd.structure_model.sample import score_structures
    from e3diff_amd.structure_model.utils import CosineTables
    from helpers import synthetic_pockets
    B, L, F, T = 3, 16, 8, 8
    pk = synthetic_pockets(B, L, seed=1, lig_range=(3, 9))
    angles = torch.zeros(B, L, F)
    betas = CosineTables(T).betas

    def score(angles=angles, T=T, betas=betas, **kw):      # no model: nothing below may reach it
        return score_structures(None, kw.pop("ligand_mask", pk["ligand_attn_mask"]), angles, kw.pop("receptor_seq", pk["receptor_seq"]),
                                pk["receptor_attn_mask"], pk["receptor_angles"], T, betas, **kw)
    for bad, msg in ((torch.zeros(B, L), "angles must be a"), (torch.zeros(B, L, 6), "multiple of 4"),
                     (torch.zeros(B, L, 36), "multiple of 4 in")):
        with pytest.raises(ValueError, match=msg):
            score(bad, seed=1)
    with pytest.raises(ValueError, match="ligand_mask must be"):
        score(seed=1, ligand_mask=pk["ligand_attn_mask"][:, :-1])
    with pytest.raises(ValueError, match="receptor_seq must be"):
        score(seed=1, receptor_seq=pk["receptor_seq"][:2])
    with pytest.raises(ValueError, match="betas for total_timesteps"):
        score(seed=1, T=9)
    with pytest.raises(ValueError, match="item_ids key the seeded draws"):
        score(item_ids=[1, 2, 3])
    with pytest.raises(ValueError, match="either injected noises or a seed"):
        score(seed=1, noises=torch.zeros(T, B, L, F))
    with pytest.raises(ValueError, match="noises must be a tensor of"):
        score(noises=torch.zeros(T - 1, B, L, F))
    for bad in (0, -2):
        with pytest.raises(ValueError, match="levels must be a positive stride"):
            score(seed=1, levels=bad)
    with pytest.raises(ValueError, match="details must be a dict"):
        score(seed=1, details=[])
    with pytest.raises(ValueError, match="single seed"):
        score(seed=[1, 2], details={})
    for bad in (torch.ones(B, L), torch.ones(B, L, F, dtype=torch.uint8), torch.ones(B, L + 1, dtype=torch.bool)):
        with pytest.raises(ValueError, match="score_mask must be a bool tensor"):
            score(seed=1, score_mask=bad)
    with pytest.raises(ValueError, match="levels_per_launch"):
        score(seed=1, levels_per_launch=0)
    with pytest.raises(ValueError, match="seed must lie in"):
        score(seed=[1, -2])
    with pytest.raises(ValueError, match="empty list of seeds"):
        score(seed=[])
    with pytest.raises(ValueError, match="3 item ids|item ids for a batch"):
        score(seed=1, item_ids=[1, 2])
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="scale must be positive"):
            score(seed=1, scale=bad)
    big = 65537
    with pytest.raises(ValueError, match="keyed streams hold steps up to 65535"):
        score(seed=1, T=big, betas=torch.full((big,), 0.01))
    with pytest.raises(AttributeError):                              # T - 1 == 65535 fits; unseeded, any T does
        score(seed=1, T=big - 1, betas=torch.full((big - 1,), 0.01), levels=4096)
    with pytest.raises(AttributeError):                              # every check passed: the model is asked for its device
        score(seed=1, score_mask=torch.ones(B, L, F, dtype=torch.bool))
    params = inspect.signature(score_structures).parameters
    assert list(params) == ["model", "ligand_mask", "angles", "receptor_seq", "receptor_mask", "receptor_angle", "total_timesteps",
                            "betas", "levels", "seed", "item_ids", "noises", "scale", "score_mask", "trim_padding",
                            "levels_per_launch", "details"]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(params)[8:]) and "pack" not in params


# ------------------------------------------------------------------------------------------------ the tool
def load_tool():
    """tools/score_structures.py as a module (tests/test_structure_score_gpu.py runs its ``main``)."""
    spec = importlib.util.spec_from_file_location("score_structures_tool", os.path.join(ROOT, "tools", "score_structures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_parses_its_arguments(capsys):
    tool = load_tool()
    base = ["--data", "biolip.pt", "--model", "m.ckpt", "-o", "scores.json"]
    a = tool.parse_args(base + ["--native"])
    assert a.native and a.samples is None and a.seeds == [0] and a.levels is None and a.split == "test"
    a = tool.parse_args(base[:-1] + ["s.pkl", "--samples", "a.pkl", "b.pkl", "--seeds", "1,2,0x10", "--levels", "5"])
    assert a.samples == ["a.pkl", "b.pkl"] and a.seeds == [1, 2, 16] and a.levels == 5 and a.output == "s.pkl" and not a.native
    for bad, text in ((base, "one of the arguments --samples --native is required"),
                      (base + ["--native", "--samples", "x.pkl"], "not allowed with"),
                      (base + ["--samples"], "expected at least one argument"),
                      (base + ["--native", "--seeds", "1,x"], "seeds must be integers"),
                      (base + ["--native", "--seeds", ""], "one or more integers"),
                      (base + ["--native", "--seeds", "3,3"], "given twice"),
                      (base + ["--native", "--levels", "0"], "positive integer"),
                      (base[:-1] + ["scores.csv", "--native"], ".json or .pkl"),
                      (["--native", "-o", "s.json", "--model", "m"], "--data")):
        with pytest.raises(SystemExit) as stop:
            tool.parse_args(bad)
        assert stop.value.code == 2 and text in capsys.readouterr().err, bad
    with pytest.raises(SystemExit) as stop:
        tool.parse_args(["--help"])
    text = capsys.readouterr().out
    assert stop.value.code == 0
    for word in ("--samples", "--native", "--seeds", "--levels", "nats per angle", "not a certified"):
        assert word in text, word
    assert tool.ranks_within([0, 1, 0, 1, 0], [0.5, 2.0, 0.25, float("nan"), 0.5]) == [2, 1, 1, 2, 3]
    with pytest.raises(ValueError, match="1abc_B: the ligand has 3 residues, entry 0 of x.pkl 4"):
        tool.replicate_angles([np.zeros((4, 8), dtype=np.float32)], [3], ["1abc_B"], 16, 8, "x.pkl")
    with pytest.raises(ValueError, match="holds 2 backbones, the dataset 1"):
        tool.replicate_angles([np.zeros((3, 8), dtype=np.float32)] * 2, [3], ["1abc_B"], 16, 8, "x.pkl")
    got = tool.replicate_angles([np.ones((3, 8), dtype=np.float32)], [3, 5], ["a", "b"], 16, 8, "x.pkl")
    assert tuple(got.shape) == (1, 16, 8) and float(got.sum()) == 24.0
