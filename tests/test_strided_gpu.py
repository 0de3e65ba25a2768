"""GPU: strided (DDIM / respaced) structure sampling.  ``e3d_strided_step_wrap`` against the numpy float64 statement
(tests/strided_ref.py) evaluated from the same fp32 table row; its keyed form against the unkeyed form fed the keyed
draws; and chains: eager against graph replay, no draws at eta = 0, seeded chains that follow the item through batch,
frame and launch mode, the ancestral path unchanged, and the last entry = the wrapped x0 estimate.

Error bound of one update (u = 2^-24).  The update has eight fp32 roundings, each at most u of
    G = a_s rsa (|x| + |s1m e|) + |c_dir e| + |sigma z|,
so |got - ref| <= 10 u G (eight to first order, ten covers second order).  With ``wrap`` the comparison is by circular
distance and wrap_pi's two additions add 4 u (|v| + pi), v the value before the wrap.  With ``wrap_x0`` the x0 estimate is
wrapped before it is scaled by a_s: elements whose float64 x0 lies within 8 u rsa (|x| + |s1m e|) of a cut (where a
legitimate rounding flips x0 by 2 pi) are excluded -- under 1 % of them -- and on the rest G stays as above (it bounds
the wrapped form's a_s |wrap(x0)| term by term: |wrap(x0)| <= |x0| <= rsa (|x| + |s1m e|)), while the inner wrap_pi's two
additions add a_s 4 u (|x0| + pi), the same allowance as for the outer wrap, scaled by a_s.  (Putting a_s |wrap(x0)| in
the PLACE of the x0 term of G cannot hold for any fp32 evaluation: at t = 980 of the 1000-step table rsa = 33.8, x0 reaches
260 and carries roundings of 260 u that the wrap does not shrink, while |wrap(x0)| <= pi.)
"""
import warnings

import numpy as np
import pytest
import torch

import strided_ref as R
from test_keyed_sampling_gpu import WRAPPED_TOL, _structure_setup, _wrapped_diff, key_table

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
N_BIG = 2048 * 256 * 4 + 5                 # more float4 groups than the capped grid has threads, plus a tail
SIZES = (1, 3, 4, 5, 8 * 37, N_BIG)
TIMESTEPS = (999, 980, 500, 20, 0)         # 999 is not visited at step 20: its row is NaN
T_FULL, STEP = 1000, 20


def _t(t):
    return torch.full((1,), t, dtype=torch.int64, device=DEV)


@pytest.fixture(scope="module")
def data(pkg, hip):
    """Inputs shared by the kernel tests (smaller sizes are prefixes of the largest) and the three tables."""
    from e3diff_amd.structure_model.utils import CosineTables, StridedTables
    rng = np.random.default_rng(20)
    x = rng.uniform(-np.pi, np.pi, N_BIG).astype(np.float32)
    x[x >= np.float32(np.pi)] = -np.float32(np.pi)
    e = rng.standard_normal(N_BIG).astype(np.float32)
    z = rng.standard_normal(N_BIG).astype(np.float32)
    tab = CosineTables(T_FULL)
    order = list(reversed(range(0, T_FULL, STEP)))
    tables = {eta: StridedTables(tab, order, eta) for eta in (0.0, 0.5, 1.0)}
    return {"x": x, "e": e, "z": z, "dx": torch.from_numpy(x).to(DEV), "de": torch.from_numpy(e).to(DEV),
            "dz": torch.from_numpy(z).to(DEV), "tables": tables,
            "coef": {eta: st.coef.to(DEV) for eta, st in tables.items()}}


def _bound(row, parts, pre, wrap, wrap_x0):
    b = 10 * U * parts["G"]
    if wrap_x0:
        b = b + float(row[2]) * 4 * U * (np.abs(parts["x0_raw"]) + np.pi)
    if wrap:
        b = b + 4 * U * (np.abs(pre) + np.pi)
    return b


def _check(row, got, x, e, z, wrap, wrap_x0, what):
    """Assert the bound of the module docstring on every (non-excluded) element; returns the worst error / bound."""
    ref, parts = R.update(row, x, e, z, wrap=False, wrap_x0=wrap_x0)       # ref before the outer wrap
    got = got.astype(np.float64)
    err = R.circ(got, ref) if wrap else np.abs(got - ref)
    bound = _bound(row, parts, ref, wrap, wrap_x0)
    keep = np.ones(ref.shape, dtype=bool)
    if wrap_x0:
        cut = np.pi + 2 * np.pi * np.round((parts["x0_raw"] - np.pi) / (2 * np.pi))
        keep = np.abs(parts["x0_raw"] - cut) >= 8 * U * parts["x0_mag"]
        assert 1.0 - keep.mean() < 0.01, (what, "excluded share", 1.0 - keep.mean())
    if wrap:
        assert np.abs(got).max() <= np.pi + 1e-6
    ratio = (err[keep] / bound[keep]).max() if keep.any() else 0.0
    assert (err[keep] <= bound[keep]).all(), (what, "worst |got - ref| / bound", ratio)
    units = (err[keep] / (U * parts["G"][keep])).max() if (keep.any() and not wrap and not wrap_x0) else None
    return ratio, units


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_kernel_against_the_float64_ref(pkg, hip, data, eta, wrap):
    ops = pkg.ops
    coef, rows = data["coef"][eta], data["tables"][eta].coef.numpy()
    worst, worst_units = 0.0, 0.0
    for t in TIMESTEPS:
        for n in SIZES:
            got = ops.strided_step_wrap(data["dx"][:n], data["de"][:n], data["dz"][:n], coef, _t(t), wrap=wrap).cpu().numpy()
            if np.isnan(rows[t]).any():                                     # a row that is not visited: NaN everywhere
                assert t == 999 and np.isnan(got).all()
                continue
            r, units = _check(rows[t], got, data["x"][:n], data["e"][:n], data["z"][:n], wrap, False, (t, n, eta, wrap))
            worst = max(worst, r)
            worst_units = max(worst_units, units or 0.0)
    print(f"strided kernel eta={eta} wrap={wrap}: worst |got - ref| / bound = {worst:.3f}"
          + ("" if wrap else f"; worst |got - ref| = {worst_units:.2f} u G (bound 10)"))


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_kernel_with_wrapped_x0(pkg, hip, data, eta, wrap):
    ops = pkg.ops
    coef, rows = data["coef"][eta], data["tables"][eta].coef.numpy()
    worst = 0.0
    for t in TIMESTEPS:
        for n in (5, 8 * 37, N_BIG):
            got = ops.strided_step_wrap(data["dx"][:n], data["de"][:n], data["dz"][:n], coef, _t(t), wrap=wrap,
                                        wrap_x0=True).cpu().numpy()
            if np.isnan(rows[t]).any():
                assert t == 999 and np.isnan(got).all()
                continue
            r, _ = _check(rows[t], got, data["x"][:n], data["e"][:n], data["z"][:n], wrap, True, (t, n, eta, wrap))
            worst = max(worst, r)
            if t == 0 and not wrap:      # a_s = 1, c_dir = sigma = 0: the step returns the wrapped x0 estimate itself
                assert np.abs(got).max() <= np.pi + 1e-6
    print(f"strided kernel wrap_x0 eta={eta} wrap={wrap}: worst |got - ref| / bound = {worst:.3f}")


def test_out_may_alias_x(pkg, hip, data):
    ops = pkg.ops
    for n in (5, N_BIG):
        for eta, wrap_x0 in ((0.0, False), (1.0, True)):
            args = (data["de"][:n], data["dz"][:n], data["coef"][eta], _t(500))
            want = ops.strided_step_wrap(data["dx"][:n], *args, wrap=True, wrap_x0=wrap_x0)
            x = data["dx"][:n].clone()
            got = ops.strided_step_wrap(x, *args, wrap=True, wrap_x0=wrap_x0, out=x)
            assert got is x and torch.equal(got, want)
    keys = key_table().to(DEV)
    rows = keys.shape[0]
    x, e = data["dx"][:rows * 8].reshape(rows, 8), data["de"][:rows * 8].reshape(rows, 8)
    want = ops.keyed_strided_step_wrap(x, e, data["coef"][1.0], _t(500), keys, 7)
    xa = x.clone()
    assert torch.equal(ops.keyed_strided_step_wrap(xa, e, data["coef"][1.0], _t(500), keys, 7, out=xa), want)


@pytest.mark.parametrize("bad", [-1, T_FULL])
def test_step_index_outside_the_table_gives_nan(pkg, hip, data, bad):
    ops = pkg.ops
    n = 4 * 300 + 3
    x, e, z, coef = data["dx"][:n], data["de"][:n], data["dz"][:n], data["coef"][1.0]
    want = ops.strided_step_wrap(x, e, z, coef, _t(500))
    out = torch.zeros(n, device=DEV)
    ops.strided_step_wrap(x, e, z, coef, _t(bad), out=out)
    assert torch.isnan(out).all()
    assert torch.equal(ops.strided_step_wrap(x, e, z, coef, _t(500), out=out), want)
    keys = key_table().to(DEV)
    rows = keys.shape[0]
    xk, ek = data["dx"][:rows * 8].reshape(rows, 8), data["de"][:rows * 8].reshape(rows, 8)
    want = ops.keyed_strided_step_wrap(xk, ek, coef, _t(500), keys, 3)
    out = torch.zeros(rows, 8, device=DEV)
    ops.keyed_strided_step_wrap(xk, ek, coef, _t(bad), keys, 3, out=out)
    assert torch.isnan(out).all()
    assert torch.equal(ops.keyed_strided_step_wrap(xk, ek, coef, _t(500), keys, 3, out=out), want)


def test_eta_zero_reads_nothing_through_noise(pkg, hip, data):
    ops = pkg.ops
    for n in (5, 8 * 37, N_BIG):
        x, e = data["dx"][:n], data["de"][:n]
        poison = torch.full((n,), float("nan"), device=DEV)
        for t in (980, 500, 0):
            for wrap in (False, True):
                a = ops.strided_step_wrap(x, e, None, data["coef"][0.0], _t(t), wrap=wrap)
                b = ops.strided_step_wrap(x, e, poison, data["coef"][0.0], _t(t), wrap=wrap)
                assert torch.isfinite(a).all() and torch.equal(a, b)
        # eta = 1: the last visited step has sigma == 0 too
        b = ops.strided_step_wrap(x, e, poison, data["coef"][1.0], _t(0))
        assert torch.equal(b, ops.strided_step_wrap(x, e, None, data["coef"][1.0], _t(0)))


# ------------------------------------------------------------------------------------------------ keyed form
def test_keyed_form_equals_the_unkeyed_form_with_the_keyed_draws(pkg, hip, data):
    ops = pkg.ops
    keys = key_table().to(DEV)
    rows = keys.shape[0]
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(rows, 8, generator=g) * 6 - 3).to(DEV)
    eps = torch.randn(rows, 8, generator=g).to(DEV)
    seed = 77
    for eta in (0.0, 0.5, 1.0):
        coef = data["coef"][eta]
        for t in (980, 500, 20, 0):
            z = ops.keyed_draws(keys, seed, 1, t, ops.KEYED_NORMAL, 8)
            for wrap, wrap_x0 in ((True, False), (False, False), (True, True)):
                kw = dict(wrap=wrap, wrap_x0=wrap_x0)
                got = ops.keyed_strided_step_wrap(x, eps, coef, _t(t), keys, seed, **kw)
                want = ops.strided_step_wrap(x, eps, z, coef, _t(t), **kw)
                assert torch.equal(got, want), (eta, t, wrap, wrap_x0)
                mean = ops.strided_step_wrap(x, eps, None, coef, _t(t), **kw)
                assert torch.equal(got[-1], mean[-1])                      # sentinel row: no noise
                if eta == 0.0 or t == 0:
                    assert torch.equal(got, mean)                          # sigma == 0: the mean
                else:
                    assert not torch.equal(got[:-1], mean[:-1])
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.keyed_strided_step_wrap(x[:, :6].contiguous(), eps[:, :6].contiguous(), coef, _t(0), keys, seed)


# ------------------------------------------------------------------------------------------------ chains
T_CHAIN, STEP_CHAIN = 12, 3
IDS = [11, (1 << 35) + 2, 7, 123456]


@pytest.fixture(scope="module")
def setup(pkg, hip):
    model, pk, tab = _structure_setup(B=4, L=128, T=T_CHAIN)
    g = torch.Generator().manual_seed(5)
    from e3diff_amd.structure_model.utils import modulo_with_wrapped_range
    x_T = modulo_with_wrapped_range(torch.randn(4, 128, 8, generator=g)).to(DEV)
    order = list(reversed(range(0, T_CHAIN, STEP_CHAIN)))
    noises = torch.randn(len(order), 4, 128, 8, generator=g).to(DEV)
    return {"model": model, "pk": pk, "tab": tab, "x_T": x_T, "noises": noises, "order": order}


def _args(s, sel=None):
    pk = s["pk"] if sel is None else {k: v[sel].contiguous() for k, v in s["pk"].items()}
    x_T = s["x_T"] if sel is None else s["x_T"][sel].contiguous()
    return (s["model"], pk["ligand_attn_mask"], x_T, pk["receptor_seq"], pk["receptor_attn_mask"], pk["receptor_angles"],
            T_CHAIN, s["tab"])


def _graphed_chain(S, s, eta, noises=None, seed=None, wrap_x0=False):
    """The padded chain with every step replayed from one captured GraphedReverseStep (p_sample_loop itself never
    replays chains of four steps)."""
    from e3diff_amd import keyed
    from e3diff_amd.structure_model.utils import StridedTables
    model, pk, order = s["model"], s["pk"], s["order"]
    st = StridedTables(s["tab"], order, eta)
    cache = model.encode_receptor(pk["receptor_seq"], pk["receptor_angles"], pk["receptor_attn_mask"])
    mod_rows = model.timestep_modulation(torch.tensor(order, device=DEV, dtype=torch.long))
    mod_table = torch.zeros((T_CHAIN, mod_rows.shape[1]), device=DEV)
    mod_table[order] = mod_rows
    keys = None if seed is None else keyed.padded_keys(IDS, 128, DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        g = S.GraphedReverseStep(model, pk["ligand_attn_mask"].contiguous().float(), cache, s["tab"], s["x_T"],
                                 draw=noises is None, mod_table=mod_table, row_keys=keys, seed=seed, strided=st,
                                 wrap_x0=wrap_x0)
    out, x = [], s["x_T"]
    for n, i in enumerate(order):
        x = g.step(i, x, None if noises is None else noises[n])
        out.append(x.clone())
    return torch.stack(out)


@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_eager_chain_equals_the_graphed_chain(pkg, hip, setup, eta):
    from e3diff_amd.structure_model import sample as S
    kw = dict(return_device=True, update="strided", eta=eta)
    with torch.no_grad():
        eager = S.p_sample_loop(*_args(setup), noises=setup["noises"], step=STEP_CHAIN, use_graph=False, **kw)
        graph = _graphed_chain(S, setup, eta, noises=setup["noises"])
    assert eager.shape == (4, 4, 128, 8) and torch.isfinite(eager).all() and eager.abs().max() <= 3.1416
    assert torch.equal(eager, graph)
    if eta == 1.0:      # the noise term is live: other draws, another chain
        other = S.p_sample_loop(*_args(setup), noises=setup["noises"].flip(0), step=STEP_CHAIN, use_graph=False, **kw)
        assert not torch.equal(other, eager)
    # and through p_sample_loop's own capture (six steps: long enough to replay)
    e2 = S.p_sample_loop(*_args(setup), noises=setup["noises"].repeat(2, 1, 1, 1)[:6], step=2, use_graph=False, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        g2 = S.p_sample_loop(*_args(setup), noises=setup["noises"].repeat(2, 1, 1, 1)[:6], step=2, use_graph=True, **kw)
    assert e2.shape[0] == 6 and torch.equal(e2, g2)


def test_eta_zero_draws_no_random_numbers(pkg, hip, setup):
    from e3diff_amd.structure_model import sample as S
    kw = dict(return_device=True, update="strided", eta=0.0, step=STEP_CHAIN)
    runs = []
    for seed, extra in ((1, {}), (2, {}), (3, {"step": 2, "use_graph": True})):
        torch.manual_seed(seed)
        cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
        runs.append(S.p_sample_loop(*_args(setup), **{**kw, **extra}))
        assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(DEV), dev_state)
    assert torch.equal(runs[0], runs[1]) and torch.isfinite(runs[2]).all()
    torch.manual_seed(4)
    dev_state = torch.cuda.get_rng_state(DEV)
    with torch.no_grad():
        graph = _graphed_chain(S, setup, 0.0)
    assert torch.equal(torch.cuda.get_rng_state(DEV), dev_state) and torch.equal(graph, runs[0])
    # eta = 1 with default draws does depend on the generator
    torch.manual_seed(1)
    a = S.p_sample_loop(*_args(setup), **{**kw, "eta": 1.0})
    torch.manual_seed(2)
    assert not torch.equal(a, S.p_sample_loop(*_args(setup), **{**kw, "eta": 1.0}))


def _seeded(S, s, seed, sel=None, **kw):
    sel = list(range(4)) if sel is None else sel
    args = list(_args(s, sel))
    args[2] = S.keyed_x_T(seed, [IDS[i] for i in sel], 128, 8, device=DEV)
    return S.p_sample_loop(*args, return_device=True, step=STEP_CHAIN, seed=seed, item_ids=[IDS[i] for i in sel],
                           update="strided", eta=1.0, **kw)


def test_seeded_strided_chain_follows_the_item(pkg, hip, setup):
    from e3diff_amd.structure_model import sample as S
    seed = 2024
    base = _seeded(S, setup, seed)
    assert base.shape == (4, 4, 128, 8) and torch.isfinite(base).all()
    valid = setup["pk"]["ligand_attn_mask"].bool()[None, :, :, None].expand_as(base)
    assert torch.equal(_seeded(S, setup, seed), base)
    assert _wrapped_diff(_seeded(S, setup, seed + 1), base, valid) > 0.1
    rev = _seeded(S, setup, seed, sel=[3, 2, 1, 0])
    for b in range(4):
        assert torch.equal(rev[:, 3 - b], base[:, b])
    one = _seeded(S, setup, seed, sel=[2])
    assert _wrapped_diff(one[:, 0], base[:, 2], valid[:, 2]) < WRAPPED_TOL
    trim = _seeded(S, setup, seed, trim_padding=True)
    packed = _seeded(S, setup, seed, pack=True)
    assert _wrapped_diff(trim, base, valid) < WRAPPED_TOL
    assert _wrapped_diff(packed, base, valid) < WRAPPED_TOL
    assert _wrapped_diff(packed, trim, valid) < WRAPPED_TOL
    # eager and graphed: the same kernels on the same frame
    s2 = dict(setup, x_T=S.keyed_x_T(seed, IDS, 128, 8, device=DEV))
    with torch.no_grad():
        graph = _graphed_chain(S, s2, 1.0, seed=seed)
    assert _wrapped_diff(graph, base, valid) < WRAPPED_TOL and torch.equal(graph, base)
    # the draw at timestep t is the ancestral keyed chain's draw at t: one seeded p_sample step of each kind
    from e3diff_amd.structure_model.utils import StridedTables
    st = StridedTables(setup["tab"], setup["order"], 1.0)
    a = list(_args(setup))[:6] + [6, setup["tab"]]
    keys = pkg.keyed.padded_keys(IDS, 128, DEV)
    z = pkg.ops.keyed_draws(keys, seed, 1, 6, pkg.ops.KEYED_NORMAL, 8).reshape(4, 128, 8)
    assert torch.equal(S.p_sample(*a, seed=seed, item_ids=IDS, strided=st), S.p_sample(*a, noise=z, strided=st))
    assert torch.equal(S.p_sample(*a, seed=seed, item_ids=IDS), S.p_sample(*a, noise=z))


@pytest.mark.parametrize("step", [1, 3])
def test_ancestral_update_is_unchanged(pkg, hip, setup, step):
    """update="ancestral" (the default) against _reverse_step driven by hand with the one-step coefficients."""
    from e3diff_amd.structure_model import sample as S
    s = setup
    model, pk, tab = s["model"], s["pk"], s["tab"]
    order = list(reversed(range(0, T_CHAIN, step)))
    g = torch.Generator().manual_seed(9)
    noises = torch.randn(len(order), 4, 128, 8, generator=g).to(DEV)
    got = S.p_sample_loop(*_args(s), noises=noises, return_device=True, step=step, use_graph=False)
    same = S.p_sample_loop(*_args(s), noises=noises, return_device=True, step=step, use_graph=False, update="ancestral")
    with torch.no_grad():
        cache = model.encode_receptor(pk["receptor_seq"], pk["receptor_angles"], pk["receptor_attn_mask"])
        mod_rows = model.timestep_modulation(torch.tensor(order, device=DEV, dtype=torch.long))
        mask = pk["ligand_attn_mask"].contiguous().float()
        x, want = s["x_T"], []
        for n, i in enumerate(order):
            eps = model.decode(torch.full((4,), i, device=DEV, dtype=torch.long), x, mask, cache, mod=mod_rows[n:n + 1])
            noise, sigma = (None, 0.0) if i == 0 else (noises[n], float(tab.sigma[i]))
            x = pkg.ops.ddpm_step_wrap(x, eps.contiguous(), noise, float(tab.sqrt_recip_alphas[i]), float(tab.betas[i]),
                                       float(tab.sqrt_one_minus_alphas_cumprod[i]), sigma, wrap=True)
            want.append(x)
        by_hand = torch.stack([S._reverse_step(model, mask, xx, None, None, None, i, tab, noises[n], cache, None, True,
                                               mod=mod_rows[n:n + 1])
                               for n, (i, xx) in enumerate(zip(order, [s["x_T"]] + want[:-1]))])
    assert torch.equal(got, torch.stack(want)) and torch.equal(same, got) and torch.equal(by_hand, got)
    with pytest.raises(ValueError, match="strided"):
        S.p_sample_loop(*_args(s), noises=noises, step=step, update="ancestral", eta=0.5)


@pytest.mark.parametrize("eta,wrap_x0", [(0.0, False), (1.0, True)])
def test_last_entry_is_the_wrapped_x0_estimate(pkg, hip, setup, eta, wrap_x0):
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.utils import StridedTables
    s = setup
    model, pk, order = s["model"], s["pk"], s["order"]
    traj = S.p_sample_loop(*_args(s), noises=s["noises"], return_device=True, step=STEP_CHAIN, use_graph=False,
                           update="strided", eta=eta, wrap_x0=wrap_x0)
    with torch.no_grad():
        cache = model.encode_receptor(pk["receptor_seq"], pk["receptor_angles"], pk["receptor_attn_mask"])
        mod_rows = model.timestep_modulation(torch.tensor(order, device=DEV, dtype=torch.long))
        eps = model.decode(torch.zeros(4, device=DEV, dtype=torch.long), traj[-2], pk["ligand_attn_mask"].contiguous().float(),
                           cache, mod=mod_rows[-1:])
    row = StridedTables(s["tab"], order, eta).coef[0].numpy()
    assert row[2] == 1.0 and row[3] == 0.0 and row[4] == 0.0
    x, e = traj[-2].cpu().numpy().ravel(), eps.cpu().numpy().ravel()
    # t = 0: a_s = 1, c_dir = sigma = 0, so the update is wrap_pi of the x0 estimate (wrapped once more or not)
    x0 = (x.astype(np.float64) - float(row[0]) * e.astype(np.float64)) * float(row[1])
    assert R.circ(R.update(row, x, e, None, wrap=True, wrap_x0=wrap_x0)[0], R.wrap_pi(x0)).max() < 1e-12
    r, _ = _check(row, traj[-1].cpu().numpy().ravel(), x, e, None, True, wrap_x0, ("last entry", eta, wrap_x0))
    print(f"last entry eta={eta} wrap_x0={wrap_x0}: worst |got - wrap(x0)| / bound = {r:.3f}")


def test_entry_point_passes_the_update_through(pkg, hip, tmp_path, monkeypatch):
    """sample() hands STEP, UPDATE, ETA and WRAP_X0 to the chain."""
    from e3diff_amd import biolip
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.dataset import LigandBindingSiteDataset, NoisedAnglesDataset
    from e3diff_amd.structure_model.model import ConditionalBertForDiffusion as M
    path = biolip.write_synthetic(str(tmp_path / "biolip.pt"), 3, seed=4)
    L = 64
    ds = NoisedAnglesDataset(LigandBindingSiteDataset(path, None, L, 0), timesteps=5)
    c = dict(hidden_size=768, num_attention_heads=12, intermediate_size=1024, num_hidden_layers=2,
             max_position_embeddings=L, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    torch.manual_seed(3)
    model = M(BertConfig(**c), BertConfig(**c, is_decoder=True, add_cross_attention=True),
              feature_names=ds.feature_names, loss_func=[M.diheral_loss_func] * 8).eval().to(DEV)
    monkeypatch.setitem(S.CONFIG, "batch_size", 3)
    monkeypatch.setattr(S, "STEP", 2)
    ancestral = S.sample(model, ds, seed=31)
    monkeypatch.setattr(S, "UPDATE", "strided")
    monkeypatch.setattr(S, "WRAP_X0", True)
    runs = []
    for s in (1, 2):
        torch.manual_seed(s)                       # eta = 0 and a keyed x_T: torch's generator plays no part
        runs.append(S.sample(model, ds, seed=31))
    assert len(runs[0]) == 3
    for a, b, c0 in zip(runs[0], runs[1], ancestral):
        assert a.shape == c0.shape and a.shape[0] == 3 and np.isfinite(a).all() and np.abs(a).max() <= 3.1416
        assert np.array_equal(a, b) and not np.array_equal(a, c0)
    monkeypatch.setattr(S, "ETA", 1.0)
    noisy = S.sample(model, ds, seed=31)
    assert np.isfinite(noisy[0]).all() and not np.array_equal(noisy[0], runs[0][0])
