"""GPU: multistep (DPM-Solver++ 2M, capped weight) structure sampling.  ``e3d_multistep_step_wrap`` against the numpy
float64 statement (tests/multistep_ref.py) evaluated from the same fp32 table row, output and stored history alike; the
rows without an extrapolation term against ``e3d_strided_step_wrap`` bit for bit; aliasing; the solver error of a chain
of kernel launches on a model with a closed-form solution, against DDIM's; and chains: eager against a loop driven by
hand and against graph replay, no draws, every frame, held positions under a seed, the entry point.

Error bound of one update (u = 2^-24; x0_mag = rsa (|x| + |s1m e|), the magnitude the x0 estimate is rounded at).  Each
fp32 rounding costs at most u of the magnitude of its result, and the inputs (the row, x, e, the previous estimate) are
the reference's own, so to first order:
    x0 = fmaf(-s1m, e, x) * rsa           two roundings, each <= u x0_mag; the bound takes three:
                                          E_x0 = 3 u x0_mag   (+ 4 u (|x0| + pi) under wrap_x0: wrap_pi's two additions,
                                          the allowance test_strided_gpu.py derives, with x0 the value before the wrap)
    v  = fmaf(a_s, x0, c_dir * e)         the product: u |c_dir e|; the fma: u (a_s |x0| + |c_dir e|); x0's own error
                                          comes through a_s:   E_v = a_s E_x0 + u (a_s |x0| + 2 |c_dir e|)
    d  = x0 - prev                        x0's error, one rounding u (|x0| + |prev|), and under wrap 4 u (|d| + pi):
                                          E_d = E_x0 + u (|x0| + |prev|) (+ 4 u (|d| + pi))
    v  = fmaf(c_1, d, v)                  d's error through |c_1|, one rounding u (|c_1 d| + a_s |x0| + |c_dir e|)
where |x0| is x0_mag, or the wrapped estimate's magnitude under wrap_x0.  The sum is taken times 1.25 for the second-order
terms (test_strided_gpu.py's eight roundings bounded by ten), and the outer wrap adds 4 u (|v| + pi), the comparison
then being by circular distance.  The stored history is checked against E_x0 times 1.25.  A value that a wrap maps lies
within its rounding reach of a cut for some elements, where a legitimate rounding flips the result by 2 pi: elements
whose float64 x0 lies within 8 u x0_mag of a cut (wrap_x0) or whose float64 d lies within twice its pre-wrap error
2 (E_x0 + u (|x0| + |prev|)) of one (wrap) are excluded; their share stays under 1 % (expected: of the order 1e-5).
"""
import warnings

import numpy as np
import pytest
import torch

import multistep_ref as R
from test_keyed_sampling_gpu import WRAPPED_TOL, _structure_setup, _wrapped_diff

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
N_BIG = 2048 * 256 * 4 + 5                 # more float4 groups than the capped grid has threads, plus a tail
SIZES = (1, 3, 4, 5, 8 * 37, N_BIG)
TIMESTEPS = (999, 980, 960, 500, 20, 0)    # 999 is not visited at step 20: its row is NaN; 980 and 0 have c_1 == 0
T_FULL, STEP = 1000, 20


def _t(t):
    return torch.full((1,), t, dtype=torch.int64, device=DEV)


@pytest.fixture(scope="module")
def data(pkg, hip):
    """Inputs shared by the kernel tests (smaller sizes are prefixes of the largest) and the two tables."""
    from e3diff_amd.structure_model.utils import CosineTables, MultistepTables, StridedTables
    rng = np.random.default_rng(21)
    x = rng.uniform(-np.pi, np.pi, N_BIG).astype(np.float32)
    x[x >= np.float32(np.pi)] = -np.float32(np.pi)
    e = rng.standard_normal(N_BIG).astype(np.float32)
    prev = rng.uniform(-np.pi, np.pi, N_BIG).astype(np.float32)
    tab = CosineTables(T_FULL)
    order = list(reversed(range(0, T_FULL, STEP)))
    mt, st = MultistepTables(tab, order), StridedTables(tab, order, 0.0)
    assert order[0] == 980 and mt.coef[980, 4] == 0 and mt.coef[0, 4] == 0 and (mt.coef[[960, 500, 20], 4] > 0).all()
    return {"x": x, "e": e, "prev": prev, "dx": torch.from_numpy(x).to(DEV), "de": torch.from_numpy(e).to(DEV),
            "dprev": torch.from_numpy(prev).to(DEV), "rows": mt.coef.numpy(), "coef": mt.coef.to(DEV),
            "strided": st.coef.to(DEV)}


def _cut_distance(v):
    """Distance of v to the nearest cut of wrap_pi (an odd multiple of pi)."""
    return np.abs(v - (np.pi + 2 * np.pi * np.round((v - np.pi) / (2 * np.pi))))


def _check(row, got, hist, x, e, prev, wrap, wrap_x0, what):
    """Assert the bounds of the module docstring on every (non-excluded) element of the output and of the stored history;
    returns the worst error / bound of the two."""
    ref, ref_hist, p = R.update(row, x, e, prev, wrap=wrap, wrap_x0=wrap_x0)
    a_s, c_1 = float(row[2]), float(row[4])
    e_x0 = 3 * U * p["x0_mag"] + (4 * U * (np.abs(p["x0_raw"]) + np.pi) if wrap_x0 else 0.0)
    x0_abs = np.abs(p["x0"]) if wrap_x0 else p["x0_mag"]
    b = a_s * e_x0 + U * (a_s * x0_abs + 2 * p["dir_mag"])
    keep = np.ones(ref.shape, dtype=bool)
    if wrap_x0:
        keep &= _cut_distance(p["x0_raw"]) >= 8 * U * p["x0_mag"]
    if c_1 != 0.0:
        pre = e_x0 + U * (x0_abs + p["prev_mag"])
        e_d = pre + (4 * U * (np.abs(p["d_raw"]) + np.pi) if wrap else 0.0)
        b = b + abs(c_1) * e_d + U * (np.abs(c_1 * p["d"]) + a_s * x0_abs + p["dir_mag"])
        if wrap:
            keep &= _cut_distance(p["d_raw"]) >= 2 * pre
    b = 1.25 * b + (4 * U * (np.abs(ref) + np.pi) if wrap else 0.0)
    b_hist = 1.25 * e_x0
    assert 1.0 - keep.mean() < 0.01, (what, "excluded share", 1.0 - keep.mean())
    got, hist = got.astype(np.float64), hist.astype(np.float64)
    err = R.circ(got, ref) if wrap else np.abs(got - ref)
    err_hist = R.circ(hist, ref_hist) if wrap_x0 else np.abs(hist - ref_hist)
    if wrap:
        assert np.abs(got).max() <= np.pi + 1e-6
    if wrap_x0:
        assert np.abs(hist).max() <= np.pi + 1e-6
    if not keep.any():
        return 0.0
    r_out, r_hist = (err[keep] / b[keep]).max(), (err_hist[keep] / b_hist[keep]).max()
    assert (err[keep] <= b[keep]).all(), (what, "out: worst |got - ref| / bound", r_out)
    assert (err_hist[keep] <= b_hist[keep]).all(), (what, "hist: worst |got - ref| / bound", r_hist)
    return max(r_out, r_hist)


@pytest.mark.parametrize("wrap_x0", [False, True])
@pytest.mark.parametrize("wrap", [False, True])
def test_kernel_against_the_float64_ref(pkg, hip, data, wrap, wrap_x0):
    ops = pkg.ops
    worst = 0.0
    for t in TIMESTEPS:
        for n in SIZES:
            hist = data["dprev"][:n].clone()
            got = ops.multistep_step_wrap(data["dx"][:n], data["de"][:n], hist, data["coef"], _t(t), wrap=wrap,
                                          wrap_x0=wrap_x0).cpu().numpy()
            if np.isnan(data["rows"][t]).any():                            # a row that is not visited: NaN everywhere
                assert t == 999 and np.isnan(got).all() and torch.isnan(hist).all()
                continue
            r = _check(data["rows"][t], got, hist.cpu().numpy(), data["x"][:n], data["e"][:n], data["prev"][:n], wrap, wrap_x0,
                       (t, n, wrap, wrap_x0))
            worst = max(worst, r)
    print(f"multistep kernel wrap={wrap} wrap_x0={wrap_x0}: worst |got - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("wrap_x0", [False, True])
@pytest.mark.parametrize("wrap", [False, True])
def test_rows_without_the_term_give_the_strided_bits_and_read_no_history(pkg, hip, data, wrap, wrap_x0):
    ops = pkg.ops
    for t in (980, 0):                                                     # the first and the last visited timestep
        assert data["rows"][t][4] == 0.0
        for n in SIZES:
            x, e = data["dx"][:n], data["de"][:n]
            want = ops.strided_step_wrap(x, e, None, data["strided"], _t(t), wrap=wrap, wrap_x0=wrap_x0)
            hist = torch.full((n,), float("nan"), device=DEV)
            got = ops.multistep_step_wrap(x, e, hist, data["coef"], _t(t), wrap=wrap, wrap_x0=wrap_x0)
            assert torch.isfinite(got).all() and torch.equal(got, want), (t, n)
            assert torch.isfinite(hist).all()                              # the estimate is stored all the same
            if t == 0 and not wrap:                                        # a_s = 1, c_dir = 0: the step returns the estimate
                assert torch.equal(hist, got)


def _raw(pkg, x, e, hist_in, coef, t, wrap, wrap_x0, out, hist_out):
    """The C entry point itself: ``ops.multistep_step_wrap`` always updates the history in place."""
    rc = pkg.hip.lib().e3d_multistep_step_wrap(x.data_ptr(), e.data_ptr(), hist_in.data_ptr(), coef.data_ptr(), t.data_ptr(),
                                               coef.shape[0], int(wrap), int(wrap_x0), out.data_ptr(), hist_out.data_ptr(),
                                               x.numel(), pkg.ops._stream())
    pkg.hip.check(rc, "e3d_multistep_step_wrap")
    return out, hist_out


def test_out_may_alias_x_and_the_history_is_updated_in_place(pkg, hip, data):
    ops = pkg.ops
    for n in (5, 8 * 37, N_BIG):
        for t, wrap, wrap_x0 in ((500, True, False), (960, True, True), (20, False, False), (0, True, False)):
            x, e, prev = data["dx"][:n], data["de"][:n], data["dprev"][:n]
            want, want_hist = _raw(pkg, x, e, prev, data["coef"], _t(t), wrap, wrap_x0, torch.empty_like(x), torch.empty_like(x))
            assert torch.equal(prev, data["dprev"][:n]) and torch.equal(x, data["dx"][:n])
            xa, hist = x.clone(), prev.clone()
            got = ops.multistep_step_wrap(xa, e, hist, data["coef"], _t(t), wrap=wrap, wrap_x0=wrap_x0, out=xa)
            assert got is xa and torch.equal(got, want) and torch.equal(hist, want_hist), (n, t)
            assert not torch.equal(want_hist, prev)
    with pytest.raises(RuntimeError, match="two buffers"):     # refused before any launch
        x = data["dx"][:8].clone()
        _raw(pkg, x, data["de"][:8], data["dprev"][:8].clone(), data["coef"], _t(500), True, False, x, x)


@pytest.mark.parametrize("bad", [-1, T_FULL])
def test_step_index_outside_the_table_gives_nan(pkg, hip, data, bad):
    ops = pkg.ops
    n = 4 * 300 + 3
    x, e = data["dx"][:n], data["de"][:n]
    hist = data["dprev"][:n].clone()
    want = ops.multistep_step_wrap(x, e, hist, data["coef"], _t(500))
    want_hist = hist.clone()
    out, hist = torch.zeros(n, device=DEV), data["dprev"][:n].clone()
    ops.multistep_step_wrap(x, e, hist, data["coef"], _t(bad), out=out)
    assert torch.isnan(out).all() and torch.isnan(hist).all()
    hist = data["dprev"][:n].clone()
    assert torch.equal(ops.multistep_step_wrap(x, e, hist, data["coef"], _t(500), out=out), want) and torch.equal(hist, want_hist)


def test_solver_error_through_the_kernel(pkg, hip):
    """Gaussian data N(0.3, 0.25), 20 visited steps, 4096 starts, no wrap: eps is the exact conditional mean, computed
    with torch on the device.  The chain of kernel launches agrees with the float64 chain to 1e-4 and ends at most half as
    far from the exact end point as the same chain driven through the strided kernel (float64: 0.00106 against 0.142)."""
    from e3diff_amd.structure_model.utils import CosineTables, MultistepTables, StridedTables
    ops = pkg.ops
    m, v = 0.3, 0.25
    tab = CosineTables(T_FULL)
    order = list(reversed(range(0, T_FULL, 50)))
    assert len(order) == 20
    betas = tab.betas.double().numpy()
    ab = R.alphas_cumprod(betas)
    x_T = np.random.default_rng(0).standard_normal(4096)
    exact = R.gaussian_exact_end(x_T, ab[order[0]], m, v)
    ref_end = R.gaussian_chain(betas, order, x_T, m, v, "multistep")
    ref_err = float(np.abs(ref_end - exact).max())
    ref_ddim = R.gaussian_max_error(betas, order, x_T, m, v, "ddim")
    assert abs(ref_err - 0.00106) < 1e-5 and abs(ref_ddim - 0.142) < 1e-3
    coef = {"multistep": MultistepTables(tab, order).coef.to(DEV), "strided": StridedTables(tab, order, 0.0).coef.to(DEV)}
    ab_dev = torch.from_numpy(ab).to(DEV)

    def eps_of(x, t):                      # float64 on the device, rounded once
        a = ab_dev[t]
        return (torch.sqrt(1.0 - a) * (x.double() - torch.sqrt(a) * m) / (a * v + 1.0 - a)).float()

    ends = {}
    for rule in ("multistep", "strided"):
        x = torch.from_numpy(x_T).float().to(DEV)
        hist = torch.full_like(x, float("nan"))
        for t in order:
            if rule == "multistep":
                x = ops.multistep_step_wrap(x, eps_of(x, t), hist, coef[rule], _t(t), wrap=False)
            else:
                x = ops.strided_step_wrap(x, eps_of(x, t), None, coef[rule], _t(t), wrap=False)
        ends[rule] = x.cpu().numpy().astype(np.float64)
    # the float64 chains start from the fp32 rounding of x_T too: compare like with like
    x_T32 = x_T.astype(np.float32).astype(np.float64)
    agree = float(np.abs(ends["multistep"] - R.gaussian_chain(betas, order, x_T32, m, v, "multistep")).max())
    exact32 = R.gaussian_exact_end(x_T32, ab[order[0]], m, v)
    err = {k: float(np.abs(e - exact32).max()) for k, e in ends.items()}
    print(f"kernel chains, 20 steps, v={v}: |multistep - float64 chain| = {agree:.2e}; max error multistep {err['multistep']:.3g}, "
          f"strided {err['strided']:.3g} (x{err['strided'] / err['multistep']:.0f})")
    assert agree <= 1e-4
    assert err["multistep"] <= 0.5 * err["strided"]


# ------------------------------------------------------------------------------------------------ chains
T_CHAIN, STEP_CHAIN = 12, 3
IDS = [11, (1 << 35) + 2, 7, 123456]


@pytest.fixture(scope="module")
def setup(pkg, hip):
    model, pk, tab = _structure_setup(B=4, L=128, T=T_CHAIN)
    g = torch.Generator().manual_seed(5)
    from e3diff_amd.structure_model.utils import modulo_with_wrapped_range
    x_T = modulo_with_wrapped_range(torch.randn(4, 128, 8, generator=g)).to(DEV)
    valid = pk["ligand_attn_mask"].bool()
    assert int(valid.sum(dim=1).min()) >= 5
    held = torch.zeros(4, 128, dtype=torch.bool, device=DEV)
    held[:, 1:4] = True                                             # an anchor: residues 1-3 (every ligand has >= 5)
    return {"model": model, "pk": pk, "tab": tab, "x_T": x_T, "valid": valid, "known": pk["ligand_angles"].clone(),
            "held": held}


def _order(step):
    return list(reversed(range(0, T_CHAIN, step)))


def _args(s, sel=None, x_T=None):
    pk = s["pk"] if sel is None else {k: v[sel].contiguous() for k, v in s["pk"].items()}
    x_T = s["x_T"] if x_T is None else x_T
    x_T = x_T if sel is None else x_T[sel].contiguous()
    return (s["model"], pk["ligand_attn_mask"], x_T, pk["receptor_seq"], pk["receptor_attn_mask"], pk["receptor_angles"],
            T_CHAIN, s["tab"])


def _graphed_chain(S, s, step, wrap_x0=False):
    """The padded chain with every step replayed from one captured GraphedReverseStep (p_sample_loop itself never
    replays chains of four steps).  The graph owns the history."""
    from e3diff_amd.structure_model.utils import MultistepTables
    model, pk, order = s["model"], s["pk"], _order(step)
    cache = model.encode_receptor(pk["receptor_seq"], pk["receptor_angles"], pk["receptor_attn_mask"])
    mod_rows = model.timestep_modulation(torch.tensor(order, device=DEV, dtype=torch.long))
    mod_table = torch.zeros((T_CHAIN, mod_rows.shape[1]), device=DEV)
    mod_table[order] = mod_rows
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        g = S.GraphedReverseStep(model, pk["ligand_attn_mask"].contiguous().float(), cache, s["tab"], s["x_T"],
                                 mod_table=mod_table, multistep=MultistepTables(s["tab"], order), wrap_x0=wrap_x0)
    assert g.noise is None and g.known_noise is None and g.history.shape == s["x_T"].shape
    chains = []
    for _ in range(2):                     # the second chain finds the first one's last estimate in the history: not read
        out, x = [], s["x_T"]
        for i in order:
            x = g.step(i, x)
            out.append(x.clone())
        chains.append(torch.stack(out))
    assert torch.equal(chains[0], chains[1])
    return chains[0]


@pytest.mark.parametrize("wrap_x0", [False, True])
def test_eager_chain_equals_the_loop_by_hand_and_the_graphed_chain(pkg, hip, setup, wrap_x0):
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.utils import MultistepTables
    s = setup
    model, pk, tab, order = s["model"], s["pk"], s["tab"], _order(STEP_CHAIN)
    kw = dict(return_device=True, update="multistep", wrap_x0=wrap_x0)
    torch.manual_seed(1)
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    eager = S.p_sample_loop(*_args(s), step=STEP_CHAIN, use_graph=False, **kw)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(DEV), dev_state)
    assert eager.shape == (4, 4, 128, 8) and torch.isfinite(eager).all() and eager.abs().max() <= 3.1416
    mt = MultistepTables(tab, order)
    assert (mt.weights[1:-1] > 0).all()
    with torch.no_grad():
        cache = model.encode_receptor(pk["receptor_seq"], pk["receptor_angles"], pk["receptor_attn_mask"])
        mod_rows = model.timestep_modulation(torch.tensor(order, device=DEV, dtype=torch.long))
        mask = pk["ligand_attn_mask"].contiguous().float()
        coef = mt.coef.to(DEV)
        x, hist, want, hists = s["x_T"], torch.full_like(s["x_T"], float("nan")), [], []
        for n, i in enumerate(order):
            t = torch.full((4,), i, device=DEV, dtype=torch.long)
            eps = model.decode(t, x, mask, cache, mod=mod_rows[n:n + 1])
            x = pkg.ops.multistep_step_wrap(x, eps.contiguous(), hist, coef, t, wrap=True, wrap_x0=wrap_x0)
            want.append(x)
            hists.append(hist.clone())
        # the single-step form at the second visited timestep, the history handed in by the caller and updated in place
        t = torch.full((4,), order[1], device=DEV, dtype=torch.long)
        eps = model.decode(t, want[0], mask, cache)
        h_hand, h_single = hists[0].clone(), hists[0].clone()
        by_hand = pkg.ops.multistep_step_wrap(want[0], eps.contiguous(), h_hand, coef, t, wrap=True, wrap_x0=wrap_x0)
        single = S.p_sample(model, mask, want[0], None, None, None, t, tab, receptor_cache=cache, wrap=True, multistep=mt,
                            wrap_x0=wrap_x0, history=h_single)
        dev_state = torch.cuda.get_rng_state(DEV)
        graph = _graphed_chain(S, s, STEP_CHAIN, wrap_x0)
    assert torch.equal(eager, torch.stack(want))
    assert torch.equal(single, by_hand) and torch.equal(h_single, h_hand) and not torch.equal(h_single, hists[0])
    assert _wrapped_diff(single, want[1], s["valid"][..., None].expand_as(single)) < WRAPPED_TOL
    assert torch.equal(graph, eager) and torch.equal(torch.cuda.get_rng_state(DEV), dev_state)
    # the extrapolation is live, and the first entry is the strided chain's at eta = 0 from the same x_T
    strided = S.p_sample_loop(*_args(s), step=STEP_CHAIN, use_graph=False, return_device=True, update="strided", eta=0.0,
                              wrap_x0=wrap_x0)
    assert torch.equal(eager[0], strided[0]) and not torch.equal(eager[1], strided[1])
    # and through p_sample_loop's own capture (six steps: long enough to replay)
    e2 = S.p_sample_loop(*_args(s), step=2, use_graph=False, **kw)
    dev_state = torch.cuda.get_rng_state(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        g2 = S.p_sample_loop(*_args(s), step=2, use_graph=True, **kw)
    assert e2.shape[0] == 6 and torch.equal(e2, g2) and torch.equal(torch.cuda.get_rng_state(DEV), dev_state)


def test_a_chain_of_one_visited_timestep_is_the_x0_estimate(pkg, hip, setup):
    from e3diff_amd.structure_model import sample as S
    s = setup
    kw = dict(step=T_CHAIN, use_graph=False, return_device=True)
    one = S.p_sample_loop(*_args(s), update="multistep", **kw)
    assert one.shape[0] == 1 and torch.equal(one, S.p_sample_loop(*_args(s), update="strided", eta=0.0, **kw))


def test_frames_agree(pkg, hip, setup):
    from e3diff_amd.structure_model import sample as S
    s = setup
    kw = dict(step=STEP_CHAIN, return_device=True, update="multistep", use_graph=False)
    base = S.p_sample_loop(*_args(s), **kw)
    valid = s["valid"][None, :, :, None].expand_as(base)
    trim = S.p_sample_loop(*_args(s), trim_padding=True, **kw)
    packed = S.p_sample_loop(*_args(s), pack=True, **kw)
    diffs = [_wrapped_diff(trim, base, valid), _wrapped_diff(packed, base, valid), _wrapped_diff(packed, trim, valid)]
    print(f"multistep frames: trimmed / packed / packed - trimmed vs padded = {diffs[0]:.2e} / {diffs[1]:.2e} / {diffs[2]:.2e}")
    assert max(diffs) < WRAPPED_TOL
    assert (packed[:, ~s["valid"]] == 0).all()


def _seeded(S, s, seed, sel=None, step=STEP_CHAIN, **kw):
    sel = list(range(4)) if sel is None else sel
    ids = [IDS[i] for i in sel]
    args = list(_args(s, sel))
    args[2] = S.keyed_x_T(seed, ids, 128, 8, device=DEV)
    return S.p_sample_loop(*args, return_device=True, step=step, seed=seed, item_ids=ids, update="multistep",
                           known=s["known"][sel].contiguous(), known_mask=s["held"][sel].contiguous(), **kw)


def test_seeded_chain_with_held_positions_follows_the_item(pkg, hip, setup):
    """test_strided_gpu.py::test_seeded_strided_chain_follows_the_item's equalities, for a multistep chain whose only draws
    are those of the held positions (stream 10) and the keyed x_T."""
    from e3diff_amd.structure_model import sample as S
    s, seed = setup, 2024
    base = _seeded(S, s, seed)
    assert base.shape == (4, 4, 128, 8) and torch.isfinite(base).all()
    valid = s["valid"][None, :, :, None].expand_as(base)
    held = (s["held"] & s["valid"])[None, :, :, None].expand_as(base)
    assert torch.equal(base[-1][held[-1]], s["known"][held[-1]])             # the last entry holds ``known`` bit for bit
    assert not torch.equal(base[0][held[0]], s["known"][held[0]])
    torch.manual_seed(7)                                                      # torch's generator plays no part
    assert torch.equal(_seeded(S, s, seed), base)
    assert _wrapped_diff(_seeded(S, s, seed + 1), base, valid) > 0.1
    rev = _seeded(S, s, seed, sel=[3, 2, 1, 0])
    for b in range(4):
        assert torch.equal(rev[:, 3 - b], base[:, b])
    one = _seeded(S, s, seed, sel=[2])
    assert _wrapped_diff(one[:, 0], base[:, 2], valid[:, 2]) < WRAPPED_TOL
    assert torch.equal(one[:, 0][held[:, 2]], base[:, 2][held[:, 2]])
    trim = _seeded(S, s, seed, trim_padding=True)
    packed = _seeded(S, s, seed, pack=True)
    assert _wrapped_diff(trim, base, valid) < WRAPPED_TOL
    assert _wrapped_diff(packed, base, valid) < WRAPPED_TOL
    assert _wrapped_diff(packed, trim, valid) < WRAPPED_TOL
    for got in (trim, packed):
        assert torch.equal(got[held], base[held])
    # eager and graphed: the same kernels on the same frame (six steps: long enough to replay)
    for frame in ({}, dict(trim_padding=True), dict(pack=True)):
        eager = _seeded(S, s, seed, step=2, use_graph=False, **frame)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            graph = _seeded(S, s, seed, step=2, use_graph=True, **frame)
        assert eager.shape[0] == 6 and torch.equal(graph, eager), frame
        h6 = held[:1].expand_as(eager)
        assert torch.equal(eager[-1][h6[-1]], s["known"][h6[-1]])


def test_entry_point_passes_the_update_through(pkg, hip, tmp_path, monkeypatch):
    """sample() hands UPDATE = "multistep" (with STEP and WRAP_X0) to the chain."""
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
    monkeypatch.setattr(S, "STEP", 2)                  # visits 4, 2, 0: the middle step extrapolates
    monkeypatch.setattr(S, "ETA", 0.0)
    monkeypatch.setattr(S, "WRAP_X0", True)
    monkeypatch.setattr(S, "UPDATE", "strided")
    strided = S.sample(model, ds, seed=31)
    monkeypatch.setattr(S, "UPDATE", "multistep")
    runs = []
    for s in (1, 2):
        torch.manual_seed(s)                           # no draws and a keyed x_T: torch's generator plays no part
        runs.append(S.sample(model, ds, seed=31))
    assert len(runs[0]) == 3
    for a, b, c0 in zip(runs[0], runs[1], strided):
        assert a.shape == c0.shape and a.shape[0] == 3 and np.isfinite(a).all() and np.abs(a).max() <= 3.1416
        assert np.array_equal(a, b)
        assert np.array_equal(a[0], c0[0]) and not np.array_equal(a[1], c0[1])
    monkeypatch.setattr(S, "ETA", 0.5)
    with pytest.raises(ValueError, match="eta"):
        S.sample(model, ds, seed=31)
