"""structure_model/sample.py::StepPlan -- the one record of what a chain's reverse step is -- host-side, no GPU: the six
``ops`` launches it chooses between are replaced with recorders and the plan is driven on CPU tensors, through every cell
of {ancestral, strided eta 0, strided eta 1} x {noise buffer, keyed} x {held positions, none}, as the eager step drives
it (with the host's step index) and as the captured one does (without)."""
import itertools

import pytest
import torch

T, SEED, SCALE = 6, 77, 0.5
ORDER = [5, 3, 2, 0]                                   # the visited timesteps of the strided and the held chains
UPDATES = ("ddpm_step_wrap", "ddpm_step_wrap_table", "keyed_ddpm_step_wrap", "strided_step_wrap", "keyed_strided_step_wrap")
COMPOSES = ("known_compose_wrap", "keyed_known_compose_wrap")
RULES = {"ancestral": None, "strided0": 0.0, "strided1": 1.0}


@pytest.fixture
def calls(pkg, monkeypatch):
    """Recorders in place of the six launches: (name, positional arguments, keyword arguments) per call.  An update
    returns its ``out`` (or a new tensor), a compose its ``x``, like the launches."""
    made = []

    def recorder(name):
        def call(x, *a, **kw):
            made.append((name, (x,) + a, kw))
            if name in COMPOSES:
                return x
            return torch.empty_like(x) if kw.get("out") is None else kw["out"]
        return call

    for name in UPDATES + COMPOSES:
        monkeypatch.setattr(pkg.ops, name, recorder(name))
    return made


def _plan(pkg, rule, keyed, held):
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.utils import CosineTables, KnownLevels, StridedTables
    tab = CosineTables(T)
    kw = {}
    if RULES[rule] is not None:
        kw.update(strided=StridedTables(tab, ORDER, RULES[rule]), wrap_x0=rule == "strided1")
    if keyed:
        kw.update(row_keys=pkg.keyed.padded_keys([4, 9], 8, "cpu"), seed=SEED)
    if held:
        mask = torch.zeros(2, 8, 8, dtype=torch.uint8)
        mask[:, :3] = 1
        kw.update(known=torch.randn(2, 8, 8), known_mask=mask, known_levels=KnownLevels(tab, ORDER), known_scale=SCALE)
    return S.step_plan(tab, "cpu", table=True, **kw), kw


def _want_update_draws(plan, kw, t):
    """From the tables themselves: keyed never; a strided row by its sigma; the ancestral update everywhere but t = 0."""
    if "seed" in kw:
        return False
    if "strided" in kw:
        return float(kw["strided"].coef[t, 4]) != 0.0
    return t != 0


def _want_compose_draws(plan, kw, t):
    return "known" in kw and "seed" not in kw and float(kw["known_levels"].levels[t, 1]) != 0.0


@pytest.mark.parametrize("rule,keyed,held", list(itertools.product(RULES, (False, True), (False, True))))
def test_every_cell_launches_its_one_update_and_compose(pkg, calls, rule, keyed, held):
    plan, kw = _plan(pkg, rule, keyed, held)
    tab, strided = plan.tab, kw.get("strided")
    assert list(plan.order) == (ORDER if strided is not None or held else [5, 4, 3, 2, 1, 0])
    assert plan.coef.shape == (T, 4 if strided is None else 8) and plan.coef.dtype == torch.float32
    if strided is not None:
        assert torch.equal(plan.coef.isnan(), strided.coef.isnan()) and torch.equal(plan.coef[ORDER], strided.coef[ORDER])
    else:
        want = torch.stack([tab.sqrt_recip_alphas, tab.betas, tab.sqrt_one_minus_alphas_cumprod, tab.sigma], dim=1)
        assert torch.equal(plan.coef, want)
    # the predicates against the tables, for every step of the order
    for t in plan.order:
        assert plan.update_draws(t) is _want_update_draws(plan, kw, t)
        assert plan.compose_draws(t) is _want_compose_draws(plan, kw, t)
    draws = [plan.update_draws(t) for t in plan.order]
    if keyed or rule == "strided0":
        assert not any(draws)
    else:                                              # every step but the chain's last
        assert draws == [True] * (len(draws) - 1) + [False]
    assert [plan.compose_draws(t) for t in ORDER] == ([True, True, True, False] if held and not keyed else [False] * 4)

    x, eps = torch.randn(2, 8, 8), torch.randn(2, 8, 8)
    injected, buf, out = torch.randn(2, 8, 8), torch.randn(2, 8, 8), torch.empty(2, 8, 8)
    entry = ("keyed_" if keyed else "") + ("ddpm_step_wrap" if strided is None else "strided_step_wrap")
    for n, (t, eager, inject) in enumerate(itertools.product(plan.order, (True, False), (True, False))):
        t_dev, wrap = torch.full((2,), t, dtype=torch.long), bool(n % 2)
        del calls[:]
        # ---- update: with the host's index (eager; injected noise or a draw of its own) or without (a graph's buffer)
        noise_in = (injected if inject else None) if eager else (buf if inject else None)
        got = plan.update(x, eps, t_dev, noise_in, out, wrap, t if eager else None)
        assert len(calls) == 1 and got is out
        name, a, k = calls[0]
        assert a[0] is x and torch.equal(a[1], eps) and k["wrap"] is wrap and k["out"] is out
        if strided is not None:
            assert k["wrap_x0"] is (rule == "strided1")
        else:
            assert "wrap_x0" not in k
        if keyed:                                      # never a noise tensor: the table, the index, the keys, the seed
            assert name == entry and len(a) == 6
            assert a[2] is plan.coef and a[3] is t_dev and a[4] is kw["row_keys"] and a[5] == SEED
        elif strided is None and eager:                # the scalar launch, with the four host coefficients of row t
            assert name == "ddpm_step_wrap" and len(a) == 7
            sigma = 0.0 if t == 0 else float(tab.sigma[t])
            assert a[3:] == (float(tab.sqrt_recip_alphas[t]), float(tab.betas[t]),
                             float(tab.sqrt_one_minus_alphas_cumprod[t]), sigma)
            assert (a[2] is None) == (t == 0)
        else:
            assert name == (entry + "_table" if strided is None else entry) and len(a) == 5
            assert a[3] is plan.coef and a[4] is t_dev
        if not keyed:
            noise = a[2]
            if not eager:                              # the captured step hands its buffer (or None) through
                assert noise is noise_in
            elif not _want_update_draws(plan, kw, t):  # t = 0; a strided row with sigma == 0
                assert noise is None
            elif inject:
                assert noise is injected
            else:                                      # a fresh draw
                assert noise is not None and noise.shape == x.shape and noise is not injected and noise is not buf
        # ---- compose
        del calls[:]
        back = plan.compose(got, t_dev, noise_in, t if eager else None)
        assert back is got
        if not held:
            assert calls == []
            continue
        assert len(calls) == 1
        name, a, k = calls[0]
        assert a[0] is got and a[1] is plan.known_x0 and a[2] is plan.known_mask and not k
        assert torch.equal(plan.known_x0, kw["known"]) and torch.equal(plan.known_mask, kw["known_mask"])
        assert torch.equal(plan.levels.isnan(), kw["known_levels"].levels.isnan())
        assert torch.equal(plan.levels[ORDER], kw["known_levels"].levels[ORDER])
        if keyed:
            assert name == "keyed_known_compose_wrap"
            assert a[3] is plan.levels and a[4] is t_dev and a[5] is kw["row_keys"] and a[6:] == (SEED, SCALE)
            continue
        assert name == "known_compose_wrap" and a[4] is plan.levels and a[5] is t_dev and a[6:] == (SCALE,)
        noise = a[3]
        if not eager:
            assert noise is noise_in
        elif t == ORDER[-1]:                           # the clean level: a copy, no draw
            assert noise is None
        elif inject:
            assert noise is injected
        else:
            assert noise is not None and noise.shape == x.shape and noise is not injected


def test_the_constructor_checks_once(pkg):
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.utils import CosineTables, KnownLevels, StridedTables
    tab = CosineTables(T)
    keys = pkg.keyed.padded_keys([4, 9], 8, "cpu")
    x, m = torch.zeros(2, 8, 8), torch.ones(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="strided"):
        S.step_plan(tab, "cpu", wrap_x0=True)
    with pytest.raises(ValueError, match="seed"):
        S.step_plan(tab, "cpu", row_keys=keys)
    with pytest.raises(ValueError, match="row_keys"):
        S.step_plan(tab, "cpu", seed=SEED)
    with pytest.raises(ValueError, match="known_levels"):
        S.step_plan(tab, "cpu", known=x, known_mask=m)
    with pytest.raises(ValueError, match="known_levels"):
        S.step_plan(tab, "cpu", known=x, known_mask=m, known_levels=KnownLevels(tab, ORDER).levels)
    with pytest.raises(TypeError, match="StridedTables"):
        S.step_plan(tab, "cpu", strided=StridedTables(tab, ORDER).coef)
    with pytest.raises(ValueError, match="seed"):
        S.step_plan(tab, "cpu", row_keys=keys, seed=1 << 64)
    with pytest.raises(ValueError, match="steps"):     # keyed.check_steps: the streams hold 2^16 steps
        S.step_plan(torch.full((65537,), 0.01), "cpu", row_keys=keys, seed=SEED)
    # the plain plan -- what the benchmark's step runs -- builds and uploads no table; a plan is a frozen record
    plain = S.step_plan(tab)
    assert plain.coef is None and plain.keyed is None and plain.strided is None and plain.known_x0 is None
    assert S.step_plan(tab, "cpu", table=True).coef.shape == (T, 4)
    assert S.step_plan(tab, "cpu", row_keys=keys, seed=SEED).coef.shape == (T, 4)
    with pytest.raises(AttributeError):
        plain.wrap_x0 = True


class _Model:
    """decode() returns zeros; counts what the step asks of the model."""

    def __init__(self):
        self.decoded = []

    def encode_receptor(self, *a):
        raise AssertionError("the step was given a receptor cache")

    def decode(self, timestep, x, mask, cache, mod=None, layout=None):
        self.decoded.append(timestep)
        return torch.zeros_like(x)


@pytest.mark.parametrize("t", [0, 3])
def test_the_plain_eager_step_is_one_scalar_launch(pkg, calls, monkeypatch, t):
    """_reverse_step(..., plan=None) with an int timestep, as the benchmark calls it: the scalar ddpm_step_wrap once, with
    the four host coefficients of row t, and no synchronising look at the timestep."""
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.utils import CosineTables

    def no_sync(*a, **k):
        raise AssertionError("an int timestep needs no torch.unique")

    monkeypatch.setattr(torch, "unique", no_sync)
    tab, model = CosineTables(T), _Model()
    x, out = torch.randn(2, 8, 8), torch.empty(2, 8, 8)
    got = S._reverse_step(model, torch.ones(2, 8), x, None, None, None, t, tab, None, "cache", out, True)
    assert got is out and len(model.decoded) == 1 and model.decoded[0].tolist() == [t, t]
    assert [c[0] for c in calls] == ["ddpm_step_wrap"]
    _, a, k = calls[0]
    assert torch.equal(a[0], x) and torch.equal(a[1], torch.zeros_like(x)) and k == {"wrap": True, "out": out}
    assert a[3:] == (float(tab.sqrt_recip_alphas[t]), float(tab.betas[t]), float(tab.sqrt_one_minus_alphas_cumprod[t]),
                     float(tab.sigma[t]) if t else 0.0)
    assert (a[2] is None) == (t == 0) and (t == 0 or a[2].shape == x.shape)
