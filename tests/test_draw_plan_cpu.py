"""sequence_model/sample.py::DrawPlan -- the one record of how a sequence chain draws z_s -- host-side, no GPU: the six
``ops`` launches it chooses between are replaced with recorders and a step is driven on CPU tensors through every cell of
{categorical, argmax} x {injected uniforms, the generator's, keyed} x {no held positions, held, held with injected
uniforms} x {no controls, a record with nothing set, active controls}, with the chain's plan and with the keywords a
single call builds one from."""
import itertools

import pytest
import torch

B, L, C, T, SEED = 2, 5, 20, 50, 77
POSTERIORS = ("discrete_posterior_sample", "keyed_discrete_posterior_sample", "discrete_posterior_sample_ctl",
              "keyed_discrete_posterior_sample_ctl")
COMPOSES = ("discrete_known_compose", "keyed_discrete_known_compose")


@pytest.fixture
def calls(pkg, monkeypatch):
    """Recorders in place of the six launches: (name, positional arguments) per call.  A posterior returns new class
    indices, a compose its ``idx``, like the launches."""
    made = []

    def recorder(name):
        def call(*a, **kw):
            assert not kw, (name, kw)
            made.append((name, a))
            return a[0] if name in COMPOSES else torch.full((B, L), 3, dtype=torch.int32)
        return call

    for name in POSTERIORS + COMPOSES:
        monkeypatch.setattr(pkg.ops, name, recorder(name))
    return made


def _inputs(pkg):
    from e3diff_amd.sequence_model.utils import DiscreteUniformTransition, PredefinedNoiseScheduleDiscrete
    g = torch.Generator().manual_seed(3)
    x = torch.nn.functional.one_hot(torch.randint(0, C, (B, L), generator=g), C).float()
    s = torch.full((B, 1), 24.0)
    return dict(x=x, logits=torch.randn(B, L, C, generator=g), t=(s + 1) / T, s=s / T,
                sched=PredefinedNoiseScheduleDiscrete("cosine", T), trans=DiscreteUniformTransition(C),
                u=torch.rand(B, L, generator=g), known_u=torch.rand(B, L, generator=g),
                keys=pkg.keyed.padded_keys([4, 9], L, "cpu"), s_dev=torch.full((1,), 24, dtype=torch.long),
                x0=torch.randint(0, C, (B, L), generator=g).int(), mask=torch.ones(B, L, dtype=torch.uint8))


def _controls(pkg, kind):
    from e3diff_amd.design import DesignControls
    if kind == "none":
        return None
    if kind == "inactive":
        return DesignControls.build((B, L, C))
    return DesignControls.build((B, L, C), temperature=0.7, omit="CM")


CELLS = list(itertools.product((True, False), ("inject", "generator", "keyed"), ("free", "held", "held_inject"),
                               ("none", "inactive", "active"), ("plan", "keywords")))


@pytest.mark.parametrize("diverse,source,held,ctl,how", CELLS)
def test_every_cell_launches_its_posterior_then_its_compose(pkg, calls, diverse, source, held, ctl, how):
    from e3diff_amd.sequence_model import sample as S
    d = _inputs(pkg)
    controls = _controls(pkg, ctl)
    keyed, has_held = source == "keyed", held != "free"
    u = d["u"] if source == "inject" else None
    known_u = d["known_u"] if held == "held_inject" and not keyed else None
    if how == "plan":
        kw = {}
        if keyed:
            kw.update(row_keys=d["keys"], seed=SEED)
        if has_held:
            kw.update(known_x0=d["x0"], known_mask=d["mask"])
        plan = S.draw_plan(diverse, controls=controls, **kw)
        assert plan.diverse is diverse and (plan.keyed == (d["keys"], SEED) if keyed else plan.keyed is None)
        assert (plan.known_x0 is d["x0"] and plan.known_mask is d["mask"]) if has_held else plan.known_x0 is None
        assert plan.controls is (controls if ctl == "active" else None)
        with pytest.raises(AttributeError):                       # a frozen record
            plan.diverse = not diverse
    torch.manual_seed(5)
    if how == "plan":                                              # as a chain's step does
        got = plan.step(d["t"], d["s"], d["x"], d["logits"], d["sched"], d["trans"], d["s_dev"] if keyed else None, u, known_u)
    else:                                                          # a single call: the plan of its keywords
        got = S.sample_p_zs_given_zt_discrete(
            d["t"], d["s"], d["x"], d["logits"], d["sched"], d["trans"], diverse, False, u=u, controls=controls,
            keyed_draw=(d["keys"], SEED, d["s_dev"]) if keyed else None,
            known=((d["x0"], d["mask"], known_u) if known_u is not None else (d["x0"], d["mask"])) if has_held else None)
    assert torch.equal(got, torch.nn.functional.one_hot(torch.full((B, L), 3), C).float())
    torch.manual_seed(5)                                           # the generator's draws, in the order a step makes them
    fresh = [torch.rand(B, L), torch.rand(B, L)]

    # ---- the posterior, first
    keyed_draw, active = keyed and diverse, ctl == "active"
    assert [c[0] for c in calls] == [("keyed_" if keyed_draw else "") + "discrete_posterior_sample" + ("_ctl" if active else "")] \
        + ([("keyed_" if keyed_draw else "") + "discrete_known_compose"] if has_held else [])
    a = list(calls[0][1])
    assert a[0].dtype == torch.int32 and torch.equal(a[0], d["x"].argmax(-1).int()) and torch.equal(a[1], d["logits"])
    if active:
        assert a[2] is controls.bias and a[3] == controls.inv_temp
        del a[2:4]
    qsb, qtb = a[2], a[3]
    assert torch.equal(qsb, d["trans"].get_Qt_bar(d["sched"].get_alpha_bar(t_normalized=d["s"]), "cpu"))
    assert torch.equal(qtb, d["trans"].get_Qt_bar(d["sched"].get_alpha_bar(t_normalized=d["t"]), "cpu"))
    if keyed_draw:
        assert len(a) == 7 and a[4] is d["keys"] and a[5] == SEED and a[6] is d["s_dev"]
    else:
        assert len(a) == 5
        if not diverse:
            assert a[4] is None
        elif u is not None:
            assert a[4] is u
        else:
            assert torch.equal(a[4], fresh.pop(0))
    # ---- then the compose, on the posterior's indices
    if not has_held:
        return
    a = calls[1][1]
    assert a[0].dtype == torch.int32 and bool((a[0] == 3).all()) and a[1] is d["x0"] and a[2] is d["mask"] and a[3] is qsb
    if keyed_draw:
        assert len(a) == 7 and a[4] is d["keys"] and a[5] == SEED and a[6] is d["s_dev"]
    else:
        assert len(a) == 5
        if not diverse:
            assert a[4] is None
        elif known_u is not None:
            assert a[4] is known_u
        else:
            assert torch.equal(a[4], fresh.pop(0))


def test_the_last_step_returns_the_logits_and_launches_nothing(pkg, calls):
    from e3diff_amd.sequence_model import sample as S
    d = _inputs(pkg)
    assert S.sample_p_zs_given_zt_discrete(None, None, d["x"], d["logits"], None, None, True, True,
                                           keyed_draw=(d["keys"], SEED, d["s_dev"]), known=(d["x0"], d["mask"]),
                                           controls=_controls(pkg, "active")) is d["logits"]
    assert calls == []


def test_the_plan_refuses_once(pkg, calls):
    from e3diff_amd.sequence_model import sample as S
    d = _inputs(pkg)
    with pytest.raises(ValueError, match="seed"):
        S.draw_plan(True, row_keys=d["keys"])
    with pytest.raises(ValueError, match="row_keys"):
        S.draw_plan(True, seed=SEED)
    with pytest.raises(ValueError, match="seed"):
        S.draw_plan(True, row_keys=d["keys"], seed=1 << 64)
    args = (d["t"], d["s"], d["x"], d["logits"], d["sched"], d["trans"])
    with pytest.raises(ValueError, match="not both"):             # uniforms together with a keyed source
        S.draw_plan(True, d["keys"], SEED).step(*args, d["s_dev"], d["u"])
    with pytest.raises(ValueError, match="not both"):
        S.sample_p_zs_given_zt_discrete(*args, True, False, u=d["u"], keyed_draw=(d["keys"], SEED, d["s_dev"]))
    assert calls == []
    # an argmax chain reads no uniforms, keyed or not: nothing to refuse
    S.draw_plan(False, d["keys"], SEED).step(*args, d["s_dev"], d["u"])
    assert [c[0] for c in calls] == ["discrete_posterior_sample"] and calls[0][1][4] is None


class _Model:
    def __init__(self, logits):
        self.logits, self.seen = logits, []

    def forward(self, s, x, *args):
        self.seen.append((s, x, args))
        return self.logits


def test_a_step_hands_the_plan_and_its_operands_through(pkg, calls):
    """_denoise_step, what the eager loop and the captured body both run: the model once, then the plan's launches with
    the step's device index and uniforms."""
    from e3diff_amd.sequence_model import sample as S
    d = _inputs(pkg)
    model = _Model(d["logits"])
    plan = S.draw_plan(True, d["keys"], SEED, d["x0"], d["mask"])
    s = torch.full((B, 1), 24.0)
    S._denoise_step(model, s, T, d["x"], (1, 2, 3, 4, 5), None, d["sched"], d["trans"], plan, False, d["s_dev"])
    assert len(model.seen) == 1 and model.seen[0][0] is s and model.seen[0][2] == (1, 2, 3, 4, 5)
    assert [c[0] for c in calls] == ["keyed_discrete_posterior_sample", "keyed_discrete_known_compose"]
    assert all(c[1][-1] is d["s_dev"] for c in calls)
    del calls[:]
    plan = S.draw_plan(True, known_x0=d["x0"], known_mask=d["mask"])
    S._denoise_step(model, s, T, d["x"], (1, 2, 3, 4, 5), None, d["sched"], d["trans"], plan, False, None, d["u"], d["known_u"])
    assert [c[0] for c in calls] == ["discrete_posterior_sample", "discrete_known_compose"]
    assert calls[0][1][4] is d["u"] and calls[1][1][4] is d["known_u"]
    assert S._denoise_step(model, s, T, d["x"], (1, 2, 3, 4, 5), None, d["sched"], d["trans"], plan, True) is d["logits"]
