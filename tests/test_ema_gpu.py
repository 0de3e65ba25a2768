"""GPU: the weight EMA inside the AdamW update launch (csrc/optim.hip: e3d_adamw_ema_step / _dev behind
``ClipAdamW.attach_ema``) against the fp64 statement of tests/ema_ref.py, within n * 4u * M; that nothing else of the step
moves; the plain-torch route beside it; the update inside a replayed HIP graph; ``swapped`` on a GPU model.

Worst observed fractions of the bound are printed by every test (``pytest -s``) and recorded in DESIGN.md."""
import pytest
import torch

from ema_ref import Statement, decay_fp32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(257, 33), (1000,), (3,), (8192 * 3 + 5,), (64, 768)]


def _zoo(seed=0):
    """The tensor zoo of the optimizer test: chunk edges, scalar tails, a view at data_ptr % 16 == 4, an idle parameter, a
    late one (first gradient at step 2: its own step-count range), two groups.  Returns (named parameters, groups, busy,
    late)."""
    g = torch.Generator().manual_seed(seed)
    flat = torch.randn(4 * 8192 + 7, generator=g).to(DEV)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g).to(DEV)) for s in SHAPES]
    odd = torch.nn.Parameter(flat[1:1 + 8192 + 2])
    assert odd.data_ptr() % 16 == 4 and odd.numel() == 8192 + 2
    idle = torch.nn.Parameter(torch.randn(5, 5, generator=g).to(DEV))
    late = torch.nn.Parameter(torch.randn(1000, generator=g).to(DEV))
    groups = [dict(params=ps[:3] + [odd, idle], lr=1e-2, weight_decay=0.1), dict(params=ps[3:] + [late], lr=3e-3, weight_decay=0.0)]
    named = [(f"p{i}", p) for i, p in enumerate(ps)] + [("odd", odd), ("idle", idle), ("late", late)]
    return named, groups, ps + [odd], late


def _set_grads(busy, late, step, scale):
    g = torch.Generator(device=DEV).manual_seed(100 + step)
    for p in busy + ([late] if step >= 2 else []):
        p.grad = torch.randn(p.shape, device=DEV, generator=g) * scale


def _run(pkg, decay, warmup, device_scalars, scale, route="fused", steps=5):
    """5 clipped steps over the zoo.  route: "fused" (EMA attached), "update" (plain step + WeightEMA.update()), None (no
    EMA).  Returns dict(named, optim, ema, norms, worst, statements)."""
    from e3diff_amd.optim import ClipAdamW
    from e3diff_amd.training import WeightEMA, clip_and_step
    named, groups, busy, late = _zoo()
    optim = ClipAdamW(groups)
    optim.use_device_scalars(device_scalars)
    ema = None
    if route is not None:
        ema = WeightEMA(named, decay, warmup)
        if route == "fused":
            optim.attach_ema(ema)
    st = {n: Statement(p) for n, p in named}
    params = [p for _, p in named]
    norms, worst = [], 0.0
    for step in range(steps):
        _set_grads(busy, late, step, scale)
        norms.append(clip_and_step(params, optim, 1.0, ema=ema).clone())
        optim.zero_grad(set_to_none=True)
        if ema is not None:
            assert ema.num_updates == step + 1
            d = decay_fp32(step + 1, decay, warmup)          # the GLOBAL n, for the late parameter too
            for n, p in named:
                st[n].update(p, d)
                frac = st[n].fraction(ema.shadows[n])
                worst = max(worst, frac)
                assert frac <= 1.0, (n, step, frac)
    return dict(named=named, optim=optim, ema=ema, norms=norms, worst=worst)


@pytest.mark.parametrize("device_scalars", [False, True])
@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("decay", [0.9, 0.9999])
def test_fused_ema_against_the_fp64_statement(pkg, hip, decay, warmup, device_scalars):
    """ClipAdamW with an EMA attached, 5 clipped steps at gradient scales 50 (clip active) and 1e-3 (inactive): every shadow
    within n * 4u * M of the statement after every step, host scalars (e3d_adamw_ema_step) and device scalars
    (e3d_adamw_ema_step_dev: d_n formed on the device from the count it advances itself); the idle parameter's shadow
    equal to it; the late parameter on the schedule's d_n of the global n."""
    for scale in (50.0, 1e-3):
        r = _run(pkg, decay, warmup, device_scalars, scale)
        named, ema = dict(r["named"]), r["ema"]
        print(f"decay {decay} warmup {warmup} device_scalars {device_scalars} scale {scale}: worst fraction {r['worst']:.3f}")
        assert torch.equal(ema.shadows["idle"], named["idle"])
        assert not torch.equal(ema.shadows["late"], named["late"]) and not torch.equal(ema.shadows["odd"], named["odd"])
        assert ema.num_updates == 5
        if device_scalars:     # the device words: decay (sign bit: no warm-up) and the count, for every range
            dyn = r["optim"]._e3d_tab["dyn"].cpu()
            assert dyn.shape[0] == 3 and dyn[:, 7].tolist() == [5.0] * 3
            assert dyn[:, 6].abs().tolist() == [decay_fp32(1, decay, False)] * 3
            assert torch.signbit(dyn[:, 6]).tolist() == [not warmup] * 3


@pytest.mark.parametrize("device_scalars", [False, True])
def test_attaching_an_ema_moves_nothing_else(pkg, hip, device_scalars):
    """The same gradients through a ClipAdamW with and without an EMA: parameters, both moments and the returned norms are
    bit-equal; the EMA-less state_dict has torch.optim.AdamW's keys only."""
    for scale in (50.0, 1e-3):
        a = _run(pkg, 0.9999, True, device_scalars, scale, route="fused")
        b = _run(pkg, 0.9999, True, device_scalars, scale, route=None)
        for x, y in zip(a["norms"], b["norms"]):
            assert torch.equal(x, y)
        for (n, p), (_, q) in zip(a["named"], b["named"]):
            assert torch.equal(p, q), n
            sa, sb = a["optim"].state.get(p, {}), b["optim"].state.get(q, {})
            assert set(sa) == set(sb)
            for k in ("exp_avg", "exp_avg_sq"):
                if k in sa:
                    assert torch.equal(sa[k], sb[k]), (n, k)
            if "step" in sa:
                assert float(sa["step"]) == float(sb["step"])
        tab = b["optim"]._e3d_tab
        assert "eptr" not in tab and "ema_n" not in tab
        if device_scalars:
            assert tab["dyn"][:, 6:].abs().sum().item() == 0.0
        for r in (a, b):
            sd = r["optim"].state_dict()
            assert set(sd) == {"state", "param_groups"}
            assert all(set(v) == {"step", "exp_avg", "exp_avg_sq"} for v in sd["state"].values())
            ref = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0]
            assert all(set(g) == set(ref) for g in sd["param_groups"])


def test_fused_and_plain_torch_routes_both_follow_the_statement(pkg, hip):
    """The fused route and ``WeightEMA.update()`` after a plain ClipAdamW step, on the same gradients: both within the
    bound (checked inside ``_run``), over bit-equal parameters.  Bit-equal shadows are not required: the compiler may
    contract the fused form."""
    for warmup in (True, False):
        a = _run(pkg, 0.9, warmup, False, 50.0, route="fused")
        b = _run(pkg, 0.9, warmup, False, 50.0, route="update")
        assert b["optim"].ema is None and b["ema"].num_updates == 5
        for (n, p), (_, q) in zip(a["named"], b["named"]):
            assert torch.equal(p, q), n
        apart = max(float((a["ema"].shadows[n] - b["ema"].shadows[n]).abs().max()) for n, _ in a["named"])
        print(f"warmup {warmup}: fused worst {a['worst']:.3f}, update() worst {b['worst']:.3f}, largest |fused - update| {apart:.3e}")
        assert torch.equal(b["ema"].shadows["idle"], dict(b["named"])["idle"])


def test_attach_ema_checks_every_shadow_before_its_pointer_goes_in(pkg, hip):
    """A wrong shadow is refused in Python (a bad pointer table would be a GPU fault): wrong dtype, numel, device (CPU),
    layout, or no shadow at all for a parameter the optimizer steps."""
    from e3diff_amd.optim import ClipAdamW
    from e3diff_amd.training import WeightEMA
    for how in ("dtype", "numel", "cpu", "strided", "missing"):
        p = torch.nn.Parameter(torch.randn(6, 4, device=DEV))
        q = torch.nn.Parameter(torch.randn(5, device=DEV))
        optim = ClipAdamW([p, q], lr=1e-2)
        ema = WeightEMA([("p", p), ("q", q)] if how != "missing" else [("p", p)], 0.9)
        if how == "dtype":
            ema.shadows["p"] = ema.shadows["p"].double()
        elif how == "numel":
            ema.shadows["p"] = torch.zeros(23, device=DEV)
        elif how == "cpu":
            ema.shadows["p"] = ema.shadows["p"].cpu()
        elif how == "strided":
            ema.shadows["p"] = torch.zeros(6, 8, device=DEV)[:, ::2]
        optim.attach_ema(ema)
        p.grad, q.grad = torch.ones_like(p), torch.ones_like(q)
        p0 = p.detach().clone()
        with pytest.raises(ValueError, match="attach_ema"):
            optim.step()
        assert torch.equal(p, p0) and ema.num_updates == 0, how          # refused before anything was launched


# ---- the update inside a replayed graph: the small structure model of the graph-replay test, rebuilt here
def _small_structure_model(seed=0):
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.structure_model.model import ConditionalBertForDiffusion as M
    c = dict(hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=2, max_position_embeddings=64,
             hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    torch.manual_seed(seed)
    m = M(BertConfig(**c), BertConfig(**c, is_decoder=True, add_cross_attention=True), feature_names=list("abcdefgh"),
          loss_func=[M.diheral_loss_func] * 4 + [M.angle_loss_func] * 4, l2_lambda=0.1, learning_rate=1e-3)
    with torch.no_grad():       # adaLN_modulation[0] is zero-initialised: give the gated branches weights
        for se in (m.receptor_emb, m.timestep_emb):
            torch.nn.init.normal_(se.adaLN_modulation[0].weight, std=0.02)
    return m.train().to(DEV)


def _structure_batches(n, B=8, L=64, ragged=4):
    from helpers import synthetic_pockets
    from e3diff_amd.structure_model.dataset import noise_batch_on_device
    from e3diff_amd.structure_model.utils import CosineTables
    tab = CosineTables(100)
    out = []
    for i in range(n):
        b = B if i != ragged else B - 3                              # one ragged batch: runs eagerly between replays
        pk = {k: v.to(DEV) for k, v in synthetic_pockets(b, L, seed=10 + i).items() if torch.is_tensor(v)}
        g = torch.Generator().manual_seed(500 + i)
        t = torch.randint(0, 100, (b, 1), generator=g).to(DEV)
        noise = torch.randn(b, L, 8, generator=g).to(DEV)
        out.append(dict(pk, **noise_batch_on_device(pk["ligand_angles"], tab, timestep=t, noise=noise)))
    return out


@pytest.mark.parametrize("warmup", [True, False])
def test_ema_inside_the_graph_replayed_step(pkg, hip, warmup):
    """10 steps under training.GraphedStep with an EMA attached (eager warm-up steps, capture, replays; learning rate and
    beta1 change every step; a ragged batch runs eagerly in the middle; the optimizer state is re-loaded at step 5, so the
    step is captured a second time): the parameters are cloned after every step, and at the end every shadow is within the
    bound of the statement over those clones -- the device-side count advanced inside the captured step, once per replay."""
    from e3diff_amd import ops, training
    batches = _structure_batches(10)
    model = _small_structure_model()
    optim = model.configure_optimizers()["optimizer"]
    params = [p for p in model.parameters() if p.requires_grad]
    ema = training.WeightEMA(model, 0.9999, warmup)
    optim.attach_ema(ema)
    stepper = training.GraphedStep(model, optim, params, 1.0, ema=ema)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    st = {n: Statement(p) for n, p in named}
    replays = 0
    with ops.arithmetic("bf16x3"):
        for k, batch in enumerate(batches):
            optim.param_groups[0]["lr"] = 1e-3 * (1 + 0.25 * k)
            optim.param_groups[0]["betas"] = (0.95 - 0.01 * k, 0.999)
            stepper.step(batch)
            replays += stepper.graph is not None and k != 4
            assert ema.num_updates == k + 1
            d = decay_fp32(k + 1, 0.9999, warmup)
            for n, p in named:
                st[n].update(p, d)                                   # (clones the parameter to the host: the snapshot)
            if k == 5:
                optim.load_state_dict(optim.state_dict())
    assert ema.num_updates == 10 and stepper.graph is not None and stepper.failed is None
    assert replays >= 4
    assert {int(s["step"]) for s in optim.state.values()} == {10}
    assert optim._e3d_tab["dyn"][:, 7].tolist() == [10.0] * optim._e3d_tab["dyn"].shape[0]
    worst, moved = 0.0, 0
    for n, p in named:
        frac = st[n].fraction(ema.shadows[n])
        worst = max(worst, frac)
        assert frac <= 1.0, (n, frac)
        moved += not torch.equal(ema.shadows[n], p)
    print(f"graph replay, warmup {warmup}: worst fraction of the bound {worst:.3f} over {len(named)} tensors")
    assert moved > len(named) // 2


def test_swapped_on_a_gpu_model_reaches_the_weight_caches(pkg, hip):
    """A forward under ``swapped`` equals the forward of a twin loaded from ``model_state_dict``; a forward after the block
    equals the one before it (derived-weight caches are invalidated on entry and exit)."""
    from e3diff_amd import ops, training
    batches = _structure_batches(3, ragged=-1)
    model = _small_structure_model()
    optim = model.configure_optimizers()["optimizer"]
    params = [p for p in model.parameters() if p.requires_grad]
    ema = training.WeightEMA(model, 0.5, warmup=False)
    stepper = training.make_stepper(model, optim, params, 1.0, graph=False, ema=ema)
    assert optim.ema is ema
    with ops.arithmetic("bf16x3"):
        for b in batches[:2]:
            stepper.step(b)
        assert ema.num_updates == 2
        model.eval()
        probe = batches[2]

        def forward(m):
            with torch.no_grad():
                return m(probe["timestep"], probe["noised_ligand_angle"], probe["ligand_attn_mask"], probe["receptor_seq"],
                         probe["receptor_angles"], probe["receptor_attn_mask"]).clone()

        before = forward(model)
        ptrs = [p.data_ptr() for p in params]
        with ema.swapped(model):
            inside = forward(model)
            assert [p.data_ptr() for p in params] == ptrs
        after = forward(model)
        twin = _small_structure_model(seed=1).eval()
        twin.load_state_dict(ema.model_state_dict(model))
        want = forward(twin)
    assert torch.equal(after, before)
    assert torch.equal(inside, want)
    assert not torch.equal(inside, before)
