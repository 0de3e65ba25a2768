"""CPU: the weight EMA of training.py -- its law, the plain-torch route against the fp64 statement (tests/ema_ref.py),
``swapped``, ``fit(ema_decay=)`` and the exported entry points of the fused route (no kernel runs here)."""
import math
import os

import pytest
import torch

from ema_ref import Statement, decay_fp32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("decay", [0.0, 0.9, 0.9999])
@pytest.mark.parametrize("n", [1, 2, 9, 10 ** 4])
def test_ema_decay_at_is_the_fp32_of_the_double_expression(pkg, n, decay, warmup):
    from e3diff_amd.training import ema_decay_at
    want = min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay
    want = float(torch.tensor(want, dtype=torch.float64).to(torch.float32))
    got = ema_decay_at(n, decay, warmup)
    assert isinstance(got, float) and got == want == decay_fp32(n, decay, warmup)
    assert got == float(torch.tensor(got, dtype=torch.float32))            # an fp32 value
    assert ema_decay_at(n, decay) == ema_decay_at(n, decay, True)          # warm-up is the default


@pytest.mark.parametrize("decay", [-0.1, 1.0, math.nan])
def test_ema_decay_outside_the_unit_interval_is_refused(pkg, decay):
    from e3diff_amd.training import WeightEMA, ema_decay_at
    for warmup in (True, False):
        with pytest.raises(ValueError):
            ema_decay_at(1, decay, warmup)
        with pytest.raises(ValueError):
            WeightEMA(torch.nn.Linear(2, 2), decay, warmup)


class _Net(torch.nn.Module):
    """Two layers in use, one parameter that never gets a gradient, one buffer."""

    def __init__(self):
        super().__init__()
        self.a, self.b = torch.nn.Linear(7, 9), torch.nn.Linear(9, 3)
        self.idle = torch.nn.Parameter(torch.randn(4, 5))
        self.register_buffer("table", torch.arange(6, dtype=torch.float32))

    def forward(self, x):
        return self.b(torch.tanh(self.a(x)))


def _steps(model, optim, ema, n, first=0):
    """n AdamW steps with ema.update() after each; yields the step index after each."""
    for k in range(first, first + n):
        g = torch.Generator().manual_seed(40 + k)
        x, y = torch.randn(16, 7, generator=g), 3.0 * torch.randn(16, 3, generator=g)
        optim.zero_grad(set_to_none=True)
        ((model(x) - y) ** 2).mean().backward()
        optim.step()
        ema.update()
        yield k


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("decay", [0.0, 0.9, 0.9999])
def test_weight_ema_under_torch_adamw_stays_within_the_bound(pkg, decay, warmup):
    """6 steps of torch.optim.AdamW on a small CPU module, ``WeightEMA.update()`` after each: every shadow within
    n * 4u * M of the fp64 statement after every update; the idle parameter's shadow equal to it; buffers not averaged and
    untouched; the state_dict carries shadows, count and law and loads in place (its round trip continuing to the same
    bits: the next test)."""
    from e3diff_amd.training import WeightEMA
    torch.manual_seed(3)
    model = _Net()
    table0 = model.table.clone()
    optim = torch.optim.AdamW(model.parameters(), lr=3e-2, weight_decay=0.1)
    ema = WeightEMA(model, decay, warmup)
    assert set(ema.shadows) == {n for n, _ in model.named_parameters()} and "table" not in ema.shadows
    for name, p in model.named_parameters():
        e = ema.shadows[name]
        assert e.dtype == torch.float32 and e.is_contiguous() and torch.equal(e, p) and e.data_ptr() != p.data_ptr()
    ref = {name: Statement(p) for name, p in model.named_parameters()}
    worst = 0.0
    for k in _steps(model, optim, ema, 6):
        d = decay_fp32(k + 1, decay, warmup)
        for name, p in model.named_parameters():
            ref[name].update(p, d)
            frac = ref[name].fraction(ema.shadows[name])
            worst = max(worst, frac)
            assert frac <= 1.0, (name, k, frac)
        assert ema.num_updates == k + 1
    print(f"decay {decay} warmup {warmup}: worst fraction of the bound {worst:.3f}")
    assert torch.equal(ema.shadows["idle"], model.idle) and model.idle.grad is None
    assert torch.equal(model.table, table0)
    if decay == 0.0 and not warmup:       # w = 1: the shadow IS the parameter
        assert all(torch.equal(ema.shadows[n], p) for n, p in model.named_parameters())
    elif decay > 0:
        assert not torch.equal(ema.shadows["a.weight"], model.a.weight)

    sd = ema.state_dict()
    assert set(sd) == {"shadows", "num_updates", "decay", "warmup"} and sd["num_updates"] == 6
    assert sd["decay"] == decay and sd["warmup"] is warmup and set(sd["shadows"]) == set(ema.shadows)
    twin = WeightEMA(model, 0.5, not warmup)
    ptrs = {n: e.data_ptr() for n, e in twin.shadows.items()}
    twin.load_state_dict(sd)
    assert (twin.num_updates, twin.decay, twin.warmup) == (6, decay, warmup)
    assert {n: e.data_ptr() for n, e in twin.shadows.items()} == ptrs      # loaded in place
    assert all(torch.equal(twin.shadows[n], e) for n, e in ema.shadows.items())


def test_state_dict_round_trip_continues_to_the_same_bits(pkg):
    """Two identical runs; the second one's EMA is replaced after 3 steps by a fresh instance loaded from its state_dict."""
    from e3diff_amd.training import WeightEMA
    finals = []
    for reload in (False, True):
        torch.manual_seed(5)
        model = _Net()
        optim = torch.optim.AdamW(model.parameters(), lr=3e-2, weight_decay=0.1)
        ema = WeightEMA(model, 0.9)
        list(_steps(model, optim, ema, 3))
        if reload:
            sd = ema.state_dict()
            ema = WeightEMA(model, 0.1, warmup=False)      # shadows cloned from the CURRENT weights, another law
            ema.load_state_dict(sd)
        list(_steps(model, optim, ema, 3, first=3))
        finals.append((ema.num_updates, {n: e.clone() for n, e in ema.shadows.items()}))
    (na, ea), (nb, eb) = finals
    assert na == nb == 6 and all(torch.equal(ea[n], eb[n]) for n in ea)


def test_swapped_holds_the_ema_weights_in_place_and_restores_them(pkg):
    from e3diff_amd import ops
    from e3diff_amd.training import WeightEMA
    torch.manual_seed(7)
    model = _Net()
    optim = torch.optim.AdamW(model.parameters(), lr=3e-2)
    ema = WeightEMA(model, 0.9, warmup=False)
    list(_steps(model, optim, ema, 3))
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    ptrs = {n: p.data_ptr() for n, p in model.named_parameters()}
    table = model.table.clone()
    assert not torch.equal(before["a.weight"], ema.shadows["a.weight"])

    def inside():
        for n, p in model.named_parameters():
            assert torch.equal(p, ema.shadows[n]) and p.data_ptr() == ptrs[n] and p.requires_grad, n
        assert torch.equal(model.table, table)

    def restored():
        for n, p in model.named_parameters():
            assert torch.equal(p, before[n]) and p.data_ptr() == ptrs[n], n

    gen = ops.PARAM_GENERATION
    with ema.swapped(model) as m:
        assert m is model and ops.PARAM_GENERATION > gen
        gen = ops.PARAM_GENERATION
        inside()
    assert ops.PARAM_GENERATION > gen
    restored()
    with pytest.raises(RuntimeError, match="boom"):
        with ema.swapped(model):
            inside()
            raise RuntimeError("boom")
    restored()


# ---- fit: the toy of tests/test_training_cpu.py, with a validation value that is a function of one weight
class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a, self.b, self.unused = torch.nn.Linear(6, 8), torch.nn.Linear(8, 3), torch.nn.Linear(3, 3)
        self.register_buffer("scale", torch.tensor(2.0))
        self.seen = []                       # a.weight as every validation step saw it

    def training_step(self, batch, batch_idx):
        return ((self.b(torch.tanh(self.a(batch["x"]))) - batch["y"]) ** 2).mean()

    def validation_step(self, batch, batch_idx):
        self.seen.append(self.a.weight.detach().clone())
        return {"val_loss": self.a.weight.double().sum() * 1.0}

    def configure_optimizers(self):
        optim = torch.optim.AdamW(self.parameters(), lr=3e-2, weight_decay=0.1)
        sched = torch.optim.lr_scheduler.StepLR(optim, step_size=2, gamma=0.5)
        return {"optimizer": optim, "lr_scheduler": {"scheduler": sched, "interval": "step"}}


class _Items(torch.utils.data.Dataset):
    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        self.x, self.y = torch.randn(n, 6, generator=g), 5.0 * torch.randn(n, 3, generator=g)

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return {"x": self.x[i], "y": self.y[i]}


def _fit(training, path, **kw):
    torch.manual_seed(0)
    model = _Toy()
    train = torch.utils.data.DataLoader(_Items(10, 1), batch_size=4)
    val = torch.utils.data.DataLoader(_Items(4, 2), batch_size=2)
    history = training.fit(model, train, val, max_epochs=2, device="cpu", checkpoint_path=path, checkpoint_mode="min",
                           log=lambda *a: None, **kw)
    return model, history


def test_fit_with_ema_validates_and_checkpoints_the_ema_weights(pkg, tmp_path):
    """fit(device="cpu", ema_decay=): torch AdamW, so the plain-torch route.  The EMA of the run is reproduced here from a
    twin run's parameters; validation saw it, the checkpoint holds it under the model's own keys, and a run without
    ``ema_decay`` is what it was."""
    from e3diff_amd import training
    plain_path, ema_path = str(tmp_path / "plain.pt"), str(tmp_path / "ema.pt")
    plain, hist_plain = _fit(training, plain_path)
    assert set(hist_plain) == {"train_loss", "val_loss", "steps", "seconds"}           # today's history
    saved = torch.load(plain_path)
    # (mode "min" and a falling val value or not: the file is the model's state_dict at its best epoch -- one of the two seen)
    assert set(saved) == set(plain.state_dict())
    assert any(torch.equal(saved["a.weight"], w) for w in plain.seen)

    model, hist = _fit(training, ema_path, ema_decay=0.9, ema_warmup=False)
    assert hist["steps"] == 6 and hist["ema_updates"] == 6
    ema = hist["ema"]
    assert isinstance(ema, training.WeightEMA) and ema.num_updates == 6 and (ema.decay, ema.warmup) == (0.9, False)
    # the training trajectory itself is unchanged by the average
    assert hist["train_loss"] == hist_plain["train_loss"]
    for (n, p), q in zip(model.named_parameters(), plain.parameters()):
        assert torch.equal(p, q), n
    # validation saw the EMA weights: not the raw ones (which the plain run's validation saw), and at the end the shadow
    assert len(model.seen) == len(plain.seen) == 4
    for w_ema, w_raw in zip(model.seen, plain.seen):
        assert not torch.equal(w_ema, w_raw)
    assert torch.equal(model.seen[-1], ema.shadows["a.weight"])
    assert hist["val_loss"][-1] == float(ema.shadows["a.weight"].double().sum())
    assert hist["val_loss"] != hist_plain["val_loss"]
    # ... and the model got its own weights back
    assert not torch.equal(model.a.weight, ema.shadows["a.weight"])
    # the checkpoint: model_state_dict of the best epoch, the model's exact key set, buffers as they are
    ck = torch.load(ema_path)
    assert list(ck) == list(model.state_dict())
    assert torch.equal(ck["scale"], model.scale)
    assert any(torch.equal(ck["a.weight"], w) for w in model.seen)
    assert torch.equal(ck["unused.weight"], model.unused.weight)         # never moved: shadow == parameter
    msd = ema.model_state_dict(model)
    assert list(msd) == list(model.state_dict()) and torch.equal(msd["b.bias"], ema.shadows["b.bias"])
    twin = _Toy()
    twin.load_state_dict(msd)                                              # the drop-in point: loads unchanged
    assert torch.equal(twin.a.weight, ema.shadows["a.weight"])


def test_fit_ema_follows_the_statement(pkg):
    """The shadows ``fit`` returns are within the bound of the fp64 statement over the parameters a twin run (written out
    here) has after each of its steps, with the warm-up schedule."""
    from e3diff_amd import training
    model, hist = _fit(training, None, ema_decay=0.999)
    torch.manual_seed(0)
    ref = _Toy()
    conf = ref.configure_optimizers()
    optim, sched = conf["optimizer"], conf["lr_scheduler"]["scheduler"]
    st = {n: Statement(p) for n, p in ref.named_parameters()}
    n_up = 0
    for _ in range(2):
        for batch in torch.utils.data.DataLoader(_Items(10, 1), batch_size=4):
            loss = ref.training_step(batch, 0)
            optim.zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(list(ref.parameters()), 1.0)
            optim.step()
            sched.step()
            n_up += 1
            for n, p in ref.named_parameters():
                st[n].update(p, decay_fp32(n_up, 0.999, True))
    assert hist["ema_updates"] == n_up == 6
    for n, p in ref.named_parameters():
        assert torch.equal(p, dict(model.named_parameters())[n])
        assert st[n].fraction(hist["ema"].shadows[n]) <= 1.0, n


def test_the_fused_route_is_declared_and_exported(pkg):
    import ctypes
    header = open(os.path.join(ROOT, "include", "e3d_hip.h")).read()
    assert "#define E3D_ABI_VERSION 5" in header and pkg.hip.ABI_VERSION == 5
    lib = ctypes.CDLL(pkg.hip.LIB_PATH)
    for name in ("e3d_adamw_ema_step", "e3d_adamw_ema_step_dev"):
        assert "int " + name + "(" in header and name in pkg.hip.EXPORTS, name
        assert callable(getattr(lib, name))
    assert lib.e3d_abi_version() == 5
    for name in ("e3d_adamw_step", "e3d_adamw_step_dyn", "e3d_adamw_step_dev"):      # nothing that existed changed
        assert name in pkg.hip.EXPORTS
    # the two forms take the plain ones' arguments plus the shadow table (and, host form, the decay)
    sig = pkg.hip._SIGNATURES
    assert len(sig["e3d_adamw_ema_step"][1]) == len(sig["e3d_adamw_step"][1]) + 2
    assert len(sig["e3d_adamw_ema_step_dev"][1]) == len(sig["e3d_adamw_step_dev"][1]) + 1


def test_clip_adamw_without_an_ema_keeps_its_state_dict(pkg):
    """(CPU parameters: the fallback step.)  attach_ema on a CPU ClipAdamW routes through ``update()``; its state_dict has
    torch.optim.AdamW's keys with and without one."""
    from e3diff_amd.optim import ClipAdamW
    from e3diff_amd.training import WeightEMA, clip_and_step
    torch.manual_seed(1)
    model = _Net()
    plain = torch.optim.AdamW(model.parameters(), lr=1e-2)
    optim = ClipAdamW(model.parameters(), lr=1e-2)
    keys = set(optim.state_dict()) | {"state", "param_groups"}
    ema = WeightEMA(model, 0.5, warmup=False)
    optim.attach_ema(ema)
    x = torch.randn(4, 7)
    model(x).sum().backward()
    w0 = model.a.weight.detach().clone()
    clip_and_step(list(model.parameters()), optim, 1.0, ema=ema)
    assert ema.num_updates == 1                                            # once: by the step's fallback, not again by clip_and_step
    want = w0 + (model.a.weight.detach() - w0) * 0.5
    assert torch.equal(ema.shadows["a.weight"], want)
    assert set(optim.state_dict()) == keys == set(plain.state_dict())
    assert set(optim.state_dict()["param_groups"][0]) == set(plain.state_dict()["param_groups"][0])
    assert optim.detach_ema() is ema and optim.ema is None
    with pytest.raises(TypeError):
        optim.attach_ema(object())


def test_entry_points_refuse_a_null_shadow_table_and_a_bad_decay(pkg):
    """Host-side argument checks, made before anything is launched: every call below carries one refused argument (the other
    pointers are the address of a host buffer that is never read)."""
    import ctypes
    lib = ctypes.CDLL(pkg.hip.LIB_PATH)
    for name in ("e3d_adamw_ema_step", "e3d_adamw_ema_step_dev", "e3d_last_error"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = pkg.hip._SIGNATURES[name]
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)

    def host(ema, decay):
        return lib.e3d_adamw_ema_step(a, a, a, a, ema, a, a, a, 1, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, decay, None)

    assert host(None, 0.5) == -1 and b"null ema" in lib.e3d_last_error()
    for decay in (1.0, 1.5, -0.1, math.nan):
        assert host(a, decay) == -1 and b"outside [0, 1)" in lib.e3d_last_error(), decay
    assert lib.e3d_adamw_ema_step_dev(a, a, a, a, None, a, a, a, 1, None, a, None) == -1
    assert b"null ema" in lib.e3d_last_error()
    assert lib.e3d_adamw_ema_step_dev(a, a, a, a, a, a, a, a, 1, None, None, None) == -1       # no hyper block
