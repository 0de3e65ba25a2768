"""CPU: the host logic of training.py -- the order of the one training step and the batch loop of ``fit`` against a loop
written out here (torch modules and optimizers only: no kernel runs)."""
import pytest
import torch


class _Toy(torch.nn.Module):
    """Two linear layers in use, one never used (its gradient stays None), the LightningModule surface ``fit`` asks for."""

    def __init__(self, interval):
        super().__init__()
        self.a, self.b, self.unused = torch.nn.Linear(6, 8), torch.nn.Linear(8, 3), torch.nn.Linear(3, 3)
        self.interval, self.calls = interval, []

    def _loss(self, batch):
        return ((self.b(torch.tanh(self.a(batch["x"]))) - batch["y"]) ** 2).mean()

    def training_step(self, batch, batch_idx):
        self.calls.append(("train", batch_idx, self.training))
        return self._loss(batch)

    def validation_step(self, batch, batch_idx):
        self.calls.append(("val", batch_idx, self.training))
        return {"val_loss": self._loss(batch)}

    def configure_optimizers(self):
        optim = torch.optim.AdamW(self.parameters(), lr=3e-2, weight_decay=0.1)
        sched = torch.optim.lr_scheduler.StepLR(optim, step_size=2, gamma=0.5)
        return {"optimizer": optim, "lr_scheduler": {"scheduler": sched, "interval": self.interval}}


class _Items(torch.utils.data.Dataset):
    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        self.x, self.y = torch.randn(n, 6, generator=g), 5.0 * torch.randn(n, 3, generator=g)   # (gradients the clip bites on)

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return {"x": self.x[i], "y": self.y[i]}


def _toy(interval):
    torch.manual_seed(0)
    return _Toy(interval)


@pytest.mark.parametrize("max_steps", [None, 5])
@pytest.mark.parametrize("interval", ["step", "epoch"])
def test_fit_loop_is_the_written_out_loop(pkg, interval, max_steps):
    """``training.fit`` on CPU (plain stepper, torch AdamW, StepLR per step / per epoch, with and without ``max_steps``)
    against the loop written out below: losses, step count, parameters and the sequence of model calls, all exactly."""
    from e3diff_amd import training
    train = torch.utils.data.DataLoader(_Items(10, 1), batch_size=4)
    val = torch.utils.data.DataLoader(_Items(12, 2), batch_size=2)

    model = _toy(interval)
    history = training.fit(model, train, val, max_epochs=3, max_steps=max_steps, device="cpu", checkpoint_path=None,
                           log=lambda *a: None)

    ref = _toy(interval)
    conf = ref.configure_optimizers()
    optim, sched = conf["optimizer"], conf["lr_scheduler"]["scheduler"]
    params = list(ref.parameters())
    train_loss, val_loss, steps = [], [], 0
    for _ in range(3):
        ref.train()
        losses = []
        for batch_idx, batch in enumerate(train):
            loss = ref.training_step(batch, batch_idx)
            optim.zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            optim.step()
            if interval == "step":
                sched.step()
            losses.append(float(loss.detach()))
            steps += 1
            if max_steps is not None and steps >= max_steps:
                break
        if interval == "epoch":
            sched.step()
        train_loss.append(sum(losses) / len(losses))
        ref.eval()
        with torch.no_grad():
            vals = [float(ref.validation_step(batch, batch_idx)["val_loss"]) for batch_idx, batch in enumerate(val)]
        val_loss.append(sum(vals) / len(vals))
        if max_steps is not None and steps >= max_steps:
            break

    assert history["train_loss"] == train_loss
    assert history["val_loss"] == val_loss
    assert history["steps"] == steps == (9 if max_steps is None else 5)
    for (name, p), q in zip(model.named_parameters(), ref.parameters()):
        assert torch.equal(p, q), name
    assert model.unused.weight.grad is None
    assert model.calls == ref.calls and len(ref.calls) == (27 if max_steps is None else 17)


class _Recorder:
    """Averager and optimizer stub in one: notes what ``train_step`` calls, in order."""
    defaults = {}

    def __init__(self, log, active):
        self.log, self.active = log, active

    def _active(self):
        return self.active

    def prepare(self):
        self.log.append("prepare")

    def average(self):
        self.log.append("average")

    def mark_ready(self, p):
        self.log.append("mark_ready")

    def zero_grad(self, set_to_none=False):
        assert set_to_none
        self.log.append("zero_grad")

    def step(self):
        self.log.append("step")


@pytest.mark.parametrize("defer", [True, False])
@pytest.mark.parametrize("averager", ["active", "inactive", None])
def test_train_step_order_and_weight_gradient_queue(pkg, monkeypatch, averager, defer):
    """The one training step: training_step, zero_grad, prepare, backward, average, clip + step -- backward inside a
    ``deferred_weight_grads`` block that reports to an ACTIVE averager's ``mark_ready`` and to nobody otherwise; with
    DEFER_WEIGHT_GRADS off no block is opened."""
    from e3diff_amd import training
    from e3diff_amd.autograd import deferred_weight_grads
    monkeypatch.setattr(training, "DEFER_WEIGHT_GRADS", defer)
    log, queues = [], []
    w = torch.nn.Parameter(torch.ones(3))

    class Model:
        def training_step(self, batch, batch_idx):
            log.append("training_step")
            assert batch == {"k": 1} and batch_idx == 7
            y = w * 2.0

            def in_backward(grad):
                log.append("backward")
                queues.append(deferred_weight_grads.active)
            y.register_hook(in_backward)
            return y.sum()

    avg = None if averager is None else _Recorder(log, averager == "active")
    loss = training.train_step(Model(), _Recorder(log, False), [w], 1.0, {"k": 1}, 7, averager=avg)
    assert float(loss.detach()) == 6.0 and deferred_weight_grads.active is None
    around = [] if avg is None else ["prepare", "average"]
    assert log == ["training_step", "zero_grad"] + around[:1] + ["backward"] + around[1:] + ["step"]
    (queue,) = queues
    if not defer:
        assert queue is None
    elif averager == "active":
        assert queue.on_param == avg.mark_ready
    else:
        assert queue is not None and queue.on_param is None
    assert torch.allclose(w.grad.norm(), torch.tensor(1.0), atol=1e-5)      # clipped to the norm handed in
