"""Plain training loop that stands in for ``pl.Trainer.fit`` as the reference configures it
(structure_model/train_model.py:99-116): gradient-norm clipping, AdamW from
``model.configure_optimizers()``, scheduler stepped per EPOCH (or per step for OneCycleLR),
validation every epoch, best-checkpoint bookkeeping with the reference's ``mode='max'`` quirk,
and -- new relative to the single-GPU reference -- data-parallel gradient averaging over RCCL when
launched with one process per GPU (``torchrun``).
"""
import contextlib
import math
import os
import time

import torch

from . import autograd, keyed, ops, sharding
from .packing import trimmed_length


def adamw(params, lr, weight_decay):
    """torch.optim.AdamW as the reference builds it (structure_model/model.py:361-366).  With every parameter on the GPU
    this is ``optim.ClipAdamW``: the same optimizer (state, state_dict, hooks, schedulers) whose step -- together with the
    gradient-norm clip around it, see ``clip_and_step`` -- runs as three HIP launches over all parameters (csrc/optim.hip)
    instead of torch's multi-tensor passes (norm 0.2 ms + clip multiply 0.27 ms + fused update 0.98 ms for the 146 M
    parameters of the structure model).  E3D_FUSED_ADAMW=torch: torch's own ``fused`` kernel; =0: torch's default."""
    params = list(params)
    choice = os.environ.get("E3D_FUSED_ADAMW", "1")
    on_gpu = bool(params) and all(p.is_cuda for p in params)
    if choice == "1" and on_gpu:
        from .optim import ClipAdamW
        return ClipAdamW(params, lr=lr, weight_decay=weight_decay)
    try:
        return torch.optim.AdamW(params, lr=lr, weight_decay=weight_decay, fused=True) if (choice == "torch" and on_gpu) else \
            torch.optim.AdamW(params, lr=lr, weight_decay=weight_decay)
    except (TypeError, RuntimeError):
        return torch.optim.AdamW(params, lr=lr, weight_decay=weight_decay)


def ema_decay_at(n, decay, warmup=True):
    """THE law of the weight EMA: the decay d_n of its n-th update, n = 1, 2, ...:  min(decay, (1 + n) / (10 + n)) with
    ``warmup`` (the average follows the weights closely while few of them have been seen), ``decay`` without -- computed
    in double and rounded ONCE to fp32 (returned as a Python float holding that fp32 value).  The update of an element,
    after the optimizer update of the same step:  w = 1.0f - d_n (fp32);  e <- e + (p_new - e) * w.
    ``decay`` lies in [0, 1) (as an fp32 value too: 1 - 1e-9 rounds to 1.0f and is refused); anything else raises ValueError.
    csrc/optim.hip (``ema_decay_dev``) forms the same value from the same double expression on the device."""
    decay = float(decay)
    if not (0.0 <= decay < 1.0) or float(torch.tensor(decay, dtype=torch.float32)) >= 1.0:
        raise ValueError(f"ema decay must lie in [0, 1), got {decay!r}")
    n = int(n)
    if n < 1:
        raise ValueError(f"ema updates are counted from 1, got n={n}")
    d = min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay
    return float(torch.tensor(d, dtype=torch.float64).to(torch.float32))


class WeightEMA:
    """Exponential moving average of a model's trainable parameters (``ema_decay_at`` is its law): one fp32 contiguous
    shadow per parameter, a fresh clone at construction, keyed by the parameter's ``state_dict`` name, plus the number of
    updates made.  Buffers are not averaged.  Two routes make an update, and a step takes exactly one of them:
    ``optim.ClipAdamW.attach_ema(self)`` -- the update launch averages every parameter it writes (csrc/optim.hip) -- and
    ``update()`` in plain torch for everything else.  Either way only parameters that took the optimizer step (those with a
    gradient) are averaged: one without has not moved, and its shadow started as a copy of it.

    ``model_state_dict(model)`` is the drop-in point for the samplers: the model's ``state_dict()`` with the EMA weights."""

    def __init__(self, model_or_named_params, decay, warmup=True):
        ema_decay_at(1, decay, warmup)                   # (raises on a decay outside [0, 1))
        self.decay, self.warmup, self.num_updates = float(decay), bool(warmup), 0
        named = model_or_named_params.named_parameters() if isinstance(model_or_named_params, torch.nn.Module) \
            else model_or_named_params
        self.shadows, self._params = {}, {}
        for name, p in named:
            if p.requires_grad:
                self.shadows[name] = p.detach().to(torch.float32, copy=True).contiguous()
                self._params[name] = p
        self._by_id = {id(p): name for name, p in self._params.items()}

    def decay_at(self, n):
        return ema_decay_at(n, self.decay, self.warmup)

    def shadow_of(self, param):
        """The shadow of one of the parameters this EMA was built over (None: not one of them)."""
        name = self._by_id.get(id(param))
        return None if name is None else self.shadows[name]

    @torch.no_grad()
    def update(self):
        """One update in plain torch, after the optimizer step (and before the next ``zero_grad``): the route of every
        optimizer that is not a ClipAdamW, of CPU parameters, and of a ClipAdamW step that fell back."""
        pairs = [(self.shadows[name], p) for name, p in self._params.items() if p.grad is not None]
        if not pairs:
            return
        d = self.decay_at(self.num_updates + 1)
        w = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(d, dtype=torch.float32))    # 1.0f - d_n
        shadows = [e for e, _ in pairs]
        diff = torch._foreach_sub([p.detach().to(torch.float32).reshape(e.shape) for e, p in pairs], shadows)
        torch._foreach_mul_(diff, w)
        torch._foreach_add_(shadows, diff)
        self.num_updates += 1

    def state_dict(self):
        return {"shadows": {k: v.clone() for k, v in self.shadows.items()}, "num_updates": self.num_updates,
                "decay": self.decay, "warmup": self.warmup}

    def load_state_dict(self, state):
        """In place: the shadows keep their storage (an attached optimizer's tables and captured graphs point into it)."""
        got = state["shadows"]
        if set(got) != set(self.shadows):
            raise KeyError(f"ema state_dict: shadow names differ: {sorted(set(got) ^ set(self.shadows))}")
        ema_decay_at(1, state["decay"], state["warmup"])
        with torch.no_grad():
            for k, e in self.shadows.items():
                if got[k].shape != e.shape:
                    raise ValueError(f"ema state_dict: {k}: shape {tuple(got[k].shape)}, expected {tuple(e.shape)}")
                e.copy_(got[k])
        self.num_updates, self.decay, self.warmup = int(state["num_updates"]), float(state["decay"]), bool(state["warmup"])

    def model_state_dict(self, model):
        """``model.state_dict()`` with every averaged entry replaced by (a copy of) its shadow, in the entry's dtype: the
        same keys, buffers as they are -- what ``load_state_dict`` and the samplers' ``MODEL_PATH`` take unchanged."""
        out = {}
        for k, v in model.state_dict(keep_vars=True).items():
            name = self._by_id.get(id(v)) if isinstance(v, torch.nn.Parameter) else None
            if name is None and k in self.shadows and isinstance(v, torch.nn.Parameter) and v.requires_grad:
                name = k                                  # (another instance of the model: by name)
            out[k] = v.detach() if name is None else self.shadows[name].to(v.dtype, copy=True).reshape(v.shape)
        return out

    @contextlib.contextmanager
    def swapped(self, model):
        """The model's parameters hold the EMA weights inside the block and are restored bit for bit on exit.  Copies in
        place and never rebinds ``.data``: packed parameter views (bert.py), optimizer tables and captured graphs keep
        their pointers.  Derived-weight caches are invalidated on entry and on exit."""
        pairs = [(p, self.shadows[name]) for name, p in model.named_parameters() if name in self.shadows and p.requires_grad]
        saved = [p.detach().clone() for p, _ in pairs]
        with torch.no_grad():
            for p, e in pairs:
                p.copy_(e.reshape(p.shape))
        ops.invalidate_weight_caches()
        try:
            yield model
        finally:
            with torch.no_grad():
                for (p, _), old in zip(pairs, saved):
                    p.copy_(old)
            ops.invalidate_weight_caches()


def clip_and_step(params, optim, max_norm, fold=None, ema=None):
    """``clip_grad_norm_(params, max_norm)`` + ``optim.step()`` -- what Lightning's ``gradient_clip_val`` does around the
    reference's AdamW (structure_model/train_model.py:99-110).  Returns the total gradient norm (device tensor).
    ``ema`` (a ``WeightEMA``): updated after the step -- by the step itself where it is a ClipAdamW with this EMA attached
    (inside the update launch, or through ``update()`` when that step falls back), by ``ema.update()`` here otherwise.
    ``fold`` (E3D_FOLD_CLIP=1): hand torch's fused AdamW 1 / clip_coef as its ``grad_scale`` (the GradScaler hook) so that
    the clip happens inside the update kernel instead of a separate multi-tensor pass.  Measured on MI355X (146 M
    parameters, rocprofv3): the multiply pass it removes costs 0.27 ms, but the fused kernel with a grad_scale also writes
    every unscaled gradient back and goes from 59 to 93 us per launch x 17 = +0.59 ms -- a net LOSS of 0.3 ms, so the
    two-call form stays the default; the folded form is kept for the comparison (tests/test_training_gpu.py pins that both
    give the same parameters)."""
    from .optim import ClipAdamW
    if isinstance(optim, ClipAdamW):                  # norm, clip and update in three launches (csrc/optim.hip)
        norm = optim.step_clipped(max_norm)
        if ema is not None and optim.ema is not ema:
            ema.update()
        return norm
    if ema is not None:
        norm = clip_and_step(params, optim, max_norm, fold)
        ema.update()
        return norm
    if fold is None:
        fold = os.environ.get("E3D_FOLD_CLIP", "0") == "1"
    grads = [p.grad for p in params if p.grad is not None]
    fused = bool(optim.defaults.get("fused")) and isinstance(optim, (torch.optim.AdamW, torch.optim.Adam))
    if not fold or not max_norm or not grads or not fused or not hasattr(torch.nn.utils, "get_total_norm"):
        norm = torch.nn.utils.clip_grad_norm_(params, max_norm) if max_norm else None
        optim.step()
        return norm
    norm = torch.nn.utils.get_total_norm(grads, 2.0, error_if_nonfinite=False, foreach=True)
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    optim.grad_scale = (1.0 / coef).to(torch.float32)
    try:
        optim.step()
    finally:
        optim.grad_scale = None
    return norm


# single-process training replays the step from a HIP graph (GraphedStep); 0: eager steps
GRAPH_TRAIN = os.environ.get("E3D_TRAIN_GRAPH", "1") == "1"
DEFER_WEIGHT_GRADS = os.environ.get("E3D_DEFER_WGRAD", "1") == "1"   # autograd.deferred_weight_grads in the step


def backward(loss, averager=None):
    """``loss.backward()`` as the training step runs it: the weight gradients of all linear layers are computed together
    when the block ends (grouped launches, written into .grad, i.e. into the all-reduce buckets of an active ``averager``,
    which learns of them through ``mark_ready``); E3D_DEFER_WGRAD=0: layer by layer inside backward."""
    if not DEFER_WEIGHT_GRADS:
        loss.backward()
        return
    active = averager is not None and averager._active()
    with autograd.deferred_weight_grads(on_param=averager.mark_ready if active else None):
        loss.backward()


def train_step(model, optim, params, clip, batch, batch_idx=0, averager=None, ema=None):
    """THE training step, eagerly, on the current stream (CPU parameters and any optimizer included); returns the loss.
    ``ema``: the run's ``WeightEMA``, updated with the step (``clip_and_step``)."""
    loss = model.training_step(batch, batch_idx)
    optim.zero_grad(set_to_none=True)
    if averager is not None:
        averager.prepare()                       # grads as views of the all-reduce buckets (no-op for one process)
    backward(loss, averager)
    if averager is not None:
        averager.average()                       # RCCL all-reduce (no-op for one process)
    if ema is None:
        clip_and_step(params, optim, clip)       # global-norm clip of the averaged grads, then AdamW
    else:
        clip_and_step(params, optim, clip, ema=ema)   # ... and the weight EMA of the step
    return loss


class EagerStep:
    """The stepper of a run that replays nothing (CPU parameters, another optimizer than ClipAdamW, E3D_TRAIN_GRAPH=0):
    every step is ``train_step`` on the caller's stream.  The graph steppers below extend it and share its ``step``."""

    graph = None                                     # nothing captured

    def __init__(self, model, optim, params, gradient_clip, averager=None, ema=None):
        self.model, self.optim, self.params, self.clip, self.averager = model, optim, params, gradient_clip, averager
        self.ema = ema                                   # the run's WeightEMA (None: none), updated with every step

    def _replayed(self, batch):
        """The loss of the step if a captured graph ran it, None if it has yet to run (eagerly)."""
        return None

    def _eager(self, batch, batch_idx):
        loss = train_step(self.model, self.optim, self.params, self.clip, batch, batch_idx, self.averager, self.ema)
        ops.invalidate_weight_caches()               # belt and braces beside the global optimizer hook (ops.py)
        return loss.detach()

    def step(self, batch, batch_idx=0):
        """Returns the loss (a device tensor; for a replayed step it is overwritten by the next replay of its graph)."""
        loss = self._replayed(batch)
        return self._eager(batch, batch_idx) if loss is None else loss


class GraphedStep(EagerStep):
    """One training step -- ``training_step`` + backward with deferred weight gradients + gradient-norm clip + AdamW -- as
    a HIP graph: captured once per batch signature (tensor names, shapes, dtypes) after ``warmup`` eager steps, then
    replayed.  The eager step of the structure model needs ~25 ms of Python and launch calls for ~1 350 kernels that keep
    the GPU busy for ~27 ms: replaying removes the host from the step.

    What makes the step replayable: no device-to-host synchronisation inside it (the losses are masked means, not index
    lists); the learning rate and the AdamW step counts live in device memory (``ClipAdamW.use_device_scalars``); dropout
    decisions take a device-side epoch word on top of their baked seeds (``ops.dropout_epoch``), advanced inside the graph
    -- or, keyed (a seeded ``fit``), are regenerated from the static batch's item ids and the epoch word at every replay;
    derived-weight caches (W^T, distance-table planes) are refreshed by launches inside the captured backward / forward.
    One graph per batch signature, up to ``MAX_GRAPHS`` of them (frames trimmed to the batch's longest ligand / pocket come
    in a handful of shapes: ``trim_batch``); a signature seen fewer than ``warmup`` times, or beyond that number, runs
    eagerly (a ragged last batch).  Every graph has its own memory pool, its own gradient tensors and its own staging
    buffer for their addresses (``ClipAdamW.new_capture_staging``); parameters, moments, learning rate and step counts are
    shared.  Single process; the data-parallel step is ``GraphedDDPStep`` (two segments around the collectives)."""

    MAX_GRAPHS = 8
    REPLAY_ON_SIDE_STREAM = False                    # replays run on the caller's current stream, eager steps on self.stream
    CAPTURE_FAILED = "training step could not be captured in a HIP graph"

    def __init__(self, model, optim, params, gradient_clip, warmup=2, ema=None):
        from .optim import ClipAdamW
        if not isinstance(optim, ClipAdamW):
            raise TypeError("GraphedStep needs optim.ClipAdamW (device-side learning rate and step counts)")
        if ema is not None and optim.ema is not ema:
            # the EMA of a replayed step lives in the captured update launch: its decay and count are device words
            raise ValueError("GraphedStep: attach the EMA to the optimizer first (ClipAdamW.attach_ema)")
        super().__init__(model, optim, params, gradient_clip, ema=ema)
        self.warmup, self.seen = warmup, {}
        self.graphs = {}                             # signature -> the captured step (graph segments, static batch, loss, grads)
        self.segments = self.key = self.static = self.loss = None   # ... and the one used last
        self.failed = None
        optim.use_device_scalars(True)
        self.epoch = ops.dropout_epoch(params[0].device)
        # ONE side stream for the eager steps and for the capture: autograd binds an AccumulateGrad node to the stream
        # it was created on and keeps synchronising with that stream for as long as the node lives; eager steps on the
        # caller's stream followed by a capture on another one left the captured graph with unordered work (seen as
        # garbage gradients a few hundred replays in: tools/lab/train_soak.py)
        self.stream = torch.cuda.Stream(device=params[0].device)

    @property
    def graph(self):
        """The first segment of the captured step used last; None until something is captured."""
        return self.segments[0] if self.segments else None

    @staticmethod
    def _signature(batch):
        return tuple((k, tuple(v.shape), v.dtype) for k, v in sorted(batch.items()) if torch.is_tensor(v))

    def _record(self, static):
        """Capture the step on ``static``: (graph segments, loss tensor)."""
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=self.stream):
            loss = train_step(self.model, self.optim, self.params, self.clip, static, ema=self.ema)
            self.epoch.add_(1)
        return (graph,), loss

    def _between_segments(self):
        """What a replay runs between two segments (here there is one)."""

    def _capture(self, batch):
        """Records (does not execute) the step of this batch's signature; returns its ``graphs`` entry."""
        dev = self.params[0].device
        static = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}
        import gc
        gc.collect()                                 # autograd graphs of earlier steps (and their AccumulateGrad nodes) gone
        autograd.forget_transposes({id(p) for p in self.model.parameters()})   # nothing of another model in this graph
        torch.cuda.synchronize(dev)
        self.optim.zero_grad(set_to_none=True)       # the gradients of the replayed step live in the graph's pool
        self.optim.sync_lr()
        self.optim.new_capture_staging()             # (an earlier graph keeps re-reading ITS gradient addresses from its own)
        quiet = getattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch", None)
        if quiet is not None:      # AccumulateGrad nodes of the eager steps meet the capture stream once: expected here
            quiet(False)
        try:
            segments, loss = self._record(static)
        finally:
            if quiet is not None:
                quiet(True)
        self.optim.note_replayed_step(-1)            # capture ran step()'s host bookkeeping without executing anything
        self.tab = self.optim._e3d_tab               # the optimizer tables (parameter / moment pointers) the graph baked
        self.ptrs = [p.data_ptr() for p in self.params]
        return dict(graphs=segments, static=static, loss=loss, grads=[p.grad for p in self.params])

    def _stale(self):
        """The graph carries raw pointers: parameters that moved (``module.to()``) or optimizer state that was replaced
        (``load_state_dict``: ClipAdamW drops its tables) invalidate it, and so does an attached EMA whose count or law
        was set from outside (``WeightEMA.load_state_dict``: the device words are behind) -- warm up and capture again."""
        return (self.optim._e3d_tab is not self.tab or any(p.data_ptr() != q for p, q in zip(self.params, self.ptrs))
                or not self.optim.ema_words_current())

    def _may_capture(self, key):
        return (self.failed is None and key not in self.graphs and len(self.graphs) < self.MAX_GRAPHS
                and self.seen.get(key, 0) >= self.warmup)

    def _select(self, key):
        """Make the captured step of this signature the current one; False if there is none."""
        e = self.graphs.get(key)
        if e is None:
            return False
        if self.params[0].grad is not e["grads"][0]:   # ``p.grad`` shows the gradients of the step that ran last
            for p, g in zip(self.params, e["grads"]):
                p.grad = g
        self.segments, self.static, self.loss, self.key = e["graphs"], e["static"], e["loss"], key
        return True

    def _drop_graphs(self):
        self.graphs, self.seen = {}, {}
        self.segments = self.key = self.static = self.loss = None

    def _on_stream(self, fn, *args):
        """``fn(*args)`` (returns the loss) on ``self.stream``, ordered after and before the caller's current stream."""
        cur = torch.cuda.current_stream(self.stream.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            loss = fn(*args)
        cur.wait_stream(self.stream)
        loss.record_stream(cur)
        return loss

    def _replay(self, batch):
        for k, v in batch.items():
            if torch.is_tensor(v):
                self.static[k].copy_(v, non_blocking=True)
        self.optim.sync_lr()
        for i, graph in enumerate(self.segments):
            if i:
                self._between_segments()
            graph.replay()
        self.optim.note_replayed_step()
        ops.invalidate_weight_caches()
        return self.loss

    def _replayed(self, batch):
        key = self._signature(batch)
        if self.graphs and self._stale():
            self._drop_graphs()
        if self._may_capture(key):
            try:
                self.graphs[key] = self._capture(batch)    # (this batch runs as the first replay below)
            except Exception as e:                  # noqa: BLE001 -- any capture failure: stay eager, say so once
                self.failed = e
                self._drop_graphs()
                import traceback
                import warnings
                warnings.warn(f"{self.CAPTURE_FAILED}, staying eager: {e!r}\n" + "".join(traceback.format_exc(limit=-6)))
        if not self._select(key):
            self.seen[key] = self.seen.get(key, 0) + 1
            return None
        return self._on_stream(self._replay, batch) if self.REPLAY_ON_SIDE_STREAM else self._replay(batch)

    def _eager_body(self, batch, batch_idx):
        loss = train_step(self.model, self.optim, self.params, self.clip, batch, batch_idx, self.averager, self.ema).detach()
        self.epoch.add_(1)
        return loss

    def _eager(self, batch, batch_idx):
        return self._on_stream(self._eager_body, batch, batch_idx)


class GraphedDDPStep(GraphedStep):
    """The data-parallel step as TWO graph segments around the collectives: forward + backward (gradients written straight into
    the GradientAverager's flat buckets) | all-reduce of the buckets, eager: RCCL calls are not captured | mean, gradient-norm
    clip and AdamW.  ``world > 1`` then costs two replays and a handful of ``all_reduce`` calls per step instead of ~1 350
    eager launches (the eager data-parallel step was host-bound: as much Python as kernel time).  Captured after ``warmup``
    eager steps through the ordinary overlapped path (``prepare`` / hooks / ``average``), so every rank reaches the capture at
    the same step; ``E3D_TRAIN_GRAPH=0`` keeps that eager path for every step.  The buckets travel AFTER the backward segment
    (the eager path overlaps them with it): ~1-2 ms for the sequence model's 289 MB on eight GPUs against a ~20-ms step."""

    REPLAY_ON_SIDE_STREAM = True                     # replay and eager alike inside self.stream
    CAPTURE_FAILED = "data-parallel training step could not be captured in HIP graphs"

    def __init__(self, model, optim, params, gradient_clip, averager, warmup=2, ema=None):
        super().__init__(model, optim, params, gradient_clip, warmup, ema=ema)
        self.averager = averager
        self.world = torch.distributed.get_world_size()

    def _record(self, static):
        avg = self.averager
        g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1, stream=self.stream):
            loss = self.model.training_step(static, 0)
            avg.bind(collect_only=True)          # gradients = zeroed views of the flat buckets; hooks only take notes
            backward(loss, avg)
            self.epoch.add_(1)
        avg.finish_collect()                      # never-used parameters: grad None, as in every eager step
        with torch.cuda.graph(g2, stream=self.stream, pool=g1.pool()):
            for flat in avg.flats():
                flat.div_(self.world)
            clip_and_step(self.params, self.optim, self.clip, ema=self.ema)   # (the EMA rides in the update launch)
        return (g1, g2), loss

    def _between_segments(self):
        self.averager.all_reduce_flats()             # the only eager launches of the step


def make_stepper(model, optim, params, gradient_clip, averager=None, graph=None, ema=None):
    """The stepper a run gets: the step replayed from HIP graphs where that is possible (GPU parameters under ClipAdamW;
    ``graph`` None: E3D_TRAIN_GRAPH) -- ``GraphedStep`` for one process, ``GraphedDDPStep`` under an active averager whose
    hooks are in place -- and ``EagerStep`` everywhere else.  ``ema``: the run's ``WeightEMA``, attached to a ClipAdamW
    here (its update then rides in the optimizer's launch, captured with it) and updated in plain torch otherwise."""
    from .optim import ClipAdamW
    if ema is not None and isinstance(optim, ClipAdamW) and optim.ema is not ema:
        optim.attach_ema(ema)
    if (GRAPH_TRAIN if graph is None else graph) and params and params[0].is_cuda and isinstance(optim, ClipAdamW):
        if averager is None or not averager._active():
            return GraphedStep(model, optim, params, gradient_clip, ema=ema)
        if averager._hooked:
            return GraphedDDPStep(model, optim, params, gradient_clip, averager, ema=ema)
    return EagerStep(model, optim, params, gradient_clip, averager, ema=ema)


# the tensors of a dataset.py batch that are laid out [B, L, ...] over the ligand / the pocket frame
# (structure_model/dataset.py:119-162, sequence_model/dataset.py: the same names)
LIGAND_FRAME_KEYS = ("ligand_angles", "ligand_attn_mask", "ligand_seq", "known_noise", "noised_ligand_angle")
RECEPTOR_FRAME_KEYS = ("receptor_angles", "receptor_attn_mask", "receptor_seq")
TRIM_TRAIN = os.environ.get("E3D_TRAIN_TRIM", "0") == "1"            # default of fit(trim_padding=None)
KEYED_DROPOUT = os.environ.get("E3D_TRAIN_KEYED_DROPOUT", "1") == "1"   # default of fit(seed=, keyed_dropout=None)


def trimmed_frame(batch, multiple=32):
    """(ligand rows, pocket rows) that cover every valid position of the batch, rounded up to the attention tile."""
    return (trimmed_length(batch["ligand_attn_mask"], multiple), trimmed_length(batch["receptor_attn_mask"], multiple))


def trim_batch(batch, frame=None, multiple=32):
    """The batch on the frame of its longest ligand / pocket (``frame``: rows agreed on elsewhere, e.g. across ranks).

    dataset.py pads every item to ``max_seq_len`` = 128 rows; BioLiP ligands are 5-30 residues, so 3 of the decoder's 4
    attention tiles -- and 3/4 of the rows of every decoder GEMM, LayerNorm and activation -- are padding.  Padding cannot
    reach a valid position in the forward pass (its keys carry the -10000 bias, whose softmax weight underflows to exactly
    0.0f; every other op is row-wise) and receives exactly zero gradient in the backward pass (the losses are means over
    valid positions), so loss and parameter gradients of the trimmed batch are those of the padded one up to the order of
    the fp32 sums (tests/test_training_gpu.py::test_trimmed_*).  What changes: draws made per frame position inside the
    step (dropout, PeptideDiff.apply_aa_noise) come from a different place of the random stream -- unless they are keyed
    (``fit(seed=)``): the noising draws and the dropout decisions of a seeded run follow the item and its positions, not
    the frame (tests/test_keyed_dropout_gpu.py)."""
    Ll, Lr = frame if frame is not None else trimmed_frame(batch, multiple)
    out = dict(batch)
    for keys, n in ((LIGAND_FRAME_KEYS, Ll), (RECEPTOR_FRAME_KEYS, Lr)):
        for k in keys:
            v = out.get(k)
            if torch.is_tensor(v) and v.dim() >= 2 and v.shape[1] > n:
                out[k] = v[:, :n].contiguous()
    return out


def move_batch(batch, device):
    return {k: (v.to(device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}


class ItemIdDataset(torch.utils.data.Dataset):
    """A dataset's items plus ``item_id`` (int64 scalar: the index in this dataset), the key of the seeded training and
    validation draws (``fit(seed=)``; DESIGN.md, "Keyed sampling streams").  The default collate turns it into the
    batch's int64 [B]; every other entry is the wrapped dataset's, untouched, and its attributes (``feature_names``,
    ``tables``, ...) are reachable through the wrapper.

    ``skip_noising`` (a ``NoisedAnglesDataset`` inside): serve the un-noised item and zeros for ``timestep``,
    ``known_noise`` and ``noised_ligand_angle`` -- a seeded ``fit`` replaces the three on the device, so the CPU draws
    would be thrown away."""

    def __init__(self, dset, skip_noising=False):
        super().__init__()
        if skip_noising and not hasattr(dset, "dset"):
            raise ValueError("skip_noising needs a dataset that wraps the un-noised one (NoisedAnglesDataset)")
        self.dset, self.skip_noising = dset, skip_noising

    def __getattr__(self, name):
        if name == "dset":                       # (not set yet: unpickling in a DataLoader worker)
            raise AttributeError(name)
        return getattr(self.dset, name)

    def __len__(self):
        return len(self.dset)

    def __getitem__(self, index):
        if self.skip_noising:
            item = dict(self.dset.dset[index])
            angles = item["ligand_angles"]
            item.update(timestep=torch.zeros(1, dtype=torch.int64), known_noise=torch.zeros_like(angles),
                        noised_ligand_angle=torch.zeros_like(angles))
        else:
            item = dict(self.dset[index])
        if "item_id" in item:
            raise ValueError("the wrapped dataset's items already carry an 'item_id'")
        item["item_id"] = torch.tensor(index, dtype=torch.int64)
        return item


class _KeyedDraws:
    """What a seeded ``fit`` holds: the seed, the epoch word in device memory, and -- for a model whose batches arrive
    noised (structure model) -- the schedule tables to noise them again on the device from streams 4 / 5.  For the run it
    also switches the model's dropout to keyed decisions (streams 8 / 9) unless ``keyed_dropout`` is off."""

    def __init__(self, model, seed, device, max_epochs, loader, noise_tables, noise_scale, keyed_dropout=True):
        self.seed = keyed.check_seed(seed)
        keyed.check_epoch(max(0, max_epochs - 1))
        self.word = keyed.epoch_word(device)
        self.model = model if hasattr(model, "use_keyed_draws") else None    # draws inside the step (sequence model)
        # dropout decisions keyed by the same seed, ids and epoch word (both models: blocks.KeyedDropoutSwitch)
        self.dropout_model = model if keyed_dropout and hasattr(model, "use_keyed_dropout") else None
        self.tables = self.scale = None
        if self.model is None:
            ds = getattr(loader, "dataset", None)
            tables = noise_tables if noise_tables is not None else getattr(ds, "tables", None)
            if tables is None:
                raise ValueError("a seeded fit noises the batches on the device and needs the schedule tables: "
                                 "a loader over a NoisedAnglesDataset (inside training.ItemIdDataset), or noise_tables=")
            self.scale = float(noise_scale if noise_scale is not None else getattr(ds, "angular_var_scale", 1.0))
            keyed.check_steps(tables.timesteps)
            self.tables = _DeviceTables(tables, device)

    def __enter__(self):
        if self.model is not None:
            self.model.use_keyed_draws(self.seed, self.word)
        if self.dropout_model is not None:
            self.dropout_model.use_keyed_dropout(self.seed, self.word)
        return self

    def __exit__(self, *exc):
        if self.model is not None:
            self.model.use_keyed_draws(None)
        if self.dropout_model is not None:
            self.dropout_model.use_keyed_dropout(None)

    def set_epoch(self, epoch):
        keyed.set_epoch(self.word, epoch)

    def batch(self, batch):
        """The batch as the step takes it (on the device already)."""
        ids = keyed.batch_item_ids(batch, batch["ligand_angles"].shape[0])
        if self.tables is None:
            return batch
        from .structure_model.dataset import noise_batch_on_device
        return dict(batch, **noise_batch_on_device(batch["ligand_angles"], self.tables, scale=self.scale, seed=self.seed,
                                                   item_ids=ids, epoch=self.word))


class _DeviceTables:
    """The two forward-noising tables of a ``CosineTables`` on the device, copied once."""

    def __init__(self, tables, device):
        self.timesteps = tables.timesteps
        self.sqrt_alphas_cumprod = tables.sqrt_alphas_cumprod.to(device)
        self.sqrt_one_minus_alphas_cumprod = tables.sqrt_one_minus_alphas_cumprod.to(device)


class BestCheckpoint:
    """ModelCheckpoint(monitor='val_loss', save_top_k=1, mode=...) semantics; the reference passes
    mode='max', i.e. it keeps the HIGHEST validation loss -- reproduced by default."""

    def __init__(self, path, mode="max", ema=None):
        self.path, self.mode, self.best = path, mode, None
        self.ema = ema                                   # a WeightEMA: the file holds ITS weights (model_state_dict)

    def update(self, model, val_loss, rank=0):
        better = self.best is None or (val_loss > self.best if self.mode == "max" else val_loss < self.best)
        if better:
            self.best = val_loss
            if rank == 0 and self.path:
                torch.save(model.state_dict() if self.ema is None else self.ema.model_state_dict(model), self.path)
        return better


# The reference trains with torch.set_float32_matmul_precision("medium") (structure_model/train_model.py:120,
# sequence_model/train_model.py:114): bf16 products.  bf16x3 is 500x finer per product and is the arithmetic every
# backward kernel of this package exists in; the inference default (f16x3) has forward kernels only.
# E3D_TRAIN_ARITHMETIC=bf16 (opt-in): the reference's own training precision -- plain bf16 products in every GEMM (forward,
# input and weight gradients), bf16x3 in the attention kernels; ~1e-2-grade gradients instead of ~1e-4-grade.
TRAIN_ARITHMETIC = os.environ.get("E3D_TRAIN_ARITHMETIC", "bf16x3")


def _step_batch(batch, device, draws, trim, frame=None):
    """A loader's batch as a step takes it: trimmed (on the loader's host tensors: no device round trip; ``frame``: rows
    agreed on elsewhere), moved to the device, its keyed draws made."""
    if trim:
        batch = trim_batch(batch, frame)
    batch = move_batch(batch, device)
    return batch if draws is None else draws.batch(batch)


def fit(model, train_loader, val_loader=None, *, max_epochs, min_epochs=0, gradient_clip=1.0, device="cuda:0",
        log_every_n_steps=30, checkpoint_path="./best_val_model.pt", checkpoint_mode="max", max_steps=None,
        log=print, trim_padding=None, seed=None, noise_tables=None, noise_scale=None, keyed_dropout=None,
        ema_decay=None, ema_warmup=True):
    """Returns a history dict.  ``model`` provides training_step / validation_step /
    configure_optimizers (the reference's LightningModule surface).
    ``seed`` (default None: torch's generators, as ever): keyed training and validation draws ("Keyed sampling
    streams").  An item's timestep and noise are then functions of (seed, batch["item_id"], epoch, position) alone --
    not of the batch, the row, the frame, the DataLoader workers or the world size -- and validation draws do not depend on
    the epoch, so ``val_loss`` is a function of the weights.  Batches must carry ``item_id`` (``ItemIdDataset``).  A
    model with ``use_keyed_draws`` (sequence model) draws inside its step; any other gets ``timestep`` / ``known_noise`` /
    ``noised_ligand_angle`` replaced on the device before the step, with the tables of the loader's dataset
    (``NoisedAnglesDataset.tables`` / ``.angular_var_scale``) or ``noise_tables`` / ``noise_scale``.
    ``keyed_dropout`` (None: E3D_TRAIN_KEYED_DROPOUT, default on): under a seed, the dropout decisions of every training step
    are keyed as well -- functions of (seed, item id, epoch, dropout site, position, head, column or key) -- so a seeded
    run with dropout > 0 is reproducible whatever the batch, frame, launch mode or point of resumption; False keeps
    torch-seeded dropout under the seed.  Without a seed it has no effect.
    ``trim_padding`` (None: E3D_TRAIN_TRIM, default off = the reference's padded frames): run every training and
    validation step on the frame of the batch's longest ligand / pocket (``trim_batch``; under a process group the frame
    is the maximum over the ranks, agreed on the host, so that every rank replays the same kind of step).
    ``ema_decay`` (None: none, today's run): keep a ``WeightEMA`` of the trainable parameters with this decay
    (``ema_warmup``: the warm-up of ``ema_decay_at``), updated with every step -- inside the update launch of a ClipAdamW,
    in plain torch otherwise.  Validation then runs on the EMA weights (``WeightEMA.swapped``), the checkpoint file holds
    them (``model_state_dict``: the model's own keys, so the samplers load it as ever), ``history["ema_updates"]`` counts
    the updates and ``history["ema"]`` is the instance, for the caller to save or carry on.  Data-parallel runs need no
    collective for it: the ranks apply identical averaged gradients and hold identical shadows."""
    trim = TRIM_TRAIN if trim_padding is None else bool(trim_padding)
    with contextlib.ExitStack() as whole_run:
        whole_run.enter_context(ops.arithmetic(TRAIN_ARITHMETIC))
        rank, world, _ = sharding.init_distributed()
        model.to(device)
        draws = None
        if seed is not None:
            keyed_drop = KEYED_DROPOUT if keyed_dropout is None else bool(keyed_dropout)
            draws = whole_run.enter_context(
                _KeyedDraws(model, seed, device, max_epochs, train_loader, noise_tables, noise_scale, keyed_drop))
        sharding.broadcast_parameters(model, src=0)
        conf = model.configure_optimizers()
        optim = conf["optimizer"]
        sched = conf.get("lr_scheduler") or {}
        params = [p for p in model.parameters() if p.requires_grad]
        ema = None if ema_decay is None else WeightEMA(model, ema_decay, ema_warmup)
        averager = sharding.GradientAverager(model.parameters())
        stepper = make_stepper(model, optim, params, gradient_clip, averager) if ema is None else \
            make_stepper(model, optim, params, gradient_clip, averager, ema=ema)
        ckpt = BestCheckpoint(checkpoint_path, checkpoint_mode) if ema is None else \
            BestCheckpoint(checkpoint_path, checkpoint_mode, ema=ema)
        history = {"train_loss": [], "val_loss": [], "steps": 0, "seconds": 0.0}
        t0 = time.perf_counter()
        step = 0
        for epoch in range(max_epochs):
            model.train()
            if hasattr(getattr(train_loader, "sampler", None), "set_epoch"):
                train_loader.sampler.set_epoch(epoch)
            if draws is not None:
                draws.set_epoch(epoch)
            losses = []
            for batch_idx, batch in enumerate(train_loader):
                frame = sharding.max_over_ranks_host(trimmed_frame(batch)) if trim and world > 1 else None
                loss = stepper.step(_step_batch(batch, device, draws, trim, frame), batch_idx)
                if sched.get("interval") == "step":
                    sched["scheduler"].step()
                losses.append(loss.detach().clone())     # (a replayed step's loss tensor is overwritten by the next replay)
                step += 1
                if rank == 0 and log_every_n_steps and step % log_every_n_steps == 0:
                    log(f"epoch {epoch} step {step} train_loss {float(losses[-1]):.5f}")
                if max_steps is not None and step >= max_steps:
                    break
            if sched.get("interval") == "epoch":
                sched["scheduler"].step()
            # the per-step losses stay on the device until here: a float() per step would make the host wait for every step
            # (Lightning reads the loss for its progress bar every step; the values of the logged steps are the same)
            losses = torch.stack(losses).double().cpu().tolist() if losses else []
            mean_train = sum(losses) / max(1, len(losses))
            history["train_loss"].append(mean_train)
            if rank == 0:
                log(f"Traning Loss:{mean_train}")
            if val_loader is not None:
                model.eval()
                vals = []
                if draws is not None:
                    draws.set_epoch(None)                # the validation value: the same draws after every epoch
                with torch.no_grad(), (contextlib.nullcontext() if ema is None else ema.swapped(model)):
                    for batch_idx, batch in enumerate(val_loader):
                        out = model.validation_step(_step_batch(batch, device, draws, trim), batch_idx)
                        vals.append(float(out["val_loss"] if isinstance(out, dict) else out))
                if draws is not None:
                    draws.set_epoch(epoch)
                val = sum(vals) / max(1, len(vals)) if vals else math.nan
                if world > 1:
                    val = sharding.mean_over_ranks(val)
                history["val_loss"].append(val)
                if rank == 0:
                    log(f"Validation Loss:{val}")
                if not math.isnan(val):
                    ckpt.update(model, val, rank)
            if max_steps is not None and step >= max_steps:
                break
        history["steps"] = step
        history["seconds"] = time.perf_counter() - t0
        if ema is not None:
            history["ema_updates"], history["ema"] = ema.num_updates, ema
        return history
