"""Discrete reverse sampler of the sequence model -- entry point and function names of the
reference's sequence_model/sample.py.  The posterior (sample.py:120-139), its mixture with the
predicted x0 distribution and the categorical draw (sample.py:141-179: a Python loop over B*L
rows with a device sync per row in the reference) are ONE HIP launch, ``e3d_discrete_posterior_sample``.

Run as ``python sample.py`` from this directory after editing the constants, like the reference.
"""
if __package__ in (None, ""):  # executed as a script from inside this directory
    import os as _os, sys as _sys
    _sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))))
    import __graft_entry__ as _g
    _g.load_package()
    __package__ = "e3diff_amd.sequence_model"

import os
from dataclasses import dataclass

import torch
from torch.nn import functional as F
from torch.utils.data import DataLoader

from .. import keyed, ops, packing
from ..bert import BertConfig
from .dataset import AA_VOCAB, SPLIT_FILE, LigandBindingSiteDataset
from .model import PeptideDiff, onehot_to_index
from .utils import BlosumTransition, DiscreteUniformTransition, PredefinedNoiseScheduleDiscrete  # noqa: F401

GPU_ID = 0
DEVICE = torch.device(f"cuda:{GPU_ID}")
THREAD_NUM = 16
DATA_PATH = "./data/biolip.pt"
MODEL_PATH = ""  # trained state_dict (reference checkpoint key names)
OUTPUT_PATH = "./data/from_generated_angles/output.pkl"
# Packed chains (denoise(pack=True)): the batch runs on its valid rows only; off by default, E3D_SAMPLE_PACK=1 turns it
# on for ``run()``.
PACK = os.environ.get("E3D_SAMPLE_PACK", "0") == "1"
# Keyed draws (``run(seed=...)``): the initial one-hots and the posterior uniforms of a ligand are a function of
# (seed, dataset index), whatever its batch, order or frame.  None (default): torch's generator, as before.
SEED = int(os.environ["E3D_SAMPLE_SEED"], 0) if os.environ.get("E3D_SAMPLE_SEED") else None
# Partial redesign (``run(keep=...)``, E3D_SAMPLE_KEEP): ligand positions held at the record's own residues while the rest
# is sampled, e.g. "0-3,7" (packing.keep_mask).  "" (default): the whole sequence is designed, as before.
KEEP = os.environ.get("E3D_SAMPLE_KEEP", "")
# Design controls (``run(temperature=..., omit=..., allow=...)``; design.DesignControls): the sampling temperature of the
# steps s > 0, residue letters forbidden at every position ("CM"), and the residues allowed at chosen 0-based ligand
# positions ("3:LIV;7:DE").  Unset (default): the chain runs the launches it always ran.
TEMPERATURE = float(os.environ["E3D_SAMPLE_TEMPERATURE"]) if os.environ.get("E3D_SAMPLE_TEMPERATURE") else None
OMIT = os.environ.get("E3D_SAMPLE_OMIT", "")
ALLOW = os.environ.get("E3D_SAMPLE_ALLOW", "")

CONFIG = {
    "pocket_ext": 0,
    "timesteps": 50,
    "max_seq_len": 64,
    "noise_schedule": "cosine",

    "num_heads": 12,
    "dropout_p": 0.1,
    "hidden_size": 768,
    "num_hidden_layers": 6,
    "intermediate_size": 1024,
    "position_embedding_type": "relative_key",

    "lr": 5e-5,
    "l2_norm": 0.1,
    "loss": "smooth_l1",
    "gradient_clip": 1.0,
    "lr_scheduler": "LinearWarmup",

    "min_epochs": 100,
    "max_epochs": 150,
    "batch_size": 64,
}


def get_dataloader(file_path):
    ds = LigandBindingSiteDataset(file_path, "test", CONFIG["max_seq_len"], CONFIG["pocket_ext"],
                                  split_file=SPLIT_FILE or None)   # E3D_SPLIT_FILE
    return DataLoader(dataset=ds, batch_size=CONFIG["batch_size"], shuffle=False, num_workers=THREAD_NUM)


def build_configs(cfg=None):
    cfg = cfg or CONFIG
    common = dict(max_position_embeddings=cfg["max_seq_len"], num_attention_heads=cfg["num_heads"],
                  hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                  num_hidden_layers=cfg["num_hidden_layers"],
                  position_embedding_type=cfg["position_embedding_type"],
                  hidden_dropout_prob=cfg["dropout_p"], attention_probs_dropout_prob=cfg["dropout_p"],
                  use_cache=False)
    return BertConfig(**common), BertConfig(**common, is_decoder=True, add_cross_attention=True)


def get_model(steps_per_epoch, model_path=None) -> PeptideDiff:
    encoder_config, decoder_config = build_configs()
    model = PeptideDiff(
        encoder_config=encoder_config, decoder_config=decoder_config,
        feature_names=LigandBindingSiteDataset.feature_names, max_epochs=CONFIG["max_epochs"],
        lr_scheduler=CONFIG["lr_scheduler"], l2_lambda=CONFIG["l2_norm"], steps_per_epoch=steps_per_epoch,
        learning_rate=CONFIG["lr"], loss_func=torch.nn.CrossEntropyLoss(),
        noise_schedule=CONFIG["noise_schedule"], timesteps=CONFIG["timesteps"])
    path = MODEL_PATH if model_path is None else model_path
    if path:
        model.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
    model = model.eval().to(DEVICE)
    print(f"Model has {sum(p.numel() for p in model.parameters() if p.requires_grad)} trainable parameters")
    return model


def generate_discrete_noise(batch_size, length, num_classes=20, device=None):
    """Uniform random one-hot [B,L,C] (reference sample.py:112-116), drawn on the device."""
    device = DEVICE if device is None else device
    idx = torch.randint(0, num_classes, (batch_size, length), device=device)
    return F.one_hot(idx, num_classes).float()


def keyed_discrete_noise(seed, item_ids, length, num_classes=20, device=None):
    """Keyed x_T [B,L,C]: the one-hot of the stream-2 class of (seed, item_ids[b], l) -- generate_discrete_noise's
    distribution, drawn per item instead of per batch."""
    device = DEVICE if device is None else device
    ids = keyed.item_ids(item_ids, len(item_ids))
    keys = keyed.padded_keys(ids, length, device)
    return ops.keyed_initial_onehot(keys, seed, num_classes).reshape(len(ids), length, num_classes)


def compute_batched_over0_posterior_distribution(X_t, Q_t, Qsb, Qtb, batch):
    """[N,C,C] posterior table  (x_t Qt^T) * Qsb / (Qtb x_t)  (reference sample.py:120-139).
    API-compatibility helper in plain torch: the sampler below never materialises this tensor
    (it is fused into the HIP kernel)."""
    left = X_t.unsqueeze(-2) @ Q_t.transpose(-1, -2)[batch]
    den = Qtb[batch] @ X_t.unsqueeze(2)
    den = torch.where(den == 0, torch.full_like(den, 1e-6), den)
    return left * Qsb[batch] / den


@dataclass(frozen=True)
class DrawPlan:
    """How a chain draws z_s from the posterior, decided and checked once per chain (``draw_plan``), as
    structure_model/sample.py::StepPlan is for the angle chain; ``step`` is the one place the sampler calls the four
    posterior and the two compose launches from.  ``diverse``: categorical draws, else argmax (which reads no uniforms).
    ``keyed`` = (row keys [B*L, 2], seed): the uniforms are generated inside the kernels at the step ``s_dev`` (int64 on
    the device), stream 3 for the posterior and 11 for the held rows (keyed.py); None: uniforms [B,L], injected or
    torch.rand on the device.  ``known_x0`` (class indices int32 [B,L]) + ``known_mask`` (uint8 [B,L]): the held rows,
    redrawn from q(z_s | x0) -- column x0 of Qsb, ``PeptideDiff.apply_aa_noise``'s law at the level the step lands on.
    ``controls``: an active design.DesignControls whose bias, if any, has the logits' shape: the x0 prediction is
    softmax((logits + bias) * inv_temp)."""
    diverse: bool
    keyed: tuple = None
    known_x0: torch.Tensor = None
    known_mask: torch.Tensor = None
    controls: object = None

    def _uniforms(self, rows, u):      # of an unkeyed launch: None for argmax, else the injected ones or a fresh draw
        if not self.diverse:
            return None
        return torch.rand(rows.shape, device=rows.device) if u is None else u.contiguous().float()

    def posterior(self, xt_idx, logits, qsb, qtb, s_dev=None, u=None):
        """Class indices int32 [B,L] of z_s given z_t = ``xt_idx`` and the model's ``logits``."""
        c = self.controls
        if self.diverse and self.keyed is not None:
            if u is not None:      # here, not in draw_plan: the uniforms are a step's operand, not the chain's
                raise ValueError("sample_p_zs_given_zt_discrete: pass either uniforms or a keyed draw, not both")
            if c is None:
                return ops.keyed_discrete_posterior_sample(xt_idx, logits, qsb, qtb, *self.keyed, s_dev)
            return ops.keyed_discrete_posterior_sample_ctl(xt_idx, logits, c.bias, c.inv_temp, qsb, qtb, *self.keyed, s_dev)
        u = self._uniforms(xt_idx, u)
        if c is None:
            return ops.discrete_posterior_sample(xt_idx, logits, qsb, qtb, u)
        return ops.discrete_posterior_sample_ctl(xt_idx, logits, c.bias, c.inv_temp, qsb, qtb, u)

    def compose(self, idx, qsb, s_dev=None, u=None):
        """Redraw the held rows of ``idx`` in place; returns ``idx``."""
        if self.known_x0 is None:
            return idx
        if self.diverse and self.keyed is not None:
            return ops.keyed_discrete_known_compose(idx, self.known_x0, self.known_mask, qsb, *self.keyed, s_dev)
        return ops.discrete_known_compose(idx, self.known_x0, self.known_mask, qsb, self._uniforms(idx, u))

    def step(self, t, s, x, logits, noise_schedule, transition, s_dev=None, u=None, known_u=None):
        """One-hot z_s [B,L,C] from z_t = ``x`` at the normalised times t -> s: the two tables, ``posterior``, ``compose``."""
        qtb = transition.get_Qt_bar(noise_schedule.get_alpha_bar(t_normalized=t), x.device).contiguous()
        qsb = transition.get_Qt_bar(noise_schedule.get_alpha_bar(t_normalized=s), x.device).contiguous()
        idx = self.posterior(x.argmax(dim=-1).to(torch.int32).contiguous(), logits.contiguous().float(), qsb, qtb, s_dev, u)
        return F.one_hot(self.compose(idx, qsb, s_dev, known_u).long(), num_classes=x.shape[-1]).float()


def draw_plan(diverse, row_keys=None, seed=None, known_x0=None, known_mask=None, controls=None):
    """The DrawPlan of a chain, checked; its operands are in the chain's frame.  Controls with nothing set count as None."""
    if (row_keys is None) != (seed is None):
        raise ValueError("draw_plan: keyed draws need both row_keys and a seed")
    return DrawPlan(bool(diverse), None if seed is None else (row_keys, keyed.check_seed(seed)), known_x0, known_mask,
                    None if controls is None or not controls.active else controls)


def sample_p_zs_given_zt_discrete(t, s, noised_data, pred_noise, noise_schedule, transition, diverse,
                                  is_last_step, u=None, keyed_draw=None, known=None, controls=None):
    """z_s ~ p(z_s | z_t) for every residue (reference sample.py:141-179).  ``diverse`` draws from the categorical
    (inverse CDF with uniforms ``u`` [B,L], default torch.rand on device), otherwise argmax; the last step returns the raw
    logits, as the reference does (``denoise`` puts the held residues there and picks under the controls, once per chain).
    One step of a DrawPlan made of the keywords: ``keyed_draw`` = (row keys, seed, int64 step on the device), exclusive
    with ``u``; ``known`` = (x0 class indices, uint8 mask, uniforms of the held rows or None); ``controls``."""
    if is_last_step:
        return pred_noise
    row_keys, seed, s_dev = keyed_draw or (None, None, None)
    known_x0, known_mask, known_u = (*(known or (None, None)), None)[:3]
    return draw_plan(diverse, row_keys, seed, known_x0, known_mask, controls).step(
        t, s, noised_data, pred_noise, noise_schedule, transition, s_dev, u, known_u)


def _denoise_step(model, s, T, x, args, layouts, noise_schedule, transition, plan, is_last_step, s_dev=None, u=None,
                  known_u=None):
    """One reverse step z_t -> z_s at the step index ``s`` ([B,1] float on the device), eager or captured.  ``args`` =
    (ligand angles, ligand mask, pocket sequence, pocket angles, pocket mask); with ``layouts`` the model runs packed and
    reads no mask.  ``plan``: the chain's DrawPlan; ``s_dev``, ``u``, ``known_u``: this step's operands of ``plan.step``.
    The last step returns the raw logits."""
    ang, lmask, rseq, rang, rmask = args
    if layouts is None:
        logits = model.forward(s, x, ang, lmask, rseq, rang, rmask)
    else:
        logits = model.forward_packed(s, x, ang, rseq, rang, *layouts)[None]
    return logits if is_last_step else plan.step((s + 1) / T, s / T, x, logits, noise_schedule, transition, s_dev, u, known_u)


class GraphedDenoiseStep:
    """One reverse step of the sequence chain -- ``model.forward`` + ``sample_p_zs_given_zt_discrete`` -- captured once
    into a HIP graph and replayed per step, as structure_model/sample.py::GraphedReverseStep does for the angle chain.
    What varies between steps lives on the device: the step index ``self.s`` ([B,1] float: both normalised times, the
    schedule look-ups and the timestep embedding are computed from it inside the graph), the state ``self.x`` and the
    uniforms of the categorical draw (drawn inside the graph, or injected through ``self.u``).  The last step of a chain
    (which returns the raw logits) is not replayed.  Small chains are host-bound when launched kernel by kernel (about
    150 launches per step): default for at most ``packing.GRAPH_MAX_ROWS`` token rows, ``use_graph`` /
    E3D_SAMPLE_GRAPH override."""

    def __init__(self, model, x_like, ligand_angles, ligand_mask, receptor_seq, receptor_angles, receptor_mask, noise_schedule,
                 transition, diverse, T, inject_u=False, layouts=None, row_keys=None, seed=None, known=None, controls=None,
                 plan=None):
        """``layouts`` = (ligand, pocket) packing.PackedLayout: the step runs ``model.forward_packed`` on packed rows
        (``x_like`` [1, rows, C], packed angles and pocket inputs; the masks are not read).  The layouts' device tables
        are fixed for the chain, so the capture holds them like any other argument.
        ``row_keys`` + ``seed``: the uniforms are the keyed stream of those rows at the integer step ``self.s_idx``.
        ``known`` = (x0 class indices, uint8 mask), both like ``x_like``'s first two dimensions: the held rows are composed
        inside the body; with ``inject_u`` their uniforms are injected too (``self.known_u``).
        ``controls``: a design.DesignControls in the frame of ``x_like``; its bias is copied into a buffer the capture
        holds, like the state.  ``plan``: the chain's DrawPlan, in place of ``diverse`` and those four keywords."""
        dev = x_like.device
        if (row_keys is None) != (seed is None) or (inject_u and (seed if plan is None else plan.keyed) is not None):
            raise ValueError("a keyed graph needs row_keys and a seed, and no injected uniforms")
        if plan is None:
            controls = None if controls is None or not controls.active else controls.in_frame(torch.clone, dev)
            plan = draw_plan(diverse, row_keys, seed, *(known or ()), controls=controls)
        self.plan, self.controls, diverse, known = plan, plan.controls, plan.diverse, plan.known_x0
        self.s_idx = torch.zeros((1,), device=dev, dtype=torch.long)
        self.args = (ligand_angles, ligand_mask, receptor_seq, receptor_angles, receptor_mask)
        self.layouts = layouts
        self.model, self.schedule, self.transition, self.T = model, noise_schedule, transition, T
        self.x = x_like.clone()
        self.s = torch.zeros((x_like.shape[0], 1), device=dev)
        self.u = torch.zeros(x_like.shape[:2], device=dev) if (inject_u and diverse) else None
        self.known_u = torch.zeros(x_like.shape[:2], device=dev) if (known is not None and self.u is not None) else None
        # the warm-up draws uniforms when the chain samples (diverse, no injected u): the device generator is put back
        self.graph, self.out = packing.warm_up_and_capture(self._body, dev, restore_rng=True)

    def _body(self):
        return _denoise_step(self.model, self.s, self.T, self.x, self.args, self.layouts, self.schedule, self.transition,
                             self.plan, False, self.s_idx, self.u, self.known_u)

    def step(self, s_int, x, u=None, known_u=None):
        """z_t -> z_s for the step index ``s_int`` (> 0); returns the graph's output buffer (overwritten by the next call)."""
        if (u is not None) != (self.u is not None):
            raise ValueError("this graph was captured %s injected uniforms" % ("with" if self.u is not None else "without"))
        self.s.fill_(float(s_int))
        self.s_idx.fill_(s_int)
        if x is not self.x:
            self.x.copy_(x)
        if u is not None:
            self.u.copy_(u)
        if (known_u is not None) != (self.known_u is not None):
            raise ValueError("this graph was captured %s injected uniforms for the held rows"
                             % ("with" if self.known_u is not None else "without"))
        if known_u is not None:
            self.known_u.copy_(known_u)
        self.graph.replay()
        return self.out


@torch.no_grad()
def denoise(batch, model: PeptideDiff, noise_schedule, transition, diverse, x_T=None, us=None,
            generated_angles=None, timesteps=None, trim_padding=False, use_graph=None, pack=False, seed=None,
            item_ids=None, known_mask=None, known_us=None, controls=None, details=None):
    """Full reverse chain over CONFIG["timesteps"] steps + recovery metrics (reference
    sample.py:181-229).  ``x_T`` / ``us`` inject the initial one-hot noise and the per-step
    uniforms (parity tests); ``generated_angles`` replaces the dataset's ligand angles
    (sample_by_generated_angles.py:202).

    ``pack=True``: the chain runs on the packed valid rows of the batch -- ligand and pocket (packing.PackedLayout,
    varlen attention, ``model.forward_packed``; every item shares the step's timestep) -- so its cost follows the
    residues the items have.  The results have the same form as the padded chain's.  ``x_T`` and ``us`` (padded layout)
    are gathered to the packed rows; the default initial noise is drawn in the padded frame as before, the default
    uniforms of ``diverse`` chains are drawn for the packed rows, i.e. from a different place in the random stream.
    Masks that are not prefix masks run the trimmed frame instead (with a warning); an item with ligand rows but an
    empty pocket raises ``ValueError``.  Trimmed and packed chains equal the padded one while every softmax row's
    scores spread over less than ~9900 (packing.Frame): beyond that the reference's additive -10000 mask lets padded
    keys win rows, and the packed path computes the absent-keys softmax instead (tests/test_varlen_forms_gpu.py::
    test_packed_path_computes_the_absent_keys_softmax_where_the_reference_lets_padded_keys_win).

    ``seed``: keyed draws (keyed.py, DESIGN.md "Keyed sampling streams"): x_T and the uniforms of item b are functions
    of (seed, item_ids[b], step, position) alone, so they do not depend on the batch, its order, the frame (padded /
    trimmed / packed) or eager / graph launches.  ``item_ids`` default to 0 .. B-1 (``run`` uses the dataset index).
    Exclusive with ``x_T`` / ``us``.

    Partial redesign -- ``known_mask`` bool [B, L]: the masked ligand positions are held at ``batch["ligand_seq"]`` while
    the rest is sampled (replacement conditioning).  After every step the held rows are redrawn from q(z_s | x0), the
    forward law at the level the step landed on (``e3d_discrete_known_compose``); the last step's held rows become the
    one-hot of the true residue.  The mask is and-ed with the padding mask.  ``known_us`` is the counterpart of ``us``
    for the held rows (a list of T [B, L] tensors; with ``us``); with a ``seed`` the uniforms are keyed stream 11 and
    stream 3 -- the free rows' draws -- is untouched.  The recovery rates returned and printed then cover the FREE
    positions only (the held ones recover by construction); an item with no free position reports NaN.  A mask with
    nothing set runs the chain exactly as without the argument.  No resampling loop; sample quality has not been measured
    here (no trained checkpoint ships with the tree).

    Design controls -- ``controls``: a design.DesignControls built for this batch (temperature, ``omit``, ``allow``,
    bias).  None, or a record with nothing set, runs the chain exactly as without the argument.  When active, the bias
    goes through the frame as the state does, every posterior launch takes the x0 prediction over
    (logits + bias) / temperature, and the last step picks on the device (``e3d_discrete_final_pick``: the argmax of the
    biased logits).  The controls shape the x0 prediction; the intermediate states are noisy by construction and may pass
    through a forbidden class.  The guarantee is on the output: a designed position of the returned sequence never holds
    a forbidden residue.  The temperature acts on the steps s > 0 only.  Held positions (``known_mask``) win over the
    controls.  Under a ``seed`` an item's design depends on (seed, item id, its own controls) alone.
    ``details``: a dict, filled with ``"logp"`` and ``"entropy"`` [B, L] (the log-probability of the picked residue and
    the entropy of the last step's distribution, padded frame, NaN off the ligand) and ``"score"`` [B], the mean of
    -logp over the designed positions (valid and not held; NaN when there are none), all on the CPU; it takes the
    device pick even without controls.  The four return values keep their meaning."""
    T = CONFIG["timesteps"] if timesteps is None else timesteps
    B, max_len, C = batch["ligand_seq"].shape
    if details is not None and not isinstance(details, dict):
        raise ValueError(f"denoise: details must be a dict to fill, got {type(details).__name__}")
    if controls is not None and not controls.active:
        controls = None
    if controls is not None and controls.bias is not None and tuple(controls.bias.shape) != (B, max_len, C):
        raise ValueError(f"denoise: the controls were built for {tuple(controls.bias.shape)}, the batch is {(B, max_len, C)}")
    if known_mask is None and known_us is not None:
        raise ValueError("denoise: known_us are the uniforms of the held positions; pass known_mask")
    if known_mask is not None:
        if known_us is not None and seed is not None:
            raise ValueError("denoise: pass either injected known_us or a seed, not both")
        if not torch.is_tensor(known_mask) or known_mask.dtype != torch.bool:
            raise ValueError(f"denoise: known_mask must be a bool tensor, got {getattr(known_mask, 'dtype', type(known_mask))}")
        if tuple(known_mask.shape) != (B, max_len):
            raise ValueError(f"denoise: known_mask must be {(B, max_len)}, got {tuple(known_mask.shape)}")
        if (known_us is None) != (us is None) and seed is None and diverse:
            raise ValueError("denoise: inject us and known_us together, or neither")
        if known_us is not None and len(known_us) != T:
            raise ValueError(f"denoise: known_us must hold {T} entries, one per step, got {len(known_us)}")
    dev = next(model.parameters()).device
    ids = None
    if seed is not None:
        if x_T is not None or us is not None:
            raise ValueError("denoise: pass either injected x_T / us or a seed, not both")
        seed = keyed.check_seed(seed)
        keyed.check_steps(T)
        ids = keyed.item_ids(item_ids, B)
        x_T = keyed_discrete_noise(seed, ids, max_len, C, dev)
    elif item_ids is not None:
        raise ValueError("denoise: item_ids key the seeded draws; pass a seed with them")
    x = generate_discrete_noise(B, max_len, C, dev) if x_T is None else x_T.to(dev)
    ligand_seq = batch["ligand_seq"].to(dev)
    ligand_mask = batch["ligand_attn_mask"].to(dev)
    ligand_angles = (batch["ligand_angles"] if generated_angles is None else generated_angles).to(dev)
    receptor_seq = batch["receptor_seq"].to(dev)
    receptor_angles = batch["receptor_angles"].to(dev)
    receptor_mask = batch["receptor_attn_mask"].to(dev)
    frame = packing.Frame(ligand_mask, receptor_mask, trim=trim_padding, pack=pack)
    layouts = frame.layouts

    def state(t):
        """A ligand-side state tensor in the frame: packed rows are one item of ``rows`` rows, [1, rows, ..]."""
        t = frame.ligand(t.float())
        return t if layouts is None else t[None]

    x = state(x)
    if us is not None:
        us = [state(u.to(dev)) if u is not None and u.dim() >= 2 else u for u in us]
    ang = frame.ligand(ligand_angles.float()).contiguous()
    rseq, rang = frame.pocket(receptor_seq.float()), frame.pocket(receptor_angles.float())
    lmask, rmask = (None, None) if layouts is not None else (frame.ligand(ligand_mask), frame.pocket(receptor_mask))
    row_keys = None if seed is None else frame.row_keys(ids, dev)
    if controls is not None:      # the bias into the frame like the state
        controls = controls.in_frame(state, dev)
    held = known = None
    if known_mask is not None:
        held = known_mask.to(dev) & (ligand_mask != 0)
        if not bool(held.any()):
            held = None
    if held is not None:      # class indices and mask into the frame like the state
        known = (state(ligand_seq.argmax(dim=-1)).to(torch.int32).contiguous(), state(held).to(torch.uint8).contiguous())
        if known_us is not None:
            known_us = [state(u.to(dev)).contiguous() if u is not None else u for u in known_us]
    else:
        known_us = None
    plan = draw_plan(diverse, row_keys, seed, *(known or ()), controls=controls)
    graphed = packing.capture_graph(
        lambda: GraphedDenoiseStep(model, x, ang, lmask, rseq, rang, rmask, noise_schedule, transition, diverse, T,
                                   inject_u=us is not None, layouts=layouts, plan=plan),
        frame.rows, T, use_graph, "the sequence reverse step")
    for n, s_int in enumerate(reversed(range(T))):
        u = None if us is None else us[n]
        ku = None if known_us is None else known_us[n]
        if graphed is not None and s_int > 0:
            x = graphed.step(s_int, x, u, ku if graphed.known_u is not None else None)
            continue
        s_array = torch.full((x.shape[0], 1), float(s_int), device=dev)     # [1, 1] packed: every item shares the step
        s_dev = None if plan.keyed is None else torch.full((1,), s_int, device=dev, dtype=torch.long)     # as in the graph
        x = _denoise_step(model, s_array, T, x, (ang, lmask, rseq, rang, rmask), layouts, noise_schedule, transition, plan,
                          s_int == 0, s_dev, u, ku)
    logp = entropy = None
    if controls is not None or details is not None:      # x holds the last step's logits: pick on the device
        idx, logp, entropy = ops.discrete_final_pick(x.contiguous().float(), None if controls is None else controls.bias,
                                                     1.0 if controls is None else controls.inv_temp,
                                                     want_scores=details is not None)
        x = F.one_hot(idx.long(), num_classes=C).float()
    x = frame.restore(x if layouts is None else x[0])
    if held is not None:      # the last step returned logits: the held rows are the true residues, once per chain
        x = torch.where(held[..., None], ligand_seq.float(), x)
    pred_idx, true_idx = x.argmax(dim=-1).cpu(), ligand_seq.argmax(dim=-1).cpu()
    mask = ligand_mask.bool().cpu()
    free = mask if held is None else mask & ~held.cpu()      # recovery over the positions that were designed
    if details is not None:
        nan = torch.full((B, max_len), float("nan"))
        for key, v in (("logp", logp), ("entropy", entropy)):
            details[key] = torch.where(mask, frame.restore(v if layouts is None else v[0]).cpu(), nan)
        details["score"] = torch.where(free, -details["logp"], torch.zeros(())).sum(dim=1) / free.sum(dim=1)
    ids, true_sequences, pred_sequences, recovery_rates = [], [], [], []
    for i in range(B):
        m = mask[i]
        f = free[i]
        recovery_rates.append(((pred_idx[i][f] == true_idx[i][f]).sum() / f.sum()).item())
        pred_sequences.append("".join(AA_VOCAB[j] for j in pred_idx[i][m]))
        true_sequences.append("".join(AA_VOCAB[j] for j in true_idx[i][m]))
        sid = batch.get("structure_ids")
        ids.append(f'{sid["pdb_id"][i]}_{sid["ligand_chain"][i]}' if sid is not None else str(i))
    print(sum(recovery_rates) / len(recovery_rates))
    return ids, true_sequences, pred_sequences, recovery_rates


def score_levels(T, levels=None):
    """The step indices ``score_sequences`` evaluates and the weight of their KL terms: ``levels=None`` -> every index
    0 .. T-1 and w = 1; ``levels=k`` -> {0} and the multiples k, 2k, .. below T, w = (T - 1) / (their number), so that
    w times their sum estimates the sum over all T - 1 indices s > 0 (w = 0 when there is none)."""
    k = 1 if levels is None else int(levels)
    if k < 1:
        raise ValueError(f"score_sequences: levels must be a positive stride, got {levels!r}")
    S = [0] + list(range(k, T, k))
    return S, ((T - 1) / (len(S) - 1) if len(S) > 1 else 0.0)


def sequence_indices(sequences, ligand_mask, num_classes=20):
    """Class indices int32 [B, L] of B strings over ``AA_VOCAB``, written to the valid positions of ``ligand_mask``
    [B, L] in order, -1 elsewhere.  A string of another length than its item's ligand, or a letter outside the
    vocabulary, raises ``ValueError``."""
    valid = ligand_mask.cpu() != 0
    B, L = valid.shape
    if isinstance(sequences, str) or len(sequences) != B:
        raise ValueError(f"score_sequences: sequences must be a list of {B} strings, one per item")
    letters = {a: i for i, a in enumerate(AA_VOCAB[:num_classes])}
    idx = torch.full((B, L), -1, dtype=torch.int32)
    for b, seq in enumerate(sequences):
        n = int(valid[b].sum())
        if not isinstance(seq, str) or len(seq) != n:
            raise ValueError(f"score_sequences: item {b} has a ligand of {n} residues, its sequence "
                             f"{len(seq) if isinstance(seq, str) else type(seq).__name__}")
        bad = sorted(set(seq) - set(letters))
        if bad:
            raise ValueError(f"score_sequences: item {b}: letters {''.join(bad)!r} are outside the vocabulary {''.join(letters)}")
        idx[b, valid[b]] = torch.tensor([letters[a] for a in seq], dtype=torch.int32)
    return idx


def prior_terms(q_top, x0):
    """float64 [B, L]: KL(q(z_T | x0) || uniform) = sum_c p[c] log(C p[c]) with p the normalised column x0 of the table
    at level 1 (``q_top`` [C, C]), 0 log 0 = 0; 0 where x0 < 0.  Host arithmetic."""
    q = q_top.detach().double().cpu()
    C = q.shape[0]
    p = q / q.sum(dim=0, keepdim=True)
    per_class = torch.where(p > 0, p * torch.log(C * p.clamp_min(1e-300)), torch.zeros((), dtype=torch.float64)).sum(dim=0)
    return torch.where(x0 >= 0, per_class[x0.clamp_min(0).long()], torch.zeros((), dtype=torch.float64))


@torch.no_grad()
def score_sequences(batch, model, noise_schedule, transition, sequences=None, *, levels=None, seed=None, item_ids=None,
                    us=None, generated_angles=None, score_mask=None, trim_padding=False, timesteps=None,
                    levels_per_launch=None, details=None):
    """How much the model likes given sequences: the variational score of the sampler's own reverse law, in nats per
    residue (lower: the model likes the sequence better -- the sense of ``denoise``'s ``details["score"]``, but for any
    sequence, on one scale).

    ``sequences``: B strings over ``AA_VOCAB``, item b's as long as its ligand; None scores the batch's own ``ligand_seq``.
    With the sampler's indexing -- step index s in 0 .. T-1 reads a state at level (s + 1) / T, feeds the model the
    timestep s and lands on level s / T -- an item with sequence x0 gets, per ligand position,

      * z_t ~ q(. | x0) at level (s + 1) / T, p[c] = Qtb[c][x0] (``apply_aa_noise``'s law; every position is noised);
      * logits = model.forward(s, onehot(z_t), ...), the call the sampler makes;
      * s > 0: term = KL(q_post(. | z_t, x0) || p_theta(. | z_t)), p_theta the normalised posterior the sampler draws
        from (``e3d_discrete_posterior_sample``'s prob_out, its zero rules included) and q_post the same expression with
        the x0 prediction replaced by the one-hot of x0; 0 log 0 = 0, and +inf (never NaN) where q_post > 0 meets
        p_theta == 0, which takes an fp32 softmax underflow (a logit gap above about 100);
        s == 0: term = -log_softmax(logits)[x0] (the chain's last step picks from the raw logits);
        at every level nll = -log_softmax(logits)[x0], the denoising cross-entropy;
      * prior = sum_c p[c] log(C p[c]), p the normalised column x0 of the table at level 1 (float64, on the host).

    Over a set S of step indices that contains 0, bound = prior + term_0 + w * sum_{s in S, s > 0} term_s summed over the
    scored positions, w = (T - 1) / |S \\ {0}|, and score = bound / (number of scored positions).  ``levels=None``: all T
    indices (w = 1, the sum is exact); ``levels=k``: {0} and k, 2k, ...  (``score_levels``).

    What this number is: zero exactly when the reverse law given the model's prediction equals the reverse law given
    the true residue, at every level drawn.  The posterior's one-step matrix is a row-normalised Qsb / Qtb (as in the
    reference sampler), not the forward process's own, so this is NOT a certified bound on a log-likelihood of the
    forward process.  No trained checkpoint ships with the tree: nothing about its ranking quality has been measured.

    Draws.  ``seed``: an int or a sequence of ints; each seed gives one keyed draw per (item, level, position) -- stream
    11, "the forward-noised copy of a known residue", at the step field s -- so an item's score depends on (seed,
    ``item_ids[b]``, its sequence, its inputs) alone; terms are averaged over the seeds and ``stderr`` is the standard
    error of ``score`` over them (NaN for one seed).  ``item_ids`` default to 0 .. B-1 and need a seed.  ``seed=None``:
    uniforms from torch's generator, or injected through ``us`` [S, B, L]; a seed and ``us`` together raise.

    Levels are folded into the batch: a launch scores ``levels_per_launch`` levels x B items as one padded batch with a
    per-item timestep (default: as many as keep it at about 64 items).  ``trim_padding`` runs the trimmed frame
    (packing.Frame); packed frames share one timestep and are not offered.  ``score_mask`` bool [B, L] names the
    positions that are summed (and-ed with the padding mask; an item with none gets a NaN score).  ``generated_angles``
    replace the ligand angles as in ``denoise``.

    Returns CPU tensors: ``bound``, ``score``, ``prior``, ``stderr`` float64 [B], ``n`` int32 [B], ``terms`` and ``nll``
    float64 [S, B] (summed over the scored positions with a fixed reduction shape, ``e3d_masked_item_sums``; mean over
    seeds), ``levels`` (the list S) and ``per_residue`` float64 [B, L], combined like ``bound``, NaN off the ligand.
    ``details``: a dict that receives ``z_t`` int32 [S, B, L] and ``logits`` [S, B, L, C] in the padded frame (one seed
    only)."""
    T = CONFIG["timesteps"] if timesteps is None else timesteps
    B, max_len, C = batch["ligand_seq"].shape
    if details is not None and not isinstance(details, dict):
        raise ValueError(f"score_sequences: details must be a dict to fill, got {type(details).__name__}")
    valid = batch["ligand_attn_mask"].cpu() != 0
    if sequences is None:
        x0 = torch.where(valid, onehot_to_index(batch["ligand_seq"].cpu()), torch.full((), -1, dtype=torch.int32))
    else:
        x0 = sequence_indices(sequences, batch["ligand_attn_mask"], C)
    if seed is None and item_ids is not None:
        raise ValueError("score_sequences: item_ids key the seeded draws; pass a seed with them")
    if seed is not None and us is not None:
        raise ValueError("score_sequences: pass either injected us or a seed, not both")
    seeds = [None]
    if seed is not None:
        seeds = [keyed.check_seed(v) for v in (seed if isinstance(seed, (list, tuple)) else [seed])]
        if not seeds:
            raise ValueError("score_sequences: an empty list of seeds")
        keyed.check_steps(T)
    if details is not None and len(seeds) > 1:
        raise ValueError("score_sequences: details hold the draws of one seed; pass a single seed with them")
    S, w = score_levels(T, levels)
    if us is not None and (not torch.is_tensor(us) or tuple(us.shape) != (len(S), B, max_len)):
        raise ValueError(f"score_sequences: us must be a tensor of {(len(S), B, max_len)}, one [B, L] per level")
    scored = valid & (x0 >= 0)
    if score_mask is not None:
        if not torch.is_tensor(score_mask) or score_mask.dtype != torch.bool or tuple(score_mask.shape) != (B, max_len):
            raise ValueError(f"score_sequences: score_mask must be a bool tensor of {(B, max_len)}")
        scored = scored & score_mask.cpu()
    chunk = max(1, 64 // B) if levels_per_launch is None else int(levels_per_launch)
    if chunk < 1:
        raise ValueError(f"score_sequences: levels_per_launch must be positive, got {levels_per_launch!r}")

    dev = next(model.parameters()).device
    ids = None if seed is None else keyed.item_ids(item_ids, B)
    ligand_mask = batch["ligand_attn_mask"].to(dev)
    receptor_mask = batch["receptor_attn_mask"].to(dev)
    frame = packing.Frame(ligand_mask, receptor_mask, trim=trim_padding)
    ang = frame.ligand((batch["ligand_angles"] if generated_angles is None else generated_angles).to(dev).float()).contiguous()
    rseq, rang = frame.pocket(batch["receptor_seq"].to(dev).float()), frame.pocket(batch["receptor_angles"].to(dev).float())
    lmask, rmask = frame.ligand(ligand_mask), frame.pocket(receptor_mask)
    x0_f = frame.ligand(x0.to(dev)).contiguous()
    keys = None if seed is None else frame.row_keys(ids, dev)
    scored_d = scored.to(dev).to(torch.uint8)
    if seed is None:
        us = torch.rand(len(S), B, max_len, device=dev) if us is None else us.to(dev).float()
        us = frame.ligand(us, dim=1)

    def launch(first, n, one_seed):
        """Levels S[first : first + n] x the B items as one batch of N = n B items, level-major."""
        steps = torch.tensor(S[first:first + n], device=dev, dtype=torch.long).repeat_interleave(B)
        s = steps.float().reshape(n * B, 1)
        qtb = transition.get_Qt_bar(noise_schedule.get_alpha_bar(t_normalized=(s + 1) / T), dev).contiguous()
        qsb = transition.get_Qt_bar(noise_schedule.get_alpha_bar(t_normalized=s / T), dev).contiguous()
        x0_n = x0_f.repeat(n, 1)
        if one_seed is None:
            z = ops.discrete_q_sample(x0_n, qtb, us[first:first + n].reshape(n * B, -1).contiguous())
        else:
            z = ops.keyed_discrete_forward_levels(x0_n, qtb, keys.repeat(n, 1), steps, one_seed, T - 1)
        logits = model.forward(s, F.one_hot(z.long(), num_classes=C).float(), ang.repeat(n, 1, 1), lmask.repeat(n, 1),
                               rseq.repeat(n, 1, 1), rang.repeat(n, 1, 1), rmask.repeat(n, 1)).contiguous().float()
        term, nll = ops.discrete_score_rows(z, x0_n, logits, qsb, qtb, (steps == 0).to(torch.uint8))
        # back to the padded frame, then the fixed-shape sums over the scored positions
        z, logits, term, nll = (frame.restore(t.reshape(n, B, *t.shape[1:]), dim=1) for t in (z, logits, term, nll))
        mask = scored_d.repeat(n, 1)
        sums = [ops.masked_item_sums(t.reshape(n * B, max_len).contiguous(), mask) for t in (term, nll)]
        return z, logits, term, sums[0][0].reshape(n, B), sums[1][0].reshape(n, B), sums[0][1][:B]

    per_seed = []
    for one_seed in seeds:
        parts = [launch(first, min(chunk, len(S) - first), one_seed) for first in range(0, len(S), chunk)]
        z, logits, term, term_sums, nll_sums = (torch.cat([p[i] for p in parts]) for i in range(5))
        per_seed.append((term.double().cpu(), term_sums.double().cpu(), nll_sums.double().cpu()))
        counts = parts[0][5].cpu()
        if details is not None:
            details["z_t"], details["logits"] = z.cpu(), logits.cpu()

    def combine(v):
        """term_0 + w * the sum of the other levels, of per-level values v [S, ..] (float64, on the host)."""
        return v[0] + (w * v[1:].sum(dim=0) if len(S) > 1 else 0.0)

    prior_pos = prior_terms(transition.get_Qt_bar(noise_schedule.get_alpha_bar(t_normalized=torch.ones(1, 1, device=dev)), dev)[0], x0)
    prior = torch.where(scored, prior_pos, torch.zeros((), dtype=torch.float64)).sum(dim=1)
    bound_seeds = torch.stack([prior + combine(ts) for _, ts, _ in per_seed])            # [seeds, B]
    n = counts.to(torch.int32)
    per_item = torch.where(n > 0, 1.0 / n.double().clamp_min(1), torch.full((), float("nan"), dtype=torch.float64))
    score_seeds = bound_seeds * per_item
    nan_b = torch.full((B,), float("nan"), dtype=torch.float64)
    stderr = score_seeds.std(dim=0, unbiased=True) / len(seeds) ** 0.5 if len(seeds) > 1 else nan_b
    per_residue = prior_pos + combine(torch.stack([t for t, _, _ in per_seed]).mean(dim=0))
    return {"bound": bound_seeds.mean(dim=0), "score": score_seeds.mean(dim=0), "prior": prior, "n": n, "stderr": stderr,
            "terms": torch.stack([ts for _, ts, _ in per_seed]).mean(dim=0),
            "nll": torch.stack([ns for _, _, ns in per_seed]).mean(dim=0), "levels": list(S),
            "per_residue": torch.where(valid, per_residue, torch.full((), float("nan"), dtype=torch.float64))}


def batch_keep_mask(keep, batch, first_index):
    """``known_mask`` [B, L] of a loader batch whose first item has dataset index ``first_index`` (packing.keep_mask per
    item, cut at the ligand's length); None when ``keep`` names nothing."""
    if not (callable(keep) or keep):
        return None
    B, L = batch["ligand_seq"].shape[:2]
    lengths = batch["ligand_attn_mask"].sum(dim=1).int().tolist()
    return torch.stack([packing.keep_mask(keep, first_index + b, L, lengths[b]) for b in range(B)])


def batch_controls(batch, first_index, temperature=None, omit=None, allow=None):
    """The design.DesignControls of a loader batch whose first item has dataset index ``first_index``; an argument left
    None takes the module's default (``TEMPERATURE`` / ``OMIT`` / ``ALLOW``, the E3D_SAMPLE_* variables).  None when
    nothing is set, so that the chain runs the launches it always ran."""
    temperature = TEMPERATURE if temperature is None else temperature
    omit = OMIT if omit is None else omit
    allow = ALLOW if allow is None else allow
    if temperature is None and not omit and not (callable(allow) or allow):
        return None
    from ..design import DesignControls
    controls = DesignControls.build(batch, temperature=1.0 if temperature is None else temperature, omit=omit,
                                    allow=allow if (callable(allow) or allow) else None, first_index=first_index)
    return controls if controls.active else None


def run(transition, diverse=True, seed=None, keep=None, temperature=None, omit=None, allow=None, scores=False):
    """Sample every test ligand.  ``seed`` (default ``SEED``, E3D_SAMPLE_SEED): keyed draws by dataset index.
    ``keep`` (default ``KEEP``, E3D_SAMPLE_KEEP): partial redesign -- a position list such as "0-3,7" or a callable
    dataset index -> bool [L] (packing.keep_mask); those residues are held at the record's own ``ligand_seq``.
    Design controls (design.DesignControls; ``denoise``): ``temperature`` (E3D_SAMPLE_TEMPERATURE), ``omit`` -- residue
    letters forbidden everywhere (E3D_SAMPLE_OMIT) -- and ``allow`` -- "3:LIV;7:DE", a dict or a callable dataset index ->
    dict (E3D_SAMPLE_ALLOW).  ``scores``: the table gets a ``score`` column, the mean of -log p of the picked residues
    over a ligand's designed positions (lower: the model likes the design better); without it the table is as before."""
    import pandas as pd
    seed = SEED if seed is None else seed
    keep = KEEP if keep is None else keep
    loader = get_dataloader(DATA_PATH)
    model = get_model(len(loader))
    schedule = PredefinedNoiseScheduleDiscrete(CONFIG["noise_schedule"], CONFIG["timesteps"]).to(DEVICE)
    cols = ([], [], [], [])
    score = []
    for idx, batch in enumerate(loader):
        print(f"Generating Batch {idx}")
        n = batch["ligand_seq"].shape[0]
        first = idx * CONFIG["batch_size"]
        ids = None if seed is None else list(range(first, first + n))
        known_mask = batch_keep_mask(keep, batch, first)
        design = {}
        controls = batch_controls(batch, first, temperature, omit, allow)
        if controls is not None:
            design["controls"] = controls
        if scores:
            design["details"] = {}
        for acc, part in zip(cols, denoise(batch, model, schedule, transition, diverse, pack=PACK, seed=seed,
                                           item_ids=ids, known_mask=known_mask, **design)):
            acc.extend(part)
        if scores:
            score.extend(design["details"]["score"].tolist())
    res = pd.DataFrame(zip(*cols), columns=["structure_ids", "true_sequence", "predict_sequence", "recovery_rate"])
    if scores:
        res["score"] = score
    res.to_pickle(OUTPUT_PATH)
    print(res)
    return res


if __name__ == "__main__":
    torch.cuda.set_device(GPU_ID)
    torch.set_num_threads(THREAD_NUM)
    run(BlosumTransition(x_classes=20), diverse=True)
