"""Reverse (ancestral) sampler of the structure model -- entry point and function names of the
reference's structure_model/sample.py, restructured for the device:

  * the pocket encoder and the decoder's cross K/V run ONCE per batch (they do not depend on the
    timestep; the reference recomputes them every step, sample.py:86-89);
  * the schedule tables are built once (the reference recomputes them every step, sample.py:74);
  * update + wrap is one HIP kernel (``e3d_ddpm_step_wrap``) and the trajectory stays in HBM
    until the loop ends (the reference does a blocking D2H copy per step, sample.py:143).

Beyond the reference: ``update="strided"`` (``UPDATE``) visits every STEP-th timestep with the schedule-consistent
DDIM / respaced-ancestral update of Song et al. 2021 (``e3d_strided_step_wrap``, ``utils.StridedTables``) instead of
applying one-step coefficients to a STEP-wide jump, and ``update="multistep"`` visits the same timesteps with the
second-order multistep update DPM-Solver++(2M) of Lu et al. 2022 (``e3d_multistep_step_wrap``, ``utils.MultistepTables``):
the same one decoder forward per step, the previous step's x0 estimate kept in a history buffer, no random numbers.

Run as ``python sample.py`` from this directory after editing the constants, like the reference.
"""
if __package__ in (None, ""):  # executed as a script from inside this directory
    import os as _os, sys as _sys
    _sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))))
    import __graft_entry__ as _g
    _g.load_package()
    __package__ = "e3diff_amd.structure_model"

import math
import os
import pickle
import warnings
from dataclasses import dataclass

import torch
from torch import nn

from .. import keyed, ops, packing
from ..bert import BertConfig
from ..packing import trimmed_length  # noqa: F401  (S.trimmed_length: bench.py and the tests read it here)
from .dataset import SPLIT_FILE, LigandBindingSiteDataset, NoisedAnglesDataset
from .model import ConditionalBertForDiffusion, ReceptorCache
from .utils import CosineTables, KnownLevels, MultistepTables, ScoreTables, StridedTables

MODEL_PATH = ""  # trained state_dict (same key names as the reference's checkpoints)
OUTPUT = "./data/output.pkl"
DATA_FILE = "./data/biolip.pt"
GPU_ID = 0
STEP = 1  # stride over timesteps; >1 trades quality for speed (reference sample.py:16)
# Arithmetic of this entry point.  The reference's structure_model/sample.py never calls
# torch.set_float32_matmul_precision (only the train scripts and the sequence sampler set "medium"), i.e. it
# samples at full fp32: ``sample()`` runs the fp32-grade f16x3 kernels (two fp16 terms per operand, see ops.py; 4.9e-6
# from the CPU oracle end to end vs 3.2e-6 for the exact fp32 MFMA path) unless E3D_GEMM_MODE says otherwise.
ARITHMETIC = "f16x3"
# Update rule of the chain.  "ancestral": the reference's one-step DDPM update at every visited timestep, whatever STEP is.
# "strided" (E3D_SAMPLE_UPDATE=strided): the generalised DDIM / respaced-ancestral jump from each visited timestep straight
# to the next one (Song et al. 2021, eqs. 12 and 16; utils.StridedTables) -- the update that is consistent with the
# schedule when STEP > 1.  ETA (E3D_SAMPLE_ETA) in [0, 1]: 0 = deterministic DDIM (no draws at all), 1 = the ancestral
# variance of the respaced chain.  WRAP_X0 (E3D_SAMPLE_WRAP_X0=1): wrap the x0 estimate to [-pi, pi), the angle analogue
# of clip_denoised -- 1/sqrt(ab_t) reaches 6.4e4 at t = 999 of the cosine schedule.  Sample quality under striding has
# not been measured here (no trained checkpoint ships with the tree): tools/evaluate_samples.py measures it.
# "multistep" (E3D_SAMPLE_UPDATE=multistep): the second-order multistep jump between the same visited timesteps
# (DPM-Solver++ 2M with a capped weight; utils.MultistepTables) -- DDIM's cost per step and no draws; ETA must stay 0,
# WRAP_X0 applies.  Its sample quality is unmeasured too; its solver error on an exactly solvable model is in DESIGN.md.
UPDATE = os.environ.get("E3D_SAMPLE_UPDATE", "ancestral")
ETA = float(os.environ.get("E3D_SAMPLE_ETA", "0"))
WRAP_X0 = os.environ.get("E3D_SAMPLE_WRAP_X0", "0") == "1"
# Packed chains (p_sample_loop(pack=True)): the batch runs on its valid rows only; off by default, E3D_SAMPLE_PACK=1 turns
# it on for ``sample()``.
PACK = os.environ.get("E3D_SAMPLE_PACK", "0") == "1"
# Keyed draws (``sample(seed=...)``): every random number of a pocket's chain is a function of (seed, dataset index), so
# batch size, order, frame and launch mode do not change its sample.  None (default): torch's generator, as before.
SEED = int(os.environ["E3D_SAMPLE_SEED"], 0) if os.environ.get("E3D_SAMPLE_SEED") else None
# Partial redesign (``sample(keep=...)``, E3D_SAMPLE_KEEP): ligand positions held at the record's own angles while the
# rest is sampled, e.g. "0-3,7" (0-based, inclusive ranges, applied to every ligand; packing.keep_mask).  "" (default):
# the whole peptide is designed, as before.
KEEP = os.environ.get("E3D_SAMPLE_KEEP", "")

CONFIG = {
    "pocket_ext": 0,
    "timesteps": 1000,
    "max_seq_len": 64,

    "num_heads": 12,
    "dropout_p": 0.1,
    "hidden_size": 768,
    "num_hidden_layers": 12,
    "intermediate_size": 1024,
    "position_embedding_type": "relative_key",

    "lr": 5e-5,
    "l2_norm": 0.1,
    "loss": "smooth_l1",
    "gradient_clip": 1.0,
    "lr_scheduler": "LinearWarmup",

    "min_epochs": 500,
    "max_epochs": 1000,
    "batch_size": 64,
}

DEVICE = f"cuda:{GPU_ID}"


def _tables(betas):
    return betas if isinstance(betas, CosineTables) else CosineTables.from_betas(betas.detach().cpu().float())


@torch.no_grad()
def p_sample(model, ligand_mask, ligand_angle_noise, receptor_seq, receptor_mask, receptor_angle,
             timestep, betas, noise=None, receptor_cache=None, out=None, wrap=False, seed=None,
             item_ids=None, strided=None, wrap_x0=False, known=None, known_mask=None, known_noise=None,
             known_levels=None, known_scale=1.0, multistep=None, history=None) -> torch.Tensor:
    """One reverse step x_t -> x_{t-1} (reference sample.py:55-99).  Like the reference's
    p_sample the result is NOT wrapped unless ``wrap=True`` (p_sample_loop's sample.py:140-142
    fused into the same kernel).

    ``timestep``: int64 [B] with one distinct value (asserted, as in the reference) or an int.
    ``betas``: the schedule betas [T] (any device) or a prebuilt CosineTables.
    ``noise``: optional injected N(0,1) draw (parity tests); default torch.randn_like on device.
    ``seed``: draw the noise from the keyed stream of (seed, item_ids[b], position) instead (``item_ids`` default
    0 .. B-1; see keyed.py); exclusive with ``noise``.
    ``strided``: a StridedTables -- the step goes from ``timestep`` straight to its successor in that table's order with
    the DDIM / respaced update (``wrap_x0``: wrap the x0 estimate); eta == 0 draws nothing.
    ``multistep``: a MultistepTables -- the same jump with the second-order multistep update (``wrap_x0`` as above; no
    draws; exclusive with ``strided``).  ``history`` [B,L,F] on the device: the x0 estimate the previous step of the chain
    stored, overwritten in place with this step's; the first and the last visited timestep do not read it.
    ``known`` [B,L,F] + ``known_mask`` (bool [B,L] or [B,L,F]) + ``known_levels`` (a KnownLevels of the chain's order):
    the held positions of the result are overwritten with the forward-noised copy of ``known`` at the level the step lands
    on (``p_sample_loop``, "partial redesign"); ``known_noise`` injects its N(0,1) draw, a ``seed`` keys it (stream 10).
    """
    x = ligand_angle_noise
    x0, m8, kn = _known_chain(known, known_mask, known_noise, seed, ligand_mask, x, None, "p_sample")
    row_keys = None
    if seed is not None:
        if noise is not None:
            raise ValueError("p_sample: pass either an injected noise or a seed, not both")
        row_keys = keyed.padded_keys(keyed.item_ids(item_ids, x.shape[0]), x.shape[1], x.device)
    elif item_ids is not None:
        raise ValueError("p_sample: item_ids key the seeded draws; pass a seed with them")
    plan = step_plan(betas, x.device, strided=strided, wrap_x0=wrap_x0, row_keys=row_keys, seed=seed, known=x0,
                     known_mask=m8, known_levels=known_levels, known_scale=known_scale, multistep=multistep)
    if (multistep is None) != (history is None):
        raise ValueError("p_sample: multistep=MultistepTables(...) and history (the previous x0 estimate) go together")
    return _reverse_step(model, ligand_mask, x, receptor_seq, receptor_mask, receptor_angle, timestep, betas, noise,
                         receptor_cache, out, wrap=wrap, plan=plan, known_noise=kn, history=history)


def _known_chain(known, known_mask, known_noises, seed, ligand_mask, x, steps, who):
    """The held positions of a chain, checked, in the padded frame: known float [B,L,F], mask uint8 [B,L,F] -- and-ed with
    the padding mask --, injected noises or None; three Nones when nothing is held: the chain runs as without them."""
    if known is None and known_mask is None:
        if known_noises is not None:
            raise ValueError(f"{who}: known_noises are the draws of the held positions; pass known and known_mask")
        return None, None, None
    if known is None or known_mask is None:
        raise ValueError(f"{who}: known and known_mask go together")
    if known_noises is not None and seed is not None:
        raise ValueError(f"{who}: pass either injected known_noises or a seed, not both")
    if known_mask.dtype != torch.bool:
        raise ValueError(f"{who}: known_mask must be a bool tensor, got {known_mask.dtype}")
    shape = tuple(x.shape)
    if tuple(known.shape) != shape:
        raise ValueError(f"{who}: known must be {shape} like the state, got {tuple(known.shape)}")
    if tuple(known_mask.shape) not in (shape[:2], shape):
        raise ValueError(f"{who}: known_mask must be {shape[:2]} or {shape}, got {tuple(known_mask.shape)}")
    want = shape if steps is None else (steps,) + shape
    if known_noises is not None and tuple(known_noises.shape) != want:
        raise ValueError(f"{who}: known_noises must be {want}, got {tuple(known_noises.shape)}")
    dev = x.device
    m = known_mask.to(dev)
    m = (m if m.dim() == 3 else m[..., None]) & (ligand_mask.to(dev) != 0)[..., None]
    if not bool(m.any()):
        return None, None, None
    return (known.to(dev).float(), m.expand(shape).to(torch.uint8).contiguous(),
            None if known_noises is None else known_noises.to(dev).float())


@dataclass(frozen=True)
class StepPlan:
    """What one reverse step of a chain is, decided once per chain or ``p_sample`` call (``step_plan``): the update rule,
    the source of its draws and the held positions.  The eager step (``_reverse_step``) and the captured one
    (``GraphedReverseStep``) both run ``update`` then ``compose`` and choose nothing themselves.
    ``coef``: the device table the update reads by the step index -- [T,4] = (sqrt_recip_alpha, beta,
    sqrt_one_minus_alphas_cumprod, sigma), or ``strided.coef`` [T,8]; None where no launch of the plan reads one (the
    eager unkeyed ancestral step takes four scalars from ``tab``).  ``keyed`` = (row keys, seed): the draws are generated
    inside the kernels (keyed.py); None: noise tensors.  ``known_x0`` / ``known_mask`` (uint8) / ``known_levels`` (a
    KnownLevels; ``levels``: its table on the device) / ``known_scale``: the held positions; ``known_x0`` None: none.
    ``multistep``: a MultistepTables instead of ``strided`` (``coef``: its [T,8] table).  Its update reads and rewrites
    the chain's x0 history, which belongs to the chain and not to this record: ``update`` is handed it."""
    tab: CosineTables
    coef: torch.Tensor = None
    strided: StridedTables = None
    wrap_x0: bool = False
    keyed: tuple = None
    known_x0: torch.Tensor = None
    known_mask: torch.Tensor = None
    known_levels: KnownLevels = None
    levels: torch.Tensor = None
    known_scale: float = 1.0
    multistep: MultistepTables = None

    @property
    def order(self):
        """The timesteps a chain of this plan may visit, descending: the rows of its tables that are not NaN."""
        if self.multistep is not None:
            return self.multistep.order
        if self.strided is not None:
            return self.strided.order
        if self.known_levels is not None:
            return self.known_levels.order
        return range(self.tab.betas.shape[0] - 1, -1, -1)

    def update_draws(self, t_index):
        """Whether the update at ``t_index`` reads a noise tensor: not keyed, not t = 0 (ancestral), not a strided sigma of
        0, never the multistep update."""
        if self.keyed is not None or self.multistep is not None:
            return False
        if self.strided is not None:
            return float(self.strided.coef[t_index, 4]) != 0.0
        return t_index != 0

    def compose_draws(self, t_index):
        """Whether ``compose`` at ``t_index`` reads a noise tensor: held positions, not keyed, not the clean level."""
        return self.known_x0 is not None and self.keyed is None and float(self.known_levels.levels[t_index, 1]) != 0.0

    def update(self, x, eps_hat, t_dev, noise, out, wrap, t_index=None, history=None):
        """x_t -> x_{t-1} (``t_dev``: int64 on the device, the step index first).  With the host's ``t_index`` (eager) the
        draw is settled here -- none where ``update_draws`` says so, else ``noise`` or a fresh ``torch.randn_like`` -- and
        the unkeyed ancestral update is the scalar launch; without it (captured) ``noise`` is the graph's buffer or None.
        ``history``: the chain's x0 history, which a multistep plan reads and rewrites in place."""
        eps_hat = eps_hat.contiguous()
        if self.multistep is not None:    # t -> its successor in the table's order; no draws, keyed or not
            if history is None:
                raise ValueError("a multistep step needs the chain's history buffer (the previous x0 estimate)")
            return ops.multistep_step_wrap(x, eps_hat, history, self.coef, t_dev, wrap=wrap, wrap_x0=self.wrap_x0, out=out)
        if t_index is not None:
            noise = _eager_noise(x, noise, self.update_draws(t_index))
        if self.strided is not None:      # t -> its successor in the table's order
            if self.keyed is not None:
                return ops.keyed_strided_step_wrap(x, eps_hat, self.coef, t_dev, *self.keyed, wrap=wrap,
                                                   wrap_x0=self.wrap_x0, out=out)
            return ops.strided_step_wrap(x, eps_hat, noise, self.coef, t_dev, wrap=wrap, wrap_x0=self.wrap_x0, out=out)
        if self.keyed is not None:
            return ops.keyed_ddpm_step_wrap(x, eps_hat, self.coef, t_dev, *self.keyed, wrap=wrap, out=out)
        if t_index is None:
            return ops.ddpm_step_wrap_table(x, eps_hat, noise, self.coef, t_dev, wrap=wrap, out=out)
        sra, beta, s1m, sigma = (float(c[t_index]) for c in (self.tab.sqrt_recip_alphas, self.tab.betas,
                                                             self.tab.sqrt_one_minus_alphas_cumprod, self.tab.sigma))
        return ops.ddpm_step_wrap(x, eps_hat, noise, sra, beta, s1m, 0.0 if noise is None else sigma, wrap=wrap, out=out)

    def compose(self, x, t_dev, noise, t_index=None):
        """Overwrite the held positions of ``x`` (the update's result) in place with the forward-noised copy of
        ``known_x0`` at the level the step landed on; returns ``x``.  ``noise`` / ``t_index`` as for ``update``."""
        if self.known_x0 is None:
            return x
        if self.keyed is not None:
            return ops.keyed_known_compose_wrap(x, self.known_x0, self.known_mask, self.levels, t_dev, *self.keyed,
                                                self.known_scale)
        if t_index is not None:
            noise = _eager_noise(x, noise, self.compose_draws(t_index))
        return ops.known_compose_wrap(x, self.known_x0, self.known_mask, noise, self.levels, t_dev, self.known_scale)


def _eager_noise(x, noise, draws):
    """The noise tensor of an eager launch: None where the step draws nothing, else the injected one or a fresh draw."""
    if not draws:
        return None
    return torch.randn_like(x) if noise is None else noise.contiguous()


def step_plan(betas, dev=None, table=False, strided=None, wrap_x0=False, row_keys=None, seed=None, known=None,
              known_mask=None, known_levels=None, known_scale=1.0, multistep=None):
    """The StepPlan of a chain, checked.  ``betas``: the schedule betas or a CosineTables; ``dev``: where its tables go.
    ``table``: build the [T,4] table although the eager step would not read it (a GraphedReverseStep may run the plan); a
    keyed ancestral plan has it anyway, a strided one has its own.  ``strided``: a StridedTables (+ ``wrap_x0``);
    ``row_keys`` + ``seed``: keyed draws; ``known`` + ``known_mask`` (uint8; both like the state, in the chain's frame) +
    ``known_levels`` (a KnownLevels of the chain's order) + ``known_scale``: held positions.  ``multistep``: a
    MultistepTables (+ ``wrap_x0``) in the place of ``strided``, not next to it; a seed then keys the held positions alone."""
    tab = _tables(betas)
    if strided is not None and multistep is not None:
        raise ValueError("step_plan: strided and multistep are two update rules; pass one of them")
    if strided is None and multistep is None and wrap_x0:
        raise ValueError("step_plan: wrap_x0 belongs to the strided and multistep updates; pass strided=StridedTables(...) "
                         "or multistep=MultistepTables(...)")
    if strided is not None and not isinstance(strided, StridedTables):
        raise TypeError(f"step_plan: strided must be a StridedTables, got {type(strided).__name__}")
    if multistep is not None and not isinstance(multistep, MultistepTables):
        raise TypeError(f"step_plan: multistep must be a MultistepTables, got {type(multistep).__name__}")
    if (row_keys is None) != (seed is None):
        raise ValueError("step_plan: keyed draws need both row_keys and a seed")
    if known is not None and not isinstance(known_levels, KnownLevels):
        raise ValueError("step_plan: held positions need known_levels=KnownLevels(tables, order of the chain)")
    if seed is not None:
        keyed.check_steps(tab.betas.shape[0])
    coef = None
    if strided is not None or multistep is not None:
        coef = (strided or multistep).coef.contiguous().to(dev)
    elif table or seed is not None:
        coef = torch.stack([tab.sqrt_recip_alphas, tab.betas, tab.sqrt_one_minus_alphas_cumprod, tab.sigma],
                           dim=1).float().contiguous().to(dev)
    held = {} if known is None else dict(known_x0=known.contiguous(), known_mask=known_mask.contiguous(),
                                         known_levels=known_levels, levels=known_levels.levels.to(dev),
                                         known_scale=float(known_scale))
    return StepPlan(tab, coef, strided, bool(wrap_x0), None if seed is None else (row_keys, keyed.check_seed(seed)),
                    multistep=multistep, **held)


def keyed_x_T(seed, item_ids, L, n_ft=8, scale=1.0, device=None):
    """Keyed initial state [B, L, n_ft]: wrap_[-pi,pi)(scale * z) with z the stream-0 normals of (seed, item_ids[b], l)
    -- NoisedAnglesDataset.sample_noise's distribution, drawn per item instead of per batch."""
    device = DEVICE if device is None else device
    ids = keyed.item_ids(item_ids, len(item_ids))
    keys = keyed.padded_keys(ids, L, device)
    return ops.keyed_initial_angles(keys, seed, n_ft, scale).reshape(len(ids), L, n_ft)


def _reverse_step(model, ligand_mask, x_t, receptor_seq, receptor_mask, receptor_angle, timestep,
                  betas, noise, receptor_cache, out, wrap, mod=None, layout=None, plan=None, known_noise=None, history=None):
    """The eager reverse step: decode, ``plan.update``, ``plan.compose``.  ``plan`` None: the plain ancestral step from
    ``betas``.  ``noise`` / ``known_noise``: injected draws of the update / of the held positions.  ``history``: the
    chain's x0 history in the chain's frame (a multistep plan)."""
    plan = step_plan(betas) if plan is None else plan
    if isinstance(timestep, int):
        t_index = timestep
        timestep = t_dev = torch.full((x_t.shape[0],), t_index, device=x_t.device, dtype=torch.long)
    else:
        t_unique = torch.unique(timestep)
        assert len(t_unique) == 1, f"Got multiple values for t: {t_unique}"
        t_index = int(t_unique.item())
        t_dev = timestep.to(device=x_t.device, dtype=torch.long).contiguous()
    if receptor_cache is None:
        receptor_cache = model.encode_receptor(receptor_seq, receptor_angle, receptor_mask)
    eps_hat = model.decode(timestep, x_t, ligand_mask, receptor_cache, mod=mod, layout=layout)
    x = plan.update(x_t.contiguous().float(), eps_hat, t_dev, noise, out, wrap, t_index, history)
    return plan.compose(x, t_dev, known_noise, t_index)


class GraphedReverseStep:
    """One reverse step (decoder forward + ``StepPlan.update`` + ``StepPlan.compose``) captured once into a HIP graph and
    replayed per step.  Everything that varies between steps lives on the device: the step index (``self.t``, also the
    row of the plan's coefficient table that the update reads), the state ``self.x`` and the noise draw.  Results are
    bit-identical to the eager path for the same noise, or the same keys.  A keyed plan generates its draws inside the
    kernels from the step index and a strided one at eta == 0 draws nothing: no noise buffer.  Held positions add one
    launch after the update, on the same stream and on ``self.out``, and, unseeded, a second noise buffer filled inside
    the graph; the captured step stays one serial chain.  A multistep plan has no noise buffer either; its x0 history
    (``self.history``) is owned here, lives across replays and is updated in place inside the graph.  It starts as NaN
    and the warm-up leaves an estimate of no chain in it: the first visited timestep of a chain does not read it.

    Default for chains of at most packing.GRAPH_MAX_ROWS token rows (up to ~16 pockets of 64 residues),
    ``use_graph=True`` / E3D_SAMPLE_GRAPH=1 forces it, =0 turns it off.  Measured on MI355X, one 64-residue pocket
    (tools/bench_single.py), with the K-sliced small-M GEMMs of ~7 us per product (csrc/gemm_skinny.hip): eager launches
    are host-bound at 2.4 ms per step, a replay takes 1.5 ms."""

    def __init__(self, model, ligand_mask, cache, tab, x_like, wrap=True, draw=True, mod_table=None, layout=None,
                 row_keys=None, seed=None, strided=None, wrap_x0=False, known=None, multistep=None):
        """``tab``: the chain's StepPlan (``step_plan(..., table=True)``: the other plan arguments are then not read), or
        its schedule -- the plan is then built here from ``row_keys`` + ``seed``, ``strided`` or ``multistep`` (+
        ``wrap_x0``) and ``known`` = (x0, uint8 mask -- both like ``x_like`` --, KnownLevels, scale), as ``step_plan`` takes them.
        ``draw``: the graph draws its own N(0,1) noise each replay; False: ``step`` takes the draws (parity tests) -- the
        update's and, with held positions, theirs next to it.  A keyed plan draws inside its kernels and needs ``draw``.
        ``mod_table`` [T,6H]: row t = model.timestep_modulation(t), read on the device by the step index.
        ``layout``: the step runs on packed ligand rows (``x_like`` [rows,F]; a packed ``cache``); its segment and tile
        tables are device tensors fixed for the chain, so the capture holds them like any other argument."""
        dev = x_like.device
        plan = tab if isinstance(tab, StepPlan) else step_plan(tab, dev, True, strided, wrap_x0, row_keys, seed,
                                                               *(known or (None, None, None, 1.0)), multistep=multistep)
        if plan.keyed is not None and not draw:
            raise ValueError("a keyed graph draws its own noise")
        if plan.coef is None:
            raise ValueError("a captured step reads its coefficients from the plan's table: step_plan(..., table=True)")
        self.model, self.mask, self.cache, self.plan, self.wrap = model, ligand_mask, cache, plan, wrap
        self.mod_table, self.layout, self.draw = mod_table, layout, draw
        self.x, self.out = x_like.clone(), torch.empty_like(x_like)
        # a noise buffer only where some step of the chain reads one (none: keyed draws, or strided at eta == 0)
        self.noise = torch.zeros_like(x_like) if any(map(plan.update_draws, plan.order)) else None
        self.known_noise = torch.zeros_like(x_like) if any(map(plan.compose_draws, plan.order)) else None
        self.history = torch.full_like(x_like, float("nan")) if plan.multistep is not None else None
        # a valid row for the warm-up and the capture (unvisited rows of a strided or level table are NaN)
        self.t = torch.full((x_like.shape[0],), plan.order[-1], device=dev, dtype=torch.long)
        # The warm-up step draws from torch's generator and its state is not put back (the sequence sampler's
        # GraphedDenoiseStep does put it back): a self-drawing chain starts one step's draws further on when replayed.
        self.graph, _ = packing.warm_up_and_capture(self._body, dev)

    def _body(self):
        mod = None if self.mod_table is None else self.mod_table.index_select(0, self.t[:1])
        eps_hat = self.model.decode(self.t, self.x, self.mask, self.cache, mod=mod, layout=self.layout)
        if self.draw and self.noise is not None:
            self.noise.normal_()
        self.plan.update(self.x, eps_hat, self.t, self.noise, self.out, self.wrap, history=self.history)
        if self.draw and self.known_noise is not None:
            self.known_noise.normal_()
        self.plan.compose(self.out, self.t, self.known_noise)

    def step(self, i, x, noise=None, known_noise=None):
        """x_t -> x_{t-1} for step index i; returns the graph's output buffer (overwritten by the next call)."""
        if (noise is not None) == self.draw:
            raise ValueError("this graph was captured %s injected noise" % ("without" if self.draw else "with"))
        if known_noise is not None:
            if self.known_noise is None or self.draw:
                raise ValueError("this graph takes no injected draw for held positions")
            self.known_noise.copy_(known_noise)
        elif self.known_noise is not None and not self.draw:
            raise ValueError("this graph was captured with injected noise: pass the held positions' draw too")
        self.t.fill_(i)
        if x is not self.x:
            self.x.copy_(x)
        if noise is not None and self.noise is not None:      # a strided graph at eta == 0 has no noise term
            self.noise.copy_(noise)
        self.graph.replay()
        return self.out


@torch.no_grad()
def p_sample_loop(model: nn.Module, ligand_mask, ligand_angle_noise, receptor_seq, receptor_mask,
                  receptor_angle, total_timesteps: int, betas, disable_pbar: bool = False,
                  noises=None, return_device: bool = False, step: int = None, use_graph: bool = None,
                  trim_padding: bool = False, pack: bool = False, seed: int = None, item_ids=None,
                  update: str = "ancestral", eta: float = 0.0, wrap_x0: bool = False, known=None, known_mask=None,
                  known_noises=None, known_scale: float = 1.0) -> torch.Tensor:
    """Full reverse chain; returns [T/STEP, B, L, n_ft] (on the host like the reference,
    sample.py:101-144, unless ``return_device``).  ``noises`` [T/STEP,B,L,n_ft] injects the draws.
    ``use_graph``: replay one captured HIP graph per step (None: by size, E3D_SAMPLE_GRAPH=0/1 overrides -- see
    GraphedReverseStep); falls back to eager launches if the capture fails.

    ``trim_padding=True``: the chain runs on the rows up to the longest ligand / pocket (packing.Frame); the rows it
    drops come back as 0 (the reference's values there are never used: its sample.py:243 slices them off).

    ``pack=True``: the chain runs on the packed valid rows of the batch -- ligand and pocket (packing.PackedLayout,
    varlen attention) -- so its cost follows the residues the items have instead of the longest item.  Valid positions
    agree with the padded and trimmed chains to fp32 rounding; every padding position comes back as 0, in the same
    [T/STEP, B, L, n_ft] shape.  Injected ``noises`` (padded layout) are gathered to the packed rows; default draws are
    made for the packed rows, i.e. they come from a different place in the random stream than the padded chain's.
    Masks that are not prefix masks cannot be packed: the chain then runs the trimmed frame (with a warning).  An item
    with ligand rows but an empty pocket raises ``ValueError``.  The agreement holds while every softmax row's scores
    spread over less than ~9900 (packing.Frame): beyond that the reference's additive -10000 mask lets padded keys win
    rows, and the packed path computes the absent-keys softmax instead (tests/test_varlen_forms_gpu.py::
    test_packed_path_computes_the_absent_keys_softmax_where_the_reference_lets_padded_keys_win).

    ``seed``: keyed draws (keyed.py, DESIGN.md "Keyed sampling streams"): the noise of step i at position l of item b is
    a function of (seed, item_ids[b], i, l) alone, generated inside the update kernel -- the same whatever the batch, its
    order, the frame (padded / trimmed / packed) or eager / graph launches.  ``item_ids`` default to 0 .. B-1; pass
    each pocket's own id (the entry point uses the dataset index).  Exclusive with ``noises``.  x_T stays the caller's
    (``keyed_x_T`` draws a keyed one).

    ``update``: "ancestral" (default) applies the reference's one-step DDPM update at every visited timestep, whatever
    ``step`` is.  "strided" jumps from each visited timestep straight to the next one with the DDIM / respaced-ancestral
    update (utils.StridedTables, ``e3d_strided_step_wrap``): ``eta`` in [0, 1] scales its noise (0: deterministic, no
    random number is drawn and torch's generator is left alone; 1: the ancestral variance of the respaced chain),
    ``wrap_x0`` wraps each step's x0 estimate to [-pi, pi).  The last entry, t = 0, is the wrapped x0 estimate.  Seeded
    strided chains draw the same stream-1 normals at timestep t as seeded ancestral ones.  ``eta`` / ``wrap_x0`` with
    the ancestral update raise.  "multistep" makes the same jumps with the second-order multistep update DPM-Solver++(2M)
    (Lu et al. 2022; utils.MultistepTables, ``e3d_multistep_step_wrap``): DDIM's update with the x0 estimate extrapolated
    from the previous step's, which the chain keeps in a history buffer in its own frame (a captured step owns one that
    lives across replays).  The extrapolation weight is capped at 0.5, a deliberate difference from the paper (see
    MultistepTables).  One decoder forward per step, no random number drawn, torch's generator left alone; ``wrap_x0`` as
    for "strided"; an ``eta`` other than 0 raises.  The first entry equals that of "strided" at eta = 0, and a chain with
    one visited timestep is the x0 estimate.  Under a ``seed`` only the held positions draw (stream 10).  On a model whose
    probability-flow ODE has a closed form its end point is 2.3x to 134x closer to the exact one than DDIM's at 10 to 50
    steps; sample quality has not been measured (no trained checkpoint ships with the tree).

    Partial redesign -- ``known`` [B, L, n_ft] + ``known_mask`` (bool [B, L]: whole residues, or [B, L, n_ft]: per
    element, e.g. hold a residue's dihedrals and free its bond angles): the masked ligand positions are held at ``known``
    while the rest is sampled (replacement conditioning: Song et al. 2021, section I.2; Lugmayr et al. 2022).  After every
    step the held elements are overwritten with a fresh forward-noised copy of ``known`` at the level the step landed on --
    wrap(sqrt(ab_s) known + sqrt(1 - ab_s) wrap(known_scale z)), the law the model was trained on (``known_scale``: the
    dataset's ``angular_var_scale``) -- and after the last step with ``known`` itself, by ``e3d_known_compose_wrap``
    (utils.KnownLevels), a launch of its own after the update; the decoder reads the held content through
    self-attention.  Every entry of the result is the composed state and the last one holds ``known`` bit for bit; x_T
    stays the caller's.  The mask is and-ed with ``ligand_mask``.  Works with either update, any ``step``, every frame,
    eager or graph.  ``known_noises`` [T/STEP, B, L, n_ft] injects the N(0,1) draws z (with ``noises``); with a ``seed``
    they are keyed stream 10 at the step's index, and streams 0 / 1 -- the free positions' draws -- are untouched.  A mask
    with nothing set runs the chain exactly as without these arguments.  There is no resampling loop (RePaint's jumps
    back), and sample quality has not been measured here (no trained checkpoint ships with the tree)."""
    if update not in ("ancestral", "strided", "multistep"):
        raise ValueError(f"p_sample_loop: update must be 'ancestral', 'strided' or 'multistep', got {update!r}")
    if update == "ancestral" and (eta != 0.0 or wrap_x0):
        raise ValueError("p_sample_loop: eta belongs to update='strided', wrap_x0 to 'strided' or 'multistep'")
    if update == "multistep" and eta != 0.0:
        raise ValueError("p_sample_loop: update='multistep' draws nothing; eta belongs to update='strided'")
    step = STEP if step is None else step
    tab = _tables(betas)
    order = list(reversed(range(0, total_timesteps, step)))
    strided = StridedTables(tab, order, eta) if update == "strided" else None
    multistep = MultistepTables(tab, order) if update == "multistep" else None
    x = ligand_angle_noise.contiguous().float()
    x0, m8, known_noises = _known_chain(known, known_mask, known_noises, seed, ligand_mask, x, len(order), "p_sample_loop")
    if x0 is not None and (noises is None) != (known_noises is None) and seed is None:
        raise ValueError("p_sample_loop: inject noises and known_noises together, or neither")
    if seed is not None and noises is not None:
        raise ValueError("p_sample_loop: pass either injected noises or a seed, not both")
    if seed is None and item_ids is not None:
        raise ValueError("p_sample_loop: item_ids key the seeded draws; pass a seed with them")
    ids = None if seed is None else keyed.item_ids(item_ids, x.shape[0])
    frame = packing.Frame(ligand_mask, receptor_mask, trim=trim_padding, pack=pack)
    layout, pocket_layout = frame.layouts or (None, None)
    if pocket_layout is None:
        cache = model.encode_receptor(frame.pocket(receptor_seq), frame.pocket(receptor_angle),
                                      frame.pocket(receptor_mask))
    else:   # packs the padded pocket itself
        cache = model.encode_receptor(receptor_seq, receptor_angle, receptor_mask, layout=pocket_layout)
    x = frame.ligand(x)
    mask = None if layout is not None else frame.ligand(ligand_mask).contiguous().float()   # a packed decode reads none
    if noises is not None:
        noises = frame.ligand(noises.to(x.device).float(), dim=1)
    if x0 is not None:         # into the frame like the state; packed tails and trimmed-off rows hold nothing
        x0, m8 = frame.ligand(x0), frame.ligand(m8)
        known_noises = None if known_noises is None else frame.ligand(known_noises, dim=1)
    plan = step_plan(tab, x.device, table=True, strided=strided, wrap_x0=wrap_x0,
                     row_keys=None if seed is None else frame.row_keys(ids, x.device), seed=seed, known=x0, known_mask=m8,
                     known_levels=None if x0 is None else KnownLevels(tab, order), known_scale=known_scale,
                     multistep=multistep)
    traj = torch.empty((len(order),) + tuple(x.shape), device=x.device, dtype=torch.float32)
    # what depends on the timestep alone, for the whole chain at once: row t of the table = timestep_modulation(t)
    mod_rows = model.timestep_modulation(torch.tensor(order, device=x.device, dtype=torch.long))
    mod_table = torch.zeros((total_timesteps, mod_rows.shape[1]), device=x.device, dtype=torch.float32)
    mod_table[order] = mod_rows
    graphed = packing.capture_graph(
        lambda: GraphedReverseStep(model, mask, cache, plan, x, draw=noises is None, mod_table=mod_table, layout=layout),
        frame.rows, len(order), use_graph)
    # the eager chain's x0 history, in the chain's frame (a captured step owns its own); NaN until the first step stores one
    history = torch.full_like(x, float("nan")) if multistep is not None and graphed is None else None
    for n, i in enumerate(order):
        kn = None if known_noises is None else known_noises[n].contiguous()
        if graphed is not None:
            x = graphed.step(i, graphed.out if n else x, None if noises is None else noises[n], kn)
            traj[n].copy_(x)
        else:
            x = _reverse_step(model, mask, x, None, None, None, i, tab, None if noises is None else noises[n], cache,
                              traj[n], wrap=True, mod=mod_table[i:i + 1], layout=layout, plan=plan, known_noise=kn,
                              history=history)
    traj = frame.restore(traj, dim=1)                                     # [T/STEP, B, L, F], zeros outside the frame
    return traj if return_device else traj.cpu()


def _tiled_cache(cache, n):
    """The pocket cache of a padded or trimmed frame repeated for n levels x B items, level-major: item i reads the rows of
    item i % B.  The cross K/V keep the bound their projection left on them (the content is the same)."""
    if n == 1:
        return cache

    def rep(t):
        out = t.repeat(n, 1)
        if hasattr(t, "_e3d_absmax"):
            out._e3d_absmax = t._e3d_absmax
        return out
    rows = packing.Rows.from_mask(cache.mask.repeat(n, 1), cache.rows.row_keys)
    return ReceptorCache(rep(cache.encoder_states), None if cache.cross_kv is None else [rep(kv) for kv in cache.cross_kv],
                         rows, n * cache.B, cache.L)


def structure_prior_terms(x0, prior_ab, scale):
    """float64, x0's shape: KL(q(x_T | x0) || N(0, scale^2)) per element with both laws read as Gaussians on the line,
    ((1 - ab) + ab x0^2 / scale^2 - 1 - ln(1 - ab)) / 2 at ab = ``prior_ab`` (the level timestep T - 1 reads).  Host
    arithmetic; practically 0 for the cosine schedule."""
    ab = float(prior_ab)
    x0 = x0.detach().double().cpu()
    return ((1.0 - ab) + ab * x0 * x0 / (float(scale) ** 2) - 1.0 - math.log(1.0 - ab)) / 2.0


@torch.no_grad()
def score_structures(model, ligand_mask, angles, receptor_seq, receptor_mask, receptor_angle, total_timesteps, betas, *,
                     levels=None, seed=None, item_ids=None, noises=None, scale=1.0, score_mask=None, trim_padding=False,
                     levels_per_launch=None, details=None):
    """How much the model likes given backbones: the variational score of the sampler's own reverse law for angles the
    chain did not sample, in nats per angle (lower: the model likes the backbone better), for any backbone of a pocket --
    replicates, natives, designs of other tools -- on one scale.

    ``angles`` [B, L, F]: the clean ligand angles x0, in the layout ``p_sample_loop`` returns; the other tensors are its
    arguments.  Indexing is the sampler's (``p_sample_loop``, stride 1, ``update="ancestral"``): timestep t in 0 .. T-1
    reads a state at level ab_t, applies mean = sra_t (x - beta_t eps_hat / s1m_t), adds sigma_t z (sigma_t^2 =
    ``CosineTables.posterior_variance[t]``, sigma_0 = 0), wraps to [-pi, pi) and lands on level t - 1 (level -1: the
    sample).  For an item and a timestep t, per element:

      * eps = wrap(scale z), z ~ N(0, 1), and x_t = wrap(sqrt_ab[t] x0 + s1m[t] eps): ``e3d_q_sample_wrap``'s arithmetic
        and ``NoisedAnglesDataset``'s law (``scale``: its ``angular_var_scale``); every position is noised, padding
        included, as in training;
      * eps_hat = model.decode(t, x_t, ligand mask, receptor cache), the call the sampler makes;
      * given the same x_t, the sampler's mean and the forward posterior's mean differ by k_t (eps_hat - eps), k_t =
        beta_t / (sqrt(alpha_t) s1m_t); states live on the circle, so delta = wrap(k_t (eps_hat - eps));
      * term = h_t delta^2 + add_t.  t > 0: h_t = 1 / (2 sigma_t^2), add_t = (scale^2 - 1) / 2 - ln(scale) (0 at scale 1):
        the KL of the two Gaussian reverse laws, in nats.  t == 0: the sampler returns the wrapped x0 estimate with no
        noise, and the term is the negative log-density of a Gaussian decoder of variance beta_0 around it (Ho et al.'s
        sigma^2 = beta choice for the last step): h_0 = 1 / (2 beta_0), add_0 = ln(2 pi beta_0) / 2, which is negative
        for small beta_0 -- a term and a bound may be negative: it is a density (``utils.ScoreTables``);
      * err = wrap(eps - eps_hat), the argument of every training loss; err^2 is reported at every level as ``eps_mse``,
        the counterpart of the sequence scorer's ``nll``.  It carries no schedule weight;
      * prior = ((1 - ab) + ab x0^2 / scale^2 - 1 - ln(1 - ab)) / 2 at ab = ab_{T-1} (float64, on the host; practically 0
        for the cosine schedule).

    Over a set S of timesteps that contains 0 (``sequence_model.sample.score_levels``: ``levels=None`` every timestep,
    ``levels=k`` {0} and k, 2k, ..), bound = prior + term_0 + w * sum_{t in S, t > 0} term_t over the scored elements, w =
    (T - 1) / |S \\ {0}|, and score = bound / (number of scored elements).

    What this number is not.  Wrapped normals are treated as Gaussians with the mean difference taken on the circle.  That
    is accurate while sigma_t << pi; at the top of the cosine schedule sigma_t reaches 0.99995 rad and k_t 99.98 (T =
    1000; both from ``CosineTables(1000).betas`` in float64), and there the term is an approximation, capped at pi^2 h_t.  The score is therefore NOT a certified likelihood
    bound.  No trained checkpoint ships with the tree: nothing about its ranking quality has been measured.

    Draws.  ``seed``: an int or a list of ints; each seed gives one keyed draw per (item, level, position, block of four
    features) -- stream 12 at the step field t (keyed.py) -- so an item's score depends on (seed, ``item_ids[b]``, its
    angles, its inputs) alone; terms are averaged over the seeds in float64 on the host and ``stderr`` is the standard
    error of ``score`` over them (NaN for one seed).  ``item_ids`` default to 0 .. B-1 and need a seed.  ``seed=None``:
    ``torch.randn`` on the device, or injected ``noises`` [S, B, L, F] (N(0, 1); scaled and wrapped as above, through
    ``ops.q_sample_wrap``); a seed and ``noises`` together raise.

    The pocket encoder runs once per call.  Levels are folded into the batch: a launch decodes ``levels_per_launch``
    levels x B items with a per-item timestep against the cache's rows tiled for it (default: as many levels as keep it at
    about 64 items).  ``trim_padding`` runs the trimmed frame (packing.Frame); packed frames share one timestep and are
    not offered.  ``score_mask`` bool [B, L] or [B, L, F] names what is summed (and-ed with the padding mask; an item
    with nothing scored gets a NaN score).

    Returns CPU tensors: ``bound``, ``score``, ``prior``, ``stderr`` float64 [B]; ``n`` int32 [B], the scored elements;
    ``terms`` and ``eps_mse`` float64 [S, B] (summed over the scored elements in a fixed reduction shape,
    ``e3d_angle_score_items``; mean over seeds; ``eps_mse`` is already divided by ``n``); ``levels`` (the list S);
    ``per_residue`` float64 [B, L], combined like ``bound`` (its prior included), NaN off the ligand; ``per_feature``
    float64 [B, F], combined like ``bound`` WITHOUT the prior, so bound = prior + per_feature.sum(1).  ``details``: a
    dict that receives ``x_t``, ``eps``, ``eps_hat`` [S, B, L, F] in the padded frame (one seed only)."""
    from ..sequence_model.sample import score_levels
    who = "score_structures"
    T = int(total_timesteps)
    if details is not None and not isinstance(details, dict):
        raise ValueError(f"{who}: details must be a dict to fill, got {type(details).__name__}")
    if not torch.is_tensor(angles) or angles.dim() != 3:
        raise ValueError(f"{who}: angles must be a [B, L, F] tensor")
    B, L, F = angles.shape
    if F % 4 or not 0 < F <= 32:
        raise ValueError(f"{who}: the feature count must be a multiple of 4 in [4, 32], got {F}")
    if not torch.is_tensor(ligand_mask) or tuple(ligand_mask.shape) != (B, L):
        raise ValueError(f"{who}: ligand_mask must be {(B, L)} like the angles")
    if not torch.is_tensor(receptor_mask) or receptor_mask.dim() != 2 or receptor_mask.shape[0] != B:
        raise ValueError(f"{who}: receptor_mask must be [{B}, Lr]")
    Lr = receptor_mask.shape[1]
    for name, t in (("receptor_seq", receptor_seq), ("receptor_angle", receptor_angle)):
        if not torch.is_tensor(t) or t.dim() != 3 or tuple(t.shape[:2]) != (B, Lr):
            raise ValueError(f"{who}: {name} must be [{B}, {Lr}, .] like the receptor mask")
    tab = _tables(betas)
    if tab.betas.shape[0] != T or T < 1:
        raise ValueError(f"{who}: {tab.betas.shape[0]} betas for total_timesteps={T}")
    if seed is None and item_ids is not None:
        raise ValueError(f"{who}: item_ids key the seeded draws; pass a seed with them")
    if seed is not None and noises is not None:
        raise ValueError(f"{who}: pass either injected noises or a seed, not both")
    seeds = [None]
    if seed is not None:
        seeds = [keyed.check_seed(v) for v in (seed if isinstance(seed, (list, tuple)) else [seed])]
        if not seeds:
            raise ValueError(f"{who}: an empty list of seeds")
        keyed.check_steps(T)
    if details is not None and len(seeds) > 1:
        raise ValueError(f"{who}: details hold the draws of one seed; pass a single seed with them")
    try:
        S, w = score_levels(T, levels)
    except ValueError:
        raise ValueError(f"{who}: levels must be a positive stride, got {levels!r}") from None
    if noises is not None and (not torch.is_tensor(noises) or tuple(noises.shape) != (len(S), B, L, F)):
        raise ValueError(f"{who}: noises must be a tensor of {(len(S), B, L, F)}, one [B, L, F] per level")
    valid = ligand_mask.cpu() != 0
    scored = valid[..., None].expand(B, L, F)
    if score_mask is not None:
        if not torch.is_tensor(score_mask) or score_mask.dtype != torch.bool or tuple(score_mask.shape) not in ((B, L), (B, L, F)):
            raise ValueError(f"{who}: score_mask must be a bool tensor of {(B, L)} or {(B, L, F)}")
        sm = score_mask.cpu()
        scored = scored & (sm if sm.dim() == 3 else sm[..., None])
    chunk = max(1, 64 // B) if levels_per_launch is None else int(levels_per_launch)
    if chunk < 1:
        raise ValueError(f"{who}: levels_per_launch must be positive, got {levels_per_launch!r}")
    tables = ScoreTables(tab, scale)            # a non-positive or non-finite scale raises here
    ids = None if seed is None else keyed.item_ids(item_ids, B)

    dev = next(model.parameters()).device
    ligand_mask, receptor_mask = ligand_mask.to(dev), receptor_mask.to(dev)
    frame = packing.Frame(ligand_mask, receptor_mask, trim=trim_padding)
    cache = model.encode_receptor(frame.pocket(receptor_seq.to(dev)), frame.pocket(receptor_angle.to(dev)),
                                  frame.pocket(receptor_mask))
    x0 = angles.to(dev).float().contiguous()
    x0_f = frame.ligand(x0).contiguous()
    lmask = frame.ligand(ligand_mask).contiguous().float()
    keys = None if seed is None else frame.row_keys(ids, dev)
    sa, s1m = tab.sqrt_alphas_cumprod.float().contiguous().to(dev), tab.sqrt_one_minus_alphas_cumprod.float().contiguous().to(dev)
    coef = tables.coef.to(dev)
    scored_d = scored.to(torch.uint8).contiguous().to(dev)
    if seed is None:
        z_all = torch.randn(len(S), B, L, F, device=dev) if noises is None else noises.to(dev).float()
        z_all = frame.ligand(z_all, dim=1).contiguous()
        zero_t, one_row = torch.zeros(1, device=dev), torch.full((1,), float(scale), device=dev)

    def launch(first, n, one_seed):
        """Timesteps S[first : first + n] x the B items as one batch of N = n B items, level-major."""
        steps = torch.tensor(S[first:first + n], device=dev, dtype=torch.long).repeat_interleave(B)
        if one_seed is None:
            z = z_all[first:first + n].reshape(n * B, -1).contiguous()
            # eps = wrap(0 * 0 + scale * z): the forward-noising kernel with a one-row table (0, scale)
            eps = ops.q_sample_wrap(torch.zeros_like(z), z, torch.zeros(n * B, device=dev, dtype=torch.long), zero_t, one_row)
            eps = eps.reshape(n * B, *x0_f.shape[1:])
            x_t = ops.q_sample_wrap(x0_f.repeat(n, 1, 1), eps, steps, sa, s1m)
        else:
            eps, x_t = ops.keyed_q_sample_levels_wrap(x0_f, keys, steps, sa, s1m, scale, one_seed, T - 1)
        eps_hat = model.decode(steps, x_t, lmask.repeat(n, 1), _tiled_cache(cache, n)).contiguous().float()
        # back to the padded frame, then the terms and their fixed-shape sums over the scored elements
        x_t, eps, eps_hat = (frame.restore(t.reshape(n, B, *t.shape[1:]), dim=1).reshape(n * B, L, F).contiguous()
                             for t in (x_t, eps, eps_hat))
        out = ops.angle_score_items(eps_hat, eps, scored_d, steps, coef)
        return (x_t, eps, eps_hat) + tuple(out[k].reshape(n, B, *out[k].shape[1:]) for k in
                                           ("res_term", "feat_term", "tot_term", "tot_err2")) + (out["counts"][:B],)

    per_seed = []
    for one_seed in seeds:
        parts = [launch(first, min(chunk, len(S) - first), one_seed) for first in range(0, len(S), chunk)]
        x_t, eps, eps_hat, res_term, feat_term, tot_term, tot_err2 = (torch.cat([p[i] for p in parts]) for i in range(7))
        per_seed.append(tuple(t.double().cpu() for t in (res_term, feat_term, tot_term, tot_err2)))
        counts = parts[0][7].cpu()
        if details is not None:
            details.update({k: v.reshape(len(S), B, L, F).cpu() for k, v in (("x_t", x_t), ("eps", eps), ("eps_hat", eps_hat))})

    def combine(v):
        """term_0 + w * the sum of the other levels, of per-level values v [S, ..] (float64, on the host)."""
        return v[0] + (w * v[1:].sum(dim=0) if len(S) > 1 else 0.0)

    def seed_mean(i):
        return torch.stack([p[i] for p in per_seed]).mean(dim=0)

    prior_el = torch.where(scored, structure_prior_terms(angles, tables.prior_ab, scale), torch.zeros((), dtype=torch.float64))
    prior = prior_el.sum(dim=(1, 2))
    bound_seeds = torch.stack([prior + combine(p[2]) for p in per_seed])                  # [seeds, B]
    n = counts.to(torch.int32)
    per_item = torch.where(n > 0, 1.0 / n.double().clamp_min(1), torch.full((), float("nan"), dtype=torch.float64))
    score_seeds = bound_seeds * per_item
    nan_b = torch.full((B,), float("nan"), dtype=torch.float64)
    stderr = score_seeds.std(dim=0, unbiased=True) / len(seeds) ** 0.5 if len(seeds) > 1 else nan_b
    per_residue = prior_el.sum(dim=2) + combine(seed_mean(0))
    return {"bound": bound_seeds.mean(dim=0), "score": score_seeds.mean(dim=0), "prior": prior, "n": n, "stderr": stderr,
            "terms": seed_mean(2), "eps_mse": seed_mean(3) * per_item, "levels": list(S),
            "per_residue": torch.where(valid, per_residue, torch.full((), float("nan"), dtype=torch.float64)),
            "per_feature": combine(seed_mean(1))}


def get_dataset(file_path):
    ds = LigandBindingSiteDataset(file_path, "test", CONFIG["max_seq_len"], CONFIG["pocket_ext"],
                                  split_file=SPLIT_FILE or None)   # E3D_SPLIT_FILE
    return NoisedAnglesDataset(ds, timesteps=CONFIG["timesteps"])


def build_configs(cfg=None):
    cfg = cfg or CONFIG
    common = dict(max_position_embeddings=cfg["max_seq_len"], num_attention_heads=cfg["num_heads"],
                  hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                  num_hidden_layers=cfg["num_hidden_layers"],
                  position_embedding_type=cfg["position_embedding_type"],
                  hidden_dropout_prob=cfg["dropout_p"], attention_probs_dropout_prob=cfg["dropout_p"],
                  use_cache=False)
    return BertConfig(**common), BertConfig(**common, is_decoder=True, add_cross_attention=True)


def load_model(dataset, model_path=None):
    encoder_config, decoder_config = build_configs()
    model = ConditionalBertForDiffusion(
        encoder_config=encoder_config, decoder_config=decoder_config,
        feature_names=dataset.feature_names, epochs=CONFIG["max_epochs"],
        lr_scheduler=CONFIG["lr_scheduler"], l2_lambda=CONFIG["l2_norm"],
        steps_per_epoch=len(dataset), learning_rate=CONFIG["lr"],
        loss_func=[ConditionalBertForDiffusion.diheral_loss_func] * 4
        + [ConditionalBertForDiffusion.angle_loss_func] * 4)
    path = MODEL_PATH if model_path is None else model_path
    if path:
        model.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
    return model.eval().to(DEVICE)


def sample(model, test_angle_ds, all_batches: bool = False, seed: int = None, keep=None):
    """Sample the test pockets in batches of CONFIG["batch_size"]; returns a list of
    [T, l_i, 8] arrays trimmed to each ligand's length.  Like the reference (sample.py:237) only
    the first batch is generated unless ``all_batches``.

    ``seed`` (default ``SEED``, E3D_SAMPLE_SEED): keyed draws for x_T and the chain, keyed by the dataset index, so a
    pocket's sample does not depend on the batch size, on its place in the batch, on packing or on an arithmetic
    re-run of its batch.  The chain's update rule comes from ``STEP``, ``UPDATE``, ``ETA`` and ``WRAP_X0``.

    ``keep`` (default ``KEEP``, E3D_SAMPLE_KEEP): partial redesign -- a position list such as "0-3,7" (0-based ligand
    positions, inclusive ranges, applied to every ligand; positions beyond a ligand's length are ignored) or a callable
    dataset index -> bool [L].  Those residues are held at the record's own clean ``ligand_angles`` while the rest is
    sampled (``p_sample_loop(known=...)``)."""
    seed = SEED if seed is None else seed
    keep = KEEP if keep is None else keep
    bs = CONFIG["batch_size"]
    items = [test_angle_ds[i] for i in range(len(test_angle_ds))]

    def chunk(name):
        return [torch.stack([it[name] for it in items[i:i + bs]]) for i in range(0, len(items), bs)]

    ligand_mask, receptor_angle = chunk("ligand_attn_mask"), chunk("receptor_angles")
    receptor_seq, receptor_mask = chunk("receptor_seq"), chunk("receptor_attn_mask")
    pad, feature_size = items[0]["ligand_angles"].shape
    retval = []
    for idx, lm in enumerate(ligand_mask):
        print(f"Generating Batch {idx}/{len(ligand_mask)}")
        lengths = lm.sum(dim=1).int()
        ids = list(range(idx * bs, idx * bs + len(lengths)))      # dataset indices of the batch
        held = {}
        if callable(keep) or keep:
            held = dict(known=torch.stack([items[i]["ligand_angles"] for i in ids]).float().to(DEVICE),
                        known_mask=torch.stack([packing.keep_mask(keep, i, pad, int(l)) for i, l in zip(ids, lengths)]).to(DEVICE),
                        known_scale=test_angle_ds.angular_var_scale)
        if seed is None:
            x_T = test_angle_ds.sample_noise(torch.zeros((len(lengths), pad, feature_size)))
        else:
            x_T = keyed_x_T(seed, ids, pad, feature_size, test_angle_ds.angular_var_scale, DEVICE)
        def chain(arithmetic):
            with ops.arithmetic(arithmetic):
                return p_sample_loop(
                    model=model, ligand_mask=lm.to(DEVICE), ligand_angle_noise=x_T.to(DEVICE),
                    receptor_seq=receptor_seq[idx].to(DEVICE), receptor_mask=receptor_mask[idx].to(DEVICE),
                    receptor_angle=receptor_angle[idx].to(DEVICE), total_timesteps=test_angle_ds.timesteps,
                    betas=test_angle_ds.alpha_beta_terms["betas"], trim_padding=True,   # sliced to l_i right below
                    pack=PACK, seed=seed, item_ids=None if seed is None else ids, step=STEP, update=UPDATE, eta=ETA,
                    wrap_x0=WRAP_X0, **held)

        sampled = chain(ARITHMETIC)
        if ops.GEMM_MODES.get(ARITHMETIC) == 19 and "E3D_GEMM_MODE" not in os.environ and not bool(torch.isfinite(sampled).all()):
            # f16x3's one remaining range limit: an ACTIVATION beyond 65504 (weights are pre-scaled) turns into inf / NaN.
            # The chain is then run again in bf16x6 -- same fp32 grade, fp32 exponent range, half the speed -- and says so
            warnings.warn("structure sampling: non-finite angles in f16x3 arithmetic (an activation left the fp16 range); "
                          "re-running this batch in bf16x6")
            sampled = chain("bf16x6")
        retval.extend(sampled[:, i, :l, :].numpy() for i, l in enumerate(lengths))
        if not all_batches:
            break
    return retval


if __name__ == "__main__":
    torch.cuda.set_device(GPU_ID)
    test_angle_dataset = get_dataset(DATA_FILE)
    model = load_model(test_angle_dataset)
    sample_result = sample(model, test_angle_dataset)
    with open(OUTPUT, "+wb") as f:
        pickle.dump(sample_result, f)
