"""Blocks shared by the structure and sequence denoisers (the reference duplicates them:
structure_model/model.py:27-154 == sequence_model/model.py:26-153).  Parameter containers keep
the reference attribute names (checkpoint keys); ``run`` methods execute on HIP kernels."""
import math

import torch
from torch import nn

import contextlib
import os

from . import bert, keyed, ops
from .autograd import functional as F
from .packing import Rows

# SELayer conditioning on one-hot rows (the pocket's residue types): modulation rows from a table of the distinct rows
# (``onehot_modulation``).  0 = always the dense [M, 6H] launches (A/B runs, tests).
ADALN_TABLE = os.environ.get("E3D_ADALN_TABLE", "1") == "1"
TABLE_ROWS = 256     # the canonical inputs are padded to one row block of the GEMM kernels
_CANONICAL_ROWS = {}


class IndexedModulation:
    """What ``onehot_modulation`` hands ``SELayer.run`` in the place of ``mod``: row r's modulation is ``table[idx[r]]``
    where idx[r] >= 0, ``mod[r]`` elsewhere (``mod`` holds rows only when the device found such a row and raised
    ``other_rows``, a one-int device word)."""

    def __init__(self, idx, table, mod, other_rows):
        self.idx, self.table, self.mod, self.other_rows = idx, table, mod, other_rows
        self.shape = mod.shape


def _canonical_rows(F_in, device):
    """[TABLE_ROWS, F]: the F one-hot rows, then zero rows (row F: the padding row of a pocket)."""
    key = (F_in, device)
    t = _CANONICAL_ROWS.get(key)
    if t is None:
        t = torch.zeros(TABLE_ROWS, F_in, device=device, dtype=torch.float32)
        t[:F_in] = torch.eye(F_in, device=device, dtype=torch.float32)
        _CANONICAL_ROWS[key] = t
    return t


def onehot_modulation(layer, emb, x2d):
    """``layer.modulation(emb.run(x2d))`` for per-token features x2d [M, F] that are one-hot or all-zero rows (a pocket's
    residue types: dataset._one_hot / _pad): such input has F + 1 distinct rows, so the embedding and both modulation GEMMs
    run on a table of those rows -- in the kernel form of the M-row launch, so a table row equals the row that launch would
    have written bit for bit -- and the gates look their row up.  The M-row launches stay in the sequence behind a device
    flag that a classification pass over x2d raises for any other row (soft labels, NaN): they then run as ever and such
    rows read their own modulation; with one-hot input they return at once.  No host synchronisation.
    Inference only; returns None where the path does not apply (the caller then runs the dense one)."""
    m0, m2 = layer.adaLN_modulation[0], layer.adaLN_modulation[2]
    M, F_in = x2d.shape
    H = m0.weight.shape[0]
    params = (emb.linear.weight, emb.linear.bias, emb.LayerNorm.weight, emb.LayerNorm.bias, m0.weight, m0.bias, m2.weight, m2.bias)
    if (not ADALN_TABLE or F_in >= TABLE_ROWS or F_in > 32 or not ops.gemm_is_tiled(M)
            or (emb.training and emb.dropout.p > 0)
            or (torch.is_grad_enabled() and any(t.requires_grad for t in params + (x2d,)))):
        return None
    ln = emb.LayerNorm
    idx, other_rows = ops.classify_onehot_rows(x2d)
    # (the embedding's two kernel forms, few rows and many, run the same arithmetic in the same order: no form to ask for)
    e = ops.embed_layernorm(_canonical_rows(F_in, x2d.device), emb.linear.weight, emb.linear.bias, ln.weight, ln.bias, ln.eps)
    table = ops.gemm(ops.gemm(e, m0.weight, m0.bias, ops.ACT_SILU, plan_m=M), m2.weight, m2.bias, plan_m=M)
    c = ops.embed_layernorm(x2d, emb.linear.weight, emb.linear.bias, ln.weight, ln.bias, ln.eps, run_if=other_rows)
    mod = ops.gemm(ops.gemm(c, m0.weight, m0.bias, ops.ACT_SILU, run_if=other_rows), m2.weight, m2.bias, run_if=other_rows)
    return IndexedModulation(idx, table, mod, other_rows)


class SELayer(nn.Module):
    """adaLN-gated attention + MLP block (structure_model/model.py:27-67)."""

    def __init__(self, bert_config, mlp_ratio=4.0):
        super().__init__()
        h = bert_config.hidden_size
        self.norm1 = nn.LayerNorm(h, elementwise_affine=False)
        self.norm2 = nn.LayerNorm(h, elementwise_affine=False)
        self.adaLN_modulation = nn.Sequential(nn.Linear(h, h, bias=True), nn.SiLU(),
                                              nn.Linear(h, 6 * h, bias=True))
        self.attn = bert.BertAttention(bert_config)
        self.mlp = nn.Sequential(nn.Linear(h, int(h * mlp_ratio)), nn.GELU(),
                                 nn.Dropout(bert_config.hidden_dropout_prob),
                                 nn.Linear(int(h * mlp_ratio), h),
                                 nn.Dropout(bert_config.hidden_dropout_prob))
        nn.init.zeros_(self.adaLN_modulation[0].weight)
        nn.init.zeros_(self.adaLN_modulation[0].bias)

    def modulation(self, c):
        """adaLN_modulation(c): [n,H] -> [n,6H] (shift, scale, gate of the attention branch, then of the MLP branch)."""
        m0, m2 = self.adaLN_modulation[0], self.adaLN_modulation[2]
        return F.linear(F.linear(c, m0.weight, m0.bias, ops.ACT_SILU), m2.weight, m2.bias)

    def run(self, x, c, rows, mod=None):
        """x [rows.rows,H] (``rows``: packing.Rows); c [rows.rows,H] (per token), [B,H] (one conditioning row per item of a
        padded frame) or ONE row shared by every item.  ``mod``: the rows ``modulation(c)`` would give, computed by the
        caller in one of those forms (one row [1,6H]: samplers precompute it per timestep), or an ``IndexedModulation``
        (per token); it takes the place of ``c``."""
        if mod is None:
            mod = self.modulation(c)
        rows_per_cond = x.shape[0] // mod.shape[0]
        assert rows_per_cond in (1, rows.L, rows.rows) and rows_per_cond * mod.shape[0] == x.shape[0], (x.shape, mod.shape)
        drop = bert.Drop.of(self.attn, rows)
        att = bert.run_self_attention(self.attn, x, rows, drop)
        if isinstance(mod, IndexedModulation):
            assert rows_per_cond == 1
            gate = lambda a, y, branch: ops.adaln_gate_indexed(a, y, mod.idx, mod.table, mod.mod, branch)   # noqa: E731
        else:
            gate = lambda a, y, branch: F.adaln_gate(a, y, mod, branch, rows_per_cond)   # noqa: E731
        x = gate(x, att, 0)
        h = F.dropout(F.linear(x, self.mlp[0].weight, self.mlp[0].bias, ops.ACT_GELU), self.mlp[2].p, self.training, drop.row_keys)
        h = F.dropout(F.linear(h, self.mlp[3].weight, self.mlp[3].bias), self.mlp[4].p, self.training, drop.row_keys)
        return gate(x, h, 1)


class GaussianFourierProjection(nn.Module):
    """structure_model/model.py:69-98.  Kept as three tiny torch device ops on purpose: with raw
    integer timesteps the sin/cos arguments reach ~1e5 rad, and the reference's op order
    (t*W, *2, *pi in fp32) fixes which fp32 argument is reduced."""

    def __init__(self, embed_dim=384, scale=2 * math.pi):
        super().__init__()
        self.register_buffer("W", torch.randn(embed_dim // 2) * scale)

    def forward(self, x):
        if x.ndim > 1:
            x = x.squeeze()
        elif x.ndim < 1:
            x = x.unsqueeze(0)
        if x.ndim < 1:
            x = x.unsqueeze(0)
        x_proj = x[:, None] * self.W[None, :] * 2 * torch.pi
        return torch.cat([torch.sin(x_proj), torch.cos(x_proj)], dim=-1)


class BertEmbeddings(nn.Module):
    """Linear -> LayerNorm -> dropout (structure_model/model.py:100-118)."""

    def __init__(self, in_features, bert_config):
        super().__init__()
        self.linear = nn.Linear(in_features, bert_config.hidden_size)
        self.LayerNorm = nn.LayerNorm(bert_config.hidden_size, eps=bert_config.layer_norm_eps)
        self.dropout = nn.Dropout(bert_config.hidden_dropout_prob)

    def run(self, x2d, rows, post_add=None, rows_per_add=1):
        """x2d [rows.rows, F] (``rows``: packing.Rows).  ``post_add`` [M / rows_per_add, H] is what the caller adds to the
        embedding afterwards (the sequence model's timestep term): fused into the kernel, except in training with
        dropout, which sits between."""
        if self.training and self.dropout.p > 0:
            e = F.embed_layernorm(x2d, self.linear.weight, self.linear.bias, self.LayerNorm.weight,
                                  self.LayerNorm.bias, self.LayerNorm.eps, None, 1)
            e = F.dropout(e, self.dropout.p, row_keys=rows.row_keys)
            if post_add is not None:
                e = (e.view(-1, rows_per_add, e.shape[1]) + post_add[:, None, :]).view_as(e)
            return e
        return F.embed_layernorm(x2d, self.linear.weight, self.linear.bias, self.LayerNorm.weight,
                                   self.LayerNorm.bias, self.LayerNorm.eps, post_add, rows_per_add)


class Predictor(nn.Module):
    """AnglesPredictor / AminoAcidPredictor: dense -> GELU -> LayerNorm -> dense
    (structure_model/model.py:120-154)."""

    def __init__(self, d_model, d_out, eps=1e-12):
        super().__init__()
        self.d_model, self.d_out = d_model, d_out
        self.dense1 = nn.Linear(d_model, d_model)
        self.layer_norm = nn.LayerNorm(d_model, eps=eps)
        self.dense2 = nn.Linear(d_model, d_out)

    def run(self, x):
        h = F.linear(x, self.dense1.weight, self.dense1.bias, ops.ACT_GELU)
        h = F.residual_layernorm(h, None, self.layer_norm.weight, self.layer_norm.bias, self.layer_norm.eps)
        return F.head_linear(h, self.dense2.weight, self.dense2.bias)


class KeyedDropoutSwitch:
    """Keyed dropout for a training wrapper ("Keyed sampling streams"): with a seed, every dropout decision of
    ``training_step`` is a function of (seed, batch["item_id"], epoch, dropout site, position, head, column or key) --
    not of the batch, the row, the frame, the launch mode or the steps run before."""

    keyed_dropout = None

    def use_keyed_dropout(self, seed, epoch=None):
        """``seed=None`` switches back to torch-seeded dropout.  ``epoch``: the int64 word in device memory the row keys
        take the epoch from (``keyed.epoch_word`` / ``keyed.set_epoch``; a seeded ``training.fit`` shares the word of its
        keyed draws); default: a word of this model's own at epoch 0.  Returns the word."""
        if seed is None:
            self.keyed_dropout = None
            return None
        if epoch is None:
            epoch = keyed.epoch_word(next(self.parameters()).device)
        self.keyed_dropout = (keyed.check_seed(seed), epoch)
        return epoch

    def keyed_dropout_step(self, batch):
        """The context ``training_step`` runs in: ``ops.keyed_dropout`` over this batch's item ids -- its site counter
        starts at 0, so every step numbers its dropout calls alike -- when the switch is on and dropout acts at all."""
        cfgs = (self.encoder_config, self.decoder_config)
        acts = self.training and any(getattr(c, "hidden_dropout_prob", 0.0) > 0 or getattr(c, "attention_probs_dropout_prob", 0.0) > 0
                                     for c in cfgs)
        if self.keyed_dropout is None or not acts:
            return contextlib.nullcontext()
        seed, epoch = self.keyed_dropout
        return ops.keyed_dropout(seed, epoch, keyed.batch_item_ids(batch, batch["ligand_attn_mask"].shape[0]))


def frame_rows(mask, stream):
    """The ``packing.Rows`` of a batch's padded frame from its float key mask [B, L]; inside ``ops.keyed_dropout`` with the
    row-key table of that frame on ``stream`` (keyed.DROP_LIGAND / keyed.DROP_POCKET), built once per step and frame."""
    kd = ops.keyed_dropout_state()
    return Rows.from_mask(mask, None if kd is None else kd.row_keys(stream, mask.shape[1]))


def flat2d(x):
    """[B,L,F] -> contiguous fp32 [B*L,F] view for the kernels."""
    return x.reshape(-1, x.shape[-1]).contiguous().float()


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("the denoiser runs on HIP kernels only: move the model and its inputs to a "
                               "GPU device (there is no CPU fallback; the CPU oracle lives in oracle/ and is "
                               "test infrastructure)")
