"""BERT encoder/decoder stacks with ``relative_key`` self-attention, executed by HIP kernels.

Mirrors the module tree -- and therefore the ``state_dict`` key names, the checkpoint wire
format -- of transformers==4.38.2 ``BertEncoder`` / ``BertLayer`` /
``BertAttention`` as the reference instantiates them (structure_model/model.py:16-20,40,171,177),
but none of that package's code runs: the nn.Modules below only own parameters, and ``run_*``
execute the math as fused gfx950 kernels on [B*L, H] row-major activations.
"""
from dataclasses import dataclass
from typing import NamedTuple

import os

import torch
from torch import nn

from . import ops
from .autograd import functional as F


@dataclass
class BertConfig:
    """The subset of transformers.BertConfig the reference sets (structure_model/sample.py:160-183).
    Any object with these attributes (e.g. a real transformers.BertConfig) is accepted too."""
    hidden_size: int = 768
    num_attention_heads: int = 12
    intermediate_size: int = 1024
    num_hidden_layers: int = 12
    max_position_embeddings: int = 64
    position_embedding_type: str = "relative_key"
    hidden_dropout_prob: float = 0.1
    attention_probs_dropout_prob: float = 0.1
    layer_norm_eps: float = 1e-12
    hidden_act: str = "gelu"
    use_cache: bool = False
    is_decoder: bool = False
    add_cross_attention: bool = False


def _check_config(cfg):
    head = cfg.hidden_size // cfg.num_attention_heads
    if cfg.hidden_size % cfg.num_attention_heads or head != 64:
        raise ValueError(f"HIP attention kernel needs head dim 64 (hidden {cfg.hidden_size}, "
                         f"heads {cfg.num_attention_heads})")
    if cfg.hidden_size not in (256, 512, 768, 1024):
        raise ValueError("HIP row kernels need hidden_size in {256,512,768,1024}")
    if cfg.intermediate_size % 128:
        raise ValueError("HIP GEMM needs intermediate_size % 128 == 0")
    if getattr(cfg, "hidden_act", "gelu") != "gelu":
        raise ValueError("only the exact-erf GELU the reference uses is implemented")
    if cfg.position_embedding_type not in ("relative_key", "absolute"):
        raise ValueError(f"unsupported position_embedding_type {cfg.position_embedding_type}")


# ----------------------------------------------------------------------------- parameter tree
class BertSelfAttention(nn.Module):
    def __init__(self, cfg, position_embedding_type=None):
        super().__init__()
        h = cfg.hidden_size
        self.query, self.key, self.value = nn.Linear(h, h), nn.Linear(h, h), nn.Linear(h, h)
        self.position_embedding_type = position_embedding_type or cfg.position_embedding_type
        self.max_position_embeddings = cfg.max_position_embeddings
        if self.position_embedding_type == "relative_key":
            self.distance_embedding = nn.Embedding(2 * cfg.max_position_embeddings - 1,
                                                   h // cfg.num_attention_heads)


class BertSelfOutput(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.dense = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        self.LayerNorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class BertAttention(nn.Module):
    def __init__(self, cfg, position_embedding_type=None):
        super().__init__()
        _check_config(cfg)
        self.self = BertSelfAttention(cfg, position_embedding_type)
        self.output = BertSelfOutput(cfg)
        self.num_heads = cfg.num_attention_heads
        self.eps = cfg.layer_norm_eps
        self.config = cfg


class BertIntermediate(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.dense = nn.Linear(cfg.hidden_size, cfg.intermediate_size)


class BertOutput(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.dense = nn.Linear(cfg.intermediate_size, cfg.hidden_size)
        self.LayerNorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class BertLayer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.attention = BertAttention(cfg)
        if cfg.add_cross_attention:
            if not cfg.is_decoder:
                raise ValueError("cross attention needs is_decoder=True")
            # 4.38.2 BertLayer builds the cross attention with position_embedding_type="absolute"
            self.crossattention = BertAttention(cfg, position_embedding_type="absolute")
        self.intermediate = BertIntermediate(cfg)
        self.output = BertOutput(cfg)
        self.eps = cfg.layer_norm_eps


class BertEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        _check_config(cfg)
        self.config = cfg
        self.layer = nn.ModuleList([BertLayer(cfg) for _ in range(cfg.num_hidden_layers)])


# ----------------------------------------------------------------------------- packed weights
TIE_PACKED = os.environ.get("E3D_TIE_QKV", "1") == "1"     # 0: a fresh torch.cat per forward (A/B runs)


class _TiedPack(torch.autograd.Function):
    """(packed weight, packed bias) as differentiable functions of the parameters whose storage they ALIAS (``_tie``): no
    copy and no kernel in either direction.  The backward (only reached when the weight gradients are not deferred:
    autograd.deferred_weight_grads writes the row blocks' gradients straight into the parameters) hands each parameter
    its row block of the packed gradient."""

    @staticmethod
    def forward(ctx, w_packed, b_packed, n, *parts):
        ctx.n, ctx.rows = n, [p.shape[0] for p in parts[:n]]
        ctx.set_materialize_grads(False)      # deferred weight gradients hand back None: no zero tensors, no zero accumulation
        return w_packed.view(w_packed.shape), b_packed.view(b_packed.shape)

    @staticmethod
    def backward(ctx, gw, gb):
        gws = gw.split(ctx.rows, 0) if gw is not None else (None,) * ctx.n
        gbs = gb.split(ctx.rows, 0) if gb is not None else (None,) * ctx.n
        return (None, None, None) + tuple(gws) + tuple(gbs)


def _tie(owner, name, tensors):
    """One buffer [sum rows, ...] whose row blocks ARE the given parameters: on first use (and whenever a parameter has
    moved: ``module.to()``, a re-assigned ``.data``) the values are packed once and every parameter's ``.data`` becomes a
    view of its block.  In-place updates (optimizers, ``load_state_dict``, broadcasts) then keep the packed tensor current
    for free; names, shapes and ``state_dict`` are unchanged."""
    tied = owner.__dict__.setdefault("_e3d_tied", {})
    ent = tied.get(name)
    ok = ent is not None and ent.device == tensors[0].device
    if ok:
        at = ent.data_ptr()
        for t in tensors:
            if t.data_ptr() != at or not t.is_contiguous():
                ok = False
                break
            at += 4 * t.numel()
    if not ok:
        with torch.no_grad():
            ent = torch.cat([t.detach() for t in tensors], dim=0).contiguous()
            r0 = 0
            for t in tensors:
                t.data = ent[r0:r0 + t.shape[0]]
                r0 += t.shape[0]
        tied[name] = ent
    return ent


def _packed(owner, name, weights, biases):
    """(cat(weights), cat(biases)) of per-projection parameters.  Inference: copies cached on the owner and rebuilt when
    any source parameter changes (in-place update or re-assignment).  Training (a source requires grad and autograd is
    on): the parameters are tied to packed buffers (``_tie``) and the pair is a zero-copy alias of them -- a training
    step used to spend 72 cat kernels (0.5 ms) re-packing weights the optimizer had just updated."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in weights):
        if TIE_PACKED and all(t.dtype == torch.float32 for t in list(weights) + list(biases)):
            w, b = _TiedPack.apply(_tie(owner, "w_" + name, weights), _tie(owner, "b_" + name, biases), len(weights),
                                   *weights, *biases)
        else:
            w, b = torch.cat(list(weights), dim=0), torch.cat(list(biases), dim=0)
        w._e3d_parts, b._e3d_parts = list(weights), list(biases)   # autograd.deferred_weight_grads writes the row blocks'
        return w, b                                                 # gradients straight into these parameters
    out = []
    cache = owner.__dict__.setdefault("_e3d_pack", {})
    for key_name, tensors in (("w_" + name, weights), ("b_" + name, biases)):
        key = ops.weight_key(*tensors)    # includes the optimizer-step generation: fused optimizers do not bump _version
        hit = cache.get(key_name)
        if hit is None or hit[0] != key:
            with torch.no_grad():
                hit = (key, torch.cat([t.detach() for t in tensors], dim=0).contiguous())
            cache[key_name] = hit
        out.append(hit[1])
    return out[0], out[1]


def qkv_weights(sa):
    return _packed(sa, "qkv", [sa.query.weight, sa.key.weight, sa.value.weight], [sa.query.bias, sa.key.bias, sa.value.bias])


def kv_weights(sa):
    return _packed(sa, "kv", [sa.key.weight, sa.value.weight], [sa.key.bias, sa.value.bias])


class Drop(NamedTuple):
    """The dropout of one model-layer call: the rates after ``BertSelfOutput.dense`` / ``BertOutput.dense`` and after the
    self/cross-attention softmax (where transformers 4.38.2 applies ``nn.Dropout``) and, keyed dropout, the key table of
    the rows of x -- the query rows of both attentions (``ops.KeyedDropout.row_keys``) -- or None."""
    hidden: float
    attention: float
    row_keys: object = None

    @property
    def off(self):
        return self.hidden == 0 and self.attention == 0

    @classmethod
    def of(cls, module, rows):
        """For ``module`` (a BertEncoder or BertAttention) on ``rows`` (packing.Rows): its config's rates in training mode, zeros in eval."""
        cfg = module.config if module.training else None      # (eval: no config to read, both rates default to zero)
        drop = cls(float(getattr(cfg, "hidden_dropout_prob", 0.0)), float(getattr(cfg, "attention_probs_dropout_prob", 0.0)),
                   rows.row_keys)
        if rows.packed and not drop.off:
            raise RuntimeError("packed layouts are inference-only: put the model in eval mode")
        return drop


# ----------------------------------------------------------------------------- executors
def _attention_output(att, ctx, x, drop):
    return F.linear_residual_layernorm(ctx, att.output.dense.weight, att.output.dense.bias, x, att.output.LayerNorm.weight,
                                       att.output.LayerNorm.bias, att.eps, drop.hidden, drop.row_keys)


def _planes_for(att, x, drop):
    """The consumer of an attention context, for ``F.attention(planes_for=)``: without dropout (inference) the context's only
    reader is ``_attention_output`` -- out-projection + residual x + LayerNorm -- which may take it as activation planes."""
    return (att.output.dense.weight, x) if drop.off else None


def run_self_attention(att, x, rows, drop):
    """BertAttention on x [rows.rows, H] (``rows``: packing.Rows): fused QKV GEMM -> fused relative-key attention over
    the padded frame and its key mask, or over the segments of packed rows -> out-proj GEMM -> residual + LayerNorm."""
    sa = att.self
    w, b = qkv_weights(sa)
    qkv = F.linear(x, w, b, absmax=ops.absmax_slot(sa, "qkv", x.device))
    dist_emb = sa.distance_embedding.weight if sa.position_embedding_type == "relative_key" else None
    if rows.packed:
        H = att.num_heads * 64
        ctx = ops.attention_varlen(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], rows.layout, rows.layout, att.num_heads,
                                   dist_emb=dist_emb, max_pos=sa.max_position_embeddings)
    else:
        ctx = F.attention(qkv, None, rows.B, att.num_heads, rows.L, rows.L, key_mask=rows.mask, dist_emb=dist_emb,
                          max_pos=sa.max_position_embeddings, drop_p=drop.attention, row_keys=drop.row_keys,
                          planes_for=_planes_for(att, x, drop))
    return _attention_output(att, ctx, x, drop)


def project_cross_kv(att, enc):
    """K/V projection of the encoder states for one decoder layer -> [B*Lk, 2H].  It depends on
    neither the timestep nor the noised ligand, so samplers compute it once."""
    w, b = kv_weights(att.self)
    # (a scalar of its own, not a pool slot: samplers keep this projection -- and its bound -- for a whole chain)
    return F.linear(enc, w, b, absmax=torch.zeros(1, device=enc.device, dtype=torch.float32))


def run_cross_attention(att, x, rows, kv, kv_rows, drop):
    """Queries x (``rows``) against the projected encoder states kv (``kv_rows``).  Packed query rows take key rows that
    are packed too or a padded cache (``PackedLayout.padded_frame``)."""
    q = F.linear(x, att.self.query.weight, att.self.query.bias, absmax=ops.absmax_slot(att.self, "q", x.device))
    if rows.packed:
        H = att.num_heads * 64
        ctx = ops.attention_varlen(q, kv[:, :H], kv[:, H:], rows.layout, kv_rows.layout, att.num_heads)
    else:
        ctx = F.attention(q, kv, rows.B, att.num_heads, rows.L, kv_rows.L, key_mask=kv_rows.mask, drop_p=drop.attention,
                          row_keys=drop.row_keys, planes_for=_planes_for(att, x, drop))
    return _attention_output(att, ctx, x, drop)


def run_layer(layer, x, rows, drop, cross_kv=None, kv_rows=None):
    """One BertLayer on x (``rows``); ``cross_kv`` (``kv_rows``): the projected encoder states of a decoder layer."""
    x = run_self_attention(layer.attention, x, rows, drop)
    if hasattr(layer, "crossattention"):
        if cross_kv is None:
            raise ValueError("decoder layer needs encoder states")
        x = run_cross_attention(layer.crossattention, x, rows, cross_kv, kv_rows, drop)
    # (without dropout -- inference -- the intermediate's only reader is the BertOutput below: it may leave as activation planes)
    inter = F.linear(x, layer.intermediate.dense.weight, layer.intermediate.dense.bias, ops.ACT_GELU,
                     planes_for=(layer.output.dense.weight, x) if drop.off else None)
    return F.linear_residual_layernorm(inter, layer.output.dense.weight, layer.output.dense.bias, x,
                                       layer.output.LayerNorm.weight, layer.output.LayerNorm.bias, layer.eps, drop.hidden,
                                       drop.row_keys)


def run_encoder(encoder, x, rows, enc=None, enc_rows=None, cross_kv=None):
    """BertEncoder(...).last_hidden_state on flat activations x (``rows``: packing.Rows).  ``enc`` (``enc_rows``): the
    encoder states a decoder's cross-attention reads; ``cross_kv`` (list, one per layer) short-cuts their per-layer K/V
    projection."""
    drop = Drop.of(encoder, rows)
    for i, layer in enumerate(encoder.layer):
        kv = None
        if hasattr(layer, "crossattention"):
            kv = cross_kv[i] if cross_kv is not None else project_cross_kv(layer.crossattention, enc)
        x = run_layer(layer, x, rows, drop, kv, enc_rows)
    return x
