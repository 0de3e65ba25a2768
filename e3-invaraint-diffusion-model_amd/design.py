"""Sequence design controls: sampling temperature, residues forbidden everywhere (``omit``), residues allowed at chosen
positions (``allow``) and an additive residue bias, folded into one record the sequence sampler understands.

The record holds a bias ``[B, L, C]`` (``-inf`` forbids a class at a position) and the inverse temperature; the sampler's
kernels take softmax((logits + bias) * inv_temp) wherever they took softmax(logits) (include/e3d_hip.h, "sequence design
controls").  The controls shape the model's x0 prediction.  Intermediate states are noisy by construction and may pass
through a forbidden class; the guarantee is on the output: a designed position of the returned sequence never holds a
forbidden residue.  The temperature acts on the steps s > 0 only, the final pick is an argmax.  Host-side parsing only:
nothing here touches the GPU.
"""
import math

import numpy as np
import torch

from .structure_model.dataset import AA_VOCAB


def _letters(letters, what):
    """Class indices of a string of residue letters, each checked against AA_VOCAB."""
    if not isinstance(letters, str):
        raise TypeError(f"{what}: expected a string of residue letters, got {type(letters).__name__}")
    idx = []
    for a in letters.strip().upper():
        if a not in AA_VOCAB:
            raise ValueError(f"{what}: {a!r} is not a residue letter (one of {AA_VOCAB})")
        idx.append(AA_VOCAB.index(a))
    return sorted(set(idx))


def parse_allow(spec):
    """``"3:LIV;7:DE"`` -> {3: "LIV", 7: "DE"}: 0-based ligand positions and the residues allowed there ("" -> {}).
    A malformed entry raises ``ValueError`` with the offending token."""
    if not isinstance(spec, str):
        raise TypeError(f"allow: expected a list such as '3:LIV;7:DE', got {type(spec).__name__}")
    out = {}
    for token in spec.split(";"):
        tok = token.strip()
        if not tok:
            if spec.strip():
                raise ValueError(f"allow: empty entry in {spec!r}")
            continue
        pos, colon, letters = tok.partition(":")
        pos, letters = pos.strip(), letters.strip()
        if not colon or not (pos.isdigit() and pos.isascii()) or not letters:
            raise ValueError(f"allow: malformed entry {tok!r} in {spec!r} (expected POSITION:LETTERS)")
        if int(pos) in out:
            raise ValueError(f"allow: position {int(pos)} is named twice in {spec!r}")
        out[int(pos)] = letters
    return out


def _allow_of(allow, index):
    """The {position: letters} dict of dataset item ``index``."""
    if allow is None:
        return {}
    table = allow(index) if callable(allow) else allow
    if isinstance(table, str):
        table = parse_allow(table)
    if not isinstance(table, dict):
        raise TypeError(f"allow: expected a dict, a string or a callable returning one, got {type(table).__name__}")
    for pos in table:
        if isinstance(pos, bool) or not isinstance(pos, (int, np.integer)) or pos < 0:
            raise ValueError(f"allow: positions are 0-based integers, got {pos!r}")
    return table


class DesignControls:
    """``bias`` float32 [B, L, C] on the CPU in the padded frame (None: nothing set), ``inv_temp`` =
    np.float32(1) / np.float32(temperature), ``active`` = there is something for the sampler to apply.  Build with
    ``DesignControls.build``."""

    def __init__(self, bias, inv_temp, temperature=1.0):
        self.bias = bias
        self.inv_temp = np.float32(inv_temp)
        self.temperature = float(temperature)

    @property
    def active(self):
        return self.bias is not None or self.inv_temp != np.float32(1)

    @classmethod
    def build(cls, batch_or_shape, temperature=1.0, omit="", allow=None, bias=None, first_index=0):
        """``batch_or_shape``: a loader batch (``ligand_seq`` [B, L, C] and ``ligand_attn_mask`` [B, L], whose row sums
        are the ligands' lengths) or a shape (B, L, C), every ligand then L long.
        ``omit``: residue letters forbidden at every position.  ``allow``: {position: "LIV"}, the string "3:LIV;7:DE", or a
        callable dataset index -> either (item b has index ``first_index`` + b): everything else is forbidden at those
        0-based ligand positions; positions at or beyond a ligand's length are ignored.  ``bias``: {letter: float}, or a
        tensor [C], [L, C] or [B, L, C], added to the logits.  A position of a ligand left with no allowed class, and a
        temperature that is not a positive finite number, raise ``ValueError``."""
        if isinstance(batch_or_shape, dict):
            B, L, C = batch_or_shape["ligand_seq"].shape
            lengths = [min(int(n), L) for n in batch_or_shape["ligand_attn_mask"].sum(dim=1).tolist()]
        else:
            B, L, C = (int(v) for v in batch_or_shape)
            lengths = [L] * B
        try:
            temperature = float(temperature)
        except (TypeError, ValueError):
            raise ValueError(f"temperature must be a positive finite number, got {temperature!r}") from None
        with np.errstate(all="ignore"):      # a temperature outside fp32's range ends as 0 or inf and is refused below
            inv_temp = np.float32(1) / np.float32(temperature) if temperature > 0 else np.float32(0)
        if not (inv_temp > 0 and np.isfinite(inv_temp)):
            raise ValueError(f"temperature must be a positive finite number, got {temperature!r}")
        if C > len(AA_VOCAB) and (omit or allow is not None or isinstance(bias, dict)):
            raise ValueError(f"residue letters name {len(AA_VOCAB)} classes, the batch has {C}")
        total = None

        def table():
            return torch.zeros(B, L, C, dtype=torch.float32) if total is None else total

        if bias is not None:
            if isinstance(bias, dict):
                row = torch.zeros(C, dtype=torch.float32)
                for letter, value in bias.items():
                    idx = _letters(letter, "bias")
                    if len(idx) != 1 or idx[0] >= C:
                        raise ValueError(f"bias: keys are single residue letters, got {letter!r}")
                    row[idx[0]] = float(value)
                bias = row
            if not torch.is_tensor(bias) or tuple(bias.shape) not in ((C,), (L, C), (B, L, C)):
                raise ValueError(f"bias must be a dict of letters or a tensor [{C}], [{L}, {C}] or [{B}, {L}, {C}], got "
                                 f"{tuple(bias.shape) if torch.is_tensor(bias) else type(bias).__name__}")
            bias = bias.detach().to("cpu", torch.float32)
            if bool(torch.isnan(bias).any()) or bool((bias == math.inf).any()):
                raise ValueError("bias: NaN and +inf are not usable values (-inf forbids a class)")
            total = table() + bias
        omitted = [c for c in _letters(omit, "omit") if c < C]
        if omitted:
            total = table()
            total[:, :, omitted] = -math.inf
        if allow is not None:
            for b in range(B):
                for pos, letters in _allow_of(allow, first_index + b).items():
                    if pos >= lengths[b]:
                        continue
                    keep = [c for c in _letters(letters, f"allow[{pos}]") if c < C]
                    total = table()
                    closed = torch.ones(C, dtype=torch.bool)
                    closed[keep] = False
                    total[b, pos, closed] = -math.inf
        if total is not None:
            dead = (total == -math.inf).all(dim=-1)
            for b in range(B):
                hit = dead[b, :lengths[b]].nonzero().flatten().tolist()
                if hit:
                    raise ValueError(f"design controls leave item {first_index + b}, position {hit[0]} with no allowed residue")
            if not bool((total != 0).any()):
                total = None
        return cls(None if total is None else total.contiguous(), inv_temp, temperature)

    def in_frame(self, move, device):
        """The record a chain runs with: the bias moved onto the chain's rows by ``move`` (the function that moves the
        state) and onto ``device``, contiguous."""
        bias = None if self.bias is None else move(self.bias.to(device)).contiguous()
        return DesignControls(bias, self.inv_temp, self.temperature)
