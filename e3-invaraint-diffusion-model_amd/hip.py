"""ctypes binding of the C-ABI HIP library (include/e3d_hip.h -> libe3d_hip.so).

The library is the product's only compute path: there is no CPU or eager-PyTorch fallback.
``lib()`` raises if the shared object is missing (build it with ``__graft_entry__.build()`` or
``csrc/build.sh``).
"""
import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("E3D_HIP_LIB", os.path.join(_HERE, "libe3d_hip.so"))   # override: kernel experiments
ABI_VERSION = 5

_P = c_void_p
# The padded-attention entry points share their leading arguments (e3d_hip.h); their signatures are put together from these.
_VIEW = [_P, c_int64, c_int64]                      # pointer, batch stride, row stride
_QKV = 3 * _VIEW + [_P, c_int, _P]                  # q, k, v views, dist_emb, P, key_mask
_SHAPE = 4 * [c_int]                                # B, nh, Lq, Lk
_ATTN_FWD = _QKV + [_P, _P] + _SHAPE                # ..., out, lse, shape
_ATTN_BWD = _QKV + 3 * [_P] + 3 * _VIEW + [_P, _P] + _SHAPE   # ..., out, lse, dout, dq, dk, dv views, d_dist_emb, workspace, shape
_STREAM = [_P]
_DROP = [c_float, c_uint64]                         # drop_p, drop_seed
_DROP_KEYED = [c_float, c_uint32, _P]               # drop_p, site, row_keys
_BOUNDS = [_P, c_int, _P, _P, _P]                   # e_scratch, e_scratch_ready, q / k / e absmax
_SIGNATURES = {
    "e3d_abi_version": (c_int, []),
    "e3d_last_error": (c_char_p, []),
    "e3d_gemm_bias_act_f32": (c_int, [_P, c_int64, _P, _P, _P, c_int64, c_int, c_int, c_int, c_int, _P]),
    "e3d_gemm_bias_act_f32_split": (c_int, [_P, c_int64, _P, _P, _P, c_int64, c_int, c_int, c_int, c_int, c_int, _P]),
    "e3d_gemm_bias_act_f32_split_ex": (c_int, [_P, c_int64, _P, _P, _P, c_int64, c_int, c_int, c_int, c_int, c_int, _P, c_float, _P]),
    "e3d_gemm_bias_act_f32_split_gated": (c_int, [_P, c_int64, _P, _P, _P, c_int64, c_int, c_int, c_int, c_int, c_int, _P, c_float,
                                                  c_int, _P, _P]),
    "e3d_absmax_f32": (c_int, [_P, c_int64, _P, _P]),
    "e3d_relkey_attn_fwd": (c_int, _ATTN_FWD + _STREAM),
    "e3d_relkey_attn_fwd_split": (c_int, _ATTN_FWD + [c_int] + _STREAM),
    "e3d_gemm_skinny_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "e3d_gemm_skinny_f32_split": (c_int, [_P, c_int64, _P, _P, _P, c_int64, c_int, c_int, c_int, c_int, c_int, _P, c_int64, _P]),
    "e3d_gemm_skinny_f32_split_ex": (c_int, [_P, c_int64, _P, _P, _P, c_int64, c_int, c_int, c_int, c_int, c_int, _P, c_int64, _P, c_float, _P]),
    "e3d_gemm_skinny_plan_select": (None, [c_int, c_int]),
    "e3d_gemm_skinny_residual_layernorm_f32_split": (c_int, [_P, c_int64, _P, _P, _P, _P, _P, c_float, _P, c_int, c_int, c_int,
                                                     c_int, _P, c_int64, _P]),
    "e3d_gemm_skinny_residual_layernorm_f32_split_ex": (c_int, [_P, c_int64, _P, _P, _P, _P, _P, c_float, _P, c_int, c_int, c_int,
                                                        c_int, _P, c_int64, c_float, _P]),
    "e3d_attn_skip_padded_tiles": (c_int, [c_int]),
    "e3d_gemm_kernel_select": (c_int, [c_int]),
    "e3d_gemm_general_select": (c_int, [c_int]),
    "e3d_attn_rescale_tau": (c_float, [c_float]),
    "e3d_residual_layernorm_fwd": (c_int, [_P, _P, _P, _P, c_float, _P, _P, c_int, c_int, _P]),
    "e3d_adaln_gate_fwd": (c_int, [_P, _P, _P, c_int, c_int, _P, c_int, c_int, _P]),
    "e3d_embed_layernorm_fwd": (c_int, [_P, c_int, _P, _P, _P, _P, c_float, _P, c_int, _P, _P, c_int, c_int, _P]),
    "e3d_adaln_gate_indexed_fwd": (c_int, [_P, _P, _P, _P, c_int, _P, c_int, _P, c_int, c_int, _P]),
    "e3d_classify_onehot_rows": (c_int, [_P, c_int, _P, _P, c_int, _P]),
    "e3d_embed_layernorm_fwd_ex": (c_int, [_P, c_int, _P, _P, _P, _P, c_float, _P, c_int, _P, _P, c_int, c_int, _P, _P]),
    "e3d_nerf_backbone": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P]),
    # training (backward) side
    "e3d_gemm_f32_split_general": (c_int, [_P, c_int64, c_int, _P, c_int64, c_int, _P, _P, c_int64, c_int, c_int,
                                           c_int, c_int, c_int, _P]),
    "e3d_transpose_grouped_f32": (c_int, [_P, _P, c_int, c_int, c_int, c_int64, c_int64, _P]),
    "e3d_gemm_wgrad_grouped_f32_split": (c_int, [_P, _P, _P, _P, c_uint64, c_int, c_int64, c_int64, c_int, c_int, c_int, c_int, _P]),
    "e3d_residual_layernorm_drop_fwd": (c_int, [_P, _P, _P, _P, c_float, _P, _P, c_int, c_int, c_float, c_uint64, _P]),
    "e3d_layernorm_bwd_drop": (c_int, [_P, _P, _P, c_float, _P, _P, _P, _P, c_int, c_int, c_float, c_uint64, _P]),
    # row-complete GEMM + bias + residual + LayerNorm (ABI v4)
    "e3d_weight_planes_bytes": (c_int64, [c_int, c_int]),
    "e3d_weight_planes_f32_split": (c_int, [_P, c_int, c_int, c_int, _P, _P]),
    "e3d_gemm_residual_layernorm_supported": (c_int, [c_int, c_int, c_int, c_int64]),
    "e3d_gemm_residual_layernorm_f32_split": (c_int, [_P, c_int64, _P, _P, _P, c_int64, _P, _P, c_float, _P, c_int64,
                                                      c_int, c_int, c_int, c_int, c_float, _P]),
    # activation planes: A of the row-complete kernel as written by its producer (additions to ABI v5)
    "e3d_activation_planes_bytes": (c_int64, [c_int, c_int]),
    "e3d_activation_planes_f32_split": (c_int, [_P, c_int64, c_int, c_int, c_int, _P, _P]),
    "e3d_gemm_residual_layernorm_planes_split": (c_int, [_P, _P, _P, _P, c_int64, _P, _P, c_float, _P, c_int64,
                                                         c_int, c_int, c_int, c_int, c_float, _P]),
    "e3d_gemm_planes_supported": (c_int, [c_int, c_int, c_int, c_int64, c_int, c_int]),
    "e3d_gemm_bias_act_planes_split": (c_int, [_P, c_int64, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, c_float, _P]),
    "e3d_attn_planes_supported": (c_int, [c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int]),
    "e3d_relkey_attn_fwd_split_planes": (c_int, _QKV + [_P] + _SHAPE + [c_int] + _BOUNDS + _STREAM),
    "e3d_gemm_wgrad_ragged_f32_split": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_uint64, c_int, c_int, c_int, _P]),
    "e3d_relkey_attn_bwd_workspace_floats": (c_int64, [c_int, c_int, c_int, c_int, c_int]),
    "e3d_relkey_attn_bwd": (c_int, _ATTN_BWD + _STREAM),
    "e3d_dropout_f32": (c_int, [_P, c_float, c_uint64, _P, c_int64, _P]),
    "e3d_relkey_attn_fwd_split_drop": (c_int, _ATTN_FWD + [c_int] + _DROP + _STREAM),
    "e3d_relkey_attn_fwd_split_ex": (c_int, _ATTN_FWD + [c_int] + _DROP + _BOUNDS + _STREAM),
    "e3d_attn_scratch_bytes": (c_int64, [c_int]),
    "e3d_ddpm_step_wrap_table": (c_int, [_P, _P, _P, _P, _P, c_int, _P, c_int64, _P]),
    "e3d_relkey_attn_bwd_drop": (c_int, _ATTN_BWD + _DROP + _STREAM),
    "e3d_relkey_attn_bwd_ex": (c_int, _ATTN_BWD + [c_int] + _DROP + _STREAM),
    "e3d_attn_dropout_mask": (c_int, [c_int, c_int, c_int, c_int, c_float, c_uint64, _P, _P]),
    "e3d_layernorm_bwd": (c_int, [_P, _P, _P, c_float, _P, _P, _P, c_int, c_int, _P]),
    "e3d_layernorm_bwd_workspace_floats": (c_int64, [c_int, c_int]),
    "e3d_layernorm_bwd_ws": (c_int, [_P, _P, _P, c_float, _P, _P, _P, _P, c_int, c_int, c_float, c_uint64, _P, c_int64, _P]),
    "e3d_adaln_gate_bwd": (c_int, [_P, _P, _P, c_int, c_int, _P, _P, c_int, c_int, _P]),
    "e3d_act_fwd": (c_int, [_P, c_int, _P, c_int64, _P]),
    "e3d_act_bwd": (c_int, [_P, _P, c_int, _P, c_int64, _P]),
    "e3d_colsum": (c_int, [_P, c_int64, _P, c_int, c_int, _P]),
    "e3d_group_sum": (c_int, [_P, c_int, _P, c_int, c_int, _P]),
    "e3d_small_k_wgrad": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "e3d_head_linear_bwd_dx": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P]),
    "e3d_head_linear_fwd": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "e3d_ddpm_step_wrap": (c_int, [_P, _P, _P, c_float, c_float, c_float, c_float, c_int, _P, c_int64, _P]),
    "e3d_q_sample_wrap": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int64, _P]),
    "e3d_discrete_posterior_sample": (c_int, [_P, _P, _P, _P, _P, c_int, _P, _P, c_int, c_int, c_int, _P]),
    "e3d_discrete_q_sample": (c_int, [_P, _P, _P, c_int, _P, c_int, c_int, c_int, _P]),
    # optimizer step (ABI v3)
    "e3d_optim_chunk_elems": (c_int, []),
    "e3d_grad_global_norm": (c_int, [_P, _P, _P, _P, c_int, c_float, _P, _P, _P]),
    "e3d_adamw_step_dyn": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, _P, _P, c_float, c_float, c_float, c_float, _P]),
    "e3d_adamw_step_dev": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, _P, _P, _P]),
    "e3d_dropout_set_epoch_ptr": (c_int, [_P]),
    "e3d_adamw_step": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, _P, c_float, c_float, c_float, c_float, c_float, c_int, _P]),
    # the same update carrying the weight EMA (training.WeightEMA): one more pointer table, d_n from the host / the device block
    "e3d_adamw_ema_step": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, _P, c_float, c_float, c_float, c_float, c_float, c_int,
                                   c_float, _P]),
    "e3d_adamw_ema_step_dev": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, _P, _P, _P]),
    # attention over variable-length segments (ABI v5)
    "e3d_attn_varlen_fwd": (c_int, [_P, c_int64, _P, c_int64, _P, c_int64, _P, _P, _P, _P, _P, c_int, _P, c_int, _P,
                                    c_int64, c_int, c_int, c_int, c_int, _P]),
    # keyed (seeded) sampling draws
    "e3d_keyed_ddpm_step_wrap": (c_int, [_P, _P, _P, _P, _P, c_uint64, c_int, _P, c_int64, c_int, _P]),
    "e3d_keyed_discrete_posterior_sample": (c_int, [_P, _P, _P, _P, _P, c_uint64, _P, _P, c_int, c_int, c_int, _P]),
    "e3d_keyed_draws": (c_int, [_P, c_uint64, c_int, c_int, c_int, c_int, c_int, c_float, _P, c_int64, _P]),
    # strided (DDIM / respaced) structure update: [T,8] coefficient table, step index on the device
    "e3d_strided_step_wrap": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, _P, c_int64, _P]),
    "e3d_keyed_strided_step_wrap": (c_int, [_P, _P, _P, _P, c_int, _P, c_uint64, c_int, c_int, _P, c_int64, c_int, _P]),
    # multistep (DPM-Solver++ 2M) structure update: the strided arguments plus the x0 history in and out (an addition)
    "e3d_multistep_step_wrap": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, _P, _P, c_int64, _P]),
    # partial redesign: held positions overwritten in place after the update (additions, no signature changed)
    "e3d_known_compose_wrap": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_float, c_int64, _P]),
    "e3d_keyed_known_compose_wrap": (c_int, [_P, _P, _P, _P, _P, c_int, c_float, _P, c_uint64, c_int64, c_int, _P]),
    "e3d_discrete_known_compose": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "e3d_keyed_discrete_known_compose": (c_int, [_P, _P, _P, _P, _P, c_uint64, _P, c_int, c_int, c_int, _P]),
    # sequence design controls: the posterior over (logits + bias) * inv_temp, and the last step's pick with its scores
    "e3d_discrete_posterior_sample_ctl": (c_int, [_P, _P, _P, c_float, _P, _P, _P, c_int, _P, _P, c_int, c_int, c_int, _P]),
    "e3d_keyed_discrete_posterior_sample_ctl": (c_int, [_P, _P, _P, c_float, _P, _P, _P, c_uint64, _P, _P, c_int, c_int, c_int,
                                                        _P]),
    "e3d_discrete_final_pick": (c_int, [_P, _P, c_float, _P, _P, _P, c_int64, c_int, _P]),
    # scoring supplied sequences: forward noising at per-item levels, per-row score terms, fixed-shape item sums
    "e3d_keyed_discrete_forward_levels": (c_int, [_P, _P, _P, _P, c_int, c_uint64, _P, c_int, c_int, c_int, _P]),
    "e3d_discrete_score_rows": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "e3d_masked_item_sums": (c_int, [_P, _P, _P, _P, c_int, c_int, _P]),
    # scoring supplied structures: keyed forward noising at per-item levels (stream 12), per-element terms + fixed-shape sums
    "e3d_keyed_q_sample_levels_wrap": (c_int, [_P, _P, _P, c_int, _P, _P, c_int, c_float, c_uint64, _P, _P, c_int, c_int, c_int,
                                               c_int, _P]),
    "e3d_angle_score_items": (c_int, [_P] * 5 + [c_int] + [_P] * 9 + [c_int, c_int, c_int, c_int, _P]),
    # keyed training and validation draws (ids and epoch read from device memory)
    "e3d_keyed_timesteps": (c_int, [_P, _P, c_uint64, c_int, c_int, _P, c_int, _P]),
    "e3d_keyed_q_sample_wrap": (c_int, [_P, _P, _P, _P, c_int, c_float, _P, _P, c_uint64, _P, _P, c_int, c_int, c_int, _P]),
    "e3d_keyed_discrete_q_sample": (c_int, [_P, _P, _P, _P, c_uint64, _P, c_int, c_int, c_int, _P]),
    # keyed dropout decisions: (drop_p, site, row_keys) in the place of (drop_p, drop_seed)
    "e3d_keyed_drop_row_keys": (c_int, [_P, c_int, c_int, _P, c_uint64, c_int, _P, _P]),
    "e3d_dropout_f32_keyed": (c_int, [_P, c_float, c_uint32, _P, _P, c_int, c_int, _P]),
    "e3d_keyed_attn_dropout_mask": (c_int, [c_int, c_int, c_int, c_int, c_float, c_uint32, _P, _P, _P]),
    "e3d_residual_layernorm_drop_fwd_keyed": (c_int, [_P, _P, _P, _P, c_float, _P, _P, c_int, c_int, c_float, c_uint32, _P, _P]),
    "e3d_layernorm_bwd_drop_keyed": (c_int, [_P, _P, _P, c_float, _P, _P, _P, _P, c_int, c_int, c_float, c_uint32, _P, _P]),
    "e3d_layernorm_bwd_ws_keyed": (c_int, [_P, _P, _P, c_float, _P, _P, _P, _P, c_int, c_int, c_float, c_uint32, _P, _P, c_int64,
                                           _P]),
    "e3d_relkey_attn_fwd_split_drop_keyed": (c_int, _ATTN_FWD + [c_int] + _DROP_KEYED + _STREAM),
    "e3d_relkey_attn_fwd_split_ex_keyed": (c_int, _ATTN_FWD + [c_int] + _DROP_KEYED + _BOUNDS + _STREAM),
    "e3d_relkey_attn_bwd_drop_keyed": (c_int, _ATTN_BWD + _DROP_KEYED + _STREAM),
    "e3d_relkey_attn_bwd_ex_keyed": (c_int, _ATTN_BWD + [c_int] + _DROP_KEYED + _STREAM),
    # featurization of PDB coordinates (featurize.py)
    "e3d_backbone_angles": (c_int, [_P, _P, _P, _P, c_int, c_float, _P]),
    "e3d_contact_residues": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P]),
    # rigid superposition of structure pairs (evaluate.py)
    "e3d_superpose_pairs": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    # secondary structure, hydrogen bonds, bends and clashes of backbones (evaluate.py, featurize.py)
    "e3d_backbone_geometry": (c_int, 12 * [_P] + [c_int, c_int, c_double, c_double, _P]),
    # local alignment of sequence sets (similarity.py)
    "e3d_align_workspace_bytes": (c_int64, [c_int, c_int]),
    "e3d_align_pairs": (c_int, 9 * [_P] + [c_int64] + 7 * [c_int] + [_P]),
}
EXPORTS = tuple(_SIGNATURES)

_lib = None


class HipExtensionMissing(RuntimeError):
    pass


def lib():
    """Load (once) and return the ctypes handle; fail loudly when the library is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipExtensionMissing(
                f"{LIB_PATH} not found: the HIP extension is the only compute path of this package "
                "(no CPU fallback). Build it with `python -c 'import __graft_entry__ as g; g.build()'`.")
        # torch ships its own libamdhip64; import it FIRST so that this library binds to the same
        # HIP runtime instance (two runtimes in one process do not share the device context).
        import torch  # noqa: F401
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the header and the .so disagree
            fn.restype, fn.argtypes = res, args
        got = handle.e3d_abi_version()
        if got != ABI_VERSION:
            raise HipExtensionMissing(f"{LIB_PATH}: ABI version {got}, binding expects {ABI_VERSION}")
        _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().e3d_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (rc={rc}): {msg}")
