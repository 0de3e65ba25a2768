"""Tensor-level wrappers over the C-ABI: allocate outputs with torch (device memory + stream
plumbing only) and enqueue the HIP kernels on torch's current stream."""
import contextlib
import math
import os
import warnings

import torch

from . import hip, keyed

ACT_NONE, ACT_GELU, ACT_SILU = 0, 1, 2


def _stream():
    return torch.cuda.current_stream().cuda_stream


# Per-launch timing hook for bench.py: when TRACE is a list, timed launches append
# (kernel name, start event, end event, meta) -- HIP events on the launch stream.
TRACE = None


# roctx ranges around the hot-path kernels (K1 rel-key attention, K2 cross attention, K3 their
# backward, K4 adaLN gate, K5 LayerNorm / GEMM epilogues, K6 DDPM update + wrap, K7 discrete posterior; plus the
# GEMMs).  E3D_ROCTX=1 (tools/profile_round.sh sets it) loads libroctx64 and brackets every launch of those ops;
# `rocprofv3 --marker-trace` then shows the ranges next to the kernel trace.  Off by default: two ctypes calls
# per launch are measurable in the single-pocket loop.
_ROCTX = None


def _roctx():
    global _ROCTX
    if _ROCTX is None:
        _ROCTX = False
        if os.environ.get("E3D_ROCTX") == "1":
            import ctypes
            for name in ("libroctx64.so", "libroctx64.so.4", "/opt/rocm/lib/libroctx64.so"):
                try:
                    lib = ctypes.CDLL(name)
                    lib.roctxRangePushA.argtypes = [ctypes.c_char_p]
                    _ROCTX = lib
                    break
                except OSError:
                    continue
    return _ROCTX


ROCTX_NAMES = {"attn_relkey": b"K1 relkey_attention_fwd", "attn_cross": b"K2 cross_attention_fwd",
               "attn_bwd": b"K3 attention_bwd", "adaln_gate": b"K4 adaln_gate",
               "residual_layernorm": b"K5 residual_layernorm", "embed_layernorm": b"K5 embed_layernorm",
               "gemm_layernorm": b"K5 gemm_residual_layernorm",
               "gemm": b"K5 gemm_bias_act", "ddpm_step_wrap": b"K6 ddpm_step_wrap",
               "discrete_posterior": b"K7 discrete_posterior_sample", "discrete_q_sample": b"K7 discrete_q_sample"}


class _timed:
    """Brackets one launch: HIP events on the launch stream when bench.py collects a TRACE, a roctx range when
    E3D_ROCTX=1."""

    def __init__(self, name, meta=None):
        self.on = TRACE is not None
        self.rx = _roctx()
        self.name = name
        if self.on:
            self.rec = (name, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), meta)

    def __enter__(self):
        if self.rx:
            self.rx.roctxRangePushA(ROCTX_NAMES.get(self.name, self.name.encode()))
        if self.on:
            self.rec[1].record()

    def __exit__(self, *exc):
        if self.on:
            self.rec[2].record()
            TRACE.append(self.rec)
        if self.rx:
            self.rx.roctxRangePop()


def _chk(t, name, dtype=torch.float32):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (this package has no CPU path), got {t.device}")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")


def _p(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------- derived-weight caches
# Tensors derived from parameters (packed QKV weights, W^T for the input-gradient GEMM, the distance-table planes) are
# cached on their source and keyed on (tensor._version, data_ptr, PARAM_GENERATION).  ``_version`` alone is NOT enough:
# torch's fused optimizer kernels (torch.optim.AdamW(fused=True), used by training.adamw) update parameters without
# bumping it, so a cache keyed only on the version would keep serving the weights of the first step.  Every
# optimizer step therefore bumps PARAM_GENERATION through a global post-step hook (registered at import); code that
# writes parameter storage by other means behind autograd's back calls ``invalidate_weight_caches()`` itself.
PARAM_GENERATION = 0


def invalidate_weight_caches(*_args, **_kwargs):
    global PARAM_GENERATION
    PARAM_GENERATION += 1


def weight_key(*tensors):
    return (PARAM_GENERATION,) + tuple((t.data_ptr(), t._version) for t in tensors)


try:
    from torch.optim.optimizer import register_optimizer_step_post_hook as _reg_post_hook
    _reg_post_hook(invalidate_weight_caches)
except ImportError:      # very old torch: training.fit() bumps the generation after every step instead
    pass


# ---------------------------------------------------------------------------------------------- |out| bounds
# The attention kernels may skip key tiles that are padding in every position only when that is exact: the reference
# masks additively with -10000 (structure_model/model.py:226-231), so a padded key stays out of the softmax only while
# the scores of a row spread over less than ~9900 (include/e3d_hip.h, e3d_attn_skip_padded_tiles).  The proof comes from
# the GEMMs that produce Q and K: launched with ``absmax=<slot>`` they raise a device scalar to the largest |output|
# (atomic max in the epilogue), the attention call reads the scalars on the device.  Slots are one float each in a
# per-device pool, handed out once per owner (a BertSelfAttention module) and only ever raised by the kernels:
# ``reset_absmax()`` (one fill launch) zeroes them all -- models call it once per batch / sampling chain, so a slot holds
# the running maximum of that chain.  A stale (too large) value is still a valid bound: it can only cost the skip.
_ABSMAX_POOLS = {}      # device index -> [current pool tensor, slots handed out of it, earlier (full) pool tensors]
ABSMAX_POOL_SLOTS = 4096


def absmax_slot(owner, name, device):
    """The device scalar (1-element view) that bounds |outputs| of ``owner``'s projection ``name``."""
    slots = owner.__dict__.setdefault("_e3d_absmax", {})
    key = (name, device.index)
    t = slots.get(key)
    if t is None:
        ent = _ABSMAX_POOLS.get(device.index)
        if ent is None:
            ent = _ABSMAX_POOLS[device.index] = [torch.zeros(ABSMAX_POOL_SLOTS, device=device, dtype=torch.float32), 0, []]
        if ent[1] >= ABSMAX_POOL_SLOTS:     # slots are never handed back (a process that builds model after model): grow
            ent[2].append(ent[0])
            ent[0], ent[1] = torch.zeros(ABSMAX_POOL_SLOTS, device=device, dtype=torch.float32), 0
        t = slots[key] = ent[0][ent[1]:ent[1] + 1]
        ent[1] += 1
    return t


def reset_absmax(device=None):
    """Zero every slot of the device's pool (one launch): the start of a batch or of a sampling chain."""
    idx = torch.cuda.current_device() if device is None else torch.device(device).index
    ent = _ABSMAX_POOLS.get(idx)
    if ent is not None:
        ent[0].zero_()
        for old_pool in ent[2]:
            old_pool.zero_()


def absmax(x, target=None):
    """max(target, max |x|) as a 1-element device tensor (e3d_absmax_f32); NaN / inf in x give NaN / inf."""
    _chk(x, "absmax.x")
    assert x.is_contiguous()
    if target is None:
        target = torch.zeros(1, device=x.device, dtype=torch.float32)
    hip.check(hip.lib().e3d_absmax_f32(_p(x), x.numel(), _p(target), _stream()), "e3d_absmax_f32")
    return target


# GEMM arithmetic: "f32" = exact fp32 MFMA; "bf16x3" / "bf16x6" = fp32 operands split into 2 / 3
# bf16 terms on the bf16 matrix cores with fp32 accumulation (gemm_split.hip).  bf16x6 is fp32-grade
# (4e-7 end-to-end vs 1.8e-6 for fp32 itself), bf16x3 ~2.6e-5 end-to-end (tolerance 1e-4).
# "f16x3" = 2 fp16 terms (11 + 11 bits), 3 cross products: fp32-grade accuracy at the cost of bf16x3 for operands
# inside the fp16 range (|x| < 65504 -- larger values give inf/NaN, loudly; include/e3d_hip.h E3D_TERMS_F16X3);
# forward GEMMs and the cooperative attention kernel, every other path of that mode runs bf16x6 / fp32 kernels.
# "bf16" = plain bf16 products (operands rounded to bf16, ONE MFMA per product, fp32 accumulate: ~2^-8 per product) -- the
# precision the reference's TRAIN scripts select (torch.set_float32_matmul_precision("medium"),
# structure_model/train_model.py:120).  GEMMs only (the attention kernels then run bf16x3), opt-in through
# E3D_TRAIN_ARITHMETIC=bf16 / ops.arithmetic("bf16"); never an inference default: it is 1e-2-grade, not 1e-4.
GEMM_MODES = {"f32": 0, "bf16x3": 3, "bf16x6": 6, "f16x3": 19, "bf16": 1}
GEMM_MODE = os.environ.get("E3D_GEMM_MODE", "f16x3")   # inference default: fp32 grade at bf16x3 speed
if GEMM_MODE not in GEMM_MODES:
    raise ValueError(f"E3D_GEMM_MODE must be one of {sorted(GEMM_MODES)}, got {GEMM_MODE!r}")


def set_gemm_mode(mode):
    global GEMM_MODE
    if mode not in GEMM_MODES:
        raise ValueError(f"gemm mode must be one of {sorted(GEMM_MODES)}, got {mode!r}")
    prev, GEMM_MODE = GEMM_MODE, mode
    return prev


# f16x3 weights: two fp16 terms carry 22 bits only while BOTH are normal numbers -- an element below 2^-3 = 0.125
# already has its low term in the fp16 subnormals (absolute floor 2^-25), and nn.Linear weights are ~0.02-0.05.  Each
# weight is therefore multiplied by a power of two (exact) that puts its largest |element| in [2^11, 2^12) -- elements
# down to 2^-15 of the largest keep 22 bits, the largest is 16x below the fp16 maximum, a weight of ANY magnitude is safe
# -- and the kernels multiply the accumulator by the inverse power (exact) before the bias (``out_scale`` of the *_ex
# entry points).  Scaled copies are cached on the weight tensor (keyed like every derived-weight cache); building one
# reads max |w| back to the host, once per weight and version.  Activations are not scaled: the path's GEMM inputs are
# LayerNorm / GELU / softmax outputs, and an activation beyond 65504 gives inf / NaN -- loudly.
F16_WEIGHT_EXP = 12
_f16_warned = False


def f16_weight(weight):
    """(weight * 2^k, 2^-k): the f16x3 operand of ``weight`` and the accumulator scale that undoes it."""
    global _f16_warned
    ent = getattr(weight, "_e3d_f16w", None)
    key = weight_key(weight)
    if ent is not None and ent[0] == key:
        return ent[1], ent[2]
    if torch.cuda.is_current_stream_capturing():
        # no host read-back inside a capture, and no silent fallback either: a graph captured with the raw
        # weight would run f16x3 on un-pre-scaled weights at every replay.  The capturers (GraphedReverseStep,
        # GraphedDenoiseStep) run their body eagerly first, which fills this cache; their except-paths fall back to eager
        # launches if this is ever raised.
        raise RuntimeError("f16x3: the pre-scaled copy of a weight is missing inside a stream capture -- run the step eagerly once "
                           "before capturing it (building the copy reads max |w| back to the host)")
    with torch.no_grad():
        amax = float(weight.detach().abs().max())
        if not math.isfinite(amax) or amax == 0.0:
            if not math.isfinite(amax) and not _f16_warned:
                _f16_warned = True
                warnings.warn("f16x3: a weight holds inf / NaN -- used as it is (the outputs will say so)")
            scaled, inv = weight.detach(), 1.0
        else:
            k = max(-120, min(120, F16_WEIGHT_EXP - math.frexp(amax)[1]))
            scaled, inv = (weight.detach() * (2.0 ** k)).contiguous(), 2.0 ** -k
    try:
        weight._e3d_f16w = (key, scaled, inv)
    except AttributeError:
        pass
    return scaled, inv


# Small launches (one to ~16 pockets per step) go to the "skinny" kernels (csrc/gemm_skinny.hip: K cut across
# workgroups so the whole chip streams the weight, partial tiles in a workspace, a second launch finishes the rows).  The
# workspace must not be shared by launches that may run concurrently: one per (device, stream), grown on demand and kept.
# Where they win (tools/lab/skinny_ab.py, graph-timed, K = 768): up to ~768 output tiles of 32x32 -- M = 64: 7.4 us
# against 21-28 us tiled, M = 256: 11 against 23.5, M = 512 x N = 768: 15.5 against 23.8, M = 1024 x N = 768: 21.5
# against 24.2; beyond that the tiled kernels (a 24-step k chain, ~24 us) are faster (M = 512 x N = 2304: 33 vs 24.5).
# E3D_GEMM_SKINNY=0 disables the path (A/B timing).
SKINNY_MAX_M = 1024 if os.environ.get("E3D_GEMM_SKINNY", "1") == "1" else 0
# plain GEMMs (no fused LayerNorm finish) above this many rows take the general kernel's 128x64 four-wave form instead (round 4:
# 18.8 / 23.0 / 19.4 us against 21.6 / 27.1 / 27.5 skinny at M = 1024 for (N, K) = (768, 768) / (768, 1024) / (1024, 768);
# at M = 512 the skinny kernels win two of the three: profiles/r04_gemm_mid_m_ab.log)
SKINNY_GEMM_MAX_M = int(os.environ.get("E3D_GEMM_SKINNY_MAX_M", "512"))
SKINNY_MAX_TILES = 768
_SKINNY_WS = {}
_SKINNY_RETIRED = []


def _skinny_workspace(device, M, N, K):
    nbytes = hip.lib().e3d_gemm_skinny_workspace_bytes(M, N, K)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _SKINNY_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        # (under a graph capture this comes from the graph's private pool and is kept alive here: replay-safe; a workspace
        #  that is outgrown is parked, not freed -- an earlier capture on this stream may have baked its address)
        if ws is not None:
            _SKINNY_RETIRED.append(ws)
        ws = _SKINNY_WS[key] = torch.empty(max(nbytes, 8 << 20), dtype=torch.uint8, device=device)
    return ws


def _skinny_ok(terms, M, N, K, a):
    return (terms in (3, 19) and 0 < M <= SKINNY_MAX_M and N % 32 == 0 and K % 16 == 0 and a.stride(0) % 4 == 0
            and -(-M // 32) * (N // 32) <= SKINNY_MAX_TILES)


def gemm_is_tiled(M, mode=None):
    """Whether ``gemm`` sends a launch of M rows to the tiled split kernels (gemm_split.hip): the only ones that take
    ``plan_m`` / ``run_if``.  (Conservative below the skinny bound: the tile count is not looked at.)"""
    terms = GEMM_MODES[GEMM_MODE if mode is None else mode]
    return terms != 0 and not (terms in (3, 19) and M <= min(SKINNY_MAX_M, SKINNY_GEMM_MAX_M))


def gemm(a, weight, bias=None, act=ACT_NONE, out=None, mode=None, absmax=None, prescale=True, plan_m=None, run_if=None,
         planes_out=False):
    """out[M,N] = act(a[M,K] @ weight[N,K]^T + bias).  ``a`` may be a row-strided 2-D view; its start and row stride must
    stay 16-byte aligned (the kernels load float4s): a view that starts off alignment (``x[:, 1:1+K]``) raises a
    RuntimeError naming the alignment, nothing is copied.  ``absmax`` (1-element
    device tensor, act = none): raised to the largest |out| by the kernel's epilogue (split arithmetics; the exact-f32
    kernels have no use for it -- their attention twin never skips key tiles).  ``prescale`` (f16x3 only): run the
    product on the cached power-of-two-scaled copy of the weight (``f16_weight``); False for weights that change every
    step (the training forward).  ``plan_m`` / ``run_if`` (tiled split kernels only -- ``gemm_is_tiled(plan_m)``; include/e3d_hip.h,
    e3d_gemm_bias_act_f32_split_gated): the kernel form a launch of plan_m rows would take, so that these rows equal the rows of
    that launch bit for bit; a one-int device word that, when zero, turns the launch into an empty dispatch (``out`` is
    then not written).  ``planes_out`` (inference; the caller has asked ``gemm_planes_ok``): the result is returned as
    ``ActPlanes``, the form its one reader -- ``linear_residual_layernorm`` on the row-complete kernel -- consumes."""
    _chk(a, "gemm.a"); _chk(weight, "gemm.weight"); _chk(bias, "gemm.bias")
    assert a.dim() == 2 and a.stride(1) == 1 and weight.is_contiguous()
    M, K = a.shape
    N = weight.shape[0]
    assert weight.shape[1] == K, (a.shape, weight.shape)
    terms = GEMM_MODES[GEMM_MODE if mode is None else mode]
    if planes_out:
        assert out is None and plan_m is None and run_if is None and prescale and terms in (3, 19)
        if absmax is not None:
            _chk(absmax, "gemm.absmax")
            assert act == ACT_NONE and absmax.numel() == 1
        scale = 1.0
        if terms == 19:
            weight, scale = f16_weight(weight)
        out = torch.empty((M * N * 4,), device=a.device, dtype=torch.uint8)
        with _timed("gemm", (M, N, K, act)):
            hip.check(hip.lib().e3d_gemm_bias_act_planes_split(_p(a), a.stride(0), _p(weight), _p(bias), _p(out), M, N, K, act,
                                                               terms, _p(absmax), scale, _stream()),
                      "e3d_gemm_bias_act_planes_split")
        return ActPlanes(out, M, N, terms)
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=torch.float32)
    assert out.dim() == 2 and out.stride(1) == 1 and out.shape == (M, N)
    if absmax is not None:
        _chk(absmax, "gemm.absmax")
        assert act == ACT_NONE and absmax.numel() == 1
    scale = 1.0
    if terms == 19 and prescale:
        weight, scale = f16_weight(weight)
    if plan_m is not None or run_if is not None:
        _chk(run_if, "gemm.run_if", torch.int32)
        plan_m = M if plan_m is None else plan_m
        if not gemm_is_tiled(plan_m, mode):
            raise ValueError(f"gemm: plan_m / run_if exist on the tiled split kernels only (plan_m={plan_m}, mode={mode or GEMM_MODE})")
        # (a launch that may be skipped is kept out of the "gemm" records: their time is set against their flops)
        with _timed("gemm" if run_if is None else "gemm_gated", (M, N, K, act)):
            hip.check(hip.lib().e3d_gemm_bias_act_f32_split_gated(
                _p(a), a.stride(0), _p(weight), _p(bias), _p(out), out.stride(0), M, N, K, act, terms, _p(absmax), scale,
                plan_m, _p(run_if), _stream()), "e3d_gemm_bias_act_f32_split_gated")
        return out
    with _timed("gemm", (M, N, K, act)):
        if _skinny_ok(terms, M, N, K, a) and out.stride(0) % 4 == 0 and M <= min(SKINNY_MAX_M, SKINNY_GEMM_MAX_M):
            ws = _skinny_workspace(a.device, M, N, K)
            hip.check(hip.lib().e3d_gemm_skinny_f32_split_ex(_p(a), a.stride(0), _p(weight), _p(bias), _p(out), out.stride(0),
                                                             M, N, K, act, terms, _p(ws), ws.numel(), _p(absmax), scale, _stream()),
                      "e3d_gemm_skinny_f32_split_ex")
        elif terms == 0:
            hip.check(hip.lib().e3d_gemm_bias_act_f32(_p(a), a.stride(0), _p(weight), _p(bias), _p(out),
                                                      out.stride(0), M, N, K, act, _stream()), "e3d_gemm_bias_act_f32")
        else:
            hip.check(hip.lib().e3d_gemm_bias_act_f32_split_ex(
                _p(a), a.stride(0), _p(weight), _p(bias), _p(out), out.stride(0), M, N, K, act, terms, _p(absmax), scale,
                _stream()), "e3d_gemm_bias_act_f32_split_ex")
    return out


class arithmetic:
    """``with ops.arithmetic("bf16x6"):`` -- GEMM and attention arithmetic for the enclosed calls (entry points use it
    to mirror the precision the reference runs that script at; E3D_GEMM_MODE / E3D_ATTN_MODE in the environment
    win over an entry point's default)."""

    def __init__(self, mode, respect_env=True):
        self.gemm = os.environ.get("E3D_GEMM_MODE", mode) if respect_env else mode
        self.attn = os.environ.get("E3D_ATTN_MODE", self.gemm) if respect_env else mode

    def __enter__(self):
        self.prev = (set_gemm_mode(self.gemm), set_attn_mode(self.attn))
        return self

    def __exit__(self, *exc):
        set_gemm_mode(self.prev[0])
        set_attn_mode(self.prev[1])


ATTN_MODE = os.environ.get("E3D_ATTN_MODE", GEMM_MODE)   # same choices and meaning as GEMM_MODE
if ATTN_MODE == "bf16":
    ATTN_MODE = "bf16x3"
if ATTN_MODE not in GEMM_MODES:
    raise ValueError(f"E3D_ATTN_MODE must be one of {sorted(GEMM_MODES)}, got {ATTN_MODE!r}")


def set_attn_mode(mode):
    global ATTN_MODE
    if mode not in GEMM_MODES:
        raise ValueError(f"attention mode must be one of {sorted(GEMM_MODES)}, got {mode!r}")
    if mode == "bf16":      # the single-product form exists for the GEMMs only
        mode = "bf16x3"
    prev, ATTN_MODE = ATTN_MODE, mode
    return prev


_DROPOUT_EPOCH = {}


def dropout_epoch(device):
    """The device word every dropout launch on ``device`` adds to its seed INSIDE the kernel (created and registered with
    the library on first use: include/e3d_hip.h, e3d_dropout_set_epoch_ptr).  A training step replayed from a HIP graph
    carries the seeds of its capture as baked arguments; it advances this word instead (``training.GraphedStep``), so every
    replay draws fresh decisions while the forward and backward launches of one step still agree."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    t = _DROPOUT_EPOCH.get(idx)
    if t is None:
        t = torch.zeros(1, dtype=torch.int64, device=f"cuda:{idx}")
        with torch.cuda.device(idx):
            hip.check(hip.lib().e3d_dropout_set_epoch_ptr(t.data_ptr()), "e3d_dropout_set_epoch_ptr")
        _DROPOUT_EPOCH[idx] = t
    return t


MAX_DROPOUT_SITES = 1 << 24     # group index = site << 40 | head << 24 | group (include/e3d_hip.h)
MAX_DROPOUT_HEADS = 1 << 16


class KeyedDropout:
    """The keyed dropout decisions of ONE seeded training step ("Keyed sampling streams"): the seed, the epoch
    word and the batch's item ids (both in device memory, where a captured step finds the current ones at every replay),
    the row-key tables built from them -- one launch per (stream, frame length), inside the step -- and the site counter:
    the ordinal of the dropout call within the step, which starts at 0 for every step and is the same on every frame,
    because the model makes the same calls in the same order."""

    def __init__(self, seed, epoch_word, ids):
        self.seed, self.epoch, self.ids = keyed.check_seed(seed), epoch_word, ids
        self.site = 0
        self._tables = {}

    def next_site(self):
        site = self.site
        if site >= MAX_DROPOUT_SITES:
            raise ValueError(f"keyed dropout holds {MAX_DROPOUT_SITES} sites per step")
        self.site = site + 1
        return site

    def row_keys(self, stream, L):
        """uint64 keys of the rows of this batch's [B, L] frame on ``stream`` (keyed.DROP_LIGAND / DROP_POCKET), as int64."""
        t = self._tables.get((stream, L))
        if t is None:
            t = self._tables[(stream, L)] = keyed_drop_row_keys(self.ids, L, self.epoch, self.seed, stream)
        return t


_KEYED_DROPOUT = None


def keyed_dropout_state():
    """The ``KeyedDropout`` of the step being built, or None (torch-seeded dropout)."""
    return _KEYED_DROPOUT


@contextlib.contextmanager
def keyed_dropout(seed, epoch_word, ids):
    """Inside: dropout sites take keyed decisions -- ``next_dropout_seed`` hands out site ordinals (from 0) and makes no
    torch generator call; every site must be given the key table of its rows."""
    global _KEYED_DROPOUT
    prev, _KEYED_DROPOUT = _KEYED_DROPOUT, KeyedDropout(seed, epoch_word, ids)
    try:
        yield _KEYED_DROPOUT
    finally:
        _KEYED_DROPOUT = prev


def next_dropout_seed():
    """A fresh 63-bit seed for one dropout site call, drawn from torch's global CPU generator
    (so ``torch.manual_seed`` makes training runs repeatable).  Inside ``keyed_dropout``: the site's ordinal."""
    if _KEYED_DROPOUT is not None:
        return _KEYED_DROPOUT.next_site()
    return int(torch.randint(0, 2 ** 62, (), dtype=torch.int64))


def site_drop(p, row_keys=None):
    """The ``drop`` value of one dropout site call: (p, seed) from torch's generator, or -- inside ``keyed_dropout`` --
    (p, site, row_keys) with the key table of the rows the site works on (attention: the query rows)."""
    if _KEYED_DROPOUT is None:
        if row_keys is not None:
            raise RuntimeError("row keys given to a dropout site outside ops.keyed_dropout")
        return float(p), next_dropout_seed()
    if row_keys is None:
        raise RuntimeError("a dropout site inside ops.keyed_dropout needs the key table of its rows")
    return float(p), next_dropout_seed(), row_keys


def _keyed_drop(drop, rows, what, heads=1):
    """(p, site, row-key pointer) of a keyed ``drop`` = (p, site, row_keys), checked against the site's rows."""
    p, site, row_keys = drop
    if not 0 <= int(site) < MAX_DROPOUT_SITES:
        raise ValueError(f"{what}: dropout site {site} outside [0, 2^24)")
    if heads >= MAX_DROPOUT_HEADS:
        raise ValueError(f"{what}: keyed dropout holds fewer than 2^16 heads, got {heads}")
    if row_keys.dtype != torch.int64 or not row_keys.is_cuda or not row_keys.is_contiguous() or row_keys.numel() != rows:
        raise ValueError(f"{what}: row keys must be a contiguous int64 device tensor of {rows} keys")
    return float(p), int(site), _p(row_keys)


def keyed_drop_row_keys(ids, L, epoch_word, seed, stream):
    """Row keys of a [B, L] frame for keyed dropout: key[b * L + l] = w0 | w1 << 32 of the Philox words of
    (seed, ids[b], stream, epoch, l) -- int64 [B * L] holding the uint64 bits.  ``ids`` int64 [B] and ``epoch_word`` are
    read on the device."""
    if stream not in (keyed.DROP_LIGAND, keyed.DROP_POCKET):
        raise ValueError(f"dropout row keys live on streams {keyed.DROP_LIGAND} / {keyed.DROP_POCKET}, got {stream}")
    if L > keyed.MAX_POSITION:
        raise ValueError(f"keyed streams hold positions below 2^24, got a frame of {L}")
    B = ids.numel()
    assert ids.dtype == torch.int64 and ids.is_cuda and ids.is_contiguous() and epoch_word.dtype == torch.int64 and epoch_word.is_cuda
    out = torch.empty((B * L,), device=ids.device, dtype=torch.int64)
    hip.check(hip.lib().e3d_keyed_drop_row_keys(_p(ids), B, L, _p(epoch_word), keyed.check_seed(seed), int(stream), _p(out),
                                                _stream()), "e3d_keyed_drop_row_keys")
    return out


def dropout(x, p, seed, out=None, row_keys=None):
    """out = x * keep / (1 - p'): the counter-based dropout of include/e3d_hip.h.  The backward pass is the
    same call on the gradient with the same (p, seed).  ``row_keys`` (keyed decisions): x is [rows, H] with one key per
    row and ``seed`` is the site."""
    _chk(x, "dropout.x")
    assert x.is_contiguous()
    out = torch.empty_like(x) if out is None else out
    if row_keys is not None:
        H = x.shape[-1]
        M = x.numel() // H
        p, site, keys = _keyed_drop((p, seed, row_keys), M, "dropout")
        hip.check(hip.lib().e3d_dropout_f32_keyed(_p(x), p, site, keys, _p(out), M, H, _stream()), "e3d_dropout_f32_keyed")
        return out
    hip.check(hip.lib().e3d_dropout_f32(_p(x), float(p), int(seed), _p(out), x.numel(), _stream()), "e3d_dropout_f32")
    return out


def keyed_attn_dropout_mask(B, nh, Lq, Lk, p, site, row_keys):
    """Test aid: multipliers applied to the attention probabilities by ``attention(..., drop=(p, site, row_keys))``."""
    out = torch.empty((B, nh, Lq, Lk), device=row_keys.device, dtype=torch.float32)
    p, site, keys = _keyed_drop((p, site, row_keys), B * Lq, "keyed_attn_dropout_mask", nh)
    hip.check(hip.lib().e3d_keyed_attn_dropout_mask(B, nh, Lq, Lk, p, site, keys, _p(out), _stream()),
              "e3d_keyed_attn_dropout_mask")
    return out


def attn_dropout_mask(B, nh, Lq, Lk, p, seed, device="cuda"):
    """Test aid: multipliers applied to the attention probabilities by ``attention(..., drop=(p, seed))``."""
    out = torch.empty((B, nh, Lq, Lk), device=device, dtype=torch.float32)
    hip.check(hip.lib().e3d_attn_dropout_mask(B, nh, Lq, Lk, float(p), int(seed), _p(out), _stream()),
              "e3d_attn_dropout_mask")
    return out


def _attn_view(t, L):
    """(pointer, batch stride, row stride) of a [B * L, ...] row-strided view, as the attention entry points take it."""
    rs = t.stride(0)
    return _p(t), L * rs, rs


def _attn_inputs(q, k, v, Lq, Lk, dist_emb, max_pos, key_mask):
    """The arguments every padded-attention entry point, forward or backward, starts with."""
    return (*_attn_view(q, Lq), *_attn_view(k, Lk), *_attn_view(v, Lk), _p(dist_emb), max_pos, _p(key_mask))


def attention(q, k, v, B, nh, Lq, Lk, key_mask=None, dist_emb=None, max_pos=0, want_lse=False, mode=None, drop=None,
              bounds=None, planes_out=False):
    """q [B*Lq, >=nh*64] / k, v [B*Lk, ...] row-strided 2-D views (e.g. slices of a fused QKV
    buffer).  Returns ctx [B*Lq, nh*64] (and lse [B,nh,Lq]).  ``drop`` = (p, seed): dropout on the
    normalised probabilities (training); the exact-fp32 mode then runs its fp32-grade bf16x6 twin.  ``drop`` =
    (p, site, row_keys): keyed decisions, row_keys the table of the [B, Lq] query frame.
    ``bounds`` = (q_absmax, k_absmax): 1-element device tensors bounding |element| of the Q rows and of ALL K rows
    (``gemm(..., absmax=)``); with them the split kernels skip all-padding key tiles when that is provably exact,
    without them every call sweeps all keys.
    ``planes_out`` (inference; the caller has asked ``attention_planes_ok``): ctx is returned as ``ActPlanes``, the form
    its one reader -- ``linear_residual_layernorm`` on the row-complete kernel -- consumes."""
    for n, t in (("q", q), ("k", k), ("v", v), ("key_mask", key_mask), ("dist_emb", dist_emb)):
        _chk(t, "attention." + n)
    assert q.stride(1) == 1 and k.stride(1) == 1 and v.stride(1) == 1
    assert q.shape[0] == B * Lq and k.shape[0] == B * Lk and v.shape[0] == B * Lk
    if key_mask is not None:
        assert key_mask.is_contiguous() and key_mask.shape == (B, Lk)
    if dist_emb is not None:
        assert dist_emb.is_contiguous() and dist_emb.shape == (2 * max_pos - 1, 64), dist_emb.shape
    terms = GEMM_MODES[ATTN_MODE if mode is None else mode]
    if planes_out:
        assert not want_lse and (drop is None or drop[0] <= 0) and terms in (3, 19)
        out = torch.empty((B * Lq * nh * 64 * 4,), device=q.device, dtype=torch.uint8)
    else:
        out = torch.empty((B * Lq, nh * 64), device=q.device, dtype=torch.float32)
    lse = torch.empty((B, nh, Lq), device=q.device, dtype=torch.float32) if want_lse else None
    with _timed("attn_relkey" if dist_emb is not None else "attn_cross", (B, nh, Lq, Lk)):
        inputs = _attn_inputs(q, k, v, Lq, Lk, dist_emb, max_pos, key_mask)
        args = (*inputs, _p(out), _p(lse), B, nh, Lq, Lk)
        dropping = drop is not None and drop[0] > 0
        if terms == 0 and not dropping:
            hip.check(hip.lib().e3d_relkey_attn_fwd(*args, _stream()), "e3d_relkey_attn_fwd")
        else:
            # scratch for the bf16 planes of dist_emb (cooperative kernel): a torch allocation keeps the call
            # free of stream-ordered hipMallocAsync, so the launch sequence can be captured into a HIP graph
            scratch, ready, e_abs = None, 0, None
            q_abs, k_abs = bounds if bounds is not None else (None, None)
            if dist_emb is not None:
                # inference (grad disabled): the planes are kept across calls, keyed by the tensor's version / storage
                infer = not torch.is_grad_enabled()
                ent = getattr(dist_emb, "_e3d_planes", None) if infer else None
                if ent is not None and ent[0] == weight_key(dist_emb) + (Lk, terms):
                    scratch, ready, e_abs = ent[1], 1, ent[2]
                else:
                    scratch = torch.empty((hip.lib().e3d_attn_scratch_bytes(Lk),), device=q.device, dtype=torch.uint8)
                    # training (weights change every step): a pool slot of the table, raised by this call -- never lowered,
                    # so a value from an earlier step is still a bound; inference keeps a scalar of its own with the planes
                    # (a pool slot would be zeroed by the next chain's reset while the cached planes live on)
                    # (the call that writes the planes raises the slot it is given to max |table| itself -- no launch for it -- but
                    #  only a call that carries all three bounds hands the slot over: without them the scalar kept with the cached
                    #  planes is computed here, so that it is a bound for whichever later call re-uses the planes)
                    e_abs = None
                    have_bounds = q_abs is not None and k_abs is not None
                    if have_bounds and not infer:
                        try:
                            e_abs = absmax_slot(dist_emb, "e", q.device)
                        except AttributeError:
                            e_abs = torch.zeros(1, device=q.device, dtype=torch.float32)
                    elif have_bounds:
                        e_abs = torch.zeros(1, device=q.device, dtype=torch.float32)
                    if infer and not torch.cuda.is_current_stream_capturing():
                        try:
                            if e_abs is None:
                                e_abs = absmax(dist_emb.detach())
                            dist_emb._e3d_planes = (weight_key(dist_emb) + (Lk, terms), scratch, e_abs)
                        except AttributeError:
                            pass
            p, seed = (float(drop[0]), int(drop[1])) if dropping else (0.0, 0)
            if q_abs is None or k_abs is None or (dist_emb is not None and e_abs is None):
                q_abs = k_abs = e_abs = None
            if planes_out:
                hip.check(hip.lib().e3d_relkey_attn_fwd_split_planes(*inputs, _p(out), B, nh, Lq, Lk, terms, _p(scratch), ready,
                                                                     _p(q_abs), _p(k_abs), _p(e_abs), _stream()),
                          "e3d_relkey_attn_fwd_split_planes")
                return ActPlanes(out, B * Lq, nh * 64, terms)
            if dropping and len(drop) == 3:
                p, site, keys = _keyed_drop(drop, B * Lq, "attention", nh)
                hip.check(hip.lib().e3d_relkey_attn_fwd_split_ex_keyed(*args, terms or 6, p, site, keys, _p(scratch), ready,
                                                                       _p(q_abs), _p(k_abs), _p(e_abs), _stream()),
                          "e3d_relkey_attn_fwd_split_ex_keyed")
                return (out, lse) if want_lse else out
            hip.check(hip.lib().e3d_relkey_attn_fwd_split_ex(*args, terms or 6, p, seed, _p(scratch), ready, _p(q_abs),
                                                             _p(k_abs), _p(e_abs), _stream()),
                      "e3d_relkey_attn_fwd_split_ex")
    return (out, lse) if want_lse else out


def attention_varlen(q, k, v, q_layout, k_layout, nh, dist_emb=None, max_pos=0, mode=None):
    """Attention over the segments of packed batches (packing.PackedLayout; include/e3d_hip.h, e3d_attn_varlen_fwd).
    q [q_layout.rows, >= nh*64] and k, v [k_layout.rows, ...] are row-strided 2-D views (e.g. slices of a fused QKV
    buffer).  Segment s of the queries attends to segment s of the keys -- a packed buffer, or a padded cache when
    ``k_layout.padded_frame``.  With ``dist_emb`` (rel-key self-attention) both layouts must have the same lengths.
    Returns ctx [q_layout.rows, nh*64]; rows of no segment are zero.  Inference only (no backward exists): raises when
    grad mode is on and an input requires grad -- a call that autograd would have to differentiate.
    Arithmetic (``mode``, default ATTN_MODE): bf16x3 / bf16x6 / f16x3 as ``attention``; "f32" runs the fp32-grade bf16x6
    form here (there is no exact-fp32 varlen kernel), while ``attention`` runs its exact fp32 MFMA kernel -- a packed
    chain under E3D_GEMM_MODE=f32 therefore differs from the padded one by bf16x6 rounding (~1e-6) in attention."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (q, k, v, dist_emb)):
        raise RuntimeError("attention_varlen is inference-only: run it under torch.no_grad()")
    for n, t in (("q", q), ("k", k), ("v", v), ("dist_emb", dist_emb)):
        _chk(t, "attention_varlen." + n)
    assert q.dim() == 2 and q.stride(1) == 1 and k.stride(1) == 1 and v.stride(1) == 1
    if q.shape[0] != q_layout.rows or k.shape[0] != k_layout.rows or v.shape[0] != k_layout.rows:
        raise ValueError(f"attention_varlen: rows q {q.shape[0]} / k {k.shape[0]} / v {v.shape[0]} against layouts of "
                         f"{q_layout.rows} / {k_layout.rows} rows")
    if q_layout.B != k_layout.B:
        raise ValueError(f"attention_varlen: {q_layout.B} query segments against {k_layout.B} key segments")
    if dist_emb is not None:
        assert dist_emb.is_contiguous() and dist_emb.shape == (2 * max_pos - 1, 64), dist_emb.shape
        if not q_layout.same_segments(k_layout):
            raise ValueError("attention_varlen: relative_key self-attention needs q_len == k_len for every segment")
    alloc = torch.zeros if q_layout.padded_frame else torch.empty   # (a packed layout's kernel writes every row)
    out = alloc((q_layout.rows, nh * 64), device=q.device, dtype=torch.float32)
    terms = GEMM_MODES[ATTN_MODE if mode is None else mode]
    if q_layout.n_tiles == 0:
        return out
    with _timed("attn_varlen", (q_layout.B, nh, q_layout.rows, k_layout.rows)):
        hip.check(hip.lib().e3d_attn_varlen_fwd(
            _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(q_layout.start_dev), _p(q_layout.len_dev),
            _p(k_layout.start_dev), _p(k_layout.len_dev), _p(q_layout.tiles), q_layout.n_tiles, _p(dist_emb), max_pos,
            _p(out), q_layout.rows, nh, q_layout.max_len, k_layout.max_len, terms, _stream()), "e3d_attn_varlen_fwd")
    return out


def residual_layernorm(x, residual, gamma, beta, eps, want_s=False, drop=None):
    """LayerNorm(x + residual); ``drop`` = (p, seed): LayerNorm(dropout(x) + residual) with the multipliers of
    ``dropout(x, p, seed)`` applied inside the kernel; (p, site, row_keys): keyed decisions, one key per row of x."""
    for n, t in (("x", x), ("residual", residual), ("gamma", gamma), ("beta", beta)):
        _chk(t, "residual_layernorm." + n)
    assert x.is_contiguous() and (residual is None or residual.is_contiguous())
    M, H = x.shape
    out = torch.empty_like(x)
    s = torch.empty_like(x) if want_s else None
    with _timed("residual_layernorm", (M, H)):
        if drop is not None and drop[0] > 0 and len(drop) == 3:
            p, site, keys = _keyed_drop(drop, M, "residual_layernorm")
            hip.check(hip.lib().e3d_residual_layernorm_drop_fwd_keyed(_p(x), _p(residual), _p(gamma), _p(beta), eps, _p(s), _p(out),
                                                                      M, H, p, site, keys, _stream()),
                      "e3d_residual_layernorm_drop_fwd_keyed")
        elif drop is not None and drop[0] > 0:
            hip.check(hip.lib().e3d_residual_layernorm_drop_fwd(_p(x), _p(residual), _p(gamma), _p(beta), eps, _p(s), _p(out), M, H,
                                                                float(drop[0]), int(drop[1]), _stream()),
                      "e3d_residual_layernorm_drop_fwd")
        else:
            hip.check(hip.lib().e3d_residual_layernorm_fwd(_p(x), _p(residual), _p(gamma), _p(beta), eps, _p(s),
                                                           _p(out), M, H, _stream()), "e3d_residual_layernorm_fwd")
    return (out, s) if want_s else out


# Row-complete GEMM + bias + residual + LayerNorm (csrc/gemm_rowln.hip): BertSelfOutput / BertOutput in ONE launch at large
# M -- a workgroup owns whole 768-wide rows, the pre-norm sum never leaves its registers.  The weight goes in PRE-SPLIT
# into its two 16-bit terms (fragment-order planes, built once per weight version by a small kernel and cached on the
# weight like every derived-weight cache).  From ROWLN_MIN_M rows upwards: measured against the pair in one process
# (tools/lab/rowln_ab.py, f16x3, K = 768 / 1024): M = 65536 257 / 319 us against 323 / 376, M = 32768 137 / 172 against
# 168 / 208, M = 16384 66 / 83 against 84 / 98, M = 8192 41 / 51 against 53 / 61 (one 32-row tile per CU); smaller launches stay
# on the skinny / 128 x 128 forms.  E3D_GEMM_ROWLN=0 switches the path off (A/B runs).
# In inference the kernel's A operand arrives as ACTIVATION PLANES wherever its producer can write them (``ActPlanes`` below:
# the attention context for BertSelfOutput, the GELU intermediate for BertOutput): the split then happens once in the
# producer instead of once per consumer wave -- M = 65536: 259 -> 249 us at K = 768, 328 -> 313 us at K = 1024 inside the
# sampling step, bit-identical (profiles/README.md "Activation planes"; E3D_ACT_PLANES=0 = fp32 rows).
ROWLN_MIN_M = int(os.environ.get("E3D_GEMM_ROWLN_MIN_M", "8192")) if os.environ.get("E3D_GEMM_ROWLN", "1") == "1" else 1 << 62


def weight_planes(weight, terms):
    """(planes, out_scale): ``weight`` [N, K] split into its hi / lo 16-bit terms in MFMA-fragment order
    (e3d_weight_planes_f32_split); for f16x3 the power-of-two-scaled copy is split and its inverse power returned."""
    ent = getattr(weight, "_e3d_planes_w", None)
    key = weight_key(weight) + (terms,)
    if ent is not None and ent[0] == key:
        return ent[1], ent[2]
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("weight_planes: cache miss inside a stream capture (warm the op up before capturing)")
    src, scale = f16_weight(weight) if terms == 19 else (weight.detach(), 1.0)
    N, K = src.shape
    nbytes = hip.lib().e3d_weight_planes_bytes(N, K)
    if nbytes < 0:
        raise ValueError(f"weight_planes: unsupported shape {tuple(src.shape)}")
    planes = torch.empty((nbytes,), dtype=torch.uint8, device=src.device)
    hip.check(hip.lib().e3d_weight_planes_f32_split(_p(src), N, K, terms, _p(planes), _stream()), "e3d_weight_planes_f32_split")
    try:
        weight._e3d_planes_w = (key, planes, scale)
    except AttributeError:
        pass
    return planes, scale


def rowln_ok(terms, M, H, K, a, residual=None):
    """Whether the row-complete kernel takes this call: its staging needs A (and the residual) 16-byte aligned, so a view
    that starts off alignment goes to the pair instead.  ``a`` None: A will come as planes (a fresh allocation)."""
    return (terms in (3, 19) and M >= ROWLN_MIN_M and (a is None or (a.stride(1) == 1 and a.data_ptr() % 16 == 0))
            and (residual is None or (residual.stride(1) == 1 and residual.stride(0) % 4 == 0 and residual.data_ptr() % 16 == 0))
            and bool(hip.lib().e3d_gemm_residual_layernorm_supported(M, H, K, K if a is None else a.stride(0))))


# Activation planes (csrc/gemm_rowln.hip): in inference the A operand of a row-complete launch is written
# by exactly one kernel and read by nobody else, so the producer stores it as the consumer's MFMA fragments -- the two 16-bit
# split terms, [32-row block][k16 step][plane][lane] x 16 B, byte for byte what every wave of the consumer would otherwise
# form from the fp32 rows (eight times per element) -- and the results are bit-identical.  Producers: the 4-wave
# cooperative attention kernel (BertSelfOutput's input) and the persistent GEMM (GELU: BertOutput's input).  E3D_ACT_PLANES=0 restores the fp32 launches (A/B runs).
# (E3D_ACT_PLANES=gemm / attn: that producer only)
ACT_PLANES = {"1": True, "0": False, "gemm": "gemm", "attn": "attn"}.get(os.environ.get("E3D_ACT_PLANES", "1"))
if ACT_PLANES is None:
    raise ValueError(f"E3D_ACT_PLANES must be 1, 0, gemm or attn, got {os.environ['E3D_ACT_PLANES']!r}")
ACT_PLANES_CALLS = 0     # row-complete launches that read planes (tests: the path was taken)


class ActPlanes:
    """An [M, K] activation in the plane format: ``data`` is the uint8 buffer (M K 4 bytes), ``terms`` the split (3 / 19)."""
    __slots__ = ("data", "shape", "terms")
    requires_grad = False

    def __init__(self, data, M, K, terms):
        self.data, self.shape, self.terms = data, (M, K), terms

    @property
    def device(self):
        return self.data.device

    def decode(self):
        """(hi, lo) as [M, K] fp16 / bf16 tensors (tests, debugging): the layout read back by index arithmetic."""
        M, K = self.shape
        dt = torch.float16 if self.terms == 19 else torch.bfloat16
        t = self.data.view(dt).view(M // 32, K // 16, 2, 2, 32, 8)      # [rb][ks][plane][lane >> 5][lane & 31][j]
        t = t.permute(2, 0, 4, 1, 3, 5).reshape(2, M, K)
        return t[0], t[1]


def activation_planes(x, mode=None):
    """``x`` [M, K] fp32 (row-strided) -> ActPlanes, by the kernel that defines the format."""
    _chk(x, "activation_planes.x")
    M, K = x.shape
    terms = GEMM_MODES[GEMM_MODE if mode is None else mode]
    nbytes = hip.lib().e3d_activation_planes_bytes(M, K)
    if nbytes < 0 or terms not in (3, 19) or x.stride(1) != 1:
        raise ValueError(f"activation_planes: unsupported shape {tuple(x.shape)} / terms {terms}")
    out = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    hip.check(hip.lib().e3d_activation_planes_f32_split(_p(x), x.stride(0), M, K, terms, _p(out), _stream()),
              "e3d_activation_planes_f32_split")
    return ActPlanes(out, M, K, terms)


def gemm_planes_ok(a, weight, bias, act, out_features, residual=None, mode=None):
    """Decided BEFORE the GEMM launch: whether ``gemm(a, weight, bias, act)`` may leave as planes -- the consumer
    (``linear_residual_layernorm`` with ``out_features`` columns and this residual) takes the row-complete kernel, the GEMM
    lands on the persistent kernel, and nothing needs gradients."""
    if ACT_PLANES not in (True, "gemm") or torch.is_grad_enabled():
        return False
    terms = GEMM_MODES[GEMM_MODE if mode is None else mode]
    M, K = a.shape
    N = weight.shape[0]
    return (terms in (3, 19) and rowln_ok(terms, M, out_features, N, None, residual) and a.stride(1) == 1
            and a.data_ptr() % 16 == 0 and (bias is None or bias.data_ptr() % 16 == 0)
            and not (_skinny_ok(terms, M, N, K, a) and M <= min(SKINNY_MAX_M, SKINNY_GEMM_MAX_M))
            and bool(hip.lib().e3d_gemm_planes_supported(M, N, K, a.stride(0), act, terms)))


def attention_planes_ok(q, k, v, nh, Lq, Lk, out_features, residual=None, mode=None):
    """Decided BEFORE the attention launch: whether its context may leave as planes -- the consumer
    (``linear_residual_layernorm`` with ``out_features`` columns and this residual) takes the row-complete kernel, the
    attention lands on the 4-wave cooperative kernel, both run the same split, and nothing needs gradients."""
    if ACT_PLANES not in (True, "attn") or torch.is_grad_enabled():
        return False
    terms = GEMM_MODES[ATTN_MODE if mode is None else mode]
    if terms != GEMM_MODES[GEMM_MODE] or terms not in (3, 19):
        return False
    return (rowln_ok(terms, q.shape[0], out_features, nh * 64, None, residual) and v.stride(1) == 1 and k.stride(1) == 1
            and bool(hip.lib().e3d_attn_planes_supported(k.stride(0), Lk * v.stride(0), v.stride(0), Lq, Lk, terms, 1)))


def linear_residual_layernorm(a, weight, bias, residual, gamma, beta, eps, mode=None):
    """LayerNorm(a @ weight^T + bias + residual) * gamma + beta  (BertSelfOutput / BertOutput in eval mode).  Large M: the
    row-complete kernel (one launch, no pre-norm tensor); small M: the second launch of the skinny GEMM does the row
    finish (bit-identical to gemm + residual_layernorm); otherwise the pair."""
    M, K = a.shape
    H = weight.shape[0]
    terms = GEMM_MODES[GEMM_MODE if mode is None else mode]
    if isinstance(a, ActPlanes):
        global ACT_PLANES_CALLS
        if a.terms != terms or not rowln_ok(terms, M, H, K, None, residual):
            raise RuntimeError(f"linear_residual_layernorm: no kernel reads activation planes at M={M} H={H} K={K} terms={terms}")
        _chk(a.data, "linear_residual_layernorm.a", torch.uint8)
        for t, n in ((weight, "weight"), (bias, "bias"), (residual, "residual"), (gamma, "gamma"), (beta, "beta")):
            _chk(t, "linear_residual_layernorm." + n)
        assert weight.is_contiguous() and weight.shape[1] == K and (residual is None or residual.shape == (M, H))
        planes, scale = weight_planes(weight, terms)
        out = torch.empty((M, H), device=a.device, dtype=torch.float32)
        with _timed("gemm_layernorm", (M, H, K)):
            hip.check(hip.lib().e3d_gemm_residual_layernorm_planes_split(
                _p(a.data), _p(planes), _p(bias), _p(residual), residual.stride(0) if residual is not None else 0,
                _p(gamma), _p(beta), eps, _p(out), out.stride(0), M, H, K, terms, scale, _stream()),
                "e3d_gemm_residual_layernorm_planes_split")
        ACT_PLANES_CALLS += 1
        return out
    if rowln_ok(terms, M, H, K, a, residual):
        for t, n in ((a, "a"), (weight, "weight"), (bias, "bias"), (residual, "residual"), (gamma, "gamma"), (beta, "beta")):
            _chk(t, "linear_residual_layernorm." + n)
        assert weight.is_contiguous() and weight.shape[1] == K and (residual is None or residual.shape == (M, H))
        planes, scale = weight_planes(weight, terms)
        out = torch.empty((M, H), device=a.device, dtype=torch.float32)
        with _timed("gemm_layernorm", (M, H, K)):
            hip.check(hip.lib().e3d_gemm_residual_layernorm_f32_split(
                _p(a), a.stride(0), _p(planes), _p(bias), _p(residual), residual.stride(0) if residual is not None else 0,
                _p(gamma), _p(beta), eps, _p(out), out.stride(0), M, H, K, terms, scale, _stream()),
                "e3d_gemm_residual_layernorm_f32_split")
        return out
    if not (_skinny_ok(terms, M, H, K, a) and H in (256, 512, 768, 1024) and a.stride(1) == 1):
        return residual_layernorm(gemm(a, weight, bias, mode=mode), residual, gamma, beta, eps)
    for t, n in ((a, "a"), (weight, "weight"), (bias, "bias"), (residual, "residual"), (gamma, "gamma"), (beta, "beta")):
        _chk(t, "linear_residual_layernorm." + n)
    assert weight.is_contiguous() and weight.shape[1] == K and (residual is None or (residual.is_contiguous() and residual.shape == (M, H)))
    out = torch.empty((M, H), device=a.device, dtype=torch.float32)
    ws = _skinny_workspace(a.device, M, H, K)
    scale = 1.0
    if terms == 19:
        weight, scale = f16_weight(weight)
    with _timed("gemm_layernorm", (M, H, K)):
        hip.check(hip.lib().e3d_gemm_skinny_residual_layernorm_f32_split_ex(
            _p(a), a.stride(0), _p(weight), _p(bias), _p(residual), _p(gamma), _p(beta), eps, _p(out), M, H, K, terms,
            _p(ws), ws.numel(), scale, _stream()), "e3d_gemm_skinny_residual_layernorm_f32_split_ex")
    return out

def adaln_gate(x, y, mod, branch, rows_per_cond):
    for n, t in (("x", x), ("y", y), ("mod", mod)):
        _chk(t, "adaln_gate." + n)
    assert x.is_contiguous() and y.is_contiguous() and mod.is_contiguous()
    M, H = x.shape
    assert mod.shape[1] == 6 * H and mod.shape[0] * rows_per_cond == M, (mod.shape, M, rows_per_cond)
    out = torch.empty_like(x)
    with _timed("adaln_gate", (M, H)):
        hip.check(hip.lib().e3d_adaln_gate_fwd(_p(x), _p(y), _p(mod), branch, rows_per_cond, _p(out),
                                               M, H, _stream()), "e3d_adaln_gate_fwd")
    return out


def adaln_gate_indexed(x, y, idx, table, mod, branch):
    """``adaln_gate`` (rows_per_cond = 1) with row r's modulation taken from ``table[idx[r]]`` ([rows, 6H]) where idx[r]
    names a table row, from ``mod[r]`` ([M, 6H]) elsewhere."""
    for n, t in (("x", x), ("y", y), ("table", table), ("mod", mod)):
        _chk(t, "adaln_gate_indexed." + n)
    _chk(idx, "adaln_gate_indexed.idx", torch.int32)
    assert x.is_contiguous() and y.is_contiguous() and mod.is_contiguous() and table.is_contiguous() and idx.is_contiguous()
    M, H = x.shape
    assert y.shape == x.shape and mod.shape == (M, 6 * H) and table.shape[1] == 6 * H and idx.shape == (M,), (mod.shape, table.shape, idx.shape)
    out = torch.empty_like(x)
    with _timed("adaln_gate", (M, H)):
        hip.check(hip.lib().e3d_adaln_gate_indexed_fwd(_p(x), _p(y), _p(idx), _p(table), table.shape[0], _p(mod), branch,
                                                       _p(out), M, H, _stream()), "e3d_adaln_gate_indexed_fwd")
    return out


def classify_onehot_rows(x, flag=None):
    """(idx int32 [M], flag int32 [1]) of x [M, F <= 32]: idx[m] = k for a row that is exactly 1.0 at k and zero elsewhere,
    F for an all-zero row, -1 for any other row (NaN included); ``flag`` (zeroed here when not given) is raised when any row
    got -1.  No host synchronisation."""
    _chk(x, "classify_onehot_rows.x")
    assert x.dim() == 2 and x.is_contiguous()
    M, F = x.shape
    if flag is None:
        flag = torch.zeros(1, device=x.device, dtype=torch.int32)
    _chk(flag, "classify_onehot_rows.flag", torch.int32)
    idx = torch.empty(M, device=x.device, dtype=torch.int32)
    with _timed("classify_onehot", (M, F)):
        hip.check(hip.lib().e3d_classify_onehot_rows(_p(x), F, _p(idx), _p(flag), M, _stream()), "e3d_classify_onehot_rows")
    return idx, flag


def embed_layernorm(x, weight, bias, gamma, beta, eps, post_add=None, rows_per_add=1, want_z=False, run_if=None):
    for n, t in (("x", x), ("weight", weight), ("bias", bias), ("gamma", gamma), ("beta", beta),
                 ("post_add", post_add)):
        _chk(t, "embed_layernorm." + n)
    assert x.is_contiguous() and weight.is_contiguous()
    M, F = x.shape
    H = weight.shape[0]
    assert weight.shape[1] == F
    if post_add is not None:
        assert post_add.is_contiguous() and post_add.shape == (M // rows_per_add, H)
    out = torch.empty((M, H), device=x.device, dtype=torch.float32)
    z = torch.empty_like(out) if want_z else None
    _chk(run_if, "embed_layernorm.run_if", torch.int32)
    with _timed("embed_layernorm", (M, H)):   # run_if: as in ``gemm``
        hip.check(hip.lib().e3d_embed_layernorm_fwd_ex(_p(x), F, _p(weight), _p(bias), _p(gamma), _p(beta), eps,
                                                       _p(post_add), rows_per_add, _p(z), _p(out), M, H, _p(run_if),
                                                       _stream()), "e3d_embed_layernorm_fwd_ex")
    return (out, z) if want_z else out


def head_linear(x, weight, bias):
    for n, t in (("x", x), ("weight", weight), ("bias", bias)):
        _chk(t, "head_linear." + n)
    assert x.is_contiguous() and weight.is_contiguous()
    M, H = x.shape
    n_out = weight.shape[0]
    out = torch.empty((M, n_out), device=x.device, dtype=torch.float32)
    hip.check(hip.lib().e3d_head_linear_fwd(_p(x), _p(weight), _p(bias), _p(out), M, H, n_out, _stream()),
              "e3d_head_linear_fwd")
    return out


def _chk_update(name, x, eps_hat, noise, coef_table, width, t_dev, out):
    """The operand checks the continuous updates share: the DDPM update (a [T, ``width`` 4] table; ``coef_table`` and
    ``t_dev`` None in the scalar form) and the strided one (8).  Returns ``out``, allocated like ``x`` when None."""
    for n, t in (("x", x), ("eps_hat", eps_hat), ("noise", noise), ("coef_table", coef_table)):
        _chk(t, f"{name}.{n}")
    _chk(t_dev, name + ".t_dev", torch.int64)
    assert x.is_contiguous() and eps_hat.is_contiguous() and eps_hat.shape == x.shape
    assert noise is None or (noise.is_contiguous() and noise.shape == x.shape)
    assert coef_table is None or (coef_table.is_contiguous() and coef_table.dim() == 2 and coef_table.shape[1] == width)
    return torch.empty_like(x) if out is None else out


def ddpm_step_wrap(x, eps_hat, noise, sqrt_recip_alpha, beta, sqrt_one_minus_ab, sigma, wrap=True, out=None):
    out = _chk_update("ddpm_step_wrap", x, eps_hat, noise, None, 4, None, out)
    with _timed("ddpm_step_wrap"):
        hip.check(hip.lib().e3d_ddpm_step_wrap(_p(x), _p(eps_hat), _p(noise), sqrt_recip_alpha, beta,
                                               sqrt_one_minus_ab, sigma, int(wrap), _p(out), x.numel(), _stream()),
                  "e3d_ddpm_step_wrap")
    return out


def ddpm_step_wrap_table(x, eps_hat, noise, coef_table, t_dev, wrap=True, out=None):
    """ddpm_step_wrap with the step index on the device (``t_dev`` int64, first element) and the four
    coefficients in ``coef_table`` [T,4]: nothing host-side changes between steps (HIP-graph replay)."""
    out = _chk_update("ddpm_step_wrap_table", x, eps_hat, noise, coef_table, 4, t_dev, out)
    with _timed("ddpm_step_wrap"):
        hip.check(hip.lib().e3d_ddpm_step_wrap_table(_p(x), _p(eps_hat), _p(noise), _p(coef_table), _p(t_dev), int(wrap),
                                                     _p(out), x.numel(), _stream()), "e3d_ddpm_step_wrap_table")
    return out


def strided_step_wrap(x, eps_hat, noise, coef_table, t_dev, wrap=True, wrap_x0=False, out=None):
    """The strided (DDIM / respaced) update t -> successor(t): x0 form with the coefficients in row ``t_dev[0]`` of
    ``coef_table`` [T,8] (structure_model.utils.StridedTables.coef).  ``noise`` None: no noise term; a row with
    sigma == 0 reads nothing through ``noise``.  ``wrap_x0``: wrap the x0 estimate to [-pi, pi).  ``out`` may be ``x``."""
    out = _chk_update("strided_step_wrap", x, eps_hat, noise, coef_table, 8, t_dev, out)
    with _timed("strided_step_wrap"):
        hip.check(hip.lib().e3d_strided_step_wrap(_p(x), _p(eps_hat), _p(noise), _p(coef_table), _p(t_dev),
                                                  coef_table.shape[0], int(wrap), int(wrap_x0), _p(out), x.numel(),
                                                  _stream()), "e3d_strided_step_wrap")
    return out


def multistep_step_wrap(x, eps_hat, hist, coef_table, t_dev, wrap=True, wrap_x0=False, out=None):
    """The second-order multistep update t -> successor(t) (DPM-Solver++ 2M, capped weight): the strided update at
    eta == 0 plus c_1 * (x0 - hist), with the coefficients in row ``t_dev[0]`` of ``coef_table`` [T,8]
    (structure_model.utils.MultistepTables.coef).  ``hist``: the x0 estimate the previous step stored, like ``x``; it is
    updated in place with this step's estimate, and a row with c_1 == 0 does not read it.  ``wrap``: the difference of the
    two estimates is taken on the circle, like the state.  Draws nothing.  ``out`` may be ``x``; returns ``out``."""
    out = _chk_update("multistep_step_wrap", x, eps_hat, None, coef_table, 8, t_dev, out)
    _chk(hist, "multistep_step_wrap.hist")
    assert hist is not None and hist.is_contiguous() and hist.shape == x.shape
    assert hist.data_ptr() != out.data_ptr() and hist.data_ptr() != x.data_ptr()
    with _timed("multistep_step_wrap"):
        hip.check(hip.lib().e3d_multistep_step_wrap(_p(x), _p(eps_hat), _p(hist), _p(coef_table), _p(t_dev),
                                                    coef_table.shape[0], int(wrap), int(wrap_x0), _p(out), _p(hist),
                                                    x.numel(), _stream()), "e3d_multistep_step_wrap")
    return out


def q_sample_wrap(x0, noise, t, sqrt_ab, sqrt_1mab):
    for n, tt in (("x0", x0), ("noise", noise), ("sqrt_ab", sqrt_ab), ("sqrt_1mab", sqrt_1mab)):
        _chk(tt, "q_sample_wrap." + n)
    _chk(t, "q_sample_wrap.t", torch.int64)
    assert x0.is_contiguous() and noise.is_contiguous() and t.is_contiguous()
    B = x0.shape[0]
    out = torch.empty_like(x0)
    hip.check(hip.lib().e3d_q_sample_wrap(_p(x0), _p(noise), _p(t), _p(sqrt_ab), _p(sqrt_1mab), _p(out),
                                          B, x0.numel() // B, _stream()), "e3d_q_sample_wrap")
    return out


def _chk_posterior(xt_idx, logits, qsb, qtb):
    """The operand checks the four posterior launches share; returns B, L, C and the int32 [B,L] output."""
    _chk(xt_idx, "xt_idx", torch.int32); _chk(logits, "logits"); _chk(qsb, "qsb"); _chk(qtb, "qtb")
    B, L, C = logits.shape
    assert xt_idx.is_contiguous() and logits.is_contiguous() and qsb.is_contiguous() and qtb.is_contiguous()
    assert qsb.shape == (B, C, C) and qtb.shape == (B, C, C) and xt_idx.shape == (B, L)
    return B, L, C, torch.empty((B, L), device=logits.device, dtype=torch.int32)


_POSTERIOR_ENTRIES = {(False, False): "e3d_discrete_posterior_sample", (True, False): "e3d_keyed_discrete_posterior_sample",
                      (False, True): "e3d_discrete_posterior_sample_ctl",
                      (True, True): "e3d_keyed_discrete_posterior_sample_ctl"}      # (keyed?, controls?)


def _posterior(name, xt_idx, logits, qsb, qtb, u=None, want_prob=False, keyed_draw=None, ctl=None):
    """The launch behind the four posterior wrappers, ``name`` the caller's.  ``keyed_draw`` = (row_keys, seed, s_dev):
    the keyed entry point (a categorical draw, no ``prob``), else the one that reads ``u``; ``ctl`` = (bias, inv_temp):
    the design-control form of either."""
    if ctl is not None:      # the check first: it speaks for a bias that is no tensor
        inv_temp = _chk_ctl(logits, *ctl, name)
        ctl = (_p(ctl[0]), inv_temp)
    B, L, C, out = _chk_posterior(xt_idx, logits, qsb, qtb)
    prob = torch.empty((B, L, C), device=logits.device, dtype=torch.float32) if want_prob else None
    if keyed_draw is None:
        _chk(u, "u")
        draw = (_p(u), 0 if u is None else 1, _p(out), _p(prob))
    else:
        row_keys, seed, s_dev = keyed_draw
        _chk(s_dev, "s_dev", torch.int64)
        _chk_keys(row_keys, B * L, name)
        draw = (_p(row_keys), keyed.check_seed(seed), _p(s_dev), _p(out))
    entry = _POSTERIOR_ENTRIES[keyed_draw is not None, ctl is not None]
    with _timed("discrete_posterior"):
        hip.check(getattr(hip.lib(), entry)(_p(xt_idx), _p(logits), *(ctl or ()), _p(qsb), _p(qtb), *draw, B, L, C,
                                            _stream()), entry)
    return (out, prob) if want_prob else out


def discrete_posterior_sample(xt_idx, logits, qsb, qtb, u=None, want_prob=False):
    """xt_idx int32 [B,L]; logits [B,L,C]; qsb/qtb [B,C,C]; u [B,L] uniforms or None (argmax)."""
    return _posterior("discrete_posterior_sample", xt_idx, logits, qsb, qtb, u, want_prob)


def discrete_q_sample(x0_idx, qtb, u=None):
    """x0_idx int32 [B,L] (-1 = padding row); qtb [B,C,C]; u [B,L] uniforms or None (argmax)."""
    _chk(x0_idx, "x0_idx", torch.int32); _chk(qtb, "qtb"); _chk(u, "u")
    B, L = x0_idx.shape
    C = qtb.shape[-1]
    assert x0_idx.is_contiguous() and qtb.is_contiguous() and qtb.shape == (B, C, C)
    out = torch.empty((B, L), device=qtb.device, dtype=torch.int32)
    with _timed("discrete_q_sample"):
        hip.check(hip.lib().e3d_discrete_q_sample(_p(x0_idx), _p(qtb), _p(u), 0 if u is None else 1, _p(out),
                                                  B, L, C, _stream()), "e3d_discrete_q_sample")
    return out


# ---------------------------------------------------------------------------------------------- keyed (seeded) draws
# Row-key tables come from keyed.py: int64 [rows, 2] = (item id, position), position < 0 for rows of no item.

def _chk_keys(row_keys, rows, name):
    _chk(row_keys, name + ".row_keys", torch.int64)
    if not (row_keys.is_contiguous() and row_keys.dim() == 2 and row_keys.shape == (rows, 2)):
        raise ValueError(f"{name}: row_keys must be a contiguous [{rows}, 2] table, got {tuple(row_keys.shape)}")


def _keyed_rows(name, x, row_keys, table):
    """The geometry of a keyed launch on ``x`` [.., F]: (rows, F) with rows = x.numel() // F, F % 4 == 0, one key per row;
    ``table`` is read by the step index, which a keyed stream holds up to 65535."""
    F = x.shape[-1]
    if F % 4:
        raise ValueError(f"{name}: the feature count must be a multiple of 4, got {F}")
    rows = x.numel() // F
    _chk_keys(row_keys, rows, name)
    if table.shape[0] - 1 > 65535:
        raise ValueError(f"{name}: keyed streams hold steps up to 65535, the table has {table.shape[0]}")
    return rows, F


def keyed_ddpm_step_wrap(x, eps_hat, coef_table, t_dev, row_keys, seed, wrap=True, out=None):
    """ddpm_step_wrap_table with the N(0,1) draw generated in the kernel from (seed, row key, stream 1, t_dev[0]):
    x / eps_hat [.., F] with rows = x.numel() // F, F % 4 == 0.  No noise buffer, no host sync: graph-capturable."""
    out = _chk_update("keyed_ddpm_step_wrap", x, eps_hat, None, coef_table, 4, t_dev, out)
    rows, F = _keyed_rows("keyed_ddpm_step_wrap", x, row_keys, coef_table)
    with _timed("keyed_ddpm_step_wrap"):
        hip.check(hip.lib().e3d_keyed_ddpm_step_wrap(_p(x), _p(eps_hat), _p(coef_table), _p(t_dev), _p(row_keys),
                                                     keyed.check_seed(seed), int(wrap), _p(out), rows, F, _stream()),
                  "e3d_keyed_ddpm_step_wrap")
    return out


def keyed_strided_step_wrap(x, eps_hat, coef_table, t_dev, row_keys, seed, wrap=True, wrap_x0=False, out=None):
    """strided_step_wrap with the N(0,1) draw generated in the kernel from (seed, row key, stream 1, t_dev[0]) -- the
    draws of keyed_ddpm_step_wrap at the same step; x / eps_hat [.., F], rows = x.numel() // F, F % 4 == 0."""
    out = _chk_update("keyed_strided_step_wrap", x, eps_hat, None, coef_table, 8, t_dev, out)
    rows, F = _keyed_rows("keyed_strided_step_wrap", x, row_keys, coef_table)
    with _timed("keyed_strided_step_wrap"):
        hip.check(hip.lib().e3d_keyed_strided_step_wrap(_p(x), _p(eps_hat), _p(coef_table), _p(t_dev), coef_table.shape[0],
                                                        _p(row_keys), keyed.check_seed(seed), int(wrap), int(wrap_x0),
                                                        _p(out), rows, F, _stream()), "e3d_keyed_strided_step_wrap")
    return out


def keyed_discrete_posterior_sample(xt_idx, logits, qsb, qtb, row_keys, seed, s_dev):
    """discrete_posterior_sample (categorical draw) with the uniforms from (seed, row key, stream 3, s_dev[0]);
    row_keys [B * L, 2]."""
    return _posterior("keyed_discrete_posterior_sample", xt_idx, logits, qsb, qtb, keyed_draw=(row_keys, seed, s_dev))


# ------------------------------------------------------------------------------------------ sequence design controls
# The posterior and the last step's pick over the effective logits (logits + bias) * inv_temp (design.DesignControls).

def _chk_ctl(logits, bias, inv_temp, name):
    """The checks the design-control launches share; returns inv_temp as a Python float (an exact fp32 value)."""
    _chk(logits, name + ".logits"); _chk(bias, name + ".bias")
    if logits.dim() != 3 or not logits.is_contiguous():
        raise ValueError(f"{name}: logits must be contiguous [B, L, C], got {tuple(logits.shape)}")
    if bias is not None and not (bias.is_contiguous() and bias.shape == logits.shape):
        raise ValueError(f"{name}: bias must be contiguous and of the logits' shape {tuple(logits.shape)}, got "
                         f"{tuple(bias.shape)}")
    inv_temp = float(inv_temp)
    if not (0.0 < inv_temp < float("inf")):
        raise ValueError(f"{name}: inv_temp must be positive and finite, got {inv_temp}")
    return inv_temp


def discrete_posterior_sample_ctl(xt_idx, logits, bias, inv_temp, qsb, qtb, u=None, want_prob=False):
    """discrete_posterior_sample with the softmax over (logits + bias) * inv_temp: bias contiguous [B,L,C] (-inf forbids
    a class) or None for zero; inv_temp > 0."""
    return _posterior("discrete_posterior_sample_ctl", xt_idx, logits, qsb, qtb, u, want_prob, ctl=(bias, inv_temp))


def keyed_discrete_posterior_sample_ctl(xt_idx, logits, bias, inv_temp, qsb, qtb, row_keys, seed, s_dev):
    """keyed_discrete_posterior_sample with the softmax over (logits + bias) * inv_temp; stream 3, the same counters."""
    return _posterior("keyed_discrete_posterior_sample_ctl", xt_idx, logits, qsb, qtb, keyed_draw=(row_keys, seed, s_dev),
                      ctl=(bias, inv_temp))


def discrete_final_pick(logits, bias=None, inv_temp=1.0, want_scores=True):
    """The last step's pick on logits [B,L,C]: (idx int32 [B,L], logp [B,L], entropy [B,L]) -- the first maximum of
    (logits + bias) * inv_temp, its log-probability under the softmax of those, and that softmax's entropy; a row whose
    classes are all forbidden gives index 0 and NaN scores.  ``want_scores`` False: (idx, None, None)."""
    inv_temp = _chk_ctl(logits, bias, inv_temp, "discrete_final_pick")
    B, L, C = logits.shape
    idx = torch.empty((B, L), device=logits.device, dtype=torch.int32)
    logp = torch.empty((B, L), device=logits.device, dtype=torch.float32) if want_scores else None
    ent = torch.empty((B, L), device=logits.device, dtype=torch.float32) if want_scores else None
    if B * L:
        with _timed("discrete_final_pick"):
            hip.check(hip.lib().e3d_discrete_final_pick(_p(logits), _p(bias), inv_temp, _p(idx), _p(logp), _p(ent), B * L, C,
                                                        _stream()), "e3d_discrete_final_pick")
    return idx, logp, ent


# ------------------------------------------------------------------------ partial redesign (replacement conditioning)
# Held ligand positions are overwritten in place after the update of a step, by launches of their own on its stream.

def _chk_known(x, x0, mask, name):
    _chk(x, name + ".x"); _chk(x0, name + ".x0"); _chk(mask, name + ".mask", torch.uint8)
    if not (x.is_contiguous() and x0.is_contiguous() and mask.is_contiguous()):
        raise ValueError(f"{name}: x, x0 and mask must be contiguous")
    if x0.shape != x.shape or mask.shape != x.shape:
        raise ValueError(f"{name}: x {tuple(x.shape)}, x0 {tuple(x0.shape)} and mask {tuple(mask.shape)} must agree")


def _chk_levels(level_table, t_dev, name):
    _chk(level_table, name + ".level_table"); _chk(t_dev, name + ".t_dev", torch.int64)
    if not (level_table.is_contiguous() and level_table.dim() == 2 and level_table.shape[1] == 2):
        raise ValueError(f"{name}: level_table must be a contiguous [T, 2] table, got {tuple(level_table.shape)}")


def known_compose_wrap(x, x0, mask, noise, level_table, t_dev, scale=1.0):
    """In place on ``x``: where ``mask`` (uint8, x's shape) is set, x = the forward-noised copy of ``x0`` at the level
    row ``t_dev[0]`` of ``level_table`` [T,2] names (structure_model.utils.KnownLevels.levels) with the N(0,1) draws
    ``noise`` -- wrap(a x0 + s1m wrap(scale noise)); x0 itself at the clean level (s1m == 0).  ``noise`` None at a noisy
    level, a NaN row or a step index outside the table: the held elements become NaN.  Returns ``x``."""
    _chk_known(x, x0, mask, "known_compose_wrap")
    _chk_levels(level_table, t_dev, "known_compose_wrap")
    _chk(noise, "known_compose_wrap.noise")
    if noise is not None and not (noise.is_contiguous() and noise.shape == x.shape):
        raise ValueError("known_compose_wrap: noise must be contiguous and of x's shape")
    if x.numel():
        with _timed("known_compose_wrap"):
            hip.check(hip.lib().e3d_known_compose_wrap(_p(x), _p(x0), _p(mask), _p(noise), _p(level_table), _p(t_dev),
                                                       level_table.shape[0], float(scale), x.numel(), _stream()),
                      "e3d_known_compose_wrap")
    return x


def keyed_known_compose_wrap(x, x0, mask, level_table, t_dev, row_keys, seed, scale=1.0):
    """known_compose_wrap with the draws generated in the kernel from (seed, row key, stream 10, t_dev[0]); x [.., F],
    rows = x.numel() // F, F % 4 == 0.  Rows of no item are left alone."""
    _chk_known(x, x0, mask, "keyed_known_compose_wrap")
    _chk_levels(level_table, t_dev, "keyed_known_compose_wrap")
    rows, F = _keyed_rows("keyed_known_compose_wrap", x, row_keys, level_table)
    with _timed("keyed_known_compose_wrap"):
        hip.check(hip.lib().e3d_keyed_known_compose_wrap(_p(x), _p(x0), _p(mask), _p(level_table), _p(t_dev),
                                                         level_table.shape[0], float(scale), _p(row_keys),
                                                         keyed.check_seed(seed), rows, F, _stream()),
                  "e3d_keyed_known_compose_wrap")
    return x


def _discrete_known_compose(name, idx, x0_idx, mask, qsb, u=None, keyed_draw=None):
    """The launch behind the two wrappers, ``name`` the caller's: ``keyed_draw`` = (row_keys, seed, s_dev) takes the keyed
    entry point, else the one that reads ``u``."""
    _chk(idx, name + ".idx", torch.int32); _chk(x0_idx, name + ".x0_idx", torch.int32)
    _chk(mask, name + ".mask", torch.uint8); _chk(qsb, name + ".qsb")
    if idx.dim() != 2 or x0_idx.shape != idx.shape or mask.shape != idx.shape:
        raise ValueError(f"{name}: idx {tuple(idx.shape)}, x0_idx {tuple(x0_idx.shape)} and mask {tuple(mask.shape)} must be "
                         "the same [B, L]")
    B, L = idx.shape
    C = qsb.shape[-1]
    if qsb.shape != (B, C, C):
        raise ValueError(f"{name}: qsb must be [{B}, C, C], got {tuple(qsb.shape)}")
    if not (idx.is_contiguous() and x0_idx.is_contiguous() and mask.is_contiguous() and qsb.is_contiguous()):
        raise ValueError(f"{name}: arguments must be contiguous")
    if keyed_draw is None:
        _chk(u, name + ".u")
        if u is not None and not (u.is_contiguous() and u.numel() == B * L):
            raise ValueError(f"{name}: u must be contiguous [B, L]")
        entry, draw = "e3d_discrete_known_compose", (_p(u), 0 if u is None else 1)
    else:
        row_keys, seed, s_dev = keyed_draw
        _chk(s_dev, name + ".s_dev", torch.int64)
        _chk_keys(row_keys, B * L, name)
        entry, draw = "e3d_keyed_discrete_known_compose", (_p(row_keys), keyed.check_seed(seed), _p(s_dev))
    with _timed("discrete_known_compose"):
        hip.check(getattr(hip.lib(), entry)(_p(idx), _p(x0_idx), _p(mask), _p(qsb), *draw, B, L, C, _stream()), entry)
    return idx


def discrete_known_compose(idx, x0_idx, mask, qsb, u=None):
    """In place on ``idx`` int32 [B,L]: a row with ``mask`` (uint8) set and x0_idx >= 0 is redrawn from column x0_idx of
    ``qsb`` [B,C,C] -- discrete_q_sample's law; u [B,L] uniforms or None (argmax).  Returns ``idx``."""
    return _discrete_known_compose("discrete_known_compose", idx, x0_idx, mask, qsb, u)


def keyed_discrete_known_compose(idx, x0_idx, mask, qsb, row_keys, seed, s_dev):
    """discrete_known_compose (categorical draw) with the uniforms from (seed, row key, stream 11, s_dev[0]);
    row_keys [B * L, 2]."""
    return _discrete_known_compose("keyed_discrete_known_compose", idx, x0_idx, mask, qsb,
                                   keyed_draw=(row_keys, seed, s_dev))


# ------------------------------------------------------------------------------------------ scoring supplied sequences
# N = levels x items rows of tables per launch (sequence_model/sample.py::score_sequences).

def keyed_discrete_forward_levels(x0_idx, qtb, row_keys, level_steps, seed, max_step):
    """z_t int32 [N,L] of N items at their own levels: row (n, l) drawn from column x0_idx[n, l] (int32, -1 = padding row)
    of ``qtb`` [N,C,C] with the uniform of (seed, row key, stream 11, level_steps[n]); ``level_steps`` int64 [N] on the
    device, every entry in [0, max_step].  Rows of no item get class 0.  For equal steps this is
    keyed_discrete_known_compose with a full mask."""
    name = "keyed_discrete_forward_levels"
    _chk(x0_idx, name + ".x0_idx", torch.int32); _chk(qtb, name + ".qtb"); _chk(level_steps, name + ".level_steps", torch.int64)
    if x0_idx.dim() != 2:
        raise ValueError(f"{name}: x0_idx must be [N, L], got {tuple(x0_idx.shape)}")
    N, L = x0_idx.shape
    C = qtb.shape[-1]
    if qtb.shape != (N, C, C) or level_steps.shape != (N,):
        raise ValueError(f"{name}: qtb must be [{N}, C, C] and level_steps [{N}], got {tuple(qtb.shape)} and "
                         f"{tuple(level_steps.shape)}")
    if not (x0_idx.is_contiguous() and qtb.is_contiguous() and level_steps.is_contiguous()):
        raise ValueError(f"{name}: arguments must be contiguous")
    if not 0 <= int(max_step) <= keyed.MAX_STEP:
        raise ValueError(f"{name}: keyed streams hold steps up to {keyed.MAX_STEP}, got max_step={max_step}")
    if L > keyed.MAX_POSITION:
        raise ValueError(f"{name}: keyed streams hold positions below 2^24, got a frame of {L}")
    _chk_keys(row_keys, N * L, name)
    out = torch.empty((N, L), device=qtb.device, dtype=torch.int32)
    with _timed("discrete_forward_levels"):
        hip.check(hip.lib().e3d_keyed_discrete_forward_levels(_p(x0_idx), _p(qtb), _p(row_keys), _p(level_steps), int(max_step),
                                                              keyed.check_seed(seed), _p(out), N, L, C, _stream()),
                  "e3d_keyed_discrete_forward_levels")
    return out


def discrete_score_rows(xt_idx, x0_idx, logits, qsb, qtb, is_final, want_probs=False):
    """(term, nll) float [N,L] of rows whose clean class is known: nll = -log_softmax(logits)[x0]; term = KL(q || p) in
    nats with p the posterior of discrete_posterior_sample (want_prob) and q the same expression under the one-hot of
    x0; items with ``is_final`` (uint8 [N]) set have term = nll and never read their tables.  Rows with x0_idx < 0: NaN.
    ``want_probs``: (term, nll, p, q) with p, q [N,L,C]."""
    name = "discrete_score_rows"
    N, L, C, _ = _chk_posterior(xt_idx, logits, qsb, qtb)
    _chk(x0_idx, name + ".x0_idx", torch.int32); _chk(is_final, name + ".is_final", torch.uint8)
    if x0_idx.shape != (N, L) or is_final.shape != (N,) or not (x0_idx.is_contiguous() and is_final.is_contiguous()):
        raise ValueError(f"{name}: x0_idx must be a contiguous [{N}, {L}] and is_final a contiguous [{N}], got "
                         f"{tuple(x0_idx.shape)} and {tuple(is_final.shape)}")
    term = torch.empty((N, L), device=logits.device, dtype=torch.float32)
    nll = torch.empty_like(term)
    p = torch.empty((N, L, C), device=logits.device, dtype=torch.float32) if want_probs else None
    q = torch.empty_like(p) if want_probs else None
    with _timed("discrete_score_rows"):
        hip.check(hip.lib().e3d_discrete_score_rows(_p(xt_idx), _p(x0_idx), _p(logits), _p(qsb), _p(qtb), _p(is_final), _p(term),
                                                    _p(nll), _p(p), _p(q), N, L, C, _stream()), "e3d_discrete_score_rows")
    return (term, nll, p, q) if want_probs else (term, nll)


def masked_item_sums(values, mask):
    """(sums float [N], counts int32 [N]) of values [N,L] over mask (uint8 [N,L]) != 0, in a fixed reduction shape: the
    same bits for an item whatever its padding or batch.  Masked-out values are not read into the sum (NaN allowed)."""
    name = "masked_item_sums"
    _chk(values, name + ".values"); _chk(mask, name + ".mask", torch.uint8)
    if values.dim() != 2 or mask.shape != values.shape or not (values.is_contiguous() and mask.is_contiguous()):
        raise ValueError(f"{name}: values and mask must be the same contiguous [N, L], got {tuple(values.shape)} and "
                         f"{tuple(mask.shape)}")
    N, L = values.shape
    sums = torch.zeros((N,), device=values.device, dtype=torch.float32)
    counts = torch.zeros((N,), device=values.device, dtype=torch.int32)
    if N * L:
        with _timed("masked_item_sums"):
            hip.check(hip.lib().e3d_masked_item_sums(_p(values), _p(mask), _p(sums), _p(counts), N, L, _stream()),
                      "e3d_masked_item_sums")
    return sums, counts


# ----------------------------------------------------------------------------------------- scoring supplied structures
# N = levels x items per launch, level-major (structure_model/sample.py::score_structures).

def _chk_level_steps(level_steps, B, name):
    """``level_steps`` int64 [N] on the device, N a positive multiple of B; returns N."""
    _chk(level_steps, name + ".level_steps", torch.int64)
    if level_steps.dim() != 1 or not level_steps.is_contiguous() or level_steps.numel() == 0 or level_steps.numel() % B:
        raise ValueError(f"{name}: level_steps must be a contiguous [N] with N a positive multiple of the {B} items, got "
                         f"{tuple(level_steps.shape)}")
    return level_steps.numel()


def keyed_q_sample_levels_wrap(x0, row_keys, level_steps, sqrt_ab, sqrt_1mab, scale, seed, max_step):
    """(noise, x_t) float [N, L, F] of N = n * B items at their own levels: item i is item i % B of ``x0`` [B, L, F] (and of
    ``row_keys`` [B * L, 2]) at timestep ``level_steps[i]`` (int64 [N] on the device, every entry in [0, max_step]), noise =
    wrap(scale * z) with z the normals of (seed, row key, stream 12, that step), x_t = wrap(sqrt_ab[t] x0 + sqrt_1mab[t]
    noise) -- q_sample_wrap's arithmetic.  Rows of no item get zeros, an item with a step outside the tables NaN."""
    name = "keyed_q_sample_levels_wrap"
    for n, tt in (("x0", x0), ("sqrt_ab", sqrt_ab), ("sqrt_1mab", sqrt_1mab)):
        _chk(tt, f"{name}.{n}")
    if x0.dim() != 3 or x0.shape[-1] % 4 or not x0.is_contiguous() or x0.numel() == 0:
        raise ValueError(f"{name}: x0 must be a contiguous [B, L, F] with F a multiple of 4, got {tuple(x0.shape)}")
    B, L, F = x0.shape
    N = _chk_level_steps(level_steps, B, name)
    if not (sqrt_ab.is_contiguous() and sqrt_1mab.is_contiguous() and sqrt_ab.dim() == 1 and sqrt_ab.shape == sqrt_1mab.shape
            and sqrt_ab.numel() > 0):
        raise ValueError(f"{name}: sqrt_ab and sqrt_1mab must be contiguous [T] tables of one length")
    if not 0 <= int(max_step) <= keyed.MAX_STEP:
        raise ValueError(f"{name}: keyed streams hold steps up to {keyed.MAX_STEP}, got max_step={max_step}")
    if L > keyed.MAX_POSITION:
        raise ValueError(f"{name}: keyed streams hold positions below 2^24, got a frame of {L}")
    _chk_keys(row_keys, B * L, name)
    noise = torch.empty((N, L, F), device=x0.device, dtype=torch.float32)
    x_t = torch.empty_like(noise)
    with _timed("keyed_q_sample_levels_wrap"):
        hip.check(hip.lib().e3d_keyed_q_sample_levels_wrap(_p(x0), _p(row_keys), _p(level_steps), int(max_step), _p(sqrt_ab),
                                                           _p(sqrt_1mab), sqrt_ab.shape[0], float(scale),
                                                           keyed.check_seed(seed), _p(noise), _p(x_t), N, B, L, F, _stream()),
                  "e3d_keyed_q_sample_levels_wrap")
    return noise, x_t


def angle_score_items(eps_hat, eps, mask, level_steps, coef, want_elements=False):
    """The score terms of N = n * B items and their fixed-shape sums: ``eps_hat``, ``eps`` float [N, L, F]; ``mask`` uint8
    [B, L, F], per element, read as item i % B; ``level_steps`` int64 [N] on the device; ``coef`` [T, 4] = ScoreTables.coef.
    Returns a dict: ``res_term`` / ``res_err2`` [N, L], ``feat_term`` / ``feat_err2`` [N, F], ``tot_term`` / ``tot_err2``
    [N], ``counts`` int32 [N] -- sums over the masked elements of term = h wrap(k (eps_hat - eps))^2 + add and of
    wrap(eps - eps_hat)^2, the same bits for an item whatever its padding or batch -- and, with ``want_elements``,
    ``term`` / ``err`` [N, L, F].  An item with a step outside [0, T): NaN."""
    name = "angle_score_items"
    _chk(eps_hat, name + ".eps_hat"); _chk(eps, name + ".eps"); _chk(mask, name + ".mask", torch.uint8); _chk(coef, name + ".coef")
    if eps_hat.dim() != 3 or eps.shape != eps_hat.shape or not (eps_hat.is_contiguous() and eps.is_contiguous()) \
            or eps_hat.numel() == 0:
        raise ValueError(f"{name}: eps_hat and eps must be the same contiguous [N, L, F], got {tuple(eps_hat.shape)} and "
                         f"{tuple(eps.shape)}")
    N, L, F = eps_hat.shape
    if F % 4 or F > 32:
        raise ValueError(f"{name}: the feature count must be a multiple of 4 in [4, 32], got {F}")
    if mask.dim() != 3 or mask.shape[1:] != (L, F) or mask.shape[0] == 0 or not mask.is_contiguous():
        raise ValueError(f"{name}: mask must be a contiguous [B, {L}, {F}], got {tuple(mask.shape)}")
    if _chk_level_steps(level_steps, mask.shape[0], name) != N:
        raise ValueError(f"{name}: {level_steps.numel()} level_steps for {N} items")
    if not (coef.is_contiguous() and coef.dim() == 2 and coef.shape[1] == 4 and coef.shape[0] > 0):
        raise ValueError(f"{name}: coef must be a contiguous [T, 4] table, got {tuple(coef.shape)}")
    dev = eps_hat.device
    out = {"res_term": (N, L), "res_err2": (N, L), "feat_term": (N, F), "feat_err2": (N, F), "tot_term": (N,), "tot_err2": (N,)}
    if want_elements:
        out.update(term=(N, L, F), err=(N, L, F))
    out = {k: torch.empty(shape, device=dev, dtype=torch.float32) for k, shape in out.items()}
    out["counts"] = torch.empty((N,), device=dev, dtype=torch.int32)
    with _timed("angle_score_items"):
        hip.check(hip.lib().e3d_angle_score_items(_p(eps_hat), _p(eps), _p(mask), _p(level_steps), _p(coef), coef.shape[0],
                                                  _p(out.get("term")), _p(out.get("err")), _p(out["res_term"]),
                                                  _p(out["res_err2"]), _p(out["feat_term"]), _p(out["feat_err2"]),
                                                  _p(out["tot_term"]), _p(out["tot_err2"]), _p(out["counts"]), N,
                                                  mask.shape[0], L, F, _stream()), "e3d_angle_score_items")
    return out


KEYED_NORMAL, KEYED_UNIFORM, KEYED_ONEHOT, KEYED_CLASS = 0, 1, 2, 3


def keyed_draws(row_keys, seed, stream, t, kind, width=0, wrap=False, scale=1.0):
    """Raw keyed draws of (stream, step t) for every row of ``row_keys`` (rows of no item: zeros).  ``kind``:
    KEYED_NORMAL -> float [rows, width] (wrap: wrap_[-pi,pi)(scale * z)); KEYED_UNIFORM -> float [rows];
    KEYED_ONEHOT -> float [rows, width] one-hot of a class in [0, width); KEYED_CLASS -> int32 [rows]."""
    _chk(row_keys, "keyed_draws.row_keys", torch.int64)
    rows = row_keys.shape[0]
    _chk_keys(row_keys, rows, "keyed_draws")
    if not 0 <= int(t) <= 65535:
        raise ValueError(f"keyed_draws: step {t} outside [0, 65535]")
    if kind == KEYED_NORMAL and width % 4:
        raise ValueError(f"keyed_draws: the feature count must be a multiple of 4, got {width}")
    shape, dtype = {KEYED_NORMAL: ((rows, width), torch.float32), KEYED_UNIFORM: ((rows,), torch.float32),
                    KEYED_ONEHOT: ((rows, width), torch.float32), KEYED_CLASS: ((rows,), torch.int32)}[kind]
    out = torch.empty(shape, device=row_keys.device, dtype=dtype)
    if rows:
        hip.check(hip.lib().e3d_keyed_draws(_p(row_keys), keyed.check_seed(seed), int(stream), int(t), int(kind), int(width),
                                            int(wrap), float(scale), _p(out), rows, _stream()), "e3d_keyed_draws")
    return out


def keyed_initial_angles(row_keys, seed, F, scale=1.0):
    """Keyed structure x_T: wrap_[-pi,pi)(scale * z), z the stream-0 normals, [rows, F]."""
    return keyed_draws(row_keys, seed, keyed.STRUCT_XT, 0, KEYED_NORMAL, F, wrap=True, scale=scale)


def keyed_initial_onehot(row_keys, seed, C):
    """Keyed sequence x_T: one-hot of the stream-2 class of every row, float [rows, C]."""
    return keyed_draws(row_keys, seed, keyed.SEQ_XT, 0, KEYED_ONEHOT, C)


# ------------------------------------------------------------------------------- keyed training and validation draws
# ``item_ids`` int64 [B] and ``epoch`` (an int64 scalar tensor, keyed.epoch_word) are read on the device by the kernels:
# a captured training step replays them with the static batch's ids and whatever the epoch word holds.

def _chk_ids_epoch(item_ids, epoch, B, name):
    _chk(item_ids, name + ".item_ids", torch.int64)
    _chk(epoch, name + ".epoch", torch.int64)
    if not (item_ids.is_contiguous() and item_ids.shape == (B,)):
        raise ValueError(f"{name}: item_ids must be a contiguous int64 [{B}], got {tuple(item_ids.shape)}")
    if epoch.numel() != 1:
        raise ValueError(f"{name}: the epoch is one int64 on the device, got {tuple(epoch.shape)}")


def keyed_timesteps(item_ids, epoch, seed, stream, C):
    """int64 [B] timesteps in [0, C): stream keyed.TRAIN_STRUCT_T (C = T) or keyed.TRAIN_SEQ_T (C = T + 1)."""
    if stream not in (keyed.TRAIN_STRUCT_T, keyed.TRAIN_SEQ_T):
        raise ValueError(f"keyed_timesteps: stream {stream} is not a timestep stream")
    if not 1 <= int(C) <= 1 << 24:
        raise ValueError(f"keyed_timesteps: class count {C}")
    B = item_ids.shape[0]
    _chk_ids_epoch(item_ids, epoch, B, "keyed_timesteps")
    out = torch.empty((B,), device=item_ids.device, dtype=torch.int64)
    with _timed("keyed_timesteps"):
        hip.check(hip.lib().e3d_keyed_timesteps(_p(item_ids), _p(epoch), keyed.check_seed(seed), int(stream), int(C),
                                                _p(out), B, _stream()), "e3d_keyed_timesteps")
    return out


def keyed_q_sample_wrap(x0, t, sqrt_ab, sqrt_1mab, scale, item_ids, epoch, seed):
    """(known_noise, x_t) of q_sample_wrap with the noise wrap(scale * z) drawn in the kernel from stream 5:
    x0 [B, L, F], F % 4 == 0; t int64 [B] on the device."""
    for n, tt in (("x0", x0), ("sqrt_ab", sqrt_ab), ("sqrt_1mab", sqrt_1mab)):
        _chk(tt, "keyed_q_sample_wrap." + n)
    _chk(t, "keyed_q_sample_wrap.t", torch.int64)
    if x0.dim() != 3 or x0.shape[-1] % 4:
        raise ValueError(f"keyed_q_sample_wrap: x0 must be [B, L, F] with F a multiple of 4, got {tuple(x0.shape)}")
    B, L, F = x0.shape
    if L > keyed.MAX_POSITION:
        raise ValueError(f"keyed streams hold positions below 2^24, got a frame of {L}")
    _chk_ids_epoch(item_ids, epoch, B, "keyed_q_sample_wrap")
    assert x0.is_contiguous() and t.is_contiguous() and t.shape == (B,)
    assert sqrt_ab.is_contiguous() and sqrt_1mab.is_contiguous() and sqrt_ab.shape == sqrt_1mab.shape and sqrt_ab.dim() == 1
    noise, x_t = torch.empty_like(x0), torch.empty_like(x0)
    with _timed("keyed_q_sample_wrap"):
        hip.check(hip.lib().e3d_keyed_q_sample_wrap(_p(x0), _p(t), _p(sqrt_ab), _p(sqrt_1mab), sqrt_ab.shape[0], float(scale),
                                                    _p(item_ids), _p(epoch), keyed.check_seed(seed), _p(noise), _p(x_t),
                                                    B, L, F, _stream()), "e3d_keyed_q_sample_wrap")
    return noise, x_t


def keyed_discrete_q_sample(x0_idx, qtb, item_ids, epoch, seed):
    """discrete_q_sample (categorical draw) with the uniform of (b, l) from stream 7 of (item_ids[b], epoch, l)."""
    _chk(x0_idx, "x0_idx", torch.int32); _chk(qtb, "qtb")
    B, L = x0_idx.shape
    C = qtb.shape[-1]
    if L > keyed.MAX_POSITION:
        raise ValueError(f"keyed streams hold positions below 2^24, got a frame of {L}")
    _chk_ids_epoch(item_ids, epoch, B, "keyed_discrete_q_sample")
    assert x0_idx.is_contiguous() and qtb.is_contiguous() and qtb.shape == (B, C, C)
    out = torch.empty((B, L), device=qtb.device, dtype=torch.int32)
    with _timed("discrete_q_sample"):
        hip.check(hip.lib().e3d_keyed_discrete_q_sample(_p(x0_idx), _p(qtb), _p(item_ids), _p(epoch), keyed.check_seed(seed),
                                                        _p(out), B, L, C, _stream()), "e3d_keyed_discrete_q_sample")
    return out


# ---------------------------------------------------------------------------------------------- sequence alignment
# csrc/seq_align.hip.  Queries longer than 32 residues hand a strip's last row on through a workspace of 1 MiB slots, one
# per wave in flight: as many as there are (long query, 64 targets) items, 1024 at the most.  It is a plain allocation
# of the call, handed back to torch's allocator on return (stream-ordered, so the launch that uses it is safe); calls
# whose queries all fit one strip fetch none.
ALIGN_SLOT_BYTES = 1 << 20
ALIGN_STRIP = 32


def align_pairs(q_codes, q_off, t_codes, t_off, subst, gap_open=11, gap_extend=1, upper_only=False, out=None,
                long_queries=None):
    """Local alignment (Smith-Waterman, affine gaps) of every query with every target: ``e3d_align_pairs`` as it is.
    q_codes / t_codes u8 (indices into ``AA_VOCAB``, packed), q_off / t_off i32 [n+1], subst i8 [20,20]; returns
    (score, matches, columns), i32 [Q,T] each -- or fills ``out``, three contiguous i32 [Q,T] tensors.  Bad sequences
    give -2 and, with ``upper_only``, pairs t <= q give -1 (include/e3d_hip.h).  Targets are taken in the order given.
    ``long_queries``: how many queries are longer than 32 residues, when the caller knows (True: some).  0 / False: no
    workspace is fetched, and a longer query would count as a bad sequence; None: every query may be, unless all
    codes together fit one strip."""
    _chk(q_codes, "q_codes", torch.uint8); _chk(t_codes, "t_codes", torch.uint8); _chk(subst, "subst", torch.int8)
    _chk(q_off, "q_off", torch.int32); _chk(t_off, "t_off", torch.int32)
    Q, T = q_off.numel() - 1, t_off.numel() - 1
    assert all(x.is_contiguous() for x in (q_codes, q_off, t_codes, t_off, subst)) and subst.numel() == 400
    dev = q_codes.device
    if out is None:
        out = tuple(torch.empty((Q, T), device=dev, dtype=torch.int32) for _ in range(3))
    for o in out:
        _chk(o, "out", torch.int32)
        assert o.is_contiguous() and tuple(o.shape) == (Q, T), (o.shape, o.stride())
    if long_queries is None:
        long_queries = q_codes.numel() > ALIGN_STRIP
    n_long = Q if long_queries is True else min(int(long_queries), Q)
    ws = torch.empty(hip.lib().e3d_align_workspace_bytes(n_long, T), dtype=torch.uint8, device=dev) if n_long else None
    hip.check(hip.lib().e3d_align_pairs(_p(q_codes), _p(q_off), _p(t_codes), _p(t_off), _p(subst), *(_p(o) for o in out),
                                        _p(ws), 0 if ws is None else ws.numel(), Q, T, q_codes.numel(), t_codes.numel(),
                                        int(gap_open), int(gap_extend), int(bool(upper_only)), _stream()),
              "e3d_align_pairs")
    return tuple(out)
