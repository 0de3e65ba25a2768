"""Activation planes: the A operand of the row-complete GEMM + LayerNorm kernel written by its producer in the form the
kernel consumes (``ops.ActPlanes``).

An [M, K] fp32 activation is stored as its two 16-bit split terms in MFMA-fragment order,

    planes[((rb * (K / 16) + ks) * 2 + plane) * 1024 + lane * 16 + 2 j] = term_plane(X[32 rb + (lane & 31)][16 ks + 8 (lane >> 5) + j]),

the terms being exactly those ``gemm_rowln_kernel`` forms from fp32 rows: hi = round16(x), lo = round16(x - hi), in fp16
(f16x3) or bf16 (bf16x3).  Nothing of this may change a bit of a result, so every check is bitwise:

* ``test_gemm_planes_*``: the persistent GEMM's plane output (act none / GELU, bias, ``out_scale`` != 1) decoded on the host
  against the split of its fp32 output;
* ``test_attention_planes_*``: the cooperative attention kernel's plane output against the split of its fp32 output (rel-key
  with padded keys, cross attention, tile skip on and off);
* ``test_rowln_from_planes``: the row-complete kernel fed planes against the same kernel fed the fp32 rows (every tile form:
  32 / 64 / 96 rows and the 96 + 96 + 64 walk of one workgroup, with and without a residual, rows scaled by 1e3 / 1e-3);
* ``test_structure_layers_end_to_end``: one encoder + one decoder layer of the structure model at M = 8192 (the row-complete
  threshold) with ``ops.ACT_PLANES`` on and off, and a counter that shows the plane path was taken.

The host decode is ``_decode`` below: a view and a permutation, written from the layout formula above.
"""
import math

import pytest
import torch

from helpers import seeded_state_dict, synthetic_pockets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [("f16x3", torch.float16), ("bf16x3", torch.bfloat16)]


def g(seed):
    return torch.Generator().manual_seed(seed)


def _decode(buf, M, K, dt):
    """(hi, lo) [M, K] from the plane bytes: [rb][ks][plane][lane >> 5][lane & 31][j] -> row 32 rb + (lane & 31),
    column 16 ks + 8 (lane >> 5) + j."""
    t = buf.view(dt).view(M // 32, K // 16, 2, 2, 32, 8).permute(2, 0, 4, 1, 3, 5).reshape(2, M, K)
    return t[0], t[1]


def _split(x, dt):
    """The 2-term split of the kernels: hi = round(x), lo = round(x - hi), both round-to-nearest-even in ``dt``."""
    hi = x.to(dt)
    return hi, (x - hi.float()).to(dt)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def _assert_planes_are_split_of(planes, x, dt):
    M, K = x.shape
    assert planes.shape == (M, K) and planes.data.numel() == M * K * 4
    hi, lo = _decode(planes.data, M, K, dt)
    want_hi, want_lo = _split(x, dt)
    assert _same_bits(hi, want_hi), "hi plane"
    assert _same_bits(lo, want_lo), "lo plane"


# ------------------------------------------------------------------------------------------------ the format itself
@pytest.mark.parametrize("mode,dt", MODES)
def test_activation_planes_kernel_matches_the_documented_layout(pkg, hip, mode, dt):
    """``e3d_activation_planes_f32_split`` (the format's definition as a kernel) against the host formula, on a row-strided
    input whose values span normal, fp16-subnormal-lo and large magnitudes; ``ActPlanes.decode`` is the same permutation."""
    M, K = 96, 80
    x_full = torch.randn(M, K + 16, generator=g(1)).to(DEV)
    x_full[5] *= 1e3
    x_full[40] *= 1e-3
    x = x_full[:, :K]
    planes = pkg.ops.activation_planes(x, mode=mode)
    _assert_planes_are_split_of(planes, x, dt)
    hi, lo = planes.decode()
    assert _same_bits(hi, _split(x, dt)[0]) and _same_bits(lo, _split(x, dt)[1])


# ------------------------------------------------------------------------------------------------ GEMM -> planes
@pytest.fixture
def persistent_gemm(pkg, hip, monkeypatch):
    """Every tiled launch on the persistent 256x256 kernel, whatever its tile count; nothing on the skinny (split-K) kernels."""
    monkeypatch.setattr(pkg.ops, "SKINNY_GEMM_MAX_M", 0)
    prev = hip.e3d_gemm_kernel_select(5)
    yield
    hip.e3d_gemm_kernel_select(prev)


@pytest.mark.parametrize("K", [32, 96, 768])
@pytest.mark.parametrize("N", [256, 1024])
@pytest.mark.parametrize("M", [256, 768])
@pytest.mark.parametrize("mode,dt", MODES)
def test_gemm_planes_equal_split_of_fp32_output(pkg, hip, persistent_gemm, mode, dt, M, N, K):
    """act = none and GELU with a bias; M = 768 at N = 256 gives a workgroup stream of one tile each on three workgroups, at
    N = 1024 twelve tiles.  (f16x3 runs on the power-of-two-scaled weight: out_scale != 1 in every f16x3 case.)"""
    a = torch.randn(M, K, generator=g(M + N + K)).to(DEV)
    w = (torch.randn(N, K, generator=g(N + K)) / math.sqrt(K)).to(DEV).contiguous()
    b = torch.randn(N, generator=g(7)).to(DEV)
    assert hip.e3d_gemm_planes_supported(M, N, K, K, 0, pkg.ops.GEMM_MODES[mode])
    for act in (pkg.ops.ACT_NONE, pkg.ops.ACT_GELU):
        want = pkg.ops.gemm(a, w, b, act, mode=mode)
        got = pkg.ops.gemm(a, w, b, act, mode=mode, planes_out=True)
        assert torch.isfinite(want).all()
        _assert_planes_are_split_of(got, want, dt)


@pytest.mark.parametrize("factor", [1024.0 * 3, 1.0 / 4096])
def test_gemm_planes_with_out_scale(pkg, hip, persistent_gemm, factor):
    """A weight far from the fp16 sweet spot: ``f16_weight`` rescales it and the kernel multiplies the sums by 2^-k != 1
    before the bias; also a row-strided A and the largest |out| (act = none) raised by the plane epilogue."""
    M, N, K = 768, 256, 96
    a_full = torch.randn(M, K + 32, generator=g(21)).to(DEV)
    a = a_full[:, :K]
    w = (torch.randn(N, K, generator=g(22)) * factor).to(DEV).contiguous()
    b = (torch.randn(N, generator=g(23)) * factor).to(DEV)
    assert pkg.ops.f16_weight(w)[1] != 1.0
    for act in (pkg.ops.ACT_NONE, pkg.ops.ACT_GELU):
        want = pkg.ops.gemm(a, w, b, act, mode="f16x3")
        got = pkg.ops.gemm(a, w, b, act, mode="f16x3", planes_out=True)
        assert torch.isfinite(want).all()
        _assert_planes_are_split_of(got, want, torch.float16)
    amax = torch.zeros(1, device=DEV)
    pkg.ops.gemm(a, w, b, mode="f16x3", planes_out=True, absmax=amax)
    assert float(amax) == float(pkg.ops.gemm(a, w, b, mode="f16x3").abs().max())


def test_gemm_planes_refused_where_no_kernel_writes_them(pkg, hip):
    """M = 128 is no whole 256-row tile: the predicate says no and the entry point fails instead of storing fp32."""
    assert not hip.e3d_gemm_planes_supported(128, 256, 96, 96, 0, 19)
    a, w = torch.randn(128, 96, device=DEV), torch.randn(256, 96, device=DEV)
    with pytest.raises(RuntimeError):
        pkg.ops.gemm(a, w, None, mode="f16x3", planes_out=True)


# ------------------------------------------------------------------------------------------------ attention -> planes
def _attention_case(relkey):
    B, nh = 2, 3
    if relkey:
        Lq = Lk = 128
        qkv = torch.randn(B * Lq, 3 * nh * 64, generator=g(11))
        q, k, v = qkv[:, :nh * 64], qkv[:, nh * 64:2 * nh * 64], qkv[:, 2 * nh * 64:]
        mask = torch.ones(B, Lk)
        mask[:, Lk - 40:] = 0.0                               # the last 40 keys are padding
        dist = torch.randn(2 * Lq - 1, 64, generator=g(12)) * 0.5
        return B, nh, Lq, Lk, qkv, None, mask, dist
    Lq, Lk = 128, 96
    q = torch.randn(B * Lq, nh * 64, generator=g(13))
    kv = torch.randn(B * Lk, 2 * nh * 64, generator=g(14))
    return B, nh, Lq, Lk, q, kv, None, None


@pytest.mark.parametrize("skip", [1, 0])
@pytest.mark.parametrize("relkey", [True, False])
@pytest.mark.parametrize("mode,dt", MODES)
def test_attention_planes_equal_split_of_fp32_output(pkg, hip, monkeypatch, mode, dt, relkey, skip):
    B, nh, Lq, Lk, q_src, kv_src, mask, dist = _attention_case(relkey)
    H = nh * 64
    q_src = q_src.to(DEV)
    kv_src = kv_src.to(DEV) if kv_src is not None else None
    q, k, v = (q_src[:, :H], q_src[:, H:2 * H], q_src[:, 2 * H:]) if kv_src is None else (q_src, kv_src[:, :H], kv_src[:, H:])
    mask = mask.to(DEV) if mask is not None else None
    dist = dist.to(DEV).contiguous() if dist is not None else None
    bounds = (pkg.ops.absmax(q.contiguous()), pkg.ops.absmax(k.contiguous()))    # with bounds the padded key tile may be skipped
    terms = pkg.ops.GEMM_MODES[mode]
    assert hip.e3d_attn_planes_supported(k.stride(0), Lk * v.stride(0), v.stride(0), Lq, Lk, terms, 1)
    prev = hip.e3d_attn_skip_padded_tiles(skip)
    try:
        with torch.no_grad():
            kw = dict(key_mask=mask, dist_emb=dist, max_pos=Lq if relkey else 0, mode=mode, bounds=bounds)
            want = pkg.ops.attention(q, k, v, B, nh, Lq, Lk, **kw)
            got = pkg.ops.attention(q, k, v, B, nh, Lq, Lk, planes_out=True, **kw)
    finally:
        hip.e3d_attn_skip_padded_tiles(prev)
    assert isinstance(got, pkg.ops.ActPlanes) and got.terms == terms and torch.isfinite(want).all()
    _assert_planes_are_split_of(got, want, dt)


def test_attention_planes_refused_where_no_kernel_writes_them(pkg, hip):
    """Lq = 96 (three query tiles: the per-wave kernel's shape) has no plane output: the predicate says so and the entry
    point fails instead of storing fp32."""
    assert not hip.e3d_attn_planes_supported(192, 96 * 192, 192, 96, 96, 19, 1)
    q = torch.randn(96, 192, device=DEV)
    with pytest.raises(RuntimeError), torch.no_grad():
        pkg.ops.attention(q, q, q, 1, 3, 96, 96, mode="f16x3", planes_out=True)


# ------------------------------------------------------------------------------------------------ planes -> row-LN
@pytest.fixture(scope="module")
def rowln_weights():
    H = 768
    out = {}
    for K in (64, 768, 1024):
        out[K] = ((torch.randn(H, K, generator=g(K)) / math.sqrt(K)).to(DEV).contiguous(), torch.randn(H, generator=g(K + 1)).to(DEV))
    return out, (torch.rand(H, generator=g(3)) + 0.5).to(DEV), torch.randn(H, generator=g(4)).to(DEV)


@pytest.mark.parametrize("K", [64, 768, 1024])
@pytest.mark.parametrize("M", [32, 96, 160, 256, 288])
@pytest.mark.parametrize("mode,dt", MODES)
def test_rowln_from_planes(pkg, hip, monkeypatch, rowln_weights, mode, dt, M, K):
    monkeypatch.setattr(pkg.ops, "ROWLN_MIN_M", 1)
    H = 768
    ws, gamma, beta = rowln_weights
    w, b = ws[K]
    a = torch.randn(M, K, generator=g(M + K))
    a[1] *= 1e3
    a[M // 2] *= 1e-3
    a[M - 1] *= 1e3
    a = a.to(DEV)
    res = (torch.randn(M, H, generator=g(2)) * 3 + 0.5).to(DEV)
    planes = pkg.ops.activation_planes(a, mode=mode)
    before = pkg.ops.ACT_PLANES_CALLS
    for r in (res, None):
        want = pkg.ops.linear_residual_layernorm(a, w, b, r, gamma, beta, 1e-12, mode=mode)
        got = pkg.ops.linear_residual_layernorm(planes, w, b, r, gamma, beta, 1e-12, mode=mode)
        assert torch.isfinite(want).all() and torch.equal(got, want)
    assert pkg.ops.ACT_PLANES_CALLS == before + 2


@pytest.mark.parametrize("M", [16384, 24576, 65536 - 32])
@pytest.mark.parametrize("mode,dt", MODES)
def test_rowln_from_planes_multi_tile(pkg, hip, rowln_weights, mode, dt, M):
    """A workgroup's row group is M / (number of CUs) rounded up to 32 rows, so on a 256-CU device the small shapes above
    are all single 32-row tiles.  These reach the other tile forms there: 64 rows per workgroup (one 64-row tile), 96 (one
    96-row tile), 256 (the 96 + 96 + 64 walk in its four orders, and a last workgroup that is 32 rows short)."""
    H, K = 768, 768
    ws, gamma, beta = rowln_weights
    w, b = ws[K]
    gen = torch.Generator(device=DEV).manual_seed(M)
    a = torch.randn(M, K, device=DEV, generator=gen)
    a[::97] *= 1e3
    a[5::101] *= 1e-3
    res = torch.randn(M, H, device=DEV, generator=gen) * 3 + 0.5
    planes = pkg.ops.activation_planes(a, mode=mode)
    want = pkg.ops.linear_residual_layernorm(a, w, b, res, gamma, beta, 1e-12, mode=mode)
    got = pkg.ops.linear_residual_layernorm(planes, w, b, res, gamma, beta, 1e-12, mode=mode)
    assert torch.isfinite(want).all() and torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def layer_model(pkg):
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.structure_model.model import ConditionalBertForDiffusionBase
    B, L = 64, 128
    common = dict(hidden_size=768, num_attention_heads=12, intermediate_size=1024, num_hidden_layers=1,
                  max_position_embeddings=L)
    model = ConditionalBertForDiffusionBase(BertConfig(**common),
                                            BertConfig(**common, is_decoder=True, add_cross_attention=True), 8)
    model.load_state_dict(seeded_state_dict({k: v.shape for k, v in model.state_dict().items()}, seed=1))
    pk = {k: v.to(DEV) for k, v in synthetic_pockets(B, L, seed=2).items() if torch.is_tensor(v)}
    x_t = torch.randn(B, L, 8, generator=g(5)).to(DEV)
    t = torch.randint(0, 1000, (B,), generator=g(6)).to(DEV)
    return model.eval().to(DEV), pk, x_t, t


@pytest.mark.parametrize("persistent", [False, True])
@pytest.mark.parametrize("mode", ["f16x3", "bf16x3"])
def test_structure_layers_end_to_end(pkg, hip, layer_model, monkeypatch, mode, persistent):
    """One encoder + one decoder layer, B = 64, L = 128 (M = 8192 = ROWLN_MIN_M): the predicted noise with activation planes
    equals the fp32-activation launches bit for bit, and the plane-input row-complete entry point was really called: by every
    BertSelfOutput (K = 768: the attention contexts) -- and, once the GELU GEMMs run the persistent kernel as they do at the
    workload's M = 65 536 (here: 128 tiles, forced), by every BertOutput (K = 1024) as well.  The ``ops.TRACE`` records
    (names and shape tuples, which ``bench.py --full`` keys its report on) are the same on both paths."""
    model, pk, x_t, t = layer_model

    def run(on):
        monkeypatch.setattr(pkg.ops, "ACT_PLANES", on)
        monkeypatch.setattr(pkg.ops, "TRACE", [])
        before = pkg.ops.ACT_PLANES_CALLS
        with torch.no_grad():
            out = model(t, x_t, pk["ligand_attn_mask"], pk["receptor_seq"], pk["receptor_angles"], pk["receptor_attn_mask"])
        return out, pkg.ops.ACT_PLANES_CALLS - before, [(r[0], r[3]) for r in pkg.ops.TRACE]

    prev, prev_a = pkg.ops.set_gemm_mode(mode), pkg.ops.set_attn_mode(mode)
    prev_k = hip.e3d_gemm_kernel_select(5 if persistent else -1)
    try:
        want, n_off, trace_off = run(False)
        got, n_on, trace_on = run(True)
    finally:
        hip.e3d_gemm_kernel_select(prev_k)
        pkg.ops.set_gemm_mode(prev)
        pkg.ops.set_attn_mode(prev_a)
    assert trace_on == trace_off
    rowln = [meta for name, meta in trace_on if name == "gemm_layernorm" and meta[0] >= pkg.ops.ROWLN_MIN_M]
    n_self, n_out = sum(1 for m in rowln if m[2] == 768), sum(1 for m in rowln if m[2] == 1024)
    assert n_self >= 3 and n_out >= 2 and n_self + n_out == len(rowln), rowln
    assert n_off == 0 and n_on == n_self + (n_out if persistent else 0), (n_off, n_on, n_self, n_out)
    assert torch.isfinite(want).all() and torch.equal(got, want)
