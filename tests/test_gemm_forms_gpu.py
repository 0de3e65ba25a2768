"""Every GEMM kernel instantiation, forced one by one, against an fp64 CPU statement of the same operation.

``ops.gemm`` / ``autograd.gemm_general`` choose among a dozen kernels by layout, arithmetic, tile count, M, N and the CU
count (``csrc/gemm_split.hip`` ``launch()`` / ``dispatch()``), so the shape-driven tests elsewhere reach only the forms
their shapes happen to select.  Here each *effective* instantiation -- one row per real launch site; nominal forms that
fall through to another (form 4 -> 3 outside the 2-term forward layout, form 3 -> 2 for three terms or a K-major A) have
no row of their own -- is forced through the library's switches (``forced()`` below: ``e3d_gemm_kernel_select`` pref,
``e3d_gemm_general_select`` form, ``e3d_gemm_skinny_plan_select``) or through the operand property its predicate reads.

Terms: 1 = plain bf16 (RNE operands), 3 = bf16x3, 6 = bf16x6, 19 = f16x3 (fp16 terms in the forward layout; a K-major
operand runs the 3-term bf16 kernels, so 19 there is asserted bit-identical to 6).  NS = bf16 / fp16 terms per operand.

====================  ========  ===============================  ==================================  ===========================================
layout (A, B)         NS, type  instantiation (tile)             forced by                           launch line / test id
====================  ========  ===============================  ==================================  ===========================================
forward (row, row)    1 bf16    general form 1 (256x128)         pref 0, form 1                      1228 > 1269          test_forward_general_form[bf16-1]
forward               1 bf16    general form 2 (128x128, 4 wv)   pref 0, form 2                      1219 > 1269          test_forward_general_form[bf16-2]
forward               1 bf16    general form 3 (128x128, 8 wv)   pref 0, form 3 (or 4)               1216 > 1269          test_forward_general_form[bf16-3]
forward               1 bf16    256x256 interleaved              pref 3, >= 160 tiles                1169 > 1116          test_forward_256x256[bf16-interleaved]
forward               1 bf16    256x256 classic (2 buffers)      pref 1, >= 256 tiles                1173 > 1116          test_forward_256x256[bf16-classic]
forward               2 bf16    general form 1 / 2 / 3           pref 0, form 1 / 2 / 3              1228/1219/1216 > 1269  test_forward_general_form[bf16x3-1..3]
forward               2 bf16    general form 4 (128x64, 4 wv)    pref 0, form 4                      1207 > 1269          test_forward_general_form[bf16x3-4]
forward               2 bf16    persistent 256x256               pref 5, M % 256 == N % 256 == 0     1163 > 1099          test_forward_persistent[bf16x3]
forward               2 bf16    256x256 interleaved              pref 3, >= 256 tiles                1165 > 1116          test_forward_256x256[bf16x3-interleaved]
forward               2 bf16    256x256 classic (2 buffers)      pref 1, >= 256 tiles                1173 > 1116          test_forward_256x256[bf16x3-classic]
forward               2 fp16    general form 1 / 2 / 3 / 4       pref 0, form 1 / 2 / 3 / 4          1228/1219/1216/1207 > 1269  test_forward_general_form[f16x3-1..4]
forward               2 fp16    persistent 256x256               pref 5, M % 256 == N % 256 == 0     1163 > 1099          test_forward_persistent[f16x3]
forward               2 fp16    256x256 interleaved / classic    pref 3 / pref 1, >= 256 tiles       1165 / 1173 > 1116   test_forward_256x256[f16x3-*]
forward               3 bf16    general form 1 / 2               pref 0, form 1 / 2                  1228 / 1219 > 1269   test_forward_general_form[bf16x6-1..2]
forward               3 bf16    256x256 classic (1 buffer)       pref 1, >= 256 tiles                1173 > 1116          test_forward_256x256[bf16x6-classic]
forward, exact fp32   --        gemm_nt_f32 (128x128)            its one kernel                      gemm_f32.hip:173     test_forward_exact_f32
input grad (row, KM)  1, 2 bf16 general form 1 / 2 / 3           form 1 / 2 / 3                      1228/1219/1216 > 1269  test_kmajor_general_form[dgrad-bf16*-*]
input grad (row, KM)  3 bf16    general form 1 / 2 (t 6 and 19)  form 1 / 2                          1228 / 1219 > 1269   test_kmajor_general_form[dgrad-bf16x6-*]
(KM, row)             1,2,3     general form 1 / 2               form 1 / 2                          1228 / 1219 > 1269   test_kmajor_general_form[kmaj_row-*]
wgrad (KM, KM)        1,2,3     form 1, transposing staging      form 1; quads, 16-B aligned         1226 > 1269          test_weight_gradient_form[*-tr]
wgrad (KM, KM)        1,2,3     form 1, dword staging            form 1; B at a 1-float offset       1228 > 1269          test_weight_gradient_form[*-dword]
wgrad (KM, KM)        1,2,3     form 2 (128x128)                 form 2                              1219 > 1269          test_weight_gradient_form[*-form2]
wgrad (KM, KM)        1,2,3     split-K of each of the three     few tiles, tokens >= 1024           1249 > 1269 (grid y) test_weight_gradient_form[*] (K = 4001, 1061)
wgrad, grouped        1,2,3     gemm_wgrad_grouped_kernel, TR    quads, aligned, in span             1397 / 1401 / 1405   test_wgrad_forms_gpu.py::test_reduction_edges[grouped-*-tr], test_output_edges[grouped-*-tr]
wgrad, grouped        1,2,3     the same, dword staging          one predicate term turned           1398 / 1402 / 1406   test_wgrad_forms_gpu.py::test_reduction_edges[grouped-*-dword], test_staging_predicate[*-grouped-*]
wgrad, ragged         1,2,3     gemm_wgrad_ragged_kernel, TR     EVERY problem eligible              1449 / 1453 / 1457   test_wgrad_forms_gpu.py::test_reduction_edges[ragged-*-tr], test_problem_table[*-ragged-*]
wgrad, ragged         1,2,3     the same, dword staging          ONE odd problem (first or last)     1450 / 1454 / 1458   test_wgrad_forms_gpu.py::test_reduction_edges[ragged-*-dword], test_staging_predicate[*-ragged-*]
skinny                2 bf16/fp16  32x32 per wave, K slices      plan (1, 2^20) / (64, 16) / (0, 0)  gemm_skinny.hip:265  test_skinny[*-one|max|default]
skinny + residual LN  2 bf16/fp16  the same + LayerNorm finish   plan (1, 2^20) / (64, 16) / (0, 0)  gemm_skinny.hip:357  test_skinny_residual_layernorm[*]
====================  ========  ===============================  ==================================  ===========================================

Launch lines are those of csrc/gemm_split.hip unless a file is named: ``a > b`` = the branch of ``launch()`` (line a) that
selects the form and the ``hipLaunchKernelGGL`` it ends in (1099: persistent, 1116: 256x256, 1269: general kernel, where
split-K is the grid's y extent).  The two batched weight-gradient families (one launch site per NS and staging) have a
forms file of their own, tests/test_wgrad_forms_gpu.py.

Edges every instantiation sees (where its layout allows them): M = tile rows - 1, tile rows + 1 and a single row (the
transposing weight-gradient staging needs M % 4 == 0: tile rows -/+ 4 there; the persistent kernel needs M % 256 == 0);
ragged N (the general entry point; ``e3d_gemm_bias_act_f32_split_ex`` asks for N % 128 == 0); one k-step and an odd
number of them (K = 32, 96) and an even number (the k loop runs k-steps in pairs: K = 832; K-major reductions also
K = 20, 45, 800, 4001 -- the persistent kernel needs K >= 64); A a
column block of a wider buffer (lda > K) whose padding holds NaN; the output a view ``big[:M, :N]`` of a NaN buffer with
extra rows and ldc > N, everything outside [M, N] still NaN afterwards (on split-K also the ldc == N memset branch);
forward layouts: each activation per kernel family, bias present and absent, ``absmax`` == max |out| exactly, and
``out_scale`` != 1 (a power-of-two-scaled weight: the f16x3 operand always, the bf16 arithmetics in one case each);
weight-gradient split-K with a bias column that must be added exactly once.

References: fp64 products of the operands (plain-bf16 mode: of the operands rounded to bf16 with round-to-nearest-even,
as the kernel's term split rounds them), so every arithmetic's bound is its own error: 5e-6 (bf16, bf16x6, f16x3, fp32)
and 3e-5 (bf16x3) of max |ref|, and every 32 x 32 output block within 4x that bound of its own largest |ref|.  Calls
without split-K are run twice and must be bit-identical.
"""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
MODES = {1: "bf16", 3: "bf16x3", 6: "bf16x6", 19: "f16x3", 0: "f32"}
TOL = {0: 5e-6, 1: 5e-6, 3: 3e-5, 6: 5e-6, 19: 5e-6}
ACT = {0: lambda x: x, 1: F.gelu, 2: F.silu}


@contextlib.contextmanager
def forced(hip, pref=None, form=None, plan=None):
    """Force a kernel choice for the enclosed calls; the previous values come back whatever happens (the skinny plan
    returns to its defaults)."""
    prev_pref, prev_form = hip.e3d_gemm_kernel_select(-1), hip.e3d_gemm_general_select(-1)
    try:
        if pref is not None:
            hip.e3d_gemm_kernel_select(pref)
        if form is not None:
            hip.e3d_gemm_general_select(form)
        if plan is not None:
            hip.e3d_gemm_skinny_plan_select(*plan)
        yield
    finally:
        hip.e3d_gemm_kernel_select(prev_pref)
        hip.e3d_gemm_general_select(prev_form)
        hip.e3d_gemm_skinny_plan_select(0, 0)


@pytest.fixture(scope="module", autouse=True)
def selections_unchanged(hip):
    """No test of this module may leave a forced kernel choice behind for the tests that run after it."""
    before = (hip.e3d_gemm_kernel_select(-1), hip.e3d_gemm_general_select(-1))
    yield
    assert (hip.e3d_gemm_kernel_select(-1), hip.e3d_gemm_general_select(-1)) == before


# ----------------------------------------------------------------------------------------------------- operands
# Logical operands a [M, K], b [N, K] (out = a b^T); stored K-contiguous ("row": a column block of a NaN-padded buffer) or
# K-major (the transpose, a column block of a NaN-padded [K, rows + 20] buffer).  Cached with their fp64 products.
_OPS, _REF = {}, {}


def _stored(x, kmajor, col0):
    rows, K = x.shape
    if kmajor:
        buf = torch.full((K, rows + 20), NAN)
        buf[:, col0:col0 + rows] = x.t()
        return buf.to(DEV)[:, col0:col0 + rows]
    buf = torch.full((rows, K + 32), NAN)
    buf[:, col0:col0 + K] = x
    return buf.to(DEV)[:, col0:col0 + K]


def operands(M, N, K, a_kmaj=False, b_kmaj=False, b_col0=4, contiguous_b=False):
    key = (M, N, K, a_kmaj, b_kmaj, b_col0, contiguous_b)
    if key not in _OPS:
        gen = torch.Generator().manual_seed(M * 7919 + N * 31 + K)
        a = torch.randn(M, K, generator=gen)
        b = torch.randn(N, K, generator=gen) / math.sqrt(K)
        a_st = _stored(a, a_kmaj, 8 if a_kmaj else 16)
        b_st = b.to(DEV) if contiguous_b else _stored(b, b_kmaj, b_col0)
        _OPS[key] = (a, b, a_st, b_st)
    return _OPS[key]


def product(a, b, rounded):
    """fp64 a b^T on the CPU (``rounded``: of the operands rounded to bf16, RNE -- what the plain-bf16 kernels multiply)."""
    key = (id(a), id(b), rounded)
    if key not in _REF:
        if rounded:
            a, b = a.bfloat16(), b.bfloat16()
        _REF[key] = (a.double() @ b.double().t()).to(DEV)
    return _REF[key]


def reference(a, b, terms, bias=None, act=0):
    ref = product(a, b, terms == 1)
    if bias is not None:
        ref = ref + bias.double()
    return ACT[act](ref)


def f16_prescale(pkg, w):
    """The power-of-two-scaled weight and the out_scale that undoes it (what ops.gemm runs f16x3 on)."""
    return pkg.ops.f16_weight(w)


def _p(t):
    return None if t is None else t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


def call(pkg, name, *args):
    pkg.hip.check(getattr(pkg.hip.lib(), name)(*args, _s()), name)


def check_close(got, ref, tol, what):
    got = got.double()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    scale = float(ref.abs().max())
    assert float(err.max()) <= tol * scale, f"{what}: rel err {float(err.max()) / scale:.3g} > {tol:g}"
    # every 32 x 32 block against its own magnitude: a wrong tile in a ragged corner cannot hide under the global max
    M, N = got.shape
    pm, pn = -M % 32, -N % 32
    eb = F.pad(err, (0, pn, 0, pm)).view((M + pm) // 32, 32, (N + pn) // 32, 32).amax((1, 3))
    rb = F.pad(ref.abs(), (0, pn, 0, pm)).view((M + pm) // 32, 32, (N + pn) // 32, 32).amax((1, 3))
    bad = eb > 4 * tol * rb.clamp_min(1e-3 * scale)
    assert not bad.any(), f"{what}: 32x32 blocks {bad.nonzero()[:4].tolist()} off by {float((eb / rb)[bad].max()):.3g} (rel)"


def run(fn, M, N, ref, tol, what, absmax=False, repeat=True, extra_cols=36):
    """fn(out, absmax_slot) writes out = a view [M, N] of a NaN buffer with 3 extra rows and ``extra_cols`` extra columns;
    nothing outside it may change.  Twice (bit-identical) unless ``repeat`` is False (split-K: atomics)."""
    outs = []
    for _ in range(2 if repeat else 1):
        big = torch.full((M + 3, N + extra_cols), NAN, device=DEV)
        slot = torch.zeros(1, device=DEV) if absmax else None
        fn(big[:M, :N], slot)
        torch.cuda.synchronize()
        assert big[M:].isnan().all() and big[:M, N:].isnan().all(), f"{what}: a write outside [M, N]"
        out = big[:M, :N]
        if absmax:
            assert float(slot) == float(out.abs().max()), f"{what}: absmax {float(slot)} != {float(out.abs().max())}"
        outs.append(out)
    check_close(outs[0], ref, tol, what)
    if repeat:
        assert torch.equal(outs[0], outs[1]), f"{what}: repeated call differs"
    return outs[0]


# ----------------------------------------------------------------------------------------------------- forward layout
def forward_case(pkg, terms, M, N, K, act, bias, absmax, pw, entry, what):
    """One forward call: ``entry`` "ex" = e3d_gemm_bias_act_f32_split_ex (absmax, out_scale), "general" =
    e3d_gemm_f32_split_general (ragged N), "f32" = the exact-fp32 kernel.  ``pw``: the weight is passed times 2^pw and
    out_scale = 2^-pw (f16x3 through the "ex" entry: always its pre-scaled weight)."""
    a, b, a_st, w = operands(M, N, K, contiguous_b=True)
    bias_t = torch.randn(N, generator=torch.Generator().manual_seed(N)) if bias else None
    bias_d = bias_t.to(DEV) if bias else None
    scale = 1.0
    if entry == "ex" and terms == 19:
        w, scale = f16_prescale(pkg, w)
    elif entry == "ex" and pw:
        w, scale = w * 2.0 ** pw, 2.0 ** -pw
    ref = reference(a, b, terms, bias_t.to(DEV) if bias else None, act)

    def fn(out, slot):
        if entry == "ex":
            call(pkg, "e3d_gemm_bias_act_f32_split_ex", _p(a_st), a_st.stride(0), _p(w), _p(bias_d), _p(out), out.stride(0),
                 M, N, K, act, terms, _p(slot), scale)
        elif entry == "general":
            call(pkg, "e3d_gemm_f32_split_general", _p(a_st), a_st.stride(0), 0, _p(w), w.stride(0), 0, _p(bias_d), _p(out),
                 out.stride(0), M, N, K, act, terms)
        else:
            call(pkg, "e3d_gemm_bias_act_f32", _p(a_st), a_st.stride(0), _p(w), _p(bias_d), _p(out), out.stride(0), M, N, K, act)
    return run(fn, M, N, ref, TOL[terms], what, absmax=absmax)


def general_cases(BM):
    return [dict(M=1, N=128, K=32, act=1, bias=True, absmax=False, pw=4, entry="ex"),
            dict(M=BM + 1, N=256, K=96, act=0, bias=False, absmax=True, pw=0, entry="ex"),
            dict(M=BM - 1, N=200, K=832, act=2, bias=True, absmax=False, pw=0, entry="general")]


TILE_ROWS = {1: 256, 2: 128, 3: 128, 4: 128}
FWD_FORMS = [(1, 1), (1, 2), (1, 3), (3, 1), (3, 2), (3, 3), (3, 4), (19, 1), (19, 2), (19, 3), (19, 4), (6, 1), (6, 2)]


@pytest.mark.parametrize("terms,form", FWD_FORMS, ids=[f"{MODES[t]}-{f}" for t, f in FWD_FORMS])
def test_forward_general_form(pkg, hip, terms, form):
    with forced(hip, pref=0, form=form):
        for c in general_cases(TILE_ROWS[form]):
            forward_case(pkg, terms, what=f"{MODES[terms]} form {form} {c}", **c)


BIG = [dict(M=16385, N=1024, K=96, act=0, bias=False, absmax=True, pw=0, entry="ex"),
       dict(M=16383, N=1024, K=32, act=1, bias=True, absmax=False, pw=4, entry="ex"),
       dict(M=16385, N=1024, K=96, act=2, bias=True, absmax=False, pw=0, entry="ex")]
FWD_256 = [(1, 3), (1, 1), (3, 3), (3, 1), (19, 3), (19, 1), (6, 1)]


@pytest.mark.parametrize("terms,pref", FWD_256,
                         ids=[f"{MODES[t]}-{'interleaved' if p == 3 else 'classic'}" for t, p in FWD_256])
def test_forward_256x256(pkg, hip, terms, pref):
    """The 256x256 kernels at >= 256 tiles (M ragged by one row either way, N = 1024): interleaved staging (pref 3) and
    the classic loop (pref 1)."""
    with forced(hip, pref=pref):
        for c in BIG:
            forward_case(pkg, terms, what=f"{MODES[terms]} pref {pref} {c}", **c)


@pytest.mark.parametrize("terms", [3, 19], ids=["bf16x3", "f16x3"])
def test_forward_persistent(pkg, hip, terms):
    """The persistent 256x256 kernel at any tile count (pref 5; it needs M, N multiples of 256 and K >= 64)."""
    cases = [dict(M=512, N=512, K=64, act=0, bias=False, absmax=True, pw=0, entry="ex"),
             dict(M=256, N=768, K=96, act=1, bias=True, absmax=False, pw=4, entry="ex"),
             dict(M=768, N=256, K=800, act=2, bias=True, absmax=False, pw=0, entry="ex")]
    with forced(hip, pref=5):
        for c in cases:
            forward_case(pkg, terms, what=f"{MODES[terms]} persistent {c}", **c)


def test_forward_exact_f32(pkg, hip):
    for c in [dict(M=1, N=128, K=32, act=1, bias=True), dict(M=129, N=256, K=96, act=0, bias=False),
              dict(M=127, N=384, K=832, act=2, bias=True)]:
        forward_case(pkg, 0, absmax=False, pw=0, entry="f32", what=f"f32 {c}", **c)


# ----------------------------------------------------------------------------------------------------- K-major layouts
def kmajor_case(pkg, terms, layout, M, N, K, bias, what, b_col0=4, extra_cols=36):
    a_kmaj, b_kmaj = {"dgrad": (False, True), "kmaj_row": (True, False), "wgrad": (True, True)}[layout]
    a, b, a_st, b_st = operands(M, N, K, a_kmaj, b_kmaj, b_col0)
    bias_t = torch.randn(N, generator=torch.Generator().manual_seed(N + 1)) if bias else None
    bias_d = bias_t.to(DEV) if bias else None
    ref = reference(a, b, terms, bias_d)
    tiles_256 = -(-M // 256) * -(-N // 128)
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    split = layout == "wgrad" and K >= 1024 and tiles_256 * 2 < cus   # few tiles, long reduction: launch_general's split-K

    def fn(out, slot):
        call(pkg, "e3d_gemm_f32_split_general", _p(a_st), a_st.stride(0), int(a_kmaj), _p(b_st), b_st.stride(0), int(b_kmaj),
             _p(bias_d), _p(out), out.stride(0), M, N, K, 0, terms)
    return run(fn, M, N, ref, TOL[terms], what, repeat=not split, extra_cols=extra_cols)


KM_FORMS = ([("dgrad", t, f) for t in (1, 3) for f in (1, 2, 3)] + [("dgrad", 6, f) for f in (1, 2)]
            + [("kmaj_row", t, f) for t in (1, 3, 6) for f in (1, 2)])


@pytest.mark.parametrize("layout,terms,form", KM_FORMS, ids=[f"{l}-{MODES[t]}-{f}" for l, t, f in KM_FORMS])
def test_kmajor_general_form(pkg, hip, layout, terms, form):
    """Input-gradient (row, K-major) and (K-major, row) layouts: ragged M and N, one / three / 26 k-steps, B or A a column
    block of a wider buffer.  Terms 19 runs the 3-term bf16 kernels here: bit-identical to terms 6."""
    BM = 256 if form == 1 else 128
    cases = [dict(M=1, N=200, K=32, bias=True), dict(M=BM + 1, N=128, K=96, bias=False),
             dict(M=BM - 1, N=257, K=832, bias=True)]
    with forced(hip, form=form):
        for c in cases:
            out = kmajor_case(pkg, terms, layout, what=f"{layout} {MODES[terms]} form {form} {c}", **c)
            if terms == 6:
                assert torch.equal(out, kmajor_case(pkg, 19, layout, what=f"{layout} f16x3 form {form} {c}", **c))


WG = [(t, v) for t in (1, 3, 6) for v in ("tr", "dword", "form2")]


@pytest.mark.parametrize("terms,variant", WG, ids=[f"{MODES[t]}-{v}" for t, v in WG])
def test_weight_gradient_form(pkg, hip, terms, variant):
    """dW = dz^T x (both K-major, reduction over the tokens).  "tr": float4 staging with transposing fragment reads (needs
    M, N, strides in whole quads and 16-byte aligned operands: M = tile -/+ 4); "dword": the same form with B one float
    off 16-byte alignment; "form2": 128x128.  K = 20 / 800 / 45 reduce in one / 25 / 2 k-steps; K = 4001 and 1061 take
    split-K (partial last chunk, K % 32 != 0, a bias column added once; ldc > N: the 2-D zeroing kernel, ldc == N: the
    memset)."""
    b_col0 = 5 if variant == "dword" else 4
    if variant == "tr":
        shapes = [(4, 200, 20), (252, 132, 800), (260, 200, 45), (252, 124, 4001), (8, 16, 1061)]
    elif variant == "dword":
        shapes = [(1, 200, 20), (257, 131, 800), (255, 129, 45), (255, 129, 4001), (7, 15, 1061)]
    else:
        shapes = [(1, 200, 20), (129, 131, 800), (127, 129, 45), (127, 129, 4001), (7, 15, 1061)]
    with forced(hip, form=2 if variant == "form2" else 1):
        for i, (M, N, K) in enumerate(shapes):
            if variant == "tr":
                assert M % 4 == 0 and N % 4 == 0
            what = f"wgrad {MODES[terms]} {variant} M={M} N={N} K={K}"
            out = kmajor_case(pkg, terms, "wgrad", M, N, K, bias=i % 2 == 0 or K == 4001, what=what, b_col0=b_col0,
                              extra_cols=0 if K == 1061 else 36)
            if terms == 6 and K < 1024:
                assert torch.equal(out, kmajor_case(pkg, 19, "wgrad", M, N, K, bias=i % 2 == 0, what=what, b_col0=b_col0))


# ----------------------------------------------------------------------------------------------------- forms agree
CROSS = [("fwd", 1, (1, 2, 3)), ("fwd", 3, (1, 2, 3, 4)), ("fwd", 19, (1, 2, 3, 4)), ("fwd", 6, (1, 2)),
         ("dgrad", 1, (1, 2, 3)), ("dgrad", 3, (1, 2, 3)), ("dgrad", 6, (1, 2)), ("wgrad", 3, (1, 2))]


@pytest.mark.parametrize("layout,terms,forms", CROSS, ids=[f"{l}-{MODES[t]}" for l, t, _ in CROSS])
def test_forms_of_one_arithmetic_agree(pkg, hip, layout, terms, forms):
    M, N, K = 300, 256, 96
    outs = []
    for form in forms:
        with forced(hip, pref=0, form=form):
            if layout == "fwd":
                outs.append(forward_case(pkg, terms, M, N, K, 0, True, False, 0, "general", f"fwd form {form}"))
            else:
                outs.append(kmajor_case(pkg, terms, layout, M, N, K, True, f"{layout} form {form}"))
    for form, o in zip(forms[1:], outs[1:]):
        d = float((o - outs[0]).abs().max()) / float(outs[0].abs().max())
        assert d <= TOL[terms], (forms[0], form, d)


# ----------------------------------------------------------------------------------------------------- skinny kernels
PLANS = {"one": (1, 1 << 20), "max": (64, 16), "default": (0, 0)}
SK = [(t, p) for t in (3, 19) for p in PLANS]


@pytest.mark.parametrize("terms,plan", SK, ids=[f"{MODES[t]}-{p}" for t, p in SK])
def test_skinny(pkg, hip, terms, plan):
    """The small-M kernels under the one-slice plan, the most-slices plan and the default one: K = 16 (one k-block), 48,
    800 (a partial last slice under the most-slices plan), M = 1 / 31 / 33 (32-row tiles)."""
    cases = [dict(M=1, N=96, K=48, act=1, bias=True, absmax=False, pw=4),
             dict(M=33, N=128, K=800, act=0, bias=False, absmax=True, pw=0),
             dict(M=31, N=256, K=16, act=2, bias=True, absmax=False, pw=0)]
    with forced(hip, plan=PLANS[plan]):
        for c in cases:
            M, N, K = c["M"], c["N"], c["K"]
            a, b, a_st, w = operands(M, N, K, contiguous_b=True)
            bias_t = torch.randn(N, generator=torch.Generator().manual_seed(N)) if c["bias"] else None
            bias_d = bias_t.to(DEV) if c["bias"] else None
            if terms == 19:
                w, scale = f16_prescale(pkg, w)
            else:
                w, scale = w * 2.0 ** c["pw"], 2.0 ** -c["pw"]
            nbytes = pkg.hip.lib().e3d_gemm_skinny_workspace_bytes(M, N, K)
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)

            def fn(out, slot):
                call(pkg, "e3d_gemm_skinny_f32_split_ex", _p(a_st), a_st.stride(0), _p(w), _p(bias_d), _p(out), out.stride(0),
                     M, N, K, c["act"], terms, _p(ws), ws.numel(), _p(slot), scale)
            run(fn, M, N, reference(a, b, terms, bias_d, c["act"]), TOL[terms], f"skinny {MODES[terms]} {plan} {c}",
                absmax=c["absmax"])


@pytest.mark.parametrize("terms,plan", SK, ids=[f"{MODES[t]}-{p}" for t, p in SK])
def test_skinny_residual_layernorm(pkg, hip, terms, plan):
    with forced(hip, plan=PLANS[plan]):
        for M, H, K, with_res in ((1, 256, 48, True), (33, 768, 800, False), (31, 512, 16, True)):
            a, b, a_st, w = operands(M, H, K, contiguous_b=True)
            gen = torch.Generator().manual_seed(M + H)
            bias, gamma, beta = torch.randn(H, generator=gen), torch.rand(H, generator=gen) + 0.5, torch.randn(H, generator=gen)
            res = torch.randn(M, H, generator=gen) if with_res else None
            bd, gd, be = bias.to(DEV), gamma.to(DEV), beta.to(DEV)
            rd = res.to(DEV) if with_res else None
            w, scale = f16_prescale(pkg, w) if terms == 19 else (w, 1.0)
            ws = torch.empty(max(pkg.hip.lib().e3d_gemm_skinny_workspace_bytes(M, H, K), 16), dtype=torch.uint8, device=DEV)
            outs = []
            for _ in range(2):
                out = torch.empty(M, H, device=DEV)
                call(pkg, "e3d_gemm_skinny_residual_layernorm_f32_split_ex", _p(a_st), a_st.stride(0), _p(w), _p(bd), _p(rd),
                     _p(gd), _p(be), 1e-12, _p(out), M, H, K, terms, _p(ws), ws.numel(), scale)
                outs.append(out)
            pre = reference(a, b, terms, bd) + (0 if res is None else rd.double())
            ref = F.layer_norm(pre, (H,), gd.double(), be.double(), 1e-12)
            check_close(outs[0], ref, 4 * TOL[terms], f"skinny LN {MODES[terms]} {plan} M={M} H={H} K={K}")
            assert torch.equal(outs[0], outs[1])


# ----------------------------------------------------------------------------------------------------- misaligned operands
@pytest.mark.parametrize("mode,M", [("f32", 300), ("bf16", 300), ("bf16x3", 300), ("bf16x6", 300), ("f16x3", 300),
                                    ("f16x3", 64)])
def test_gemm_refuses_a_misaligned_activation(pkg, hip, mode, M):
    """``ops.gemm`` with A = x[:, 1:1+K] (row stride a multiple of 4 floats, start 4 bytes off 16-byte alignment): every
    kernel family (exact fp32, tiled split, skinny) refuses with a RuntimeError that names the alignment."""
    K, N = 256, 256
    x = torch.randn(M, K + 4, device=DEV)
    a = x[:, 1:1 + K]
    assert a.data_ptr() % 16 == 4
    w, b = torch.randn(N, K, device=DEV) / 16, torch.randn(N, device=DEV)
    with pytest.raises(RuntimeError, match="align"):
        pkg.ops.gemm(a, w, b, mode=mode)
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode,tol", [("f16x3", 5e-6), ("bf16x3", 3e-5)])
def test_linear_residual_layernorm_with_misaligned_operands(pkg, hip, monkeypatch, mode, tol):
    """The row-complete kernel needs A and the residual 16-byte aligned; its predicate (``rowln_ok``) checks that, so a
    residual one float off alignment takes the pair (GEMM, then the LayerNorm kernel) and gives the right numbers, and an
    A one float off is refused as ``ops.gemm`` refuses it."""
    monkeypatch.setattr(pkg.ops, "ROWLN_MIN_M", 1)
    M, K, H = 4096, 768, 768
    gen = torch.Generator().manual_seed(11)
    a = torch.randn(M, K, generator=gen)
    w = torch.randn(H, K, generator=gen) / math.sqrt(K)
    b, res = torch.randn(H, generator=gen), torch.randn(M, H, generator=gen) * 3 + 0.5
    gamma, beta = torch.rand(H, generator=gen) + 0.5, torch.randn(H, generator=gen)
    ad, wd, bd, gd, be = (t.to(DEV) for t in (a, w, b, gamma, beta))
    terms = pkg.ops.GEMM_MODES[mode]
    assert pkg.ops.rowln_ok(terms, M, H, K, ad)
    r_buf = torch.empty(M * H + 1, device=DEV)
    r_buf[1:] = res.to(DEV).view(-1)
    rd = r_buf[1:].view(M, H)                                   # contiguous, 4 bytes off 16-byte alignment
    assert rd.data_ptr() % 16 == 4
    got = pkg.ops.linear_residual_layernorm(ad, wd, bd, rd, gd, be, 1e-12, mode=mode)
    rows = torch.randperm(M, generator=torch.Generator().manual_seed(5))[:1024]
    pre = F.linear(a[rows].double(), w.double(), b.double()) + res[rows].double()
    ref = F.layer_norm(pre, (H,), gamma.double(), beta.double(), 1e-12)
    check_close(got[rows.to(DEV)], ref.to(DEV), 4 * tol, f"{mode} misaligned residual")

    a_buf = torch.empty(M, K + 4, device=DEV)
    a_buf[:, 1:1 + K] = ad
    am = a_buf[:, 1:1 + K]
    assert am.data_ptr() % 16 == 4 and not pkg.ops.rowln_ok(terms, M, H, K, am)
    with pytest.raises(RuntimeError, match="align"):
        pkg.ops.linear_residual_layernorm(am, wd, bd, None, gd, be, 1e-12, mode=mode)
    torch.cuda.synchronize()
