"""The row-complete GEMM + LayerNorm kernel (csrc/gemm_rowln.hip, ``gemm_rowln_kernel``) in every row-group walk, at short
reductions that cross tile changes and over the ABI surface the wrappers never use, against the fp64 statement of
tests/rowln_ref.py.  Both entry points are called through the C ABI (``e3d_gemm_residual_layernorm_f32_split``: fp32 rows,
``e3d_gemm_residual_layernorm_planes_split``: activation planes); weight planes come from ``ops.weight_planes``, activation
planes from ``ops.activation_planes``.

Launch sites and edges (R = csrc/gemm_rowln.hip):

==========================================  ==================================================  ==========================================
what                                        forced by                                           test id
==========================================  ==================================================  ==========================================
R launch_rowln<_Float16> / <__bf16>         terms 19 / 3, fp32-row entry point                  every test, [f16x3-*] / [bf16x3-*]
R launch_rowln<E, true> (A_PLANES)          the plane entry point, same operands                every test (bit-equal to the fp32-row form)
tile_body<1> / <2> / <3> (32 / 64 / 96)     the walk of the group (table below)                 test_row_group_walks[*]
two tiles: 64 + 64                          g = 128                                             test_row_group_walks[*-128]
96 then 64; 64 as the LAST tile             g = 160, 224, 320, 352                              test_row_group_walks[*-160|224|320|352]
96 after 96 (twice: 288)                    g = 192, 288                                        test_row_group_walks[*-192|288]
four orders of a 256-row group              g = 256, blocks 0 / 8 / 16 / 24                     test_row_group_walks[*-256], test_short_reductions_across_tiles[*-256]
four tiles in one group                     g = 320, 352; 256 in order 3                        test_row_group_walks[*-320|352|256]
short last group (32 .. 288 rows)           M = smallest_m(g): not a multiple of g              test_row_group_walks[*] (last block checked)
K = 64: two pairs, the tail right behind    npairs = 2: min(p + 2, npairs - 1) re-fetches at 0  test_row_group_walks[*-64-*], test_short_reductions_across_tiles[*-64-*]
K = 96: one fetch ahead, one re-fetch       npairs = 3: pair 2 fetched at p = 0, again at 1     ...[*-96-*]
K = 128 / 768 / 1024                        the steady-state ring, 4 / 24 / 32 pairs            ...[*-128-*|*-768-*|*-1024-*]
next tile's prefetch under the epilogue     every group with more than one tile                 both of the above
residual == NULL (tail re-fetches W)        residual None                                       every test (both forms in each case)
bias == NULL                                bias None                                           test_abi_edges[no_bias]
out_scale != 1 with bf16 terms              weight x 2^3, out_scale 2^-3                        test_abi_edges[out_scale]
eps 1e-12 / 1e-5 / 1e-2                     eps                                                 test_abi_edges[eps_*]
ldo > N, ldr > N, lda > K                   out / residual / A column blocks of wider buffers   test_abi_edges[*]
rows >= M unwritten                         sentinel rows behind every output                   every test
predicate == entry point's acceptance       refusing (M, N, K, lda)                             test_predicate_and_routes
ops.rowln_ok alignment rules                views at +4 bytes, residual row stride 770          test_predicate_and_routes
M % 32 != 0 takes the pair                  M = 8192 + 16                                       test_predicate_and_routes
==========================================  ==================================================  ==========================================

Groups and walks on a 256-CU device (M = smallest_m(g, 256) = (g - 32) 256 + 32; the launches follow the device's own
multiprocessor count, so on another device the same groups are reached at other M):

=====  ======  =====  ============  ====================================================================
g      M       grid   last group    walk of a full group
=====  ======  =====  ============  ====================================================================
96     16416   171    96            96                                 (test_short_reductions_across_tiles)
128    24608   193    32            64 64
160    32800   205    160           96 64
192    40992   214    96            96 96
224    49184   220    128           96 64 64
256    57376   225    32            96 96 64 | 64 96 96 | 96 64 96 | 64 64 64 64   (block >> 3) & 3 = 0 | 1 | 2 | 3
288    65568   228    192           96 96 96
320    73760   231    160           96 96 64 64
352    81952   233    288           96 96 96 64
=====  ======  =====  ============  ====================================================================

Checks per launch.  (1) All rows against the unfused pair ``ops.residual_layernorm(ops.gemm(...))`` at <= 1e-6 max |pair| (the
bound tests/test_kernels_gpu.py asserts; the pair is itself pinned to fp64 by the GEMM and row-op forms tests).  (2) Whole
row groups -- the first workgroup of each walk order (blocks 0, 8, 16, 24), the two before the last and the last, short one
-- against fp64 with the per-row allowance of tests/rowln_ref.py.  (3) The plane-fed entry point bit-identical to the
fp32-row one.  (4) A second launch bit-identical to the first (no atomics).  (5) Sentinel rows behind the output bit-unchanged
and no sentinel left in it.  Inputs: tests/rowln_ref.py (rows x 1e3 and x 1e-3; every row differs from the rows 32, 64 and 96
places after it, so a tile that reads its predecessor's LDS image cannot pass).  No case is shaped to fault: the guards
exist so that an overrun lands inside the allocation and fails an assertion.

Measured on an MI355X (256 CUs), largest figure per arithmetic, f16x3 / bf16x3 [asserted]:
  test_row_group_walks                 err / allowance 0.092 / 0.070 [1];  |fused - pair| / max |pair| 2.2e-7 / 2.3e-7 [1e-6]
  test_short_reductions_across_tiles   err / allowance 0.071 / 0.062 [1];  |fused - pair| / max |pair| 2.2e-7 / 1.9e-7 [1e-6]
  test_abi_edges, "spread" residual    err / allowance 0.076 / 0.066 [1];  no_bias without a residual 0.205 (f16x3)
  test_abi_edges, "large_mean"         err / allowance 0.710 / 0.582 [1]:  the rows x 1e-3, where the allowance is little more
                                       than 2e-6 of |out| and z = 40 + ... is rounded to an ulp of 40 (3.8e-6) before the
                                       statistics; torch's fp32 evaluation of the same rows uses 0.82 / 0.68 of it
                                       (tests/test_rowln_ref_cpu.py).  Without the residual 0.076 / 0.055.
  test_abi_edges[out_scale]            the scaled launch equals the unscaled one bit for bit (0 of the allowance [1])
  test_predicate_and_routes            the pair at M = 8208: err / allowance 0.075 / 0.069 [1]
Every test prints its figures (``record``); each case takes 0.05 - 1.2 s, the whole file about 15 s.
"""
import pytest
import torch

import rowln_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
N = R.RN
G = 16                  # guard rows
SENTINEL = -7777.25
SENTINEL_BITS = int(torch.tensor(SENTINEL).view(torch.int32))
PAIR_BOUND = 1e-6       # of max |pair| (tests/test_kernels_gpu.py::test_gemm_rowln_matches_the_unfused_pair)

FIGURES = {}            # (test, mode) -> [largest err / allowance, largest |fused - pair| / max |pair|]


# ----------------------------------------------------------------------------------------------------- plumbing
def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def n_cu(hip):
    return R.cu_count(torch.cuda.get_device_properties(0).multi_processor_count)


_PARAMS = {}


def params(K):
    """((w, bias, gamma, beta) on the CPU, the same on the device); the device weight carries its plane cache."""
    if K not in _PARAMS:
        cpu = R.params(K)
        _PARAMS[K] = (cpu, tuple(t.to(DEV).contiguous() for t in cpu))
    return _PARAMS[K]


class Out:
    """An [M, 768] output, row stride ``ld``, at column ``col0`` of a sentinel-filled [M + 2 G, ld] allocation."""

    def __init__(self, M, ld=N, col0=0):
        self.M = M
        self.big = torch.full((M + 2 * G, ld), SENTINEL, device=DEV)
        self.v = self.big[G:G + M, col0:col0 + N]
        self.ld, self.col0 = ld, col0

    def get(self, what):
        guard = bits(self.big) == SENTINEL_BITS
        inside = guard[G:G + self.M, self.col0:self.col0 + N]
        assert not bool(inside.any()), f"{what}: {int(inside.sum())} output words were never written"
        inside.fill_(True)
        assert bool(guard.all()), f"{what}: {int((~guard).sum())} words outside the output were written"
        return self.v.contiguous()


def launch(pkg, a, w_planes, bias, res, gamma, beta, eps, out, terms, scale, what):
    """One launch; ``a`` is a row-strided fp32 view (the fp32-row entry point) or ``ops.ActPlanes`` (the plane one)."""
    lib = pkg.hip.lib()
    M, K = a.shape
    ldr = 0 if res is None else res.stride(0)
    tail = (_p(bias), _p(res), ldr, _p(gamma), _p(beta), eps, _p(out.v), out.ld, M, N, K, terms, scale, _s())
    if isinstance(a, pkg.ops.ActPlanes):
        assert a.terms == terms
        pkg.hip.check(lib.e3d_gemm_residual_layernorm_planes_split(_p(a.data), _p(w_planes), *tail), what)
    else:
        assert a.stride(1) == 1
        pkg.hip.check(lib.e3d_gemm_residual_layernorm_f32_split(_p(a), a.stride(0), _p(w_planes), *tail), what)
    torch.cuda.synchronize()
    return out.get(what)


def both_entry_points_twice(pkg, a, planes, w_planes, bias, res, gamma, beta, eps, terms, scale, what, ld=N, col0=0):
    """fp32 rows twice and planes once, each into a fresh guarded output: the same bits.  Returns the result."""
    got = launch(pkg, a, w_planes, bias, res, gamma, beta, eps, Out(a.shape[0], ld, col0), terms, scale, what)
    again = launch(pkg, a, w_planes, bias, res, gamma, beta, eps, Out(a.shape[0], ld, col0), terms, scale, what)
    assert torch.equal(bits(got), bits(again)), f"{what}: a second launch differs"
    fed = launch(pkg, planes, w_planes, bias, res, gamma, beta, eps, Out(a.shape[0], ld, col0), terms, scale, what + " (planes)")
    assert torch.equal(bits(got), bits(fed)), f"{what}: the plane-fed entry point differs from the fp32-row one"
    return got


def fp64_rows(got, rows, a, cpu, bias_on, res, eps, terms, what, scale=1.0):
    """Rows ``rows`` (an index tensor, or None for all) of ``got`` against the fp64 statement; the largest err / allowance."""
    w, b, ga, be = cpu
    pick = (lambda t: t.cpu()) if rows is None else (lambda t: t[rows].cpu())
    return R.check_rows(pick(got), pick(a), w, b if bias_on else None, None if res is None else pick(res), ga, be, eps, terms,
                        what, out_scale=scale)


def record(test, mode, excess, pair=None):
    f = FIGURES.setdefault((test, mode), [0.0, 0.0])
    f[0], f[1] = max(f[0], excess), max(f[1], pair or 0.0)
    line = f"{test} {mode}: err / allowance {excess:.3f} (so far {f[0]:.3f}) [1]"
    if pair is not None:
        line += f", |fused - pair| / max |pair| {pair:.2e} (so far {f[1]:.2e}) [{PAIR_BOUND:g}]"
    print(line)


def check_walk(pkg, n_cu, test, M, K, mode):
    """The checks of the module docstring at one (M, K, arithmetic), with and without a residual."""
    terms = R.MODES[mode]
    cpu, (wd, bd, gd, bed) = params(K)
    a, res = R.inputs(M, K, "spread", DEV)
    assert R.rows_differ(a) and R.rows_differ(res)
    w_planes, scale = pkg.ops.weight_planes(wd, terms)
    planes = pkg.ops.activation_planes(a, mode=mode)
    blocks = R.checked_blocks(M, n_cu)
    rows = torch.cat([torch.arange(*R.block_rows(M, n_cu, b)) for b in blocks]).to(DEV)
    rpw, grid, last = R.group_rows(M, n_cu)
    for r in (res, None):
        what = f"{test} M={M} ({grid} groups of {rpw}, last {last}) K={K} {mode} residual={r is not None}"
        got = both_entry_points_twice(pkg, a, planes, w_planes, bd, r, gd, bed, 1e-12, terms, scale, what)
        pair = pkg.ops.residual_layernorm(pkg.ops.gemm(a, wd, bd, mode=mode), r, gd, bed, 1e-12)
        d = float((got - pair).abs().max()) / float(pair.abs().max())
        excess = fp64_rows(got, rows, a, cpu, True, r, 1e-12, terms, what)
        record(test, mode, excess, d)
        assert d <= PAIR_BOUND, f"{what}: |fused - pair| = {d:.3g} of max |pair|"


# ----------------------------------------------------------------------------------------------------- the walks
@pytest.mark.parametrize("g", R.GROUPS)
@pytest.mark.parametrize("K", R.WALK_KS)
@pytest.mark.parametrize("mode", list(R.MODES))
def test_row_group_walks(pkg, hip, n_cu, mode, K, g):
    M = R.smallest_m(g, n_cu)
    assert R.group_rows(M, n_cu)[0] == g
    check_walk(pkg, n_cu, "walks", M, K, mode)


@pytest.mark.parametrize("g", [96, 256])
@pytest.mark.parametrize("K", R.SHORT_KS)
@pytest.mark.parametrize("mode", list(R.MODES))
def test_short_reductions_across_tiles(pkg, hip, n_cu, mode, K, g):
    """Two, three and four k32 pairs (and 32 of them) where a workgroup has a further tile to prefetch: one 96-row tile
    per workgroup, and the four orders of a 256-row group."""
    M = R.smallest_m(g, n_cu)
    assert R.group_rows(M, n_cu)[0] == g
    check_walk(pkg, n_cu, "short reductions", M, K, mode)


# ----------------------------------------------------------------------------------------------------- ABI edges
def block_of(x, ld, col0, fill=NAN):
    """x [M, C] as columns col0 .. col0 + C of a [M + G, ld] buffer of ``fill`` (NaN: padding columns and the rows from M on)."""
    M, C = x.shape
    buf = torch.full((M + G, ld), fill, device=DEV)
    buf[:M, col0:col0 + C] = x
    return buf[:M, col0:col0 + C]


@pytest.mark.parametrize("case", R.ABI_CASES, ids=lambda c: c[0])
def test_abi_edges(pkg, hip, n_cu, case):
    """out = block [G : G + M, 8 : 8 + 768] of a sentinel buffer with ldo = 800; A = columns 16 .. 16 + K of a NaN buffer with
    lda = K + 32; the residual = columns 32 .. 32 + 768 of a NaN buffer with ldr = 832; NaN rows from M on in both.  Every
    row against fp64."""
    name, mode, family, bias_on, wexp, eps = case
    terms, K = R.MODES[mode], R.ABI_K
    M = R.smallest_m(64, n_cu)
    cpu, (wd, bd, gd, bed) = params(K)
    a0, res0 = R.inputs(M, K, family, DEV)
    a, res = block_of(a0, K + 32, 16), block_of(res0, N + 64, 32)
    assert a.data_ptr() % 16 == 0 and res.data_ptr() % 16 == 0 and a.stride(0) == K + 32 and res.stride(0) == N + 64
    planes = pkg.ops.activation_planes(a, mode=mode)
    w_planes, scale = pkg.ops.weight_planes(wd, terms)
    bias = bd if bias_on else None
    for r in (res, None):
        what = f"abi {name} M={M} K={K} {mode} residual={r is not None}"
        got = both_entry_points_twice(pkg, a, planes, w_planes, bias, r, gd, bed, eps, terms, scale, what, ld=N + 32, col0=8)
        excess = fp64_rows(got, None, a0, cpu, bias_on, None if r is None else res0, eps, terms, what)
        if wexp:
            # the weight times 2^wexp (exact), undone by out_scale on the accumulators: the unscaled launch to the allowance
            assert terms == 3 and scale == 1.0
            scaled_planes, s2 = pkg.ops.weight_planes((wd * 2.0 ** wexp).contiguous(), terms)
            assert s2 == 1.0
            scaled = both_entry_points_twice(pkg, a, planes, scaled_planes, bias, r, gd, bed, eps, terms, 2.0 ** -wexp,
                                             what + " scaled", ld=N + 32, col0=8)
            excess = max(excess, fp64_rows(scaled, None, a0, cpu, bias_on, None if r is None else res0, eps, terms, what + " scaled"))
            ref, prod, zhat, rstd = R.statement(a0.cpu(), cpu[0], cpu[1] if bias_on else None, None if r is None else res0.cpu(),
                                                cpu[2], cpu[3], eps)
            worst, row = R.row_excess(scaled, got.double().cpu(), R.allowance(ref, prod, zhat, rstd, cpu[2], terms))
            print(f"{what}: scaled against unscaled launch {worst:.3g} of the allowance (bit-equal: {torch.equal(scaled, got)})")
            assert worst <= 1.0, f"{what}: out_scale changes row {row} by {worst:.3g} of its allowance"
        record("abi " + name, mode, excess)


# ----------------------------------------------------------------------------------------------------- predicate, routes
REFUSED = [(0, N, 64, 64), (16, N, 64, 64), (48, N, 64, 64), (-32, N, 64, 64), (96, 512, 64, 64), (96, 1024, 64, 64),
           (96, N, 32, 32), (96, N, 80, 80), (96, N, 48, 48), (96, N, 64, 60), (96, N, 64, 66), (96, N, 64, 12_000_000),
           (96, N, 64, 2 ** 30 // 96 // 4 * 4 + 4), (8192 + 16, N, 96, 96)]
ACCEPTED = [(32, N, 64, 64), (96, N, 96, 128), (81952, N, 768, 768), (96, N, 64, 2 ** 30 // 96 // 4 * 4), (8224, N, 1024, 1056)]


def test_predicate_and_routes(pkg, hip, monkeypatch):
    ok = hip.e3d_gemm_residual_layernorm_supported
    for shape in ACCEPTED:
        assert ok(*shape), shape
    # refusing shapes only: nothing is launched, the message names the rule and the output keeps its bits
    buf, out = torch.zeros(96 * 128, device=DEV), Out(96)
    before = out.big.clone()
    for M, Nn, K, lda in REFUSED:
        assert not ok(M, Nn, K, lda), (M, Nn, K, lda)
        rc = hip.e3d_gemm_residual_layernorm_f32_split(_p(buf), lda, _p(buf), _p(buf), None, 0, _p(buf), _p(buf), 1e-12, _p(out.v), N,
                                                       M, Nn, K, 19, 1.0, _s())
        msg = hip.e3d_last_error().decode(errors="replace")
        assert rc != 0 and "gemm_residual_layernorm" in msg and f"M={M}" in msg, (M, Nn, K, lda, rc, msg)
        if not ok(M, Nn, K, K):         # the plane entry point has no lda: it asks the predicate with lda = K
            rc = hip.e3d_gemm_residual_layernorm_planes_split(_p(buf), _p(buf), _p(buf), None, 0, _p(buf), _p(buf), 1e-12, _p(out.v), N,
                                                              M, Nn, K, 19, 1.0, _s())
            msg = hip.e3d_last_error().decode(errors="replace")
            assert rc != 0 and "(planes)" in msg, (M, Nn, K, rc, msg)
    for ldr in (N - 4, N + 2, 80_000_000):      # the residual's rules are the entry points' own
        rc = hip.e3d_gemm_residual_layernorm_f32_split(_p(buf), 64, _p(buf), _p(buf), _p(buf), ldr, _p(buf), _p(buf), 1e-12, _p(out.v),
                                                       N, 96, N, 64, 19, 1.0, _s())
        assert rc != 0 and "residual" in hip.e3d_last_error().decode(errors="replace"), ldr
    torch.cuda.synchronize()
    assert torch.equal(bits(out.big), bits(before)), "a refused call wrote its output"

    # ops.rowln_ok, the host predicate of the wrappers: no launch
    monkeypatch.setattr(pkg.ops, "ROWLN_MIN_M", 8192)
    M, K = 8192, 64
    flat_a, flat_r = torch.zeros(M * K + 4, device=DEV), torch.zeros(M * N + 4, device=DEV)
    a, a_off = flat_a[:M * K].view(M, K), flat_a[1:1 + M * K].view(M, K)
    r, r_off = flat_r[:M * N].view(M, N), flat_r[1:1 + M * N].view(M, N)
    r_ld = torch.zeros(M, N + 2, device=DEV)[:, :N]
    assert a.data_ptr() % 16 == 0 and a_off.data_ptr() % 16 == 4 and r_off.data_ptr() % 16 == 4 and r_ld.stride(0) % 4 == 2
    assert pkg.ops.rowln_ok(19, M, N, K, a, r) and pkg.ops.rowln_ok(3, M, N, K, a, None) and pkg.ops.rowln_ok(19, M, N, K, None, r)
    assert not pkg.ops.rowln_ok(19, M, N, K, a_off, r) and not pkg.ops.rowln_ok(19, M, N, K, a_off, None)
    assert not pkg.ops.rowln_ok(19, M, N, K, a, r_off) and not pkg.ops.rowln_ok(19, M, N, K, None, r_off)
    assert not pkg.ops.rowln_ok(19, M, N, K, a, r_ld) and not pkg.ops.rowln_ok(19, M, N, K, None, r_ld)
    assert not pkg.ops.rowln_ok(19, M - 32, N, K, a[:M - 32], None) and not pkg.ops.rowln_ok(0, M, N, K, a, r)

    # M = 8192 + 16 is no whole 32-row block: the wrapper takes the pair, and the pair matches fp64
    M, K = 8192 + 16, 96
    cpu, (wd, bd, gd, bed) = params(K)
    a, res = R.inputs(M, K, "spread", DEV)
    for mode, terms in R.MODES.items():
        assert not pkg.ops.rowln_ok(terms, M, N, K, a, res)
        monkeypatch.setattr(pkg.ops, "TRACE", [])
        got = pkg.ops.linear_residual_layernorm(a, wd, bd, res, gd, bed, 1e-12, mode=mode)
        torch.cuda.synchronize()
        assert [rec[0] for rec in pkg.ops.TRACE] == ["gemm", "residual_layernorm"], [rec[0] for rec in pkg.ops.TRACE]
        monkeypatch.setattr(pkg.ops, "TRACE", None)
        record("route M % 32 != 0", mode, fp64_rows(got, None, a, cpu, True, res, 1e-12, terms, f"pair at M={M} {mode}"))
