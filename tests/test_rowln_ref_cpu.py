"""tests/rowln_ref.py checked without a GPU.

1. The mirrors of the kernel's host arithmetic (``group_rows`` = launch_rowln, ``walk`` = next_tile_rows) against the row
   groups and walks written out by hand for a 256-CU device: a wrong mirror would make the GPU forms test check the wrong
   rows and describe the wrong launches.
2. The fp64 statement against torch's own layer_norm in float64.
3. The per-row allowance, for every input family, K and case the GPU forms test uses: not vacuous (allow_r <= 1e-3 of the
   row's largest |out|) and not too tight (torch's fp32 matmul + layer_norm pass it).  An input that fails either is changed,
   never the allowance.
"""
import pytest
import torch
import torch.nn.functional as F

import rowln_ref as R

N_CU = 256
# g -> (smallest M with g-row groups on 256 CUs, rows of its last workgroup, the walk of a full group)
BY_HAND = {
    128: (24608, 32, [64, 64]),
    160: (32800, 160, [96, 64]),
    192: (40992, 96, [96, 96]),
    224: (49184, 128, [96, 64, 64]),
    256: (57376, 32, [96, 96, 64]),
    288: (65568, 192, [96, 96, 96]),
    320: (73760, 160, [96, 96, 64, 64]),
    352: (81952, 288, [96, 96, 96, 64]),
}


# ----------------------------------------------------------------------------------------------------- host arithmetic
def test_cu_count_rounds_down_to_eight():
    assert [R.cu_count(n) for n in (256, 260, 304, 255, 8, 7, 1)] == [256, 256, 304, 248, 8, 8, 8]


@pytest.mark.parametrize("g", R.GROUPS)
def test_smallest_m_and_groups_on_256_cus(g):
    M, last, tiles = BY_HAND[g]
    assert R.smallest_m(g, N_CU) == M
    rpw, grid, got_last = R.group_rows(M, N_CU)
    assert (rpw, got_last) == (g, last) and (grid - 1) * g + last == M and grid <= N_CU + 1
    assert R.group_rows(M - 32, N_CU)[0] == g - 32          # the smallest: 32 rows fewer give the next smaller group
    assert R.walk(g, 0) == tiles and sum(tiles) == g
    if g != 256:                                            # only a 256-row group has orders
        assert all(R.walk(g, p) == tiles for p in range(4))
    assert sum(R.walk(last, 1)) == last


def test_group_rows_of_the_shapes_older_tests_launch():
    """tests/test_kernels_gpu.py and tests/test_activation_planes_gpu.py on 256 CUs: groups of 32, 64, 96 and 256 rows, one
    224-row last group."""
    assert R.group_rows(4096, N_CU) == (32, 128, 32)
    assert R.group_rows(8192 + 160, N_CU) == (64, 131, 32)
    assert R.group_rows(16384, N_CU) == (64, 256, 64)
    assert R.group_rows(24576, N_CU) == (96, 256, 96)
    assert R.group_rows(65536, N_CU) == (256, 256, 256)
    assert R.group_rows(65536 - 32, N_CU) == (256, 256, 224)
    assert R.group_rows(32768, N_CU) == (128, 256, 128)     # 256 pockets at L = 128
    assert R.group_rows(32, N_CU) == (32, 1, 32) and R.group_rows(288, 8) == (64, 5, 32)


def test_walks():
    assert R.walk(32) == [32] and R.walk(64) == [64] and R.walk(96) == [96]
    assert [R.walk(256, p) for p in range(4)] == [[96, 96, 64], [64, 96, 96], [96, 64, 96], [64, 64, 64, 64]]
    assert [R.pattern_of(b) for b in (0, 7, 8, 16, 24, 31, 32, 255)] == [0, 0, 1, 2, 3, 3, 0, 3]
    assert R.walk(224, 3) == [96, 64, 64] and R.walk(128, 1) == [64, 64]      # a short last group of a 256-row launch
    for g in range(32, 1025, 32):
        for p in range(4):
            t = R.walk(g, p)
            assert sum(t) == g and set(t) <= {32, 64, 96} and (32 not in t or g == 32)


def test_checked_blocks_cover_every_order_and_the_short_group():
    for g in R.GROUPS:
        M = R.smallest_m(g, N_CU)
        blocks = R.checked_blocks(M, N_CU)
        grid = R.group_rows(M, N_CU)[1]
        assert {R.pattern_of(b) for b in blocks} == {0, 1, 2, 3} and blocks[-1] == grid - 1 and len(blocks) == 7
        rows = sum(e - s for s, e in (R.block_rows(M, N_CU, b) for b in blocks))
        assert rows == 6 * g + BY_HAND[g][1] <= 2500
        assert R.block_rows(M, N_CU, grid - 1) == (M - BY_HAND[g][1], M)


# ----------------------------------------------------------------------------------------------------- statement
def test_statement_matches_torch_in_float64():
    K = 96
    w, b, ga, be = R.params(K)
    a, res = R.inputs(64, K)
    for r in (res, None):
        for bias in (b, None):
            for eps in (1e-12, 1e-2):
                z = a.double() @ w.double().t() * 0.125 + (0 if bias is None else bias.double()) + (0 if r is None else r.double())
                want = F.layer_norm(z, (R.RN,), ga.double(), be.double(), eps)
                out, prod, zhat, rstd = R.statement(a, w, bias, r, ga, be, eps, out_scale=0.125)
                assert float((out - want).abs().max()) <= 1e-12 * float(want.abs().max())
                assert torch.equal(prod, a.double() @ w.double().t() * 0.125)
                assert float((zhat.var(1, unbiased=False) + eps * rstd ** 2 - 1).abs().max()) <= 1e-12       # biased variance, eps inside
    # a power-of-two pre-multiplier on the weight and its inverse as out_scale: the same statement, exactly
    assert torch.equal(R.statement(a, w * 8, b, res, ga, be, 1e-12, out_scale=0.125)[0], R.statement(a, w, b, res, ga, be, 1e-12)[0])


def test_inputs_are_what_the_families_say():
    for fam in R.FAMILIES:
        a, res = R.inputs(1024, 64, fam)
        big, small = a[::97].abs().mean(), a[5::101].abs().mean()
        assert 500 < float(big) < 1200 and 5e-4 < float(small) < 1.2e-3
        assert R.rows_differ(a) and R.rows_differ(res)
        mean, spread = float(res.mean()), float(res.std())
        assert (abs(mean - 0.5) < 0.02 and abs(spread - 3) < 0.02) if fam == "spread" else (abs(mean - 40) < 0.01 and abs(spread - 0.5) < 0.01)
        again = R.inputs(1024, 64, fam)
        assert torch.equal(a, again[0]) and torch.equal(res, again[1])
    assert not R.rows_differ(torch.arange(64.0).remainder(32).reshape(64, 1).expand(64, 4))
    w, b, ga, be = R.params(768)
    assert abs(float(w.std()) * 768 ** 0.5 - 1) < 0.01 and 0.5 <= float(ga.min()) and float(ga.max()) < 1.5


# ----------------------------------------------------------------------------------------------------- allowance
def allowance_figures(K, family, mode, with_bias, with_res, eps, what):
    M = 1024                 # 11 rows x 1e3, 11 rows x 1e-3
    w, b, ga, be = R.params(K)
    a, res = R.inputs(M, K, family)
    bias, r = (b if with_bias else None), (res if with_res else None)
    ref, prod, zhat, rstd = R.statement(a, w, bias, r, ga, be, eps)
    allow = R.allowance(ref, prod, zhat, rstd, ga, R.MODES[mode])
    vac = float((allow / ref.abs().amax(1)).max())
    tight, row = R.row_excess(R.statement_f32(a, w, bias, r, ga, be, eps), ref, allow)
    print(f"{what}: allowance <= {vac:.2e} of a row's largest |out|; fp32 torch uses {tight:.3f} of it (row {row})")
    assert vac <= 1e-3, f"{what}: the allowance is {vac:.3g} of a row's own magnitude -- vacuous"
    assert tight <= 1.0, f"{what}: torch's fp32 evaluation misses the allowance at row {row} ({tight:.3g}) -- too tight"


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("mode", list(R.MODES))
@pytest.mark.parametrize("K", sorted(set(R.WALK_KS + R.SHORT_KS)))
def test_allowance_for_the_walk_inputs(K, mode, with_res):
    allowance_figures(K, "spread", mode, True, with_res, 1e-12, f"K={K} {mode} residual={with_res}")


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("case", R.ABI_CASES, ids=lambda c: c[0])
def test_allowance_for_the_abi_cases(case, with_res):
    name, mode, family, with_bias, _, eps = case
    allowance_figures(R.ABI_K, family, mode, with_bias, with_res, eps, f"{name} residual={with_res}")


def test_allowance_rejects_a_wrong_statistic_and_a_stale_tile():
    """What the allowance is for: an unbiased variance, eps left out where it matters, gamma and beta exchanged, a row that
    shows its predecessor tile's result -- each is far outside it."""
    K = 96
    w, b, ga, be = R.params(K)
    a, res = R.inputs(256, K)
    ref, prod, zhat, rstd = R.statement(a, w, b, res, ga, be, 1e-12)
    allow = R.allowance(ref, prod, zhat, rstd, ga, 3)
    assert R.row_excess(ref.float(), ref, allow)[0] <= 1.0
    z = prod + b.double() + res.double()
    unbiased = (z - z.mean(1, keepdim=True)) / z.std(1, keepdim=True) * ga.double() + be.double()
    assert R.row_excess(unbiased, ref, R.allowance(ref, prod, zhat, rstd, ga, 19))[0] > 1.0
    assert R.row_excess(zhat * be.double() + be.double(), ref, allow)[0] > 100
    stale = ref.clone()
    stale[96:128] = ref[64:96]
    assert R.row_excess(stale, ref, allow)[0] > 100
    ref2 = R.statement(a, w, None, None, ga, be, 1e-2)[0]
    parts = R.statement(a, w, None, None, ga, be, 1e-12)
    assert R.row_excess(ref2, parts[0], R.allowance(*parts, ga, 19))[0] > 100
