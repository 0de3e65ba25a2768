"""tests/varlen_ref.py checked without a GPU.

1. The segment statement against the additive-mask fp64 statement of the padded frame (the reference model's semantics,
   ``Case.reference`` of tests/test_attention_edges_gpu.py) on the valid rows: 1e-12 relative at randn scale for every
   rel-key case and every cross item that has keys; more than 0.1 apart on the large-score case built to separate them.
2. The mirrors of the host arithmetic: ``layout`` against packing.PackedLayout, the clamp marks of the rel-key cases
   against the table blocks the kernel loads, the workgroup shapes the case list promises.
3. The sharp case: rows all but one-hot, and no row whose two LARGEST scores lie closer than 1e-3 |s|max.  (Any two scores
   of a 64-key row of std 256 lie that close somewhere; only a tie at the top can decide a row, a pair further down
   carries weight exp(-gap to the top) whichever way it is ordered.)
4. The figures: the per-segment rule catches what the whole-output rule lets through.
"""
import pytest
import torch

import varlen_ref as R


# ----------------------------------------------------------------------------------------------------- semantics
@pytest.mark.parametrize("case", R.RELKEY_CASES, ids=lambda c: c.name)
def test_segments_equal_the_additive_mask_frame_at_randn_scale_relkey(case):
    inp = R.relkey_inputs(case)
    L = max(case.lengths)
    qf, kf, vf = R.frames(inp, L, L)
    frame = R.additive_mask_statement(qf, kf, vf, case.lengths, case.nh, inp.E, case.P)
    for s, n in enumerate(case.lengths):
        assert inp.ref[s].shape == (n, case.nh * 64) and inp.ref[s].dtype == torch.float64
        if n:
            assert R.rel_err(inp.ref[s], frame[s, :n]) <= 1e-12, s


def test_segments_equal_the_additive_mask_frame_at_randn_scale_cross():
    """Every cross item with queries and keys.  The keyless item has no counterpart: the additive statement spreads its
    rows evenly over the padding (packing.check_cross refuses such a batch); the segment statement gives zero rows."""
    inp = R.cross_inputs()
    qf, kf, vf = R.frames(inp, R.CROSS_FRAME, R.CROSS_FRAME)
    frame = R.additive_mask_statement(qf, kf, vf, R.CROSS_K, R.CROSS_NH)
    compared = 0
    for s, (nq, nk) in enumerate(zip(R.CROSS_Q, R.CROSS_K)):
        if nq and nk:
            assert R.rel_err(inp.ref[s], frame[s, :nq]) <= 1e-12, s
            compared += 1
        elif nq:
            assert inp.ref[s].shape == (nq, inp.H) and not inp.ref[s].any()
            assert torch.isfinite(frame[s]).all() and frame[s, :nq].abs().max() > 0.01
    assert compared == 4 and R.CROSS_K[-1] == 0 and R.CROSS_Q[-1] > 0 and R.CROSS_Q[1] == 0 and R.CROSS_K[1] > 0


def test_large_scores_separate_the_two_statements():
    inp, (qf, kf, vf) = R.contract_case()
    lens, L = R.CONTRACT["lengths"], R.CONTRACT["L"]
    frame = R.additive_mask_statement(qf, kf, vf, lens, inp.nh, inp.E, inp.P)
    short, full = lens.index(min(lens)), lens.index(L)
    assert R.rel_err(inp.ref[short], frame[short, :lens[short]]) > 0.1       # padded keys win the short item's rows
    assert R.rel_err(inp.ref[full], frame[full]) <= 1e-12                    # no padding: nothing to part over
    assert R.rel_err(torch.cat(inp.ref), torch.cat([frame[b, :n] for b, n in enumerate(lens)])) > 0.1
    # exact small integers, as the construction promises
    for x in (qf, kf, inp.E):
        assert torch.equal(x, x.round()) and float(x.abs().max()) <= 92


# ----------------------------------------------------------------------------------------------------- host arithmetic
@pytest.mark.parametrize("padded", [False, True])
def test_layout_mirrors_packed_layout(pkg, padded):
    for lengths, L in [(c.lengths, c.P) for c in R.RELKEY_CASES] + [(R.CROSS_Q, R.CROSS_FRAME), (R.CROSS_K, R.CROSS_FRAME),
                                                                     ([0, 0], 32), (R.PLACEMENT["packed"], 40)]:
        lay = pkg.packing.PackedLayout(lengths, L, "cpu", padded_frame=padded)
        assert R.layout(lengths, L, padded) == (lay.starts, lay.rows, lay.total)
        assert R.units(lengths, 3, padded)[0] == lay.n_tiles


@pytest.mark.parametrize("case", R.RELKEY_CASES, ids=lambda c: c.name)
def test_clamp_marks_follow_from_the_table_blocks(case):
    P, longest = case.P, max(case.lengths)
    low, high = R.clamps(P, case.lengths)
    assert (low, high) == (case.low, case.high)
    # the conditions in closed form
    assert low == (P % 32 != 0 and longest > 32 * (P // 32))
    assert high == any(q0 > P - 33 for n in case.lengths for q0 in range(0, n, 32))
    assert longest <= P


def test_table_blocks_cover_the_distances_of_their_tiles():
    """Block ``q0 - r0 - 32 + P`` and the one 32 rows above it hold row l - r + P - 1 of every (l, r) of the tile pair."""
    for P, L in ((16, 16), (33, 33), (100, 97), (64, 64)):
        blocks = R.table_blocks(P, L)
        per_tile = 1 + -(-L // 32)
        for t, q0 in enumerate(range(0, L, 32)):
            assert blocks[t * per_tile] == q0 + P
            for kt, r0 in enumerate(range(0, L, 32)):
                lo = blocks[t * per_tile + 1 + kt]
                need = [l - r + P - 1 for l in range(q0, min(q0 + 32, L)) for r in range(r0, min(r0 + 32, L))]
                assert lo <= min(need) and max(need) <= lo + 63 and 0 <= min(need) and max(need) <= 2 * P - 2


def test_cases_reach_the_workgroup_shapes_they_name():
    by = R.RELKEY_BY_NAME
    u = {n: R.units(c.lengths, c.nh) for n, c in by.items()}
    assert u["P16"] == (6, 18, 5) and u["P16"][1] % 4 != 0                   # an idle wave next to working ones
    assert u["P33"] == (7, 7, 2) and R.layout(by["P33"].lengths, 33)[1:] == (128, 99)   # tail entry = unit 6, with 4 and 5
    assert R.layout(by["P96"].lengths, 96)[1:] == (192, 192) and u["P96"][0] == 6        # no tail entry
    assert R.layout(by["P64"].lengths, 64)[2] == 161
    assert sorted({-(-n // 32) for c in R.RELKEY_CASES for n in c.lengths}) == [0, 1, 2, 3, 4]   # key tiles: both parities
    assert {c.nh for c in R.RELKEY_CASES} == {1, 3, 5}
    assert all(R.CROSS_PAD[n] % 4 == r for n, r in (("q", 0), ("k", 0), ("v", 2))) and len(set(R.CROSS_PAD.values())) == 3
    assert R.layout([0, 0], 32) == ([0, 0], 32, 0) and R.units([0, 0], 3) == (1, 3, 1)


# ----------------------------------------------------------------------------------------------------- sharp rows
def test_sharp_case_is_one_hot_and_decided_by_no_tie():
    inp = R.sharp_inputs()
    rows = hot = 0
    gap, smax = float("inf"), 0.0
    for q, k, v in zip(inp.q, inp.k, inp.v):
        _, s = R.segment_statement(q, k, v, inp.nh, inp.E, inp.P, want_scores=True)
        p = torch.softmax(s, -1)
        rows += p.shape[0] * p.shape[1]
        hot += int((p.amax(-1) > 0.99).sum())
        if s.shape[-1] > 1:
            top = s.topk(2, -1).values
            gap = min(gap, float((top[..., 0] - top[..., 1]).min()))
        smax = max(smax, float(s.abs().max()))
    print(f"sharp seed {R.SHARP['seed']}: {hot} of {rows} rows above 0.99; smallest top gap {gap:.3f}, |s|max {smax:.1f}")
    assert hot >= 0.9 * rows
    assert gap >= 1e-3 * smax
    assert smax > 500                                                       # the regime: scores of std ~256


# ----------------------------------------------------------------------------------------------------- figures
def test_per_segment_rule_catches_what_the_whole_output_rule_passes():
    g, tol = R.gen(3), 1e-5
    ref = [0.05 * torch.randn(40, 64, generator=g, dtype=R.F64), torch.randn(0, 64, dtype=R.F64),
           torch.randn(5, 64, generator=g, dtype=R.F64)]                     # a segment of small outputs next to a large one
    scale = [float(r.abs().max()) for r in (ref[0], ref[2])]
    assert scale[1] > 5 * scale[0]
    ok = lambda figs: all(e < b for _, e, b in figs)  # noqa: E731
    assert ok(R.figures([r.float() for r in ref], ref, tol, "fp32-rounded"))
    off = [r.clone() for r in ref]
    off[0][3, 7] += 0.9 * tol * scale[1]                                    # inside the whole-output bound ...
    figs = R.figures(off, ref, tol, "off")
    assert figs[0][1] < tol and not ok(figs)                                # ... and outside segment 0's own
    with pytest.raises(AssertionError):
        R.report(figs)
    nan = [r.clone() for r in ref]
    nan[2][0, 0] = R.NAN
    assert not ok(R.figures(nan, ref, tol, "nan"))
    # a keyless segment must be exactly zero
    zero = [torch.zeros(3, 64, dtype=R.F64)]
    assert ok(R.figures([torch.zeros(3, 64)], zero, tol, "zero")) and not ok(R.figures([torch.full((3, 64), 1e-30)], zero, tol, "tiny"))
