"""tests/wgrad_ref.py checked without a GPU.

1. The fp64 statement against torch.autograd of a Linear layer, and the accumulate / plain-bf16 variants of it.
2. Coverage: the case table of tests/test_wgrad_forms_gpu.py reaches all twelve (entry point, NS, TR) kernel cells under the
   restated launcher predicate, every predicate term is turned ALONE at least once per entry point (in the ragged launch on
   the first and on the last problem), and every case's staging, tile count and k-tile count are what its id claims.
3. Conditioning: the reference computed from operands moved by one fp32 ulp each, and the fp32-rounded reference moved by
   one ulp, meet the bounds the GPU test asserts -- an input that fails here is too ill-conditioned for any fp32 kernel; the
   input is changed, never the bound.
4. The memory layout the GPU test uses keeps its guards, alignments and NaN padding.
"""
import re

import pytest
import torch
import torch.nn.functional as F

import wgrad_ref as W

CASES = W.all_cases()
IDS = [c.id for c in CASES]


def test_statement_matches_autograd_of_a_linear_layer():
    M, N, K = 37, 12, 20
    p = W.P(N, K, seed=5)
    dz, x = W.operands(M, p)
    w = torch.zeros(N, K, dtype=W.F64, requires_grad=True)
    b = torch.zeros(N, dtype=W.F64, requires_grad=True)
    F.linear(x.double(), w, b).backward(dz.double())
    dW, db = W.statement(dz, x, 3)
    assert float((dW - w.grad).abs().max()) <= 1e-12 * float(dW.abs().max())
    assert float((db - b.grad).abs().max()) <= 1e-12 * float(db.abs().max())
    ow, ob = W.old_contents(M, p)
    aW, ab = W.statement(dz, x, 6, ow, ob)
    assert torch.equal(aW, dW + ow.double()) and torch.equal(ab, db + ob.double())
    rW, rb = W.statement(dz, x, 1)          # plain bf16: rounded operands in the product, fp32 values in the column sums
    assert torch.equal(rW, dz.bfloat16().double().t() @ x.bfloat16().double()) and torch.equal(rb, db)
    assert float((rW - dW).abs().max()) > 1e-4 * float(dW.abs().max())


def test_ids_are_unique():
    assert len(set(IDS)) == len(IDS)
    assert len(CASES) == len({(c.name, c.entry, c.terms, c.M, c.tr) for c in CASES})


def test_every_kernel_cell_is_reached():
    cells = {c.cell for c in CASES}
    assert cells == {(e, ns, tr) for e in W.ENTRIES for ns in (1, 2, 3) for tr in (True, False)}
    for cell in W.CELLS:      # and each by the reduction edges (nk = 1 .. 5, full and partial) and the output edges
        red = W.reduction_cases(*cell)
        assert sorted(c.M for c in red) == [1, 31, 32, 33, 64, 65, 96, 97, 128, 129]
        assert {c.nk for c in red} == {1, 2, 3, 4, 5}
        assert all(c.cell == (cell[0], W.NS[cell[1]], cell[2]) for c in red + W.edge_cases(*cell))
    for tr in W.STAGINGS:
        shapes = {(p.N, p.K) for e in W.ENTRIES for c in W.edge_cases(e, 3, tr) for p in c.probs}
        assert {4, 252, 256, 260} <= {n for n, _ in shapes} and {4, 124, 128, 132} <= {k for _, k in shapes}
        if not tr:
            assert {1, 255, 257} <= {n for n, _ in shapes} and {1, 127, 129} <= {k for _, k in shapes}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_is_what_its_id_claims(case):
    m = re.fullmatch(r".*-(grouped|ragged)-(bf16|bf16x3|bf16x6)-(tr|dword)-t(\d+)-nk(\d+)", case.id)
    assert m and m.group(1) == case.entry and W.MODES[case.terms] == m.group(2)
    assert 1 <= len(case.probs) <= 64
    assert W.launch_tr(case) == (m.group(3) == "tr"), "the staging the launcher's predicate selects"
    assert sum(p.tiles for p in case.probs) == int(m.group(4))
    assert -(-case.M // W.BK) == int(m.group(5))
    if case.entry == "grouped":
        assert len({(p.N, p.K, p.ldz, p.ldx) for p in case.probs}) == 1
    failing = [W.failing_terms(case.M, p) for p in case.probs]
    assert any(failing) == (not case.tr)
    if case.flip is not None:          # exactly one term, exactly where the case says
        term, where = case.flip
        at = {"all": range(len(failing)), "first": [0], "last": [len(failing) - 1]}[where]
        assert all(f == ({term} if i in at else set()) for i, f in enumerate(failing)), failing


def test_every_predicate_term_is_turned_alone():
    for entry in W.ENTRIES:
        flips = {c.flip for c in CASES if c.entry == entry and c.flip}
        assert {t for t, _ in flips} == set(W.PREDICATE_TERMS), entry
        if entry == "ragged":          # one odd problem turns the whole launch: first and last
            for term in W.PREDICATE_TERMS[:6]:
                assert {(term, "first"), (term, "last")} <= flips, term
        for terms in (1, 3, 6):
            assert W.launch_tr(W.flip_base(entry, terms))
    for term in W.SAME_DATA_FLIPS:
        assert (W.FLIPPED[term].N, W.FLIPPED[term].K) == (W.FLIP_BASE.N, W.FLIP_BASE.K)


def test_problem_table_edges():
    cases = {c.id: c for c in W.table_cases()}
    assert {len(c.probs) for c in cases.values() if c.entry == "grouped"} >= {1, 2, 63, 64}
    ragged = [c for c in cases.values() if c.entry == "ragged"]
    assert {c.tiles for c in cases.values()} >= {1, 7, 8, 9, 65}
    assert {c.tiles for c in ragged} >= {1, 7, 8, 9, 64, 65, 148}
    cyc = next(c for c in ragged if c.name == "count64cyc")
    assert [p.tiles for p in cyc.probs[:6]] == [1, 2, 4, 1, 2, 4] and len(cyc.probs) == 64
    for c in cases.values():
        if len(c.probs) == 64:
            want = {"lone_db": (), "count64lo": W.ACC_AT[:2], "count64hi": W.ACC_AT[2:]}.get(c.name, W.ACC_AT)
            assert c.bits == sum(1 << i for i in want)
    assert any(c.db_null and c.bits for c in ragged) and any(c.db_null and c.bits for c in cases.values() if c.entry == "grouped")
    lone = next(c for c in ragged if c.name == "lone_db")
    assert [i for i, p in enumerate(lone.probs) if p.bias] == [0, 17]
    assert any(not p.bias for p in cyc.probs) and any(p.bias and p.tiles == 4 for p in cyc.probs)


def test_predicate_restatement():
    assert W.tr_span_ok(2, (1 << 24) - 4) and not W.tr_span_ok(2, 1 << 24)
    assert W.tr_span_ok((1 << 19) - 1, 1024) and not W.tr_span_ok(1 << 19, 1024)
    assert not W.tr_span_ok(0, 4) and not W.tr_span_ok(4, 0)
    ok = dict(M=8, N=4, K=4, ldz=8, ldx=8, dz_ptrs=[16, 32], x_ptrs=[64, 48])
    assert W.grouped_tr(**ok)
    for k, v in dict(N=6, K=5, ldz=9, ldx=10, dz_ptrs=[16, 36], x_ptrs=[68, 48], M=1 << 28).items():
        assert not W.grouped_tr(**{**ok, k: v}), k
    assert W.ragged_tr(8, [4, 8], [4, 4], [8, 8], [8, 12], [16, 32], [64, 48])
    assert not W.ragged_tr(8, [4, 8], [4, 4], [8, 8], [8, 13], [16, 32], [64, 48])


# ----------------------------------------------------------------------------------------------------- conditioning
def _one_ulp(t, key):
    up = torch.rand(t.shape, generator=W.gen(*key)) < 0.5
    return torch.where(up, torch.nextafter(t, torch.full_like(t, float("inf"))), torch.nextafter(t, torch.full_like(t, float("-inf"))))


SMALL = [c for c in CASES if not c.big]


@pytest.mark.parametrize("case", SMALL, ids=[c.id for c in SMALL])
def test_conditioning(case):
    seen = set()
    for p in case.seeded():
        key = (p.N, p.K, p.seed, p.acc)
        if key in seen:
            continue
        seen.add(key)
        dz, x = W.operands(case.M, p)
        assert dz.shape == (case.M, p.N) and x.shape == (case.M, p.K)
        ref_w, ref_b = W.reference(case.M, p, case.terms)
        old = W.old_contents(case.M, p) if p.acc else (None, None)
        got_w, got_b = W.statement(_one_ulp(dz, (p.N, p.K, 1)), _one_ulp(x, (p.N, p.K, 2)), case.terms, *old)
        what = f"{case.id} problem {p}"
        if case.terms != 1:            # (plain bf16 rounds the operands: a one-ulp move may cross a bf16 rounding boundary)
            W.check_close(got_w, ref_w, W.TOL[case.terms], what + " dW, operands at one ulp")
        W.check_within(got_b, ref_b, W.db_bound(case.M, dz, old[1]), what + " db, operands at one ulp")
        W.check_close(_one_ulp(ref_w.float(), (p.N, 3)), ref_w, W.TOL[case.terms], what + " dW at one ulp")
        W.check_within(_one_ulp(ref_b.float(), (p.N, 4)), ref_b, W.db_bound(case.M, dz, old[1]), what + " db at one ulp")


def test_long_reduction_bound_holds_for_fp32_and_catches_a_wrapped_reduction():
    """The derived bound of the two 2^19-token launches: torch's own fp32 product lies within it, a product that lost the
    rows past 2^18 (a byte count wrapped at 2^30) does not -- and neither does one that lost a sixteenth of them."""
    M, p = 1 << 19, W.P(8, 4, ldz=1024, seed=0, positive=True)
    dz, x = W.operands(M, p)
    ref, _ = W.statement(dz, x, 3)
    bound = W.long_reduction_bound(M, dz, x, ref, 3)
    W.check_within(dz.t() @ x, ref, bound, "fp32 product")
    wrapped, _ = W.statement(dz[:M // 2], x[:M // 2], 3)
    assert not bool(((wrapped - ref).abs() <= bound).any())
    short, _ = W.statement(dz[:M - M // 16], x[:M - M // 16], 3)
    assert not bool(((short - ref).abs() <= bound).any())
    assert all(c.probs[0].positive for c in CASES if c.M >= (1 << 19) - 1)


# ----------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("case", [c for c in CASES if c.name in ("edges", "count64cyc", "flip_dz_plus_4B_last", "span_ld")],
                         ids=lambda c: c.id)
def test_layout_keeps_guards_and_padding(case):
    zo, xo, n_in = W.in_layout(case)
    spans = []
    for p, z, x in zip(case.probs, zo, xo):
        assert (z - W.ZC0 - p.zoff) % 16 == 0 and (x - W.XC0 - p.xoff) % 16 == 0          # buffers start on 64 bytes
        assert z % 4 == p.zoff % 4 and x % 4 == p.xoff % 4 and W.ZC0 >= 4 and W.XC0 >= 4   # a non-zero column offset
        if not case.big:
            spans.append((z - W.ZC0 - p.zoff, (case.M + W.TAIL) * p.ldz))
        spans.append((x - W.XC0 - p.xoff, (case.M + W.TAIL) * p.ldx))
    spans.sort()
    assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= n_in
    wo, bo, n_out = W.out_layout(case)
    blocks = sorted([(o, p.N * p.K, max(W.G_ROWS * p.K, W.G_WORDS)) for o, p in zip(wo, case.probs)]
                    + [(o, p.N, W.G_WORDS) for o, p in zip(bo, case.probs)])
    at = 0
    for o, n, g in blocks:
        assert o - at >= g and g >= W.G_WORDS
        at = o + n
    assert n_out - at >= blocks[-1][2]
