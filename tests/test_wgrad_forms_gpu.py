"""Every batched weight-gradient kernel instantiation, forced one by one through the C ABI, against the fp64 statement of
tests/wgrad_ref.py (whose case table, predicate restatement and input conditioning tests/test_wgrad_ref_cpu.py checks).

``e3d_gemm_wgrad_grouped_f32_split`` (one shape, up to 64 problems) and ``e3d_gemm_wgrad_ragged_f32_split`` (any shapes; every
weight and bias gradient of a training step leaves through it) launch twelve instantiations of the shared workgroup body:
NS = bf16 terms per operand (terms 1 / 3 / 6 and 19), TR = the transposing float4 / buffer-descriptor staging against the
dword staging.  Nothing but the operands selects the staging, so each cell is forced by the operand property its launcher's
predicate reads.  One row per ``go(...)`` launch site of csrc/gemm_split.hip (every test id below carries the cell as
``<entry>-<arithmetic>-<tr|dword>``):

====  ====================================  ==================================================  ================================================
line  instantiation                         forced by                                           test id
====  ====================================  ==================================================  ================================================
1397  gemm_wgrad_grouped_kernel<1, true>    terms 1; N, K, ldz, ldx in quads, dz | x 16-B        test_reduction_edges[grouped-bf16-tr], test_output_edges[grouped-bf16-tr]
1398  gemm_wgrad_grouped_kernel<1, false>   terms 1; N = 257 / one predicate term turned         test_reduction_edges[grouped-bf16-dword], test_output_edges[grouped-bf16-dword], test_staging_predicate[flip_*-grouped-bf16-dword-*]
1401  gemm_wgrad_grouped_kernel<2, true>    terms 3; quads, aligned, in span                     test_reduction_edges[grouped-bf16x3-tr], test_output_edges[grouped-bf16x3-tr], test_problem_table[count*-grouped-*], test_tr_span[span_under-grouped-*]
1402  gemm_wgrad_grouped_kernel<2, false>   terms 3; a term turned; ld >= 2^24; M ld 4 >= 2^31   test_reduction_edges[grouped-bf16x3-dword], test_output_edges[grouped-bf16x3-dword], test_staging_predicate[flip_*-grouped-bf16x3-dword-*], test_tr_span[span_ld-grouped-*|span_bytes-grouped-*]
1405  gemm_wgrad_grouped_kernel<3, true>    terms 6 and 19 (bit-identical); quads, aligned       test_reduction_edges[grouped-bf16x6-tr], test_output_edges[grouped-bf16x6-tr], test_problem_table[nodb-grouped-*]
1406  gemm_wgrad_grouped_kernel<3, false>   terms 6 and 19; N = 257 / one term turned            test_reduction_edges[grouped-bf16x6-dword], test_output_edges[grouped-bf16x6-dword], test_staging_predicate[flip_*-grouped-bf16x6-dword-*]
1449  gemm_wgrad_ragged_kernel<1, true>     terms 1; EVERY problem in quads, aligned, in span    test_reduction_edges[ragged-bf16-tr], test_output_edges[ragged-bf16-tr], test_problem_table[count64cyc-ragged-bf16-*]
1450  gemm_wgrad_ragged_kernel<1, false>    terms 1; ONE odd problem (first or last)             test_reduction_edges[ragged-bf16-dword], test_output_edges[ragged-bf16-dword], test_staging_predicate[flip_*-ragged-bf16-dword-*]
1453  gemm_wgrad_ragged_kernel<2, true>     terms 3; every problem eligible                      test_reduction_edges[ragged-bf16x3-tr], test_output_edges[ragged-bf16x3-tr], test_problem_table[*-ragged-bf16x3-tr-*], test_tr_span[span_under-ragged-*], test_host_queue[bf16x3]
1454  gemm_wgrad_ragged_kernel<2, false>    terms 3; one odd problem; either span clause         test_reduction_edges[ragged-bf16x3-dword], test_output_edges[ragged-bf16x3-dword], test_staging_predicate[flip_*-ragged-bf16x3-dword-*], test_problem_table[count64cyc_oddlast-*], test_tr_span[span_ld-ragged-*|span_bytes-ragged-*]
1457  gemm_wgrad_ragged_kernel<3, true>     terms 6 and 19; every problem eligible               test_reduction_edges[ragged-bf16x6-tr], test_output_edges[ragged-bf16x6-tr], test_problem_table[count64cyc-ragged-bf16x6-*|nodb-ragged-*], test_host_queue[bf16x6]
1458  gemm_wgrad_ragged_kernel<3, false>    terms 6 and 19; one odd problem                      test_reduction_edges[ragged-bf16x6-dword], test_output_edges[ragged-bf16x6-dword], test_staging_predicate[flip_*-ragged-bf16x6-dword-*]
====  ====================================  ==================================================  ================================================

What only these kernels execute, and where it is reached: the column-sum (bias-gradient) epilogue in its TR and dword
branch, over two tile rows (N = 260: a second tile row of 4 rows, 257: of one row) and written by tile column 0 only
(K = 132, 129: two tile columns); the accumulate store (bits at p = 0, 31, 32, 63, neighbours clear; together, and the low and the high pair apart); the problem look-up
(``lid / tiles`` and the bisection over tile_start, 64 problems of 1 / 2 / 4 tiles); xcd_remap over 1, 7, 8, 9, 65, 96 and 148
tiles; per-problem row strides.  Reduction edges M = 1 .. 129 give nk = 1 .. 5 k-tiles, each with a full and a partial last
one, in every cell (NS <= 2 under TR: the two-register-set pipeline whose prologue special-cases nk = 1, 2, 3).

Conventions (those of tests/test_rowops_forms_gpu.py).  Every dW_p is an [N, K] block and every db_p an [N] block of ONE
sentinel-filled arena, with >= 16 guard rows (>= 64 guard words for db) on both sides: every word outside the blocks must be
bit-unchanged afterwards, and the sentinel must not survive inside a block -- except in the db block of a problem without
a bias, which must keep it.  Accumulating problems start from known old contents.  dz_p and x_p are column blocks at a
non-zero column offset of wider buffers whose other columns and whose 32 rows after row M - 1 hold NaN: both stagers clamp
(or let the buffer range check answer zero) instead of multiplying by a mask, so correct code never consumes one.  The guards
exist so that an overrun lands inside the allocation and fails an assertion; no case is shaped to fault.  Every launch
runs twice and must be bit-identical (no atomics); terms 19 must be bit-identical to terms 6; every problem has its own
data, so a misrouted tile shows.

Bounds: wgrad_ref.py (dW: 5e-6 / 3e-5 (bf16x3) of max |ref| and per 32 x 32 block; db: derived; the 2^19-token launches:
derived).  No bound here was measured or tuned.
"""
import ctypes

import pytest
import torch

import wgrad_ref as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ABI = {"grouped": "e3d_gemm_wgrad_grouped_f32_split", "ragged": "e3d_gemm_wgrad_ragged_f32_split"}
BIG_FLOATS = (2 + W.TAIL) << 24      # the shared dz buffer of the e3d_tr_span_ok cases: 34 rows of 2^24 floats, 2.1 GiB


def bits(t):
    return t.contiguous().view(torch.int32)


def _place(flat, at, ld, block):
    flat.as_strided(tuple(block.shape), (ld, 1), at).copy_(block)


class Launch:
    """The memory of one case: inputs in one NaN-filled buffer, outputs in one sentinel-filled arena (wgrad_ref.in_layout /
    out_layout), and the argument record of its entry point."""

    def __init__(self, case, big=None):
        self.case, self.probs, M = case, case.seeded(), case.M
        zo, xo, n_in = W.in_layout(case)
        host = torch.full((n_in,), W.NAN)
        for p, z, x in zip(self.probs, zo, xo):
            dz, xx = W.operands(M, p)
            if not case.big:
                _place(host, z, p.ldz, dz)
            _place(host, x, p.ldx, xx)
        self.inp = host.to(DEV)
        base = self.inp.data_ptr()
        assert base % 64 == 0
        self.x_ptr = [base + 4 * o for o in xo]
        self.dz_ptr = [base + 4 * o for o in zo]
        if case.big:
            p, rows = self.probs[0], M + W.TAIL
            assert len(self.probs) == 1 and rows * p.ldz <= big.numel() and big.data_ptr() % 64 == 0
            big.fill_(W.NAN)
            big[:rows * p.ldz].view(rows, p.ldz)[:M, zo[0]:zo[0] + p.N] = W.operands(M, p)[0].to(DEV)
            self.dz_ptr = [big.data_ptr() + 4 * zo[0]]
        self.wo, self.bo, n_out = W.out_layout(case)
        arena, inside = torch.full((n_out,), W.SENTINEL), torch.zeros(n_out, dtype=torch.bool)
        for p, w, b in zip(self.probs, self.wo, self.bo):
            live_b = p.bias and not case.db_null
            inside[w:w + p.N * p.K] = True
            inside[b:b + p.N] = live_b
            if p.acc:
                ow, ob = W.old_contents(M, p)
                arena[w:w + p.N * p.K] = ow.reshape(-1)
                if live_b:
                    arena[b:b + p.N] = ob
        self.arena0, self.inside = arena.to(DEV), inside.to(DEV)

    def staging(self):
        """TR or not, by the restated predicate on the REAL pointers."""
        ps, M = self.probs, self.case.M
        if self.case.entry == "grouped":
            return W.grouped_tr(M, ps[0].N, ps[0].K, ps[0].ldz, ps[0].ldx, self.dz_ptr, self.x_ptr)
        return W.ragged_tr(M, [p.N for p in ps], [p.K for p in ps], [p.ldz for p in ps], [p.ldx for p in ps], self.dz_ptr, self.x_ptr)

    def args(self, arena, terms=None):
        base, c = arena.data_ptr(), self.case
        db = None if c.db_null else [base + 4 * o if p.bias else None for p, o in zip(self.probs, self.bo)]
        return dict(dz=list(self.dz_ptr), x=list(self.x_ptr), dw=[base + 4 * o for o in self.wo], db=db,
                    N=[p.N for p in self.probs], K=[p.K for p in self.probs], ldz=[p.ldz for p in self.probs],
                    ldx=[p.ldx for p in self.probs], bits=c.bits, count=len(self.probs), M=c.M, terms=terms or c.terms)


def invoke(pkg, entry, a):
    """The raw C-ABI call of an argument record (the lists may be longer or shorter than ``count``: the refusals)."""
    ptrs = lambda v: None if v is None else (ctypes.c_void_p * len(v))(*v)     # noqa: E731
    ints = lambda v, ty: (ty * len(v))(*v)                                     # noqa: E731
    lib, s = pkg.hip.lib(), torch.cuda.current_stream().cuda_stream
    if entry == "grouped":
        return lib.e3d_gemm_wgrad_grouped_f32_split(ptrs(a["dz"]), ptrs(a["x"]), ptrs(a["dw"]), ptrs(a["db"]), a["bits"], a["count"],
                                                    a["ldz"][0], a["ldx"][0], a["N"][0], a["K"][0], a["M"], a["terms"], s)
    return lib.e3d_gemm_wgrad_ragged_f32_split(ptrs(a["dz"]), ptrs(a["x"]), ptrs(a["dw"]), ptrs(a["db"]), ints(a["N"], ctypes.c_int),
                                               ints(a["K"], ctypes.c_int), ints(a["ldz"], ctypes.c_int64), ints(a["ldx"], ctypes.c_int64),
                                               a["bits"], a["count"], a["M"], a["terms"], s)


def launch(pkg, L, terms=None):
    """One launch into a fresh copy of the arena; returns the arena."""
    arena = L.arena0.clone()
    pkg.hip.check(invoke(pkg, L.case.entry, L.args(arena, terms)), ABI[L.case.entry])
    torch.cuda.synchronize()
    return arena


def verify(L, arena, terms=None):
    """Guards, sentinels and every problem's dW / db against fp64; returns [(dW, db or None)] on the host."""
    c, what = L.case, L.case.id
    terms = terms or c.terms
    same = bits(arena) == bits(L.arena0)
    assert bool(same[~L.inside].all()), f"{what}: a write outside the output blocks (or into the db block of a problem without a bias)"
    host, outs = arena.cpu(), []
    for i, (p, w, b) in enumerate(zip(L.probs, L.wo, L.bo)):
        dz, x = W.operands(c.M, p)
        old = W.old_contents(c.M, p) if p.acc else (None, None)
        live_b = p.bias and not c.db_null
        ref_w, ref_b = W.reference(c.M, p, terms)
        got_w = host[w:w + p.N * p.K].view(p.N, p.K)
        assert not bool((got_w == W.SENTINEL).any()), f"{what}: problem {i}: the sentinel survives in dW"
        if c.M >= (1 << 19) - 1:
            W.check_within(got_w, ref_w, W.long_reduction_bound(c.M, dz, x, ref_w, terms), f"{what}: problem {i} dW")
        else:
            W.check_close(got_w, ref_w, W.TOL[terms], f"{what}: problem {i} {p} dW")
        got_b = None
        if live_b:
            got_b = host[b:b + p.N]
            assert not bool((got_b == W.SENTINEL).any()), f"{what}: problem {i}: the sentinel survives in db"
            W.check_within(got_b, ref_b, W.db_bound(c.M, dz, old[1]), f"{what}: problem {i} {p} db")
        outs.append((got_w, got_b))
    return outs


def forms_case(pkg, case, big=None):
    L = Launch(case, big)
    assert L.staging() == case.tr, f"{case.id}: the operands do not select the staging the case claims"
    first = launch(pkg, L)
    outs = verify(L, first)
    assert torch.equal(bits(first), bits(launch(pkg, L))), f"{case.id}: a repeated launch differs"
    if case.terms == 6:
        assert torch.equal(bits(first), bits(launch(pkg, L, 19))), f"{case.id}: terms 19 differs from terms 6"
    return outs


CELL_IDS = [W.cell_id(*c) for c in W.CELLS]


@pytest.mark.parametrize("entry,terms,tr", W.CELLS, ids=CELL_IDS)
def test_reduction_edges(pkg, hip, entry, terms, tr):
    """M = 1, 31, 32, 33, 64, 65, 96, 97, 128, 129: nk = 1 .. 5, each with a full and a partial last k-tile."""
    for case in W.reduction_cases(entry, terms, tr):
        forms_case(pkg, case)


@pytest.mark.parametrize("entry,terms,tr", W.CELLS, ids=CELL_IDS)
def test_output_edges(pkg, hip, entry, terms, tr):
    """N in {4, 252, 256, 260} x K in {4, 124, 128, 132} (dword: also N = 1, 255, 257 and K = 1, 127, 129) around the 256 x 128 tile."""
    for case in W.edge_cases(entry, terms, tr):
        forms_case(pkg, case)


_BASE = {}
FLIPS = W.flip_cases()


@pytest.mark.parametrize("case", FLIPS, ids=[c.id for c in FLIPS])
def test_staging_predicate(pkg, hip, case):
    """One term of the launcher's predicate turned at a time from a TR-eligible launch (in the ragged launch on a single
    problem, first or last): the dword staging's result meets the bounds, and where the turned launch multiplies the same
    data (a stride or a pointer turned) it agrees with the transposing staging's within the arithmetic's bound."""
    key = (case.entry, case.terms)
    if key not in _BASE:
        _BASE[key] = forms_case(pkg, W.flip_base(*key))
    outs = forms_case(pkg, case)
    if case.flip[0] in W.SAME_DATA_FLIPS:
        for i, ((gw, gb), (bw, bb)) in enumerate(zip(outs, _BASE[key])):
            d = float((gw.double() - bw.double()).abs().max()) / float(bw.abs().max())
            assert d <= W.TOL[case.terms], (case.id, i, d)
            dz = W.operands(case.M, case.seeded()[i])[0]
            assert bool(((gb.double() - bb.double()).abs() <= 2 * W.db_bound(case.M, dz)).all()), (case.id, i)


@pytest.fixture(scope="module")
def big_buffer(hip):
    buf = torch.empty(BIG_FLOATS, device=DEV)
    yield buf
    del buf
    torch.cuda.empty_cache()


SPANS = W.span_cases()


@pytest.mark.parametrize("case", SPANS, ids=[c.id for c in SPANS])
def test_tr_span(pkg, hip, big_buffer, case):
    """Both clauses of e3d_tr_span_ok on a dz inside one NaN-filled 2 GiB buffer (only its 8 live columns come from the
    host): a row stride of 2^24 floats, and 2^31 - 4096 bytes (TR) against 2^31 bytes (dword) of reduction rows."""
    forms_case(pkg, case, big_buffer)


TABLE = W.table_cases()


@pytest.mark.parametrize("case", TABLE, ids=[c.id for c in TABLE])
def test_problem_table(pkg, hip, case):
    forms_case(pkg, case)


@pytest.mark.parametrize("kind", W.REFUSALS)
@pytest.mark.parametrize("entry", W.ENTRIES)
def test_refusals(pkg, hip, entry, kind):
    """Refused before anything is launched: an error code, a message through hip.check, the arena bit-unchanged -- and the
    same launch with the argument put right still runs."""
    case = W.flip_base(entry, 3)
    L = Launch(case)
    arena = L.arena0.clone()
    a = L.args(arena)
    if kind == "count0":
        a["count"] = 0
    elif kind == "count65":
        a["count"] = 65
        for k in ("dz", "x", "dw", "db", "N", "K", "ldz", "ldx"):
            a[k] = (a[k] * 22)[:65]
    elif kind == "terms2":
        a["terms"] = 2
    elif kind == "ldz_below_N":
        a["ldz"] = [a["N"][0] - 4] * 3 if entry == "grouped" else [a["ldz"][0], a["N"][1] - 4, a["ldz"][2]]
    elif kind == "ldx_below_K":
        a["ldx"] = [a["K"][0] - 4] * 3 if entry == "grouped" else [a["ldx"][0], a["ldx"][1], a["K"][2] - 4]
    elif kind.startswith("null_"):
        a[kind[5:]][1] = None
    else:
        assert kind == "M0"
        a["M"] = 0
    rc = invoke(pkg, entry, a)
    assert rc != 0
    with pytest.raises(RuntimeError, match=r"\): gemm_wgrad_" + entry + ":"):
        pkg.hip.check(rc, ABI[entry])
    torch.cuda.synchronize()
    assert torch.equal(bits(arena), bits(L.arena0)), f"{entry} {kind}: a refused launch wrote"
    verify(L, launch(pkg, L))


# ----------------------------------------------------------------------------------------------------- the host queue
def _layers():
    """(N, K, token-count index, bias?) of 72 tiny Linears: 67 of the first token count (more than one launch of 64), 5 of the
    second; mostly one 256 x 128 tile, ten of two tile rows (76 tiles in the larger group: under the default MIN_TILES = 96)."""
    out = []
    for i in range(67):
        out.append((384 if i % 7 == 3 else (128, 256)[i % 2], (32, 64, 96, 128)[i % 4], 0, i % 5 != 2))
    for i in range(5):
        out.append(((128, 256, 384)[i % 3], (64, 32, 128)[i % 3], 1, i != 1))
    return out


TOKENS = (40, 72)
TWICE, MIXED = 11, 20       # layer used twice in the forward pass; layer whose weight already holds a gradient, its bias none


@pytest.mark.parametrize("mode", ["bf16x3", "bf16x6"])
def test_host_queue(pkg, hip, monkeypatch, mode):
    """autograd.deferred_weight_grads over 72 tiny Linears of mixed shapes with MIN_TILES = 1: two token counts, more than 64
    layers of one of them (two ragged launches in one flush), a weight used twice (second round, accumulate bit), a layer
    whose weight holds a gradient while its bias has none (per-layer path), layers without a bias -- every gradient against
    fp64 autograd; and the same loss with the default MIN_TILES, where every layer goes the per-layer way."""
    from e3diff_amd.autograd import deferred_weight_grads, functional
    layers, terms = _layers(), pkg.ops.GEMM_MODES[mode]
    assert sum(-(-n // 256) * -(-k // 128) for n, k, t, _ in layers if t == 0) + 2 < deferred_weight_grads.MIN_TILES
    ws = [torch.randn(n, k, generator=W.gen(i, 1)) / k ** 0.5 for i, (n, k, _, _) in enumerate(layers)]
    bs = [torch.randn(n, generator=W.gen(i, 2)) if hb else None for i, (n, _, _, hb) in enumerate(layers)]
    uses = [(i, 0) for i in range(len(layers))] + [(TWICE, 1)]
    xs = {(i, u): torch.randn(TOKENS[layers[i][2]], layers[i][1], generator=W.gen(i, u, 3)) for i, u in uses}
    gos = {(i, u): torch.randn(TOKENS[layers[i][2]], layers[i][0], generator=W.gen(i, u, 4)) for i, u in uses}
    preset = torch.randn(ws[MIXED].shape, generator=W.gen(5))
    assert bs[MIXED] is not None and bs[TWICE] is not None and layers[TWICE][2] == 0

    rw = [w.double().requires_grad_(True) for w in ws]
    rb = [None if b is None else b.double().requires_grad_(True) for b in bs]
    sum((torch.nn.functional.linear(xs[k].double(), rw[k[0]], rb[k[0]]) * gos[k].double()).sum() for k in uses).backward()
    rw[MIXED].grad += preset.double()

    lib = pkg.hip.lib()
    real, calls = lib.e3d_gemm_wgrad_ragged_f32_split, []

    def spy(*a):
        calls.append((a[9], a[8], a[10], a[11]))      # (count, accumulate bits, M, terms)
        return real(*a)
    monkeypatch.setattr(lib, "e3d_gemm_wgrad_ragged_f32_split", spy, raising=False)
    xd, gd = {k: v.to(DEV) for k, v in xs.items()}, {k: v.to(DEV) for k, v in gos.items()}

    def device_gradients():
        dw = [w.to(DEV).requires_grad_(True) for w in ws]
        db = [None if b is None else b.to(DEV).requires_grad_(True) for b in bs]
        dw[MIXED].grad = preset.to(DEV)
        with pkg.ops.arithmetic(mode, respect_env=False), deferred_weight_grads() as q:
            sum((functional.linear(xd[k], dw[k[0]], db[k[0]]) * gd[k]).sum() for k in uses).backward()
            assert q.queued_total == len(uses)
        torch.cuda.synchronize()
        return dw, db

    def check(dw, db, what):
        for i, (n, k, t, hb) in enumerate(layers):
            mine = [u for u in uses if u[0] == i]
            W.check_close(dw[i].grad.cpu(), rw[i].grad, W.TOL[terms], f"{what}: layer {i} {layers[i]} dW")
            if hb:
                s = sum(gos[u].double().abs().sum(0) for u in mine)
                bound = (TOKENS[t] * len(mine) + 8 * len(mine)) * 2.0 ** -24 * s      # one fp32 summation of every use's rows
                W.check_within(db[i].grad.cpu(), rb[i].grad, bound, f"{what}: layer {i} {layers[i]} db")

    monkeypatch.setattr(deferred_weight_grads, "MIN_TILES", 1)
    calls.clear()
    check(*device_gradients(), "grouped")
    # first token count: 66 layers (one took the per-layer path) in launches of 64 and 2, then the second use alone with its
    # accumulate bit; second token count: 5 layers
    assert sorted(calls) == sorted([(64, 0, 40, terms), (2, 0, 40, terms), (1, 1, 40, terms), (5, 0, 72, terms)]), calls
    monkeypatch.undo()
    monkeypatch.setattr(lib, "e3d_gemm_wgrad_ragged_f32_split", spy, raising=False)
    calls.clear()
    check(*device_gradients(), "per layer")
    assert calls == [], calls
