"""GPU: every launch site of csrc/optim.hip against the fp64 statement of tests/optim_ref.py -- e3d_grad_global_norm and
the five update entry points e3d_adamw_step / _step_dyn / _step_dev / _ema_step / _ema_step_dev, called through the C ABI
with pointer tables, chunk tables and hyper blocks built here (ClipAdamW's host logic is not in the picture).

Layout.  Every role (p, g, m, v, shadow) is one flat device buffer; a tensor is a slice of it at a 16-byte aligned
address, or 4 bytes past one for the misaligned views, with at least GAP floats of sentinel on both sides: a fixed bit
pattern around p, m, v and the shadow (bit-unchanged afterwards), NaN around every gradient (a read past numel poisons the
norm).  The zoo and the views are optim_ref.tensors().

Norm.  Within 2e-6 relative of the float64 norm.  Why the kernel's summation tree fits (optim_ref.norm_tolerance_note): a
thread adds at most 32 squares with fmaf, then s0 + s1, six butterfly levels and three adds of wave sums, all terms
positive: 42 u on a partial; double from there; the square root halves it and the fp32 rounding of the norm adds one:
22 u = 1.3e-6.  The coefficient is held to 3 u of the float64 expression of the device's own norm (fl(norm + 1e-6f), the
constant, the division) and is exactly 1.0f at and above the boundary.

Update.  p, m and v of every element within the bounds of optim_ref.update started from the pre-step fp32 state; shadows
within ema_ref's 4 u M of the statement fed the device's own new parameter; the EMA forms bit-equal to the plain forms in
p, m, v; a second run bit-identical.  Host- and device-scalar forms are each held to the bound and not to each other
(host and device pow may differ in the last place); whether they are bit-equal is printed.

Every test prints its worst fraction of the bound (``pytest -s``); DESIGN.md records them."""
import math

import numpy as np
import pytest
import torch

import optim_ref as R
from ema_ref import Statement, decay_fp32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP = 8                                    # floats of sentinel between two slices, at least
SENTINEL = np.float32(-12345.678)
PLAIN = ("e3d_adamw_step", "e3d_adamw_step_dyn", "e3d_adamw_step_dev")
EMA = ("e3d_adamw_ema_step", "e3d_adamw_ema_step_dev")
ENTRIES = PLAIN + EMA


class Layout:
    """Flat sentinel-padded buffers of the five roles for tensors [(numel, misaligned roles)], with their pointer, numel
    and chunk tables on the device.  ``data``: dict role -> list of fp32 numpy arrays."""

    def __init__(self, tensors, data):
        self.numels = [n for n, _ in tensors]
        self.off = {k: [] for k in "pgmve"}
        size = {}
        for k in "pgmve":
            pos = 4 * GAP
            for n, mis in tensors:
                start = pos + (1 if k in mis else 0)
                self.off[k].append(start)
                pos = (start + n + GAP + 3) // 4 * 4
            size[k] = pos + 4 * GAP
        self.host, self.mask = {}, {}
        for k in "pgmve":
            buf = np.full(size[k], np.nan if k == "g" else SENTINEL, dtype=np.float32)
            mask = np.ones(size[k], dtype=bool)                      # True: sentinel
            for o, n, a in zip(self.off[k], self.numels, data[k]):
                assert a.dtype == np.float32 and a.shape == (n,)
                buf[o:o + n] = a
                mask[o:o + n] = False
            self.host[k], self.mask[k] = buf, mask
        self.dev = {k: torch.from_numpy(self.host[k]).to(DEV) for k in "pgmve"}
        self.ptr = {}
        for k in "pgmve":
            base = self.dev[k].data_ptr()
            assert base % 16 == 0
            addr = [base + 4 * o for o in self.off[k]]
            for a, (n, mis), o in zip(addr, tensors, self.off[k]):
                assert a % 16 == (4 if o % 4 else 0)
                assert 4 * GAP <= o and o + n + GAP <= size[k]       # inside the buffer, sentinels on both sides
            self.ptr[k] = torch.tensor(addr, dtype=torch.int64).to(DEV)
        self.numel = torch.tensor(self.numels, dtype=torch.int64).to(DEV)
        ct, cf, self.first_chunk = [], [], []
        for i, n in enumerate(self.numels):
            self.first_chunk.append(len(ct))
            for f in range(0, n, R.CHUNK):
                ct.append(i)
                cf.append(f)
        self.first_chunk.append(len(ct))
        self.n_chunks = len(ct)
        self.chunk_tensor = torch.tensor(ct, dtype=torch.int32).to(DEV)
        self.chunk_first = torch.tensor(cf, dtype=torch.int64).to(DEV)
        self.partial = torch.full((self.n_chunks + 2 * GAP,), float(SENTINEL), dtype=torch.float32, device=DEV)
        self.nc = torch.full((2 + 2 * GAP,), float(SENTINEL), dtype=torch.float32, device=DEV)

    def reset(self):
        for k in "pmve":
            self.dev[k].copy_(torch.from_numpy(self.host[k]))

    def read(self, k):
        """(list of the role's tensors as fp32 CPU tensors, True when every sentinel of the buffer is bit-unchanged)."""
        got = self.dev[k].cpu().numpy()
        same = np.array_equal(got.view(np.int32)[self.mask[k]], self.host[k].view(np.int32)[self.mask[k]])
        return [torch.from_numpy(got[o:o + n].copy()) for o, n in zip(self.off[k], self.numels)], same

    def norm(self, lib, max_norm):
        """Runs the two norm launches; returns (norm, coef) as fp32-valued Python floats.  The partials and the result sit
        between sentinels of their own."""
        stream = torch.cuda.current_stream().cuda_stream
        rc = lib.e3d_grad_global_norm(self.ptr["g"].data_ptr(), self.numel.data_ptr(), self.chunk_tensor.data_ptr(),
                                      self.chunk_first.data_ptr(), self.n_chunks, float(max_norm),
                                      self.partial.data_ptr() + 4 * GAP, self.nc.data_ptr() + 4 * GAP, stream)
        assert rc == 0
        nc, part = self.nc.cpu(), self.partial.cpu()
        for t, n in ((nc, 2), (part, self.n_chunks)):
            edge = torch.cat([t[:GAP], t[GAP + n:]])
            assert bool((edge == float(SENTINEL)).all())
        return float(nc[GAP]), float(nc[GAP + 1])

    def clip_ptr(self):
        return self.nc.data_ptr() + 4 * GAP


def _hyper_block(hyper, t, ema=None):
    """The 8-float device block of one range: lr, steps taken, b1, b2, eps, wd, EMA decay (sign bit: no warm-up), EMA
    updates made."""
    lr, b1, b2, eps, wd = hyper
    enc, n = 0.0, 0.0
    if ema is not None:
        decay, warmup, n = ema
        enc = math.copysign(float(decay), 1.0 if warmup else -1.0)
    return [lr, float(t - 1), b1, b2, eps, wd, enc, float(n)]


def _launch(lib, entry, L, hyper, t, clip, c0=0, c1=None, ema=None, dyn_ptr=None, keep=None):
    """One update launch over chunks [c0, c1).  ``clip``: pointer or None.  ``dyn_ptr``: a hyper block already on the device
    (chunk-range test); otherwise one is built.  ``keep``: a list that keeps the block alive."""
    c1 = L.n_chunks if c1 is None else c1
    assert 0 <= c0 < c1 <= L.n_chunks
    stream = torch.cuda.current_stream().cuda_stream
    lr, b1, b2, eps, wd = hyper
    tabs = [L.ptr["p"].data_ptr(), L.ptr["g"].data_ptr(), L.ptr["m"].data_ptr(), L.ptr["v"].data_ptr()]
    if entry in EMA:
        tabs.append(L.ptr["e"].data_ptr())
    tabs += [L.numel.data_ptr(), L.chunk_tensor.data_ptr() + 4 * c0, L.chunk_first.data_ptr() + 8 * c0, c1 - c0, clip]
    if entry in ("e3d_adamw_step_dyn", "e3d_adamw_step_dev", "e3d_adamw_ema_step_dev") and dyn_ptr is None:
        block = torch.tensor(_hyper_block(hyper, t, ema), dtype=torch.float32).to(DEV)
        if keep is not None:
            keep.append(block)
        dyn_ptr = block.data_ptr()
    if entry == "e3d_adamw_step":
        rc = lib.e3d_adamw_step(*tabs, lr, b1, b2, eps, wd, int(t), stream)
    elif entry == "e3d_adamw_step_dyn":
        rc = lib.e3d_adamw_step_dyn(*tabs, dyn_ptr, b1, b2, eps, wd, stream)
    elif entry == "e3d_adamw_step_dev":
        rc = lib.e3d_adamw_step_dev(*tabs, dyn_ptr, stream)
    elif entry == "e3d_adamw_ema_step":
        decay, warmup, n = ema
        rc = lib.e3d_adamw_ema_step(*tabs, lr, b1, b2, eps, wd, int(t), decay_fp32(n + 1, decay, warmup), stream)
    else:
        rc = lib.e3d_adamw_ema_step_dev(*tabs, dyn_ptr, stream)
    torch.cuda.synchronize()
    assert rc == 0, entry


def _check(L, x, hyper, t, coef, entry, ema, which=None, ref_cache=None):
    """Reads p, m, v (and the shadow) back and holds tensors ``which`` (all by default) to the statement.  Returns
    (worst p, m, v, shadow fractions, the tensors read)."""
    got = {}
    for k in "pmve":
        got[k], same = L.read(k)
        assert same, f"{entry}: a sentinel of the {k} buffer changed"
    worst = [0.0, 0.0, 0.0, 0.0]
    for i in (range(len(L.numels)) if which is None else which):
        key = (i, t, coef, hyper)
        ref = ref_cache.get(key) if ref_cache is not None else None
        if ref is None:
            ref = R.update(x["p"][i], x["g"][i], x["m"][i], x["v"][i], hyper, t, coef)
            if ref_cache is not None:
                ref_cache[key] = ref
        fr = list(R.fractions(got["p"][i], got["m"][i], got["v"][i], ref))
        e0 = torch.from_numpy(x["e"][i])
        if entry in EMA:
            decay, warmup, n = ema
            st = Statement(e0)
            st.update(got["p"][i], decay_fp32(n + 1, decay, warmup))
            fr.append(st.fraction(got["e"][i]))
        else:
            assert torch.equal(got["e"][i], e0)
            fr.append(0.0)
        assert max(fr) <= 1.0, (entry, i, L.numels[i], fr)
        worst = [max(a, b) for a, b in zip(worst, fr)]
    return worst, got


def _bit_diff(a, b):
    """[(tensor index, number of elements that differ in bits, the first of them)] of two lists of tensors."""
    out = []
    for i, (x, y) in enumerate(zip(a, b)):
        ne = (x.view(torch.int32) != y.view(torch.int32)).nonzero().reshape(-1)
        if ne.numel():
            out.append((i, int(ne.numel()), int(ne[0])))
    return out


def _same_bits(a, b):
    return not _bit_diff(a, b)


@pytest.fixture(scope="module")
def lib(pkg, hip):
    assert hip.e3d_optim_chunk_elems() == R.CHUNK
    return hip


# ---------------------------------------------------------------------------------------------------- the update
@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_every_update_entry_point_against_the_statement(lib, case):
    """One row of the shared case table through all five update entry points over the zoo and the misaligned views."""
    tensors = R.tensors()
    x = R.case_inputs(case)
    L = Layout(tensors, x)
    hyper, t, ema = R.case_hyper(case), case["t"], case["ema"]
    coef, clip = 1.0, None
    if case["clip"] is not None:
        norm32, coef = L.norm(lib, case["clip"])
        norm, _ = R.clip(x["g"], case["clip"])
        assert abs(norm32 - norm) <= R.NORM_RTOL * norm
        assert (coef < 1.0) == (case["gscale"] > 1.0)
        clip = L.clip_ptr()
    keep, cache, results = [], {}, {}
    for entry in ENTRIES:
        L.reset()
        _launch(lib, entry, L, hyper, t, clip, ema=ema, keep=keep)
        worst, got = _check(L, x, hyper, t, coef, entry, ema, ref_cache=cache)
        assert not any(torch.equal(got["p"][i], torch.from_numpy(x["p"][i])) for i in range(len(tensors)))
        L.reset()
        _launch(lib, entry, L, hyper, t, clip, ema=ema, keep=keep)
        for k in "pmve":
            assert _same_bits(L.read(k)[0], got[k]), (entry, k, "second run differs")
        results[entry] = got
        print(f"{case['name']} {entry}: worst fraction p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f} shadow {worst[3]:.3f}")
    for plain, fused in (("e3d_adamw_step", "e3d_adamw_ema_step"), ("e3d_adamw_step_dev", "e3d_adamw_ema_step_dev")):
        for k in "pmv":
            assert _same_bits(results[plain][k], results[fused][k]), (fused, k, _bit_diff(results[plain][k], results[fused][k]))
    for k in "pmv":
        assert _same_bits(results["e3d_adamw_step_dyn"][k], results["e3d_adamw_step_dev"][k]), k      # the same device arithmetic
    host_dev = all(_same_bits(results["e3d_adamw_step"][k], results["e3d_adamw_step_dev"][k]) for k in "pmv")
    print(f"{case['name']}: host- and device-scalar forms bit-equal: {host_dev}")


def test_device_ema_decay_with_and_without_the_sign_bit(lib):
    """e3d_adamw_ema_step_dev forms d_n from words 6 and 7 of the block: decay_fp32(word 7 + 1), with warm-up (positive
    word 6) and without (sign bit set, -0.0f for decay 0), at counts on both sides of the warm-up's crossing of the decay.
    The shadow is held to the statement with that d_n; two laws that give the same d_n give the same bits."""
    case = R.CASES[1]
    sizes = [(5, ()), (R.CHUNK + 1, ()), (1021, ("e",))]
    x = R.case_inputs(case, [n for n, _ in sizes])
    L = Layout(sizes, x)
    hyper, t = R.case_hyper(case), case["t"]
    shadows, worst = {}, 0.0
    for ema in ((0.9, True, 0), (0.9, True, 78), (0.9, True, 79), (0.9, True, 5000), (0.9, False, 0), (0.9, False, 5000),
                (0.0, False, 3), (0.0, True, 3), (0.9999, True, 2 ** 20)):
        L.reset()
        _launch(lib, "e3d_adamw_ema_step_dev", L, hyper, t, None, ema=ema)
        w, got = _check(L, x, hyper, t, 1.0, "e3d_adamw_ema_step_dev", ema)
        worst = max(worst, w[3])
        shadows[ema] = got["e"]
    assert decay_fp32(79, 0.9, True) < decay_fp32(80, 0.9, True) == decay_fp32(1, 0.9, False)
    assert _same_bits(shadows[(0.9, True, 5000)], shadows[(0.9, False, 0)])
    assert _same_bits(shadows[(0.9, True, 79)], shadows[(0.9, False, 5000)])
    assert _same_bits(shadows[(0.0, False, 3)], shadows[(0.0, True, 3)])
    assert not _same_bits(shadows[(0.9, True, 0)], shadows[(0.9, False, 0)])
    assert not _same_bits(shadows[(0.9, True, 78)], shadows[(0.9, True, 79)])
    print(f"device d_n: worst shadow fraction {worst:.3f}")


def test_chunk_ranges_move_by_their_own_scalars(lib):
    """chunk_tensor + c0, chunk_first + c0, n_chunks = c1 - c0, as ClipAdamW.step passes them: two ranges with different
    scalars (for the device forms: hyper blocks at dyn + 8 r of one table), tensors before, between and after the ranges.
    Each range moves by its own scalars; every tensor outside is bit-unchanged, in all five roles."""
    case = R.CASES[5]
    sizes = [(1021, ()), (R.CHUNK + 1, ()), (5, ("p",)), (3, ()), (3 * R.CHUNK + 5, ()), (R.CHUNK, ("g",)), (4, ())]
    x = R.case_inputs(case, [n for n, _ in sizes])
    L = Layout(sizes, x)
    ranges = [((1, 2), R.hyper32(1e-2, 0.9, 0.999, 1e-8, 0.1), 2, (0.9, True, 1)),
              ((4, 5), R.hyper32(3e-3, 0.85, 0.95, 1e-3, 0.0), 1000, (0.9, True, 1))]
    outside = [0, 3, 6]
    dyn = torch.tensor([_hyper_block(h, t, e) for _, h, t, e in ranges], dtype=torch.float32).to(DEV)
    assert dyn.shape == (2, 8)
    norm32, coef = L.norm(lib, 1.0)
    assert coef < 1.0
    for entry in ENTRIES:
        L.reset()
        for r, (ts, hyper, t, ema) in enumerate(ranges):
            c0, c1 = L.first_chunk[ts[0]], L.first_chunk[ts[-1] + 1]
            _launch(lib, entry, L, hyper, t, L.clip_ptr(), c0, c1, ema=ema, dyn_ptr=dyn.data_ptr() + 4 * 8 * r)
        worst = [0.0] * 4
        for ts, hyper, t, ema in ranges:
            w, got = _check(L, x, hyper, t, coef, entry, ema, which=ts)
            worst = [max(a, b) for a, b in zip(worst, w)]
        for i in outside:
            for k in "pmve":
                assert torch.equal(got[k][i].view(torch.int32), torch.from_numpy(x[k][i]).view(torch.int32)), (entry, i, k)
        print(f"ranges {entry}: worst fraction p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f} shadow {worst[3]:.3f}")


# ---------------------------------------------------------------------------------------------------- the norm
def _norm_case(lib, tensors, gscale, seed):
    numels = [n for n, _ in tensors]
    x = R.gen_inputs(numels, seed, gscale, "zero")
    L = Layout(tensors, x)
    return L, x


@pytest.mark.parametrize("gscale", [50.0, 1e-3])
@pytest.mark.parametrize("table", ["zoo", "300-partials"])
def test_norm_and_coefficient_against_float64(lib, table, gscale):
    """The two norm launches on the zoo with its views, and on 300 one-chunk tensors of numel 1..300 (300 partials: the
    final kernel's stride loop takes a second trip): norm within 2e-6 of float64, coefficient within 3 u of the float64
    expression of the device's norm, clip active (scale 50) and inactive (1e-3); the boundary: max_norm chosen from the
    device norm so that max_norm / (norm + 1e-6f) is exactly 1, one ulp below and one ulp above; a second run is
    bit-identical (no atomics)."""
    tensors = R.tensors() if table == "zoo" else [(n, ()) for n in range(1, 301)]
    L, x = _norm_case(lib, tensors, gscale, 7)
    assert table == "zoo" or L.n_chunks == 300
    norm, coef = R.clip(x["g"], 1.0)
    norm32, coef32 = L.norm(lib, 1.0)
    err_u = abs(norm32 - norm) / norm / R.U
    print(f"norm {table} scale {gscale}: {err_u:.2f} u from float64 ({L.n_chunks} partials)")
    assert abs(norm32 - norm) <= R.NORM_RTOL * norm
    want = R.coef_from_norm(norm32, 1.0)
    assert (coef32 == 1.0) if want == 1.0 else (abs(coef32 - want) <= R.COEF_RTOL * want and coef32 < 1.0)
    assert (coef32 < 1.0) == (gscale > 1.0)
    assert L.norm(lib, 1.0) == (norm32, coef32)
    # the boundary r == 1: d = fl(norm + 1e-6f) is what the kernel divides by
    d = np.float32(norm32) + np.float32(1e-6)
    for max_norm, exact_one in ((d, True), (np.nextafter(d, np.float32(np.inf)), True), (np.nextafter(d, np.float32(0)), False)):
        n2, c2 = L.norm(lib, float(max_norm))
        assert n2 == norm32
        if exact_one:
            assert c2 == 1.0
        else:
            want = R.coef_from_norm(norm32, float(max_norm))
            assert c2 < 1.0 and abs(c2 - want) <= R.COEF_RTOL * want


@pytest.mark.parametrize("bad", ["nan", "inf", "-inf"])
def test_non_finite_gradients_as_clip_grad_norm(lib, bad):
    """One non-finite gradient element, as tests/test_optim_ref_cpu.py has it for torch.  NaN: norm and coefficient NaN and
    every element of p, m, v NaN after an update.  inf: norm inf, coefficient 0, NaN at that element only, g' = 0 and the
    result within bound everywhere else.  Host- and device-scalar forms; sentinels and shadows unchanged."""
    case = R.CASES[3]
    tensors = [(5, ()), (1021, ()), (R.CHUNK + 1, ("g",)), (2 * R.CHUNK, ())]
    x = R.case_inputs(case, [n for n, _ in tensors])
    x["g"][1][77] = float(bad)
    L = Layout(tensors, x)
    hyper, t = R.case_hyper(case), case["t"]
    norm, coef = R.clip(x["g"], 1.0)
    norm32, coef32 = L.norm(lib, 1.0)
    if bad == "nan":
        assert math.isnan(norm) and math.isnan(coef) and math.isnan(norm32) and math.isnan(coef32)
    else:
        assert norm == math.inf and coef == 0.0 and norm32 == math.inf and coef32 == 0.0
    for entry in PLAIN:
        L.reset()
        _launch(lib, entry, L, hyper, t, L.clip_ptr())
        worst, got = _check(L, x, hyper, t, coef, entry, None)      # (NaN where the statement is NaN, and only there)
        for i in range(len(tensors)):
            for k in "pmv":
                n_bad = int((~torch.isfinite(got[k][i])).sum())
                assert n_bad == int(torch.isnan(got[k][i]).sum())
                assert n_bad == (got[k][i].numel() if bad == "nan" else (1 if i == 1 else 0)), (entry, i, k, n_bad)
        if bad != "nan":
            assert bool(torch.isnan(got["p"][1][77]))
        print(f"{bad} {entry}: worst fraction on the finite elements p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")
