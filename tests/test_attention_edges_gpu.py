"""GPU: the attention kernels against fp64 at the edges of their tiling, gradients asserted part by part.

The reference everywhere is the fp64 torch statement of the existing attention tests -- (scores + rel-key term) / 8,
+ (1 - mask) * -10000, softmax, @ v -- differentiated by torch autograd in fp64.  Inputs are randn, not scaled up.
Tolerances are the project's existing ones: forward f32 1e-5, bf16x6 1e-5, bf16x3 1e-4, f16x3 1e-5 (test_attention_self);
backward bf16x6 2e-5, bf16x3 1e-4, f32 2e-5 (test_self_attention_backward,
test_attention_probability_dropout_forward_and_backward).

Mode and shape pick the kernel form through the public API (no selector is used here):

| Direction | Mode              | Condition              | Kernel                                                              |
|-----------|-------------------|------------------------|---------------------------------------------------------------------|
| Forward   | f32               | any                    | exact kernel of attn_relkey.hip                                     |
| Forward   | bf16x6            | any                    | per-wave split kernel (attn_relkey_split.hip), 4- and 8-tile frames too |
| Forward   | bf16x3 / f16x3    | ceil(Lq/32) % 4 == 0   | cooperative kernel (attn_relkey_coop.hip)                           |
| Forward   | bf16x3 / f16x3    | otherwise              | per-wave split kernel                                               |
| Backward  | f32 / bf16x6      | any                    | fp32-MFMA two-launch kernels (attn_bwd.hip)                         |
| Backward  | bf16x3            | Lq, Lk <= 128          | fused kernel (attn_bwd_coop.hip)                                    |
| Backward  | bf16x3            | otherwise              | two-launch split kernels (attn_bwd_split.hip)                       |

Three mask kinds: ``prefix`` (lengths chosen by hand per case: always the full length and a very short item -- one key
in forward cases, two in backward cases, because an item with one valid key has dq = dk = 0 exactly, which has a test of
its own), ``holes`` (``holes_mask``) and ``none``.  Every item of every case has at least one valid key.
"""
import pytest
import torch

from helpers import rel_err
from oracle import bert as obert

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NH = 2
H = NH * 64

FWD_MODES = (("f32", 1e-5), ("bf16x6", 1e-5), ("bf16x3", 1e-4), ("f16x3", 1e-5))
BWD_MODES = (("bf16x6", 2e-5), ("bf16x3", 1e-4), ("f32", 2e-5))


def g(seed):
    return torch.Generator().manual_seed(seed)


def leaf(t, dev=None, dtype=None):
    t = t.detach().clone()
    if dtype is not None:
        t = t.to(dtype)
    if dev is not None:
        t = t.to(dev)
    return t.requires_grad_(True)


@pytest.fixture()
def Fm(pkg):
    from e3diff_amd.autograd import functional
    return functional


# ------------------------------------------------------------------------------------------------- masks and cases
def holes_mask(B, Lk, seed=11):
    """Bernoulli(0.6) keys, then: one whole 32-key tile in the middle zeroed (Lk > 64); item 0's last valid key BEFORE the
    last key tile (the skip logic derives k_tiles from the last valid key: the sweep of item 0 is cut); item 1's last
    valid key at Lk - 1 (full sweep across the hole); at least two valid keys per item."""
    assert B >= 2 and Lk > 32
    m = (torch.rand(B, Lk, generator=g(seed)) < 0.6).float()
    kt = (Lk + 31) // 32
    hole = (kt - 1) // 2 if Lk > 64 else None     # never tile 0, never the last tile
    if hole is not None:
        m[:, 32 * hole:32 * hole + 32] = 0
    last0 = 32 * (hole if hole == kt - 2 else kt - 1) - 6
    m[0, last0 + 1:] = 0
    m[0, last0] = 1
    m[1, Lk - 1] = 1
    for b in range(B):
        if m[b].sum() < 2:
            m[b, :2] = 1
    assert (int(m[0].nonzero().max()) >> 5) + 1 < kt and m[1, Lk - 1] == 1 and (m.sum(1) >= 2).all()
    assert hole is None or m[:, 32 * hole:32 * hole + 32].sum() == 0
    return m


class Case:
    """Inputs of one attention call (CPU fp32) and its key mask.  Self-attention: packed qkv [B L, 3H]; cross-attention:
    q [B Lq, H] and packed kv [B Lk, 2H]."""

    def __init__(self, Lq, Lk, cross, relkey=False, P=0, mask="prefix", lens=None, B=None):
        assert cross or Lq == Lk
        self.Lq, self.Lk, self.cross, self.P = Lq, Lk, cross, (P if relkey else 0)
        if mask == "prefix":
            assert max(lens) == Lk and min(lens) >= 1
            self.B = len(lens)
            self.mask = (torch.arange(Lk)[None] < torch.tensor(lens)[:, None]).float()
        elif mask == "holes":
            self.B = 3
            self.mask = holes_mask(self.B, Lk)
        else:
            self.B = B or 2
            self.mask = None
        B = self.B
        if cross:
            self.q_src = torch.randn(B * Lq, H, generator=g(1))
            self.kv_src = torch.randn(B * Lk, 2 * H, generator=g(2))
        else:
            self.q_src = torch.randn(B * Lq, 3 * H, generator=g(Lq))
            self.kv_src = None
        self.E = torch.randn(2 * P - 1, 64, generator=g(P + 1)) if relkey else None
        self.go = torch.randn(B * Lq, H, generator=g(9))

    def views(self, q_src, kv_src):
        if kv_src is None:
            return q_src[:, :H], q_src[:, H:2 * H], q_src[:, 2 * H:]
        return q_src, kv_src[:, :H], kv_src[:, H:]

    def parts(self, dq_src, dkv_src):
        """(name, gradient part) of the packed gradients: column slices."""
        dq, dk, dv = self.views(dq_src, dkv_src)
        return (("dq", dq), ("dk", dk), ("dv", dv))

    def reference(self, q_src, kv_src, E, mult=None):
        """fp64 statement -> (out [B Lq, H], scores [B, nh, Lq, Lk]); ``mult``: dropout multipliers on the probabilities."""
        q, k, v = self.views(q_src, kv_src)
        sp = lambda x, L: x.reshape(self.B, L, NH, 64).permute(0, 2, 1, 3)  # noqa: E731
        q, k, v = sp(q, self.Lq), sp(k, self.Lk), sp(v, self.Lk)
        s = q @ k.transpose(-1, -2)
        if E is not None:
            s = s + obert.relkey_scores_literal(q, E, self.P)
        s = s / 8.0
        if self.mask is not None:
            s = s + ((1.0 - self.mask.to(s.dtype)) * -10000.0)[:, None, None, :]
        p = torch.softmax(s, -1)
        if mult is not None:
            p = p * mult
        return (p @ v).permute(0, 2, 1, 3).reshape(self.B * self.Lq, H), s

    def reference_grads(self, mult=None):
        """fp64 autograd -> (out, {dq, dk, dv[, dE]}) as fp32 CPU tensors."""
        qr = leaf(self.q_src, dtype=torch.double)
        kvr = leaf(self.kv_src, dtype=torch.double) if self.cross else None
        Er = leaf(self.E, dtype=torch.double) if self.E is not None else None
        out, _ = self.reference(qr, kvr, Er, mult)
        out.backward(self.go.double())
        want = {n: t.float() for n, t in self.parts(qr.grad, kvr.grad if self.cross else None)}
        if Er is not None:
            want["dE"] = Er.grad.float()
        return out.detach().float(), want


def _report(figures):
    """Print every figure of a case, then assert them all (NaN fails: ``not e < tol``)."""
    for what, e, tol in figures:
        print(f"{what}: {e:.3e} ({tol:g})")
    bad = [(what, e, tol) for what, e, tol in figures if not e < tol]
    assert not bad, bad


def _forward_figures(pkg, c, with_bounds=False, modes=FWD_MODES):
    q_dev = c.q_src.to(DEV)
    kv_dev = c.kv_src.to(DEV) if c.cross else None
    q, k, v = c.views(q_dev, kv_dev)
    mask = c.mask.to(DEV) if c.mask is not None else None
    E = c.E.to(DEV) if c.E is not None else None
    ref, s = c.reference(c.q_src.double(), c.kv_src.double() if c.cross else None, c.E.double() if c.E is not None else None)
    ref, ref_lse = ref.float(), torch.logsumexp(s, -1).float()
    bounds = None
    if with_bounds:       # |element| bound of the Q and K rows: engages the padded-tile skip of the split kernels
        bound = pkg.ops.absmax(q_dev)
        assert float(bound) == float(c.q_src.abs().max())
        bounds = (bound, bound)
    figures = []
    for mode, tol in modes:
        got, lse = pkg.ops.attention(q, k, v, c.B, NH, c.Lq, c.Lk, key_mask=mask, dist_emb=E, max_pos=c.P, want_lse=True,
                                     mode=mode, bounds=bounds)
        figures += [(f"{mode} out", rel_err(got, ref), tol), (f"{mode} lse", rel_err(lse, ref_lse), tol)]
    return figures


def _backward_run(pkg, Fm, c, mode, drop_p=0.0):
    """Fm.attention(...).backward(go) in ``mode`` -> (out, {dq, dk, dv[, dE]})."""
    prev = pkg.ops.set_attn_mode(mode)
    try:
        qd = leaf(c.q_src, DEV)
        kvd = leaf(c.kv_src, DEV) if c.cross else None
        Ed = leaf(c.E, DEV) if c.E is not None else None
        out = Fm.attention(qd, kvd, c.B, NH, c.Lq, c.Lk, key_mask=c.mask.to(DEV) if c.mask is not None else None,
                           dist_emb=Ed, max_pos=c.P, drop_p=drop_p)
        out.backward(c.go.to(DEV))
    finally:
        pkg.ops.set_attn_mode(prev)
    got = dict(c.parts(qd.grad, kvd.grad if c.cross else None))
    if Ed is not None:
        got["dE"] = Ed.grad
    return out.detach(), got


def _backward_figures(pkg, Fm, c, modes=BWD_MODES):
    _, want = c.reference_grads()
    figures = []
    for mode, tol in modes:
        _, got = _backward_run(pkg, Fm, c, mode)
        figures += [(f"{mode} {n}", rel_err(got[n], want[n]), tol) for n in want]
    return figures


# ----------------------------------------------------------------------------------------- 1. forward edge matrix
# self-attention, prefix masks.  Kernel forms (table above): L = 1, 31, 33 the per-wave kernel in every split mode;
# L = 97, 100, 127 (4 query tiles) and 225 (8) the cooperative kernel in bf16x3 / f16x3 with a partly filled last
# query tile, an odd number of key tiles never (4 / 8) but a last key tile of 1 (97, 225), 4 (100) and 31 (127) rows.
FWD_SELF_PREFIX = {1: [1, 1], 31: [31, 1, 17], 33: [33, 1, 32], 97: [97, 1, 64], 100: [100, 1, 33], 127: [127, 1, 96],
                   225: [225, 1, 129]}


@pytest.mark.parametrize("relkey", [True, False])
@pytest.mark.parametrize("L", sorted(FWD_SELF_PREFIX))
def test_forward_self_ragged_lengths(pkg, hip, L, relkey):
    _report(_forward_figures(pkg, Case(L, L, False, relkey, L, "prefix", FWD_SELF_PREFIX[L])))


@pytest.mark.parametrize("relkey", [True, False])
@pytest.mark.parametrize("L", [33, 100, 225])
def test_forward_self_ragged_lengths_without_a_mask(pkg, hip, L, relkey):
    """No key mask: the keys past Lk in the last key tile are then excluded by the tile's row count alone (with a mask
    the cooperative kernel's range-checked mask load reads them as padded, which hides a wrong row count)."""
    _report(_forward_figures(pkg, Case(L, L, False, relkey, L, "none", B=2)))


@pytest.mark.parametrize("L", [97, 225])
def test_forward_self_table_longer_than_the_frame(pkg, hip, L):
    """P = L + 7: the distance table is longer than the frame, so the P - 1 offset differs from L - 1 (cooperative kernel:
    the fragment-order planes start at row P + 32 (j - J0); per-wave and exact kernels: e_lo = q0 - r0 - 31 + P - 1)."""
    _report(_forward_figures(pkg, Case(L, L, False, True, L + 7, "prefix", FWD_SELF_PREFIX[L])))


# masks with holes against fp64: 97 (ragged cooperative frame), 128 and 256 (full cooperative frames: 4 and 8 key tiles,
# the hole is tile 1 / 3).  Without bounds every kernel sweeps all keys; with bounds the split kernels stop after the tile
# of the last valid key (item 0: cut before the last tile; item 1: full sweep across the hole).
@pytest.mark.parametrize("relkey", [True, False])
@pytest.mark.parametrize("L,with_bounds", [(97, False), (128, False), (256, False), (128, True), (256, True)])
def test_forward_self_masks_with_holes(pkg, hip, L, with_bounds, relkey):
    _report(_forward_figures(pkg, Case(L, L, False, relkey, L, "holes"), with_bounds))


# cross-attention (no rel-key).  Lq = 128 and 100: 4 query tiles, the cooperative kernel in bf16x3 / f16x3 -- Lk = 1 and
# 31 (one key tile, Lk < 32), 33 (two tiles, a one-row last tile: the clamped prefetch of the two-tiles-per-iteration
# sweep), 70 and 96 (odd k_tiles = 3), 160 (5 tiles under a ragged query frame), 257 (9 tiles, one-row last tile, the
# mask loop beyond the 256 keys kept in registers), 300 (10 tiles).  Lq = 1 and 40: the per-wave kernel, Lk = 128 / 200.
FWD_CROSS_PREFIX = {(128, 1): [1, 1], (128, 31): [31, 1, 16], (128, 33): [33, 1, 32], (128, 70): [70, 1, 64],
                    (128, 96): [96, 1, 65], (100, 160): [160, 1, 129], (128, 257): [257, 1, 256],
                    (128, 300): [300, 1, 255], (1, 128): [128, 1, 97], (40, 200): [200, 1, 33]}
FWD_CROSS = [(s, m) for s in FWD_CROSS_PREFIX for m in ("none", "prefix")] + \
            [(s, "holes") for s in ((128, 96), (128, 300), (40, 200))]


@pytest.mark.parametrize("shape,mask", FWD_CROSS, ids=[f"{s[0]}x{s[1]}-{m}" for s, m in FWD_CROSS])
def test_forward_cross_edge_shapes(pkg, hip, shape, mask):
    # (no element bounds: every kernel sweeps all keys, holes included; the test below engages the skip at Lk > 256)
    Lq, Lk = shape
    _report(_forward_figures(pkg, Case(Lq, Lk, True, mask=mask, lens=FWD_CROSS_PREFIX[shape], B=3)))


@pytest.mark.parametrize("shape", [(128, 300), (128, 257)])
def test_forward_cross_long_key_frames_with_the_tile_skip_engaged(pkg, hip, shape):
    """Lk > 256 with element bounds: the cooperative kernel's scan of the key mask beyond the 256 keys it keeps in
    registers decides k_tiles (prefix lengths 1 / 255 / 256: the sweep stops inside the first 256 keys; full length and
    holes: the last valid key lies beyond them)."""
    Lq, Lk = shape
    for mask in ("prefix", "holes"):
        c = Case(Lq, Lk, True, mask=mask, lens=FWD_CROSS_PREFIX[shape])
        bound = pkg.ops.absmax(torch.cat([c.q_src.flatten(), c.kv_src.flatten()]).to(DEV))
        q, k, v = c.views(c.q_src.to(DEV), c.kv_src.to(DEV))
        ref, s = c.reference(c.q_src.double(), c.kv_src.double(), None)
        figures = []
        for mode, tol in FWD_MODES[1:]:
            got, lse = pkg.ops.attention(q, k, v, c.B, NH, Lq, Lk, key_mask=c.mask.to(DEV), want_lse=True, mode=mode,
                                         bounds=(bound, bound))
            figures += [(f"{mask} {mode} out", rel_err(got, ref.float()), tol),
                        (f"{mask} {mode} lse", rel_err(lse, torch.logsumexp(s, -1).float()), tol)]
        _report(figures)


# ---------------------------------------------------------------------------- 2. backward edge matrix, per part
# self-attention.  bf16x3: L <= 128 the fused kernel (2: one tile of two rows; 31, 33: partial first / second tile; 97,
# 100: a last tile of 1 / 4 rows; 128: the last fused shape), 129, 160, 225 the two-launch split kernels (5, 5 and 8
# tiles, last tile of 1 / 32 / 1 rows).  bf16x6 and f32: the fp32-MFMA two-launch kernels at every one of them.
BWD_SELF_PREFIX = {2: [2, 2], 31: [31, 2, 17], 33: [33, 2, 32], 97: [97, 2, 64], 100: [100, 2, 33], 128: [128, 2, 97],
                   129: [129, 2, 128], 160: [160, 2, 129], 225: [225, 2, 129]}
BWD_SELF = [(L, "prefix") for L in sorted(BWD_SELF_PREFIX)] + [(L, "holes") for L in (100, 128, 160)]


@pytest.mark.parametrize("relkey", [True, False])
@pytest.mark.parametrize("L,mask", BWD_SELF, ids=[f"{L}-{m}" for L, m in BWD_SELF])
def test_backward_self_per_part(pkg, hip, Fm, L, mask, relkey):
    _report(_backward_figures(pkg, Fm, Case(L, L, False, relkey, L, mask, BWD_SELF_PREFIX[L])))


# cross-attention.  bf16x3 fused: 128x2, 100x33, 128x96, 97x128 (rectangular, ragged on either side); two-launch split
# kernels as soon as ONE side crosses 128: 129x64, 64x129, 40x200, 200x40, 128x300.
BWD_CROSS_PREFIX = {(128, 2): [2, 2], (100, 33): [33, 2, 32], (128, 96): [96, 2, 65], (97, 128): [128, 2, 97],
                    (129, 64): [64, 2, 33], (64, 129): [129, 2, 128], (40, 200): [200, 2, 33], (200, 40): [40, 2, 32],
                    (128, 300): [300, 2, 257]}
BWD_CROSS = [(s, "prefix") for s in BWD_CROSS_PREFIX] + [(s, "holes") for s in ((128, 96), (40, 200))]


@pytest.mark.parametrize("shape,mask", BWD_CROSS, ids=[f"{s[0]}x{s[1]}-{m}" for s, m in BWD_CROSS])
def test_backward_cross_per_part(pkg, hip, Fm, shape, mask):
    Lq, Lk = shape
    _report(_backward_figures(pkg, Fm, Case(Lq, Lk, True, mask=mask, lens=BWD_CROSS_PREFIX[shape])))


@pytest.mark.parametrize("kind", ["self33", "cross128x1"])
def test_backward_where_the_reference_gradient_is_identically_zero(pkg, hip, Fm, kind):
    """An item with exactly ONE valid key has softmax = (1, 0, ...) whatever q and k are: dq = dk = 0 in exact arithmetic.
    dv (and dE) are compared as everywhere; dq / dk of the one-key item must be noise-sized:
    |dS| <= 64 max|dout| max|v| and dq = dS k / 8 give max|dq| <= tol * 8 max|dout| max|v| max|k| (max|q| for dk) --
    deliberately loose: it catches garbage, not rounding.  The other item of the self case keeps the relative bound."""
    if kind == "self33":
        c = Case(33, 33, False, True, 33, "prefix", [33, 1])
        one_key = [1]
    else:
        c = Case(128, 1, True, mask="none", B=2)
        one_key = [0, 1]
    _, want = c.reference_grads()
    q, k, v = c.views(c.q_src, c.kv_src)
    scale = {"dq": 8 * float(c.go.abs().max()) * float(v.abs().max()) * float(k.abs().max()),
             "dk": 8 * float(c.go.abs().max()) * float(v.abs().max()) * float(q.abs().max())}
    rows = lambda t, L, items: t.reshape(c.B, L, -1)[items]  # noqa: E731
    others = [b for b in range(c.B) if b not in one_key]
    figures = []
    for mode, tol in BWD_MODES:
        _, got = _backward_run(pkg, Fm, c, mode)
        figures += [(f"{mode} {n}", rel_err(got[n], want[n]), tol) for n in want if n in ("dv", "dE")]
        for n, L in (("dq", c.Lq), ("dk", c.Lk)):
            assert float(rows(want[n], L, one_key).abs().max()) < 1e-30          # (the reference: exact zeros up to fp64 noise)
            figures.append((f"{mode} max|{n}| of the one-key items / scale", float(rows(got[n], L, one_key).abs().max()) / scale[n], tol))
            if others:
                figures.append((f"{mode} {n} of the other items", rel_err(rows(got[n], L, others), rows(want[n], L, others)), tol))
    _report(figures)


# ---------------------------------- 3. every output row written, nothing beyond, batch strides honoured (C entry points)
SENTINEL = -12345.6789       # (finite, non-zero: float equality with it is bit identity)
TAIL = 64                    # sentinel rows behind every output allocation
GAP = 8                      # rows between the items of a strided frame: batch stride (L + 8) * row stride
DIRECT_SHAPES = {"self100": (100, 100, False, [100, 33]), "cross128x70": (128, 70, True, [70, 3]),
                 "cross129x40": (129, 40, True, [40, 3])}


def _direct_case(name):
    Lq, Lk, cross, lens = DIRECT_SHAPES[name]
    return Case(Lq, Lk, cross, not cross, Lq, "prefix", lens)


def _strided_input(x, B, L):
    """[B L, W] -> device frame [B, L + GAP, W] whose gap rows are NaN."""
    f = torch.full((B, L + GAP, x.shape[1]), float("nan"))
    f[:, :L] = x.view(B, L, -1)
    return f.to(DEV)


def _guarded(rows, width, B=None, L=None):
    """An output allocation of ``rows`` rows (+ TAIL sentinel rows); the rows that belong to an item are NaN, everything
    else holds the sentinel.  With (B, L): a strided frame [B, L + GAP, width], ``rows`` = B (L + GAP).
    Returns (buffer, bool row index of the item rows)."""
    buf = torch.full((rows + TAIL, width), SENTINEL, device=DEV)
    item = torch.zeros(rows + TAIL, dtype=torch.bool, device=DEV)
    if B is None:
        item[:rows] = True
    else:
        item[:rows].view(B, L + GAP)[:, :L] = True
    buf[item] = float("nan")
    return buf, item


def _check_guarded(figures, what, buf, item, want, tol):
    got = buf[item]
    assert torch.isfinite(got).all(), f"{what}: rows left unwritten (or not finite)"
    assert torch.equal(buf[~item], torch.full_like(buf[~item], SENTINEL)), f"{what}: written outside the item rows"
    figures.append((what, rel_err(got.reshape(want.shape), want), tol))


class _Direct:
    """Strided device frames of a case and the forward call through the C ABI, as ops.attention makes it."""

    def __init__(self, pkg, lib, c):
        self.pkg, self.lib, self.c = pkg, lib, c
        self.qf = _strided_input(c.q_src, c.B, c.Lq)
        self.kvf = _strided_input(c.kv_src, c.B, c.Lk) if c.cross else None
        q, k, v = c.views(self.qf.view(-1, self.qf.shape[-1]), self.kvf.view(-1, 2 * H) if c.cross else None)
        self.in_args = ()
        for t, L in ((q, c.Lq), (k, c.Lk), (v, c.Lk)):
            assert t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0
            self.in_args += (t.data_ptr(), (L + GAP) * t.stride(0), t.stride(0))
        self.E = c.E.to(DEV) if c.E is not None else None
        self.mask = c.mask.to(DEV)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.out, self.out_item = _guarded(c.B * c.Lq, H)
        self.lse, self.lse_item = _guarded(c.B * NH, c.Lq)

    def forward(self, terms):
        c, lib, p = self.c, self.lib, self.pkg.ops._p
        args = self.in_args + (p(self.E), c.P, p(self.mask), p(self.out), p(self.lse), c.B, NH, c.Lq, c.Lk)
        if terms == 0:
            self.pkg.hip.check(lib.e3d_relkey_attn_fwd(*args, self.stream), "e3d_relkey_attn_fwd")
            return
        self.scratch = None
        if self.E is not None:      # the planes of the distance table (cooperative kernel), with a tail of their own
            n = lib.e3d_attn_scratch_bytes(c.Lk)
            self.scratch = torch.full((n + 1024,), 0x5A, dtype=torch.uint8, device=DEV)
        self.pkg.hip.check(lib.e3d_relkey_attn_fwd_split_ex(*args, terms, 0.0, 0, p(self.scratch), 0, None, None, None,
                                                            self.stream), "e3d_relkey_attn_fwd_split_ex")
        if self.scratch is not None:
            assert bool((self.scratch[n:] == 0x5A).all()), "distance-table planes written past the scratch"


@pytest.mark.parametrize("mode,tol", FWD_MODES)
@pytest.mark.parametrize("name", sorted(DIRECT_SHAPES))
def test_forward_writes_every_row_and_nothing_else_from_strided_frames(pkg, hip, name, mode, tol):
    """e3d_relkey_attn_fwd / e3d_relkey_attn_fwd_split_ex on inputs whose batch stride is (L + 8) x the row stride (the
    Python wrappers always pass L x row stride), NaN in the rows between the items; out / lse prefilled with NaN and
    followed by sentinel rows.  self100: rel-key, cooperative kernel on a ragged frame in bf16x3 / f16x3; 128x70: the
    cooperative kernel with 3 key tiles; 129x40: 5 query tiles, the per-wave kernel."""
    c = _direct_case(name)
    ref, s = c.reference(c.q_src.double(), c.kv_src.double() if c.cross else None, c.E.double() if c.E is not None else None)
    d = _Direct(pkg, hip, c)
    d.forward(pkg.ops.GEMM_MODES[mode])
    figures = []
    _check_guarded(figures, f"{mode} out", d.out, d.out_item, ref.float(), tol)
    _check_guarded(figures, f"{mode} lse", d.lse, d.lse_item, torch.logsumexp(s, -1).float().reshape(c.B * NH, c.Lq), tol)
    _report(figures)


@pytest.mark.parametrize("terms,tol", [(0, 2e-5), (6, 2e-5), (3, 1e-4)])
@pytest.mark.parametrize("name", sorted(DIRECT_SHAPES))
def test_backward_writes_every_row_and_nothing_else_into_strided_frames(pkg, hip, name, terms, tol):
    """e3d_relkey_attn_bwd_ex as _Attention.backward calls it, but with inputs AND gradient outputs in frames of batch
    stride (L + 8) x row stride, every output (and the workspace) prefilled with NaN, sentinel rows between the items and
    behind every allocation.  Every gradient row of an item -- padded queries and keys included, the reference defines
    them -- must be finite and match fp64; nothing else may change.  terms 3: the fused kernel at 100 and 128x70, the
    two-launch split kernels at 129x40; terms 0 / 6: the fp32-MFMA kernels."""
    c = _direct_case(name)
    _, want = c.reference_grads()
    d = _Direct(pkg, hip, c)
    d.forward(terms)
    assert torch.isfinite(d.out[d.out_item]).all() and torch.isfinite(d.lse[d.lse_item]).all()
    lib, p = hip, pkg.ops._p
    dqf, dq_item = _guarded(c.B * (c.Lq + GAP), d.qf.shape[-1], c.B, c.Lq)
    dkvf, dkv_item = _guarded(c.B * (c.Lk + GAP), 2 * H, c.B, c.Lk) if c.cross else (None, None)
    dq, dk, dv = c.views(dqf, dkvf)
    dE, dE_item = _guarded(2 * c.P - 1, 64) if c.E is not None else (None, None)
    n_ws = lib.e3d_relkey_attn_bwd_workspace_floats(c.B, NH, c.Lq, c.Lk, int(c.E is not None))
    ws = torch.full((n_ws + TAIL * 64,), float("nan"), device=DEV)
    ws[n_ws:] = SENTINEL
    out_args = ()
    for t, L in ((dq, c.Lq), (dk, c.Lk), (dv, c.Lk)):
        assert t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0
        out_args += (t.data_ptr(), (L + GAP) * t.stride(0), t.stride(0))
    dout = c.go.to(DEV)
    pkg.hip.check(lib.e3d_relkey_attn_bwd_ex(*d.in_args, p(d.E), c.P, p(d.mask), p(d.out), p(d.lse), p(dout), *out_args, p(dE),
                                             p(ws), c.B, NH, c.Lq, c.Lk, terms, 0.0, 0, d.stream), "e3d_relkey_attn_bwd_ex")
    assert torch.equal(ws[n_ws:], torch.full_like(ws[n_ws:], SENTINEL)), "written past the workspace"
    figures = []
    if c.cross:
        _check_guarded(figures, f"terms {terms} dq", dqf, dq_item, want["dq"], tol)
        got_kv = dkvf[dkv_item]
        assert torch.isfinite(got_kv).all(), "dk / dv: rows left unwritten (or not finite)"
        assert torch.equal(dkvf[~dkv_item], torch.full_like(dkvf[~dkv_item], SENTINEL)), "dk / dv: written outside the item rows"
        figures += [(f"terms {terms} dk", rel_err(got_kv[:, :H], want["dk"]), tol),
                    (f"terms {terms} dv", rel_err(got_kv[:, H:], want["dv"]), tol)]
    else:
        got = dqf[dq_item]
        assert torch.isfinite(got).all(), "dq / dk / dv: rows left unwritten (or not finite)"
        assert torch.equal(dqf[~dq_item], torch.full_like(dqf[~dq_item], SENTINEL)), "dq / dk / dv: written outside the item rows"
        figures += [(f"terms {terms} {n}", rel_err(t, want[n]), tol) for n, t in c.parts(got, None)]
        _check_guarded(figures, f"terms {terms} dE", dE, dE_item, want["dE"], tol)
    _report(figures)


# --------------------------------------- 3b. Q, K, V and dq, dk, dv in frames of their own, no two strides alike
# Through ops.attention K and V share one buffer and Q / K / V one row stride, so the library could swap the strides of
# two views and every other test would still pass.  Here each view has a frame [B, L + gap, row stride] of its own:
# row strides are distinct multiples of 4 floats (16-byte rows) above H = 128, gaps differ, so do the batch strides.
SEPARATE = {"q": (132, 8), "k": (136, 5), "v": (144, 3), "dq": (140, 6), "dk": (148, 2), "dv": (152, 7)}   # row stride, gap


def _separate_input(x, B, L, name):
    """[B L, H] -> (device frame [B, L + gap, row stride], view triple); pad columns and gap rows are NaN."""
    rs, gap = SEPARATE[name]
    f = torch.full((B, L + gap, rs), float("nan"))
    f[:, :L, :H] = x.reshape(B, L, H)
    f = f.to(DEV)
    return f, (f.data_ptr(), (L + gap) * rs, rs)


def _separate_output(B, L, name):
    """(buffer, bool element index of the item elements, view triple): the item elements are NaN; pad columns, gap rows
    and TAIL rows behind the frame hold the sentinel."""
    rs, gap = SEPARATE[name]
    rows = B * (L + gap)
    buf = torch.full((rows + TAIL, rs), SENTINEL, device=DEV)
    item = torch.zeros_like(buf, dtype=torch.bool)
    item[:rows].view(B, L + gap, rs)[:, :L, :H] = True
    buf[item] = float("nan")
    return buf, item, (buf.data_ptr(), (L + gap) * rs, rs)


class _DirectSeparate(_Direct):
    def __init__(self, pkg, lib, c):
        self.pkg, self.lib, self.c = pkg, lib, c
        q, k, v = c.views(c.q_src, c.kv_src)
        self.frames, self.in_args = [], ()        # (the frames are kept alive)
        for name, t, L in (("q", q, c.Lq), ("k", k, c.Lk), ("v", v, c.Lk)):
            f, triple = _separate_input(t, c.B, L, name)
            self.frames.append(f)
            self.in_args += triple
        assert len(set(self.in_args[1::3])) == 3 and len(set(self.in_args[2::3])) == 3
        self.E = c.E.to(DEV) if c.E is not None else None
        self.mask = c.mask.to(DEV)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.out, self.out_item = _guarded(c.B * c.Lq, H)
        self.lse, self.lse_item = _guarded(c.B * NH, c.Lq)


_separate_refs = {}


def _separate_reference(name):
    """(case, fp64 out, fp64 lse, fp64 gradients) of a DIRECT_SHAPES case, computed once."""
    if name not in _separate_refs:
        c = _direct_case(name)
        _, s = c.reference(c.q_src.double(), c.kv_src.double() if c.cross else None, c.E.double() if c.E is not None else None)
        out, want = c.reference_grads()
        _separate_refs[name] = (c, out, torch.logsumexp(s, -1).float().reshape(c.B * NH, c.Lq), want)
    return _separate_refs[name]


@pytest.mark.parametrize("mode,tol", FWD_MODES)
@pytest.mark.parametrize("name", sorted(DIRECT_SHAPES))
def test_forward_from_separate_frames_of_pairwise_different_strides(pkg, hip, name, mode, tol):
    """test_forward_writes_every_row_and_nothing_else_from_strided_frames with Q, K and V in three frames whose row
    strides (132, 136, 144) and batch strides all differ: a batch or row stride taken from the wrong view reads NaN
    (pad columns, gap rows) or the wrong rows."""
    c, ref, ref_lse, _ = _separate_reference(name)
    d = _DirectSeparate(pkg, hip, c)
    d.forward(pkg.ops.GEMM_MODES[mode])
    figures = []
    _check_guarded(figures, f"{mode} out", d.out, d.out_item, ref, tol)
    _check_guarded(figures, f"{mode} lse", d.lse, d.lse_item, ref_lse, tol)
    _report(figures)


@pytest.mark.parametrize("terms,tol", [(0, 2e-5), (6, 2e-5), (3, 1e-4)])
@pytest.mark.parametrize("name", sorted(DIRECT_SHAPES))
def test_backward_into_separate_frames_of_pairwise_different_strides(pkg, hip, name, terms, tol):
    """test_backward_writes_every_row_and_nothing_else_into_strided_frames with Q, K, V and dq, dk, dv in six frames, no
    two row strides and no two batch strides alike: every gradient element of an item finite and equal to fp64; pad
    columns, gap rows, the rows behind every frame and behind the workspace untouched."""
    c, _, _, want = _separate_reference(name)
    d = _DirectSeparate(pkg, hip, c)
    d.forward(terms)
    assert torch.isfinite(d.out[d.out_item]).all() and torch.isfinite(d.lse[d.lse_item]).all()
    lib, p = hip, pkg.ops._p
    grads = {n: _separate_output(c.B, L, n) for n, L in (("dq", c.Lq), ("dk", c.Lk), ("dv", c.Lk))}
    out_args = grads["dq"][2] + grads["dk"][2] + grads["dv"][2]
    assert len(set((d.in_args + out_args)[1::3])) == 6 and len(set((d.in_args + out_args)[2::3])) == 6
    dE, dE_item = _guarded(2 * c.P - 1, 64) if c.E is not None else (None, None)
    n_ws = lib.e3d_relkey_attn_bwd_workspace_floats(c.B, NH, c.Lq, c.Lk, int(c.E is not None))
    ws = torch.full((n_ws + TAIL * 64,), float("nan"), device=DEV)
    ws[n_ws:] = SENTINEL
    dout = c.go.to(DEV)
    pkg.hip.check(lib.e3d_relkey_attn_bwd_ex(*d.in_args, p(d.E), c.P, p(d.mask), p(d.out), p(d.lse), p(dout), *out_args, p(dE),
                                             p(ws), c.B, NH, c.Lq, c.Lk, terms, 0.0, 0, d.stream), "e3d_relkey_attn_bwd_ex")
    assert torch.equal(ws[n_ws:], torch.full_like(ws[n_ws:], SENTINEL)), "written past the workspace"
    figures = []
    for n, (buf, item, _) in grads.items():
        _check_guarded(figures, f"terms {terms} {n}", buf, item, want[n], tol)
    if c.E is not None:
        _check_guarded(figures, f"terms {terms} dE", dE, dE_item, want["dE"], tol)
    _report(figures)


# ------------------------------------------------------------------- 4. dropout on the ragged cooperative shapes
@pytest.mark.parametrize("name", ["self100", "cross128x70"])
def test_dropout_on_ragged_cooperative_shapes(pkg, hip, Fm, name):
    """The pattern of test_attention_probability_dropout_forward_and_backward (the library regenerates the multipliers,
    the fp64 statement consumes them) at L = 100 with rel-key and at 128 x 70: in bf16x3 the DROP instantiation of the
    cooperative forward on a partial last query tile / an odd number of key tiles, and the regenerated decisions of the
    fused backward; bf16x6 the per-wave forward and the fp32-MFMA backward.  Forward and per-part backward."""
    ops, p = pkg.ops, 0.1
    if name == "self100":
        c = Case(100, 100, False, True, 100, "prefix", [100, 2, 33])
    else:
        c = Case(128, 70, True, mask="prefix", lens=[70, 2, 64])
    figures = []
    for mode, tol in (("bf16x6", 2e-5), ("bf16x3", 1e-4)):
        torch.manual_seed(100)
        seed = ops.next_dropout_seed()
        mult = ops.attn_dropout_mask(c.B, NH, c.Lq, c.Lk, p, seed).cpu()
        assert torch.unique(mult).tolist() == [0.0, pytest.approx(65536.0 / (65536 - 6554))]
        assert abs((mult == 0).float().mean().item() - 0.1) < 0.02
        ref_out, want = c.reference_grads(mult.double())
        torch.manual_seed(100)             # Fm.attention draws the same seed
        out, got = _backward_run(pkg, Fm, c, mode, drop_p=p)
        figures.append((f"{mode} out", rel_err(out, ref_out), tol))
        figures += [(f"{mode} {n}", rel_err(got[n], want[n]), tol) for n in want]
    _report(figures)
