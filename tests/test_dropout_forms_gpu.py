"""GPU: the seeded (unkeyed) dropout stream in every kernel that draws from it, against tests/dropout_ref.py -- a numpy
restatement written from the header's prose, tied to the published SplitMix64 sequence by tests/test_dropout_ref_cpu.py.
The other dropout tests compare kernels with multipliers that the library itself exports (e3d_attn_dropout_mask, dropout
of ones): a mistake in the shared law of csrc/e3d_common.h passes all of them.  Here nothing of the library tells the
test what the decisions are.  Every comparison is bit for bit unless it names a tolerance.

The device epoch word (e3d_dropout_set_epoch_ptr) is part of the law and is process-global: every test READS it
(``ops.dropout_epoch``) and hands the value to the restatement; where a test sets it (0, 1, 2^40 + 3) it restores the old
value in a ``finally``.  No test assumes a value.

One row per launch site and branch (D = csrc/dropout.hip, R = csrc/rowops.hip, T = csrc/train_ops.hip):

=====  ====================================  ==========================================  ==============================================
line   kernel                                branch, and what reaches it                 test id
=====  ====================================  ==========================================  ==============================================
D:80   dropout_kernel                        tail group only: n < 4                      test_elementwise_small[1|2|3-*]
D:80   dropout_kernel                        full groups, empty tail: n % 4 == 0         test_elementwise_small[4|8|1024-*]
D:80   dropout_kernel                        full groups + tail, > 1 block: n >= 1021    test_elementwise_small[1023|1025-*]
D:80   dropout_kernel                        the last single-trip size, 8192 blocks      test_elementwise_large[8388607-*]
D:80   dropout_kernel                        second trip of the stride loop with the     test_elementwise_large[8389811-*]
                                             3-element tail inside it: n >= 8388608
D:80   dropout_kernel                        p = 0 (thr 0, scale 1), guarded out         test_elementwise_c_entry_point_with_guards
D:90   attn_drop_mask_kernel                 one trip, Lk < 4 / Lk % 4 = 2               test_attention_mask[1-1-1-1|2-3-5-3|2-2-33-70]
D:90   attn_drop_mask_kernel                 second key trip: Lk > 256                   test_attention_mask[1-2-40-257|3-2-100-300]
D:115  dropout_rows_kernel (keyed)           row-stride loop: M > 32768                  test_keyed_rows_past_the_grid_cap
R:332  residual_layernorm_kernel<V, true>    V = 1, 3, 4; e3d_residual_layernorm_drop_fwd  test_fused_hidden_sites[*]
T:579  layernorm_bwd_kernel<V, true>, ws     e3d_layernorm_bwd_ws, drop_p > 0            test_fused_hidden_sites[*]
T:624  layernorm_bwd_kernel<V, true>         e3d_layernorm_bwd_drop                      test_fused_hidden_sites[*]
-      attention forward, DROP               f32, bf16x6 and f16x3 (no DROP form of its  test_attention_forward[*]
                                             own: attn_coop_ok): per-wave split kernel in
                                             its three-term form; bf16x3: cooperative
                                             kernel (4 query tiles), 10 / 9 key tiles with
                                             and without the padded-tile skip, ragged L = 100
-      attention backward, DROP              f32 / bf16x6: fp32-MFMA two-launch kernels;  test_attention_backward[*]
                                             bf16x3: fused kernel at 128 x 96, two-launch
                                             split kernels at 160 and 40 x 200; holes masks
=====  ====================================  ==========================================  ==============================================

Tolerances are the project's existing ones: FWD_MODES / BWD_MODES of test_attention_edges_gpu.py, 2e-5 for the fused
residual LayerNorm forward (test_dropout_folded_into_the_residual_layernorm_kernels' family).  Worst error / tolerance
measured on an MI355X (each test prints its figures):

  residual LayerNorm forward (2e-5)                 0.003 / 0.004 / 0.004 / 0.007 at (1, 256) / (5, 768) / (33, 1024) / (70, 768)
  attention forward  cross 128 x 300                0.112  (bf16x3 1.12e-5 of 1e-4; the three-term modes 1.2e-7 of 1e-5)
                     cross 128 x 257                0.071  (bf16x3 7.1e-6; three-term 1.3e-7); the same figures with the skip
                     self 100, rel-key              0.066  (bf16x3 6.6e-6; three-term 3.0e-7)
  attention backward self 160, holes                0.125  (bf16x3 dk, dE 1.25e-5 of 1e-4; bf16x6 / f32 at most 1.3e-6 of 2e-5)
                     cross 40 x 200, holes          0.123  (bf16x3 dv 1.23e-5; bf16x6 / f32 at most 1.3e-6)
                     cross 128 x 96, prefix         0.119  (bf16x3 dk 1.20e-5; bf16x6 / f32 at most 4.7e-7)
The whole file: 49 tests in 5.4 s, the slowest 0.9 s.  No kernel disagreed with the restatement.
"""
import contextlib

import numpy as np
import pytest
import torch

import dropout_ref as D
import keyed_dropout_ref as KD
from helpers import rel_err
from test_attention_edges_gpu import (BWD_CROSS_PREFIX, BWD_MODES, FWD_CROSS_PREFIX, FWD_MODES, FWD_SELF_PREFIX, NH, Case, Fm,  # noqa: F401
                                      _backward_run, _report)
from test_rowops_forms_gpu import Out, Vec, bits, call, p as ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPOCHS = (0, 1, 2 ** 40 + 3)
PS = (0.1, 0.5)


def g(seed):
    return torch.Generator().manual_seed(seed)


@contextlib.contextmanager
def epoch_word(pkg, value=None):
    """The device epoch word as an unsigned Python integer; ``value``: set for the duration, the old value restored."""
    word = pkg.ops.dropout_epoch(DEV)
    old = word.clone()
    try:
        if value is not None:
            word.fill_(value)
        yield int(word.item()) & D.MASK64
    finally:
        word.copy_(old)
        torch.cuda.synchronize()


def drawn_seed(pkg, k):
    """The seed the next dropout site draws under torch.manual_seed(k); the generator is left where the site finds it."""
    torch.manual_seed(k)
    seed = pkg.ops.next_dropout_seed()
    torch.manual_seed(k)
    return seed


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ e3d_dropout_f32
def check_elementwise(pkg, n, p, epoch, seed):
    mult = dev(D.elementwise_mult(n, p, seed, epoch))
    x = torch.randn(n, generator=g(n % 1000 + 1)).to(DEV)
    got = pkg.ops.dropout(x, p, seed)
    assert torch.equal(bits(got), bits(x * mult)), f"n={n} p={p} epoch={epoch}: x * multiplier"
    ones = pkg.ops.dropout(torch.ones(n, device=DEV), p, seed)
    assert torch.equal(bits(ones), bits(mult)), f"n={n} p={p} epoch={epoch}: multipliers"
    return mult


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025])
def test_elementwise_small(pkg, hip, n, p):
    with epoch_word(pkg) as epoch:
        check_elementwise(pkg, n, p, epoch, 0x1234567 + n)


@pytest.mark.parametrize("value", EPOCHS)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("n", [8388607, 8388608 + 1203])
def test_elementwise_large(pkg, hip, n, p, value):
    """8388607: 2097152 groups, the last one a 3-element tail = one trip of 8192 x 256 threads.  8389811: 2097453 groups,
    301 threads take a second trip, the last of them the 3-element tail."""
    assert ((n >> 2) + 1 > 8192 * 256) == (n > 8388607) and n % 4 == 3
    with epoch_word(pkg, value) as epoch:
        assert epoch == value
        mult = check_elementwise(pkg, n, p, epoch, 987654321)
    drop = float((mult == 0).float().mean())
    assert abs(drop - D.threshold(p) / 65536) < 1e-3, drop


def test_elementwise_c_entry_point_with_guards(pkg, hip):
    """e3d_dropout_f32 itself, ``out`` between guard words: a tail of 1, 2 and 3 elements and the two-trip size; p = 0."""
    with epoch_word(pkg) as epoch:
        for n, p, seed in ((5, 0.5, 3), (1023, 0.1, 2 ** 63 + 5), (1026, 0.5, 2 ** 64 - 1), (8388608 + 1203, 0.1, 77), (7, 0.0, 11)):
            x = torch.randn(n, generator=g(4)).to(DEV)
            out = Vec(n)
            call(pkg, "e3d_dropout_f32", ptr(x), p, seed, out.ptr, n)
            got = out.get(f"e3d_dropout_f32 n={n}")
            mult = dev(D.elementwise_mult(n, p, seed, epoch))
            assert torch.equal(bits(got), bits(x * mult)), (n, p, seed)
            if p == 0.0:
                assert torch.equal(bits(got), bits(x))


# ------------------------------------------------------------------------------------------------ e3d_attn_dropout_mask
MASK_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 3), (2, 2, 33, 70), (1, 2, 40, 257), (3, 2, 100, 300)]


@pytest.mark.parametrize("shape", MASK_SHAPES, ids=["-".join(map(str, s)) for s in MASK_SHAPES])
def test_attention_mask(pkg, hip, shape):
    B, nh, Lq, Lk = shape
    for value in (None,) + (EPOCHS if shape == (2, 2, 33, 70) else ()):
        with epoch_word(pkg, value) as epoch:
            for p in PS:
                for seed in (5, 0xFEDCBA9876543210):
                    got = pkg.ops.attn_dropout_mask(B, nh, Lq, Lk, p, seed, device=DEV).cpu().numpy()
                    want = D.attn_mult(B, nh, Lq, Lk, p, seed, epoch)
                    assert got.shape == want.shape and np.array_equal(got, want), (shape, p, seed, epoch)


# ------------------------------------------------------------------------------------------------ keyed rows, M > 32768
def test_keyed_rows_past_the_grid_cap(pkg, hip):
    """dropout_rows_kernel: 8192 blocks x 4 rows; rows 32768 .. 32772 are the second trip of blocks 0 and 1."""
    M, H, p, site = 32768 + 5, 8, 0.1, 9
    keys = torch.randint(-2 ** 63, 2 ** 63 - 1, (M,), generator=g(6), dtype=torch.int64)
    got = pkg.ops.dropout(torch.ones(M, H, device=DEV), p, site, row_keys=keys.to(DEV)).cpu().numpy()
    want = KD.hidden_mult(keys.numpy().view(np.uint64), H, p, site)
    assert np.array_equal(got[32768:], want[32768:]), "the rows of the second trip"
    assert np.array_equal(got[:32768], want[:32768]), "the rows of the first trip"


# ------------------------------------------------------------------------------------------------ fused hidden sites
@pytest.mark.parametrize("M,H", [(1, 256), (5, 768), (33, 1024), (70, 768)])
def test_fused_hidden_sites(pkg, hip, M, H):
    """LayerNorm(dropout(x) + r) and its backward with the decisions of tests/dropout_ref.py -- not those of the unfused
    launch.  Backward: ds_dropped = ds * multiplier bit for bit (zero exactly where the restated multiplier is zero, ds *
    scale elsewhere), from e3d_layernorm_bwd_ws and from e3d_layernorm_bwd_drop.  Forward: the fp64 statement
    LN(x * mult + r) within 2e-5, and the pre-norm sum s = x * mult + r in fp32 exactly."""
    from e3diff_amd import autograd as AG
    ops, p, eps = pkg.ops, 0.1, 1e-12
    gen = g(M + H)
    x, r = torch.randn(M, H, generator=gen), torch.randn(M, H, generator=gen)
    ga, be = 1 + 0.1 * torch.randn(H, generator=gen), torch.randn(H, generator=gen)
    dy = torch.randn(M, H, generator=gen)
    xd, rd, gd, bd, dyd = (t.to(DEV) for t in (x, r, ga, be, dy))
    seed = drawn_seed(pkg, 40 + M)
    with epoch_word(pkg) as epoch:
        mult = D.hidden_mult(M, H, p, seed, epoch)
        out, s = ops.residual_layernorm(xd, rd, gd, bd, eps, want_s=True, drop=(p, seed))
        ds, _, _, dsd = AG.layernorm_bwd(dyd, s, gd, eps, drop=(p, seed))
        ds2, dsd2, both = Out(M, H), Out(M, H), Out(2, H)
        call(pkg, "e3d_layernorm_bwd_drop", ptr(dyd), ptr(s), ptr(gd), eps, ds2.ptr, dsd2.ptr, both.row(0), both.row(1), M, H, p, seed)
    mt = torch.from_numpy(mult)
    scale = torch.tensor(float(D.scale(p)))
    assert set(np.unique(mult).tolist()) <= {0.0, float(scale)}
    # forward
    s32 = x * mt + r
    assert torch.equal(bits(s.cpu()), bits(s32)), "s is not fp32 x * multiplier + r"
    ref = torch.nn.functional.layer_norm(x.double() * mt.double() + r.double(), (H,), ga.double(), be.double(), eps)
    e = rel_err(out, ref.float())
    print(f"M={M} H={H} residual_layernorm_drop_fwd out: {e:.3e} (2e-5), ratio {e / 2e-5:.3f}")
    assert e < 2e-5, e
    # backward
    for what, a, b in (("e3d_layernorm_bwd_ws", ds.cpu(), dsd.cpu()),
                       ("e3d_layernorm_bwd_drop", ds2.get("ds").cpu(), dsd2.get("ds_dropped").cpu())):
        zero = mt == 0
        assert bool((b[zero] == 0).all()), f"{what}: ds_dropped not zero where the multiplier is zero"
        assert torch.equal(bits(b[~zero]), bits((a * scale)[~zero])), f"{what}: ds_dropped != ds * scale where kept"
        assert bool((a != 0).all()) and bool((b[~zero] != 0).all())           # (so the zeros above are decisions)
    assert torch.equal(bits(ds.cpu()), bits(ds2.get("ds").cpu()))
    assert both.guards_intact()


# ------------------------------------------------------------------------------------------------ attention kernels
P_ATTN = 0.1


def restated_mult(pkg, c, seed, epoch):
    return torch.from_numpy(D.attn_mult(c.B, NH, c.Lq, c.Lk, P_ATTN, seed, epoch)).double()


FWD_DROP_CASES = {"cross128x300": lambda: Case(128, 300, True, mask="prefix", lens=FWD_CROSS_PREFIX[(128, 300)]),
                  "cross128x257": lambda: Case(128, 257, True, mask="prefix", lens=FWD_CROSS_PREFIX[(128, 257)]),
                  "self100": lambda: Case(100, 100, False, True, 100, "prefix", FWD_SELF_PREFIX[100])}


@pytest.mark.parametrize("name", sorted(FWD_DROP_CASES))
def test_attention_forward(pkg, hip, name):
    """ops.attention(..., drop=(p, seed)) in all four modes against the fp64 statement with the RESTATED multipliers.
    The cross frames also run with element bounds, which engage the padded-tile skip (the sweep then stops after the tile
    of the last valid key: the group index of a key tile must not depend on how many tiles are swept)."""
    c = FWD_DROP_CASES[name]()
    ops = pkg.ops
    seed = drawn_seed(pkg, 100)
    q_dev, kv_dev = c.q_src.to(DEV), (c.kv_src.to(DEV) if c.cross else None)
    q, k, v = c.views(q_dev, kv_dev)
    E = c.E.to(DEV) if c.E is not None else None
    figures = []
    with epoch_word(pkg) as epoch:
        mult = restated_mult(pkg, c, seed, epoch)
        ref, _ = c.reference(c.q_src.double(), c.kv_src.double() if c.cross else None, c.E.double() if c.E is not None else None, mult)
        plain, _ = c.reference(c.q_src.double(), c.kv_src.double() if c.cross else None, c.E.double() if c.E is not None else None)
        assert rel_err(ref, plain) > 1e-2                                # (the multipliers matter at this tolerance)
        bound = ops.absmax(torch.cat([q_dev.flatten()] + ([kv_dev.flatten()] if c.cross else [])))
        for with_bounds in ((False, True) if c.cross else (False,)):
            for mode, tol in FWD_MODES:
                got = ops.attention(q, k, v, c.B, NH, c.Lq, c.Lk, key_mask=c.mask.to(DEV), dist_emb=E, max_pos=c.P, mode=mode,
                                    drop=(P_ATTN, seed), bounds=(bound, bound) if with_bounds else None)
                figures.append((f"{name} {mode}{' skip' if with_bounds else ''} out", rel_err(got, ref.float()), tol))
    print(f"{name}: worst error / tolerance {max(e / t for _, e, t in figures):.3f}")
    _report(figures)


BWD_DROP_CASES = {"self160-holes": lambda: Case(160, 160, False, True, 160, "holes"),
                  "cross40x200-holes": lambda: Case(40, 200, True, mask="holes"),
                  "cross128x96-prefix": lambda: Case(128, 96, True, mask="prefix", lens=BWD_CROSS_PREFIX[(128, 96)])}


@pytest.mark.parametrize("name", sorted(BWD_DROP_CASES))
def test_attention_backward(pkg, hip, Fm, name):
    """Fm.attention(..., drop_p).backward in the three modes: out and every gradient part against fp64 autograd through
    the statement with the restated multipliers of the seed the call draws."""
    c = BWD_DROP_CASES[name]()
    figures = []
    with epoch_word(pkg) as epoch:
        seed = drawn_seed(pkg, 100)
        ref_out, want = c.reference_grads(restated_mult(pkg, c, seed, epoch))
        for mode, tol in BWD_MODES:
            assert drawn_seed(pkg, 100) == seed                          # Fm.attention draws the same seed
            out, got = _backward_run(pkg, Fm, c, mode, drop_p=P_ATTN)
            figures.append((f"{name} {mode} out", rel_err(out, ref_out), tol))
            figures += [(f"{name} {mode} {n}", rel_err(got[n], want[n]), tol) for n in want]
    print(f"{name}: worst error / tolerance {max(e / t for _, e, t in figures):.3f}")
    _report(figures)
