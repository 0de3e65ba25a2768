"""The stride guard of the row-complete GEMM + LayerNorm entry points (csrc/gemm_rowln.hip), without a GPU.

The kernel addresses the rows of a tile by 32-bit byte offsets from the tile's first row -- ``(row * lda + chunk) * 4`` for
the up to 96 rows of A, ``(row * ldr + 4 lane) * 4`` for the 16 rows of a residual chunk -- so the predicate and the entry
points must refuse every stride at which the largest of them no longer fits: 96 lda < 2^30 and 16 ldr < 2^30.  (Under the
earlier 2^31 limits lda = 12 000 000 was accepted and row 95's offset wrapped past 2^32.)  Argument checks run before any
launch, so the refusals are observable on a machine without a device.
"""
import pytest
import torch

RBM, N = 96, 768
LDA_MAX = (2 ** 30 // RBM) // 4 * 4           # the largest accepted lda: a multiple of 4 with 96 lda < 2^30


def last_byte(lda):
    """One past the last byte a lane of the kernel reads of A, from the tile's first row: row 95, chunk 7 (floats 28..31)."""
    return ((RBM - 1) * lda + 28) * 4 + 16


def test_predicate_refuses_strides_whose_byte_offsets_wrap(pkg):
    ok = pkg.hip.lib().e3d_gemm_residual_layernorm_supported
    assert not ok(96, N, 64, 12_000_000) and last_byte(12_000_000) > 2 ** 32
    for lda in (768, 3072, LDA_MAX):
        assert ok(96, N, 64, lda), lda
    assert LDA_MAX % 4 == 0 and RBM * LDA_MAX < 2 ** 30 <= RBM * (LDA_MAX + 4)
    assert not ok(96, N, 64, LDA_MAX + 4) and not ok(96, N, 64, 2 ** 30 // RBM - 4)      # (the latter: not a multiple of 4)
    # whatever the predicate accepts keeps the largest byte offset inside 32 bits
    gen = torch.Generator().manual_seed(5)
    tried = list(range(LDA_MAX - 64, LDA_MAX + 68, 4)) + [2 ** 31 // RBM // 4 * 4, 2 ** 31 // RBM // 4 * 4 - 4, 2 ** 32 // RBM // 4 * 4]
    tried += [int(v) * 4 for v in torch.randint(16, 2 ** 29, (2000,), generator=gen)]
    accepted = [lda for lda in tried if ok(96, N, 64, lda)]
    assert len(accepted) > 10 and len(accepted) < len(tried)
    for lda in accepted:
        assert last_byte(lda) <= 2 ** 32, lda
    for lda in tried:
        assert bool(ok(96, N, 64, lda)) == (RBM * lda < 2 ** 30), lda


@pytest.mark.parametrize("entry", ["f32", "planes"])
def test_entry_points_refuse_a_wrapping_residual_stride_before_any_launch(pkg, entry):
    lib = pkg.hip.lib()
    buf = torch.zeros(4096 + 4)
    ptr = buf.data_ptr() + (-buf.data_ptr()) % 16            # a 16-byte aligned host address: never dereferenced
    assert ptr % 16 == 0
    M, K, ldr = 96, 64, 80_000_000
    assert 2 ** 30 <= 16 * ldr < 2 ** 31 and ldr % 4 == 0      # accepted by the earlier limit
    assert (15 * ldr + 4 * 63) * 4 + 2048 + 16 > 2 ** 32       # row 15 of a chunk, last third, last lane: wraps

    def call(ldr_):
        if entry == "f32":
            return lib.e3d_gemm_residual_layernorm_f32_split(ptr, K, ptr, ptr, ptr, ldr_, ptr, ptr, 1e-12, ptr, N, M, N, K, 19, 1.0, None)
        return lib.e3d_gemm_residual_layernorm_planes_split(ptr, ptr, ptr, ptr, ldr_, ptr, ptr, 1e-12, ptr, N, M, N, K, 19, 1.0, None)

    assert call(ldr) != 0
    msg = lib.e3d_last_error()
    assert b"residual" in msg and b"16*ldr < 2^30" in msg and b"80000000" in msg, msg
    assert call(2 ** 30 // 16) != 0 and b"16*ldr < 2^30" in lib.e3d_last_error()      # the first refused stride
    if entry == "f32":       # lda: the predicate speaks through the entry point
        assert lib.e3d_gemm_residual_layernorm_f32_split(ptr, 12_000_000, ptr, ptr, None, 0, ptr, ptr, 1e-12, ptr, N, M, N, K, 19, 1.0, None) != 0
        assert b"96*lda < 2^30" in lib.e3d_last_error() and b"12000000" in lib.e3d_last_error()
