// Dropout for the training path (reference: nn.Dropout(p = 0.1) in BertEmbeddings, BertSelfOutput,
// BertOutput, the SELayer MLP -- structure_model/model.py:45-47,109-117 -- and on the attention
// probabilities in transformers 4.38.2 BertSelfAttention).  Decisions come from the counter-based
// generator of e3d_common.h, so the backward pass re-applies the same op to the gradient.
#include "e3d_common.h"
#include "e3d_philox.h"

namespace {

__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, E3dDrop d_in, float* __restrict__ out,
                                                      int64_t n) {
    const E3dDrop d = e3d_drop_resolve(d_in);
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4 + 1; i += stride) {
        float m[4];
        e3d_drop_mult4(d, (uint64_t)i, m);
        if (i < n4) {
            f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] *= m[j];
            reinterpret_cast<f32x4*>(out)[i] = v;
        } else {
            for (int j = 0; 4 * n4 + j < n; ++j) out[4 * n4 + j] = x[4 * n4 + j] * m[j];
        }
    }
}

// keyed decisions on an [M, H] tensor (H % 4 == 0): a wave per row, the row's key read once
__global__ __launch_bounds__(256) void dropout_rows_kernel(const float* __restrict__ x, E3dDrop d, float* __restrict__ out,
                                                           int M, int H4) {
    const int lane = threadIdx.x & 63;
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < M; row += gridDim.x * 4) {
        const uint64_t rt = e3d_drop_hidden_row(d, row, H4);
        const f32x4* xr = reinterpret_cast<const f32x4*>(x) + (int64_t)row * H4;
        f32x4* orow = reinterpret_cast<f32x4*>(out) + (int64_t)row * H4;
        for (int g = lane; g < H4; g += 64) {
            float m[4];
            e3d_drop_mult4_row(d, rt, (uint32_t)g, m);
            f32x4 v = xr[g];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] *= m[j];
            orow[g] = v;
        }
    }
}

// multipliers of the attention-probability dropout, [B*nh, Lq, Lk] (test aid: the kernels never store them)
__global__ __launch_bounds__(256) void attn_drop_mask_kernel(E3dDrop d_in, float* __restrict__ out, int nh, int Lq, int Lk,
                                                             int64_t n_rows) {
    const E3dDrop d = e3d_drop_resolve(d_in);
    const int64_t row = blockIdx.x;   // (bh, q)
    if (row >= n_rows) return;
    const int bh = (int)(row / Lq), q = (int)(row % Lq);
    const uint64_t rt = e3d_drop_attn_row(d, bh / nh, bh % nh, nh, Lq, Lk, q);
    for (int key0 = 4 * threadIdx.x; key0 < Lk; key0 += 4 * blockDim.x) {
        float m[4];
        e3d_drop_mult4_row(d, rt, (uint32_t)(key0 >> 2), m);
        for (int j = 0; j < 4 && key0 + j < Lk; ++j) out[row * Lk + key0 + j] = m[j];
    }
}

// The key of frame row r = b * L + l: words 0 and 1 of (seed, ids[b], stream, epoch, l, block 0) -- e3d_philox.h
__global__ __launch_bounds__(256) void keyed_drop_row_keys_kernel(const int64_t* __restrict__ ids, int L,
                                                                  const int64_t* __restrict__ epoch_word, uint64_t seed,
                                                                  int stream, uint64_t* __restrict__ out, int64_t rows) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const E3dU32x4 w = e3d_keyed_words(seed, (uint64_t)ids[r / L], stream, (uint32_t)*epoch_word & 0xFFFFu, (uint32_t)(r % L), 0);
    out[r] = (uint64_t)w.w[0] | (uint64_t)w.w[1] << 32;
}

}  // namespace

extern "C" int e3d_dropout_f32(const float* x, float p, uint64_t seed, float* out, int64_t n, void* stream) {
    E3D_REQUIRE(x && out && n > 0, "dropout: bad arguments");
    E3D_REQUIRE(p >= 0.f && p < 1.f, "dropout: p=%g outside [0, 1)", (double)p);
    E3D_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0, "dropout: pointers must be 16B aligned");
    int64_t blocks = ((n >> 2) + 1 + 255) / 256;
    blocks = blocks > 8192 ? 8192 : blocks;
    hipLaunchKernelGGL(dropout_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, e3d_drop_make(p, seed),
                       out, n);
    return e3d_launch_status("e3d_dropout_f32");
}

extern "C" int e3d_attn_dropout_mask(int B, int nh, int Lq, int Lk, float p, uint64_t seed, float* out, void* stream) {
    E3D_REQUIRE(out && B > 0 && nh > 0 && Lq > 0 && Lk > 0, "attn_dropout_mask: bad arguments");
    E3D_REQUIRE(p >= 0.f && p < 1.f, "attn_dropout_mask: p=%g outside [0, 1)", (double)p);
    const int64_t rows = (int64_t)B * nh * Lq;
    E3D_REQUIRE(rows < (1ll << 31), "attn_dropout_mask: too many rows");
    hipLaunchKernelGGL(attn_drop_mask_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, e3d_drop_make(p, seed),
                       out, nh, Lq, Lk, rows);
    return e3d_launch_status("e3d_attn_dropout_mask");
}

// ---------------------------------------------------------------- keyed decisions ("Keyed sampling streams")
extern "C" int e3d_keyed_drop_row_keys(const int64_t* ids, int B, int L, const int64_t* epoch_word, uint64_t seed, int stream,
                                       uint64_t* out, void* st) {
    E3D_REQUIRE(ids && epoch_word && out && B > 0 && L > 0, "keyed_drop_row_keys: bad arguments");
    E3D_REQUIRE(L <= (1 << 24), "keyed_drop_row_keys: positions must stay below 2^24 (L=%d)", L);
    E3D_REQUIRE(stream == E3D_DROP_STREAM_LIGAND || stream == E3D_DROP_STREAM_POCKET, "keyed_drop_row_keys: stream %d", stream);
    const int64_t rows = (int64_t)B * L;
    E3D_REQUIRE(rows < (1ll << 31), "keyed_drop_row_keys: too many rows");
    hipLaunchKernelGGL(keyed_drop_row_keys_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)st, ids, L,
                       epoch_word, seed, stream, out, rows);
    return e3d_launch_status("e3d_keyed_drop_row_keys");
}

extern "C" int e3d_dropout_f32_keyed(const float* x, float p, uint32_t site, const uint64_t* row_keys, float* out, int M, int H,
                                     void* stream) {
    E3D_REQUIRE(x && out && row_keys && M > 0 && H > 0 && H % 4 == 0, "dropout_keyed: bad arguments (M=%d, H=%d)", M, H);
    E3D_REQUIRE(p >= 0.f && p < 1.f, "dropout_keyed: p=%g outside [0, 1)", (double)p);
    E3D_REQUIRE(site < E3D_DROP_MAX_SITE, "dropout_keyed: site %u does not fit 24 bits", site);
    E3D_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0, "dropout_keyed: pointers must be 16B aligned");
    const int blocks = (M + 3) / 4 < 8192 ? (M + 3) / 4 : 8192;
    hipLaunchKernelGGL(dropout_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x,
                       e3d_drop_make_keyed(p, site, row_keys), out, M, H / 4);
    return e3d_launch_status("e3d_dropout_f32_keyed");
}

// ``row_keys``: the table of the [B, Lq] QUERY frame
extern "C" int e3d_keyed_attn_dropout_mask(int B, int nh, int Lq, int Lk, float p, uint32_t site, const uint64_t* row_keys,
                                           float* out, void* stream) {
    E3D_REQUIRE(out && row_keys && B > 0 && nh > 0 && Lq > 0 && Lk > 0, "keyed_attn_dropout_mask: bad arguments");
    E3D_REQUIRE(p >= 0.f && p < 1.f, "keyed_attn_dropout_mask: p=%g outside [0, 1)", (double)p);
    E3D_REQUIRE(site < E3D_DROP_MAX_SITE && nh < E3D_DROP_MAX_HEADS, "keyed_attn_dropout_mask: site %u / %d heads out of range",
                site, nh);
    const int64_t rows = (int64_t)B * nh * Lq;
    E3D_REQUIRE(rows < (1ll << 31), "keyed_attn_dropout_mask: too many rows");
    hipLaunchKernelGGL(attn_drop_mask_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream,
                       e3d_drop_make_keyed(p, site, row_keys), out, nh, Lq, Lk, rows);
    return e3d_launch_status("e3d_keyed_attn_dropout_mask");
}
