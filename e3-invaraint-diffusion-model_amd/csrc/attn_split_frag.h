// Split-operand MFMA helpers shared by the per-wave attention forward kernels (attn_relkey_split.hip,
// attn_varlen.hip): fp32 -> 2 / 3 bf16 (or 2 fp16) term splits, 32x64 operand tiles staged through a
// per-wave LDS buffer, the V gather in PV-operand order and the cross-term MFMA sums.
#pragma once
#include "e3d_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
// element type of the split terms: __bf16 (bf16x3 / bf16x6) or _Float16 (f16x3, NS = 2 only; include/e3d_hip.h)
template <typename E> struct AV;
template <> struct AV<__bf16> { typedef bf16x8 x8; };
template <> struct AV<_Float16> { typedef f16x8 x8; };
template <typename X> struct Elem;
template <> struct Elem<bf16x8> { typedef __bf16 type; };
template <> struct Elem<f16x8> { typedef _Float16 type; };
__device__ __forceinline__ f32x16 mma16(const bf16x8 a, const bf16x8 b, const f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mma16(const f16x8 a, const f16x8 b, const f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

constexpr int D = 64;
constexpr int RING_LD = 34;
constexpr int RING_F = 64 * RING_LD;
constexpr int STG_LD = 68;             // staging rows: 64 floats + 16 B pad (conflict-free b128 fragment reads)
constexpr int STG_F = 32 * STG_LD;
constexpr int WAVE_LDS_F = RING_F + STG_F + 32;  // + per-tile key bias row

template <int NS, typename X8>
__device__ __forceinline__ void split8(const float (&x)[8], X8 (&parts)[NS]) {
    typedef typename Elem<X8>::type E;
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = x[j];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const E p = (E)r[j];
            parts[s][j] = p;
            r[j] -= (float)p;
        }
}

template <int NS>
__device__ __forceinline__ void split8(const float (&x)[8], f16x8 (&parts)[NS]) {
    static_assert(NS == 2, "fp16 terms exist as the two-term split only");
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        e3d_f16x2 h, l;
        e3d_split2_f16(x[j], x[j + 1], h, l);
        parts[0][j] = h[0]; parts[0][j + 1] = h[1];
        parts[1][j] = l[0]; parts[1][j + 1] = l[1];
    }
}

// one row's 64 head-dim values -> 4 k-blocks x NS parts (lane takes floats 16kb + 8h .. +7)
template <int NS, typename X8>
__device__ __forceinline__ void load_row_split(X8 (&f)[4][NS], const float* row_ptr, int half) {
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(row_ptr + 16 * kb + 8 * half);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(row_ptr + 16 * kb + 8 * half + 4);
        const float x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        split8<NS>(x, f[kb]);
    }
}

// A 32-row x 64-float operand tile (rows row_lo .. row_lo+31 clamped to [row_min,row_max], row stride rs)
// -> MFMA fragments.  Fragment-shaped global loads (16 B per lane from 32 different rows) are
// address-coalescer bound, so the wave loads the tile in full 256-byte rows (4 rows per
// instruction), parks it in its private LDS staging buffer and reads the fragments back.
struct TileRegs { f32x4 v[8]; };

// ``base`` is wave-uniform (scalar registers); lane offsets stay 32-bit (one (b,h) slab is < 2^31 elements)
__device__ __forceinline__ void tile_load(TileRegs& t, const float* base, int rs, int row_lo, int row_min,
                                          int row_max, int lane) {
    if (row_lo >= row_min && row_lo + 31 <= row_max) {  // wave-uniform: one lane offset + scalar row steps
        const unsigned off = (unsigned)((row_lo + (lane >> 4)) * rs + 4 * (lane & 15));
#pragma unroll
        for (int i = 0; i < 8; ++i) t.v[i] = *reinterpret_cast<const f32x4*>(base + (off + (unsigned)(4 * i * rs)));
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = min(max(row_lo + 4 * i + (lane >> 4), row_min), row_max);
            t.v[i] = *reinterpret_cast<const f32x4*>(base + (unsigned)(row * rs + 4 * (lane & 15)));
        }
    }
}

template <int NS, typename X8>
__device__ __forceinline__ void tile_to_frags(X8 (&f)[4][NS], const TileRegs& t, float* stg, int lane) {
    __builtin_amdgcn_wave_barrier();  // earlier readers of the staging buffer are done (in-order LDS)
#pragma unroll
    for (int i = 0; i < 8; ++i)
        *reinterpret_cast<f32x4*>(stg + (4 * i + (lane >> 4)) * STG_LD + 4 * (lane & 15)) = t.v[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const float* row = stg + (lane & 31) * STG_LD + 8 * (lane >> 5);
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(row + 16 * kb);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(row + 16 * kb + 4);
        const float x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        split8<NS>(x, f[kb]);
    }
}

// exp(x) for x <= 0 via the hardware exp2 (v_exp_f32): relative error <= ~2e-6 for x in [-20, 0],
// results below 2^-126 flush to zero (harmless in a softmax numerator).
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

struct VRegs { float2 v[16]; };

// V rows in PV-operand order: entry 8*st + j is key row rho(st,half,j), head dims 2c, 2c+1
__device__ __forceinline__ void v_load(VRegs& t, const float* vb, int v_rs, int r0, int Lk, int c, int half) {
    if (r0 + 32 <= Lk) {  // wave-uniform fast path
        const unsigned off = (unsigned)((r0 + 4 * half) * v_rs + 2 * c);
#pragma unroll
        for (int i = 0; i < 16; ++i)
            t.v[i] = *reinterpret_cast<const float2*>(vb + (off + (unsigned)(((i & 3) + 8 * (i >> 2)) * v_rs)));
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = min(r0 + mfma32_row(i, half), Lk - 1);
            t.v[i] = *reinterpret_cast<const float2*>(vb + (unsigned)(key * v_rs + 2 * c));
        }
    }
}

// acc += sum over the significant cross terms of a (A operand parts) x b (B operand parts)
template <int NS, typename X8>
__device__ __forceinline__ f32x16 mfma_terms(const X8 (&a)[NS], const X8 (&b)[NS], f32x16 acc) {
    if (NS == 3) {
        acc = mma16(a[1], b[1], acc);
        acc = mma16(a[0], b[NS - 1], acc);
        acc = mma16(a[NS - 1], b[0], acc);
    }
    acc = mma16(a[0], b[1], acc);
    acc = mma16(a[1], b[0], acc);
    acc = mma16(a[0], b[0], acc);
    return acc;
}

// tile[i][j] = X_i . Y_j (i on accumulator rows, j on lanes)
template <int NS, typename X8>
__device__ __forceinline__ f32x16 dot_tile(const X8 (&x)[4][NS], const X8 (&y)[4][NS]) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) acc = mfma_terms<NS>(x[kb], y[kb], acc);
    return acc;
}

}  // namespace
