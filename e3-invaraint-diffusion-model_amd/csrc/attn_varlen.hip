// Fused attention forward over variable-length SEGMENTS (packed batches, inference): the per-wave split kernel of
// attn_relkey_split.hip -- same operand maps, LDS ring, split arithmetic and online softmax -- with the batch index
// replaced by a segment table.  Segment s owns query rows q_start[s] .. q_start[s] + q_len[s] - 1 and key / value rows
// k_start[s] .. k_start[s] + k_len[s] - 1 of row-strided buffers; positions (the rel-key term, the key tiles) are
// measured from the segment start, so a segment computes what e3d_relkey_attn_fwd_split computes on one item of
// Lq = q_len[s], Lk = k_len[s] with no key mask.
//
// Work comes from a tile table built once per layout: entry i = (segment, q0) for a 32-query tile of that segment, or
// (-1, row0) for a 32-row block of the packed buffer's tail (rows that belong to no segment), which the wave zeroes.
// One wave takes one (entry, head): no idle waves for short segments, no grid sized by the longest one.
//
// Keys past k_len[s] are clamped to the segment's last row when loaded (no other segment's rows are read) and carry a
// -inf bias, i.e. exp() weight 0 -- they do not exist for the row.  Inside one segment lane offsets stay 32-bit (the
// host checks max(len) x row stride < 2^30); segment bases are 64-bit element offsets.
#include "attn_split_frag.h"

namespace {

template <int NS, bool RELKEY, typename E>
__global__ __launch_bounds__(256, 2) void attn_varlen_kernel(
    const float* __restrict__ q, int64_t q_rs, const float* __restrict__ k, int64_t k_rs, const float* __restrict__ v,
    int64_t v_rs, const int* __restrict__ q_start, const int* __restrict__ q_len, const int* __restrict__ k_start,
    const int* __restrict__ k_len, const int* __restrict__ tiles, int n_units, const float* __restrict__ dist_emb, int P,
    float* __restrict__ out, int64_t out_rows, int nh) {
    typedef typename AV<E>::x8 X8;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int qi = lane & 31, half = lane >> 5;
    const int unit = xcd_remap(blockIdx.x, gridDim.x) * (blockDim.x >> 6) + wid;
    if (unit >= n_units) return;
    // (entry, head), the heads of one entry on consecutive units
    const int h = unit % nh, entry = unit / nh;
    const int seg = tiles[2 * entry], q0 = tiles[2 * entry + 1];
    const int64_t ocol = (int64_t)nh * D;

    if (seg < 0) {   // tail block: rows q0 .. q0 + 31 (below out_rows) of no segment get zero output
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < 8; ++i) {
            const int64_t row = (int64_t)q0 + 4 * i + (lane >> 4);
            if (row < out_rows) *reinterpret_cast<f32x4*>(out + row * ocol + h * D + 4 * (lane & 15)) = z;
        }
        return;
    }
    const int Lq = q_len[seg], Lk = k_len[seg];
    const int64_t qs = q_start[seg];
    float* orow = out + (qs + q0 + qi) * ocol + h * D;
    if (Lk <= 0) {   // (packing.check_cross refuses such batches, the op does not: no row is read, the tile's rows are zero)
        if (q0 + qi < Lq)
            for (int c = 0; c < 64; c += 4) *reinterpret_cast<f32x4*>(orow + c) = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    float* ring = smem + wid * WAVE_LDS_F;
    float* stg = ring + RING_F;
    float* kbias = stg + STG_F;

    const int lq = min(q0 + qi, Lq - 1);
    X8 qf[4][NS];
    load_row_split<NS>(qf, q + (qs + lq) * q_rs + h * D, half);

    const int64_t ks = k_start[seg];
    const float* kb_ = k + ks * k_rs + h * D;
    const float* vb = v + ks * v_rs + h * D;

    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;

    int rot = 0;
    if (RELKEY) {
        TileRegs ereg;
        tile_load(ereg, dist_emb, D, q0 + 1 + P - 1, 0, 2 * P - 2, lane);
        X8 ef[4][NS];
        tile_to_frags<NS>(ef, ereg, stg, lane);
        const f32x16 t = dot_tile<NS>(ef, qf);
#pragma unroll
        for (int r = 0; r < 16; ++r) ring[(32 + mfma32_row(r, half)) * RING_LD + qi] = t[r];
    }

    const int k_tiles = (Lk + 31) >> 5;
    for (int kt = 0; kt < k_tiles; ++kt) {
        const int r0 = kt * 32;
        TileRegs kreg, ereg;
        VRegs vreg;
        tile_load(kreg, kb_, (int)k_rs, r0, 0, Lk - 1, lane);
        if (RELKEY) tile_load(ereg, dist_emb, D, q0 - r0 - 31 + P - 1, 0, 2 * P - 2, lane);
        if (half == 0) kbias[qi] = r0 + qi < Lk ? 0.f : -INFINITY;
        f32x16 s;
        {
            X8 kf[4][NS];
            tile_to_frags<NS>(kf, kreg, stg, lane);
            s = dot_tile<NS>(kf, qf);
        }
        if (RELKEY) {
            X8 ef[4][NS];
            tile_to_frags<NS>(ef, ereg, stg, lane);
            const f32x16 t = dot_tile<NS>(ef, qf);
#pragma unroll
            for (int r = 0; r < 16; ++r) ring[((mfma32_row(r, half) + rot) & 63) * RING_LD + qi] = t[r];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int x = qi - mfma32_row(r, half) + 31;
                s[r] += ring[((x + rot) & 63) * RING_LD + qi];
            }
            __builtin_amdgcn_wave_barrier();
            rot ^= 32;
        }

        v_load(vreg, vb, (int)v_rs, r0, Lk, qi, half);  // in flight under the softmax arithmetic
        float tmax = -INFINITY;
#pragma unroll
        for (int g = 0; g < 4; ++g) {  // rows 8g + 4*half + {0..3}: one 16-byte LDS read per group
            const f32x4 bv = *reinterpret_cast<const f32x4*>(kbias + 8 * g + 4 * half);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s[4 * g + j] = s[4 * g + j] * 0.125f + bv[j];
                tmax = fmaxf(tmax, s[4 * g + j]);
            }
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float m_new = fmaxf(m_run, tmax);   // finite: every tile holds key r0 < Lk
        const float alpha = fast_exp(m_run - m_new);
        m_run = m_new;
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = fast_exp(s[r] - m_new);
            psum += s[r];
        }
        l_run = l_run * alpha + psum;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }

#pragma unroll
        for (int st = 0; st < 2; ++st) {
            float pv[8], v0[8], v1[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                pv[j] = s[8 * st + j];
                v0[j] = vreg.v[8 * st + j].x;
                v1[j] = vreg.v[8 * st + j].y;
            }
            X8 pb[NS], a0[NS], a1[NS];
            split8<NS>(pv, pb);
            split8<NS>(v0, a0);
            split8<NS>(v1, a1);
            o0 = mfma_terms<NS>(a0, pb, o0);
            o1 = mfma_terms<NS>(a1, pb, o1);
        }
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    if (q0 + qi < Lq) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 lo, hi;
            lo[0] = o0[4 * g + 0] * inv; lo[1] = o1[4 * g + 0] * inv;
            lo[2] = o0[4 * g + 1] * inv; lo[3] = o1[4 * g + 1] * inv;
            hi[0] = o0[4 * g + 2] * inv; hi[1] = o1[4 * g + 2] * inv;
            hi[2] = o0[4 * g + 3] * inv; hi[3] = o1[4 * g + 3] * inv;
            *reinterpret_cast<f32x4*>(orow + 16 * g + 8 * half) = lo;
            *reinterpret_cast<f32x4*>(orow + 16 * g + 8 * half + 4) = hi;
        }
    }
}

template <int NS, typename E = __bf16>
int launch(const float* q, int64_t q_rs, const float* k, int64_t k_rs, const float* v, int64_t v_rs, const int* q_start,
           const int* q_len, const int* k_start, const int* k_len, const int* tiles, int n_tiles, const float* dist_emb,
           int P, float* out, int64_t out_rows, int nh, hipStream_t s) {
    const int n_units = n_tiles * nh;
    const int wpb = 4;
    const int n_blocks = (n_units + wpb - 1) / wpb;
    const size_t lds = (size_t)wpb * WAVE_LDS_F * sizeof(float);
    if (dist_emb)
        hipLaunchKernelGGL((attn_varlen_kernel<NS, true, E>), dim3(n_blocks), dim3(64 * wpb), lds, s, q, q_rs, k, k_rs, v,
                           v_rs, q_start, q_len, k_start, k_len, tiles, n_units, dist_emb, P, out, out_rows, nh);
    else
        hipLaunchKernelGGL((attn_varlen_kernel<NS, false, E>), dim3(n_blocks), dim3(64 * wpb), lds, s, q, q_rs, k, k_rs, v,
                           v_rs, q_start, q_len, k_start, k_len, tiles, n_units, dist_emb, P, out, out_rows, nh);
    return e3d_launch_status("e3d_attn_varlen_fwd");
}

}  // namespace

extern "C" int e3d_attn_varlen_fwd(const float* q, int64_t q_rs, const float* k, int64_t k_rs, const float* v,
                                   int64_t v_rs, const int* q_start, const int* q_len, const int* k_start,
                                   const int* k_len, const int* tiles, int n_tiles, const float* dist_emb, int P,
                                   float* out, int64_t out_rows, int nh, int max_q_len, int max_k_len, int terms,
                                   void* stream) {
    E3D_REQUIRE(q && k && v && out && q_start && q_len && k_start && k_len && tiles, "attn_varlen: null pointer");
    E3D_REQUIRE(nh > 0 && n_tiles > 0 && out_rows > 0 && max_q_len >= 0 && max_k_len >= 0,
                "attn_varlen: bad shape nh=%d n_tiles=%d out_rows=%lld", nh, n_tiles, (long long)out_rows);
    E3D_REQUIRE(q_rs % 4 == 0 && k_rs % 4 == 0 && v_rs % 2 == 0 && q_rs >= nh * 64 && k_rs >= nh * 64 && v_rs >= nh * 64,
                "attn_varlen: row strides must cover nh x 64 floats and keep 16B (q,k) / 8B (v) alignment");
    E3D_REQUIRE(((uintptr_t)q % 16) == 0 && ((uintptr_t)k % 16) == 0 && ((uintptr_t)v % 16) == 0 &&
                    ((uintptr_t)out % 16) == 0, "attn_varlen: pointers must be 16B aligned");
    E3D_REQUIRE(terms == 0 || terms == 3 || terms == 6 || terms == E3D_TERMS_F16X3,
                "attn_varlen: terms must be 0, 3, 6 or 19 (got %d)", terms);
    E3D_REQUIRE((int64_t)max_k_len * k_rs < (1ll << 30) && (int64_t)max_k_len * v_rs < (1ll << 30),
                "attn_varlen: one segment's K/V rows must span below 2^30 elements (32-bit lane offsets)");
    E3D_REQUIRE((int64_t)n_tiles * nh < (1ll << 30), "attn_varlen: too many tiles");
    if (dist_emb) {
        E3D_REQUIRE(max_q_len <= P && max_k_len <= P, "attn_varlen: relative_key needs segment lengths <= P (%d, %d, P=%d)",
                    max_q_len, max_k_len, P);
        E3D_REQUIRE(((uintptr_t)dist_emb % 16) == 0, "attn_varlen: dist_emb must be 16B aligned");
    }
    hipStream_t s = (hipStream_t)stream;
    if (terms == E3D_TERMS_F16X3)
        return launch<2, _Float16>(q, q_rs, k, k_rs, v, v_rs, q_start, q_len, k_start, k_len, tiles, n_tiles, dist_emb, P,
                                   out, out_rows, nh, s);
    if (terms == 3)
        return launch<2>(q, q_rs, k, k_rs, v, v_rs, q_start, q_len, k_start, k_len, tiles, n_tiles, dist_emb, P, out,
                         out_rows, nh, s);
    return launch<3>(q, q_rs, k, k_rs, v, v_rs, q_start, q_len, k_start, k_len, tiles, n_tiles, dist_emb, P, out,
                     out_rows, nh, s);   // bf16x6, and the fp32-grade form of terms 0 (f32)
}
