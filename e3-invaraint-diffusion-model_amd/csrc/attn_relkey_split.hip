// Fused relative-key attention forward on the bf16 matrix cores with SPLIT fp32 operands and fp32
// accumulation -- same algorithm, layouts and LDS ring as attn_relkey.hip (query on the MFMA lane,
// key on the accumulator rows, online softmax in fp32 registers), but every product
//     S^T = K Q^T,   T^T = E Q^T (rel-key),   O^T += V^T P^T
// runs as 3 (TERMS=3: operands split in 2 bf16 terms) or 6 (TERMS=6: 3 terms, fp32-grade) cross
// products of v_mfma_f32_32x32x16_bf16: 36 / 72 MFMA issue slots of 32 cycles per 32x32 score tile
// instead of 96 slots of 64 cycles for the exact fp32 MFMA kernel.
//
// Operand maps (32x32x16: lane (r = lane&31, h = lane>>5) holds k = 8h + j, j = 0..7):
//   K / E / Q rows: 8 consecutive head-dim floats (2 x 16 B loads) per 16-wide k block;
//   P^T as the B operand of PV: accumulator registers 8s..8s+7 of the score tile, i.e. key row
//     rho(s,h,j) = (j&3) + 8(2s + (j>>2)) + 4h, so V^T is gathered with the same permutation
//     (8 x 8-byte loads of V[r0 + rho][2c .. 2c+1] per step; the lane owns head dims 2c, 2c+1).
#include "attn_split_frag.h"

namespace {

template <int NS, bool RELKEY, bool DROP, typename E>
__global__ __launch_bounds__(256, 2) void attn_fwd_split_kernel(
    const float* __restrict__ q, int64_t q_bs, int64_t q_rs, const float* __restrict__ k, int64_t k_bs,
    int64_t k_rs, const float* __restrict__ v, int64_t v_bs, int64_t v_rs, const float* __restrict__ dist_emb,
    int P, const float* __restrict__ key_mask, float* __restrict__ out, float* __restrict__ lse, int nh, int Lq,
    int Lk, int q_tiles, int n_units, int skip_padded_tiles, E3dBounds bnd, E3dDrop drop_in) {
    const E3dDrop drop = e3d_drop_resolve(drop_in);   // + the device-side epoch (graph replays: e3d_common.h)
    typedef typename AV<E>::x8 bf16x8;   // (name kept from the bf16 form: 8 split terms of type E)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int qi = lane & 31, half = lane >> 5;
    const int unit = xcd_remap(blockIdx.x, gridDim.x) * (blockDim.x >> 6) + wid;
    if (unit >= n_units) return;
    const int qt = unit % q_tiles, bh = unit / q_tiles, h = bh % nh, b = bh / nh;
    float* ring = smem + wid * WAVE_LDS_F;
    float* stg = ring + RING_F;
    float* kbias = stg + STG_F;

    const int q0 = qt * 32;
    const int lq = min(q0 + qi, Lq - 1);
    uint64_t drop_row = 0;   // dropout: this query row's part of the hash input (its key, when the decisions are keyed)
    if (DROP) drop_row = e3d_drop_attn_row(drop, b, h, nh, Lq, Lk, lq);
    bf16x8 qf[4][NS];
    load_row_split<NS>(qf, q + b * q_bs + (int64_t)lq * q_rs + h * D, half);

    const float* kb_ = k + b * k_bs + h * D;
    const float* vb = v + b * v_bs + h * D;
    const float* mb = key_mask ? key_mask + (int64_t)b * Lk : nullptr;

    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;

    int rot = 0;
    if (RELKEY) {
        TileRegs ereg;
        tile_load(ereg, dist_emb, D, q0 + 1 + P - 1, 0, 2 * P - 2, lane);
        bf16x8 ef[4][NS];
        tile_to_frags<NS>(ef, ereg, stg, lane);
        const f32x16 t = dot_tile<NS>(ef, qf);
#pragma unroll
        for (int r = 0; r < 16; ++r) ring[(32 + mfma32_row(r, half)) * RING_LD + qi] = t[r];
    }

    // Trailing key tiles that are padding in every position contribute exp(s - 10000 - m) == 0.0f exactly
    // (fp32 underflow) AS LONG AS the scores of a row spread over less than ~9900 -- the reference's mask is additive
    // (structure_model/model.py:226-231), so with |q|, |k| in the thousands a padded key does reach the softmax, and
    // skipping it would be wrong (found at 0.47 max-norm in the weights-x4 regime of the margin test).  The sweep stops
    // after the tile of the last valid key only when the caller's element bounds prove the spread small
    // (e3d_mask_skip_is_exact); the result is then bit-identical to the full sweep.  An all-padding item (no valid key)
    // keeps the full sweep, as the reference then softmaxes the uniformly shifted scores.
    int k_tiles = (Lk + 31) >> 5;
    if (mb && skip_padded_tiles && e3d_mask_skip_is_exact(bnd)) {
        int last = -1;
        for (int base = 0; base < Lk; base += 64) {
            const int key = base + lane;
            const bool valid = key < Lk && mb[key] != 0.f;
            const unsigned long long bits = __ballot(valid);
            if (bits) last = base + 63 - __builtin_clzll(bits);
        }
        if (last >= 0) k_tiles = (last >> 5) + 1;
    }
    for (int kt = 0; kt < k_tiles; ++kt) {
        const int r0 = kt * 32;
        TileRegs kreg, ereg;
        VRegs vreg;
        tile_load(kreg, kb_, (int)k_rs, r0, 0, Lk - 1, lane);
        if (RELKEY) tile_load(ereg, dist_emb, D, q0 - r0 - 31 + P - 1, 0, 2 * P - 2, lane);
        {   // additive key bias of this tile: one coalesced load, shared through LDS
            const int key = r0 + qi;
            float bias = -INFINITY;
            if (key < Lk) bias = mb ? (1.0f - mb[key]) * -10000.0f : 0.f;
            if (half == 0) kbias[qi] = bias;
        }
        f32x16 s;
        {
            bf16x8 kf[4][NS];
            tile_to_frags<NS>(kf, kreg, stg, lane);
            s = dot_tile<NS>(kf, qf);
        }
        if (RELKEY) {
            bf16x8 ef[4][NS];
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
        const float m_new = fmaxf(m_run, tmax);
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
        if (DROP) {   // dropout on the probabilities: the row sum above stays un-dropped (softmax first, then dropout)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float m[4];
                e3d_drop_mult4_row(drop, drop_row, (uint32_t)((r0 >> 2) + 2 * g + half), m);
#pragma unroll
                for (int j = 0; j < 4; ++j) s[4 * g + j] *= m[j];
            }
        }

        // O^T += V^T P^T, two 16-key steps; P^T registers 8st..8st+7 are the B operand
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            float pv[8], v0[8], v1[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                pv[j] = s[8 * st + j];
                v0[j] = vreg.v[8 * st + j].x;
                v1[j] = vreg.v[8 * st + j].y;
            }
            bf16x8 pb[NS], a0[NS], a1[NS];
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
        float* orow = out + ((int64_t)b * Lq + q0 + qi) * (nh * D) + h * D;
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
        if (lse && half == 0) lse[((int64_t)b * nh + h) * Lq + q0 + qi] = m_run + logf(l_tot);
    }
}

int g_skip_padded = 1;

template <int NS, bool DROP = false, typename E = __bf16>
int launch(const E3dAttnFwd& a, E3dBounds bnd, hipStream_t s, E3dDrop drop = E3dDrop{0, 0, 1.f}) {
    const int q_tiles = (a.Lq + 31) / 32;
    const int n_units = a.B * a.nh * q_tiles;
    const int wpb = 4;
    const int n_blocks = (n_units + wpb - 1) / wpb;
    const size_t lds = (size_t)wpb * WAVE_LDS_F * sizeof(float);
    if (a.dist_emb)
        hipLaunchKernelGGL((attn_fwd_split_kernel<NS, true, DROP, E>), dim3(n_blocks), dim3(64 * wpb), lds, s, E3D_VIEW(a.q),
                           E3D_VIEW(a.k), E3D_VIEW(a.v), a.dist_emb, a.P, a.key_mask, a.out, a.lse, a.nh, a.Lq, a.Lk, q_tiles,
                           n_units, g_skip_padded, bnd, drop);
    else
        hipLaunchKernelGGL((attn_fwd_split_kernel<NS, false, DROP, E>), dim3(n_blocks), dim3(64 * wpb), lds, s, E3D_VIEW(a.q),
                           E3D_VIEW(a.k), E3D_VIEW(a.v), a.dist_emb, a.P, a.key_mask, a.out, a.lse, a.nh, a.Lq, a.Lk, q_tiles,
                           n_units, g_skip_padded, bnd, drop);
    return e3d_launch_status("e3d_relkey_attn_fwd_split");
}

}  // namespace

extern "C" int e3d_attn_skip_padded_tiles(int enable) {
    const int prev = g_skip_padded;
    g_skip_padded = enable ? 1 : 0;
    return prev;
}

// whether a call of these strides and lengths lands on the 4-wave cooperative kernel (the one form with a plane output)
static bool attn_coop_ok(int64_t k_rs, int64_t v_bs, int64_t v_rs, int Lq, int Lk, int terms, bool dropping, bool have_scratch) {
    static int coop = -1;   // E3D_ATTN_COOP=0: per-wave kernel below for every shape (A/B experiments)
    if (coop < 0) {
        const char* e = getenv("E3D_ATTN_COOP");
        coop = e ? atoi(e) : 1;
    }
    // two-wave groups (q_tiles % 4 != 0) measured slower than the per-wave kernel: too little sharing per barrier
    // the cooperative kernel reads the distance table as fragment-order bf16 planes from a CALLER-provided scratch
    // (e3d_attn_scratch_bytes); without one the per-wave kernel below serves the call -- the library never allocates.
    // With dropout (training) the cooperative kernel exists in bf16x3.
    // (its staging goes through buffer descriptors of one key tile's rows: 32-bit byte offsets and record counts, i.e. an
    //  item's K / V rows must span less than 2 GiB -- Lk x row stride x 4 bytes; the per-wave kernel serves anything wider)
    const bool span_ok = (int64_t)Lk * (k_rs > v_rs ? k_rs : v_rs) * 4 < ((int64_t)1 << 31) && k_rs > 0 && v_rs > 0 &&
                         k_rs < ((int64_t)1 << 24) && v_rs < ((int64_t)1 << 24);     // (a tile's 32 rows in a 32-bit offset)
    return (terms == 3 || (terms == E3D_TERMS_F16X3 && !dropping)) && coop && span_ok && v_rs % 4 == 0 && v_bs % 4 == 0 &&
           ((Lq + 31) / 32) % 4 == 0 && have_scratch;
}

// the body of e3d_relkey_attn_fwd_split_ex and of its keyed form; ``planes_out``: ``a.out`` receives activation planes
// (e3d_relkey_attn_fwd_split_planes)
static int attn_fwd_dispatch(const E3dAttnFwd& a, int terms, const E3dAttnDrop& drop, void* e_scratch, int e_scratch_ready,
                             const float* q_absmax, const float* k_absmax, float* e_absmax, void* stream,
                             bool planes_out = false) {
    const E3dBounds bnd{q_absmax, k_absmax, a.dist_emb ? e_absmax : nullptr};
    E3D_REQUIRE(!a.dist_emb || !q_absmax || e_absmax, "attn_split: rel-key attention with element bounds needs e_absmax too");
    E3D_REQUIRE(drop.p >= 0.f && drop.p < 1.f, "attn_split: drop_p=%g outside [0, 1)", (double)drop.p);
    E3D_REQUIRE(a.q.p && a.k.p && a.v.p && a.out, "attn_split: null pointer");
    E3D_REQUIRE(a.B > 0 && a.nh > 0 && a.Lq > 0 && a.Lk > 0, "attn_split: bad shape B=%d nh=%d Lq=%d Lk=%d", a.B, a.nh, a.Lq,
                a.Lk);
    E3D_REQUIRE(a.q.rs % 4 == 0 && a.k.rs % 4 == 0 && a.v.rs % 2 == 0 && a.q.bs % 4 == 0 && a.k.bs % 4 == 0 && a.v.bs % 2 == 0,
                "attn_split: strides must keep 16B (q,k) / 8B (v) alignment");
    E3D_REQUIRE(((uintptr_t)a.q.p % 16) == 0 && ((uintptr_t)a.k.p % 16) == 0 && ((uintptr_t)a.v.p % 16) == 0 &&
                    ((uintptr_t)a.out % 16) == 0, "attn_split: pointers must be 16B aligned");
    E3D_REQUIRE(terms == 3 || terms == 6 || terms == E3D_TERMS_F16X3, "attn_split: terms must be 3, 6 or 19 (got %d)", terms);
    const int f16 = terms == E3D_TERMS_F16X3;
    E3D_REQUIRE((int64_t)a.Lk * a.k.rs < (1ll << 30) && (int64_t)a.Lk * a.v.rs < (1ll << 30),
                "attn_split: one batch item's K/V slab must stay below 2^30 elements (32-bit lane offsets)");
    if (a.dist_emb) {
        E3D_REQUIRE(a.Lq == a.Lk && a.Lq <= a.P, "attn_split: relative_key needs Lq == Lk <= P (Lq=%d Lk=%d P=%d)", a.Lq, a.Lk,
                    a.P);
        E3D_REQUIRE(((uintptr_t)a.dist_emb % 16) == 0, "attn_split: dist_emb must be 16B aligned");
    }
    E3D_REQUIRE((int64_t)a.B * a.nh * ((a.Lq + 31) / 32) < (1ll << 30), "attn_split: too many tiles");
    hipStream_t s = (hipStream_t)stream;
    if (a.dist_emb && e_scratch && !e_scratch_ready) {
        // whichever kernel serves this call, a scratch handed in is valid afterwards (callers cache it)
        const int rc = e3d_attn_fill_planes(a.dist_emb, a.P, a.Lk, e_scratch, f16, e_absmax, s);   // (also raises *e_absmax)
        if (rc) return rc;
        e_scratch_ready = 1;
    }
    if (attn_coop_ok(a.k.rs, a.v.bs, a.v.rs, a.Lq, a.Lk, terms, drop.on(), !a.dist_emb || e_scratch))
        return e3d_attn_coop_launch(a, g_skip_padded, bnd, e_scratch, e_scratch_ready, f16, drop, planes_out, s);
    E3D_REQUIRE(!planes_out, "attn_split: plane output needs the cooperative kernel (e3d_attn_planes_supported)");
    if (drop.on())   // training with attention-probability dropout, other shapes / arithmetics: per-wave kernel
        return terms == 3 ? launch<2, true>(a, bnd, s, drop.d) : launch<3, true>(a, bnd, s, drop.d);
    if (f16) return launch<2, false, _Float16>(a, bnd, s);
    return terms == 3 ? launch<2>(a, bnd, s) : launch<3>(a, bnd, s);
}

extern "C" int e3d_relkey_attn_fwd_split_ex(const float* q, int64_t q_bs, int64_t q_rs, const float* k, int64_t k_bs,
                                            int64_t k_rs, const float* v, int64_t v_bs, int64_t v_rs,
                                            const float* dist_emb, int P, const float* key_mask, float* out,
                                            float* lse, int B, int nh, int Lq, int Lk, int terms, float drop_p,
                                            uint64_t drop_seed, void* e_scratch, int e_scratch_ready, const float* q_absmax,
                                            const float* k_absmax, float* e_absmax, void* stream) {
    return attn_fwd_dispatch({{q, q_bs, q_rs}, {k, k_bs, k_rs}, {v, v_bs, v_rs}, dist_emb, P, key_mask, out, lse, B, nh, Lq, Lk},
                             terms, {drop_p, e3d_drop_make(drop_p, drop_seed)}, e_scratch, e_scratch_ready, q_absmax, k_absmax,
                             e_absmax, stream);
}

// As e3d_relkey_attn_fwd_split_ex with keyed dropout decisions (drop_p > 0): ``row_keys`` uint64 [B * Lq], the table of the
// QUERY frame (e3d_keyed_drop_row_keys); ``site`` < 2^24, nh < 2^16
extern "C" int e3d_relkey_attn_fwd_split_ex_keyed(const float* q, int64_t q_bs, int64_t q_rs, const float* k, int64_t k_bs,
                                                  int64_t k_rs, const float* v, int64_t v_bs, int64_t v_rs,
                                                  const float* dist_emb, int P, const float* key_mask, float* out,
                                                  float* lse, int B, int nh, int Lq, int Lk, int terms, float drop_p,
                                                  uint32_t site, const uint64_t* row_keys, void* e_scratch, int e_scratch_ready,
                                                  const float* q_absmax, const float* k_absmax, float* e_absmax, void* stream) {
    E3D_REQUIRE(row_keys && drop_p > 0.f, "attn_split (keyed): row keys and drop_p > 0 required");
    E3D_REQUIRE(site < E3D_DROP_MAX_SITE && nh < E3D_DROP_MAX_HEADS, "attn_split (keyed): site %u / %d heads out of range", site, nh);
    return attn_fwd_dispatch({{q, q_bs, q_rs}, {k, k_bs, k_rs}, {v, v_bs, v_rs}, dist_emb, P, key_mask, out, lse, B, nh, Lq, Lk},
                             terms, {drop_p, e3d_drop_make_keyed(drop_p, site, row_keys)}, e_scratch, e_scratch_ready, q_absmax,
                             k_absmax, e_absmax, stream);
}

extern "C" int e3d_relkey_attn_fwd_split(const float* q, int64_t q_bs, int64_t q_rs, const float* k, int64_t k_bs,
                                         int64_t k_rs, const float* v, int64_t v_bs, int64_t v_rs,
                                         const float* dist_emb, int P, const float* key_mask, float* out, float* lse,
                                         int B, int nh, int Lq, int Lk, int terms, void* stream) {
    return e3d_relkey_attn_fwd_split_ex(q, q_bs, q_rs, k, k_bs, k_rs, v, v_bs, v_rs, dist_emb, P, key_mask, out, lse, B,
                                        nh, Lq, Lk, terms, 0.f, 0, nullptr, 0, nullptr, nullptr, nullptr, stream);
}

extern "C" int e3d_relkey_attn_fwd_split_drop(const float* q, int64_t q_bs, int64_t q_rs, const float* k, int64_t k_bs,
                                              int64_t k_rs, const float* v, int64_t v_bs, int64_t v_rs,
                                              const float* dist_emb, int P, const float* key_mask, float* out,
                                              float* lse, int B, int nh, int Lq, int Lk, int terms, float drop_p,
                                              uint64_t drop_seed, void* stream) {
    return e3d_relkey_attn_fwd_split_ex(q, q_bs, q_rs, k, k_bs, k_rs, v, v_bs, v_rs, dist_emb, P, key_mask, out, lse, B,
                                        nh, Lq, Lk, terms, drop_p, drop_seed, nullptr, 0, nullptr, nullptr, nullptr, stream);
}

extern "C" int e3d_relkey_attn_fwd_split_drop_keyed(const float* q, int64_t q_bs, int64_t q_rs, const float* k, int64_t k_bs,
                                                    int64_t k_rs, const float* v, int64_t v_bs, int64_t v_rs,
                                                    const float* dist_emb, int P, const float* key_mask, float* out,
                                                    float* lse, int B, int nh, int Lq, int Lk, int terms, float drop_p,
                                                    uint32_t site, const uint64_t* row_keys, void* stream) {
    return e3d_relkey_attn_fwd_split_ex_keyed(q, q_bs, q_rs, k, k_bs, k_rs, v, v_bs, v_rs, dist_emb, P, key_mask, out, lse, B,
                                              nh, Lq, Lk, terms, drop_p, site, row_keys, nullptr, 0, nullptr, nullptr, nullptr,
                                              stream);
}

// Plane output (inference): the context leaves as ACTIVATION PLANES of the [B * Lq, nh * 64] matrix (e3d_activation_planes_f32_split's
// format, bit for bit the split of what e3d_relkey_attn_fwd_split_ex stores), for e3d_gemm_residual_layernorm_planes_split.
// Exists where the 4-wave cooperative kernel serves the call: e3d_attn_planes_supported says so beforehand, anything else is an error.
extern "C" int e3d_attn_planes_supported(int64_t k_rs, int64_t v_bs, int64_t v_rs, int Lq, int Lk, int terms, int have_scratch) {
    return (terms == 3 || terms == E3D_TERMS_F16X3) && Lq > 0 && Lq % 32 == 0 && Lk > 0 &&
           attn_coop_ok(k_rs, v_bs, v_rs, Lq, Lk, terms, false, have_scratch != 0) && e3d_attn_coop_waves(Lq) == 4;
}

extern "C" int e3d_relkey_attn_fwd_split_planes(const float* q, int64_t q_bs, int64_t q_rs, const float* k, int64_t k_bs,
                                                int64_t k_rs, const float* v, int64_t v_bs, int64_t v_rs,
                                                const float* dist_emb, int P, const float* key_mask, void* out_planes,
                                                int B, int nh, int Lq, int Lk, int terms, void* e_scratch, int e_scratch_ready,
                                                const float* q_absmax, const float* k_absmax, float* e_absmax, void* stream) {
    E3D_REQUIRE(e3d_attn_planes_supported(k_rs, v_bs, v_rs, Lq, Lk, terms, !dist_emb || e_scratch),
                "attn_split (planes): this call does not land on the 4-wave cooperative kernel (Lq=%d Lk=%d terms=%d)", Lq, Lk, terms);
    return attn_fwd_dispatch({{q, q_bs, q_rs}, {k, k_bs, k_rs}, {v, v_bs, v_rs}, dist_emb, P, key_mask,
                              reinterpret_cast<float*>(out_planes), nullptr, B, nh, Lq, Lk},
                             terms, {0.f, e3d_drop_make(0.f, 0)}, e_scratch, e_scratch_ready, q_absmax, k_absmax, e_absmax, stream,
                             true);
}
