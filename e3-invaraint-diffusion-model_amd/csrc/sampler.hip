// Diffusion-process kernels: DDPM ancestral update + angular wrap, the strided (DDIM / respaced) update t -> s < t and
// its second-order multistep form, forward noising, the discrete (BLOSUM / uniform transition) posterior + categorical draw, the score terms of a
// supplied sequence under that posterior, and the score terms of supplied backbone angles under the DDPM update.  All
// HBM- or latency-bound.
// The keyed forms (seeded chains) generate their draws in-register from (seed, row key, step): e3d_philox.h.
#include "e3d_common.h"
#include "e3d_philox.h"
#include <initializer_list>

namespace {

// modulo_with_wrapped_range(v, -pi, pi): ((v - (-pi)) % 2pi) + (-pi) with torch's floored
// remainder (fmod, then +b when the sign differs); constants rounded to fp32 like torch does
// for python scalars.  (structure_model/utils.py:20-40)
__device__ __forceinline__ float wrap_pi(float v) {
    const float pi_f = 3.14159265358979323846f;
    const float top = 6.28318530717958647692f;
    const float sft = v + pi_f;
    float r = fmodf(sft, top);
    if (r != 0.f && r < 0.f) r += top;
    return r - pi_f;
}

// The step field of a training draw: the epoch word in device memory (a captured step replays it); 65535 = validation.
__device__ __forceinline__ uint32_t keyed_epoch(const int64_t* __restrict__ epoch_dev) {
    return (uint32_t)epoch_dev[0] & 0xFFFFu;
}

// ---------------------------------------------------------------- the draw source of the continuous updates
// The DDPM update, the strided update and the known compose each have one body; where the four N(0,1) draws of float4
// group i come from is the template parameter KEYED and this record, both chosen by the entry point:
//   buffer (KEYED false): a load from ``noise`` (may be null: the kernel then asks for no draws)
//   keyed  (KEYED true):  one Philox call on (seed, row key, stream, step, block) over a key table of rows x nb groups --
//                         one thread per (row, block j of 4 features) gets the 4 normals of features 4j .. 4j+3
// Same arithmetic per element either way, so a keyed launch equals the buffer form fed with the keyed normals.
struct Draws {
    const float* noise;
    const int64_t* row_keys;
    uint64_t seed;
    int stream, nb;
};

__device__ __forceinline__ bool keyed_row(const int64_t* __restrict__ row_keys, int64_t row, uint64_t& item,
                                          uint32_t& pos) {
    const int64_t p = row_keys[2 * row + 1];
    item = (uint64_t)row_keys[2 * row];
    pos = (uint32_t)p;
    return p >= 0;
}

// Does float4 group i belong to a row of an item (a buffer: always)?  ``want``: also fill z with the group's draws at ``step``.
template <bool KEYED>
__device__ __forceinline__ bool draws4(const Draws d, uint32_t step, int64_t i, bool want, float (&z)[4]) {
    if (!KEYED) {
        if (want) {
            const f32x4 v = reinterpret_cast<const f32x4*>(d.noise)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = v[j];
        }
        return true;
    }
    const int64_t row = i / d.nb;
    uint64_t item;
    uint32_t pos;
    if (!keyed_row(d.row_keys, row, item, pos)) return false;
    if (want) e3d_keyed_normal4(e3d_keyed_words(d.seed, item, d.stream, step, pos, (uint32_t)(i - row * d.nb)), z);
    return true;
}

// ---------------------------------------------------------------- DDPM ancestral update
struct DdpmCoef { float sra, beta, s1m, sigma; };

// ``z``: the element's draw, or null for the mean alone.  Taken by address so that a caller's load of the draw and this
// add share one branch: the compiler's choice between a fused multiply-add and two rounded products for the noise term
// (the n % 4 tail gets the former, the float4 loop the latter) hangs on that, and seeded results on the choice.
__device__ __forceinline__ float ddpm_elem(const DdpmCoef c, float x, float e, const float* z, int wrap) {
    float mean = c.sra * (x - c.beta * e / c.s1m);
    if (z) mean = mean + c.sigma * *z;
    return wrap ? wrap_pi(mean) : mean;
}

// ``out`` may be ``x``: every element is read before it is written, by the thread that writes it.
// KEYED: always the table form, the draws from stream d.stream at step t_dev[0]; a row of no item gets the mean, and at
// sigma == 0 there is no Philox call and the key table is not read.  A keyed launch has n == 4 * n4: no tail.
template <bool KEYED>
__global__ __launch_bounds__(256) void ddpm_step_wrap_kernel(
    const float* x, const float* __restrict__ eps_hat, const Draws d, DdpmCoef c, const float* __restrict__ coef_table,
    const int64_t* __restrict__ t_dev, int wrap, float* out, int64_t n4, int64_t n) {
    bool noisy = KEYED || d.noise != nullptr;
    uint32_t step = 0;
    if (KEYED || coef_table) {   // graph-replayable form: the step index lives on the device, the coefficients in a [T,4] table
        const int64_t t = t_dev[0];
        c = DdpmCoef{coef_table[4 * t], coef_table[4 * t + 1], coef_table[4 * t + 2], coef_table[4 * t + 3]};
        step = (uint32_t)t;
        if (c.sigma == 0.f) noisy = false;   // t == 0: the mean, exactly as the scalar form
    }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
        const f32x4 ev = reinterpret_cast<const f32x4*>(eps_hat)[i];
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        const bool has = noisy && draws4<KEYED>(d, step, i, true, z);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = ddpm_elem(c, xv[j], ev[j], has ? &z[j] : nullptr, wrap);
        reinterpret_cast<f32x4*>(out)[i] = o;
    }
    if (KEYED) return;
    // tail (n % 4)
    const int64_t r = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) out[r] = ddpm_elem(c, x[r], eps_hat[r], noisy ? d.noise + r : nullptr, wrap);
}

// ---------------------------------------------------------------- strided (DDIM / respaced-ancestral) update
// The schedule-consistent jump from t to its successor s < t (Song et al. 2021, eqs. 12 and 16) in the x0 form -- the
// wrap of the x0 estimate is nonlinear, so the update cannot be collapsed into one linear expression:
//   x0 = (x - s1m e) rsa;  wrap_x0: x0 = wrap_pi(x0);  mean = a_s x0 + c_dir e;  out = mean (+ sigma z);  wrap: wrap_pi(out)
// Row t of the [T,8] table (structure_model/utils.py, StridedTables) = (s1m, rsa, a_s, c_dir, sigma, 0, 0, 0).  The
// multiply-adds are written as fmaf, so both instantiations (and the tail) round alike whatever the compiler contracts.
struct StridedCoef { float s1m, rsa, a_s, c_dir, sigma; };

__device__ __forceinline__ StridedCoef strided_row(const float* __restrict__ coef_table, int64_t t) {
    const float* r = coef_table + 8 * t;
    return StridedCoef{r[0], r[1], r[2], r[3], r[4]};
}

__device__ __forceinline__ float strided_elem(const StridedCoef c, float x, float e, float z, bool noisy, int wrap,
                                              int wrap_x0) {
    float x0 = fmaf(-c.s1m, e, x) * c.rsa;
    if (wrap_x0) x0 = wrap_pi(x0);
    float v = fmaf(c.a_s, x0, c.c_dir * e);
    if (noisy) v = fmaf(c.sigma, z, v);
    return wrap ? wrap_pi(v) : v;
}

// A step index outside [0, T): no table row is read, every output is NaN (a wrong index must not pass for a sample)
__device__ __forceinline__ void strided_fill_nan(float* __restrict__ out, int64_t n4, int64_t n) {
    const float q = __builtin_nanf("");
    const f32x4 qv = {q, q, q, q};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = first; i < n4; i += stride) reinterpret_cast<f32x4*>(out)[i] = qv;
    if (n4 * 4 + first < n) out[n4 * 4 + first] = q;
}

// ``out`` may be ``x``: every element is read before it is written, by the thread that writes it.
// KEYED: the draws come from the ancestral keyed launch's stream at step t_dev[0], so a pocket's draw at timestep t is
// the same under either update; a row of no item gets no noise term.  A keyed launch has n == 4 * n4: no tail.
template <bool KEYED>
__global__ __launch_bounds__(256) void strided_step_wrap_kernel(
    const float* x, const float* __restrict__ eps_hat, const Draws d, const float* __restrict__ coef_table,
    const int64_t* __restrict__ t_dev, int T, int wrap, int wrap_x0, float* out, int64_t n4, int64_t n) {
    const int64_t t = t_dev[0];
    if (t < 0 || t >= T) { strided_fill_nan(out, n4, n); return; }
    const StridedCoef c = strided_row(coef_table, t);
    // sigma == 0 (eta = 0, or the last step): nothing is read through noise, no Philox call, the key table is not read
    const bool noisy = (KEYED || d.noise != nullptr) && c.sigma != 0.f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
        const f32x4 ev = reinterpret_cast<const f32x4*>(eps_hat)[i];
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        const bool has = noisy && draws4<KEYED>(d, (uint32_t)t, i, true, z);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = strided_elem(c, xv[j], ev[j], z[j], has, wrap, wrap_x0);
        reinterpret_cast<f32x4*>(out)[i] = o;
    }
    if (KEYED) return;
    // tail (n % 4)
    const int64_t r = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) out[r] = strided_elem(c, x[r], eps_hat[r], noisy ? d.noise[r] : 0.f, noisy, wrap, wrap_x0);
}

// ---------------------------------------------------------------- multistep (DPM-Solver++ 2M) update
// The strided update at eta = 0 plus one term that extrapolates with the x0 estimate the previous step stored (Lu et al.
// 2022, the second-order multistep rule in its data-prediction form; the weight is capped, see MultistepTables):
//   x0 = (x - s1m e) rsa;  wrap_x0: x0 = wrap_pi(x0);  v = a_s x0 + c_dir e
//   c_1 != 0:  d = x0 - prev;  wrap: d = wrap_pi(d);  v += c_1 d          hist = x0;  out = wrap ? wrap_pi(v) : v
// Row t of the [T,8] table (structure_model/utils.py, MultistepTables) = (s1m, rsa, a_s, c_dir, c_1, 0, 0, 0).  The
// expressions up to v are strided_elem's without its noise term, fmaf for fmaf: a row with c_1 == 0 gives its bits.
struct MultistepCoef { float s1m, rsa, a_s, c_dir, c_1; };

__device__ __forceinline__ float multistep_elem(const MultistepCoef c, float x, float e, float prev, bool extrapolate,
                                                int wrap, int wrap_x0, float& hist) {
    float x0 = fmaf(-c.s1m, e, x) * c.rsa;
    if (wrap_x0) x0 = wrap_pi(x0);
    float v = fmaf(c.a_s, x0, c.c_dir * e);
    if (extrapolate) {
        float d = x0 - prev;
        if (wrap) d = wrap_pi(d);   // the state lives on the circle: so does the difference of two estimates of it
        v = fmaf(c.c_1, d, v);
    }
    hist = x0;
    return wrap ? wrap_pi(v) : v;
}

// ``out`` may be ``x`` and ``hist_out`` may be ``hist_in``: every element is read before it is written, by the thread
// that writes it.  A row with c_1 == 0 (the first and the last visited timestep) reads nothing through hist_in.  A step
// index outside [0, T): no table row is read, both outputs are NaN.
__global__ __launch_bounds__(256) void multistep_step_wrap_kernel(
    const float* x, const float* __restrict__ eps_hat, const float* hist_in, const float* __restrict__ coef_table,
    const int64_t* __restrict__ t_dev, int T, int wrap, int wrap_x0, float* out, float* hist_out, int64_t n4, int64_t n) {
    const int64_t t = t_dev[0];
    if (t < 0 || t >= T) {
        strided_fill_nan(out, n4, n);
        strided_fill_nan(hist_out, n4, n);
        return;
    }
    const float* r = coef_table + 8 * t;
    const MultistepCoef c{r[0], r[1], r[2], r[3], r[4]};
    const bool extrapolate = c.c_1 != 0.f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
        const f32x4 ev = reinterpret_cast<const f32x4*>(eps_hat)[i];
        f32x4 pv = {0.f, 0.f, 0.f, 0.f};
        if (extrapolate) pv = reinterpret_cast<const f32x4*>(hist_in)[i];
        f32x4 o, h;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float hj;
            o[j] = multistep_elem(c, xv[j], ev[j], pv[j], extrapolate, wrap, wrap_x0, hj);
            h[j] = hj;
        }
        reinterpret_cast<f32x4*>(out)[i] = o;
        reinterpret_cast<f32x4*>(hist_out)[i] = h;
    }
    // tail (n % 4)
    const int64_t q = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) {
        float hq;
        out[q] = multistep_elem(c, x[q], eps_hat[q], extrapolate ? hist_in[q] : 0.f, extrapolate, wrap, wrap_x0, hq);
        hist_out[q] = hq;
    }
}

// q(x_t | x_0) of one element: wrap(a_t x0 + s_t noise); shared by the buffer form and the keyed form
__device__ __forceinline__ float q_sample_wrap_elem(float a, float s, float x0, float noise) {
    return wrap_pi(a * x0 + s * noise);
}

__global__ __launch_bounds__(256) void q_sample_wrap_kernel(
    const float* __restrict__ x0, const float* __restrict__ noise, const int64_t* __restrict__ t,
    const float* __restrict__ sqrt_ab, const float* __restrict__ sqrt_1mab, float* __restrict__ out,
    int64_t per, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t ti = t[i / per];
        out[i] = q_sample_wrap_elem(sqrt_ab[ti], sqrt_1mab[ti], x0[i], noise[i]);
    }
}

constexpr int CMAX = 32;

// inverse-CDF categorical draw / argmax on a row of C probabilities held in registers
__device__ __forceinline__ int pick_class(const float (&p)[CMAX], int C, float total, int mode, float u) {
    int best = 0;
    if (mode == 0) {
        float bv = p[0];
#pragma unroll
        for (int c = 1; c < CMAX; ++c)
            if (c < C && p[c] > bv) { bv = p[c]; best = c; }
    } else {
        // index = #{c : cumsum[c] <= u * total}, clamped to C-1
        const float thr = u * total;
        float cum = 0.f;
        int cnt = 0;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) { cum += p[c]; cnt += (cum <= thr) ? 1 : 0; }
        best = cnt < C - 1 ? cnt : C - 1;
    }
    return best;
}

// Design controls: the effective logit z = (logit + bias) * inv_temp, one add and then one multiply in fp32.  A sum
// times a factor has no fused form, and contraction is switched off here so that the product is rounded before anything
// is subtracted from it: z is a function of the three fp32 inputs alone.  bias -inf forbids the class (z = -inf).
__device__ __forceinline__ float effective_logit(float logit, float bias, float inv_temp) {
#pragma clang fp contract(off)
    const float sum = logit + bias;
    return sum * inv_temp;
}

// ---------------------------------------------------------------- what the discrete kernels share
// Column x0 of a CxC table in registers, p[c] = q[c][x0] = (q @ onehot(x0))[c]: the forward law of a row whose clean
// class is x0 (model.py:305-308).  Returns the column's sum.
__device__ __forceinline__ float table_column(const float* __restrict__ q, int x0, int C, float (&p)[CMAX]) {
    float tot = 0.f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        p[c] = c < C ? q[c * C + x0] : 0.f;
        tot += p[c];
    }
    return tot;
}

// The uniform of a keyed draw: word 0 of block 0 of (seed, item, stream, step, position).
__device__ __forceinline__ float keyed_uniform_at(uint64_t seed, uint64_t item, int stream, uint32_t step, uint32_t pos) {
    return e3d_keyed_uniform(e3d_keyed_words(seed, item, stream, step, pos, 0).w[0]);
}

// ... of row n of a key table.  False, and ``un`` as it was, for a row of no item: what such a row gets is its kernel's rule.
__device__ __forceinline__ bool keyed_row_uniform(const int64_t* __restrict__ row_keys, int64_t n, uint64_t seed, int stream,
                                                  uint32_t step, float& un) {
    uint64_t item;
    uint32_t pos;
    if (!keyed_row(row_keys, n, item, pos)) return false;
    un = keyed_uniform_at(seed, item, stream, step, pos);
    return true;
}

// The three CxC tables of a workgroup's item in LDS, what p(z_s | z_t) is made of: Qsb, Qtb and
// Qt = (Qsb/Qtb) / rowsum(Qsb/Qtb)   (sequence_model/sample.py:160), filled for item b; s_rs holds the C row sums.  Three
// barriers: all threads of the workgroup come here, or none.
__device__ __forceinline__ void load_posterior_tables(float* s_qsb, float* s_qtb, float* s_qt, float* s_rs,
                                                      const float* __restrict__ Qsb, const float* __restrict__ Qtb, int b,
                                                      int C) {
    const int tid = threadIdx.x, CC = C * C;
    for (int i = tid; i < CC; i += blockDim.x) {
        s_qsb[i] = Qsb[(int64_t)b * CC + i];
        s_qtb[i] = Qtb[(int64_t)b * CC + i];
    }
    __syncthreads();
    if (tid < C) {
        float rs = 0.f;
        for (int j = 0; j < C; ++j) rs += s_qsb[tid * C + j] / s_qtb[tid * C + j];
        s_rs[tid] = rs;
    }
    __syncthreads();
    for (int i = tid; i < CC; i += blockDim.x) s_qt[i] = (s_qsb[i] / s_qtb[i]) / s_rs[i / C];
    __syncthreads();
}

// Qtb[x0][xt], the denominator of the x0 term of the posterior; 0 -> 1e-6   (sample.py:128)
__device__ __forceinline__ float posterior_den(const float* s_qtb, int x0, int xt, int C) {
    const float den = s_qtb[x0 * C + xt];
    return den == 0.f ? 1e-6f : den;
}

// The posterior of a row, stated once for discrete_posterior_kernel and discrete_score_rows_kernel -- as macros: as
// functions, in every form measured, these steps changed the compiled posterior kernel with controls (slower per launch,
// or fewer waves per SIMD), while a macro leaves each kernel the code of the expression written out in it.
#define UNROLL _Pragma("unroll")

// p[c] / sum(p) over the C classes, zero beyond them; a row that sums to zero is 1e-5 everywhere first (sample.py:166).
// ntot: the sum of the result.
#define NORMALISE_ROW(p_, C_, ntot_)                                                         \
    do {                                                                                     \
        float tot_ = 0.f;                                                                    \
        UNROLL for (int c = 0; c < CMAX; ++c)                                                \
            if (c < C_) tot_ += p_[c];                                                       \
        if (tot_ == 0.f) {                                                                   \
            UNROLL for (int c = 0; c < CMAX; ++c) p_[c] = c < C_ ? 1e-5f : 0.f;              \
            tot_ = 0.f;                                                                      \
            UNROLL for (int c = 0; c < CMAX; ++c)                                            \
                if (c < C_) tot_ += p_[c];                                                   \
        }                                                                                    \
        ntot_ = 0.f;                                                                         \
        UNROLL for (int c = 0; c < CMAX; ++c) {                                              \
            p_[c] = c < C_ ? p_[c] / tot_ : 0.f;                                             \
            ntot_ += p_[c];                                                                  \
        }                                                                                    \
    } while (0)

// pred = exp(z - mx) and se its sum, z the C logits at lg (CTL: the effective logits, bias [rows, C] or NULL for zero)
// and mx their maximum.  none: every class forbidden -- -inf - -inf is NaN, so no exponential is taken: pred = 0, se = 0.
#define POSTERIOR_SOFTMAX(CTL_, lg_, bias_, inv_temp_, n_, C_, pred_, mx_, none_, se_)                                \
    do {                                                                                                               \
        mx_ = -INFINITY;                                                                                               \
        UNROLL for (int c = 0; c < CMAX; ++c) {                                                                        \
            if (CTL_) pred_[c] = c < C_ ? effective_logit(lg_[c], bias_ ? bias_[n_ * C_ + c] : 0.f, inv_temp_) : -INFINITY; \
            else pred_[c] = c < C_ ? lg_[c] : -INFINITY;                                                               \
            mx_ = fmaxf(mx_, pred_[c]);                                                                                \
        }                                                                                                              \
        none_ = CTL_ && mx_ == -INFINITY;                                                                              \
        se_ = 0.f;                                                                                                     \
        UNROLL for (int c = 0; c < CMAX; ++c) {                                                                        \
            pred_[c] = (c < C_ && !none_) ? expf(pred_[c] - mx_) : 0.f;                                                \
            se_ += pred_[c];                                                                                           \
        }                                                                                                              \
    } while (0)

// The x0 prediction pred / se (zero when none; pred holds it afterwards) mixed over x0 at class xt,
//   prob[c] = sum_x0 pred[x0] * (Qt[c][xt] * Qsb[x0][c]) / Qtb[x0][xt]   (sample.py:129-139,162-165)
// then NORMALISE_ROW: a forbidden class has pred == 0 exactly, a row with every class forbidden takes the zero-total rule.
#define POSTERIOR_MIXTURE(pred_, se_, none_, xt_, C_, s_qsb_, s_qtb_, s_qt_, prob_, ntot_)                   \
    do {                                                                                                      \
        UNROLL for (int c = 0; c < CMAX; ++c) { pred_[c] = none_ ? 0.f : pred_[c] / se_; prob_[c] = 0.f; }    \
        _Pragma("unroll 1") for (int k_ = 0; k_ < C_; ++k_) {                                                 \
            const float den_ = posterior_den(s_qtb_, k_, xt_, C_);                                            \
            const float w_ = pred_[k_];                                                                       \
            UNROLL for (int c = 0; c < CMAX; ++c)                                                             \
                if (c < C_) prob_[c] += w_ * ((s_qt_[c * C_ + xt_] * s_qsb_[k_ * C_ + c]) / den_);            \
        }                                                                                                     \
        NORMALISE_ROW(prob_, C_, ntot_);                                                                      \
    } while (0)

// One workgroup per batch item, its tables in LDS; each thread walks rows l = tid, tid+256, ...
// KEYED: the uniform of row n = b * L + l is drawn from stream 3 at step s_dev[0] with the row's key (row_keys[n]);
// rows of no item draw u = 0.
// CTL: the softmax runs over the effective logits (bias [B*L, C] or NULL for zero, inv_temp > 0).
template <bool KEYED, bool CTL>
__global__ __launch_bounds__(256) void discrete_posterior_kernel(
    const int32_t* __restrict__ xt_idx, const float* __restrict__ logits, const float* __restrict__ Qsb,
    const float* __restrict__ Qtb, const float* __restrict__ u, int mode, int32_t* __restrict__ out_idx,
    float* __restrict__ prob_out, int L, int C, const int64_t* __restrict__ row_keys, uint64_t seed,
    const int64_t* __restrict__ s_dev, const float* __restrict__ bias, float inv_temp) {
    __shared__ float s_qsb[CMAX * CMAX], s_qtb[CMAX * CMAX], s_qt[CMAX * CMAX], s_rs[CMAX];
    const int b = blockIdx.x;
    load_posterior_tables(s_qsb, s_qtb, s_qt, s_rs, Qsb, Qtb, b, C);

    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        const int64_t n = (int64_t)b * L + l;
        const int xt = xt_idx[n];
        float pred[CMAX], prob[CMAX];
        const float* lg = logits + n * C;
        float mx, se, ntot;
        bool none;
        POSTERIOR_SOFTMAX(CTL, lg, bias, inv_temp, n, C, pred, mx, none, se);
        POSTERIOR_MIXTURE(pred, se, none, xt, C, s_qsb, s_qtb, s_qt, prob, ntot);
        if (prob_out) {
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) prob_out[n * C + c] = prob[c];
        }
        float un = 0.f;
        if (KEYED) keyed_row_uniform(row_keys, n, seed, E3D_STREAM_SEQ_U, (uint32_t)s_dev[0], un);
        else if (u) un = u[n];
        out_idx[n] = pick_class(prob, C, ntot, mode, un);
    }
}

// The last step's pick under design controls, one thread per row: out_idx = the first maximum of the effective logits z,
// logp = log_softmax(z)[out_idx], entropy = -sum p log p of softmax(z) with 0 log 0 = 0.  The entropy is summed as
// p[c] * (lse - (z[c] - mx)): every term is non-negative, so nothing cancels.  A row with every class forbidden:
// out_idx = 0, logp = entropy = NaN.
__global__ __launch_bounds__(256) void discrete_final_pick_kernel(
    const float* __restrict__ logits, const float* __restrict__ bias, float inv_temp, int32_t* __restrict__ out_idx,
    float* __restrict__ logp, float* __restrict__ entropy, int64_t n_rows, int C) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_rows) return;
    const float* lg = logits + n * C;
    float z[CMAX];
    float mx = -INFINITY;
    int best = 0;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        z[c] = c < C ? effective_logit(lg[c], bias ? bias[n * C + c] : 0.f, inv_temp) : -INFINITY;
        if (z[c] > mx) { mx = z[c]; best = c; }
    }
    out_idx[n] = best;
    if (!logp && !entropy) return;
    if (mx == -INFINITY) {
        if (logp) logp[n] = __builtin_nanf("");
        if (entropy) entropy[n] = __builtin_nanf("");
        return;
    }
    float e[CMAX];
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        z[c] = z[c] - mx;
        e[c] = c < C ? expf(z[c]) : 0.f;
        se += e[c];
    }
    const float lse = logf(se);
    if (logp) logp[n] = 0.f - lse;   // z[best] - mx is exactly 0: the pick is the maximum
    if (entropy) {
        float h = 0.f;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (e[c] > 0.f) h += (e[c] / se) * (lse - z[c]);
        entropy[n] = h;
    }
}

// KEYED (training draws): the uniform of row n = b * L + l is word 0 of stream 7 for (item_ids[b], epoch_dev[0], l).
template <bool KEYED>
__global__ __launch_bounds__(256) void discrete_q_sample_kernel(
    const int32_t* __restrict__ x0_idx, const float* __restrict__ Qtb, const float* __restrict__ u,
    int mode, int32_t* __restrict__ out_idx, int L, int C, int64_t n_rows, const int64_t* __restrict__ item_ids,
    const int64_t* __restrict__ epoch_dev, uint64_t seed) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_rows) return;
    const int x0 = x0_idx[n];
    if (x0 < 0) { out_idx[n] = 0; return; }  // all-zero (padding) row -> class 0, model.py:305-308
    const int64_t b = n / L;
    float p[CMAX];
    const float tot = table_column(Qtb + b * C * C, x0, C, p);
    float un = 0.f;
    if (KEYED)
        un = keyed_uniform_at(seed, (uint64_t)item_ids[b], E3D_STREAM_TRAIN_SEQ_U, keyed_epoch(epoch_dev), (uint32_t)(n - b * L));
    else if (u) un = u[n];
    out_idx[n] = pick_class(p, C, tot, mode, un);
}

// ---------------------------------------------------------------- keyed (seeded) draws
// Raw keyed draws of one (stream, step) over a key table (rows of no item: zeros):
//   kind 0: wrap ? wrap_pi(scale * z) : z, z the normals  -> float [rows, 4 nb]   (wrap + stream 0: keyed x_T)
//   kind 1: uniforms from word 0 of block 0                -> float [rows]
//   kind 2: classes from word 0 of block 0, as one-hot     -> float [rows, C]     (stream 2: keyed sequence x_T)
//   kind 3: classes from word 0 of block 0                 -> int32 [rows]
__global__ __launch_bounds__(256) void keyed_draws_kernel(
    const int64_t* __restrict__ row_keys, uint64_t seed, int stream, uint32_t t, int kind, int nb, int C, int wrap,
    float scale, void* __restrict__ out, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t row = kind == 0 ? i / nb : i;
        const uint32_t block = kind == 0 ? (uint32_t)(i - row * nb) : 0u;
        uint64_t item;
        uint32_t pos;
        const bool has = keyed_row(row_keys, row, item, pos);
        const E3dU32x4 w = has ? e3d_keyed_words(seed, item, stream, t, pos, block) : E3dU32x4{{0u, 0u, 0u, 0u}};
        if (kind == 0) {
            float z[4] = {0.f, 0.f, 0.f, 0.f};
            if (has) e3d_keyed_normal4(w, z);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (has && wrap) ? wrap_pi(scale * z[j]) : z[j];
            reinterpret_cast<f32x4*>(out)[i] = o;
        } else if (kind == 1) {
            reinterpret_cast<float*>(out)[i] = has ? e3d_keyed_uniform(w.w[0]) : 0.f;
        } else if (kind == 2) {
            const int k = has ? e3d_keyed_class(w.w[0], C) : -1;
            float* o = reinterpret_cast<float*>(out) + i * C;
            for (int c = 0; c < C; ++c) o[c] = c == k ? 1.f : 0.f;
        } else {
            reinterpret_cast<int32_t*>(out)[i] = has ? e3d_keyed_class(w.w[0], C) : 0;
        }
    }
}

// ---------------------------------------------------------------- keyed training draws
// Frames are padded or trimmed [B, L]: row r is item r / L at position r % L; ids and the epoch live in device memory.
// Timestep of item b: class of word 0 at position 0, block 0 (stream 4: C = T; stream 6: C = T + 1).
__global__ __launch_bounds__(256) void keyed_timesteps_kernel(
    const int64_t* __restrict__ item_ids, const int64_t* __restrict__ epoch_dev, uint64_t seed, int stream, int C,
    int64_t* __restrict__ out, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    out[b] = e3d_keyed_class(e3d_keyed_words(seed, (uint64_t)item_ids[b], stream, keyed_epoch(epoch_dev), 0, 0).w[0], C);
}

// One thread per (row, block j of 4 features): noise = wrap(scale * z), z the stream-5 normals of (item, epoch,
// position, j); x_t = q_sample_wrap_elem(a_t, s_t, x0, noise).  Timesteps are clamped to the tables' T rows.
__global__ __launch_bounds__(256) void keyed_q_sample_wrap_kernel(
    const float* __restrict__ x0, const int64_t* __restrict__ t, const float* __restrict__ sqrt_ab,
    const float* __restrict__ sqrt_1mab, int T, float scale, const int64_t* __restrict__ item_ids,
    const int64_t* __restrict__ epoch_dev, uint64_t seed, float* __restrict__ noise_out, float* __restrict__ xt_out,
    int L, int nb, int64_t n4) {
    const uint32_t epoch = keyed_epoch(epoch_dev);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const int64_t row = i / nb, b = row / L;
        int64_t ti = t[b];
        ti = ti < 0 ? 0 : (ti > T - 1 ? T - 1 : ti);
        const float a = sqrt_ab[ti], s = sqrt_1mab[ti];
        float z[4];
        e3d_keyed_normal4(e3d_keyed_words(seed, (uint64_t)item_ids[b], E3D_STREAM_TRAIN_STRUCT_NOISE, epoch,
                                          (uint32_t)(row - b * L), (uint32_t)(i - row * nb)), z);
        const f32x4 xv = reinterpret_cast<const f32x4*>(x0)[i];
        f32x4 nv, o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            nv[j] = wrap_pi(scale * z[j]);
            o[j] = q_sample_wrap_elem(a, s, xv[j], nv[j]);
        }
        reinterpret_cast<f32x4*>(noise_out)[i] = nv;
        reinterpret_cast<f32x4*>(xt_out)[i] = o;
    }
}

// ---------------------------------------------------------------- partial redesign: replacement conditioning
// After the update that lands the state on noise level s, the held elements (mask != 0) are overwritten in place with a
// forward-noised copy of their known values at level s: x = q_sample_wrap_elem(a, s1m, x0, wrap_pi(scale * z)) with
// (a, s1m) = row t_dev[0] of the [T,2] level table (structure_model/utils.py, KnownLevels) -- the forward law the model
// was trained on.  s1m == 0 (the clean level): x = x0, a copy.  A step index outside [0, T), a NaN row (a timestep that is
// not visited) or a noisy level without draws: the held elements become NaN.  Elements with mask == 0 are not written.
struct KnownLevel { float a, s1m; int kind; };   // kind 0: copy x0, 1: noised copy, 2: NaN

__device__ __forceinline__ KnownLevel known_level(const float* __restrict__ level_table, const int64_t* __restrict__ t_dev,
                                                  int T, bool have_draws) {
    const int64_t t = t_dev[0];
    if (t < 0 || t >= T) return KnownLevel{0.f, 0.f, 2};
    const float a = level_table[2 * t], s1m = level_table[2 * t + 1];
    if (a != a || s1m != s1m) return KnownLevel{a, s1m, 2};
    if (s1m == 0.f) return KnownLevel{a, s1m, 0};
    return KnownLevel{a, s1m, have_draws ? 1 : 2};
}

__device__ __forceinline__ float known_elem(const KnownLevel lv, float scale, float x0, float z) {
    if (lv.kind == 0) return x0;
    if (lv.kind == 2) return __builtin_nanf("");
    return q_sample_wrap_elem(lv.a, lv.s1m, x0, wrap_pi(scale * z));
}

// the four mask bytes of float4 group i as one word (0: the group is free); byte j != 0: element j is held
__device__ __forceinline__ uint32_t known_mask4(const uint8_t* __restrict__ mask, int64_t i) {
    return reinterpret_cast<const uint32_t*>(mask)[i];
}

__device__ __forceinline__ void known_store4(float* x, int64_t i, uint32_t m4, const f32x4 v) {
    if (((m4 & 0xFFu) != 0) && ((m4 & 0xFF00u) != 0) && ((m4 & 0xFF0000u) != 0) && ((m4 & 0xFF000000u) != 0)) {
        reinterpret_cast<f32x4*>(x)[i] = v;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if ((m4 >> (8 * j)) & 0xFFu) x[4 * i + j] = v[j];
}

// KEYED: z = the normals of (seed, item, stream d.stream, step t_dev[0], position, block), laid out as the update's
// stream.  Rows of no item are left alone at every level; a float4 group with no held element makes no Philox call.  A
// keyed launch has n == 4 * n4: no tail.
template <bool KEYED>
__global__ __launch_bounds__(256) void known_compose_wrap_kernel(
    float* x, const float* __restrict__ x0, const uint8_t* __restrict__ mask, const Draws d,
    const float* __restrict__ level_table, const int64_t* __restrict__ t_dev, int T, float scale, int64_t n4, int64_t n) {
    const KnownLevel lv = known_level(level_table, t_dev, T, KEYED || d.noise != nullptr);
    const bool noisy = lv.kind == 1;
    const uint32_t step = (uint32_t)t_dev[0];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const uint32_t m4 = known_mask4(mask, i);
        if (m4 == 0u) continue;
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (!draws4<KEYED>(d, step, i, noisy, z)) continue;
        const f32x4 kv = reinterpret_cast<const f32x4*>(x0)[i];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = known_elem(lv, scale, kv[j], z[j]);
        known_store4(x, i, m4, o);
    }
    if (KEYED) return;
    // tail (n % 4)
    const int64_t r = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n && mask[r]) x[r] = known_elem(lv, scale, x0[r], noisy ? d.noise[r] : 0.f);
}

// Sequence chain: the class index of a held row (mask != 0, x0 >= 0) is redrawn in place from column x0 of Qsb, the
// forward law at the level the step lands on -- p[c] = Qsb[b][c][x0], discrete_q_sample_kernel's convention and
// arithmetic.  KEYED: the uniform is word 0 of stream 11 at step s_dev[0] with the row's key; rows of no item are left alone.
template <bool KEYED>
__global__ __launch_bounds__(256) void discrete_known_compose_kernel(
    int32_t* idx, const int32_t* __restrict__ x0_idx, const uint8_t* __restrict__ mask, const float* __restrict__ Qsb,
    const float* __restrict__ u, int mode, int L, int C, int64_t n_rows, const int64_t* __restrict__ row_keys, uint64_t seed,
    const int64_t* __restrict__ s_dev) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_rows || mask[n] == 0) return;
    const int x0 = x0_idx[n];
    if (x0 < 0 || x0 >= C) return;
    float p[CMAX];
    const float tot = table_column(Qsb + (n / L) * C * C, x0, C, p);
    float un = 0.f;
    if (KEYED && !keyed_row_uniform(row_keys, n, seed, E3D_KNOWN_STREAM_SEQ, (uint32_t)s_dev[0], un)) return;
    if (!KEYED && u) un = u[n];
    idx[n] = pick_class(p, C, tot, mode, un);
}

// ---------------------------------------------------------------- scoring supplied sequences
// Forward noising of N = levels x items at once: row (n, l) is drawn from column x0 of Qtb[n], discrete_q_sample_kernel's
// convention and arithmetic, with the uniform of stream 11 at the step field level_steps[n] -- the draw
// discrete_known_compose_kernel<true> makes for a held row at that step.  A row of no item (x0 outside [0, C), a key
// position outside [0, 2^24), a step outside [0, max_step]) gets class 0.
__global__ __launch_bounds__(256) void discrete_forward_levels_kernel(
    const int32_t* __restrict__ x0_idx, const float* __restrict__ Qtb, const int64_t* __restrict__ row_keys,
    const int64_t* __restrict__ level_steps, int max_step, uint64_t seed, int32_t* __restrict__ out_idx, int L, int C,
    int64_t n_rows) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_rows) return;
    const int x0 = x0_idx[n];
    const int64_t pos = row_keys[2 * n + 1];
    const int64_t step = level_steps[n / L];
    if (x0 < 0 || x0 >= C || pos < 0 || pos >= ((int64_t)1 << 24) || step < 0 || step > max_step) {
        out_idx[n] = 0;
        return;
    }
    float p[CMAX];
    const float tot = table_column(Qtb + (n / L) * C * C, x0, C, p);
    const float un = keyed_uniform_at(seed, (uint64_t)row_keys[2 * n], E3D_KNOWN_STREAM_SEQ, (uint32_t)step, (uint32_t)pos);
    out_idx[n] = pick_class(p, C, tot, 1, un);
}

// The score terms of rows whose clean class x0 is known; one workgroup per item, its tables in LDS.  p is
// discrete_posterior_kernel's prob by construction: both kernels are load_posterior_tables, POSTERIOR_SOFTMAX and
// POSTERIOR_MIXTURE, so p_out == its prob_out, bit for bit.
//   nll  = -log_softmax(logits)[x0] = lse - (logit[x0] - mx), lse = logf(se): mx and se are POSTERIOR_SOFTMAX's
//   p    = POSTERIOR_MIXTURE under that prediction
//   q    = the same expression under the one-hot of x0.  Only the x0 term of the mixture is non-zero there, and
//          0 + 1 * v == v in fp32, fused or not, so the C - 1 zero terms are not computed: the x0 term with
//          posterior_den's guard, then NORMALISE_ROW
//   term = KL(q || p) = sum_c q[c] * (logf(q[c]) - logf(p[c])) over the classes with q[c] > 0, in class order (0 log 0
//          = 0).  A class with q > 0 and p == 0 adds +inf; no term is -inf or NaN, so the sum is finite or +inf.
// is_final items (the chain's last step picks from the raw logits): term = nll, the tables are not read, p_out and
// q_out get NaN.  A row with x0 or xt outside [0, C): NaN in every output.
__global__ __launch_bounds__(256) void discrete_score_rows_kernel(
    const int32_t* __restrict__ xt_idx, const int32_t* __restrict__ x0_idx, const float* __restrict__ logits,
    const float* __restrict__ Qsb, const float* __restrict__ Qtb, const uint8_t* __restrict__ is_final,
    float* __restrict__ term, float* __restrict__ nll, float* __restrict__ p_out, float* __restrict__ q_out, int L, int C) {
    __shared__ float s_qsb[CMAX * CMAX], s_qtb[CMAX * CMAX], s_qt[CMAX * CMAX], s_rs[CMAX];
    const int b = blockIdx.x;
    const bool fin = is_final[b] != 0;      // one value per workgroup: the barriers below are met by all or by none
    if (!fin) load_posterior_tables(s_qsb, s_qtb, s_qt, s_rs, Qsb, Qtb, b, C);
    const float nan = __builtin_nanf("");

    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        const int64_t n = (int64_t)b * L + l;
        const int xt = xt_idx[n], x0 = x0_idx[n];
        const bool row = x0 >= 0 && x0 < C && xt >= 0 && xt < C;
        float pred[CMAX], prob[CMAX];
        float mx, se, ntot, ce = nan;
        bool none = false;
        if (row) {
            const float* lg = logits + n * C;
            POSTERIOR_SOFTMAX(false, lg, ((const float*)nullptr), 1.f, n, C, pred, mx, none, se);
            ce = logf(se) - (lg[x0] - mx);
        }
        nll[n] = ce;
        if (!row || fin) {
            term[n] = ce;
            for (int c = 0; c < C; ++c) {
                if (p_out) p_out[n * C + c] = nan;
                if (q_out) q_out[n * C + c] = nan;
            }
            continue;
        }
        POSTERIOR_MIXTURE(pred, se, none, xt, C, s_qsb, s_qtb, s_qt, prob, ntot);
        // q: the x0 term alone; pred is free now and holds it
        const float qden = posterior_den(s_qtb, x0, xt, C);
#pragma unroll
        for (int c = 0; c < CMAX; ++c) pred[c] = c < C ? (s_qt[c * C + xt] * s_qsb[x0 * C + c]) / qden : 0.f;
        NORMALISE_ROW(pred, C, ntot);
        float kl = 0.f;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (pred[c] > 0.f) kl += prob[c] > 0.f ? pred[c] * (logf(pred[c]) - logf(prob[c])) : INFINITY;
        term[n] = kl;
        if (p_out) {
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) p_out[n * C + c] = prob[c];
        }
        if (q_out) {
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) q_out[n * C + c] = pred[c];
        }
    }
}

// Masked sums of the rows of values [N, L], one wave per item and no atomics: lane j adds positions j, j + 64, ... in
// order, a masked-out position adding an exact +0, then the 64 lanes meet in a fixed xor butterfly (32, 16, .. 1).  The
// result is a function of the item's (position, value) pairs alone: trailing masked-out positions add +0 to sums that
// are never -0, so an item gives the same bits at L = 64 and L = 128, alone or in any batch.
__global__ __launch_bounds__(64) void masked_item_sums_kernel(
    const float* __restrict__ values, const uint8_t* __restrict__ mask, float* __restrict__ sums,
    int32_t* __restrict__ counts, int L) {
    const int64_t base = (int64_t)blockIdx.x * L;
    const int lane = threadIdx.x;
    float acc = 0.f;
    int cnt = 0;
    for (int l = lane; l < L; l += 64) {
        const bool on = mask[base + l] != 0;
        acc += on ? values[base + l] : 0.f;
        cnt += on ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        acc += __shfl_xor(acc, off, 64);
        cnt += __shfl_xor(cnt, off, 64);
    }
    if (lane == 0) {
        sums[blockIdx.x] = acc;
        counts[blockIdx.x] = cnt;
    }
}

// ---------------------------------------------------------------- scoring supplied structures
// Forward noising of N = n * B items at their own levels, one thread per (row, block j of 4 features): item n reads
// x0 and the keys of item n % B (level-major, the host tiles nothing), noise = wrap(scale * z) with z the stream-12
// normals of (item, step level_steps[n], position, j) in stream 1's block layout, x_t = q_sample_wrap_elem(a, s, x0,
// noise) with (a, s) = row step of the two tables -- keyed_q_sample_wrap_kernel's arithmetic.  An item whose step lies
// outside [0, min(max_step, T - 1)] reads no table row and gets NaN; a row of no item (a key position outside
// [0, 2^24)) gets zeros.
__global__ __launch_bounds__(256) void keyed_q_sample_levels_wrap_kernel(
    const float* __restrict__ x0, const int64_t* __restrict__ row_keys, const int64_t* __restrict__ level_steps,
    int max_step, const float* __restrict__ sqrt_ab, const float* __restrict__ sqrt_1mab, int T, float scale, uint64_t seed,
    float* __restrict__ noise_out, float* __restrict__ xt_out, int64_t item4, int64_t batch4, int nb, int64_t n4) {
    const int64_t top = max_step < T - 1 ? max_step : T - 1;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const int64_t step = level_steps[i / item4];
        const int64_t src = i % batch4;                 // the float4 group of item n % B
        const int64_t row = src / nb;
        const int64_t pos = row_keys[2 * row + 1];
        f32x4 nv = {0.f, 0.f, 0.f, 0.f}, o = {0.f, 0.f, 0.f, 0.f};
        if (step < 0 || step > top) {
            const float q = __builtin_nanf("");
            nv = f32x4{q, q, q, q};
            o = nv;
        } else if (pos >= 0 && pos < ((int64_t)1 << 24)) {
            const float a = sqrt_ab[step], s = sqrt_1mab[step];
            float z[4];
            e3d_keyed_normal4(e3d_keyed_words(seed, (uint64_t)row_keys[2 * row], E3D_SCORE_STRUCT_NOISE, (uint32_t)step,
                                              (uint32_t)pos, (uint32_t)(src - row * nb)), z);
            const f32x4 xv = reinterpret_cast<const f32x4*>(x0)[src];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                nv[j] = wrap_pi(scale * z[j]);
                o[j] = q_sample_wrap_elem(a, s, xv[j], nv[j]);
            }
        }
        reinterpret_cast<f32x4*>(noise_out)[i] = nv;
        reinterpret_cast<f32x4*>(xt_out)[i] = o;
    }
}

// The score terms of one element from row t of the [T,4] table (structure_model/utils.py, ScoreTables) = (k, h, add, 0):
//   err = wrap_pi(eps - eps_hat)   delta = wrap_pi(k * (eps_hat - eps))   term = h * (delta * delta) + add   err2 = err * err
// Contraction is off: every product is rounded before it is added to, so term and err2 are functions of the fp32 inputs
// alone and the sums below are sums of the stored values.
struct ScoreCoef { float k, h, add; };

__device__ __forceinline__ void angle_score_elem(const ScoreCoef c, float eps_hat, float eps, float& term, float& err,
                                                 float& err2) {
#pragma clang fp contract(off)
    err = wrap_pi(eps - eps_hat);
    const float d = c.k * (eps_hat - eps);
    const float delta = wrap_pi(d);
    const float sq = delta * delta;
    const float scaled = c.h * sq;
    term = scaled + c.add;
    err2 = err * err;
}

constexpr int SCORE_FMAX = 32;

// One wave per item n, no atomics.  Lane j takes positions j, j + 64, ... in order; a residue's value is the sum of its
// masked elements in feature order, a masked-out element adding an exact +0 through a select (NaN may sit there); the
// lane adds its residues in order, then the 64 lanes meet in a fixed xor butterfly (32, 16, .. 1).  Per-feature sums
// take the same lane walk and butterfly.  The sums are a function of the item's (position, feature, value) triples
// alone, and tot_* == masked_item_sums_kernel on res_* with the any-element-set residue mask, bit for bit: that kernel
// adds the same values (an unset residue's is +0 here, and +0 there) in the same order.  mask is read as item n % B.
// A step outside [0, T): no table row is read, every float output is NaN; counts is the mask's count regardless.
__global__ __launch_bounds__(64) void angle_score_items_kernel(
    const float* __restrict__ eps_hat, const float* __restrict__ eps, const uint8_t* __restrict__ mask,
    const int64_t* __restrict__ level_steps, const float* __restrict__ coef, int T, float* __restrict__ term,
    float* __restrict__ err, float* __restrict__ res_term, float* __restrict__ res_err2, float* __restrict__ feat_term,
    float* __restrict__ feat_err2, float* __restrict__ tot_term, float* __restrict__ tot_err2, int32_t* __restrict__ counts,
    int B, int L, int nb) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const int64_t base = (int64_t)n * L * nb, mbase = (int64_t)(n % B) * L * nb;      // in groups of 4 elements
    const int64_t step = level_steps[n];
    const bool bad = step < 0 || step >= T;
    const float nan = __builtin_nanf("");
    const ScoreCoef c = bad ? ScoreCoef{nan, nan, nan} : ScoreCoef{coef[4 * step], coef[4 * step + 1], coef[4 * step + 2]};
    float ft[SCORE_FMAX], fe[SCORE_FMAX];
#pragma unroll
    for (int f = 0; f < SCORE_FMAX; ++f) ft[f] = fe[f] = 0.f;
    float acc_t = 0.f, acc_e = 0.f;
    int cnt = 0;
    for (int l = lane; l < L; l += 64) {
        float rt = 0.f, re = 0.f;
#pragma unroll
        for (int j = 0; j < SCORE_FMAX / 4; ++j) {
            if (j < nb) {
                const int64_t g = (int64_t)l * nb + j;
                const f32x4 hv = reinterpret_cast<const f32x4*>(eps_hat)[base + g];
                const f32x4 ev = reinterpret_cast<const f32x4*>(eps)[base + g];
                const uint32_t m4 = reinterpret_cast<const uint32_t*>(mask)[mbase + g];
                f32x4 tv, rv;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float t, r, r2;
                    angle_score_elem(c, hv[q], ev[q], t, r, r2);
                    if (bad) t = r = r2 = nan;
                    tv[q] = t;
                    rv[q] = r;
                    const bool on = ((m4 >> (8 * q)) & 0xFFu) != 0;
                    const float st = on ? t : 0.f, se = on ? r2 : 0.f;
                    rt += st;
                    re += se;
                    ft[4 * j + q] += st;
                    fe[4 * j + q] += se;
                    cnt += on ? 1 : 0;
                }
                if (term) reinterpret_cast<f32x4*>(term)[base + g] = tv;
                if (err) reinterpret_cast<f32x4*>(err)[base + g] = rv;
            }
        }
        if (res_term) res_term[(int64_t)n * L + l] = bad ? nan : rt;
        if (res_err2) res_err2[(int64_t)n * L + l] = bad ? nan : re;
        acc_t += rt;
        acc_e += re;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        acc_t += __shfl_xor(acc_t, off, 64);
        acc_e += __shfl_xor(acc_e, off, 64);
        cnt += __shfl_xor(cnt, off, 64);
    }
#pragma unroll
    for (int f = 0; f < SCORE_FMAX; ++f) {
        if (f < 4 * nb) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                ft[f] += __shfl_xor(ft[f], off, 64);
                fe[f] += __shfl_xor(fe[f], off, 64);
            }
        }
    }
    if (lane != 0) return;
    tot_term[n] = bad ? nan : acc_t;
    tot_err2[n] = bad ? nan : acc_e;
    counts[n] = cnt;
#pragma unroll
    for (int f = 0; f < SCORE_FMAX; ++f) {
        if (f < 4 * nb) {
            if (feat_term) feat_term[(int64_t)n * 4 * nb + f] = bad ? nan : ft[f];
            if (feat_err2) feat_err2[(int64_t)n * 4 * nb + f] = bad ? nan : fe[f];
        }
    }
}

}  // namespace

// ---------------------------------------------------------------- what the entry points share
// 256-thread blocks: one thread per item, or -- a grid-stride sweep over n items -- at least one block and at most 2048
static unsigned row_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }
static unsigned sweep_blocks(int64_t n) { return n <= 0 ? 1u : (n > 2048 * 256 ? 2048u : row_blocks(n)); }

static bool aligned16(std::initializer_list<const void*> ptrs) {   // a null pointer (an absent operand) passes
    for (const void* p : ptrs)
        if ((uintptr_t)p % 16) return false;
    return true;
}
#define REQUIRE_ALIGNED16(name, ...) E3D_REQUIRE(aligned16({__VA_ARGS__}), name ": pointers must be 16B aligned")

// A keyed row is at most 256 blocks of 4 features: the block is a byte of the Philox counter (e3d_philox.h)
static bool keyed_width(int F) { return F > 0 && F % 4 == 0 && F / 4 <= 256; }
#define REQUIRE_KEYED_WIDTH(name, F) \
    E3D_REQUIRE(keyed_width(F), name ": F must be a multiple of 4 in [4, 1024] (F=%d)", F)
// ... and the step is 16 bits of it: a table read by the step index has at most 65536 rows
#define REQUIRE_KEYED_STEPS(name, T) E3D_REQUIRE(T <= 65536, name ": keyed streams hold steps up to 65535 (T=%d)", T)

// The discrete kernels hold a row's classes in CMAX registers; mode 0 is argmax, 1 the categorical draw from uniforms u
#define REQUIRE_CLASSES(name, lo, C) E3D_REQUIRE(C >= lo && C <= CMAX, name ": C must be in [" #lo ",%d] (C=%d)", CMAX, C)
#define REQUIRE_MODE(name, mode, u) E3D_REQUIRE(mode == 0 || (mode == 1 && u), name ": mode 1 needs uniforms")

static Draws buffer_draws(const float* noise) { return Draws{noise, nullptr, 0ull, 0, 1}; }
static Draws keyed_draws_of(const int64_t* row_keys, uint64_t seed, int stream, int F) {
    return Draws{nullptr, row_keys, seed, stream, F / 4};
}

extern "C" int e3d_ddpm_step_wrap(const float* x, const float* eps_hat, const float* noise,
                                  float sqrt_recip_alpha, float beta, float sqrt_one_minus_ab,
                                  float sigma, int wrap, float* out, int64_t n, void* stream) {
    E3D_REQUIRE(x && eps_hat && out && n > 0, "ddpm_step_wrap: bad arguments");
    REQUIRE_ALIGNED16("ddpm_step_wrap", x, eps_hat, out, noise);
    hipLaunchKernelGGL(ddpm_step_wrap_kernel<false>, dim3(sweep_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, x, eps_hat,
                       buffer_draws(sigma != 0.f ? noise : nullptr), DdpmCoef{sqrt_recip_alpha, beta, sqrt_one_minus_ab, sigma},
                       nullptr, nullptr, wrap, out, n / 4, n);
    return e3d_launch_status("e3d_ddpm_step_wrap");
}

extern "C" int e3d_ddpm_step_wrap_table(const float* x, const float* eps_hat, const float* noise,
                                        const float* coef_table, const int64_t* t_dev, int wrap, float* out,
                                        int64_t n, void* stream) {
    E3D_REQUIRE(x && eps_hat && noise && coef_table && t_dev && out && n > 0, "ddpm_step_wrap_table: bad arguments");
    REQUIRE_ALIGNED16("ddpm_step_wrap_table", x, eps_hat, out, noise);
    hipLaunchKernelGGL(ddpm_step_wrap_kernel<false>, dim3(sweep_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, x, eps_hat,
                       buffer_draws(noise), DdpmCoef{0.f, 0.f, 1.f, 0.f}, coef_table, t_dev, wrap, out, n / 4, n);
    return e3d_launch_status("e3d_ddpm_step_wrap_table");
}

extern "C" int e3d_strided_step_wrap(const float* x, const float* eps_hat, const float* noise, const float* coef_table,
                                     const int64_t* t_dev, int T, int wrap, int wrap_x0, float* out, int64_t n,
                                     void* stream) {
    E3D_REQUIRE(x && eps_hat && coef_table && t_dev && out && n > 0 && T > 0, "strided_step_wrap: bad arguments");
    REQUIRE_ALIGNED16("strided_step_wrap", x, eps_hat, out, noise);
    hipLaunchKernelGGL(strided_step_wrap_kernel<false>, dim3(sweep_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, x,
                       eps_hat, buffer_draws(noise), coef_table, t_dev, T, wrap, wrap_x0, out, n / 4, n);
    return e3d_launch_status("e3d_strided_step_wrap");
}

extern "C" int e3d_multistep_step_wrap(const float* x, const float* eps_hat, const float* hist_in, const float* coef_table,
                                       const int64_t* t_dev, int T, int wrap, int wrap_x0, float* out, float* hist_out,
                                       int64_t n, void* stream) {
    E3D_REQUIRE(x && eps_hat && hist_in && coef_table && t_dev && out && hist_out && n > 0 && T > 0,
                "multistep_step_wrap: bad arguments");
    E3D_REQUIRE(out != hist_out, "multistep_step_wrap: out and hist_out must be two buffers");
    REQUIRE_ALIGNED16("multistep_step_wrap", x, eps_hat, hist_in, out, hist_out);
    hipLaunchKernelGGL(multistep_step_wrap_kernel, dim3(sweep_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, x, eps_hat,
                       hist_in, coef_table, t_dev, T, wrap, wrap_x0, out, hist_out, n / 4, n);
    return e3d_launch_status("e3d_multistep_step_wrap");
}

extern "C" int e3d_q_sample_wrap(const float* x0, const float* noise, const int64_t* t,
                                 const float* sqrt_ab, const float* sqrt_1mab, float* out, int B,
                                 int64_t per, void* stream) {
    E3D_REQUIRE(x0 && noise && t && sqrt_ab && sqrt_1mab && out && B > 0 && per > 0, "q_sample_wrap: bad arguments");
    const int64_t n = (int64_t)B * per;
    hipLaunchKernelGGL(q_sample_wrap_kernel, dim3(sweep_blocks(n)), dim3(256), 0, (hipStream_t)stream, x0, noise, t,
                       sqrt_ab, sqrt_1mab, out, per, n);
    return e3d_launch_status("e3d_q_sample_wrap");
}

extern "C" int e3d_discrete_posterior_sample(const int32_t* xt_idx, const float* logits,
                                             const float* Qsb, const float* Qtb, const float* u,
                                             int mode, int32_t* out_idx, float* prob_out, int B,
                                             int L, int C, void* stream) {
    E3D_REQUIRE(xt_idx && logits && Qsb && Qtb && out_idx && B > 0 && L > 0, "discrete_posterior: bad arguments");
    REQUIRE_CLASSES("discrete_posterior", 2, C);
    REQUIRE_MODE("discrete_posterior", mode, u);
    hipLaunchKernelGGL((discrete_posterior_kernel<false, false>), dim3(B), dim3(256), 0, (hipStream_t)stream, xt_idx, logits,
                       Qsb, Qtb, u, mode, out_idx, prob_out, L, C, nullptr, 0ull, nullptr, nullptr, 1.f);
    return e3d_launch_status("e3d_discrete_posterior_sample");
}

extern "C" int e3d_discrete_q_sample(const int32_t* x0_idx, const float* Qtb, const float* u, int mode,
                                     int32_t* out_idx, int B, int L, int C, void* stream) {
    E3D_REQUIRE(x0_idx && Qtb && out_idx && B > 0 && L > 0, "discrete_q_sample: bad arguments");
    REQUIRE_CLASSES("discrete_q_sample", 2, C);
    REQUIRE_MODE("discrete_q_sample", mode, u);
    const int64_t n = (int64_t)B * L;
    hipLaunchKernelGGL(discrete_q_sample_kernel<false>, dim3(row_blocks(n)), dim3(256), 0,
                       (hipStream_t)stream, x0_idx, Qtb, u, mode, out_idx, L, C, n, nullptr, nullptr, 0ull);
    return e3d_launch_status("e3d_discrete_q_sample");
}

// ---------------------------------------------------------------- keyed (seeded) entry points
extern "C" int e3d_keyed_ddpm_step_wrap(const float* x, const float* eps_hat, const float* coef_table, const int64_t* t_dev,
                                        const int64_t* row_keys, uint64_t seed, int wrap, float* out, int64_t rows, int F,
                                        void* stream) {
    E3D_REQUIRE(x && eps_hat && coef_table && t_dev && row_keys && out && rows > 0, "keyed_ddpm_step_wrap: bad arguments");
    REQUIRE_KEYED_WIDTH("keyed_ddpm_step_wrap", F);
    REQUIRE_ALIGNED16("keyed_ddpm_step_wrap", x, eps_hat, out);
    const int64_t n4 = rows * (F / 4);
    hipLaunchKernelGGL(ddpm_step_wrap_kernel<true>, dim3(sweep_blocks(n4)), dim3(256), 0, (hipStream_t)stream, x, eps_hat,
                       keyed_draws_of(row_keys, seed, E3D_STREAM_STRUCT_STEP, F), DdpmCoef{0.f, 0.f, 1.f, 0.f}, coef_table,
                       t_dev, wrap, out, n4, 4 * n4);
    return e3d_launch_status("e3d_keyed_ddpm_step_wrap");
}

extern "C" int e3d_keyed_strided_step_wrap(const float* x, const float* eps_hat, const float* coef_table,
                                           const int64_t* t_dev, int T, const int64_t* row_keys, uint64_t seed, int wrap,
                                           int wrap_x0, float* out, int64_t rows, int F, void* stream) {
    E3D_REQUIRE(x && eps_hat && coef_table && t_dev && row_keys && out && rows > 0 && T > 0,
                "keyed_strided_step_wrap: bad arguments");
    REQUIRE_KEYED_WIDTH("keyed_strided_step_wrap", F);
    REQUIRE_KEYED_STEPS("keyed_strided_step_wrap", T);
    REQUIRE_ALIGNED16("keyed_strided_step_wrap", x, eps_hat, out);
    const int64_t n4 = rows * (F / 4);
    hipLaunchKernelGGL(strided_step_wrap_kernel<true>, dim3(sweep_blocks(n4)), dim3(256), 0, (hipStream_t)stream, x, eps_hat,
                       keyed_draws_of(row_keys, seed, E3D_STREAM_STRUCT_STEP, F), coef_table, t_dev, T, wrap, wrap_x0, out, n4,
                       4 * n4);
    return e3d_launch_status("e3d_keyed_strided_step_wrap");
}

extern "C" int e3d_keyed_discrete_posterior_sample(const int32_t* xt_idx, const float* logits, const float* Qsb,
                                                   const float* Qtb, const int64_t* row_keys, uint64_t seed,
                                                   const int64_t* s_dev, int32_t* out_idx, int B, int L, int C,
                                                   void* stream) {
    E3D_REQUIRE(xt_idx && logits && Qsb && Qtb && row_keys && s_dev && out_idx && B > 0 && L > 0,
                "keyed_discrete_posterior: bad arguments");
    REQUIRE_CLASSES("keyed_discrete_posterior", 2, C);
    hipLaunchKernelGGL((discrete_posterior_kernel<true, false>), dim3(B), dim3(256), 0, (hipStream_t)stream, xt_idx, logits,
                       Qsb, Qtb, nullptr, 1, out_idx, nullptr, L, C, row_keys, seed, s_dev, nullptr, 1.f);
    return e3d_launch_status("e3d_keyed_discrete_posterior_sample");
}

extern "C" int e3d_keyed_draws(const int64_t* row_keys, uint64_t seed, int stream_id, int t, int kind, int width,
                               int wrap, float scale, void* out, int64_t rows, void* stream) {
    E3D_REQUIRE(row_keys && out && rows > 0, "keyed_draws: bad arguments");
    E3D_REQUIRE(((stream_id >= 0 && stream_id <= 3) || stream_id == E3D_KNOWN_STREAM_STRUCT ||
                 stream_id == E3D_KNOWN_STREAM_SEQ || stream_id == E3D_SCORE_STRUCT_NOISE) && t >= 0 && t <= 65535,
                "keyed_draws: stream %d / step %d out of range", stream_id, t);
    E3D_REQUIRE(kind >= 0 && kind <= 3, "keyed_draws: kind %d", kind);
    E3D_REQUIRE(kind != 0 || (keyed_width(width) && aligned16({out})),
                "keyed_draws: normals need F a multiple of 4 in [4, 1024] (F=%d) and a 16B aligned output", width);
    E3D_REQUIRE(kind < 2 || (width >= 2 && width <= 1 << 24), "keyed_draws: class count %d", width);
    const int nb = kind == 0 ? width / 4 : 1;
    const int64_t n = rows * nb;
    hipLaunchKernelGGL(keyed_draws_kernel, dim3(sweep_blocks(n)), dim3(256), 0, (hipStream_t)stream, row_keys, seed,
                       stream_id, (uint32_t)t, kind, nb, width, wrap, scale, out, n);
    return e3d_launch_status("e3d_keyed_draws");
}

// ---------------------------------------------------------------- keyed training draws (entry points)
extern "C" int e3d_keyed_timesteps(const int64_t* item_ids, const int64_t* epoch_dev, uint64_t seed, int stream_id, int C,
                                   int64_t* out, int B, void* stream) {
    E3D_REQUIRE(item_ids && epoch_dev && out && B > 0, "keyed_timesteps: bad arguments");
    E3D_REQUIRE(stream_id == E3D_STREAM_TRAIN_STRUCT_T || stream_id == E3D_STREAM_TRAIN_SEQ_T,
                "keyed_timesteps: stream %d is not a timestep stream", stream_id);
    E3D_REQUIRE(C >= 1 && C <= 1 << 24, "keyed_timesteps: class count %d", C);
    hipLaunchKernelGGL(keyed_timesteps_kernel, dim3(row_blocks(B)), dim3(256), 0, (hipStream_t)stream,
                       item_ids, epoch_dev, seed, stream_id, C, out, B);
    return e3d_launch_status("e3d_keyed_timesteps");
}

extern "C" int e3d_keyed_q_sample_wrap(const float* x0, const int64_t* t, const float* sqrt_ab, const float* sqrt_1mab,
                                       int T, float scale, const int64_t* item_ids, const int64_t* epoch_dev,
                                       uint64_t seed, float* noise_out, float* xt_out, int B, int L, int F,
                                       void* stream) {
    E3D_REQUIRE(x0 && t && sqrt_ab && sqrt_1mab && item_ids && epoch_dev && noise_out && xt_out && B > 0 && L > 0 && T > 0,
                "keyed_q_sample_wrap: bad arguments");
    E3D_REQUIRE(L <= 1 << 24, "keyed_q_sample_wrap: positions must stay below 2^24 (L=%d)", L);
    REQUIRE_KEYED_WIDTH("keyed_q_sample_wrap", F);
    REQUIRE_ALIGNED16("keyed_q_sample_wrap", x0, noise_out, xt_out);
    const int64_t n4 = (int64_t)B * L * (F / 4);
    hipLaunchKernelGGL(keyed_q_sample_wrap_kernel, dim3(sweep_blocks(n4)), dim3(256), 0, (hipStream_t)stream, x0, t, sqrt_ab,
                       sqrt_1mab, T, scale, item_ids, epoch_dev, seed, noise_out, xt_out, L, F / 4, n4);
    return e3d_launch_status("e3d_keyed_q_sample_wrap");
}

extern "C" int e3d_keyed_discrete_q_sample(const int32_t* x0_idx, const float* Qtb, const int64_t* item_ids,
                                           const int64_t* epoch_dev, uint64_t seed, int32_t* out_idx, int B, int L, int C,
                                           void* stream) {
    E3D_REQUIRE(x0_idx && Qtb && item_ids && epoch_dev && out_idx && B > 0 && L > 0, "keyed_discrete_q_sample: bad arguments");
    E3D_REQUIRE(L <= 1 << 24, "keyed_discrete_q_sample: positions must stay below 2^24 (L=%d)", L);
    REQUIRE_CLASSES("keyed_discrete_q_sample", 2, C);
    const int64_t n = (int64_t)B * L;
    hipLaunchKernelGGL(discrete_q_sample_kernel<true>, dim3(row_blocks(n)), dim3(256), 0,
                       (hipStream_t)stream, x0_idx, Qtb, nullptr, 1, out_idx, L, C, n, item_ids, epoch_dev, seed);
    return e3d_launch_status("e3d_keyed_discrete_q_sample");
}

// ---------------------------------------------------------------- partial redesign (entry points)
extern "C" int e3d_known_compose_wrap(float* x, const float* x0, const uint8_t* mask, const float* noise,
                                      const float* level_table, const int64_t* t_dev, int T, float scale, int64_t n,
                                      void* stream) {
    E3D_REQUIRE(x && x0 && mask && level_table && t_dev && n > 0 && T > 0, "known_compose_wrap: bad arguments");
    E3D_REQUIRE(aligned16({x, x0, noise}) && ((uintptr_t)mask % 4) == 0,
                "known_compose_wrap: x, x0, noise must be 16B and mask 4B aligned");
    hipLaunchKernelGGL(known_compose_wrap_kernel<false>, dim3(sweep_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, x, x0,
                       mask, buffer_draws(noise), level_table, t_dev, T, scale, n / 4, n);
    return e3d_launch_status("e3d_known_compose_wrap");
}

extern "C" int e3d_keyed_known_compose_wrap(float* x, const float* x0, const uint8_t* mask, const float* level_table,
                                            const int64_t* t_dev, int T, float scale, const int64_t* row_keys,
                                            uint64_t seed, int64_t rows, int F, void* stream) {
    E3D_REQUIRE(x && x0 && mask && level_table && t_dev && row_keys && rows > 0 && T > 0,
                "keyed_known_compose_wrap: bad arguments");
    REQUIRE_KEYED_WIDTH("keyed_known_compose_wrap", F);
    REQUIRE_KEYED_STEPS("keyed_known_compose_wrap", T);
    E3D_REQUIRE(aligned16({x, x0}) && ((uintptr_t)mask % 4) == 0,
                "keyed_known_compose_wrap: x, x0 must be 16B and mask 4B aligned");
    const int64_t n4 = rows * (F / 4);
    hipLaunchKernelGGL(known_compose_wrap_kernel<true>, dim3(sweep_blocks(n4)), dim3(256), 0, (hipStream_t)stream, x, x0, mask,
                       keyed_draws_of(row_keys, seed, E3D_KNOWN_STREAM_STRUCT, F), level_table, t_dev, T, scale, n4, 4 * n4);
    return e3d_launch_status("e3d_keyed_known_compose_wrap");
}

extern "C" int e3d_discrete_known_compose(int32_t* idx, const int32_t* x0_idx, const uint8_t* mask, const float* Qsb,
                                          const float* u, int mode, int B, int L, int C, void* stream) {
    E3D_REQUIRE(idx && x0_idx && mask && Qsb && B > 0 && L > 0, "discrete_known_compose: bad arguments");
    REQUIRE_CLASSES("discrete_known_compose", 2, C);
    REQUIRE_MODE("discrete_known_compose", mode, u);
    const int64_t n = (int64_t)B * L;
    hipLaunchKernelGGL(discrete_known_compose_kernel<false>, dim3(row_blocks(n)), dim3(256), 0,
                       (hipStream_t)stream, idx, x0_idx, mask, Qsb, u, mode, L, C, n, nullptr, 0ull, nullptr);
    return e3d_launch_status("e3d_discrete_known_compose");
}

extern "C" int e3d_keyed_discrete_known_compose(int32_t* idx, const int32_t* x0_idx, const uint8_t* mask,
                                                const float* Qsb, const int64_t* row_keys, uint64_t seed,
                                                const int64_t* s_dev, int B, int L, int C, void* stream) {
    E3D_REQUIRE(idx && x0_idx && mask && Qsb && row_keys && s_dev && B > 0 && L > 0,
                "keyed_discrete_known_compose: bad arguments");
    REQUIRE_CLASSES("keyed_discrete_known_compose", 2, C);
    const int64_t n = (int64_t)B * L;
    hipLaunchKernelGGL(discrete_known_compose_kernel<true>, dim3(row_blocks(n)), dim3(256), 0,
                       (hipStream_t)stream, idx, x0_idx, mask, Qsb, nullptr, 1, L, C, n, row_keys, seed, s_dev);
    return e3d_launch_status("e3d_keyed_discrete_known_compose");
}

// ---------------------------------------------------------------- design controls (entry points)
// inv_temp must be a positive finite number (NaN fails the first comparison)
static bool good_inv_temp(float inv_temp) { return inv_temp > 0.f && inv_temp <= 3.402823466e38f; }

extern "C" int e3d_discrete_posterior_sample_ctl(const int32_t* xt_idx, const float* logits, const float* bias,
                                                 float inv_temp, const float* Qsb, const float* Qtb, const float* u,
                                                 int mode, int32_t* out_idx, float* prob_out, int B, int L, int C,
                                                 void* stream) {
    E3D_REQUIRE(xt_idx && logits && Qsb && Qtb && out_idx && B > 0 && L > 0, "discrete_posterior_ctl: bad arguments");
    REQUIRE_CLASSES("discrete_posterior_ctl", 1, C);
    E3D_REQUIRE(good_inv_temp(inv_temp), "discrete_posterior_ctl: inv_temp must be positive and finite (inv_temp=%g)",
                (double)inv_temp);
    REQUIRE_MODE("discrete_posterior_ctl", mode, u);
    hipLaunchKernelGGL((discrete_posterior_kernel<false, true>), dim3(B), dim3(256), 0, (hipStream_t)stream, xt_idx, logits,
                       Qsb, Qtb, u, mode, out_idx, prob_out, L, C, nullptr, 0ull, nullptr, bias, inv_temp);
    return e3d_launch_status("e3d_discrete_posterior_sample_ctl");
}

extern "C" int e3d_keyed_discrete_posterior_sample_ctl(const int32_t* xt_idx, const float* logits, const float* bias,
                                                       float inv_temp, const float* Qsb, const float* Qtb,
                                                       const int64_t* row_keys, uint64_t seed, const int64_t* s_dev,
                                                       int32_t* out_idx, int B, int L, int C, void* stream) {
    E3D_REQUIRE(xt_idx && logits && Qsb && Qtb && row_keys && s_dev && out_idx && B > 0 && L > 0,
                "keyed_discrete_posterior_ctl: bad arguments");
    REQUIRE_CLASSES("keyed_discrete_posterior_ctl", 1, C);
    E3D_REQUIRE(good_inv_temp(inv_temp), "keyed_discrete_posterior_ctl: inv_temp must be positive and finite (inv_temp=%g)",
                (double)inv_temp);
    hipLaunchKernelGGL((discrete_posterior_kernel<true, true>), dim3(B), dim3(256), 0, (hipStream_t)stream, xt_idx, logits,
                       Qsb, Qtb, nullptr, 1, out_idx, nullptr, L, C, row_keys, seed, s_dev, bias, inv_temp);
    return e3d_launch_status("e3d_keyed_discrete_posterior_sample_ctl");
}

extern "C" int e3d_discrete_final_pick(const float* logits, const float* bias, float inv_temp, int32_t* out_idx,
                                       float* logp, float* entropy, int64_t rows, int C, void* stream) {
    E3D_REQUIRE(logits && out_idx && rows > 0, "discrete_final_pick: bad arguments");
    E3D_REQUIRE(rows <= (int64_t)2147483647 * 256,"discrete_final_pick: too many rows (rows=%lld)", (long long)rows);
    REQUIRE_CLASSES("discrete_final_pick", 1, C);
    E3D_REQUIRE(good_inv_temp(inv_temp), "discrete_final_pick: inv_temp must be positive and finite (inv_temp=%g)",
                (double)inv_temp);
    hipLaunchKernelGGL(discrete_final_pick_kernel, dim3(row_blocks(rows)), dim3(256), 0, (hipStream_t)stream,
                       logits, bias, inv_temp, out_idx, logp, entropy, rows, C);
    return e3d_launch_status("e3d_discrete_final_pick");
}

// ---------------------------------------------------------------- scoring supplied sequences (entry points)
extern "C" int e3d_keyed_discrete_forward_levels(const int32_t* x0_idx, const float* Qtb, const int64_t* row_keys,
                                                 const int64_t* level_steps, int max_step, uint64_t seed,
                                                 int32_t* out_idx, int N, int L, int C, void* stream) {
    E3D_REQUIRE(x0_idx && Qtb && row_keys && level_steps && out_idx && N > 0 && L > 0,
                "keyed_discrete_forward_levels: bad arguments");
    E3D_REQUIRE(max_step >= 0 && max_step <= 65535,
                "keyed_discrete_forward_levels: keyed streams hold steps up to 65535 (max_step=%d)", max_step);
    E3D_REQUIRE(L <= 1 << 24, "keyed_discrete_forward_levels: positions must stay below 2^24 (L=%d)", L);
    REQUIRE_CLASSES("keyed_discrete_forward_levels", 2, C);
    const int64_t n = (int64_t)N * L;
    hipLaunchKernelGGL(discrete_forward_levels_kernel, dim3(row_blocks(n)), dim3(256), 0, (hipStream_t)stream, x0_idx, Qtb,
                       row_keys, level_steps, max_step, seed, out_idx, L, C, n);
    return e3d_launch_status("e3d_keyed_discrete_forward_levels");
}

extern "C" int e3d_discrete_score_rows(const int32_t* xt_idx, const int32_t* x0_idx, const float* logits, const float* Qsb,
                                       const float* Qtb, const uint8_t* is_final, float* term, float* nll, float* p_out,
                                       float* q_out, int N, int L, int C, void* stream) {
    E3D_REQUIRE(xt_idx && x0_idx && logits && Qsb && Qtb && is_final && term && nll && N > 0 && L > 0,
                "discrete_score_rows: bad arguments");
    REQUIRE_CLASSES("discrete_score_rows", 2, C);
    hipLaunchKernelGGL(discrete_score_rows_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, xt_idx, x0_idx, logits, Qsb,
                       Qtb, is_final, term, nll, p_out, q_out, L, C);
    return e3d_launch_status("e3d_discrete_score_rows");
}

extern "C" int e3d_masked_item_sums(const float* values, const uint8_t* mask, float* sums, int32_t* counts, int N, int L,
                                    void* stream) {
    E3D_REQUIRE(values && mask && sums && counts && N > 0 && L > 0, "masked_item_sums: bad arguments");
    hipLaunchKernelGGL(masked_item_sums_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, values, mask, sums, counts, L);
    return e3d_launch_status("e3d_masked_item_sums");
}

// ---------------------------------------------------------------- scoring supplied structures (entry points)
extern "C" int e3d_keyed_q_sample_levels_wrap(const float* x0, const int64_t* row_keys, const int64_t* level_steps,
                                              int max_step, const float* sqrt_ab, const float* sqrt_1mab, int T, float scale,
                                              uint64_t seed, float* noise_out, float* xt_out, int N, int B, int L, int F,
                                              void* stream) {
    E3D_REQUIRE(x0 && row_keys && level_steps && sqrt_ab && sqrt_1mab && noise_out && xt_out && N > 0 && B > 0 && L > 0 && T > 0,
                "keyed_q_sample_levels_wrap: bad arguments");
    E3D_REQUIRE(N % B == 0, "keyed_q_sample_levels_wrap: N must be a multiple of B (N=%d, B=%d)", N, B);
    E3D_REQUIRE(max_step >= 0 && max_step <= 65535,
                "keyed_q_sample_levels_wrap: keyed streams hold steps up to 65535 (max_step=%d)", max_step);
    E3D_REQUIRE(L <= 1 << 24, "keyed_q_sample_levels_wrap: positions must stay below 2^24 (L=%d)", L);
    REQUIRE_KEYED_WIDTH("keyed_q_sample_levels_wrap", F);
    REQUIRE_ALIGNED16("keyed_q_sample_levels_wrap", x0, noise_out, xt_out);
    const int64_t item4 = (int64_t)L * (F / 4), n4 = (int64_t)N * item4;
    hipLaunchKernelGGL(keyed_q_sample_levels_wrap_kernel, dim3(sweep_blocks(n4)), dim3(256), 0, (hipStream_t)stream, x0,
                       row_keys, level_steps, max_step, sqrt_ab, sqrt_1mab, T, scale, seed, noise_out, xt_out, item4,
                       (int64_t)B * item4, F / 4, n4);
    return e3d_launch_status("e3d_keyed_q_sample_levels_wrap");
}

extern "C" int e3d_angle_score_items(const float* eps_hat, const float* eps, const uint8_t* mask, const int64_t* level_steps,
                                     const float* coef, int T, float* term, float* err, float* res_term, float* res_err2,
                                     float* feat_term, float* feat_err2, float* tot_term, float* tot_err2, int32_t* counts,
                                     int N, int B, int L, int F, void* stream) {
    E3D_REQUIRE(eps_hat && eps && mask && level_steps && coef && tot_term && tot_err2 && counts && N > 0 && B > 0 && L > 0 &&
                    T > 0,
                "angle_score_items: bad arguments");
    E3D_REQUIRE(N % B == 0, "angle_score_items: N must be a multiple of B (N=%d, B=%d)", N, B);
    E3D_REQUIRE(F > 0 && F % 4 == 0 && F <= SCORE_FMAX, "angle_score_items: F must be a multiple of 4 in [4, %d] (F=%d)",
                SCORE_FMAX, F);
    E3D_REQUIRE(aligned16({eps_hat, eps, term, err}) && ((uintptr_t)mask % 4) == 0,
                "angle_score_items: eps_hat, eps, term, err must be 16B and mask 4B aligned");
    hipLaunchKernelGGL(angle_score_items_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, eps_hat, eps, mask, level_steps,
                       coef, T, term, err, res_term, res_err2, feat_term, feat_err2, tot_term, tot_err2, counts, B, L, F / 4);
    return e3d_launch_status("e3d_angle_score_items");
}
