/*
 * e3d_hip.h -- C-ABI of the MI355X (gfx950) denoising hot path.
 *
 * The reference (LabJunBMI/E3-invaraint-diffusion-model) is pure Python and exposes no
 * FFI/plugin interface of its own; its seam is the Python call
 * surface of structure_model/{model,sample}.py and sequence_model/{model,sample}.py.  This
 * header is therefore the boundary the reference-side binding (ctypes)
 * would load: plain pointers and sizes, no torch types.  Each entry point cites the
 * reference lines (relative to /root/reference) whose arithmetic it replaces.
 *
 * Conventions
 *   - every pointer is DEVICE memory (HBM), fp32 row-major unless stated, 16-byte aligned;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing
 *     synchronises with the host and nothing is allocated;
 *   - return value: 0 = enqueued, <0 = argument error (message via e3d_last_error()),
 *     >0 = hipError_t from the launch.
 */
#ifndef E3D_HIP_H
#define E3D_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define E3D_ABI_VERSION 5

/* ``terms`` of the split-operand entry points: how an fp32 operand enters the 16-bit matrix cores.
 *   3  (bf16x3): 2 bf16 terms, 3 cross products, ~2^-17 per product, fp32 exponent range;
 *   6  (bf16x6): 3 bf16 terms, 6 cross products, ~2^-24 (fp32 grade), fp32 exponent range;
 *   19 (f16x3):  2 fp16 terms (11 bits each), 3 cross products, ~2^-21 per product -- fp32 grade at the cost of
 *                bf16x3 -- for operands inside the fp16 range: |x| < 65504 (larger values become inf, i.e. the result is
 *                NaN/inf, never silently wrong), elements below 2^-14 carry an ABSOLUTE error of 2^-25.  Forward
 *                (K-contiguous) GEMM layout and the cooperative attention kernel; other paths run bf16x6. */
#define E3D_TERMS_BF16 1   /* plain bf16 products (RNE operands, ~2^-8), fp32 accumulate: the reference's TRAINING precision
                            * (torch.set_float32_matmul_precision("medium"), structure_model/train_model.py:120); GEMM entry
                            * points only, opt-in (E3D_TRAIN_ARITHMETIC=bf16) -- never an inference default */
#define E3D_TERMS_BF16X3 3
#define E3D_TERMS_BF16X6 6
#define E3D_TERMS_F16X3 19

#define E3D_ACT_NONE 0
#define E3D_ACT_GELU 1 /* exact erf GELU: transformers get_activation("gelu"), nn.GELU() */
#define E3D_ACT_SILU 2 /* nn.SiLU in SELayer.adaLN_modulation, structure_model/model.py:34 */

int e3d_abi_version(void);
const char* e3d_last_error(void);

/* out[M,N] = act(A[M,K] @ W[N,K]^T + bias[N]) -- every nn.Linear of the path
 * (BertSelfAttention query/key/value, BertSelfOutput.dense, BertIntermediate, BertOutput:
 * transformers 4.38.2 modeling_bert.py; SELayer.adaLN_modulation / mlp:
 * structure_model/model.py:32-47; predictor dense1: structure_model/model.py:149-151).
 * lda/ldc are row strides in elements.  Requires N % 128 == 0, K % 32 == 0.  bias may be NULL. */
int e3d_gemm_bias_act_f32(const float* A, int64_t lda, const float* W, const float* bias,
                          float* out, int64_t ldc, int M, int N, int K, int act, void* stream);

/* Same contract as e3d_gemm_bias_act_f32, computed on the bf16 matrix cores with each fp32
 * operand split into 2 (terms = 3 cross products) or 3 (terms = 6) bf16 terms and fp32
 * accumulation: fp32-grade results (terms = 6: ~2^-24 per product; terms = 3: ~2^-17) at 6/16 or
 * 3/16 of the exact kernel's MFMA cost. */
int e3d_gemm_bias_act_f32_split(const float* A, int64_t lda, const float* W, const float* bias,
                                float* out, int64_t ldc, int M, int N, int K, int act, int terms,
                                void* stream);

/* e3d_gemm_bias_act_f32_split that also reports the largest |out| it wrote: ``out_absmax`` (device, one float, may be
 * NULL) is raised atomically to max(*out_absmax, max |out[m][n]|) -- never lowered, so the caller zeroes it when it wants
 * a fresh figure; a NaN / inf output leaves a NaN / inf there.  act must be E3D_ACT_NONE when out_absmax is given.
 * Purpose: the bounds of e3d_relkey_attn_fwd_split_ex (below), which let the attention kernels skip all-padding key
 * tiles only when that is provably exact.  Costs two integer VALU operations per output element.
 * ``out_scale``: out = act(out_scale * (A W^T) + bias).  For terms = 19 (f16x3) a caller hands in W * 2^k (exact) with k
 * chosen so that max |W| 2^k sits near 2^12, and out_scale = 2^-k (exact): both fp16 terms of every weight element down
 * to 2^-15 of the largest are then normal numbers (22 bits), instead of an absolute 2^-25 floor below 2^-14 -- a
 * uniformly tiny weight (|w| ~ 1e-6) goes from ~2e-2 to fp32-grade relative error -- and a weight beyond the fp16 range
 * cannot overflow.  1.0f = the plain product (bit-identical to e3d_gemm_bias_act_f32_split). */
int e3d_gemm_bias_act_f32_split_ex(const float* A, int64_t lda, const float* W, const float* bias, float* out,
                                   int64_t ldc, int M, int N, int K, int act, int terms, float* out_absmax,
                                   float out_scale, void* stream);
/* The _ex entry point with two more arguments, for launches whose rows may already be known from a table
 * (SELayer conditioning on one-hot residue rows, blocks.onehot_modulation):
 * ``plan_m`` > 0: the kernel form is chosen as for a launch of plan_m rows (0: by M, as the _ex entry point does).  A
 *   tile's result does not depend on which other row blocks the launch has, so a few rows computed apart with
 *   plan_m = M_dense equal the same rows of the M_dense-row launch bit for bit.
 * ``run_if`` (device, one int, may be NULL): every workgroup reads the word first and returns when it is zero -- the
 *   launch then costs an empty dispatch and ``out`` is not written. */
int e3d_gemm_bias_act_f32_split_gated(const float* A, int64_t lda, const float* W, const float* bias, float* out,
                                      int64_t ldc, int M, int N, int K, int act, int terms, float* out_absmax,
                                      float out_scale, int plan_m, const int* run_if, void* stream);
/* target = max(target, max_i |x[i]|), same conventions (distance-embedding tables, test aids). */
int e3d_absmax_f32(const float* x, int64_t n, float* target, void* stream);

/* Fused attention, head dim 64 ("edge aggregation" of the north star):
 *   S = (Q K^T + R) / sqrt(64) + (1 - key_mask) * -10000;  out = softmax(S) V
 *   R[l,r] = q_l . dist_emb[l - r + P - 1]   (relative_key, only when dist_emb != NULL)
 * Replaces transformers 4.38.2 BertSelfAttention.forward as called from
 * structure_model/model.py:40,62,197-213 and sequence_model/model.py:39,226-235, plus
 * _exetend_attention_mask (structure_model/model.py:226-231).
 *   q: token (b,l) head h at q + b*q_bs + l*q_rs + h*64 (element strides), same for k, v;
 *   key_mask [B,Lk] holds 1.0/0.0 (NULL = all ones); out [B,Lq,nh*64];
 *   lse (optional, [B,nh,Lq]) receives log-sum-exp of S rows for the backward pass.
 * Requires Lq,Lk >= 1; with dist_emb: Lq == Lk <= P and dist_emb is [2P-1,64]. */
int e3d_relkey_attn_fwd(const float* q, int64_t q_bs, int64_t q_rs,
                        const float* k, int64_t k_bs, int64_t k_rs,
                        const float* v, int64_t v_bs, int64_t v_rs,
                        const float* dist_emb, int P, const float* key_mask,
                        float* out, float* lse, int B, int nh, int Lq, int Lk, void* stream);

/* Same contract as e3d_relkey_attn_fwd on the bf16 matrix cores: K, E, Q, V and the softmax
 * probabilities enter the MFMAs as 2 (terms = 3) or 3 (terms = 6, fp32-grade) bf16 split terms,
 * accumulation, softmax and the rel-key skew stay fp32.
 * Softmax exponential: exp(x) is evaluated as exp2(x * log2(e)) on the hardware v_exp_f32 (<= 1 ulp of fp32
 * exp2; the product x * log2(e) rounds once more), not libm expf -- inside the 1e-4 contract
 * (tests/test_kernels_gpu.py), stated here because SURVEY H2 asks for it.  The exact-fp32 entry point above
 * (e3d_relkey_attn_fwd) uses libm expf.
 * This entry point takes no scratch and never allocates: rel-key calls run the per-wave kernel.  The faster
 * workgroup-cooperative kernel needs the distance table as bf16 planes in caller-provided memory -- bind
 * e3d_relkey_attn_fwd_split_ex (below) for that. */
int e3d_relkey_attn_fwd_split(const float* q, int64_t q_bs, int64_t q_rs,
                              const float* k, int64_t k_bs, int64_t k_rs,
                              const float* v, int64_t v_bs, int64_t v_rs,
                              const float* dist_emb, int P, const float* key_mask,
                              float* out, float* lse, int B, int nh, int Lq, int Lk, int terms,
                              void* stream);

/* The same product for small launches (one to ~16 pockets per step: BASELINE configs[0]; M <= 4096 accepted, the host mirror
 * sends up to ~768 output tiles of 32x32 here, where it beats the tiled kernels), cut along K as well so
 * that the whole chip streams the weight: one wave per (32 rows, 32 columns, K slice) writes a partial tile into the
 * workspace, a second small launch sums the slices in slice order (deterministic) and applies bias and activation.
 * Two launches on the given stream.  terms = 3 (bf16x3) or 19 (f16x3).  N % 32 == 0, K % 16 == 0, lda % 4 == 0,
 * ldc % 4 == 0; A, W, bias, out 16-byte aligned.
 * ``workspace``: device memory of >= e3d_gemm_skinny_workspace_bytes(M, N, K) bytes, 16-byte aligned, no initialisation
 * needed, not shared by launches that may run concurrently (one per stream). */
int64_t e3d_gemm_skinny_workspace_bytes(int M, int N, int K);
int e3d_gemm_skinny_f32_split(const float* A, int64_t lda, const float* W, const float* bias, float* out,
                              int64_t ldc, int M, int N, int K, int act, int terms, void* workspace,
                              int64_t workspace_bytes, void* stream);
/* ... with the |out| maximum and the accumulator scale of e3d_gemm_bias_act_f32_split_ex (``out_absmax`` may be NULL;
 * act = none when given; out_scale = 1.0f: the plain product). */
int e3d_gemm_skinny_f32_split_ex(const float* A, int64_t lda, const float* W, const float* bias, float* out,
                                 int64_t ldc, int M, int N, int K, int act, int terms, void* workspace,
                                 int64_t workspace_bytes, float* out_absmax, float out_scale, void* stream);
/* Diagnostic switch (A/B timing, tools/lab/skinny_ab.py): the K-slicing plan of the kernels above -- waves per CU the
 * plan aims for (times 2; default 3 = 1.5 per CU) and the shortest K slice (default 96).  Query the workspace size AFTER
 * changing the plan.  Results differ between plans only by fp32 summation order. */
void e3d_gemm_skinny_plan_select(int waves_per_cu_x2, int min_k_slice);
/* BertSelfOutput / BertOutput in one call (transformers 4.38.2 modeling_bert.py: dense -> dropout(eval: identity) ->
 * LayerNorm(hidden + input)):  out[M,H] = LayerNorm(A . W^T + bias + residual) * gamma + beta, the second launch of the
 * product above doing the row finish.  Bit-identical to e3d_gemm_skinny_f32_split followed by
 * e3d_residual_layernorm_fwd.  H in {256, 512, 768, 1024}; out is contiguous [M,H]; residual may be NULL. */
int e3d_gemm_skinny_residual_layernorm_f32_split(const float* A, int64_t lda, const float* W, const float* bias,
                                                 const float* residual, const float* gamma, const float* beta, float eps,
                                                 float* out, int M, int H, int K, int terms, void* workspace,
                                                 int64_t workspace_bytes, void* stream);
/* ... with out_scale: LayerNorm(out_scale * (A W^T) + bias + residual). */
int e3d_gemm_skinny_residual_layernorm_f32_split_ex(const float* A, int64_t lda, const float* W, const float* bias,
                                                    const float* residual, const float* gamma, const float* beta,
                                                    float eps, float* out, int M, int H, int K, int terms,
                                                    void* workspace, int64_t workspace_bytes, float out_scale,
                                                    void* stream);

/* Diagnostic switch (A/B timing, tools/bench_kernels.py): which kernel form serves large-M forward launches of
 * e3d_gemm_bias_act_f32_split with terms = 3 -- 4 = persistent 256x256 (default), 3 = 256x256 with interleaved
 * staging, 1 = classic 256x256 loop, 0 = 256x128, 5 = persistent whatever the tile count (experiments).  Results are identical in every form (same products, same
 * accumulation order).  pref < 0 only queries.  Returns the previous value. */
int e3d_gemm_kernel_select(int pref);
/* The same for the general kernel (every launch the persistent / 256x256 forms do not take: medium and small M, the
 * training layouts): 0 = by shape (default), 1 = 256x128 tiles (8 waves), 2 = 128x128 (4 waves), 3 = 128x128 on 8 waves,
 * 4 = 128x64 on 4 waves (48 KB of LDS: up to three workgroups per CU; forward / input-gradient layout of the 2-term
 * arithmetics, other layouts fall back to 3).  Identical results in every form (up to the order of the split-K atomics of
 * the weight-gradient layout).  form < 0 only queries. */
int e3d_gemm_general_select(int form);

/* Diagnostic (tests/test_kernels_gpu.py): the cooperative bf16x3 attention kernel keeps its running softmax maximum
 * until a key tile exceeds it by more than 2^tau (default tau = 8, log2 units; results are mathematically
 * unchanged -- O and the row sum stay relative to the same maximum).  tau = 0 restores the classic online softmax
 * (rescale on every new maximum).  tau < 0 only queries.  Returns the previous value. */
float e3d_attn_rescale_tau(float tau);

/* Process-wide switch of the split attention kernels (default 1): stop the key sweep after the tile
 * holding the last valid key of the item WHEN the call's element bounds (q_absmax / k_absmax / e_absmax of
 * e3d_relkey_attn_fwd_split_ex) prove that trailing all-padding tiles contribute exp(s - 10000 - m) = 0.0f exactly --
 * the reference masks additively (structure_model/model.py:226-231), so that holds only while the scores of a row
 * spread over less than ~9900: 16 qa (ka + ea) < 9890.  Results are then bit-identical to the dense sweep; calls
 * without bounds, or whose bounds do not prove it, always run the dense sweep.  0 = dense sweep for every call
 * (timing comparisons).  Returns the previous setting. */
int e3d_attn_skip_padded_tiles(int enable);

/* out[M,H] = LayerNorm_eps(x[M,H] (+ residual[M,H])) * gamma + beta
 * -- BertSelfOutput / BertOutput (4.38.2) with the dense bias already added by the GEMM,
 * and predictor.layer_norm (structure_model/model.py:152).  residual may be NULL.
 * s_out (may be NULL) receives the pre-norm rows x + residual that the backward needs.
 * H must be 256, 512, 768 or 1024. */
int e3d_residual_layernorm_fwd(const float* x, const float* residual, const float* gamma,
                               const float* beta, float eps, float* s_out, float* out, int M,
                               int H, void* stream);

/* SELayer gated branch (structure_model/model.py:61-67):
 *   out = x + gate * (LayerNorm_1e-5_noaffine(y) * (1 + scale) + shift)
 * mod is the adaLN_modulation output [Mc, 6H]; (shift,scale,gate) are chunks
 * (3*branch, 3*branch+1, 3*branch+2) with branch 0 = msa, 1 = mlp.  Row m of x uses row
 * m / rows_per_cond of mod (rows_per_cond = L when c is [B,1,H], 1 when c is [B,L,H]). */
int e3d_adaln_gate_fwd(const float* x, const float* y, const float* mod, int branch,
                       int rows_per_cond, float* out, int M, int H, void* stream);

/* The gate with the modulation row looked up: row m takes (shift, scale, gate) from table[idx[m]] ([table_rows, 6H]) when
 * 0 <= idx[m] < table_rows, from mod[m] ([M, 6H], rows_per_cond = 1) otherwise.  Arithmetic per row as above. */
int e3d_adaln_gate_indexed_fwd(const float* x, const float* y, const int* idx, const float* table, int table_rows,
                               const float* mod, int branch, float* out, int M, int H, void* stream);

/* Rows of one-hot features (a residue type per pocket row, or a padding row of zeros): idx[m] = k when row m of x [M,F]
 * is exactly 1.0f at position k and +0.0f / -0.0f elsewhere, F when every element is zero, -1 otherwise (NaN included).
 * *flag (device, one int, zeroed by the caller) is set non-zero when any row got -1.  F <= 32. */
int e3d_classify_onehot_rows(const float* x, int F, int* idx, int* flag, int M, void* stream);

/* BertEmbeddings (structure_model/model.py:111-118, eval):
 *   out[M,H] = LayerNorm_eps(x[M,F] @ W[H,F]^T + b) * gamma + beta (+ post_add[m / rows_per_add])
 * post_add ([M / rows_per_add, H], may be NULL) is the timestep embedding the sequence model
 * adds after the embedding (sequence_model/model.py:213,220).  F <= 32.  z_out (may be NULL)
 * receives the pre-LayerNorm rows x W^T + b that the backward needs. */
int e3d_embed_layernorm_fwd(const float* x, int F, const float* W, const float* b,
                            const float* gamma, const float* beta, float eps,
                            const float* post_add, int rows_per_add, float* z_out, float* out,
                            int M, int H, void* stream);
/* ... with ``run_if`` of e3d_gemm_bias_act_f32_split_gated. */
int e3d_embed_layernorm_fwd_ex(const float* x, int F, const float* W, const float* b,
                               const float* gamma, const float* beta, float eps,
                               const float* post_add, int rows_per_add, float* z_out, float* out,
                               int M, int H, const int* run_if, void* stream);

/* predictor.dense2 (structure_model/model.py:153): out[M,Nout] = x[M,H] @ W[Nout,H]^T + b,
 * Nout <= 32 (8 angles / 20 amino-acid logits). */
int e3d_head_linear_fwd(const float* x, const float* W, const float* b, float* out, int M,
                        int H, int Nout, void* stream);

/* One DDPM ancestral update (+ wrap) (structure_model/sample.py:90-99,140-142 and
 * utils.py:20-40):  mean = sqrt_recip_alpha * (x - beta * eps_hat / sqrt_one_minus_ab)
 *   v = mean + sigma * noise   (noise == NULL or sigma == 0: no noise term)
 *   out = wrap ? wrap_[-pi,pi)(v) : v          (p_sample_loop wraps, bare p_sample does not)
 * n = number of elements. */
int e3d_ddpm_step_wrap(const float* x, const float* eps_hat, const float* noise,
                       float sqrt_recip_alpha, float beta, float sqrt_one_minus_ab, float sigma,
                       int wrap, float* out, int64_t n, void* stream);

/* e3d_ddpm_step_wrap with the step index on the device: coefficients are row t_dev[0] of
 * coef_table [T,4] = (sqrt_recip_alpha, beta, sqrt_one_minus_alphas_cumprod, sigma); sigma == 0 (t == 0)
 * skips the noise term exactly like the scalar form.  No host scalar changes from step to step, so a
 * captured hipGraph of the whole reverse step can be replayed (structure_model/sample.py). */
int e3d_ddpm_step_wrap_table(const float* x, const float* eps_hat, const float* noise,
                             const float* coef_table, const int64_t* t_dev, int wrap, float* out,
                             int64_t n, void* stream);

/* One strided (DDIM / respaced-ancestral) update t -> s < t, the schedule-consistent jump of Song et al. 2021, eqs. 12
 * and 16 (no counterpart in the reference, whose STEP > 1 applies the one-step coefficients).  Per element:
 *   x0 = (x - s1m * eps_hat) * rsa;   wrap_x0: x0 = wrap_[-pi,pi)(x0)   (the angle analogue of clip_denoised)
 *   v  = a_s * x0 + c_dir * eps_hat (+ sigma * noise);   out = wrap ? wrap_[-pi,pi)(v) : v
 * with (s1m, rsa, a_s, c_dir, sigma, 0, 0, 0) = row t_dev[0] of coef_table [T,8] (structure_model/utils.py,
 * StridedTables: sqrt(1 - ab_t), 1 / sqrt(ab_t), sqrt(ab_s), sqrt(1 - ab_s - sigma^2), sigma).  The step index is read
 * on the device, so a captured graph replays it.  noise may be NULL (sigma is then taken as 0); nothing is read through
 * noise when the row's sigma == 0.  t_dev[0] outside [0, T): no table row is read and every output is NaN.  out may
 * alias x.  n = number of elements. */
int e3d_strided_step_wrap(const float* x, const float* eps_hat, const float* noise, const float* coef_table,
                          const int64_t* t_dev, int T, int wrap, int wrap_x0, float* out, int64_t n, void* stream);

/* One second-order multistep update t -> s < t: DPM-Solver++(2M) of Lu et al. 2022 in its data-prediction form, with
 * the extrapolation weight capped (structure_model/utils.py, MultistepTables).  It is the strided update at eta = 0 plus
 * one term built from the x0 estimate that the previous step stored; it draws nothing.  Per element:
 *   x0 = (x - s1m * eps_hat) * rsa;   wrap_x0: x0 = wrap_[-pi,pi)(x0)
 *   v  = a_s * x0 + c_dir * eps_hat
 *   c_1 != 0:  d = x0 - hist_in;   wrap: d = wrap_[-pi,pi)(d);   v = v + c_1 * d
 *   hist_out = x0;   out = wrap ? wrap_[-pi,pi)(v) : v
 * with (s1m, rsa, a_s, c_dir, c_1, 0, 0, 0) = row t_dev[0] of coef_table [T,8].  A row with c_1 == 0 (the first and the
 * last visited timestep) reads nothing through hist_in and gives the bits of e3d_strided_step_wrap at sigma == 0.
 * t_dev[0] outside [0, T): no table row is read and out and hist_out are NaN.  out may alias x and hist_out may alias
 * hist_in; out and hist_out are two buffers.  All five arrays 16-byte aligned.  n = number of elements. */
int e3d_multistep_step_wrap(const float* x, const float* eps_hat, const float* hist_in, const float* coef_table,
                            const int64_t* t_dev, int T, int wrap, int wrap_x0, float* out, float* hist_out, int64_t n,
                            void* stream);

/* Forward noising q(x_t | x_0) with wrap (structure_model/dataset.py:211-228):
 *   out[b] = wrap(sqrt_ab[t[b]] * x0[b] + sqrt_1mab[t[b]] * noise[b]),  per = elements per item. */
int e3d_q_sample_wrap(const float* x0, const float* noise, const int64_t* t,
                      const float* sqrt_ab, const float* sqrt_1mab, float* out, int B,
                      int64_t per, void* stream);

/* Discrete reverse step p(z_s | z_t) (sequence_model/sample.py:120-179), C = 20 classes:
 *   prob[n,:] = normalise( sum_x0 softmax(logits[n])[x0] * (Qt[b]^T[xt,:] * Qsb[b][x0,:]) / Qtb[b][x0,xt] )
 * with Qt = rownorm(Qsb/Qtb) computed in-kernel; x_t given as class indices [B*L] (int32; the
 * reference carries one-hots).  mode 0: argmax (diverse=False); mode 1: inverse-CDF draw with
 * uniforms u[B*L] (diverse=True).  Writes class index out_idx[B*L] and, if prob_out != NULL,
 * prob [B*L,C]. */
int e3d_discrete_posterior_sample(const int32_t* xt_idx, const float* logits, const float* Qsb,
                                  const float* Qtb, const float* u, int mode, int32_t* out_idx,
                                  float* prob_out, int B, int L, int C, void* stream);

/* Forward discrete noising (sequence_model/model.py:291-311): prob[n,:] = Qtb[b][:, x0[n]];
 * x0 index < 0 marks a padding (all-zero one-hot) row -> class 0.  u as above. */
int e3d_discrete_q_sample(const int32_t* x0_idx, const float* Qtb, const float* u, int mode,
                          int32_t* out_idx, int B, int L, int C, void* stream);

/* ------------------------------------------------------------------ keyed (seeded) sampling draws
 * Every random number of a seeded chain is Philox4x32-10 of the counter (item id lo, item id hi, stream << 16 | step,
 * position << 8 | block) under the key (seed lo, seed hi), mapped to fp32 from 24-bit fields ("Keyed
 * sampling streams"; csrc/e3d_philox.h).  Streams: 0 structure x_T, 1 structure reverse-step noise, 2 sequence initial
 * one-hot, 3 sequence posterior uniforms (10 and 11: the held positions of a partial redesign, further down).  ``row_keys`` int64 [rows, 2] = (item id, position) per row; a negative
 * position marks a row of no item (a packed buffer's tail), which draws nothing.  The caller guarantees positions
 * < 2^24 and steps <= 65535.  Step indices are read from DEVICE memory (``t_dev`` / ``s_dev``, first element), so a
 * captured graph replays them. */

/* e3d_ddpm_step_wrap_table with the noise generated in-register: row r, features 4j .. 4j+3 take the normals of
 * (seed, row_keys[r], stream 1, t_dev[0], block j).  x / eps_hat / out [rows, F], F % 4 == 0, F <= 1024.  Equals
 * e3d_ddpm_step_wrap_table fed with those normals (zeros on rows of no item); sigma == 0 (t == 0) gives the mean. */
int e3d_keyed_ddpm_step_wrap(const float* x, const float* eps_hat, const float* coef_table, const int64_t* t_dev,
                             const int64_t* row_keys, uint64_t seed, int wrap, float* out, int64_t rows, int F,
                             void* stream);

/* e3d_strided_step_wrap with the noise generated in-register from stream 1 at step t_dev[0], keyed by (item, position,
 * block) -- the stream of e3d_keyed_ddpm_step_wrap, so a pocket's draw at timestep t is the same under either update.
 * Equals e3d_strided_step_wrap fed with those normals; rows of no item get no noise term; sigma == 0 draws nothing.
 * x / eps_hat / out [rows, F], F % 4 == 0, F <= 1024; T <= 65536. */
int e3d_keyed_strided_step_wrap(const float* x, const float* eps_hat, const float* coef_table, const int64_t* t_dev,
                                int T, const int64_t* row_keys, uint64_t seed, int wrap, int wrap_x0, float* out,
                                int64_t rows, int F, void* stream);

/* e3d_discrete_posterior_sample in mode 1 with the uniform of row n = b * L + l drawn from stream 3 at step s_dev[0]
 * with key row_keys[n] (padded [B, L] batches, or a packed buffer as B = 1, L = rows); rows of no item draw u = 0. */
int e3d_keyed_discrete_posterior_sample(const int32_t* xt_idx, const float* logits, const float* Qsb,
                                        const float* Qtb, const int64_t* row_keys, uint64_t seed,
                                        const int64_t* s_dev, int32_t* out_idx, int B, int L, int C, void* stream);

/* Raw keyed draws of one (stream_id, t) for every row of a key table; rows of no item give zeros.
 *   kind 0: normals float [rows, width] (width % 4 == 0); wrap != 0: wrap_[-pi,pi)(scale * z) (stream 0: keyed x_T);
 *   kind 1: uniforms float [rows] (word 0 of block 0);
 *   kind 2: classes in [0, width) from word 0 of block 0, as a float one-hot [rows, width] (stream 2: keyed x_T);
 *   kind 3: the same classes as int32 [rows]. */
int e3d_keyed_draws(const int64_t* row_keys, uint64_t seed, int stream_id, int t, int kind, int width, int wrap,
                    float scale, void* out, int64_t rows, void* stream);

/* ------------------------------------------------------------------ partial redesign (replacement conditioning)
 * Holding chosen ligand positions fixed during a reverse chain (Song et al. 2021, section I.2; Lugmayr et al. 2022,
 * without the resampling loop): after the update that lands the state on noise level s, the held elements are
 * overwritten with a fresh forward-noised copy of their known values at level s; after the last step with the known
 * values themselves.  These are launches of their own, after the update kernel of the step and on its stream: the
 * update kernels, their signatures and their results stay bit for bit, and these entry points are additions to ABI v5. */

/* In place on x [n]: for every element with mask[i] != 0 (uint8, per element), with (a, s1m) = row t_dev[0] of
 * level_table [T,2] (structure_model/utils.py, KnownLevels: the level the state is on AFTER the step at t):
 *   s1m == 0 (the clean level):  x = x0                                (a copy: bit for bit)
 *   otherwise:                   x = wrap_[-pi,pi)(a * x0 + s1m * wrap_[-pi,pi)(scale * noise))
 * -- the arithmetic of e3d_q_sample_wrap on the noise of NoisedAnglesDataset.sample_noise.  t_dev[0] outside [0, T), a
 * NaN row (a timestep the chain does not visit), or noise == NULL at a level with s1m != 0: the held elements become NaN.
 * Elements with mask == 0 are not written.  x, x0, noise 16 B aligned, mask 4 B aligned. */
int e3d_known_compose_wrap(float* x, const float* x0, const uint8_t* mask, const float* noise, const float* level_table,
                           const int64_t* t_dev, int T, float scale, int64_t n, void* stream);

/* The same with the normals generated in-register: row r, features 4j .. 4j+3 take those of (seed, row_keys[r], stream
 * 10, t_dev[0], block j), the block layout of stream 1.  Equals e3d_known_compose_wrap fed with those normals.  Rows of
 * no item are left alone; a group of four features with no held element makes no Philox call.  x / x0 / mask [rows, F],
 * F % 4 == 0, F <= 1024; T <= 65536. */
int e3d_keyed_known_compose_wrap(float* x, const float* x0, const uint8_t* mask, const float* level_table,
                                 const int64_t* t_dev, int T, float scale, const int64_t* row_keys, uint64_t seed,
                                 int64_t rows, int F, void* stream);

/* Sequence chain, in place on the class indices idx [B*L] that e3d_discrete_posterior_sample wrote: a row n with
 * mask[n] != 0 and 0 <= x0_idx[n] < C is redrawn from prob[c] = Qsb[b][c][x0_idx[n]] (b = n / L), the convention and
 * arithmetic of e3d_discrete_q_sample at the level the step lands on.  mode 0: argmax; mode 1: inverse-CDF draw with
 * u [B*L].  Every other row is left alone. */
int e3d_discrete_known_compose(int32_t* idx, const int32_t* x0_idx, const uint8_t* mask, const float* Qsb,
                               const float* u, int mode, int B, int L, int C, void* stream);

/* The same in mode 1 with the uniform of row n taken from word 0 of stream 11 at step s_dev[0] with key row_keys[n]
 * (a packed buffer: B = 1, L = rows); rows of no item are left alone. */
int e3d_keyed_discrete_known_compose(int32_t* idx, const int32_t* x0_idx, const uint8_t* mask, const float* Qsb,
                                     const int64_t* row_keys, uint64_t seed, const int64_t* s_dev, int B, int L,
                                     int C, void* stream);

/* ------------------------------------------------------------------ sequence design controls
 * Temperature, per-position residue bias and design scores of the sequence chain.  The controls shape the model's x0
 * prediction: wherever the posterior kernel takes softmax(logits[n]) it takes softmax(z[n]) instead, with the
 * EFFECTIVE LOGITS
 *   z[n,c] = (logits[n,c] + bias[n,c]) * inv_temp        (fp32: one add, then one multiply, never fused)
 * bias float [B*L, C] or NULL for zero; bias == -inf forbids class c at row n; inv_temp = 1 / temperature > 0, by
 * value.  A forbidden class has probability exactly 0 in the x0 prediction, so it contributes nothing to the posterior.
 * The intermediate states z_s are noisy by construction (the forward law Qsb spreads every class) and may pass through
 * a forbidden class; the guarantee is on the chain's OUTPUT, which the final-pick entry point below takes as the argmax
 * of z: it never holds a forbidden class.  The temperature therefore acts on the steps s > 0 only.  No new random
 * stream: the keyed form draws stream 3 with the counters of the entry point it extends.  These entry points are
 * additions to ABI v5; the two posterior entry points above share the kernel body and keep their results bit for bit. */

/* The posterior of the reverse step over the effective logits; every other argument, the arithmetic and the launch
 * shape are those of the entry point without controls.  A row whose classes are all forbidden takes an all-zero x0
 * prediction and hence the zero-total rule (1e-5 per class, i.e. 1 / C after the normalisation): never NaN.
 * C in [1, 32]; inv_temp must be positive and finite. */
int e3d_discrete_posterior_sample_ctl(const int32_t* xt_idx, const float* logits, const float* bias, float inv_temp,
                                      const float* Qsb, const float* Qtb, const float* u, int mode, int32_t* out_idx,
                                      float* prob_out, int B, int L, int C, void* stream);

/* The same in mode 1 with the uniforms of the keyed entry point: stream 3 at step s_dev[0] with key row_keys[n], the
 * same counters; rows of no item draw u = 0. */
int e3d_keyed_discrete_posterior_sample_ctl(const int32_t* xt_idx, const float* logits, const float* bias,
                                            float inv_temp, const float* Qsb, const float* Qtb,
                                            const int64_t* row_keys, uint64_t seed, const int64_t* s_dev,
                                            int32_t* out_idx, int B, int L, int C, void* stream);

/* The last step's pick, one thread per row of logits [rows, C]:
 *   out_idx[n] = the first maximum of z[n];   logp[n] = log_softmax(z[n])[out_idx[n]];
 *   entropy[n] = -sum_c p log p of p = softmax(z[n]), a forbidden class counting 0 (0 log 0 = 0).
 * logp and entropy may each be NULL.  A row whose classes are all forbidden: out_idx = 0, logp = entropy = NaN. */
int e3d_discrete_final_pick(const float* logits, const float* bias, float inv_temp, int32_t* out_idx, float* logp,
                            float* entropy, int64_t rows, int C, void* stream);

/* ------------------------------------------------------------------ scoring supplied sequences
 * The variational score of the sampler's own reverse law for a sequence x0 the chain did not sample
 * (sequence_model/sample.py::score_sequences; DESIGN.md, "Scoring sequences").  Levels do not depend on one another, so
 * N = levels x items rows of tables go through one launch each.  Additions to ABI v5.
 *
 * Forward noising of N items at their own levels: row (n, l) of out_idx [N*L] is drawn from
 * prob[c] = Qtb[n][c][x0_idx[n*L + l]], e3d_discrete_q_sample's convention and arithmetic, with the uniform of word 0
 * of stream 11 at the step field level_steps[n] (int64 [N], DEVICE memory) with key row_keys[n*L + l] -- for equal
 * steps, e3d_keyed_discrete_known_compose with a full mask, bit for bit.  max_step <= 65535 is the caller's bound on
 * level_steps.  Class 0 for a row of no item: x0 outside [0, C), a key position outside [0, 2^24), a step outside
 * [0, max_step]. */
int e3d_keyed_discrete_forward_levels(const int32_t* x0_idx, const float* Qtb, const int64_t* row_keys,
                                      const int64_t* level_steps, int max_step, uint64_t seed, int32_t* out_idx, int N,
                                      int L, int C, void* stream);

/* Per-row score terms, one workgroup per item n with Qsb[n], Qtb[n] [C, C] in LDS:
 *   nll[n,l]  = -log_softmax(logits[n,l])[x0]
 *   p         = prob_out of e3d_discrete_posterior_sample on the same inputs, bit for bit
 *   q         = the same expression with the x0 prediction replaced by the one-hot of x0
 *   term[n,l] = KL(q || p) in nats, 0 log 0 = 0; +inf when a class has q > 0 and p == 0; never NaN for a valid row
 * is_final[n] != 0 (uint8 [N]): term = nll, bit for bit, Qsb and Qtb are not read and p_out / q_out get NaN.
 * p_out, q_out [N*L, C] may each be NULL.  A row with x0 or xt outside [0, C): NaN in every output. */
int e3d_discrete_score_rows(const int32_t* xt_idx, const int32_t* x0_idx, const float* logits, const float* Qsb,
                            const float* Qtb, const uint8_t* is_final, float* term, float* nll, float* p_out,
                            float* q_out, int N, int L, int C, void* stream);

/* sums[n] = the sum of values[n, l] over mask[n, l] != 0 and counts[n] their number, one wave per item: lane j adds
 * positions j, j + 64, ... in order (a masked-out position adds an exact +0, whatever its value), then a fixed xor
 * butterfly over the 64 lanes.  No atomics; the result is a function of the item's (position, value) pairs alone, the
 * same bits for any L >= the last set position and in any batch. */
int e3d_masked_item_sums(const float* values, const uint8_t* mask, float* sums, int32_t* counts, int N, int L,
                         void* stream);

/* ------------------------------------------------------------------ scoring supplied structures
 * The score of the structure sampler's own reverse law for backbone angles x0 the chain did not sample
 * (structure_model/sample.py::score_structures; DESIGN.md, "Scoring structures").  Levels do not depend on one another,
 * so N = n * B items (n levels of the B supplied items, level-major: item i is item i % B at level i / B) go through one
 * launch each.  Additions to ABI v5.
 *
 * Forward noising of the N items at their own levels with the noise drawn in-register from stream 12:
 *   noise_out = wrap(scale * z),  xt_out = wrap(sqrt_ab[t] * x0 + sqrt_1mab[t] * noise_out),  t = level_steps[i]
 * (the arithmetic of e3d_q_sample_wrap and e3d_keyed_q_sample_wrap), z the normals of (seed, row key, stream 12, step t,
 * block j -> features 4j .. 4j+3, the block layout of stream 1).  x0 [B, L, F] and row_keys [B*L, 2] are given once: item
 * i reads those of item i % B.  level_steps int64 [N] in DEVICE memory; max_step <= 65535 is the caller's bound on it.
 * noise_out, xt_out [N, L, F].  A row of no item (a key position outside [0, 2^24)) gets zeros in both outputs; an item
 * whose step lies outside [0, min(max_step, T - 1)] gets NaN in both and reads no table row.  F % 4 == 0, F <= 1024,
 * N % B == 0. */
int e3d_keyed_q_sample_levels_wrap(const float* x0, const int64_t* row_keys, const int64_t* level_steps, int max_step,
                                   const float* sqrt_ab, const float* sqrt_1mab, int T, float scale, uint64_t seed,
                                   float* noise_out, float* xt_out, int N, int B, int L, int F, void* stream);

/* Per-element score terms of N items and their fixed-shape sums, one wave per item.  With (k, h, add, 0) = row
 * level_steps[i] of coef [T, 4] (structure_model/utils.py, ScoreTables), per element in fp32, every product rounded
 * before it is added to:
 *   err   = wrap_[-pi,pi)(eps - eps_hat)
 *   delta = wrap_[-pi,pi)(k * (eps_hat - eps));   term = h * (delta * delta) + add
 * eps_hat, eps [N, L, F]; mask uint8 [B, L, F], per element, read as item i % B; level_steps int64 [N], DEVICE memory.
 * Outputs (term, err, res_*, feat_* may each be NULL): term, err [N, L, F] (every element, masked or not);
 * res_term, res_err2 [N, L]; feat_term, feat_err2 [N, F]; tot_term, tot_err2 [N]: sums of term and of err * err over
 * the elements with mask != 0; counts int32 [N]: their number.
 * Reduction shape: lane j of the wave takes positions j, j + 64, ... in order; a residue's value is the sum of its masked
 * elements in feature order, a masked-out element adding an exact +0 through a select (NaN may sit there); the lane adds
 * its residues in order; a fixed xor butterfly (32, 16, .. 1) over the 64 lanes gives the total.  Per-feature sums take
 * the same lane walk and butterfly.  No atomics: the sums are a function of the item's (position, feature, value)
 * triples alone -- the same bits for any L >= the last set position, in any batch -- and tot_* equals
 * e3d_masked_item_sums applied to res_* with the any-element-set residue mask, bit for bit.
 * An item whose step lies outside [0, T) reads no table row and gets NaN in every float output (counts stays the
 * mask's count).  F % 4 == 0, F <= 32, N % B == 0; float pointers 16 B aligned, mask 4 B aligned. */
int e3d_angle_score_items(const float* eps_hat, const float* eps, const uint8_t* mask, const int64_t* level_steps,
                          const float* coef, int T, float* term, float* err, float* res_term, float* res_err2,
                          float* feat_term, float* feat_err2, float* tot_term, float* tot_err2, int32_t* counts, int N,
                          int B, int L, int F, void* stream);

/* ------------------------------------------------------------------ keyed training and validation draws
 * The same generator and counter layout with the EPOCH in the step field (training epochs 0 .. 65534; 65535 is the
 * validation value) and streams 4 structure timestep, 5 structure forward noise, 6 sequence timestep, 7 sequence
 * forward-noising uniform.  Frames are padded or trimmed [B, L]: row r is item r / L at position r % L.  ``item_ids``
 * int64 [B] and ``epoch_dev`` (int64, first element) are read from DEVICE memory by the kernels, so a captured
 * training step replays them with whatever the static batch and the epoch word hold.  Nothing is allocated or read
 * back. */

/* out[b] = class in [0, C) of word 0 of (seed, item_ids[b], stream_id, epoch, position 0, block 0); stream_id 4
 * (C = T) or 6 (C = T + 1). */
int e3d_keyed_timesteps(const int64_t* item_ids, const int64_t* epoch_dev, uint64_t seed, int stream_id, int C,
                        int64_t* out, int B, void* stream);

/* Structure forward noising with the noise drawn in-register from stream 5:
 *   noise_out = wrap(scale * z),  xt_out = wrap(sqrt_ab[t[b]] * x0 + sqrt_1mab[t[b]] * noise_out)
 * (the arithmetic of e3d_q_sample_wrap), z the normals of (position l, block j -> features 4j .. 4j+3).  x0 and both
 * outputs [B, L, F], F % 4 == 0, F <= 1024; t int64 [B] on the device, clamped to the T rows of the two tables. */
int e3d_keyed_q_sample_wrap(const float* x0, const int64_t* t, const float* sqrt_ab, const float* sqrt_1mab, int T,
                            float scale, const int64_t* item_ids, const int64_t* epoch_dev, uint64_t seed,
                            float* noise_out, float* xt_out, int B, int L, int F, void* stream);

/* e3d_discrete_q_sample in mode 1 with the uniform of row b * L + l taken from stream 7 (word 0 of block 0 at
 * position l) instead of a buffer; x0 index < 0 (padding row) -> class 0. */
int e3d_keyed_discrete_q_sample(const int32_t* x0_idx, const float* Qtb, const int64_t* item_ids,
                                const int64_t* epoch_dev, uint64_t seed, int32_t* out_idx, int B, int L, int C,
                                void* stream);

/* NeRF backbone builder, the step after structure sampling (structure_model/create_pdb.py:104-155,
 * 175-234): angles [B,L,8] fp32 in the dataset's column order
 * (phi psi omega dihedral_o tau CA:C:1N 1C:N:CA CA:C:O), lengths int32 [B] -> coords float64
 * [B,L,4,3] (N, CA, C, O per residue; residues >= length zeroed), optionally centred per pocket
 * (NERFBuilder.centered_cartesian_coords).  Bond lengths are the reference's constants. */
int e3d_nerf_backbone(const float* angles, const int32_t* lengths, double* coords, int center,
                      int B, int L, void* stream);

/* ------------------------------------------------------------------ training (backward) side
 * The reference trains through torch.autograd on these same modules (Lightning training_step,
 * structure_model/model.py:305-319, sequence_model/model.py:347-367); the entry points below are
 * the hand-written backward of each fused forward kernel. */

/* General-layout split GEMM (the three GEMMs of one nn.Linear share it):
 *   out[M,N] = act(A . B^T + bias), A logical [M,K], B logical [N,K];
 *   x_kmajor = 0: element (r,k) at X[r*ld + k];  x_kmajor = 1: at X[k*ld + r] (transposed storage).
 *   forward  y = x W^T : (0,0);  dgrad dx = dy W : A = dy (0), B = W as [K'][N'] (1);
 *   wgrad dW = dy^T x : A = dy (1), B = x (1).  K-major operands allow any K (tail zero-filled). */
int e3d_gemm_f32_split_general(const float* A, int64_t lda, int a_kmajor, const float* B, int64_t ldb,
                               int b_kmajor, const float* bias, float* out, int64_t ldc, int M, int N,
                               int K, int act, int terms, void* stream);

/* Weight and bias gradients of up to 64 linear layers of ONE shape in one launch (the backward of nn.Linear for every
 * layer of a model at once: torch.autograd computes them layer by layer, Lightning training_step as above):
 *   dW_p[N,K] (contiguous) = dz_p^T . x_p,   db_p[N] = column sums of dz_p      p = 0 .. count-1
 * dz_p [M,N] (row stride ldz), x_p [M,K] (row stride ldx); the reduction runs over the M token rows.  A single layer
 * has too few output tiles for the chip and needs split-K with atomics on a zeroed output; a model's layers together
 * fill it with whole reductions: no atomics, no memsets, deterministic.
 * dz, x, dw, db: HOST arrays of ``count`` device pointers (db may be NULL, or hold NULL entries: no bias gradient).
 * accumulate_bits: bit p set -> dW_p and db_p are added to (a weight that already holds a gradient), else overwritten.
 * Two problems of one launch must not share an output.  terms = 3 (bf16x3), 6 or 19 (bf16x6). */
int e3d_gemm_wgrad_grouped_f32_split(const float* const* dz, const float* const* x, float* const* dw, float* const* db,
                                     uint64_t accumulate_bits, int count, int64_t ldz, int64_t ldx, int N, int K, int M,
                                     int terms, void* stream);

/* The same launch for layers of DIFFERENT shapes and row strides over ONE token count M (ABI v3): problem p is
 * dW_p[N[p], K[p]] = dz_p^T x_p with row strides ldz[p] / ldx[p]; ``db`` (and single entries of it) may be NULL.  A model's
 * weight gradients then take ceil(layers / 64) launches whose grids fill the chip in whole rounds but for one tail, instead
 * of one launch per (shape, stride) group with a partial last round each. */
int e3d_gemm_wgrad_ragged_f32_split(const float* const* dz, const float* const* x, float* const* dw, float* const* db,
                                    const int* N, const int* K, const int64_t* ldz, const int64_t* ldx,
                                    uint64_t accumulate_bits, int count, int M, int terms, void* stream);

/* Backward of e3d_relkey_attn_fwd.  out / lse are the forward's outputs, dout [B,Lq,nh*64].
 * Writes dq, dk, dv (strided like q, k, v) and, with dist_emb, d_dist_emb [2P-1,64] (overwritten).
 * workspace: e3d_relkey_attn_bwd_workspace_floats(...) floats (materialised P and dS tiles + the
 * per-wave dist_emb partial blocks). */
int64_t e3d_relkey_attn_bwd_workspace_floats(int B, int nh, int Lq, int Lk, int relkey);
int e3d_relkey_attn_bwd(const float* q, int64_t q_bs, int64_t q_rs, const float* k, int64_t k_bs,
                        int64_t k_rs, const float* v, int64_t v_bs, int64_t v_rs,
                        const float* dist_emb, int P, const float* key_mask, const float* out,
                        const float* lse, const float* dout, float* dq, int64_t dq_bs, int64_t dq_rs,
                        float* dk, int64_t dk_bs, int64_t dk_rs, float* dv, int64_t dv_bs,
                        int64_t dv_rs, float* d_dist_emb, float* workspace, int B, int nh, int Lq,
                        int Lk, void* stream);

/* ---- dropout (training): reference nn.Dropout(hidden_dropout_prob) in BertEmbeddings
 * (structure_model/model.py:109-117), the SELayer MLP (model.py:45-47), BertSelfOutput / BertOutput and
 * attention_probs_dropout_prob inside BertSelfAttention (transformers 4.38.2).  Decisions are a pure
 * function of (seed, element index): 16-bit fields of a splitmix64 hash, keep iff field >= round(p*65536),
 * kept values scaled by 65536 / (65536 - round(p*65536)).  The backward pass applies the same call to the
 * gradient; nothing is stored. */
int e3d_dropout_f32(const float* x, float p, uint64_t seed, float* out, int64_t n, void* stream);

/* e3d_relkey_attn_fwd_split with dropout on the normalised probabilities (drop_p == 0: identical to it). */
int e3d_relkey_attn_fwd_split_drop(const float* q, int64_t q_bs, int64_t q_rs, const float* k, int64_t k_bs,
                                   int64_t k_rs, const float* v, int64_t v_bs, int64_t v_rs,
                                   const float* dist_emb, int P, const float* key_mask, float* out,
                                   float* lse, int B, int nh, int Lq, int Lk, int terms, float drop_p,
                                   uint64_t drop_seed, void* stream);

/* The full form of the two above: ``e_scratch`` (device, >= e3d_attn_scratch_bytes(Lk) bytes, 16-byte
 * aligned, or NULL) receives the fragment-order bf16 hi/lo planes of dist_emb that the cooperative kernel
 * reads; with NULL (and a dist_emb) the per-wave kernel serves the call instead -- the library never
 * allocates.  ``e_scratch_ready`` != 0: the scratch still holds the planes written by an earlier call with the
 * same dist_emb values and Lk (constant weights: inference) -- the 5-us pre-pass is skipped.
 * ``q_absmax`` / ``k_absmax`` / ``e_absmax`` (device, one float each, or NULL): upper bounds of |element| over the
 * call's Q rows, K rows (INCLUDING padded positions) and the distance table (required with dist_emb when the other
 * two are given) -- as left by e3d_gemm_bias_act_f32_split_ex / e3d_absmax_f32.  They only decide whether all-padding
 * key tiles may be skipped (see e3d_attn_skip_padded_tiles); NULL = never skip.  Read on the device: no host sync.
 * When the call writes the planes itself (e_scratch given, e_scratch_ready == 0) it also RAISES *e_absmax to the largest
 * |element| of the table rows it reads (round 4: the bound costs no launch of its own -- hand in a slot that holds 0 or an
 * earlier bound; a value that is already larger stays). */
int64_t e3d_attn_scratch_bytes(int Lk);
int e3d_relkey_attn_fwd_split_ex(const float* q, int64_t q_bs, int64_t q_rs, const float* k, int64_t k_bs,
                                 int64_t k_rs, const float* v, int64_t v_bs, int64_t v_rs,
                                 const float* dist_emb, int P, const float* key_mask, float* out,
                                 float* lse, int B, int nh, int Lq, int Lk, int terms, float drop_p,
                                 uint64_t drop_seed, void* e_scratch, int e_scratch_ready, const float* q_absmax,
                                 const float* k_absmax, float* e_absmax, void* stream);

/* ---- attention over variable-length segments (ABI v5; packed batches, inference) ------------------------------------
 * Segment s owns query rows q_start[s] .. q_start[s] + q_len[s] - 1 (rows of q: q + row * q_rs + h * 64) and key /
 * value rows k_start[s] .. k_start[s] + k_len[s] - 1; the int32 arrays live on the device.  Each segment computes what
 * e3d_relkey_attn_fwd_split computes on one item with Lq = q_len[s], Lk = k_len[s] and no key mask: keys outside the
 * segment do not exist for its rows.  This equals the padded frame on the valid rows for the reason that makes
 * trimming exact (e3d_attn_skip_padded_tiles): a padded key's weight exp(s - 10000 - m) is 0.0f as long as the row's
 * scores spread over less than ~9900.  With dist_emb ([2P-1, 64]) the rel-key term uses positions measured from the
 * segment start and needs q_len[s] == k_len[s] <= P.  K rows can be a packed buffer (k_start = prefix sums) or a padded
 * [B, Lr] cache (k_start[s] = s * Lr).
 * ``tiles`` [n_tiles, 2] int32 (device): (segment, q0) for every 32-query tile of every segment (sum ceil(q_len / 32)
 * entries), plus (-1, row0) for each 32-row block of query rows that belong to no segment (a packed buffer's tail):
 * those rows of ``out`` are written as zeros.  ``out`` [out_rows, nh * 64] contiguous.  max_q_len / max_k_len bound the
 * lengths (host-side checks only: max_k_len x row stride < 2^30).  ``terms`` 3 / 6 / 19 as above; 0 (f32) runs bf16x6.
 * One wave per (tile entry, head); no dropout, no lse; nothing is allocated and nothing is read back (graph-capturable). */
int e3d_attn_varlen_fwd(const float* q, int64_t q_rs, const float* k, int64_t k_rs, const float* v, int64_t v_rs,
                        const int* q_start, const int* q_len, const int* k_start, const int* k_len, const int* tiles,
                        int n_tiles, const float* dist_emb, int P, float* out, int64_t out_rows, int nh, int max_q_len,
                        int max_k_len, int terms, void* stream);

/* e3d_relkey_attn_bwd for a forward that used (drop_p, drop_seed). */
int e3d_relkey_attn_bwd_drop(const float* q, int64_t q_bs, int64_t q_rs, const float* k, int64_t k_bs,
                             int64_t k_rs, const float* v, int64_t v_bs, int64_t v_rs,
                             const float* dist_emb, int P, const float* key_mask, const float* out,
                             const float* lse, const float* dout, float* dq, int64_t dq_bs,
                             int64_t dq_rs, float* dk, int64_t dk_bs, int64_t dk_rs, float* dv,
                             int64_t dv_bs, int64_t dv_rs, float* d_dist_emb, float* workspace, int B,
                             int nh, int Lq, int Lk, float drop_p, uint64_t drop_seed, void* stream);

/* The full form: ``terms`` selects the arithmetic of the backward products -- 0 = exact fp32 MFMA (what the two
 * entry points above run), 3 = bf16x3 split operands on the bf16 MFMA (fp32 accumulation; 5x fewer matrix-pipe
 * cycles), 6 = the fp32 MFMA kernels again (no bf16x6 backward: the fp32-grade mode stays exact). */
int e3d_relkey_attn_bwd_ex(const float* q, int64_t q_bs, int64_t q_rs, const float* k, int64_t k_bs,
                           int64_t k_rs, const float* v, int64_t v_bs, int64_t v_rs,
                           const float* dist_emb, int P, const float* key_mask, const float* out,
                           const float* lse, const float* dout, float* dq, int64_t dq_bs, int64_t dq_rs,
                           float* dk, int64_t dk_bs, int64_t dk_rs, float* dv, int64_t dv_bs,
                           int64_t dv_rs, float* d_dist_emb, float* workspace, int B, int nh, int Lq,
                           int Lk, int terms, float drop_p, uint64_t drop_seed, void* stream);

/* Test aid: the multipliers (0 or 1/(1-p')) the two calls above apply to P[b,h,q,key] -> out [B,nh,Lq,Lk]. */
int e3d_attn_dropout_mask(int B, int nh, int Lq, int Lk, float p, uint64_t seed, float* out, void* stream);

/* LayerNorm backward on the saved pre-norm rows s [M,H]: ds = dLN/ds, dgamma/dbeta (overwritten;
 * gamma == NULL: no affine, as SELayer.norm1/norm2). */
int e3d_layernorm_bwd(const float* dy, const float* s, const float* gamma, float eps, float* ds,
                      float* dgamma, float* dbeta, int M, int H, void* stream);

/* Backward of e3d_adaln_gate_fwd w.r.t. y (-> dy) and mod (-> dmod [Mc,6H]: stored when
 * rows_per_cond == 1, ACCUMULATED when > 1 -- zero it once before the two branch calls);
 * the gradient w.r.t. x is dout itself. */
int e3d_adaln_gate_bwd(const float* dout, const float* y, const float* mod, int branch,
                       int rows_per_cond, float* dy, float* dmod, int M, int H, void* stream);

/* Activations on saved pre-activations (training keeps z; inference fuses them into the GEMM). */
int e3d_act_fwd(const float* z, int act, float* out, int64_t n, void* stream);
int e3d_act_bwd(const float* dh, const float* z, int act, float* dz, int64_t n, void* stream);

/* out[n] = sum_m x[m,n] (bias gradients);  out[g,:] = sum of rows_per_group consecutive rows. */
int e3d_colsum(const float* x, int64_t ld, float* out, int M, int N, void* stream);
/* Up to 64 matrices of one shape transposed in one launch: dst_p[c * ld_dst + r] = src_p[r * ld_src + c], r < rows,
 * c < cols.  src, dst: HOST arrays of ``count`` device pointers.  (Training: W^T of every weight once per optimizer
 * step, for the input-gradient GEMM dz . W in the forward layout -- one launch per weight shape instead of one copy
 * kernel per layer; ld_dst lets the transposes of query / key / value land side by side as the W^T of the packed QKV.) */
int e3d_transpose_grouped_f32(const float* const* src, float* const* dst, int count, int rows, int cols, int64_t ld_src,
                              int64_t ld_dst, void* stream);
int e3d_group_sum(const float* x, int rows_per_group, float* out, int M, int H, void* stream);

/* dW[h,f] (transpose_out: [f,h]) = sum_m g[m,h] x[m,f], db[h] = sum_m g[m,h]; F <= 32
 * (BertEmbeddings.linear and predictor.dense2 weight gradients). */
int e3d_small_k_wgrad(const float* g, const float* x, float* dW, float* db, int M, int H, int F,
                      int transpose_out, void* stream);

/* dx[M,H] = dout[M,Nout] @ W[Nout,H] (input gradient of predictor.dense2). */
int e3d_head_linear_bwd_dx(const float* dout, const float* W, float* dx, int M, int H, int Nout,
                           void* stream);

/* nn.Dropout between the dense layer and the residual LayerNorm of BertSelfOutput / BertOutput (training mode; transformers
 * 4.38.2 modeling_bert.py) folded into the LayerNorm kernels: the forward applies the multipliers of e3d_dropout_f32 for
 * the same (p, seed) to x as it reads it (element index = row * H + column), the backward writes both ds (gradient of the
 * pre-norm sum = of the residual) and ds_dropped = ds * multipliers (gradient of x): no [M, H] dropout pass in either
 * direction.  Same (p, seed) in both calls. */
int e3d_residual_layernorm_drop_fwd(const float* x, const float* residual, const float* gamma, const float* beta, float eps,
                                    float* s_out, float* out, int M, int H, float drop_p, uint64_t drop_seed, void* stream);
int e3d_layernorm_bwd_drop(const float* dy, const float* s, const float* gamma, float eps, float* ds, float* ds_dropped,
                           float* dgamma, float* dbeta, int M, int H, float drop_p, uint64_t drop_seed, void* stream);
/* Both of the above in one entry point (ds_dropped == NULL: no dropout) with the parameter gradients summed through a caller
 * workspace of e3d_layernorm_bwd_workspace_floats(M, H) floats -- per-block partial rows, added up in a fixed order by a second
 * launch -- instead of float atomics on a zero-filled output: deterministic, and what autograd.layernorm_bwd calls (round 4:
 * 256-512 adders per address were most of the launch).  Backward of torch.nn.LayerNorm in BertSelfOutput / BertOutput
 * (transformers 4.38.2 modeling_bert.py) and SELayer.norm1 / norm2 (structure_model/model.py:27-67). */
int64_t e3d_layernorm_bwd_workspace_floats(int M, int H);
int e3d_layernorm_bwd_ws(const float* dy, const float* s, const float* gamma, float eps, float* ds, float* ds_dropped,
                         float* dgamma, float* dbeta, int M, int H, float drop_p, uint64_t drop_seed, float* workspace,
                         int64_t workspace_floats, void* stream);

/* ---- row-complete GEMM + bias + residual + LayerNorm (ABI v4; inference at large M) ----------------------------------
 * BertSelfOutput / BertOutput whole -- LayerNorm(dense(x) + residual), transformers 4.38.2 modeling_bert.py, reached through
 * structure_model/model.py:197-213 and sequence_model/model.py:226-231 -- as ONE launch whose workgroups own whole 768-wide
 * rows: out[M,768] = LayerNorm(A[M,K] W[768,K]^T * out_scale + bias + residual) * gamma + beta.  The pre-norm sum never
 * leaves the accumulators (the GEMM + e3d_residual_layernorm_fwd pair writes it and reads it back: 4 row passes against 3).
 * Same 2-term split products in the same order as e3d_gemm_bias_act_f32_split (terms 3 or 19: the pre-norm sums are
 * bit-identical), same two-pass statistics as e3d_residual_layernorm_fwd (outputs agree to a few 1e-7).
 *   w_planes: the weight PRE-SPLIT into its two 16-bit terms in MFMA-fragment order by e3d_weight_planes_f32_split (once
 *     per weight version; e3d_weight_planes_bytes(N, K) = N K 4 bytes; for terms = 19 split the power-of-two-scaled weight
 *     and pass the inverse power as out_scale, exactly as for the *_ex GEMM entry points);
 *   residual may be NULL; A, residual and out are row-strided (lda, ldr, ldo in floats).
 * Shapes: N = 768, M % 32 == 0, K % 32 == 0, K >= 64 (e3d_gemm_residual_layernorm_supported).
 * Strides: lda >= K, ldr >= N, ldo >= N; lda % 4 == 0 and ldr % 4 == 0 (16-byte rows); 96 * lda < 2^30 and 16 * ldr < 2^30:
 * the kernel addresses the rows of one tile (96 of A, 16 of the residual) by 32-bit BYTE offsets from the tile's first row,
 * so the largest, (95 * lda + 28) * 4 + 16, must stay below 2^32.  The predicate refuses a larger lda, the entry points
 * a larger ldr. */
int64_t e3d_weight_planes_bytes(int N, int K);
int e3d_weight_planes_f32_split(const float* W, int N, int K, int terms, void* planes, void* stream);
int e3d_gemm_residual_layernorm_supported(int M, int N, int K, int64_t lda);
int e3d_gemm_residual_layernorm_f32_split(const float* A, int64_t lda, const void* w_planes, const float* bias,
                                          const float* residual, int64_t ldr, const float* gamma, const float* beta, float eps,
                                          float* out, int64_t ldo, int M, int N, int K, int terms, float out_scale, void* stream);

/* ---- activation planes (inference; additions to ABI v5) ----------------------------------------------------------------
 * The A operand of the row-complete kernel in the form it consumes: an [M, K] fp32 activation stored as its two 16-bit
 * terms (hi, lo: the 2-term split of terms = 3 / 19) in MFMA-fragment order, as many bytes as the fp32 tensor:
 *     planes[((rb * (K / 16) + ks) * 2 + plane) * 1024 + lane * 16 + 2 j] = term_plane(X[32 rb + (lane & 31)][16 ks + 8 (lane >> 5) + j])
 * (rb = 32-row block, ks = k16 step, lane < 64, j < 8; M % 32 == 0, K % 16 == 0).  A tensor in this form is written by its
 * producer and read by e3d_gemm_residual_layernorm_planes_split only; the sums are bit-identical to the fp32-A entry point.
 *   e3d_activation_planes_f32_split: the format's definition as a kernel (tests, callers without a plane-writing producer);
 *   e3d_gemm_bias_act_planes_split: e3d_gemm_bias_act_f32_split_ex (act none / GELU, terms 3 / 19) whose [M, N] result leaves as
 *     planes -- bit for bit the split of the fp32 result.  Exists where the launch takes the persistent 256x256 kernel:
 *     e3d_gemm_planes_supported says so beforehand; anything else is an error.  bias must be 16-byte aligned.
 *   e3d_relkey_attn_fwd_split_planes: e3d_relkey_attn_fwd_split_ex (no dropout, no lse) whose context leaves as planes of
 *     the [B * Lq, nh * 64] matrix -- bit for bit the split of the fp32 context.  Exists where the call lands on the 4-wave
 *     cooperative kernel and Lq % 32 == 0: e3d_attn_planes_supported (strides of k / v in floats, have_scratch = no dist_emb or
 *     an e_scratch) says so beforehand; anything else is an error, never a silent fp32 store. */
int64_t e3d_activation_planes_bytes(int M, int K);
int e3d_activation_planes_f32_split(const float* X, int64_t ldx, int M, int K, int terms, void* planes, void* stream);
int e3d_gemm_residual_layernorm_planes_split(const void* a_planes, const void* w_planes, const float* bias,
                                             const float* residual, int64_t ldr, const float* gamma, const float* beta, float eps,
                                             float* out, int64_t ldo, int M, int N, int K, int terms, float out_scale, void* stream);
int e3d_gemm_planes_supported(int M, int N, int K, int64_t lda, int act, int terms);
int e3d_gemm_bias_act_planes_split(const float* A, int64_t lda, const float* W, const float* bias, void* out_planes,
                                   int M, int N, int K, int act, int terms, float* out_absmax, float out_scale, void* stream);
int e3d_attn_planes_supported(int64_t k_rs, int64_t v_bs, int64_t v_rs, int Lq, int Lk, int terms, int have_scratch);
int e3d_relkey_attn_fwd_split_planes(const float* q, int64_t q_bs, int64_t q_rs, const float* k, int64_t k_bs,
                                     int64_t k_rs, const float* v, int64_t v_bs, int64_t v_rs,
                                     const float* dist_emb, int P, const float* key_mask, void* out_planes,
                                     int B, int nh, int Lq, int Lk, int terms, void* e_scratch, int e_scratch_ready,
                                     const float* q_absmax, const float* k_absmax, float* e_absmax, void* stream);

/* ---- optimizer step (ABI v3) ------------------------------------------------------------------------------------------
 * Global-norm gradient clip + AdamW over ALL parameters in three launches: what Lightning's gradient_clip_val = 1.0
 * (structure_model/train_model.py:99-110) and torch.optim.AdamW (structure_model/model.py:361-366,
 * sequence_model/model.py configure_optimizers) do around every training_step.  Tensors are reached through pointer
 * tables in DEVICE memory (``count`` entries: params / grads / exp_avg / exp_avg_sq pointers and element counts); the work
 * unit is a chunk of e3d_optim_chunk_elems() consecutive elements of one tensor, listed by the caller in
 * ``chunk_tensor[n_chunks]`` (table index) and ``chunk_first[n_chunks]`` (first element), both device arrays.
 *   e3d_grad_global_norm: norm_and_clip[0] = sqrt(sum g^2) (deterministic: per-chunk partials into ``partial[n_chunks]``,
 *     summed in a fixed order), norm_and_clip[1] = min(max_norm / (norm + 1e-6), 1) (NaN / inf propagate, as
 *     torch.nn.utils.clip_grad_norm_ with error_if_nonfinite=False).  Gradients are NOT rewritten.
 *   e3d_adamw_step: torch's AdamW update (decoupled weight decay, bias corrections from ``step`` >= 1) with every gradient
 *     multiplied by norm_and_clip[1] on the way in (norm_and_clip may be NULL: no clip).  */
/*   e3d_adamw_step_dyn: the same update with the learning rate and the step count read from DEVICE memory
 *     (lr_and_step[0] = lr, lr_and_step[1] = number of steps taken BEFORE this one, as a float) -- the form a captured HIP
 *     graph of the training step replays: the caller advances lr_and_step[1] on the device after the launch.
 *   e3d_adamw_step_dev (ABI v4): EVERY scalar of the update from device memory -- hyper[0..5] = lr, steps taken before this
 *     one, beta1, beta2, eps, weight_decay -- so that a replayed graph follows schedulers that move more than the learning
 *     rate (torch's OneCycleLR cycles beta1 with it: structure_model/model.py:372, sequence_model/model.py:425).
 *   e3d_dropout_set_epoch_ptr: registers (per device; NULL unregisters) a device word every dropout launch adds to its
 *     seed INSIDE the kernel (e3d_dropout_f32, e3d_relkey_attn_fwd_split_drop / _ex, e3d_relkey_attn_bwd_drop / _ex,
 *     e3d_attn_dropout_mask): a replayed graph bakes the seed arguments, so the training step advances this word instead
 *     and every replay draws fresh decisions while forward and backward of one step still agree.  */
int e3d_adamw_step_dyn(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                       const int64_t* numel, const int* chunk_tensor, const int64_t* chunk_first, int n_chunks,
                       const float* norm_and_clip, const float* lr_and_step, float beta1, float beta2, float eps,
                       float weight_decay, void* stream);
int e3d_adamw_step_dev(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                       const int64_t* numel, const int* chunk_tensor, const int64_t* chunk_first, int n_chunks,
                       const float* norm_and_clip, const float* hyper, void* stream);
int e3d_dropout_set_epoch_ptr(const uint64_t* device_word);
int e3d_optim_chunk_elems(void);
int e3d_grad_global_norm(const float* const* grads, const int64_t* numel, const int* chunk_tensor, const int64_t* chunk_first,
                         int n_chunks, float max_norm, float* partial, float* norm_and_clip, void* stream);
int e3d_adamw_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                   const int64_t* numel, const int* chunk_tensor, const int64_t* chunk_first, int n_chunks,
                   const float* norm_and_clip, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                   void* stream);

/* ---- weight EMA inside the update launch (training.WeightEMA; additions to ABI v5, nothing above changed)
 * The two forms of the update that optim.ClipAdamW launches, each also averaging the parameter it just wrote into a
 * shadow: e <- e + (p_new - e) * w, w = 1.0f - d_n (fp32).  ``ema``: one more pointer table in device memory, ``count``
 * fp32 shadows with the element counts of ``params``; each is read and written once per element (8 B on top of the
 * update's 28 B) and joins the 16-byte alignment test of the float4 path.  Parameters and both moments come out bit-equal
 * to e3d_adamw_step / e3d_adamw_step_dev.  A NULL ``ema`` is rejected.
 *   e3d_adamw_ema_step: ``ema_decay`` = d_n of THIS update, from the host (training.ema_decay_at); outside [0, 1) is
 *     rejected.
 *   e3d_adamw_ema_step_dev: d_n from the range's 8-float ``hyper`` block, whose two pad words it uses: hyper[6] = decay
 *     in [0, 1) with its SIGN BIT set when the warm-up is off (-0.0f for decay 0), hyper[7] = EMA updates made before this
 *     one, as a float (exact below 2^24); d_n = (float)min(decay, (1 + n) / (10 + n)) with n = hyper[7] + 1, in double --
 *     or (float)decay without warm-up.  The caller advances hyper[7] on the device after the launch, next to hyper[1].
 *     The block is device memory: its decay cannot be checked at the entry point.  */
int e3d_adamw_ema_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                       float* const* ema, const int64_t* numel, const int* chunk_tensor, const int64_t* chunk_first,
                       int n_chunks, const float* norm_and_clip, float lr, float beta1, float beta2, float eps,
                       float weight_decay, int step, float ema_decay, void* stream);
int e3d_adamw_ema_step_dev(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                           float* const* ema, const int64_t* numel, const int* chunk_tensor, const int64_t* chunk_first,
                           int n_chunks, const float* norm_and_clip, const float* hyper, void* stream);

/* ---- keyed dropout decisions (seeded training; additions to ABI v5)
 * With a seed, every dropout decision of a training step is a pure function of (seed, item id, epoch, site, position, head,
 * column or key) -- not of the batch, the row, the frame or the number of steps run before.
 *   e3d_keyed_drop_row_keys: one 64-bit key per row of a [B, L] frame, out[b * L + l] = w0 | w1 << 32 of
 *     Philox4x32-10(seed; ids[b]; stream << 16 | epoch; l << 8): stream 8 = ligand rows, 9 = pocket rows; ids int64 [B] and the
 *     epoch word are read from DEVICE memory, so a captured step replays the launch with the current ones.
 *   the _keyed entry points: their (drop_p, drop_seed) counterparts with (drop_p, site, row_keys) instead.  A row's key takes
 *     the place of the seed of the generator above, the group index is site << 40 | head << 24 | group with group = column >> 2
 *     (hidden states; head = 0) or key position >> 2 (attention probabilities; the row is the QUERY's, row_keys is the table of
 *     the [B, Lq] query frame), and the device word of e3d_dropout_set_epoch_ptr is NOT added.  site < 2^24 is the ordinal of the
 *     dropout call within the step; nh < 2^16.  e3d_dropout_f32_keyed takes the tensor as [M, H] rows, H % 4 == 0.  */
int e3d_keyed_drop_row_keys(const int64_t* ids, int B, int L, const int64_t* epoch_word, uint64_t seed, int stream,
                            uint64_t* out, void* st);
int e3d_dropout_f32_keyed(const float* x, float p, uint32_t site, const uint64_t* row_keys, float* out, int M, int H,
                          void* stream);
int e3d_keyed_attn_dropout_mask(int B, int nh, int Lq, int Lk, float p, uint32_t site, const uint64_t* row_keys, float* out,
                                void* stream);
int e3d_residual_layernorm_drop_fwd_keyed(const float* x, const float* residual, const float* gamma, const float* beta, float eps,
                                          float* s_out, float* out, int M, int H, float drop_p, uint32_t site,
                                          const uint64_t* row_keys, void* stream);
int e3d_layernorm_bwd_drop_keyed(const float* dy, const float* s, const float* gamma, float eps, float* ds, float* ds_dropped,
                                 float* dgamma, float* dbeta, int M, int H, float drop_p, uint32_t site, const uint64_t* row_keys,
                                 void* stream);
int e3d_layernorm_bwd_ws_keyed(const float* dy, const float* s, const float* gamma, float eps, float* ds, float* ds_dropped,
                               float* dgamma, float* dbeta, int M, int H, float drop_p, uint32_t site, const uint64_t* row_keys,
                               float* workspace, int64_t workspace_floats, void* stream);
int e3d_relkey_attn_fwd_split_drop_keyed(const float* q, int64_t q_bs, int64_t q_rs, const float* k, int64_t k_bs,
                                         int64_t k_rs, const float* v, int64_t v_bs, int64_t v_rs, const float* dist_emb,
                                         int P, const float* key_mask, float* out, float* lse, int B, int nh, int Lq, int Lk,
                                         int terms, float drop_p, uint32_t site, const uint64_t* row_keys, void* stream);
int e3d_relkey_attn_fwd_split_ex_keyed(const float* q, int64_t q_bs, int64_t q_rs, const float* k, int64_t k_bs,
                                       int64_t k_rs, const float* v, int64_t v_bs, int64_t v_rs, const float* dist_emb,
                                       int P, const float* key_mask, float* out, float* lse, int B, int nh, int Lq, int Lk,
                                       int terms, float drop_p, uint32_t site, const uint64_t* row_keys, void* e_scratch,
                                       int e_scratch_ready, const float* q_absmax, const float* k_absmax, float* e_absmax,
                                       void* stream);
int e3d_relkey_attn_bwd_drop_keyed(const float* q, int64_t q_bs, int64_t q_rs, const float* k, int64_t k_bs, int64_t k_rs,
                                   const float* v, int64_t v_bs, int64_t v_rs, const float* dist_emb, int P,
                                   const float* key_mask, const float* out, const float* lse, const float* dout, float* dq,
                                   int64_t dq_bs, int64_t dq_rs, float* dk, int64_t dk_bs, int64_t dk_rs, float* dv,
                                   int64_t dv_bs, int64_t dv_rs, float* d_dist_emb, float* workspace, int B, int nh, int Lq,
                                   int Lk, float drop_p, uint32_t site, const uint64_t* row_keys, void* stream);
int e3d_relkey_attn_bwd_ex_keyed(const float* q, int64_t q_bs, int64_t q_rs, const float* k, int64_t k_bs, int64_t k_rs,
                                 const float* v, int64_t v_bs, int64_t v_rs, const float* dist_emb, int P,
                                 const float* key_mask, const float* out, const float* lse, const float* dout, float* dq,
                                 int64_t dq_bs, int64_t dq_rs, float* dk, int64_t dk_bs, int64_t dk_rs, float* dv,
                                 int64_t dv_bs, int64_t dv_rs, float* d_dist_emb, float* workspace, int B, int nh, int Lq,
                                 int Lk, int terms, float drop_p, uint32_t site, const uint64_t* row_keys, void* stream);

/* ---- featurization of PDB coordinates (featurize.py; additions to ABI v5)
 * The inverse direction of e3d_nerf_backbone, and the pocket definition, for records built from PDB files.
 *   backbone angles: coords [R,4,3] fp32 (N, CA, C, O per residue row, many chains back to back), seg int32 [R] (the chain
 *     of a row) -> angles [R,8] fp32 radians in the STORED column order of a biolip.pt (omega, phi, psi, dihedral_o, theta1 N:CA:C,
 *     theta2 CA:C:1N, theta3 1C:N:CA, theta_o CA:C:O; clean_data/data_preprocessing.py:688-731) and status int32 [R].  A row
 *     is interior when seg[r-1] == seg[r] == seg[r+1]; every other row gets zeros and status bit 0, and no row of another
 *     chain or outside [0, R) is read.  float64 algebra from the float32 coordinates, atan2 forms (dihedral =
 *     atan2((n1 x n2) . v2 / |v2|, n1 . n2), angle = atan2(|u x w|, u . w)), one rounding to float32; the dihedral's sign is
 *     the reference's sign((n1 x n2) . v2).  KNOWN DIFFERENCE: at exact planarity the reference returns 0 (its arccos is
 *     multiplied by np.sign(0)); this kernel returns +-pi for a trans arrangement.
 *     status bit 1: a zero-length bond or a zero plane normal (the reference raises / gives NaN): zeros are written.
 *     status bit 2: C-1 - N or C - N+1 longer than max_peptide_bond (a chain break); the angles are still written, as the
 *     reference computes across breaks.
 *   contact residues: hit[row] = 1 when any atom of receptor residue row lies within cutoff (same unit as the coordinates)
 *     of any ligand atom of the SAME complex, else 0, for all complexes in one launch.  rec_xyz [n_rec_atoms,3] and lig_xyz
 *     [n_lig_atoms,3] fp32 hold the atoms of complex c at rec_off[c] .. rec_off[c+1]-1 and lig_off[c] .. lig_off[c+1]-1
 *     (int32 [n_complexes+1], on the device); rec_row int32 [n_rec_atoms] is the residue row of a receptor atom, hit int32
 *     [n_rows].  n_lig_atoms == 0 (lig_xyz may be null) gives all zeros.  The cutoff is the caller's choice: BioLiP's own
 *     binding-site rule (van-der-Waals radii) is not reproduced.
 * Both validate before any launch: null pointers, R > 0, max_peptide_bond > 0, counts, cutoff > 0. */
int e3d_backbone_angles(const float* coords, const int32_t* seg, float* angles, int32_t* status, int R,
                        float max_peptide_bond, void* stream);
int e3d_contact_residues(const float* rec_xyz, const int32_t* rec_row, const int32_t* rec_off, const float* lig_xyz,
                         const int32_t* lig_off, int32_t* hit, int n_complexes, int n_rec_atoms, int n_lig_atoms, int n_rows,
                         float cutoff, void* stream);

/* ---- rigid superposition of structure pairs (evaluate.py; an addition to ABI v5)
 * Scores sampled backbones: for each pair p the proper rotation R (det R = +1, never a reflection) and translation t that
 * minimise msd = (1/n) sum_i | R a_i + t - b_i |^2 over the n atoms a_i of structure mob[p] (the mobile one) and b_i of
 * structure ref[p] (the reference one), and that minimum.  CONVENTION: x' = R x + t maps the mobile structure onto the
 * reference one; rot is row-major.
 *   xyz fp64 [n_atoms,3]: all structures back to back; off int32 [n_structs+1]: structure s holds atoms off[s] .. off[s+1]-1
 *   (off[0] = 0); mob, ref int32 [n_pairs]; msd fp64 [n_pairs]; rot fp64 [n_pairs,9] and trans fp64 [n_pairs,3] may be null
 *   TOGETHER (msd is the same, bit for bit); status int32 [n_pairs].  All on the device.
 *   status 0: ok.  n = 1 gives msd 0 and R = identity; a collinear or planar set gives one of its minimisers.
 *   status 1: the two structures differ in atom count.       status 2: both are empty.
 *   status 3: mob[p] or ref[p] outside [0, n_structs), or an offset of theirs outside [0, n_atoms] or descending; nothing is
 *             read through such an index or offset.
 *   status 4: a non-finite coordinate (or coordinates whose float64 sums overflow).
 *   Every status but 0 writes NaN to msd, rot and trans of its pair and leaves the other pairs alone.
 * Arithmetic: float64 throughout.  Two passes (centroids, then the centred cross-covariance S and G = sum |a - abar|^2 +
 * sum |b - bbar|^2; no raw moments), the largest eigenpair of Horn's symmetric 4x4 matrix of S by cyclic Jacobi with a fixed
 * maximum of sweeps (a NaN ends in NaN, no loop waits for convergence alone), msd = max(0, (G - 2 lambda) / n).  Take the
 * square root on the caller's side: on near-identical structures msd is good to ~32 eps64 G / n, which is ~1e-6 Angstrom
 * of RMSD.  One 64-lane wave per pair, one launch for all pairs.
 * Validates before any launch: xyz, off, mob, ref, msd, status non-null; rot and trans both null or both set; n_structs,
 * n_atoms, n_pairs > 0. */
int e3d_superpose_pairs(const double* xyz, const int32_t* off, const int32_t* mob, const int32_t* ref, double* msd,
                        double* rot, double* trans, int32_t* status, int n_structs, int n_atoms, int n_pairs, void* stream);

/* ---- backbone geometry: secondary structure, hydrogen bonds, bends, clashes (evaluate.py, featurize.py; an addition to
 * ABI v5)
 * Describes backbones that have no native to be compared with, after Kabsch & Sander (Biopolymers 22, 2577 (1983)), from
 * N, CA, C, O alone, for all structures of a call at once.
 *   coords fp64 [n_residues,4,3]: N, CA, C, O per residue, all structures back to back; off int32 [n_structs+1]: structure
 *   s holds residues off[s] .. off[s+1]-1 (the convention of e3d_superpose_pairs, in residues); is_pro uint8 [n_residues]
 *   or null (no proline): a proline has no amide hydrogen.  All on the device.
 *   Per residue: ss uint8, the index into "HBEGITS-"; acc_rel int32 [.,2] and acc_e fp64 [.,2], the two lowest-energy
 *   acceptors a of this residue's N-H as (a - d, E) (DSSP's N-H-->O columns); don_rel, don_e likewise the donors d of
 *   its C=O as (d - a, E) (O-->H-N); only E < 0 counts, ties go to the lower index, an absent partner is 0 with 0.0;
 *   kappa fp64 in degrees (NaN where undefined); clash int32; hbonds int32, the acceptors of its N-H with E < -0.5;
 *   status int32: 0 ok, 1 a non-finite coordinate, 3 held by no structure with good offsets.
 * Rules (every index inside the residue's own structure; restated in float64 numpy by tests/dssp_ref.py):
 *   valid(i): all twelve coordinates finite; a residue that is not valid takes part in nothing, breaks contiguity, gets '-'.
 *   bonded(i): i not the first of its structure, valid(i-1), valid(i), |C[i-1] - N[i]| <= max_peptide_bond.
 *   contig(a, b): bonded(k) for all a < k <= b.
 *   H[i] = N[i] + unit(C[i-1] - O[i-1]); exists iff bonded(i), i no proline, |C[i-1] - O[i-1]| > 0.
 *   E(a, d), C=O of a accepting N-H of d: defined iff |a - d| >= 2, valid(a), H[d] exists and |CA[a] - CA[d]| < 9.0;
 *     27.888 (1/|O_a N_d| + 1/|C_a H_d| - 1/|O_a H_d| - 1/|C_a N_d|), floored at -9.9; -9.9 when one of the four distances is
 *     below 0.5.  hbond(a, d) := E(a, d) < -0.5.
 *   n-turn at i (n = 3, 4, 5): contig(i, i+n) and hbond(i, i+n).
 *   H on s .. s+3 when the 4-turns at s-1 and s exist; G on s .. s+2 (3-turns) only if none of the three is H, B or E;
 *   I on s .. s+4 (5-turns) only if none of the five is H, B, E or G.
 *   bridge(i, j): contig(i-1, i+1), contig(j-1, j+1), |i - j| >= 3; parallel if [hbond(i-1, j) and hbond(j, i+1)] or
 *     [hbond(j-1, i) and hbond(i, j+1)]; antiparallel if [hbond(i, j) and hbond(j, i)] or [hbond(i-1, j+1) and
 *     hbond(j-1, i+1)].  E: a bridge of type t with some j whose neighbour (i+-1, j+-1) (parallel) or (i+-1, j-+1)
 *     (antiparallel) is a bridge of type t too; B: a bridge, but none with such a neighbour.
 *   T: residues k+1 .. k+n-1 of an n-turn at k.  S: contig(i-2, i+2) and kappa(i) > 70 degrees, kappa the angle between
 *     CA[i] - CA[i-2] and CA[i+2] - CA[i] as atan2(|u x w|, u . w).  Priority H, B, E, G, I, T, S, '-'.
 *   clash[i]: atom pairs (atom of i, atom of j), j in the same structure, |i - j| >= 2, both valid, closer than
 *     clash_cutoff -- the caller's choice, not a standard.  A structure's clash number is half the sum over its residues.
 * THREE DIFFERENCES FROM DSSP: turns and bridges test the full relation E < -0.5, not DSSP's two best partners per side;
 * pairs with |a - d| = 1 have no energy; energies are not rounded to 0.001.  No beta-bulges, no sheet labels.  Agreement
 * with the mkdssp program has not been measured.
 * A residue's results depend on its own structure's coordinates alone, not on the structure's place in the call.  All
 * arithmetic float64; one call, five launches on one stream, no atomics, no host synchronisation, fixed loop bounds.
 * Offsets are checked on the device: a structure with off[s] < 0, off[s+1] > n_residues or off[s+1] < off[s] is skipped,
 * nothing is read through its offsets, and residues that no good structure holds get status 3, '-', absent partners, NaN
 * kappa and zero counts.  Structures that overlap are memory-safe and otherwise undefined.
 * Validates before any launch: coords, off and every output non-null; n_structs, n_residues > 0; clash_cutoff and
 * max_peptide_bond > 0 and finite. */
int e3d_backbone_geometry(const double* coords, const int32_t* off, const uint8_t* is_pro, uint8_t* ss, int32_t* acc_rel,
                          double* acc_e, int32_t* don_rel, double* don_e, double* kappa, int32_t* clash, int32_t* hbonds,
                          int32_t* status, int n_structs, int n_residues, double clash_cutoff, double max_peptide_bond,
                          void* stream);

/* ---- local alignment of sequence sets (similarity.py; an addition to ABI v5)
 * Smith-Waterman with affine gaps (Gotoh) of every query with every target, in integers: per pair the score of the best
 * local alignment and two counters of the path that produced it, from which the caller forms an identity.  No traceback.
 *   q_codes uint8 [n_q_codes], q_off int32 [n_q+1]: query s holds codes q_off[s] .. q_off[s+1]-1, packed back to back (the
 *   convention of e3d_backbone_geometry); t_codes, t_off [n_t+1] likewise.  A code is an index 0..19 into
 *   "ACDEFGHIKLMNPQRSTVWY".  subst int8 [20*20]: the substitution matrix in that order, the caller's choice (similarity.py
 *   passes BLOSUM62).  score, matches, columns int32 [n_q, n_t], row-major.  All on the device.
 *   Query a[1..m], target b[1..n], go = gap_open, ge = gap_extend; a gap of k columns costs go + k ge (blastp's convention):
 *     E[i][j] = max(H[i][j-1] - (go+ge), E[i][j-1] - ge)        the column consumes b_j only
 *     F[i][j] = max(H[i-1][j] - (go+ge), F[i-1][j] - ge)        the column consumes a_i only
 *     H[i][j] = max(0, H[i-1][j-1] + S[a_i][b_j], E[i][j], F[i][j])
 *   H[0][*] = H[*][0] = 0; E and F are minus infinity on the boundary (int32 arithmetic, nothing wraps).
 *   H, E and F each carry the counters of the path behind their value: matches, the diagonal columns with a_i == b_j, and
 *   columns, all columns, gaps included.  TIE RULES (identity depends on which co-optimal alignment is taken): E and F, on
 *   equal value opening from H wins over extending; H, the diagonal wins over E and E over F, a later candidate replaces an
 *   earlier one only if strictly greater; a winner <= 0 makes the cell (0, 0, 0).  The pair's result is the cell with the
 *   largest H, among equals the smallest i, then the smallest j; a pair with no positive cell gives (0, 0, 0).
 *   tests/align_ref.py restates this in Python.
 *   Lengths 1 .. E3D_ALIGN_MAX_LEN; scores then stay below 2^14 for matrix entries up to 11 and counters below 2^16.
 *   upper_only != 0: pairs with t <= q are not looked at and are written (-1, -1, -1), whatever their sequences are (a set
 *   against itself).
 *   Checked on the device: a sequence whose offsets are out of order or outside [0, n_codes], whose length is 0 or above
 *   the cap, or that holds a code >= 20 is never read through, and every pair it takes part in is written (-2, -2, -2);
 *   nothing faults, nothing outside [n_q, n_t] is written.  Offsets that make sequences overlap are memory-safe.
 *   workspace: queries longer than 32 residues need one: any whole number of 1 MiB slots, each serves one wave at a time
 *   (e3d_align_workspace_bytes(n_q, n_t) is the size that keeps the device busy), not shared between calls that may run
 *   concurrently.  Null, or smaller than a slot: the cap on QUERY length of this call is 32, and a longer query is a bad
 *   sequence like one above E3D_ALIGN_MAX_LEN (targets are not affected).
 *   A pair's three numbers depend on its two sequences, the matrix and the gap costs only -- not on n_q, n_t, its place or
 *   its neighbours.  One lane per pair, the lanes of a wave share the query and take consecutive targets: sort the targets
 *   by length for speed (any order is correct).  Two launches on one stream, no atomics, no host synchronisation.
 * Validates before any launch: every pointer but workspace non-null; n_q, n_t > 0; n_q_codes, n_t_codes >= 0;
 * gap_open >= 0, gap_extend >= 1, gap_open + gap_extend <= 127. */
#define E3D_ALIGN_MAX_LEN 1024
int64_t e3d_align_workspace_bytes(int n_q, int n_t);
int e3d_align_pairs(const uint8_t* q_codes, const int32_t* q_off, const uint8_t* t_codes, const int32_t* t_off,
                    const int8_t* subst, int32_t* score, int32_t* matches, int32_t* columns, void* workspace,
                    int64_t workspace_bytes, int n_q, int n_t, int n_q_codes, int n_t_codes, int gap_open, int gap_extend,
                    int upper_only, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* E3D_HIP_H */
