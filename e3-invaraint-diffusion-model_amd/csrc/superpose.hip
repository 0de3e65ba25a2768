// Optimal rigid superposition of structure pairs (evaluate.py): the step after nerf.hip -- how far is a sampled
// backbone from the native one, and from the other samples of its pocket.
//
// superpose_pairs_kernel: for pair p, the proper rotation R (det R = +1) and translation t that minimise
//     msd = (1/n) sum_i | R a_i + t - b_i |^2        a = atoms of structure mob[p] (mobile), b = of ref[p] (reference)
// and that minimum.  x' = R x + t maps the mobile structure onto the reference one.
// Arithmetic, all float64 (as nerf.hip and backbone_angles.hip):
//     pass 1   the two centroids (6 sums)
//     pass 2   the centred cross-covariance S[j][k] = sum (a - abar)_j (b - bbar)_k and G = sum |a - abar|^2 + sum |b - bbar|^2
//              (11 sums).  Raw moments (sum a b^T - n abar bbar^T) lose hundreds of units of G eps to cancellation and are
//              not used.
//     solve    Horn's symmetric 4x4 matrix N(S) (J. Opt. Soc. Am. A 4, 629 (1987)): its largest eigenvalue lambda belongs to
//              the unit quaternion q of R, and msd = max(0, (G - 2 lambda) / n).  A quaternion is a rotation: no reflection
//              can come out, which is the point of this form.  Cyclic Jacobi, at most MAX_SWEEPS sweeps of six rotations: a
//              NaN that reaches the solve runs that many sweeps and ends in NaN, nothing waits for convergence alone.
//              lambda is the Rayleigh quotient q^T N q of the normalised eigenvector with the ORIGINAL N (second order in
//              the eigenvector's error, and free of the rotations' accumulated rounding).
// Mapping: one 64-lane wave per pair, four per 256-thread workgroup; lanes stride over the atoms; the sums are reduced by
// xor shuffles, which leave bit-identical totals in every lane (a + b == b + a), so the status decisions and the 4x4
// solve run uniformly in all lanes and lane 0 stores the results.  No LDS, no atomics.
// Status per pair (msd, R, t are NaN unless 0):
//     0  ok.  n = 1 gives msd 0 and R = identity; collinear and planar sets give one of their minimisers.
//     1  the two structures differ in atom count
//     2  both structures are empty
//     3  mob[p] or ref[p] outside [0, n_structs), or an offset of theirs outside [0, n_atoms] or descending: nothing is
//        read through such an index or offset
//     4  a non-finite coordinate (or coordinates so large that the float64 sums overflow)
#include "e3d_common.h"

namespace {

constexpr int MAX_SWEEPS = 16;   // a symmetric 4x4 converges to float64 rounding in 5-7 sweeps (quadratic convergence)

#define E3D_HD __host__ __device__ __forceinline__

// One Jacobi rotation in the (p, q) plane: A <- J^T A J with A[p][q] -> 0, V <- V J.  p, q are compile-time after unrolling.
E3D_HD void jacobi_rotate(double (&A)[4][4], double (&V)[4][4], int p, int q, int sweep) {
    const double apq = A[p][q];
    const double g = 100.0 * fabs(apq);
    if (sweep > 3 && fabs(A[p][p]) + g == fabs(A[p][p]) && fabs(A[q][q]) + g == fabs(A[q][q])) {
        A[p][q] = A[q][p] = 0.0;   // below the rounding of both diagonal entries
        return;
    }
    if (apq == 0.0) return;
    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double akp = A[k][p], akq = A[k][q];
        A[k][p] = c * akp - s * akq;
        A[k][q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double apk = A[p][k], aqk = A[q][k];
        A[p][k] = c * apk - s * aqk;
        A[q][k] = s * apk + c * aqk;
    }
    A[p][q] = A[q][p] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - s * vkq;
        V[k][q] = s * vkp + c * vkq;
    }
}

// S (row-major, S[3 j + k] = sum a_j b_k over centred coordinates) -> the largest eigenvalue of Horn's matrix and the
// rotation (row-major) of its unit quaternion.
E3D_HD double horn_rotation(const double (&S)[9], double (&R)[9]) {
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double N[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double A[4][4], V[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            A[i][j] = N[i][j];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < MAX_SWEEPS; ++sweep) {
        const double offd = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[0][3]) + fabs(A[1][2]) + fabs(A[1][3]) + fabs(A[2][3]);
        if (offd == 0.0) break;   // false for NaN: the sweeps then run out
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) jacobi_rotate(A, V, p, q, sweep);
    }
    double best = A[0][0], qv[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (A[j][j] > best) {   // ties (n = 1: all zero) keep the lowest index, the identity quaternion
            best = A[j][j];
#pragma unroll
            for (int k = 0; k < 4; ++k) qv[k] = V[k][j];
        }
    const double inv = 1.0 / sqrt(qv[0] * qv[0] + qv[1] * qv[1] + qv[2] * qv[2] + qv[3] * qv[3]);
    const double w = qv[0] * inv, x = qv[1] * inv, y = qv[2] * inv, z = qv[3] * inv;
    const double q4[4] = {w, x, y, z};
    double lambda = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double row = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) row += N[i][j] * q4[j];
        lambda += q4[i] * row;
    }
    R[0] = w * w + x * x - y * y - z * z; R[1] = 2.0 * (x * y - w * z);         R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (y * x + w * z);         R[4] = w * w - x * x + y * y - z * z; R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (z * x - w * y);         R[7] = 2.0 * (z * y + w * x);         R[8] = w * w - x * x - y * y + z * z;
    return lambda;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void superpose_pairs_kernel(const double* __restrict__ xyz, const int32_t* __restrict__ off,
                                                              const int32_t* __restrict__ mob,
                                                              const int32_t* __restrict__ ref, double* __restrict__ msd,
                                                              double* __restrict__ rot, double* __restrict__ trans,
                                                              int32_t* __restrict__ status, int n_structs, int n_atoms,
                                                              int n_pairs) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n_pairs) return;   // a whole wave leaves: nothing below synchronises across waves
    const int im = mob[p], ir = ref[p];
    int st = 0, a0 = 0, b0 = 0, n = 0;
    if (im < 0 || im >= n_structs || ir < 0 || ir >= n_structs) {
        st = 3;
    } else {   // the tables live on the device: nothing they hold may index outside a buffer
        a0 = off[im];
        b0 = off[ir];
        const int a1 = off[im + 1], b1 = off[ir + 1];
        if (a0 < 0 || a1 > n_atoms || a1 < a0 || b0 < 0 || b1 > n_atoms || b1 < b0) st = 3;
        else if (a1 - a0 != b1 - b0) st = 1;
        else if (a1 == a0) st = 2;
        n = a1 - a0;
    }
    const double* __restrict__ A = xyz + 3 * (int64_t)a0;
    const double* __restrict__ B = xyz + 3 * (int64_t)b0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double ca[3] = {0, 0, 0}, cb[3] = {0, 0, 0}, S[9], R[9], G = 0.0, lambda = 0.0;
    if (st == 0) {   // pass 1: centroids
        for (int i = lane; i < n; i += 64)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                ca[k] += A[3 * (int64_t)i + k];
                cb[k] += B[3 * (int64_t)i + k];
            }
        bool finite = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ca[k] = wave_sum_f64(ca[k]);
            cb[k] = wave_sum_f64(cb[k]);
            finite = finite && isfinite(ca[k]) && isfinite(cb[k]);   // a NaN or inf term makes its sum NaN or inf
            ca[k] /= (double)n;
            cb[k] /= (double)n;
        }
        if (!finite) st = 4;
    }
    if (st == 0) {   // pass 2: centred cross-covariance and G
#pragma unroll
        for (int k = 0; k < 9; ++k) S[k] = 0.0;
        double ga = 0.0, gb = 0.0;
        for (int i = lane; i < n; i += 64) {
            double a[3], b[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                a[k] = A[3 * (int64_t)i + k] - ca[k];
                b[k] = B[3 * (int64_t)i + k] - cb[k];
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                ga += a[j] * a[j];
                gb += b[j] * b[j];
#pragma unroll
                for (int k = 0; k < 3; ++k) S[3 * j + k] += a[j] * b[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) S[k] = wave_sum_f64(S[k]);
        G = wave_sum_f64(ga) + wave_sum_f64(gb);
        if (!isfinite(G)) st = 4;   // finite coordinates whose squares overflow
    }
    if (st == 0) lambda = horn_rotation(S, R);
    if (lane != 0) return;
    status[p] = st;
    if (st == 0) {
        const double v = (G - 2.0 * lambda) / (double)n;
        msd[p] = v > 0.0 ? v : (v <= 0.0 ? 0.0 : v);   // max(0, v) that keeps a NaN
    } else {
        msd[p] = nan;
    }
    if (rot) {
#pragma unroll
        for (int k = 0; k < 9; ++k) rot[9 * (int64_t)p + k] = st == 0 ? R[k] : nan;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            trans[3 * (int64_t)p + j] = st == 0 ? cb[j] - (R[3 * j] * ca[0] + R[3 * j + 1] * ca[1] + R[3 * j + 2] * ca[2]) : nan;
    }
}

}  // namespace

extern "C" int e3d_superpose_pairs(const double* xyz, const int32_t* off, const int32_t* mob, const int32_t* ref, double* msd,
                                   double* rot, double* trans, int32_t* status, int n_structs, int n_atoms, int n_pairs,
                                   void* stream) {
    E3D_REQUIRE(xyz && off && mob && ref && msd && status, "superpose_pairs: null pointer");
    E3D_REQUIRE((rot == nullptr) == (trans == nullptr), "superpose_pairs: rot and trans must both be given or both be null");
    E3D_REQUIRE(n_structs > 0 && n_atoms > 0 && n_pairs > 0, "superpose_pairs: %d structures, %d atoms, %d pairs, need all > 0",
                n_structs, n_atoms, n_pairs);
    hipLaunchKernelGGL(superpose_pairs_kernel, dim3((n_pairs + 3) / 4), dim3(256), 0, (hipStream_t)stream, xyz, off, mob, ref,
                       msd, rot, trans, status, n_structs, n_atoms, n_pairs);
    return e3d_launch_status("e3d_superpose_pairs");
}
