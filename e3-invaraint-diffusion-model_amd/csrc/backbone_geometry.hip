// What a backbone IS, from N, CA, C, O alone (evaluate.py, featurize.py): secondary structure after Kabsch & Sander
// (Biopolymers 22, 2577 (1983)), backbone hydrogen bonds, bends and clashes.  The step after nerf.hip that needs no
// native structure, and the column of a record the reference took from an external DSSP program.
//
// All structures of a call lie back to back, residues off[s] .. off[s+1]-1 of structure s; every index below must lie
// inside the residue's own structure, and a residue's results are a function of its structure's coordinates alone (the
// same arithmetic in the same order wherever the structure stands in the call).  All float64.
//     valid(i)      all twelve coordinates of residue i are finite.  A residue that is not valid takes part in nothing,
//                   breaks contiguity and gets '-' and status 1.
//     bonded(i)     i is not the first of its structure, valid(i-1), valid(i), |C[i-1] - N[i]| <= max_peptide_bond.
//     contig(a, b)  bonded(k) for all a < k <= b.
//     H[i]          N[i] + unit(C[i-1] - O[i-1]); exists iff bonded(i), i is not a proline and |C[i-1] - O[i-1]| > 0.
//     E(a, d)       C=O of a accepting N-H of d; defined iff |a - d| >= 2, valid(a), H[d] exists, |CA[a] - CA[d]| < 9:
//                   27.888 (((1/|O_a N_d| + 1/|C_a H_d|) - 1/|O_a H_d|) - 1/|C_a N_d|) kcal/mol, floored at -9.9, and -9.9
//                   outright when one of the four distances is below 0.5.       hbond(a, d) := E(a, d) < -0.5.
//     n-turn at i   contig(i, i+n) and hbond(i, i+n), n = 3, 4, 5.
//     H             on s .. s+3 when the 4-turns at s-1 and s exist.
//     G             on s .. s+2 when the 3-turns at s-1 and s exist and none of the three residues is H, B or E.
//     I             on s .. s+4 when the 5-turns at s-1 and s exist and none of the five residues is H, B, E or G.
//     bridge(i, j)  contig(i-1, i+1), contig(j-1, j+1), |i - j| >= 3;
//                   parallel      [hbond(i-1, j) and hbond(j, i+1)] or [hbond(j-1, i) and hbond(i, j+1)]
//                   antiparallel  [hbond(i, j) and hbond(j, i)] or [hbond(i-1, j+1) and hbond(j-1, i+1)]
//     E / B         i has a bridge of type t with some j: E when (i+-1, j+-1) (parallel) or (i+-1, j-+1) (antiparallel)
//                   is a bridge of type t too for one such j, else B.
//     T             residues k+1 .. k+n-1 of an n-turn at k.
//     S             contig(i-2, i+2) and kappa(i) > 70 degrees; kappa = atan2(|u x w|, u . w), u = CA[i] - CA[i-2],
//                   w = CA[i+2] - CA[i], in degrees; NaN where contig(i-2, i+2) does not hold.
//     letter        the first that applies of H, B, E, G, I, T, S, '-': the index into "HBEGITS-".
//     partners      of the N-H of d: the two lowest E(a, d) < 0 as (a - d, E); of the C=O of a: the two lowest
//                   E(a, d) < 0 as (d - a, E); ties go to the lower index; an absent partner is (0, 0.0), as DSSP
//                   prints it.  hbonds[d] counts the a with hbond(a, d).
//     clash[i]      atom pairs (atom of i, atom of j), |i - j| >= 2, both valid, closer than clash_cutoff.  The cutoff is
//                   the caller's choice, not a standard.  A structure's clash number is half the sum over its residues.
// THREE DIFFERENCES FROM DSSP: turns and bridges test the full relation E < -0.5, not DSSP's two best partners per
// side; pairs with |a - d| = 1 have no energy; energies are not rounded to 0.001.  There are no beta-bulges and no
// sheet labels.  Agreement with the mkdssp program has not been measured.
//
// Launches of one call, on one stream.  (1) Every residue gets status 3, '-' and empty results.  Launches 2 to 4 run
// one column of workgroups per structure, which checks its two offsets -- 0 <= off[s] <= off[s+1] <= R, else it leaves,
// and nothing is read through such an offset -- with a thread per residue.  (2) valid(i) and bonded(i), staged in
// ``ss``.  (3) Energies, partners, clashes, kappa and the residue's own flags (turn starts, bridge, ladder, bend) as
// pure functions of the coordinates and of launch 2's bits, O(n) pairs each; the flags are staged in the upper bits of
// ``status``.  (4) The letter, from the flags of the residues within ten positions, replaces the staged bits in
// ``ss``.  (5) The staging bits of ``status`` are cleared.  No launch reads an array that it writes, and loops run over
// fixed index ranges: no atomics, no host synchronisation, nothing waits for convergence.  Residues held by no good
// structure keep what launch 1 wrote.  Structures that overlap are memory-safe and otherwise undefined.
#include "e3d_common.h"

namespace {

constexpr double Q_ENERGY = 27.888, E_FLOOR = -9.9, E_HBOND = -0.5, CA_CUTOFF = 9.0, R_MIN = 0.5, KAPPA_BEND = 70.0;
constexpr double DEG_PER_RAD = 57.295779513082320876798;
constexpr int SS_NONE = 7;
constexpr int CHUNKS = 4, THREADS = 256;   // CHUNKS workgroups stride over the residues of one structure
// staged in ss by launch 2
constexpr int S_VALID = 1, S_BONDED = 2;
// staged in status >> 8 by launch 3
constexpr int F_TURN3 = 1, F_TURN4 = 2, F_TURN5 = 4, F_BRIDGE = 8, F_LADDER = 16, F_BEND = 32;

struct V3 { double x, y, z; };
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double dist2(V3 a, V3 b) { const V3 d = sub(a, b); return dot(d, d); }

enum { AT_N = 0, AT_CA = 1, AT_C = 2, AT_O = 3 };

// One structure as the threads see it: residues lo .. hi-1 of the call
struct Chain {
    const double* __restrict__ xyz;
    const uint8_t* __restrict__ pro;
    const uint8_t* __restrict__ stage;   // S_VALID | S_BONDED per residue (launch 2)
    int lo, hi;
    __device__ __forceinline__ bool inside(int i) const { return i >= lo && i < hi; }
    __device__ __forceinline__ V3 atom(int i, int a) const {
        const double* p = xyz + 12 * (int64_t)i + 3 * a;
        return {p[0], p[1], p[2]};
    }
    __device__ __forceinline__ bool valid(int i) const { return stage[i] & S_VALID; }
    __device__ __forceinline__ bool bonded(int i) const { return i > lo && i < hi && (stage[i] & S_BONDED); }
    __device__ bool contig(int a, int b) const {   // b - a <= 5 everywhere below
        if (a < lo || b >= hi) return false;
        for (int k = a + 1; k <= b; ++k)
            if (!bonded(k)) return false;
        return true;
    }
    // E(a, d); false: not defined
    __device__ bool energy(int a, int d, double& e) const {
        if (!inside(a) || !inside(d) || (a - d < 2 && d - a < 2)) return false;
        if (!(dist2(atom(a, AT_CA), atom(d, AT_CA)) < CA_CUTOFF * CA_CUTOFF)) return false;   // most pairs end here
        if (!valid(a) || !bonded(d) || (pro && pro[d])) return false;
        const V3 n = atom(d, AT_N), co = sub(atom(d - 1, AT_C), atom(d - 1, AT_O));
        const double len = sqrt(dot(co, co));
        if (!(len > 0.0)) return false;
        const V3 h = {n.x + co.x / len, n.y + co.y / len, n.z + co.z / len};
        const V3 c = atom(a, AT_C), o = atom(a, AT_O);
        const double r_on = sqrt(dist2(o, n)), r_ch = sqrt(dist2(c, h)), r_oh = sqrt(dist2(o, h)), r_cn = sqrt(dist2(c, n));
        if (r_on < R_MIN || r_ch < R_MIN || r_oh < R_MIN || r_cn < R_MIN) {
            e = E_FLOOR;
        } else {
            e = Q_ENERGY * (((1.0 / r_on + 1.0 / r_ch) - 1.0 / r_oh) - 1.0 / r_cn);
            e = e < E_FLOOR ? E_FLOOR : e;
        }
        return true;
    }
    __device__ bool hbond(int a, int d) const {
        double e;
        return energy(a, d, e) && e < E_HBOND;
    }
    // bit 0: parallel, bit 1: antiparallel
    __device__ int bridge(int i, int j) const {
        if (i - j < 3 && j - i < 3) return 0;
        if (!contig(i - 1, i + 1) || !contig(j - 1, j + 1)) return 0;   // also: i-1, i+1, j-1, j+1 inside
        // the four pairs of bonds, one body (kept a loop: unrolled, the energy code is copied forty times per kernel):
        //   0  hbond(i-1, j) and hbond(j, i+1)        1  the same with i and j exchanged: hbond(j-1, i) and hbond(i, j+1)
        //   2  hbond(i, j) and hbond(j, i)            3  hbond(i-1, j+1) and hbond(j-1, i+1)
        int t = 0;
#pragma nounroll
        for (int k = 0; k < 4; ++k) {
            const int x = k == 1 ? j : i, y = k == 1 ? i : j;
            const int a1 = k == 2 ? x : x - 1, d1 = k == 3 ? y + 1 : y;
            const int a2 = k == 3 ? y - 1 : y, d2 = k == 2 ? x : x + 1;
            if (hbond(a1, d1) && hbond(a2, d2)) t |= k < 2 ? 1 : 2;
        }
        return t;
    }
};

// the two lowest energies below zero met so far, in index order (a tie keeps the earlier, lower index)
struct Best2 {
    int rel[2] = {0, 0};
    double e[2] = {0.0, 0.0};
    __device__ __forceinline__ void offer(int r, double v) {
        if (v < e[0]) {
            rel[1] = rel[0]; e[1] = e[0];
            rel[0] = r; e[0] = v;
        } else if (v < e[1]) {
            rel[1] = r; e[1] = v;
        }
    }
};

struct Out {
    uint8_t* ss;
    int32_t* acc_rel; double* acc_e;
    int32_t* don_rel; double* don_e;
    double* kappa;
    int32_t *clash, *hbonds, *status;
};

__global__ __launch_bounds__(256) void geometry_fill_kernel(Out o, int R) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R) return;
    o.ss[i] = SS_NONE;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        o.acc_rel[2 * (int64_t)i + k] = 0; o.acc_e[2 * (int64_t)i + k] = 0.0;
        o.don_rel[2 * (int64_t)i + k] = 0; o.don_e[2 * (int64_t)i + k] = 0.0;
    }
    o.kappa[i] = __longlong_as_double(0x7ff8000000000000ll);
    o.clash[i] = 0;
    o.hbonds[i] = 0;
    o.status[i] = 3;
}

// the structure of this column of workgroups; false: bad offsets, nothing of it may be touched
__device__ __forceinline__ bool chain_of_block(const double* xyz, const int32_t* off, const uint8_t* pro,
                                               const uint8_t* stage, int R, Chain& c) {
    const int lo = off[blockIdx.x], hi = off[blockIdx.x + 1];
    if (lo < 0 || hi > R || hi < lo) return false;
    c = {xyz, pro, stage, lo, hi};
    return true;
}

__device__ __forceinline__ bool finite_residue(const double* __restrict__ xyz, int i) {
    const double* p = xyz + 12 * (int64_t)i;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 12; ++k) ok = ok & isfinite(p[k]);   // '&': twelve independent loads, not a chain of branches
    return ok;
}

__global__ __launch_bounds__(THREADS) void geometry_stage_kernel(const double* __restrict__ xyz,
                                                                 const int32_t* __restrict__ off,
                                                                 uint8_t* __restrict__ stage, int R, double bond2) {
    Chain c;
    if (!chain_of_block(xyz, off, nullptr, nullptr, R, c)) return;
    for (int i = c.lo + blockIdx.y * THREADS + threadIdx.x; i < c.hi; i += CHUNKS * THREADS) {
        const bool valid = finite_residue(xyz, i);
        const bool bonded = valid && i > c.lo && finite_residue(xyz, i - 1) &&
                            dist2(c.atom(i - 1, AT_C), c.atom(i, AT_N)) <= bond2;
        stage[i] = (uint8_t)((valid ? S_VALID : 0) | (bonded ? S_BONDED : 0));
    }
}

__global__ __launch_bounds__(THREADS) void geometry_residue_kernel(const double* __restrict__ xyz,
                                                                   const int32_t* __restrict__ off,
                                                                   const uint8_t* __restrict__ pro, Out o, int R,
                                                                   double clash2) {
    Chain c;
    if (!chain_of_block(xyz, off, pro, o.ss, R, c)) return;   // o.ss: launch 2's bits, read only here
    for (int i = c.lo + blockIdx.y * THREADS + threadIdx.x; i < c.hi; i += CHUNKS * THREADS) {
        if (!c.valid(i)) {
            o.status[i] = 1;   // everything else as the fill left it
            continue;
        }
        V3 mine[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) mine[a] = c.atom(i, a);
        Best2 acc, don;
        int clash = 0, hbonds = 0, flags = 0;
        for (int j = c.lo; j < c.hi; ++j) {
            if (j - i < 2 && i - j < 2) continue;
            if (c.valid(j)) {
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) clash += dist2(mine[a], c.atom(j, b)) < clash2;
            }
            double e;
            if (c.energy(j, i, e)) {   // j accepts this residue's N-H
                if (e < 0.0) acc.offer(j - i, e);
                hbonds += e < E_HBOND;
            }
            if (c.energy(i, j, e) && e < 0.0) don.offer(j - i, e);   // this residue's C=O accepts j's N-H
            const int t = c.bridge(i, j);
            if (t) {
                flags |= F_BRIDGE;
#pragma nounroll
                for (int k = 0; k < 4; ++k) {   // (i-1, j-1), (i+1, j+1) parallel; (i-1, j+1), (i+1, j-1) antiparallel
                    const int di = (k & 1) ? 1 : -1, dj = k < 2 ? di : -di, type = k < 2 ? 1 : 2;
                    if ((t & type) && (c.bridge(i + di, j + dj) & type)) flags |= F_LADDER;
                }
            }
        }
#pragma nounroll
        for (int n = 3; n <= 5; ++n)
            if (c.contig(i, i + n) && c.hbond(i, i + n)) flags |= F_TURN3 << (n - 3);
        if (c.contig(i - 2, i + 2)) {
            const V3 u = sub(mine[AT_CA], c.atom(i - 2, AT_CA)), w = sub(c.atom(i + 2, AT_CA), mine[AT_CA]);
            const V3 x = {u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x};
            const double kappa = atan2(sqrt(dot(x, x)), dot(u, w)) * DEG_PER_RAD;
            o.kappa[i] = kappa;
            if (kappa > KAPPA_BEND) flags |= F_BEND;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            o.acc_rel[2 * (int64_t)i + k] = acc.rel[k]; o.acc_e[2 * (int64_t)i + k] = acc.e[k];
            o.don_rel[2 * (int64_t)i + k] = don.rel[k]; o.don_e[2 * (int64_t)i + k] = don.e[k];
        }
        o.clash[i] = clash;
        o.hbonds[i] = hbonds;
        o.status[i] = flags << 8;
    }
}

// The staged flags of residue k, 0 outside the structure.  A residue that is not valid staged none.
struct Flags {
    const int32_t* __restrict__ status;
    int lo, hi;
    __device__ __forceinline__ int at(int k) const { return k >= lo && k < hi ? status[k] >> 8 : 0; }
    __device__ __forceinline__ bool pair(int s, int f) const { return (at(s - 1) & f) && (at(s) & f); }   // helix start s
    __device__ bool is_h(int k) const {
        for (int s = k - 3; s <= k; ++s)
            if (pair(s, F_TURN4)) return true;
        return false;
    }
    __device__ bool is_hbe(int k) const { return (at(k) & F_BRIDGE) || is_h(k); }
    __device__ bool is_g(int k) const {
        for (int s = k - 2; s <= k; ++s)
            if (pair(s, F_TURN3) && !is_hbe(s) && !is_hbe(s + 1) && !is_hbe(s + 2)) return true;
        return false;
    }
    __device__ bool is_i(int k) const {
        for (int s = k - 4; s <= k; ++s) {
            if (!pair(s, F_TURN5)) continue;
            bool free_run = true;
            for (int m = s; m < s + 5; ++m) free_run = free_run && !is_hbe(m) && !is_g(m);
            if (free_run) return true;
        }
        return false;
    }
    __device__ bool is_t(int k) const {
        return (at(k - 1) & (F_TURN3 | F_TURN4 | F_TURN5)) || (at(k - 2) & (F_TURN3 | F_TURN4 | F_TURN5)) ||
               (at(k - 3) & (F_TURN4 | F_TURN5)) || (at(k - 4) & F_TURN5);
    }
};

__global__ __launch_bounds__(THREADS) void geometry_letter_kernel(const int32_t* __restrict__ off, Out o, int R) {
    Chain c;
    if (!chain_of_block(nullptr, off, nullptr, nullptr, R, c)) return;
    const Flags f = {o.status, c.lo, c.hi};
    for (int i = c.lo + blockIdx.y * THREADS + threadIdx.x; i < c.hi; i += CHUNKS * THREADS) {
        const int mine = f.at(i);
        int ss = SS_NONE;   // every residue of the structure is written: ss held launch 2's bits until here
        if ((o.status[i] & 0xff) != 0) {}   // not valid: '-'
        else if (f.is_h(i)) ss = 0;
        else if (mine & F_BRIDGE) ss = (mine & F_LADDER) ? 2 : 1;
        else if (f.is_g(i)) ss = 3;
        else if (f.is_i(i)) ss = 4;
        else if (f.is_t(i)) ss = 5;
        else if (mine & F_BEND) ss = 6;
        o.ss[i] = (uint8_t)ss;
    }
}

__global__ __launch_bounds__(256) void geometry_unstage_kernel(int32_t* __restrict__ status, int R) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < R) status[i] &= 0xff;
}

}  // namespace

extern "C" int e3d_backbone_geometry(const double* coords, const int32_t* off, const uint8_t* is_pro, uint8_t* ss,
                                     int32_t* acc_rel, double* acc_e, int32_t* don_rel, double* don_e, double* kappa,
                                     int32_t* clash, int32_t* hbonds, int32_t* status, int n_structs, int n_residues,
                                     double clash_cutoff, double max_peptide_bond, void* stream) {
    E3D_REQUIRE(coords && off && ss && acc_rel && acc_e && don_rel && don_e && kappa && clash && hbonds && status,
                "backbone_geometry: null pointer");
    E3D_REQUIRE(n_structs > 0 && n_residues > 0, "backbone_geometry: %d structures, %d residues, need all > 0", n_structs,
                n_residues);
    E3D_REQUIRE(clash_cutoff > 0.0 && isfinite(clash_cutoff) && max_peptide_bond > 0.0 && isfinite(max_peptide_bond),
                "backbone_geometry: clash_cutoff = %g, max_peptide_bond = %g, need both > 0 and finite", clash_cutoff,
                max_peptide_bond);
    const Out o = {ss, acc_rel, acc_e, don_rel, don_e, kappa, clash, hbonds, status};
    const hipStream_t s = (hipStream_t)stream;
    const dim3 per_residue((n_residues + 255) / 256), per_chain(n_structs, CHUNKS);
    hipLaunchKernelGGL(geometry_fill_kernel, per_residue, dim3(256), 0, s, o, n_residues);
    hipLaunchKernelGGL(geometry_stage_kernel, per_chain, dim3(THREADS), 0, s, coords, off, ss, n_residues,
                       max_peptide_bond * max_peptide_bond);
    hipLaunchKernelGGL(geometry_residue_kernel, per_chain, dim3(THREADS), 0, s, coords, off, is_pro, o, n_residues,
                       clash_cutoff * clash_cutoff);
    hipLaunchKernelGGL(geometry_letter_kernel, per_chain, dim3(THREADS), 0, s, off, o, n_residues);
    hipLaunchKernelGGL(geometry_unstage_kernel, per_residue, dim3(256), 0, s, status, n_residues);
    return e3d_launch_status("e3d_backbone_geometry");
}
