// Featurization of PDB coordinates (featurize.py): the inverse direction of nerf.hip.
//
// backbone_angles_kernel: N, CA, C, O coordinates of many chains laid back to back -> the eight internal angles the
// preprocessing stores per residue (clean_data/data_preprocessing.py:688-731), in biolip.STORED_ANGLE_COLUMNS order:
//     omega      dihedral(CA-1, C-1, N, CA)      theta1   angle(N, CA, C)
//     phi        dihedral(C-1, N, CA, C)         theta2   angle(CA, C, N+1)
//     psi        dihedral(N, CA, C, N+1)         theta3   angle(C-1, N, CA)
//     dihedral_o dihedral(N, CA, C, O)           theta_o  angle(CA, C, O)
// One thread per residue row.  A row is interior when both neighbours belong to its chain (seg[r-1] == seg[r] ==
// seg[r+1]); every other row -- the first and last residue of each chain, which the preprocessing drops -- gets zeros
// and status bit 0, and no thread reads a row of another chain or outside [0, R).
// Arithmetic: float64 algebra from the float32 coordinates (as nerf.hip), the atan2 forms
//     dihedral = atan2((n1 x n2) . v2 / |v2|, n1 . n2)      angle = atan2(|u x w|, u . w)
// which are well conditioned where the reference's arccos of a clipped cosine is not, one rounding to float32 at the
// end.  The dihedral's sign is the reference's, sign((n1 x n2) . v2).
// KNOWN DIFFERENCE from the reference: at EXACT planarity ((n1 x n2) . v2 == 0) the reference returns 0 for a trans
// arrangement too, because it multiplies arccos(..) = pi by np.sign(0) = 0; this kernel returns +-pi there.
// Status bits per row: 0 = not interior (zeros written); 1 = a zero-length bond or a zero plane normal (the reference
// raises or produces NaN; zeros written); 2 = C-1 - N or C - N+1 longer than max_peptide_bond: a chain break (the
// reference computes across breaks without notice, so the angles are still written).
//
// contact_residues_kernel: hit[row] = 1 when any atom of receptor residue ``row`` lies within ``cutoff`` of any ligand
// atom of the same complex.  One thread per receptor atom, all complexes in one launch.
#include "e3d_common.h"

namespace {

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 ld3(const float* p) { return {(double)p[0], (double)p[1], (double)p[2]}; }
__device__ __forceinline__ D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double norm(D3 a) { return sqrt(dot(a, a)); }

// false: degenerate (zero middle bond or a zero normal)
__device__ __forceinline__ bool dihedral(D3 p1, D3 p2, D3 p3, D3 p4, double& out) {
    const D3 v1 = sub(p2, p1), v2 = sub(p3, p2), v3 = sub(p4, p3);
    const D3 n1 = cross(v1, v2), n2 = cross(v2, v3);
    const double l2 = norm(v2);
    if (l2 == 0.0 || dot(n1, n1) == 0.0 || dot(n2, n2) == 0.0) return false;
    out = atan2(dot(cross(n1, n2), v2) / l2, dot(n1, n2));
    return true;
}
// angle at p2 between p1 and p3; false: a zero-length arm
__device__ __forceinline__ bool bond_angle(D3 p1, D3 p2, D3 p3, double& out) {
    const D3 u = sub(p2, p1), w = sub(p2, p3);
    if (dot(u, u) == 0.0 || dot(w, w) == 0.0) return false;
    out = atan2(norm(cross(u, w)), dot(u, w));
    return true;
}

__global__ __launch_bounds__(256) void backbone_angles_kernel(const float* __restrict__ coords,
                                                              const int32_t* __restrict__ seg,
                                                              float* __restrict__ angles, int32_t* __restrict__ status,
                                                              int R, double max_bond) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    float* o = angles + (int64_t)r * 8;
    bool interior = r > 0 && r < R - 1;
    if (interior) {   // the neighbours' seg entries are only read once both are known to exist
        const int32_t s = seg[r];
        interior = seg[r - 1] == s && seg[r + 1] == s;
    }
    double a[8];
    int st = 0;
    if (!interior) {
        st = 1;
    } else {
        const float* p = coords + (int64_t)r * 12;
        const D3 n = ld3(p), ca = ld3(p + 3), c = ld3(p + 6), ox = ld3(p + 9);
        const D3 pca = ld3(p - 12 + 3), pc = ld3(p - 12 + 6), nn = ld3(p + 12);
        bool ok = dihedral(pca, pc, n, ca, a[0]);
        ok = dihedral(pc, n, ca, c, a[1]) && ok;
        ok = dihedral(n, ca, c, nn, a[2]) && ok;
        ok = dihedral(n, ca, c, ox, a[3]) && ok;
        ok = bond_angle(n, ca, c, a[4]) && ok;
        ok = bond_angle(ca, c, nn, a[5]) && ok;
        ok = bond_angle(pc, n, ca, a[6]) && ok;
        ok = bond_angle(ca, c, ox, a[7]) && ok;
        if (!ok) st |= 2;
        if (norm(sub(n, pc)) > max_bond || norm(sub(nn, c)) > max_bond) st |= 4;
    }
    const bool zero = (st & 3) != 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = zero ? 0.f : (float)a[j];
    status[r] = st;
}

__global__ __launch_bounds__(256) void contact_zero_kernel(int32_t* __restrict__ hit, int n_rows) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rows) hit[i] = 0;
}

__global__ __launch_bounds__(256) void contact_residues_kernel(const float* __restrict__ rec_xyz,
                                                               const int32_t* __restrict__ rec_row,
                                                               const int32_t* __restrict__ rec_off,
                                                               const float* __restrict__ lig_xyz,
                                                               const int32_t* __restrict__ lig_off,
                                                               int32_t* __restrict__ hit, int n_complexes, int n_rec_atoms,
                                                               int n_lig_atoms, int n_rows, float cutoff2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec_atoms) return;
    const int row = rec_row[i];
    if (row < 0 || row >= n_rows) return;   // the tables live on the device: nothing they hold may index outside a buffer
    // the complex of atom i: the largest c with rec_off[c] <= i
    int lo = 0, hi = n_complexes - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rec_off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    if (i < rec_off[lo] || i >= rec_off[lo + 1]) return;   // an atom outside every complex's range touches nothing
    const int j0 = max(lig_off[lo], 0), j1 = min(lig_off[lo + 1], n_lig_atoms);
    const float x = rec_xyz[3 * (int64_t)i], y = rec_xyz[3 * (int64_t)i + 1], z = rec_xyz[3 * (int64_t)i + 2];
    for (int j = j0; j < j1; ++j) {
        const float dx = lig_xyz[3 * (int64_t)j] - x, dy = lig_xyz[3 * (int64_t)j + 1] - y, dz = lig_xyz[3 * (int64_t)j + 2] - z;
        if (fmaf(dx, dx, fmaf(dy, dy, dz * dz)) <= cutoff2) {
            atomicMax(hit + row, 1);
            return;
        }
    }
}

}  // namespace

extern "C" int e3d_backbone_angles(const float* coords, const int32_t* seg, float* angles, int32_t* status, int R,
                                   float max_peptide_bond, void* stream) {
    E3D_REQUIRE(coords && seg && angles && status, "backbone_angles: null pointer");
    E3D_REQUIRE(R > 0, "backbone_angles: R = %d rows, need > 0", R);
    E3D_REQUIRE(max_peptide_bond > 0.f, "backbone_angles: max_peptide_bond = %g, need > 0", (double)max_peptide_bond);
    hipLaunchKernelGGL(backbone_angles_kernel, dim3((R + 255) / 256), dim3(256), 0, (hipStream_t)stream, coords, seg,
                       angles, status, R, (double)max_peptide_bond);
    return e3d_launch_status("e3d_backbone_angles");
}

extern "C" int e3d_contact_residues(const float* rec_xyz, const int32_t* rec_row, const int32_t* rec_off,
                                    const float* lig_xyz, const int32_t* lig_off, int32_t* hit, int n_complexes,
                                    int n_rec_atoms, int n_lig_atoms, int n_rows, float cutoff, void* stream) {
    E3D_REQUIRE(rec_xyz && rec_row && rec_off && lig_off && hit && (lig_xyz || n_lig_atoms == 0),
                "contact_residues: null pointer");
    E3D_REQUIRE(n_complexes > 0 && n_rec_atoms > 0 && n_lig_atoms >= 0 && n_rows > 0,
                "contact_residues: %d complexes, %d receptor atoms, %d ligand atoms, %d rows", n_complexes, n_rec_atoms,
                n_lig_atoms, n_rows);
    E3D_REQUIRE(cutoff > 0.f, "contact_residues: cutoff = %g, need > 0", (double)cutoff);
    hipLaunchKernelGGL(contact_zero_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, hit, n_rows);
    if (n_lig_atoms > 0)   // no ligand atom anywhere: all zeros, and no second launch
        hipLaunchKernelGGL(contact_residues_kernel, dim3((n_rec_atoms + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                           rec_xyz, rec_row, rec_off, lig_xyz, lig_off, hit, n_complexes, n_rec_atoms, n_lig_atoms, n_rows,
                           cutoff * cutoff);
    return e3d_launch_status("e3d_contact_residues");
}
