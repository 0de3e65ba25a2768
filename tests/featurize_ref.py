"""Test infrastructure: the eight stored backbone angles as a plain float64 numpy statement (atan2 forms).

Written from the definitions (biolip.STORED_ANGLE_COLUMNS), not from the kernel: pinned against the reference's own
calc_angle / calc_dihedral by tests/golden/backbone_angles.pt (test_featurize_cpu.py)."""
import numpy as np

COLUMNS = ("omega", "phi", "psi", "dihedral_o", "theta1", "theta2", "theta3", "theta_o")


def dihedral(p1, p2, p3, p4):
    """Signed dihedral of four points (arrays [..., 3]) in radians; sign = sign((n1 x n2) . v2)."""
    v1, v2, v3 = p2 - p1, p3 - p2, p4 - p3
    n1, n2 = np.cross(v1, v2), np.cross(v2, v3)
    v2u = v2 / np.linalg.norm(v2, axis=-1, keepdims=True)
    return np.arctan2((np.cross(n1, n2) * v2u).sum(-1), (n1 * n2).sum(-1))


def angle(p1, p2, p3):
    """Angle at p2 in radians."""
    u, w = p1 - p2, p3 - p2
    return np.arctan2(np.linalg.norm(np.cross(u, w), axis=-1), (u * w).sum(-1))


def chain_angles(coords):
    """coords [n,4,3] (N, CA, C, O of ONE chain; any float dtype, promoted to float64) -> float64 [n,8] in COLUMNS order;
    the first and last row, which have no two neighbours, are zero."""
    x = np.asarray(coords, dtype=np.float64).reshape(-1, 4, 3)
    out = np.zeros((x.shape[0], 8))
    if x.shape[0] < 3:
        return out
    n, ca, c, o = (x[1:-1, k] for k in range(4))
    pca, pc, nn = x[:-2, 1], x[:-2, 2], x[2:, 0]
    out[1:-1] = np.stack([dihedral(pca, pc, n, ca), dihedral(pc, n, ca, c), dihedral(n, ca, c, nn), dihedral(n, ca, c, o),
                          angle(n, ca, c), angle(ca, c, nn), angle(pc, n, ca), angle(ca, c, o)], axis=-1)
    return out


def wrapped(d):
    """|d| on the circle."""
    return np.abs((np.asarray(d) + np.pi) % (2 * np.pi) - np.pi)


def column_map(A):
    """Angles A [n,8] in oracle.nerf.COLS order (what the NeRF builder consumes) -> what chain_angles must recover for the
    interior residues 1 .. n-2, [n-2, 8] in COLUMNS order: omega and the bond angles tau and 1C:N:CA that PLACE residue i
    are stored on residue i-1 of the builder's input."""
    A = np.asarray(A, dtype=np.float64)
    i = np.arange(1, A.shape[0] - 1)
    return np.stack([A[i - 1, 2], A[i, 0], A[i, 1], A[i, 3], A[i - 1, 4], A[i, 5], A[i - 1, 6], A[i, 7]], axis=-1)


ONE_TO_THREE = {"A": "ALA", "C": "CYS", "D": "ASP", "E": "GLU", "F": "PHE", "G": "GLY", "H": "HIS", "I": "ILE", "K": "LYS",
                "L": "LEU", "M": "MET", "N": "ASN", "P": "PRO", "Q": "GLN", "R": "ARG", "S": "SER", "T": "THR", "V": "VAL",
                "W": "TRP", "Y": "TYR"}


def pdb_text_for_chains(chains):
    """[(chain id, one-letter sequence, coords [n,4,3])] -> backbone-only PDB text, three decimals as the format has."""
    lines, serial = [], 0
    for chain_id, seq, xyz in chains:
        for r, aa in enumerate(seq):
            for k, (name, element) in enumerate((("N", "N"), ("CA", "C"), ("C", "C"), ("O", "O"))):
                serial += 1
                x, y, z = (float(v) for v in xyz[r][k])
                lines.append("ATOM  %5d  %-3s %3s %1s%4d    %8.3f%8.3f%8.3f%6.2f%6.2f          %2s" % (
                    serial, name, ONE_TO_THREE[aa], chain_id, r + 1, x, y, z, 1.0, 5.0, element))
        lines.append("TER")
    lines.append("END")
    return "\n".join(lines) + "\n"
