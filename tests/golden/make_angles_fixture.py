#!/usr/bin/env python3
"""Generate tests/golden/backbone_angles.pt by RUNNING the reference's angle functions.

    python tests/golden/make_angles_fixture.py <root of the reference checkout>

clean_data/data_preprocessing.py imports Biopython and DSSP wrappers at module level, so its two numpy-only functions
-- ``calc_angle`` and ``calc_dihedral`` -- are ast-extracted and exec'd, and the neighbour pattern of
``extract_angle_dihedrals`` (data_preprocessing.py:688-731: which atoms of residues i-1, i, i+1 feed which column) is
applied here to coordinates PROMOTED TO float64.  Nothing of the reference is copied into the repo: only coordinates in
(float32) and radians out (float64) are saved.

Coordinates come from oracle.nerf.backbone_coords, cast to float32.  No dihedral of any case lies within 1e-3 rad of 0
or +-pi (asserted): there the reference's arccos of the clipped cosine and its sign are exact to ~1e-12, and its
behaviour at exact planarity (np.sign(0) = 0 multiplies the angle) stays out of the fixture.
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import nerf as onerf  # noqa: E402

COLUMNS = ("omega", "phi", "psi", "dihedral_o", "theta1", "theta2", "theta3", "theta_o")
MARGIN = 1e-3


def load_reference(src):
    tree = ast.parse(open(src).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("calc_angle", "calc_dihedral")]
    assert len(keep) == 2, [n.name for n in keep]
    env = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), src, "exec"), env)
    return env["calc_angle"], env["calc_dihedral"]


def reference_angles(calc_angle, calc_dihedral, coords):
    """extract_angle_dihedrals on [n,4,3] float64 coordinates -> radians [n,8]; rows 0 and n-1 (no neighbours) zero."""
    out = np.zeros((coords.shape[0], 8))
    for i in range(1, coords.shape[0] - 1):
        prev_CA, prev_C = coords[i - 1, 1], coords[i - 1, 2]
        res_N, res_CA, res_C, res_O = coords[i]
        next_N = coords[i + 1, 0]
        out[i] = np.radians([
            calc_dihedral(prev_CA, prev_C, res_N, res_CA),
            calc_dihedral(prev_C, res_N, res_CA, res_C),
            calc_dihedral(res_N, res_CA, res_C, next_N),
            calc_dihedral(res_N, res_CA, res_C, res_O),
            calc_angle(res_N, res_CA, res_C),
            calc_angle(res_CA, res_C, next_N),
            calc_angle(prev_C, res_N, res_CA),
            calc_angle(res_CA, res_C, res_O),
        ])
    return out


def random_angles(rng, n):
    """[n,8] float32 in oracle.nerf.COLS order; dihedrals at least 2 * MARGIN away from 0 and +-pi."""
    ang = np.empty((n, 8), dtype=np.float32)
    mag = rng.uniform(2 * MARGIN, np.pi - 2 * MARGIN, (n, 4))
    ang[:, :4] = mag * rng.choice([-1.0, 1.0], (n, 4))
    ang[:, 4:] = rng.normal(1.95, 0.1, (n, 4))
    return ang


if __name__ == "__main__":
    src = os.path.join(sys.argv[1], "clean_data", "data_preprocessing.py")
    calc_angle, calc_dihedral = load_reference(src)
    rng = np.random.default_rng(0)
    inputs = []
    for n in (3, 4, 33, 70):
        ang = random_angles(rng, n)
        for center in (True, False):
            inputs.append((f"random_n{n}_{'centred' if center else 'uncentred'}", ang, center))
    ang = random_angles(rng, 33)
    ang[:, 2] = np.pi - rng.uniform(0.001 + MARGIN, 0.05, 33)          # every omega in (pi - 0.05, pi - 0.001)
    inputs.append(("omega_near_trans", ang, True))
    ang = random_angles(rng, 33)
    ang[:, 2] = rng.uniform(2 * MARGIN, 0.05, 33) * rng.choice([-1.0, 1.0], 33)   # omegas within 0.05 of 0 (cis)
    inputs.append(("omega_near_cis", ang, True))
    ang = random_angles(rng, 33)
    ang[:, 1] = (np.pi - rng.uniform(2 * MARGIN, 0.05, 33)) * np.where(np.arange(33) % 2, -1.0, 1.0)   # psi straddles +-pi
    inputs.append(("psi_straddles_pi", ang, False))

    cases = []
    for name, ang, center in inputs:
        xyz32 = onerf.backbone_coords(ang, center).reshape(-1, 4, 3).astype(np.float32)
        want = reference_angles(calc_angle, calc_dihedral, xyz32.astype(np.float64))
        dih = want[1:-1, :4]
        assert np.isfinite(want).all(), name
        assert (np.abs(dih) > MARGIN).all() and (np.abs(dih) < np.pi - MARGIN).all(), (name, np.abs(dih).min(), np.abs(dih).max())
        cases.append({"name": name, "coords": torch.from_numpy(xyz32), "angles": torch.from_numpy(want)})
    torch.save({"columns": list(COLUMNS), "cases": cases}, os.path.join(HERE, "backbone_angles.pt"))
    print(f"wrote backbone_angles.pt: {len(cases)} cases, {sum(c['coords'].shape[0] for c in cases)} residues")
