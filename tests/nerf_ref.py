"""The reference side of the NeRF backbone builder's tests (csrc/nerf.hip, ``nerf_backbone_kernel``): numpy, float64, CPU.

GROUND TRUTH is ``oracle.nerf.backbone_coords``, pinned bit for bit to the reference's builder by tests/golden/nerf.pt.  It
is not restated here: ``batch_reference`` calls it per chain under the kernel's batch contract, ``chain_allowance`` runs its own
code with perturbed values (below), and ``internal_coordinates`` goes the other way, from coordinates back to the inputs.

WHAT THE KERNEL COMPUTES PER PLACED ATOM.  Atom D is placed from its three predecessors a, b, c as D = c + M d with the
orthonormal frame M = (bc, n x bc, n), bc = unit(c - b), n = unit((b - a) x bc), in float64, and
    d0 = -len * cosf(A)            d1 = len * cosf(T) * sinf(A)            d2 = len * sinf(T) * sinf(A)
in FLOAT32 (len the bond length as a float32 constant, A the bond angle, T the torsion, both float32 inputs), evaluated left
to right.  Per residue i the four placements are (``PLACEMENTS``):
    k = 0   N(i)   from N, CA, C of i-1     len 1.34   A = CA:C:1N[i-1]   T = psi[i-1]
    k = 1   CA(i)  from CA, C of i-1, N(i)  len 1.46   A = 1C:N:CA[i-1]   T = omega[i-1]
    k = 2   C(i)   from C(i-1), N(i), CA(i) len 1.54   A = tau[i-1]       T = phi[i]
    k = 3   O(i)   from N, CA, C of i       len 1.22   A = CA:C:O[i]      T = dihedral_o[i]
Residue 0 has only k = 3: its N, CA, C are the builder's fixed first frame.

U_TRIG, THE ULP BOUND OF THE DEVICE'S sinf AND cosf.  U_TRIG = 1: the HIP math API reference ("HIP math API", table "Single
precision mathematical functions" of the HIP documentation in the ROCm documentation set) lists ``sinf`` and ``cosf`` with a
maximum error of 1 ulp -- the same table the project's other derivations take ``expf`` and ``logf`` from (1 ulp each,
tests/test_design_gpu.py).  A ROCm installation carries the runtime API reference but not necessarily the math API pages, so the
figure is cited from the published table; no test reads it from an installed copy.  numpy's
float32 ``sin`` / ``cos`` (the oracle's) are good to about an ulp as well, which ``test_nerf_ref_cpu.py`` confirms by holding the
oracle itself to ``internal_bound``.

``internal_bound``, DERIVED FROM THOSE OPERATIONS (e = 2^-23: one float32 ulp of x is at most e |x|, a rounding e / 2):
    d0 carries the rounding of len to float32 (e/2), cosf (U_TRIG e) and one product (e/2):      |dd0| <= (U_TRIG + 1) e |d0|
    d1, d2 carry len (e/2), two functions (2 U_TRIG e) and two products (e):               |dd1,2| <= (2 U_TRIG + 1.5) e |d1,2|
  M is orthonormal, so the recovered internal coordinates of D are those of d:
    length  r = |d|:          |dr| <= sum_j |d_j| |dd_j| / r <= (2 U_TRIG + 1.5) e len
    angle   A = atan2(rho, -d0), rho = |(d1, d2)| = len sin A:  |dA| = |x drho - rho dx| / len^2 with x = len cos A
                              <= ((2 U_TRIG + 1.5) + (U_TRIG + 1)) e |sin A cos A| = (3 U_TRIG + 2.5) e |sin A cos A|
    torsion T = atan2(d2, d1): |dT| = |d1 dd2 - d2 dd1| / rho^2 <= 2 (2 U_TRIG + 1.5) e |sin T cos T| = (2 U_TRIG + 1.5) e |sin 2T|
  The relative errors cancel out of a torsion exactly where it is 0 or pi, and out of a bond angle at pi / 2; what is left there is
  float64 rounding.  THE FLOAT64 FLOOR: every stored coordinate is rounded at the structure's coordinate magnitude A_max (eps64 / 2
  each; once more when the mean is subtracted), the frame is orthonormal to a few eps64, and the recomputation here forms
  differences of such coordinates: a bond vector is good to <= 4 eps64 (1 + A_max) in norm, a length therefore too, an angle to
  that over the shorter bond (>= 1.22), a torsion to that over rho = len sin A of the placed atom and over the same of the frame's
  own bond angle -- this is where a dihedral becomes ill-conditioned as sin(bond angle) -> 0.  ``floor`` = 32 eps64 (1 + A_max) for
  lengths and angles and 64 eps64 (1 + A_max) / sin A for torsions, plus 8 e^2 for the second-order terms dropped above, covers
  that for bond angles in [1.6, 2.3] rad (sin >= 0.745), which ``internal_bound`` REQUIRES of its input and the case generators
  guarantee.  The floor is ~1e-12 against ~4e-7 of the float32 terms.  Nothing here is fitted to the kernel.

``chain_allowance``, MEASURED ON THE REFERENCE.  Errors of the kind above do not stay local in the COORDINATES: a rotation of
one frame moves every later atom by (angle x distance).  How much is a property of the chain, so it is measured on the chain:
the oracle's own code is run with each of the three d components of every placement moved by a uniform random amount of up
to +-U float32 ulps, U = U_TRIG + 1 (the function's error plus one for the rounding of the products), 32 seeded draws; the
per-atom allowance is 2 x the largest displacement |perturbed - unperturbed| over the draws (2: a maximum over random draws
underestimates the worst case) + 16 eps64 max|coordinate| (a few float64 roundings of the coordinate magnitude: the kernel may
contract a * b + c and sums the mean in another order).  The perturbation is injected by handing the oracle module a numpy
proxy whose ``stack`` moves the one stack of three scalars in ``place_dihedral`` (the d vector); every other call passes through.
"""
import numpy as np

from oracle import nerf as onerf

U_TRIG = 1                      # documented maximum ulp error of sinf / cosf (docstring)
U = U_TRIG + 1                  # ulps each d component is moved by in chain_allowance
E32 = 2.0 ** -23
EPS64 = float(np.finfo(np.float64).eps)
DRAWS, MARGIN, FLOOR_ROUNDINGS = 32, 2.0, 16.0
ANGLE_RANGE = (1.6, 2.3)        # bond angles of every generated case; internal_bound requires it

# k: (bond length, bond-angle column, its residue offset, torsion column, its residue offset)   [onerf.COLS order]
PLACEMENTS = ((onerf.C_N_LENGTH, 5, -1, 1, -1), (onerf.N_CA_LENGTH, 6, -1, 2, -1), (onerf.CA_C_LENGTH, 4, -1, 0, 0),
              (onerf.C_O_LENGTH, 7, 0, 3, 0))
HELIX, STRAND, EXTENDED = (-57.0, -47.0), (-139.0, 135.0), (180.0, 180.0)


# ------------------------------------------------------------------------------------------------ case generators
def random_chain(n, seed):
    """The fixture's distribution: dihedrals uniform in (-pi, pi), bond angles N(1.95, 0.1) clipped to ANGLE_RANGE."""
    rng = np.random.default_rng([20240611, seed])
    ang = np.empty((n, 8), dtype=np.float32)
    ang[:, :4] = rng.uniform(-np.pi, np.pi, (n, 4))
    ang[:, 4:] = np.clip(rng.normal(1.95, 0.1, (n, 4)), *ANGLE_RANGE)
    return ang


def regular_chain(phi_psi_deg, n):
    """n residues of one (phi, psi): HELIX, STRAND or EXTENDED (the long straight chain: largest uncentred coordinates)."""
    import dssp_ref
    return dssp_ref.builder_angles([phi_psi_deg] * n)


# ------------------------------------------------------------------------------------------------ the batch contract
def batch_reference(angles, lengths, center):
    """angles [B,L,8] float32, lengths [B] -> float64 [B,L,4,3] under the kernel's contract: lengths clamped to [0, L], zero
    padding, an item of length 0 all zeros, each chain ``backbone_coords`` of its first ``len`` rows (rows beyond are not read)."""
    angles = np.asarray(angles, dtype=np.float32)
    B, L, _ = angles.shape
    out = np.zeros((B, L, 4, 3), dtype=np.float64)
    for b, n in enumerate(np.clip(np.asarray(lengths, dtype=np.int64), 0, L)):
        if n > 0:
            out[b, :n] = onerf.backbone_coords(angles[b, :n], bool(center)).reshape(n, 4, 3)
    return out


# ------------------------------------------------------------------------------------------------ internal coordinates
def _dihedral(a, b, c, d):
    b1, b2, b3 = b - a, c - b, d - c
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    return np.arctan2(np.linalg.norm(b2, axis=-1) * (b1 * n2).sum(-1), (n1 * n2).sum(-1))


def _angle(b, c, d):
    u, v = b - c, d - c
    return np.arctan2(np.linalg.norm(np.cross(u, v), axis=-1), (u * v).sum(-1))


def internal_coordinates(xyz):
    """xyz [n,4,3] -> {"length", "angle", "dihedral"}: float64 [n,4] each, entry [i,k] the internal coordinates that place atom
    k of residue i from its three predecessors (PLACEMENTS).  [0, :3] is NaN: the first frame is given, not placed."""
    X = np.asarray(xyz, dtype=np.float64).reshape(-1, 4, 3)
    n = X.shape[0]
    out = {k: np.full((n, 4), np.nan) for k in ("length", "angle", "dihedral")}
    bb = X[:, :3].reshape(-1, 3)                                     # N0 CA0 C0 N1 ...
    quads = [(bb[:-3], bb[1:-2], bb[2:-1], bb[3:], (slice(1, None), slice(0, 3))),
             (X[:, 0], X[:, 1], X[:, 2], X[:, 3], (slice(None), 3))]
    for a, b, c, d, where in quads:
        if len(d) == 0:
            continue
        shape = out["length"][where].shape
        out["length"][where] = np.linalg.norm(d - c, axis=-1).reshape(shape)
        out["angle"][where] = _angle(b, c, d).reshape(shape)
        out["dihedral"][where] = _dihedral(a, b, c, d).reshape(shape)
    return out


def expected_internal(angles):
    """The same layout from the INPUT: the constants and the angle columns each placement uses (as float64)."""
    ang = np.asarray(angles, dtype=np.float32).astype(np.float64)
    n = ang.shape[0]
    out = {k: np.full((n, 4), np.nan) for k in ("length", "angle", "dihedral")}
    for k, (length, acol, aoff, tcol, toff) in enumerate(PLACEMENTS):
        lo = 1 if k < 3 else 0
        rows = np.arange(lo, n)
        out["length"][rows, k] = length
        out["angle"][rows, k] = ang[rows + aoff, acol]
        out["dihedral"][rows, k] = ang[rows + toff, tcol]
    return out


def internal_bound(angles, coord_scale):
    """The bounds of the module docstring in the layout of ``internal_coordinates``; ``coord_scale`` = max |coordinate|."""
    want = expected_internal(angles)
    A, T = want["angle"], want["dihedral"]
    used = A[np.isfinite(A)]
    assert used.size == 0 or (used.min() >= ANGLE_RANGE[0] - 1e-6 and used.max() <= ANGLE_RANGE[1] + 1e-6), \
        "internal_bound is derived for bond angles in ANGLE_RANGE"
    floor = 32.0 * EPS64 * (1.0 + coord_scale) + 8.0 * E32 * E32
    return {"length": (2 * U_TRIG + 1.5) * E32 * want["length"] + floor,
            "angle": (3 * U_TRIG + 2.5) * E32 * np.abs(np.sin(A) * np.cos(A)) + floor,
            "dihedral": (2 * U_TRIG + 1.5) * E32 * np.abs(np.sin(2.0 * T)) + 2.0 * floor / np.sin(A)}


def internal_ratio(xyz, angles):
    """Worst |recovered - input| / internal_bound over the chain, per kind: {"length", "angle", "dihedral"} (0.0 when the
    chain defines none).  Torsion differences are wrapped."""
    X = np.asarray(xyz, dtype=np.float64).reshape(-1, 4, 3)
    got, want = internal_coordinates(X), expected_internal(angles)
    bound = internal_bound(angles, float(np.abs(X).max()))
    worst = {}
    for kind in got:
        diff = got[kind] - want[kind]
        if kind == "dihedral":
            diff = (diff + np.pi) % (2.0 * np.pi) - np.pi
        ok = np.isfinite(want[kind])
        assert np.isfinite(got[kind][ok]).all(), f"non-finite recovered {kind}"
        worst[kind] = float((np.abs(diff[ok]) / bound[kind][ok]).max()) if ok.any() else 0.0
    return worst


# ------------------------------------------------------------------------------------------------ the global allowance
class _PerturbingNumpy:
    """numpy, except that a ``stack`` of scalars -- the d vector of ``place_dihedral`` -- moves each by up to +-u float32 ulps."""

    def __init__(self, rng, u):
        self._rng, self._u = rng, u

    def __getattr__(self, name):
        return getattr(np, name)

    def stack(self, arrays, axis=0, **kw):
        if all(np.ndim(x) == 0 for x in arrays):
            arrays = [np.float64(x) + self._rng.uniform(-self._u, self._u) * np.float64(np.spacing(np.abs(np.float32(x))))
                      for x in arrays]
        return np.stack(arrays, axis=axis, **kw)


_perturbed, _allowance = {}, {}


def perturbed_coords(angles):
    """[DRAWS, 4n, 3]: the oracle's uncentred coordinates with every d component moved by up to +-U ulps; draw k is seeded
    by k alone.  Cached per chain (the CPU and GPU tests share chains)."""
    angles = np.ascontiguousarray(angles, dtype=np.float32)
    key = angles.tobytes()
    if key not in _perturbed:
        runs = []
        try:
            for k in range(DRAWS):
                onerf.np = _PerturbingNumpy(np.random.default_rng([977, k]), U)
                runs.append(onerf.backbone_coords(angles, False))
        finally:
            onerf.np = np
        _perturbed[key] = np.stack(runs)
    return _perturbed[key]


def chain_allowance(angles, center):
    """angles [n,8] -> float64 [n,4]: the allowed |got - reference| (Euclidean, per atom) for this chain (module docstring)."""
    angles = np.ascontiguousarray(angles, dtype=np.float32)
    key = (angles.tobytes(), bool(center))
    if key not in _allowance:
        _allowance[key] = _measure_allowance(angles, center)
    return _allowance[key]


def _measure_allowance(angles, center):
    ref = onerf.backbone_coords(angles, False)
    runs = perturbed_coords(angles)
    scale = float(np.abs(ref).max())
    if center:
        ref, runs = ref - ref.mean(axis=0), runs - runs.mean(axis=1, keepdims=True)
    moved = np.linalg.norm(runs - ref[None], axis=-1).max(axis=0)
    return (MARGIN * moved + FLOOR_ROUNDINGS * EPS64 * scale).reshape(-1, 4)


def allowance_ratio(got, ref, angles, center):
    """Worst |got - ref| / chain_allowance over the atoms of one chain; got, ref [n,4,3]."""
    err = np.linalg.norm(np.asarray(got, dtype=np.float64) - ref, axis=-1)
    return float((err / chain_allowance(angles, center)).max())


def mean_floor(n_atoms, coord_scale):
    """|mean of a centred chain|, and |centred - (uncentred - its float64 mean)|: a sequential float64 sum of n terms of
    magnitude <= A is good to (n - 1) (eps64 / 2) n A, its mean to (n / 2) eps64 A; the subtraction rounds each coordinate by
    eps64 / 2 of itself, and the comparison's own mean and difference add as much: (n / 2 + 4) eps64 A."""
    return (0.5 * n_atoms + 4.0) * EPS64 * coord_scale
