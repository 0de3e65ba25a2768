"""Test infrastructure: optimal rigid superposition as a plain float64 numpy statement (Kabsch, by SVD).

Written from the definition, not from the kernel (csrc/superpose.hip solves a 4x4 eigenproblem instead):
    minimise over proper rotations R (det R = +1) and translations t     msd = (1/n) sum_i | R a_i + t - b_i |^2
    centre both sets; H = sum (a_i - abar)(b_i - bbar)^T = U diag(s) V^T; d = sign(det(V U^T));
    R = V diag(1, 1, d) U^T;  t = bbar - R abar;  msd = (G - 2 (s0 + s1 + d s2)) / n,  G = sum |a - abar|^2 + sum |b - bbar|^2
``x' = R x + t`` maps the mobile set ``a`` onto the reference set ``b``."""
import numpy as np

EPS64 = float(np.finfo(np.float64).eps)


def superpose(a, b, proper=True):
    """a, b [n,3] -> (msd, R [3,3], t [3], G).  ``proper=False`` skips the det correction (the minimum over rotations AND
    reflections): for tests that show the difference."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3)
    assert a.shape == b.shape and a.shape[0] > 0, (a.shape, b.shape)
    n = a.shape[0]
    abar, bbar = a.mean(0), b.mean(0)
    ac, bc = a - abar, b - bbar
    G = float((ac * ac).sum() + (bc * bc).sum())
    U, s, Vt = np.linalg.svd(ac.T @ bc)
    d = np.sign(np.linalg.det(Vt.T @ U.T)) if proper else 1.0
    d = 1.0 if d == 0 else d
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    msd = max(0.0, (G - 2.0 * (s[0] + s[1] + d * s[2])) / n)
    return msd, R, bbar - R @ abar, G


def msd_of(a, b, R, t, dtype=np.float64):
    """The mean squared deviation that a GIVEN transform leaves: (1/n) sum | R a + t - b |^2, evaluated directly in ``dtype``
    (np.longdouble keeps the evaluation's own rounding, ~eps |x| per coordinate of UNCENTRED atoms, out of the result)."""
    a, b = np.asarray(a, dtype=dtype).reshape(-1, 3), np.asarray(b, dtype=dtype).reshape(-1, 3)
    d = a @ np.asarray(R, dtype=dtype).reshape(3, 3).T + np.asarray(t, dtype=dtype).reshape(3) - b
    return float((d * d).sum() / a.shape[0])


def translation_allowance(a, b, t):
    """What the float64 REPRESENTATION of t may add to the msd a transform leaves.  t = bbar - R abar is three products and
    three additions per component, each rounded to eps64 of its magnitude: |e| <= 8 eps64 (|abar| + |bbar| + |t|).  A common
    shift e of all atoms changes the msd by 2 e . mean(residual) + |e|^2, and the mean residual vanishes at the optimal t: |e|^2."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3)
    e = 8.0 * EPS64 * (np.linalg.norm(a.mean(0)) + np.linalg.norm(b.mean(0)) + np.linalg.norm(t))
    return float(e * e)


def msd_bound(G, n, units=32.0):
    """units x eps64 x G / n: the error unit of an msd formed as (G - 2 lambda) / n.  Two independent float64 evaluations
    (this SVD, and eigvalsh of Horn's matrix) stay within 4.5 units of a 40-digit evaluation; a raw-moment evaluation is at
    215 to 4e5; 32 admits other summation orders and rejects the wrong algorithm."""
    return units * EPS64 * G / n


def pairwise_rmsd(structs):
    """[R] arrays [n,3] of equal n -> symmetric [R,R] RMSD matrix with a zero diagonal."""
    m = np.zeros((len(structs), len(structs)))
    for i in range(len(structs)):
        for j in range(i + 1, len(structs)):
            m[i, j] = m[j, i] = np.sqrt(superpose(structs[i], structs[j])[0])
    return m


def medoid(mat):
    """The index with the smallest mean RMSD to the others (lowest index on ties); 0 for a single structure."""
    mat = np.asarray(mat, dtype=np.float64)
    return int(np.argmin(mat.sum(1)))


def random_rotation(rng):
    """A proper rotation, uniform on SO(3) (a normalised Gaussian quaternion)."""
    w, x, y, z = (q := rng.normal(size=4)) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def random_walk(rng, n, step=3.8, origin=20.0):
    """A chain of n points, consecutive ones ``step`` apart (the C-alpha spacing), starting ~``origin`` from zero."""
    d = rng.normal(size=(n, 3))
    d *= step / np.linalg.norm(d, axis=1, keepdims=True)
    d[0] = rng.normal(size=3)
    d[0] *= origin / np.linalg.norm(d[0])
    return np.cumsum(d, axis=0)


KINDS = ("independent", "rigid", "rigid_shifted", "mirrored", "rigid_noise")


def pair_of_kind(rng, n, kind):
    """(mobile a, reference b), both [n,3]: ``a`` a random walk; ``b`` another walk, or a rigid copy of ``a`` (plain, shifted
    by (1000, -2000, 500) A, of its mirror image, or with 1e-3 A of Gaussian noise)."""
    a = random_walk(rng, n)
    if kind == "independent":
        return a, random_walk(rng, n)
    R, t = random_rotation(rng), rng.normal(size=3) * 10.0
    if kind == "rigid":
        return a, a @ R.T + t
    if kind == "rigid_shifted":
        return a, a @ R.T + np.array([1000.0, -2000.0, 500.0])
    if kind == "mirrored":
        return a, (a * np.array([-1.0, 1.0, 1.0])) @ R.T + t
    if kind == "rigid_noise":
        return a, a @ R.T + t + 1e-3 * rng.normal(size=(n, 3))
    raise ValueError(kind)


def superpose_pairs(xyz, off, mob, ref):
    """The export's contract, pair by pair in numpy: (msd [P], R [P,3,3], t [P,3], status [P], G [P]); NaN where the status
    is not 0 (1 atom counts differ, 2 empty, 3 bad index or offset, 4 non-finite coordinate)."""
    xyz, off = np.asarray(xyz, dtype=np.float64).reshape(-1, 3), np.asarray(off).astype(np.int64)
    P, n_structs, n_atoms = len(mob), len(off) - 1, xyz.shape[0]
    msd, R, t = np.full(P, np.nan), np.full((P, 3, 3), np.nan), np.full((P, 3), np.nan)
    status, G = np.zeros(P, dtype=np.int32), np.full(P, np.nan)
    for p, (m, r) in enumerate(zip(mob, ref)):
        if not (0 <= m < n_structs and 0 <= r < n_structs):
            status[p] = 3
            continue
        (a0, a1), (b0, b1) = off[m:m + 2], off[r:r + 2]
        if not (0 <= a0 <= a1 <= n_atoms and 0 <= b0 <= b1 <= n_atoms):
            status[p] = 3
        elif a1 - a0 != b1 - b0:
            status[p] = 1
        elif a1 == a0:
            status[p] = 2
        elif not (np.isfinite(xyz[a0:a1]).all() and np.isfinite(xyz[b0:b1]).all()):
            status[p] = 4
        else:
            msd[p], R[p], t[p], G[p] = superpose(xyz[a0:a1], xyz[b0:b1])
    return msd, R, t, status, G


def torch_superpose(xyz, off, mob, ref, transform=True):
    """``superpose_pairs`` with the signature and return types of ``evaluate.superpose``, for injection on a CPU."""
    import torch
    msd, R, t, status, _ = superpose_pairs(xyz.numpy(), off.numpy(), mob.numpy(), ref.numpy())
    return (torch.from_numpy(np.sqrt(msd)), torch.from_numpy(R) if transform else None,
            torch.from_numpy(t) if transform else None, torch.from_numpy(status))
