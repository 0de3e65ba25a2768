"""numpy float64 restatement of csrc/backbone_geometry.hip: secondary structure, backbone hydrogen bonds, bends and
clashes from N, CA, C, O alone.  Written as loops over residues, for clarity and not for speed; THIS FILE IS THE
SPECIFICATION the kernel is tested against.  It follows Kabsch & Sander (Biopolymers 22, 2577 (1983)) with three stated
differences (below); the tests use no DSSP program, so agreement with ``mkdssp`` is neither claimed nor measured.

Rules, per structure (residues 0 .. n-1; every index below must lie inside the structure):
    valid(i)      all twelve coordinates of residue i are finite.  A residue that is not valid takes part in nothing, breaks
                  contiguity, and gets '-' and status 1.
    bonded(i)     i > 0, valid(i-1), valid(i) and |C[i-1] - N[i]| <= max_peptide_bond.
    contig(a, b)  bonded(k) for all a < k <= b.
    H[i]          N[i] + unit(C[i-1] - O[i-1]); exists iff bonded(i), i is not a proline and |C[i-1] - O[i-1]| > 0.
    E(a, d)       (C=O of a accepting N-H of d) defined iff |a - d| >= 2, valid(a), H[d] exists and |CA[a] - CA[d]| < 9:
                  27.888 (((1/|O_a N_d| + 1/|C_a H_d|) - 1/|O_a H_d|) - 1/|C_a N_d|), floored at -9.9, and -9.9 outright when
                  one of the four distances is below 0.5.         hbond(a, d) := E(a, d) < -0.5.
    n-turn at i   contig(i, i+n) and hbond(i, i+n), n = 3, 4, 5.
    H             on s .. s+3 when the 4-turns at s-1 and s exist.
    G             on s .. s+2 when the 3-turns at s-1 and s exist and none of the three residues is H, B or E.
    I             on s .. s+4 when the 5-turns at s-1 and s exist and none of the five residues is H, B, E or G.
    bridge(i, j)  contig(i-1, i+1), contig(j-1, j+1), |i - j| >= 3;
                  parallel      [hbond(i-1, j) and hbond(j, i+1)] or [hbond(j-1, i) and hbond(i, j+1)]
                  antiparallel  [hbond(i, j) and hbond(j, i)] or [hbond(i-1, j+1) and hbond(j-1, i+1)]
    E / B         i has a bridge of type t with some j: E when (i+-1, j+-1) (parallel) or (i+-1, j-+1) (antiparallel) is a
                  bridge of type t too for one such j, else B.
    T             residues k+1 .. k+n-1 of an n-turn at k.
    S             contig(i-2, i+2) and kappa(i) > 70 degrees; kappa = atan2(|u x w|, u . w) of u = CA[i] - CA[i-2],
                  w = CA[i+2] - CA[i], in degrees; NaN where contig(i-2, i+2) does not hold.
    letter        the first that applies of H, B, E, G, I, T, S, '-'.
    partners      of N-H of d: the two lowest E(a, d) < 0 as (a - d, E); of C=O of a: the two lowest E(a, d) < 0 as
                  (d - a, E); ties go to the lower index; an absent partner is (0, 0.0).  ``hbonds`` of d counts the a
                  with hbond(a, d).
    clash(i)      atom pairs (atom of i, atom of j), |i - j| >= 2, both valid, closer than clash_cutoff.
DIFFERENCES FROM DSSP: hbond is the full relation E < -0.5, not DSSP's two best partners per side; pairs with
|a - d| = 1 have no energy; energies are not rounded to 0.001.  There are no beta-bulges and no sheet labels.

MARGINS.  Every threshold decision is recorded with its distance to the threshold, relative to the threshold:
``energy`` |E + 0.5| / 0.5, ``ca`` |d_CA - 9| / 9, ``kappa`` |kappa - 70| / 70, ``clash`` |d - cutoff| / cutoff,
``peptide`` ||C - N| - max_peptide_bond| / max_peptide_bond, ``r`` |r - 0.5| / 0.5, and ``partner`` |E| (absolute: the
threshold is 0).  A test that demands EQUAL letters, counts and indices first asserts that no margin is below 1e-9, seven
orders of magnitude above float64 rounding of these expressions (bounds below).

ERROR BOUNDS, from the operations performed (u = eps64 / 2; both sides read the same float64 coordinates):
    a distance between two INPUT atoms: each difference is one rounding (relative u), three squares and two sums (3u), a
        correctly rounded square root (halves the 3u, adds u): relative error <= 3.5 u.
    H: the unit vector's components carry <= 4.5 u absolute (difference u, norm 2.5 u, quotient u, components <= 1); adding
        N rounds once more, u |H_c| <= u (A + 1) with A the structure's largest |coordinate|.  A distance r to H thus carries
        <= sqrt(3) u (5.5 + A) absolute on top of 3.5 u r: relative error <= u (3.5 + sqrt(3) (5.5 + A) / r).
    E: each term 27.888 / r inherits its distance's relative error plus a quotient and a product (2 u), and each of the
        three sums rounds by <= u sum |terms|.  One evaluation is within eps64 * 27.888 * sum_k (1 / r_k) (4 + (5 + A) / r_k);
        two evaluations (this file and the kernel, which may also contract a * b + c) differ by at most twice that, which
        ``energy_bound`` = 8 eps64 * 27.888 * sum_k (1 / r_k) (1 + (2 + A) / r_k) covers for every A >= 0.  The floor and
        the r < 0.5 rule are 1-Lipschitz or decided identically (margin ``r``), so the bound holds for them too.
    kappa: u and w carry u per component; the cross product's components <= 3 u (|ab| + |cd|), i.e. <= 6 sqrt(3) u |u||w| in
        norm, its norm 2.5 u more, the dot product <= 4 u |u||w|; atan2 moves by at most (|dy| + |dx|) / |u||w| <= 17 u, plus
        <= 2 ulp of its own result.  One evaluation: 8.5 eps64 + eps64 kappa; two: ``kappa_bound`` = 16 eps64 (2 + kappa)
        radians, converted to degrees.
The bounds are not fitted to the kernel; tests/test_geometry_gpu.py prints the worst observed ratio to them.
"""
import numpy as np

SS = "HBEGITS-"
Q_ENERGY, E_FLOOR, E_HBOND, CA_CUTOFF, R_MIN, KAPPA_BEND = 27.888, -9.9, -0.5, 9.0, 0.5, 70.0
EPS = float(np.finfo(np.float64).eps)
MARGIN_KINDS = ("energy", "ca", "kappa", "clash", "peptide", "r", "partner")
# backbone geometry of the analytic chains: omega, then the bond angles N:CA:C, CA:C:1N, 1C:N:CA, CA:C:O in degrees
OMEGA, BOND_ANGLES = np.pi, (111.0, 116.2, 121.7, 120.1)


def dist(a, b):
    d = a - b
    return float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))


def energy_bound(r, A):
    return 8.0 * EPS * Q_ENERGY * sum((1.0 / x) * (1.0 + (2.0 + A) / x) for x in r)


def kappa_bound(kappa_deg):
    return np.degrees(16.0 * EPS * (2.0 + np.radians(kappa_deg)))


def describe(X, is_pro=None, clash_cutoff=2.5, max_peptide_bond=2.5):
    """One structure: X float64 [n,4,3] (N, CA, C, O), is_pro bool [n] or None -> a dict of per-residue arrays (``ss`` the
    indices into SS, ``acc_rel`` / ``acc_e`` / ``don_rel`` / ``don_e`` [n,2], ``kappa``, ``clash``, ``hbonds``, ``status``),
    the bounds of the energies and of kappa (``acc_bound``, ``don_bound`` [n,2], ``kappa_bound`` [n]), ``letters`` (the
    string), ``energies`` {(a, d): E}, ``n_hbonds`` and ``margins`` {kind: the smallest relative margin}."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 4, 3)
    n = X.shape[0]
    N, CA, C, O = X[:, 0], X[:, 1], X[:, 2], X[:, 3]
    pro = np.zeros(n, dtype=bool) if is_pro is None else np.asarray(is_pro).astype(bool)
    valid = np.isfinite(X).all(axis=(1, 2))
    A = float(np.abs(X[valid]).max()) if valid.any() else 0.0
    margins = {k: np.inf for k in MARGIN_KINDS}

    def note(kind, value, threshold):
        margins[kind] = min(margins[kind], abs(value - threshold) / abs(threshold))

    # ---- contiguity and amide hydrogens
    bonded = np.zeros(n, dtype=bool)
    for i in range(1, n):
        if valid[i - 1] and valid[i]:
            d = dist(C[i - 1], N[i])
            note("peptide", d, max_peptide_bond)
            bonded[i] = d <= max_peptide_bond

    def contig(a, b):
        return a >= 0 and b < n and bool(bonded[a + 1:b + 1].all())

    H = {}
    for i in range(1, n):
        if bonded[i] and not pro[i]:
            co = dist(C[i - 1], O[i - 1])
            if co > 0.0:
                H[i] = N[i] + (C[i - 1] - O[i - 1]) / co

    # ---- energies of all defined pairs
    energies, bounds = {}, {}
    for d in H:
        for a in range(n):
            if abs(a - d) < 2 or not valid[a]:
                continue
            dca = dist(CA[a], CA[d])
            note("ca", dca, CA_CUTOFF)
            if not dca < CA_CUTOFF:
                continue
            r = (dist(O[a], N[d]), dist(C[a], H[d]), dist(O[a], H[d]), dist(C[a], N[d]))
            for x in r:
                note("r", x, R_MIN)
            if min(r) < R_MIN:
                e = E_FLOOR
            else:
                e = max(Q_ENERGY * (((1.0 / r[0] + 1.0 / r[1]) - 1.0 / r[2]) - 1.0 / r[3]), E_FLOOR)
            note("energy", e, E_HBOND)
            margins["partner"] = min(margins["partner"], abs(e))
            energies[a, d] = e
            bounds[a, d] = energy_bound([max(x, 1e-3) for x in r], A)

    def hbond(a, d):
        return (a, d) in energies and energies[a, d] < E_HBOND

    # ---- partners
    acc_rel, don_rel = np.zeros((n, 2), dtype=np.int32), np.zeros((n, 2), dtype=np.int32)
    acc_e, don_e, acc_b, don_b = (np.zeros((n, 2)) for _ in range(4))
    hbonds = np.zeros(n, dtype=np.int32)

    def offer(rel, en, bd, row, other, e, b):
        if e < en[row, 0]:
            rel[row, 1], en[row, 1], bd[row, 1] = rel[row, 0], en[row, 0], bd[row, 0]
            rel[row, 0], en[row, 0], bd[row, 0] = other - row, e, b
        elif e < en[row, 1]:
            rel[row, 1], en[row, 1], bd[row, 1] = other - row, e, b

    for (a, d) in sorted(energies):                 # ascending a, then d: each row meets its partners in index order
        offer(don_rel, don_e, don_b, a, d, energies[a, d], bounds[a, d])
    for (a, d) in sorted(energies, key=lambda p: (p[1], p[0])):
        offer(acc_rel, acc_e, acc_b, d, a, energies[a, d], bounds[a, d])
        hbonds[d] += energies[a, d] < E_HBOND

    # ---- turns, bridges, bends
    turn = {k: [contig(i, i + k) and hbond(i, i + k) for i in range(n)] for k in (3, 4, 5)}

    def bridge(i, j):
        """(parallel, antiparallel)"""
        if i < 1 or j < 1 or i > n - 2 or j > n - 2 or abs(i - j) < 3 or not contig(i - 1, i + 1) or not contig(j - 1, j + 1):
            return False, False
        par = (hbond(i - 1, j) and hbond(j, i + 1)) or (hbond(j - 1, i) and hbond(i, j + 1))
        anti = (hbond(i, j) and hbond(j, i)) or (hbond(i - 1, j + 1) and hbond(j - 1, i + 1))
        return par, anti

    has_bridge, ladder = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for i in range(n):
        for j in range(n):
            par, anti = bridge(i, j)
            if par:
                has_bridge[i] = True
                ladder[i] |= bridge(i - 1, j - 1)[0] or bridge(i + 1, j + 1)[0]
            if anti:
                has_bridge[i] = True
                ladder[i] |= bridge(i - 1, j + 1)[1] or bridge(i + 1, j - 1)[1]
    is_e, is_b = ladder, has_bridge & ~ladder

    kappa, kb, bend = np.full(n, np.nan), np.zeros(n), np.zeros(n, dtype=bool)
    for i in range(2, n - 2):
        if contig(i - 2, i + 2):
            u, w = CA[i] - CA[i - 2], CA[i + 2] - CA[i]
            c = np.cross(u, w)
            kappa[i] = np.degrees(np.arctan2(np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]),
                                             u[0] * w[0] + u[1] * w[1] + u[2] * w[2]))
            kb[i] = kappa_bound(kappa[i])
            note("kappa", kappa[i], KAPPA_BEND)
            bend[i] = kappa[i] > KAPPA_BEND

    # ---- letters
    is_h = np.zeros(n, dtype=bool)
    for s in range(1, n):
        if turn[4][s - 1] and turn[4][s]:
            is_h[s:s + 4] = True
    hbe = is_h | is_b | is_e
    is_g = np.zeros(n, dtype=bool)
    for s in range(1, n):
        if turn[3][s - 1] and turn[3][s] and not hbe[s:s + 3].any():
            is_g[s:s + 3] = True
    is_i = np.zeros(n, dtype=bool)
    for s in range(1, n):
        if turn[5][s - 1] and turn[5][s] and not (hbe | is_g)[s:s + 5].any():
            is_i[s:s + 5] = True
    is_t = np.zeros(n, dtype=bool)
    for k in (3, 4, 5):
        for s in range(n):
            if turn[k][s]:
                is_t[s + 1:s + k] = True
    ss = np.full(n, 7, dtype=np.uint8)
    for code, flag in reversed(list(zip(range(7), (is_h, is_b, is_e, is_g, is_i, is_t, bend)))):
        ss[flag] = code
    ss[~valid] = 7

    # ---- clashes: all atom pairs of residues at least two apart
    atoms = X.reshape(-1, 3)
    res = np.arange(4 * n) // 4
    ok = np.repeat(valid, 4)
    counted = (np.abs(res[:, None] - res[None, :]) >= 2) & ok[:, None] & ok[None, :]
    with np.errstate(invalid="ignore"):
        D = np.sqrt(((atoms[:, None, :] - atoms[None, :, :]) ** 2).sum(-1))
    if counted.any():
        margins["clash"] = float(np.abs(D[counted] - clash_cutoff).min() / clash_cutoff)
    clash = ((D < clash_cutoff) & counted).reshape(n, 4, n, 4).sum(axis=(1, 2, 3)).astype(np.int32)

    return dict(ss=ss, letters="".join(SS[c] for c in ss), acc_rel=acc_rel, acc_e=acc_e, don_rel=don_rel, don_e=don_e,
                acc_bound=acc_b, don_bound=don_b, kappa=kappa, kappa_bound=kb, clash=clash, hbonds=hbonds,
                status=np.where(valid, 0, 1).astype(np.int32), energies=energies,
                n_hbonds=sum(e < E_HBOND for e in energies.values()), margins=margins)


PER_RESIDUE = ("ss", "acc_rel", "acc_e", "don_rel", "don_e", "acc_bound", "don_bound", "kappa", "kappa_bound", "clash",
               "hbonds", "status")


def describe_call(coords, off, is_pro=None, clash_cutoff=2.5, max_peptide_bond=2.5, cache=None):
    """All structures of a call, as the export lays them out: coords [R,4,3], off [n_structs+1].  A structure whose
    offsets are not 0 <= off[s] <= off[s+1] <= R is skipped; residues that no good structure holds keep status 3, '-',
    absent partners, NaN kappa and zero counts.  ``cache`` (a dict) reuses the description of bit-identical structures."""
    coords = np.asarray(coords, dtype=np.float64).reshape(-1, 4, 3)
    R = coords.shape[0]
    out = dict(ss=np.full(R, 7, np.uint8), acc_rel=np.zeros((R, 2), np.int32), acc_e=np.zeros((R, 2)),
               don_rel=np.zeros((R, 2), np.int32), don_e=np.zeros((R, 2)), acc_bound=np.zeros((R, 2)),
               don_bound=np.zeros((R, 2)), kappa=np.full(R, np.nan), kappa_bound=np.zeros(R), clash=np.zeros(R, np.int32),
               hbonds=np.zeros(R, np.int32), status=np.full(R, 3, np.int32))
    margins = {k: np.inf for k in MARGIN_KINDS}
    structs = []
    for s in range(len(off) - 1):
        lo, hi = int(off[s]), int(off[s + 1])
        if not 0 <= lo <= hi <= R:
            structs.append(None)
            continue
        pro = None if is_pro is None else np.asarray(is_pro)[lo:hi]
        key = (coords[lo:hi].tobytes(), None if pro is None else pro.tobytes())
        one = cache.get(key) if cache is not None else None
        if one is None:
            one = describe(coords[lo:hi], pro, clash_cutoff, max_peptide_bond)
            if cache is not None:
                cache[key] = one
        for k in PER_RESIDUE:
            out[k][lo:hi] = one[k]
        for k in MARGIN_KINDS:
            margins[k] = min(margins[k], one["margins"][k])
        structs.append(one)
    out["margins"], out["structures"] = margins, structs
    return out


# ------------------------------------------------------------------------------------------------ analytic chains
def builder_angles(phi_psi_deg):
    """[(phi, psi)] in degrees -> the NeRF builder's [n,8] float32 input (oracle.nerf.COLS): omega = pi,
    dihedral_o = wrap(psi + pi), the four bond angles of BOND_ANGLES."""
    pp = np.radians(np.asarray(phi_psi_deg, dtype=np.float64).reshape(-1, 2))
    out = np.empty((pp.shape[0], 8), dtype=np.float32)
    out[:, 0], out[:, 1], out[:, 2] = pp[:, 0], pp[:, 1], OMEGA
    out[:, 3] = (pp[:, 1] + np.pi + np.pi) % (2 * np.pi) - np.pi
    out[:, 4:] = np.radians(BOND_ANGLES)
    return out


def chain_coords(phi_psi_deg):
    """The chain of ``builder_angles`` through the oracle's NeRF builder: float64 [n,4,3], centred."""
    from oracle import nerf as onerf
    return onerf.backbone_coords(builder_angles(phi_psi_deg), True).reshape(-1, 4, 3)


HAIRPIN = [(-120.0, 130.0)] * 6 + [(60.0, -120.0), (-90.0, 0.0)] + [(-120.0, 130.0)] * 6
ANALYTIC = {                                           # name: (phi / psi, the letters expected)
    "alpha": ([(-57.0, -47.0)] * 16, "-HHHHHHHHHHHHHH-"),
    "3-10": ([(-49.0, -26.0)] * 12, "-GGGGGGGGGG-"),
    "pi": ([(-57.0, -70.0)] * 14, "-IIIIIIIIIIII-"),
    "extended": ([(-139.0, 135.0)] * 12, "-" * 12),
    "polyproline": ([(-75.0, 145.0)] * 12, "-" * 12),
    "hairpin": (HAIRPIN, "-EEEEETTEEEEE-"),
}


def block_chain_angles(rng, n):
    """phi / psi (degrees) of an n-residue chain of concatenated blocks of 6 - 14 residues -- alpha, 3-10, pi, the
    hairpin, random, loose strand (-90, 120) +- 25 -- each angle with 4 degrees of jitter."""
    pp = []
    while len(pp) < n:
        kind, m = int(rng.integers(0, 6)), int(rng.integers(6, 15))
        if kind < 3:
            block = [ANALYTIC[("alpha", "3-10", "pi")[kind]][0][0]] * m
        elif kind == 3:
            block = HAIRPIN
        elif kind == 4:
            block = rng.uniform(-180.0, 180.0, (m, 2)).tolist()
        else:
            block = (np.array([-90.0, 120.0]) + rng.uniform(-25.0, 25.0, (m, 2))).tolist()
        pp += [tuple(v) for v in block]
    pp = np.asarray(pp[:n], dtype=np.float64)
    return pp + rng.normal(0.0, 4.0, pp.shape)
