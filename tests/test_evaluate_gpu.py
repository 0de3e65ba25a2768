"""GPU: the superposition kernel (csrc/superpose.hip) and the scoring of samples built on it (evaluate.py).

Tolerance of the kernel's mean squared deviation: 32 eps64 G / n (superpose_ref.msd_bound; G = the two centred sets' summed
squared norms).  Two independent float64 evaluations -- the SVD of superpose_ref and eigvalsh of Horn's matrix -- stay
within 4.5 of those units of a 40-digit evaluation over exactly the kinds and sizes used here, a raw-moment evaluation is
at 215 to 4e5: 32 admits another summation order and rejects the wrong algorithm.  Assertions are on msd, not on RMSD: on
rigid copies RMSD is only good to ~2e-6 A even in the reference (the square root of a cancelled difference).  Where a
wrapper returned RMSD its square is compared: the root and the square cost 2 more of those units at most."""
import numpy as np
import pytest
import torch

import featurize_ref as fr
import superpose_ref as sr
from oracle import nerf as onerf

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 3, 4, 63, 64, 65, 128, 129, 1024)       # the lane-stride edges and the largest backbone, 4 x 256
REPEATS = 3                                            # 10 sizes x 5 kinds x 3 = 150 pairs: not a multiple of 4


def nerf_angles(n, seed):
    rng = np.random.default_rng(seed)
    ang = np.empty((n, 8), dtype=np.float32)
    ang[:, :4] = rng.uniform(-np.pi, np.pi, (n, 4))
    ang[:, 4:] = rng.normal(1.95, 0.1, (n, 4))
    return ang


def pack(structs):
    """list of [n,3] -> (xyz [sum n, 3], off int32 [len + 1])"""
    off = np.cumsum([0] + [len(s) for s in structs]).astype(np.int32)
    return np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1, 3) for s in structs]), off


def launch(evaluate, xyz, off, mob, ref, transform=True):
    dev = [torch.from_numpy(np.asarray(a)).cuda() for a in (xyz, off, np.asarray(mob, np.int32), np.asarray(ref, np.int32))]
    msd, R, t, st = evaluate.superpose_msd(*dev, transform=transform)
    assert msd.dtype == torch.float64 and st.dtype == torch.int32
    return (msd.cpu().numpy(), None if R is None else R.cpu().numpy(), None if t is None else t.cpu().numpy(),
            st.cpu().numpy())


@pytest.fixture(scope="module")
def cases(pkg, hip):
    """Every (size, kind, repeat) pair, the reference of each (computed once) and the kernel's results of ONE launch."""
    from e3diff_amd import evaluate
    rng = np.random.default_rng(2024)
    meta, structs = [], []
    for n in SIZES:
        for kind in sr.KINDS:
            for _ in range(REPEATS):
                a, b = sr.pair_of_kind(rng, n, kind)
                meta.append((n, kind))
                structs += [a, b]
    xyz, off = pack(structs)
    P = len(meta)
    assert P % 4 != 0
    mob, ref = np.arange(P, dtype=np.int32) * 2, np.arange(P, dtype=np.int32) * 2 + 1
    want = sr.superpose_pairs(xyz, off, mob, ref)
    got = launch(evaluate, xyz, off, mob, ref)
    return dict(meta=meta, structs=structs, xyz=xyz, off=off, mob=mob, ref=ref, want=want, got=got)


# ------------------------------------------------------------------------------- 1. against the reference
def test_msd_matches_the_reference(pkg, hip, cases):
    from e3diff_amd import evaluate
    msd, _, _, st = cases["got"]
    want, _, _, want_st, G = cases["want"]
    assert not want_st.any() and not st.any()
    n = np.array([m[0] for m in cases["meta"]], dtype=np.float64)
    unit = sr.msd_bound(G, n, 1.0)
    err = np.abs(msd - want)
    ratio = np.where(unit > 0, err / np.where(unit > 0, unit, 1.0), 0.0)
    for kind in sr.KINDS:
        sel = np.array([m[1] == kind for m in cases["meta"]])
        print(f"{kind}: worst |msd - ref| = {ratio[sel].max():.2f} x eps64 G / n")
    print(f"worst observed ratio: {ratio.max():.2f} (bound 32)")
    assert (err <= sr.msd_bound(G, n)).all()
    assert (msd[n == 1] == 0.0).all()                                   # G = 0: the bound is 0 and the value exact
    # separate launches of 1 and of 5 pairs: the same values, bit for bit (a pair's wave does not depend on its place)
    for sel in ([37], [3, 44, 91, 149, 120]):
        again = launch(evaluate, cases["xyz"], cases["off"], cases["mob"][sel], cases["ref"][sel])
        assert not again[3].any() and np.array_equal(again[0], msd[sel])
        assert np.array_equal(again[1], cases["got"][1][sel]) and np.array_equal(again[2], cases["got"][2][sel])


# ------------------------------------------------------------------------------- 2. the transform
def test_transform_is_a_proper_rotation_onto_the_reference(pkg, hip, cases):
    msd, R, t, st = cases["got"]
    want, _, _, _, G = cases["want"]
    assert R.shape == (len(msd), 3, 3) and t.shape == (len(msd), 3)
    mirrored = 0
    for p, (n, kind) in enumerate(cases["meta"]):
        a, b = cases["structs"][2 * p], cases["structs"][2 * p + 1]
        # fp64 rounding of a normalised quaternion; an fp32 path fails this by five orders of magnitude
        assert np.abs(R[p] @ R[p].T - np.eye(3)).max() <= 1e-12 and np.linalg.det(R[p]) > 0, (n, kind)
        # x' = R x + t maps MOBILE onto REFERENCE: the deviation it leaves is the minimum (a rotation error d costs only
        # O(d^2), so this holds for collinear and planar sets too); a transposed R or a swapped direction is far off
        # evaluated in long double from the returned float64 R and t; what the rounding of t itself adds is second order
        # (superpose_ref.translation_allowance: ~1e-26 A^2 here, and all there is to allow when G = 0)
        left = sr.msd_of(a, b, R[p], t[p], dtype=np.longdouble)
        assert abs(left - want[p]) <= sr.msd_bound(G[p], n) + sr.translation_allowance(a, b, t[p]), (n, kind)
        if n == 1:
            assert np.array_equal(R[p], np.eye(3)) and np.array_equal(t[p], (b - a)[0])
        if kind == "mirrored" and n >= 8:
            mirrored += 1
            assert np.sqrt(want[p]) > 0.5, (n, np.sqrt(want[p]))          # the det-corrected reference: no reflection
            assert sr.superpose(a, b, proper=False)[0] <= sr.msd_bound(G[p], n)      # which a reflection would bring to 0
            assert abs(msd[p] - want[p]) <= sr.msd_bound(G[p], n)
    assert mirrored == 6 * REPEATS


# ------------------------------------------------------------------------------- 3. statuses
def test_statuses_in_one_launch(pkg, hip):
    from e3diff_amd import evaluate
    rng = np.random.default_rng(7)
    a, b = sr.pair_of_kind(rng, 5, "rigid_noise")
    c, d = sr.pair_of_kind(rng, 5, "independent")
    bad = a.copy()
    bad[3, 1] = np.nan
    structs = [a, b, sr.random_walk(rng, 4), np.zeros((0, 3)), bad, c, d]
    xyz, off = pack(structs)
    n_structs = len(structs)
    #      good   length  empty  index -1  index n_structs  NaN   good
    mob = [0,     0,      3,     -1,       0,               4,    5]
    ref = [1,     2,      3,     0,        n_structs,       0,    6]
    msd, R, t, st = launch(evaluate, xyz, off, mob, ref)
    assert st.tolist() == [0, 1, 2, 3, 3, 4, 0]
    assert np.isnan(msd[1:6]).all() and np.isnan(R[1:6]).all() and np.isnan(t[1:6]).all()
    # the good pairs are unaffected: the values of a launch that holds only them, and the reference's
    alone = launch(evaluate, xyz, off, [0, 5], [1, 6])
    assert not alone[3].any()
    for k in range(3):
        assert np.array_equal(alone[k], (msd, R, t)[k][[0, 6]])
    want = sr.superpose_pairs(xyz, off, mob, ref)
    assert want[3].tolist() == st.tolist()
    for p in (0, 6):
        assert abs(msd[p] - want[0][p]) <= sr.msd_bound(want[4][p], 5)
    # rot = trans = NULL: the same msd, bit for bit
    bare = launch(evaluate, xyz, off, mob, ref, transform=False)
    assert bare[1] is None and bare[2] is None and bare[3].tolist() == st.tolist()
    assert np.array_equal(bare[0], msd, equal_nan=True) and np.array_equal(bare[0][[0, 6]], msd[[0, 6]])
    # offsets past n_atoms: the coordinates handed over are a PREFIX (a view) of the buffer the table describes
    full = torch.from_numpy(xyz).cuda()
    head = full[:14]
    assert head.data_ptr() == full.data_ptr() and off.tolist() == [0, 5, 10, 14, 14, 19, 24, 29]
    idx = [torch.tensor(v, dtype=torch.int32).cuda() for v in ([0, 0, 3, 5], [1, 4, 3, 6])]
    cut = evaluate.superpose_msd(head, torch.from_numpy(off).cuda(), *idx)
    assert cut[3].tolist() == [0, 3, 2, 3] and float(cut[0][0]) == msd[0] and bool(torch.isnan(cut[0][1:]).all())
    # an inf counts as non-finite too, on either side of the pair
    bad[3, 1] = -np.inf
    xyz, off = pack(structs)
    assert launch(evaluate, xyz, off, [0, 4, 0], [1, 0, 4])[3].tolist() == [0, 4, 4]
    # the wrapper: RMSD = sqrt(msd), NaN where the status is not 0
    dev = [torch.from_numpy(np.asarray(v)).cuda() for v in (xyz, off, np.asarray([0, 0], np.int32), np.asarray([1, 2], np.int32))]
    rmsd, _, _, st2 = evaluate.superpose(*dev)
    assert st2.tolist() == [0, 1] and float(rmsd[0]) == np.sqrt(msd[0]) and bool(torch.isnan(rmsd[1]))


# ------------------------------------------------------------------------------- 4. pairwise matrices
def test_pairwise_matrices(pkg, hip):
    """Squares of the entries against the reference's msd; the bound as in test 1 (module docstring)."""
    from e3diff_amd import evaluate
    rng = np.random.default_rng(8)
    lengths = [5, 33, 33, 70, 70, 70, 70, 70]
    groups = [[0], [1, 2], [3, 4, 5, 6, 7]]
    coords = np.zeros((8, 70, 4, 3))
    for i, n in enumerate(lengths):
        base = sr.random_walk(rng, n)
        coords[i, :n] = base[:, None, :] + rng.normal(size=(n, 4, 3))
        coords[i, n:] = 1e6                                              # padding must not be read
    mats = evaluate.pairwise_rmsd(torch.from_numpy(coords).cuda(), torch.tensor(lengths), groups, atoms="CA")
    assert [tuple(m.shape) for m in mats] == [(1, 1), (2, 2), (5, 5)]
    assert all(m.is_cuda and m.dtype == torch.float64 for m in mats)
    assert mats[0].cpu().tolist() == [[0.0]]
    for g, mat in zip(groups, mats):
        mat = mat.cpu().numpy()
        assert np.array_equal(mat, mat.T) and not np.diag(mat).any()
        ca = [coords[i, :lengths[i], 1] for i in g]
        for x in range(len(g)):
            for y in range(x + 1, len(g)):
                want, _, _, G = sr.superpose(ca[x], ca[y])
                assert abs(mat[x, y] ** 2 - want) <= sr.msd_bound(G, len(ca[x])), (g, x, y)
        want = sr.pairwise_rmsd(ca)
        assert evaluate.medoid(torch.from_numpy(mat)) == sr.medoid(want) == int(np.argmin(want.sum(1)))
        assert evaluate.neighbour_counts(torch.from_numpy(mat).cuda(), 1e3).tolist() == [len(g) - 1] * len(g)
    # the whole backbone instead of the C-alphas: four atoms per residue
    bb = evaluate.pairwise_rmsd(torch.from_numpy(coords).cuda(), lengths, [[1, 2]], atoms="backbone")[0].cpu().numpy()
    want, _, _, G = sr.superpose(coords[1, :33].reshape(-1, 3), coords[2, :33].reshape(-1, 3))
    assert abs(bb[0, 1] ** 2 - want) <= sr.msd_bound(G, 4 * 33)


# ------------------------------------------------------------------------------- 5. the featurizer's convention
def test_round_trip_through_the_stored_columns(pkg, hip):
    """An oracle chain of n + 2 residues -> its stored angles (featurize_ref, interior rows, fp32) -> builder input
    (builder_angles_from_stored) -> the NeRF kernel -> RMSD to the original interior backbone.  The GPU value is within
    1e-4 A of the same trip through oracle.nerf + superpose_ref: the NeRF kernel's pinned 1e-4 A parity bounds it,
    RMSD being 1-Lipschitz in the rms displacement.  That value is under 0.1 A (the builder's fixed first N / CA / C
    frame, not an error; it falls with n), while the same columns fed as LABELLED are more than 1 A away."""
    from e3diff_amd import evaluate
    from e3diff_amd.structure_model.create_pdb import backbone_from_angles
    sizes = (3, 32)
    stored, interior, oracle = [], [], {}
    for n in sizes:
        X = onerf.backbone_coords(nerf_angles(n + 2, 900 + n), True).reshape(-1, 4, 3)
        S = fr.chain_angles(X)[1:-1].astype(np.float32)
        stored.append(S)
        interior.append(X[1:-1])
        for name, B in (("stored", evaluate.builder_angles_from_stored(S)), ("labelled", S)):
            oracle[n, name] = np.sqrt(sr.superpose(onerf.backbone_coords(B, True), X[1:-1].reshape(-1, 3))[0])
        print(f"n={n}: oracle round trip {oracle[n, 'stored']:.4f} A, columns as labelled {oracle[n, 'labelled']:.3f} A")
        assert oracle[n, "stored"] < 0.1 and oracle[n, "labelled"] > 1.0   # on the CPU reference first
    L = max(sizes)
    ref = torch.zeros(len(sizes), L, 4, 3, dtype=torch.float64)
    batch = {"stored": torch.zeros(len(sizes), L, 8), "labelled": torch.zeros(len(sizes), L, 8)}
    for i, n in enumerate(sizes):
        ref[i, :n] = torch.from_numpy(interior[i])
        batch["stored"][i, :n] = torch.from_numpy(evaluate.builder_angles_from_stored(stored[i]))
        batch["labelled"][i, :n] = torch.from_numpy(stored[i])
    lengths = torch.tensor(sizes, dtype=torch.int32).cuda()
    for name, angles in batch.items():
        built = backbone_from_angles(angles.cuda(), lengths, center=True)
        rmsd = evaluate.rmsd_to_reference(built, ref.cuda(), lengths, atoms="backbone").cpu().numpy()
        for i, n in enumerate(sizes):
            print(f"n={n} {name}: kernel {rmsd[i]:.6f} A, oracle {oracle[n, name]:.6f} A")
            assert abs(rmsd[i] - oracle[n, name]) <= 1e-4
    # with the transform: placing the built chain leaves exactly that RMSD, and the C-alpha form takes [B,L,3] too
    built = backbone_from_angles(batch["stored"].cuda(), lengths, center=True)
    rmsd, R, t = evaluate.rmsd_to_reference(built, ref.cuda()[:, :, 1], lengths, atoms="CA", transform=True)
    placed = (torch.einsum("bjk,blak->blaj", R, built) + t[:, None, None, :]).cpu().numpy()
    for i, n in enumerate(sizes):
        left = np.sqrt(((placed[i, :n, 1] - interior[i][:, 1]) ** 2).sum(-1).mean())
        assert abs(left - float(rmsd[i])) <= 1e-9 and float(rmsd[i]) < 0.1


# ------------------------------------------------------------------------------- 6. end to end
def test_evaluate_samples_end_to_end(pkg, hip):
    """Three synthetic pockets; replicate 0 = the native angles, replicate 1 = the native angles with one phi moved by
    1 rad.  The references are evaluated on the coordinates the device built (captured through the build hook), so the
    bound of test 1 applies; clashes equal a float64 brute force over the placed coordinates the call returns."""
    from e3diff_amd import biolip, evaluate
    from e3diff_amd.structure_model.create_pdb import backbone_from_angles
    from e3diff_amd.structure_model.dataset import LigandBindingSiteDataset
    cutoff = evaluate.DEFAULT_CLASH_CUTOFF
    ds = LigandBindingSiteDataset(None, None, max_len=64, records=biolip.synthetic_records(
        3, seed=11, receptor_len=(60, 90), ligand_len=(6, 12)))
    native = [d["angle_features"][d["ligand_mask"]].numpy() for d in ds.data]
    moved = [a.copy() for a in native]
    for a in moved:
        a[a.shape[0] // 2, 1] += 1.0                                      # phi of the stored columns
    seen = {}

    def build(angles, lengths):
        seen["coords"] = backbone_from_angles(angles.cuda(), lengths.cuda(), True)
        return seen["coords"]

    rows, placed = evaluate.evaluate_samples([native, moved], ds, return_placed=True, _build=build)
    coords = seen["coords"].cpu().numpy()                                 # per pocket: native, replicate 0, replicate 1
    assert coords.shape[0] == 9 and len(rows) == 3
    total = 0
    for i, row in enumerate(rows):
        d, l = ds.data[i], native[i].shape[0]
        nat, rep = coords[3 * i, :l], [coords[3 * i + 1, :l], coords[3 * i + 2, :l]]
        assert row["structure_ids"] == d["structure_ids"] and row["ligand_length"] == l
        assert row["backbone_rmsd_to_native_built"][0] < 1e-6
        want, _, _, G = sr.superpose(rep[1].reshape(-1, 3), nat.reshape(-1, 3))
        assert abs(row["backbone_rmsd_to_native_built"][1] ** 2 - want) <= sr.msd_bound(G, 4 * l) and want > 0.01
        pair, _, _, G = sr.superpose(rep[0][:, 1], rep[1][:, 1])
        mat = np.array(row["pairwise_ca_rmsd"])
        assert mat.shape == (2, 2) and mat[0, 0] == mat[1, 1] == 0.0 and mat[0, 1] == mat[1, 0]
        assert abs(mat[0, 1] ** 2 - pair) <= sr.msd_bound(G, l)
        assert row["medoid"] == 0 and row["mean_pairwise_ca_rmsd"] == mat[0, 1]
        lig_ca = d["coors"][d["ligand_mask"]].double().numpy()
        rec_ca = d["coors"][~d["ligand_mask"]].double().numpy()
        for r in range(2):
            want, _, _, G = sr.superpose(rep[r][:, 1], lig_ca)
            assert abs(row["ca_rmsd_to_native"][r] ** 2 - want) <= sr.msd_bound(G, l)
            xyz = placed[i][r]
            assert xyz.shape == (4 * l, 3)
            left = np.sqrt(((xyz[1::4] - lig_ca) ** 2).sum(-1).mean())   # placed ON the native C-alphas, not the reverse
            assert abs(left - row["ca_rmsd_to_native"][r]) <= 1e-9
            dist = np.linalg.norm(rec_ca[:, None] - xyz[None], axis=-1).min(1)
            assert np.abs(dist - cutoff).min() > 1e-3                    # float32 distance arithmetic cannot change a verdict
            assert row["clashes"][r] == int((dist <= cutoff).sum())
            total += row["clashes"][r]
    assert total > 0
