"""CPU: scoring of sampled peptides (evaluate.py) -- the export and its argument checks, the stored -> builder column map,
the float64 reference (superpose_ref.py) against known transforms and mirror images, the host-side packing and pair
lists, and the row assembly of ``evaluate_samples`` with every kernel replaced by its numpy statement."""
import os
import re

import numpy as np
import pytest
import torch

import featurize_ref as fr
import superpose_ref as sr
from oracle import nerf as onerf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stored_angles(n, seed):
    rng = np.random.default_rng(seed)
    ang = np.empty((n, 8), dtype=np.float32)
    ang[:, :4] = rng.uniform(-np.pi, np.pi, (n, 4))
    ang[:, 4:] = rng.normal(1.95, 0.1, (n, 4))
    return ang


# ------------------------------------------------------------------------------- 1. the export
def test_superpose_export_and_argument_checks(pkg):
    header = open(os.path.join(ROOT, "include", "e3d_hip.h")).read()
    declared = set(re.findall(r"\b(e3d_[a-z0-9_]+)\s*\(", header))
    lib = pkg.hip.lib()
    assert "e3d_superpose_pairs" in declared and "e3d_superpose_pairs" in pkg.hip.EXPORTS
    assert callable(lib.e3d_superpose_pairs)
    section = header[header.index("rigid superposition of structure pairs"):]
    assert "x' = R x + t" in section and "det R = +1" in section
    assert lib.e3d_abi_version() == 5 == pkg.hip.ABI_VERSION
    # argument validation happens before any launch: callable without a GPU
    d, i = torch.zeros(32, dtype=torch.float64).data_ptr(), torch.zeros(32, dtype=torch.int32).data_ptr()
    good = [d, i, i, i, d, d, d, i]
    for missing in (0, 1, 2, 3, 4, 7):                       # xyz, off, mob, ref, msd, status
        args = list(good)
        args[missing] = None
        assert lib.e3d_superpose_pairs(*args, 1, 1, 1, None) != 0
        assert b"null pointer" in lib.e3d_last_error()
    for rot, trans in ((d, None), (None, d)):                # only one of the two
        assert lib.e3d_superpose_pairs(d, i, i, i, d, rot, trans, i, 1, 1, 1, None) != 0
        assert b"rot and trans" in lib.e3d_last_error()
    for counts in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1)):
        assert lib.e3d_superpose_pairs(*good, *counts, None) != 0
        assert b"need all > 0" in lib.e3d_last_error()
    assert "evaluate" in pkg.__all__


def test_wrappers_refuse_cpu_tensors(pkg):
    from e3diff_amd import evaluate
    z = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate.superpose(torch.zeros(4, 3), torch.tensor([0, 2, 4]), z, z + 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate.rmsd_to_reference(torch.zeros(2, 5, 4, 3), torch.zeros(2, 5, 4, 3), torch.tensor([5, 3]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate.pairwise_rmsd(torch.zeros(2, 5, 3), [5, 5], [[0, 1]])


# ------------------------------------------------------------------------------- 2. column map
@pytest.mark.parametrize("n", [3, 4, 17])
def test_builder_angles_from_stored_inverts_the_column_map(pkg, n):
    """column_map says what the featurizer recovers (stored meaning) from builder input; the map back must give S[1:-1] bit
    for bit, for numpy arrays and torch tensors, single and batched."""
    from e3diff_amd import evaluate
    S = stored_angles(n, 40 + n)
    B = evaluate.builder_angles_from_stored(S)
    assert isinstance(B, np.ndarray) and B.dtype == np.float32 and B.shape == (n, 8)
    assert np.array_equal(fr.column_map(B), S[1:-1].astype(np.float64))
    assert not B[-1, [2, 4, 6]].any()                        # the missing S[n]: zeros
    Bt = evaluate.builder_angles_from_stored(torch.from_numpy(S))
    assert torch.is_tensor(Bt) and Bt.dtype == torch.float32 and np.array_equal(Bt.numpy(), B)
    both = evaluate.builder_angles_from_stored(np.stack([S, S[::-1]]))
    assert np.array_equal(both[0], B) and np.array_equal(both[1], evaluate.builder_angles_from_stored(S[::-1].copy()))


# ------------------------------------------------------------------------------- 3. the reference
def horn_msd(a, b):
    """An independent float64 evaluation over PROPER rotations: the largest eigenvalue of Horn's 4x4 matrix."""
    ac, bc = a - a.mean(0), b - b.mean(0)
    S = ac.T @ bc
    (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = S
    N = np.array([[xx + yy + zz, yz - zy, zx - xz, xy - yx], [yz - zy, xx - yy - zz, xy + yx, zx + xz],
                  [zx - xz, xy + yx, -xx + yy - zz, yz + zy], [xy - yx, zx + xz, yz + zy, -xx - yy + zz]])
    G = (ac * ac).sum() + (bc * bc).sum()
    return max(0.0, (G - 2.0 * np.linalg.eigvalsh(N)[-1]) / len(a)), G


def test_reference_recovers_a_known_transform():
    rng = np.random.default_rng(1)
    for n in (3, 4, 17, 64, 129):
        a = sr.random_walk(rng, n)
        R, t = sr.random_rotation(rng), rng.normal(size=3) * 30.0
        assert abs(np.linalg.det(R) - 1.0) < 1e-12
        msd, Rg, tg, G = sr.superpose(a, a @ R.T + t)
        assert msd <= sr.msd_bound(G, n)
        assert np.abs(Rg - R).max() < 1e-9 and np.abs(tg - t).max() < 1e-7
        assert sr.msd_of(a, a @ R.T + t, Rg, tg) <= sr.msd_bound(G, n)
        # the direction: R, t map the FIRST argument onto the second
        assert sr.msd_of(a @ R.T + t, a, Rg, tg) > 1.0


def test_reference_does_not_superpose_a_mirror_image_by_a_reflection():
    rng = np.random.default_rng(2)
    for n in (8, 32, 129):
        a, b = sr.pair_of_kind(rng, n, "mirrored")
        proper, R, t, G = sr.superpose(a, b)
        improper, Ri, _, _ = sr.superpose(a, b, proper=False)
        want, _ = horn_msd(a, b)
        print(f"n={n}: rmsd proper {np.sqrt(proper):.3f}, with reflections {np.sqrt(improper):.2e}")
        assert abs(proper - want) <= sr.msd_bound(G, n)              # the det-corrected value
        assert np.linalg.det(R) > 0 and np.linalg.det(Ri) < 0
        assert improper <= sr.msd_bound(G, n) and np.sqrt(proper) > 0.5 and improper < proper
        assert abs(sr.msd_of(a, b, R, t) - proper) <= sr.msd_bound(G, n)


def test_reference_pair_list_statuses():
    rng = np.random.default_rng(3)
    xyz = rng.normal(size=(10, 3))
    xyz[9, 1] = np.nan
    off = [0, 3, 6, 6, 8, 10]                                            # lengths 3, 3, 0, 2, 2 (the last holds a NaN)
    msd, R, t, st, G = sr.superpose_pairs(xyz, off, [0, 0, 2, -1, 0, 3, 1], [1, 3, 2, 0, 5, 4, 0])
    assert st.tolist() == [0, 1, 2, 3, 3, 4, 0]
    assert np.isfinite(msd[[0, 6]]).all() and np.isnan(msd[1:6]).all() and np.isnan(R[1:6]).all() and np.isnan(t[1:6]).all()
    assert abs(msd[0] - msd[6]) < 1e-12


# ------------------------------------------------------------------------------- 4. packing, pair lists, medoid
def test_padded_to_flat_packing(pkg):
    from e3diff_amd import evaluate
    x = torch.arange(3 * 5 * 4 * 3, dtype=torch.float64).reshape(3, 5, 4, 3)
    ca = evaluate.select_atoms(x, "CA")
    assert tuple(ca.shape) == (3, 5, 1, 3) and torch.equal(ca[:, :, 0], x[:, :, 1])
    assert evaluate.select_atoms(x, "backbone") is x
    assert torch.equal(evaluate.select_atoms(x[:, :, 1], "CA")[:, :, 0], x[:, :, 1])
    with pytest.raises(ValueError):
        evaluate.select_atoms(x[:, :, 1], "backbone")
    with pytest.raises(ValueError):
        evaluate.select_atoms(x, "heavy")
    flat, off = evaluate.flatten_by_lengths(ca, [5, 0, 2])
    assert off.dtype == torch.int32 and off.tolist() == [0, 5, 5, 7]
    assert torch.equal(flat, torch.cat([x[0, :5, 1], x[2, :2, 1]]))
    flat, off = evaluate.flatten_by_lengths(x, torch.tensor([1, 3, 2]))
    assert off.tolist() == [0, 4, 16, 24]
    assert torch.equal(flat, torch.cat([x[0, :1].reshape(-1, 3), x[1, :3].reshape(-1, 3), x[2, :2].reshape(-1, 3)]))
    with pytest.raises(ValueError):
        evaluate.flatten_by_lengths(x, [1, 6, 2])


def test_pairs_within_groups_and_medoid(pkg):
    from e3diff_amd import evaluate
    lengths = [7, 7, 7, 7, 7, 9, 9, 4]
    groups = [[7], [5, 6], [0, 1, 2, 3, 4]]
    mob, ref, bounds = evaluate.group_pairs(groups, lengths)
    assert mob.dtype == np.int32 and bounds == [0, 0, 1, 11]             # R (R - 1) / 2 = 0, 1, 10
    assert list(zip(mob.tolist(), ref.tolist()))[:3] == [(5, 6), (0, 1), (0, 2)]
    group_of = {m: g for g, members in enumerate(groups) for m in members}
    assert all(group_of[a] == group_of[b] and a < b for a, b in zip(mob.tolist(), ref.tolist()))
    assert len(set(zip(mob.tolist(), ref.tolist()))) == 11
    with pytest.raises(ValueError, match="mixes"):
        evaluate.group_pairs([[0, 1], [4, 5]], lengths)
    with pytest.raises(ValueError, match="mixes"):                       # on the host, before any launch: CPU tensors
        evaluate.pairwise_rmsd(torch.zeros(8, 9, 3), lengths, [[0, 5]])
    # medoid: smallest mean to the others, the lowest index on ties
    m = torch.tensor([[0.0, 1.0, 2.0], [1.0, 0.0, 1.0], [2.0, 1.0, 0.0]], dtype=torch.float64)
    assert evaluate.medoid(m) == 1
    assert evaluate.medoid(torch.tensor([[0.0, 3.0], [3.0, 0.0]])) == 0
    tie = torch.tensor([[0, 2, 1, 1], [2, 0, 1, 1], [1, 1, 0, 2], [1, 1, 2, 0]], dtype=torch.float64)
    assert evaluate.medoid(tie) == 0 and evaluate.medoid(tie[[3, 2, 1, 0]][:, [3, 2, 1, 0]]) == 0
    assert evaluate.medoid(torch.zeros(1, 1)) == 0
    assert evaluate.neighbour_counts(m, 1.0).tolist() == [1, 2, 1]
    # matrices from an injected superposition: symmetric, zero diagonal, [[0]] for one structure
    rng = np.random.default_rng(4)
    coords = torch.from_numpy(rng.normal(size=(8, 9, 3)) * 5)
    mats = evaluate.pairwise_rmsd(coords, lengths, groups, _superpose=sr.torch_superpose)
    assert [tuple(x.shape) for x in mats] == [(1, 1), (2, 2), (5, 5)] and mats[0].tolist() == [[0.0]]
    for g, mat in zip(groups, mats):
        want = sr.pairwise_rmsd([coords[i, :lengths[i]].numpy() for i in g])
        assert torch.equal(mat, mat.T) and not mat.diagonal().any() and np.allclose(mat.numpy(), want, rtol=0, atol=1e-12)
        assert evaluate.medoid(mat) == sr.medoid(want)


# ------------------------------------------------------------------------------- 5. row assembly
def numpy_build(angles, lengths):
    """The NeRF builder's contract through the oracle: [B,L,8] + lengths -> centred float64 [B,L,4,3], zero padding."""
    out = torch.zeros(angles.shape[0], angles.shape[1], 4, 3, dtype=torch.float64)
    for b, n in enumerate(lengths.tolist()):
        out[b, :n] = torch.from_numpy(onerf.backbone_coords(angles[b, :n].numpy(), True).reshape(n, 4, 3))
    return out


def numpy_contacts(rec_xyz, rec_row, rec_off, lig_xyz, lig_off, n_rows, cutoff):
    hit = np.zeros(n_rows, dtype=np.int32)
    for c in range(len(rec_off) - 1):
        r, l = rec_xyz[rec_off[c]:rec_off[c + 1]].numpy(), lig_xyz[lig_off[c]:lig_off[c + 1]].numpy()
        near = np.linalg.norm(r[:, None] - l[None], axis=-1).min(1) <= cutoff
        np.maximum.at(hit, rec_row[rec_off[c]:rec_off[c + 1]].numpy(), near.astype(np.int32))
    return torch.from_numpy(hit)


@pytest.mark.parametrize("convention", ["stored", "labelled"])
def test_evaluate_samples_row_assembly(pkg, convention):
    from e3diff_amd import biolip, evaluate
    from e3diff_amd.structure_model.dataset import LigandBindingSiteDataset, NoisedAnglesDataset
    records = biolip.synthetic_records(3, seed=5, receptor_len=(20, 30), ligand_len=(5, 9))
    ds = LigandBindingSiteDataset(None, None, max_len=64, records=records)
    data = ds.data                                                       # shuffled: item i is data[i], not records[i]
    native = [d["angle_features"][d["ligand_mask"]].numpy() for d in data]
    rng = np.random.default_rng(6)
    noisy = [a + rng.normal(size=a.shape).astype(np.float32) * 0.2 for a in native]
    traj = [np.stack([rng.normal(size=a.shape).astype(np.float32), a]) for a in noisy]      # [T,l,8]: the last step counts
    hooks = dict(device="cpu", _superpose=sr.torch_superpose, _build=numpy_build, _contacts=numpy_contacts)
    rows, placed = evaluate.evaluate_samples([native, traj], NoisedAnglesDataset(ds, timesteps=10), convention,
                                             clash_cutoff=6.0, return_placed=True, **hooks)
    assert evaluate.evaluate_samples([native, noisy], ds, convention, clash_cutoff=6.0, **hooks) == rows   # a bare dataset
    assert [r["index"] for r in rows] == [0, 1, 2]
    to_builder = evaluate.builder_angles_from_stored if convention == "stored" else (lambda a: a)
    for i, row in enumerate(rows):
        d = data[i]
        l = native[i].shape[0]
        assert row["structure_ids"] == d["structure_ids"] and row["ligand_length"] == l
        built = [onerf.backbone_coords(to_builder(a), True) for a in (native[i], native[i], noisy[i])]
        lig_ca, rec_ca = d["coors"][d["ligand_mask"]].double().numpy(), d["coors"][~d["ligand_mask"]].double().numpy()
        assert row["backbone_rmsd_to_native_built"][0] < 1e-6
        assert row["backbone_rmsd_to_native_built"][1] == pytest.approx(np.sqrt(sr.superpose(built[2], built[0])[0]), abs=1e-9)
        assert row["backbone_rmsd_to_native_built"][1] > 0.05
        pair = sr.pairwise_rmsd([built[1][1::4], built[2][1::4]])
        assert np.allclose(row["pairwise_ca_rmsd"], pair, rtol=0, atol=1e-9) and row["medoid"] == 0
        assert row["mean_pairwise_ca_rmsd"] == pytest.approx(pair[0, 1], abs=1e-9)
        for r in range(2):
            msd, R, t, _ = sr.superpose(built[1 + r][1::4], lig_ca)
            assert row["ca_rmsd_to_native"][r] == pytest.approx(np.sqrt(msd), abs=1e-9)
            want = built[1 + r] @ R.T + t                                 # the whole backbone, by the C-alpha transform
            assert placed[i][r].shape == (4 * l, 3) and np.abs(placed[i][r] - want).max() < 1e-9
            dist = np.linalg.norm(rec_ca[:, None] - want[None], axis=-1).min(1)
            assert np.abs(dist - 6.0).min() > 1e-6
            assert row["clashes"][r] == int((dist <= 6.0).sum())
    assert sum(sum(r["clashes"]) for r in rows) > 0
    single = evaluate.evaluate_samples([native], ds, convention, **hooks)
    assert single[0]["pairwise_ca_rmsd"] == [[0.0]] and single[0]["mean_pairwise_ca_rmsd"] is None and single[0]["medoid"] == 0
    with pytest.raises(ValueError, match="replicate 0"):
        evaluate.evaluate_samples([[a[:-1] for a in native]], ds, convention, **hooks)
    with pytest.raises(ValueError, match="convention"):
        evaluate.evaluate_samples([native], ds, "builder", **hooks)
    assert "not docking" in evaluate.evaluate_samples.__doc__


# ------------------------------------------------------------------------------- 6. the tool
def test_evaluate_tool_arguments_and_summary():
    import importlib.util
    spec = importlib.util.spec_from_file_location("evaluate_samples_tool", os.path.join(ROOT, "tools", "evaluate_samples.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = tool.parse_args(["a.pkl", "b.pkl", "--data", "biolip.pt", "--pdb-dir", "out", "-o", "report.json"])
    assert args.samples == ["a.pkl", "b.pkl"] and args.convention == "stored" and args.clash_cutoff == 3.0
    assert tool.parse_args(["a.pkl", "--data", "x.pt", "--convention", "labelled", "-o", "r.json"]).convention == "labelled"
    rows = [{"ca_rmsd_to_native": [1.0, 3.0], "clashes": [0, 2]}, {"ca_rmsd_to_native": [5.0, 4.0], "clashes": [1, 1]}]
    assert tool.summarize(rows) == {"pockets": 2, "replicates": 2, "median_ca_rmsd": 3.5, "median_best_of_r_ca_rmsd": 2.5,
                                    "share_under_2A": 0.25, "share_best_of_r_under_2A": 0.5, "mean_clashes": 1.0}
