"""``nerf_backbone_kernel`` (csrc/nerf.hip) at every launch edge, and the host functions above it, against the float64 side
in tests/nerf_ref.py: the second and the partly filled workgroup, lengths 0, 1, negative, L and beyond, NaN in the rows that
must not be read, a NaN sentinel in the output the kernel has to overwrite, workload lengths, non-finite angles.

Every atom is held to ``chain_allowance`` (measured on the reference: the oracle with its float32 values moved by the
documented ulp bound of sinf / cosf, tests/test_nerf_ref_cpu.py shows it rejects eight wrong builders by >= 100x), every chain's
bond lengths, bond angles and torsions to ``internal_bound`` (derived), chains of up to 64 residues to the project's older
1e-4 A as well.  Worst observed ratios on one MI355X (printed by the tests, recorded in DESIGN.md section 7):
see ``OBSERVED`` below."""
import os
import pickle

import numpy as np
import pytest
import torch

import nerf_ref as R

OBSERVED = """
    worst |got - ref| / chain_allowance by chain length (uncentred / centred), and the largest |got - ref|:
        1: 0.032 / 0.032 (1.4e-8 A)     2: 0.000 / 0.000 (bit-equal uncentred)     3: 0.238 / 0.185 (2.5e-7 A)
        32: 0.149 / 0.198 (2.1e-6 A)    33: 0.252 / 0.206 (4.0e-6 A)
        255 random: 0.267 / 0.161 (1.3e-5 A)     256 random: 0.258 / 0.110 (4.2e-5 A)
        256 helix:  0.237 / 0.040 (1.5e-5 A)     256 extended: 0.259 / 0.017 (4.5e-5 A)
    worst internal error / internal_bound: 0.345 (random chain of 255); 0.301 in the main launch
    worst |mean| or |centred - (uncentred - mean)| over mean_floor: 0.117
"""
NAN = float("nan")


def launch(pkg, hip, angles, lengths, center):
    """The C entry point itself on an output pre-filled with NaN: whatever is not NaN afterwards, the kernel wrote."""
    B, L, _ = angles.shape
    ang = torch.from_numpy(np.ascontiguousarray(angles, dtype=np.float32)).cuda()
    lens = torch.tensor(list(lengths), dtype=torch.int32).cuda()
    out = torch.full((B, L, 4, 3), NAN, dtype=torch.float64, device="cuda")
    pkg.hip.check(hip.e3d_nerf_backbone(ang.data_ptr(), lens.data_ptr(), out.data_ptr(), int(center), B, L,
                                        torch.cuda.current_stream().cuda_stream), "e3d_nerf_backbone")
    return out.cpu().numpy()


def padded(chains, L):
    """[B,L,8] with NaN in every row at or beyond a chain's length: the kernel must not read them."""
    batch = np.full((len(chains), L, 8), np.nan, dtype=np.float32)
    for b, a in enumerate(chains):
        batch[b, :len(a)] = a
    return batch


def check_chain(got, ang, center, what, flat_1e4):
    """One chain's [n,4,3] against the oracle: allowance, 1e-4 A where it held before, internal coordinates.  -> ratios"""
    n = len(ang)
    ref = R.batch_reference(ang[None], [n], center)[0]
    assert np.isfinite(got).all(), what
    ratio = R.allowance_ratio(got, ref, ang, center)
    local = R.internal_ratio(got, ang)
    err = float(np.abs(got - ref).max())
    assert ratio <= 1.0, (what, ratio, err)
    assert max(local.values()) <= 1.0, (what, local)
    if flat_1e4:
        assert err < 1e-4, (what, err)
    return ratio, max(local.values()), err


# ------------------------------------------------------------------------------------------------ main launch
B_MAIN, L_MAIN = 300, 33
CYCLE = (0, 1, 2, 3, 32, 33, -4, 40)
COPIES = (0, 255, 256, 299)


@pytest.fixture(scope="module")
def main(pkg, hip):
    """B = 300, L = 33: a full workgroup, a second one of 44 threads, both clamp directions.  Items cycle through CYCLE with
    two different chains per length; the same 33-residue chain sits at the first item, astride the workgroup boundary and at
    the last item."""
    copy = R.random_chain(33, 9000)
    lengths, chains = [], []
    for b in range(B_MAIN):
        slot, variant = b % len(CYCLE), (b // len(CYCLE)) % 2
        n = min(max(CYCLE[slot], 0), L_MAIN)
        lengths.append(CYCLE[slot])
        chains.append(R.random_chain(n, 100 + 2 * slot + variant))
    for b in COPIES:
        lengths[b], chains[b] = 33, copy
    angles = padded(chains, L_MAIN)
    out = {c: launch(pkg, hip, angles, lengths, c) for c in (False, True)}
    alone = {c: launch(pkg, hip, copy[None], [33], c) for c in (False, True)}
    wide = {c: launch(pkg, hip, padded([copy], 64), [33], c) for c in (False, True)}
    return dict(lengths=lengths, chains=chains, out=out, alone=alone, wide=wide)


@pytest.mark.gpu
@pytest.mark.parametrize("center", (False, True))
def test_main_launch_every_item_against_the_reference(main, center):
    out = main["out"][center]
    assert not np.isnan(out).any()                                    # the sentinel is gone everywhere, no NaN was read
    seen, worst = set(), {}
    for b, (length, ang) in enumerate(zip(main["lengths"], main["chains"])):
        n = len(ang)
        assert n == min(max(length, 0), L_MAIN)
        assert not out[b, n:].any() and not np.signbit(out[b, n:]).any(), f"item {b}: padding is not +0.0"
        if n:
            r = check_chain(out[b, :n], ang, center, f"item {b} length {length} center {center}", True)
            worst[n] = tuple(max(x, y) for x, y in zip(worst.get(n, (0.0, 0.0, 0.0)), r))
        seen.add((length, b >= 256))
    assert seen >= {(length, second) for length in CYCLE for second in (False, True)}     # every length in both workgroups
    for n, (ratio, local, err) in sorted(worst.items()):
        print(f"[nerf] main launch center={center} n={n}: worst error / allowance {ratio:.3f}, internal / bound {local:.3f}, "
              f"max |got - ref| {err:.2e} A")


@pytest.mark.gpu
@pytest.mark.parametrize("center", (False, True))
def test_copies_are_bit_identical_wherever_they_sit(main, center):
    """Item 0, the last thread of workgroup 0, the first of workgroup 1, the last item, a launch of its own, and a launch of
    its own in a wider frame: one chain, one result."""
    out = main["out"][center]
    first = out[0].tobytes()
    for b in COPIES[1:]:
        assert out[b].tobytes() == first, b
    assert main["alone"][center][0].tobytes() == first
    wide = main["wide"][center][0]
    assert wide[:33].tobytes() == first and not wide[33:].any()


@pytest.mark.gpu
def test_centring_is_the_mean_over_all_atoms_of_the_chain(main):
    """The centred chain's atom mean is zero, and centred = uncentred - float64 mean(uncentred), both within ``mean_floor``."""
    worst = 0.0
    for b, ang in enumerate(main["chains"]):
        n = len(ang)
        if not n:
            continue
        raw, cen = main["out"][False][b, :n].reshape(-1, 3), main["out"][True][b, :n].reshape(-1, 3)
        floor = R.mean_floor(4 * n, float(np.abs(raw).max()))
        a, d = np.abs(cen.mean(axis=0)).max(), np.abs(cen - (raw - raw.mean(axis=0))).max()
        worst = max(worst, a / floor, d / floor)
        assert a <= floor and d <= floor, (b, n, a, d, floor)
    print(f"[nerf] centring: worst |mean| or |centred - (uncentred - mean)| over mean_floor: {worst:.3f}")


# ------------------------------------------------------------------------------------------------ workload lengths
def workload_chains():
    return {"random 256": R.random_chain(256, 256), "helix 256": R.regular_chain(R.HELIX, 256),
            "extended 256": R.regular_chain(R.EXTENDED, 256), "random 255": R.random_chain(255, 255)}


@pytest.fixture(scope="module")
def workload(pkg, hip):
    chains = list(workload_chains().values())
    angles = padded(chains, 256)
    return {c: launch(pkg, hip, angles, [len(a) for a in chains], c) for c in (False, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(4), ids=lambda i: list(workload_chains())[i].replace(" ", "_"))
def test_workload_lengths(workload, which):
    """B = 4, L = 256: the project's frame.  The extended chain carries the largest uncentred coordinates and centring sums."""
    name, ang = list(workload_chains().items())[which]
    n = len(ang)
    for center in (False, True):
        out = workload[center]
        assert not np.isnan(out).any() and not out[which, n:].any()
        ratio, local, err = check_chain(out[which, :n], ang, center, f"{name} center {center}", False)
        print(f"[nerf] workload {name} center={center}: error / allowance {ratio:.3f}, internal / bound {local:.3f}, "
              f"max |got - ref| {err:.2e} A")
    raw, cen = workload[False][which, :n].reshape(-1, 3), workload[True][which, :n].reshape(-1, 3)
    floor = R.mean_floor(4 * n, float(np.abs(raw).max()))
    assert np.abs(cen.mean(axis=0)).max() <= floor and np.abs(cen - (raw - raw.mean(axis=0))).max() <= floor


@pytest.mark.gpu
@pytest.mark.parametrize("B", (256, 257))
def test_exact_workgroup_boundary(pkg, hip, B):
    """B = 256 fills one workgroup exactly; B = 257 puts a single thread into a second one."""
    pool = [R.random_chain(2, 300 + k) for k in range(3)] + [R.random_chain(1, 303)]
    chains = [pool[(b * 7 + b // 4) % 4] for b in range(B)]
    angles = padded(chains, 2)
    for center in (False, True):
        out = launch(pkg, hip, angles, [len(a) for a in chains], center)
        assert not np.isnan(out).any()
        for b, ang in enumerate(chains):
            check_chain(out[b, :len(ang)], ang, center, f"B {B} item {b}", True)
            assert not out[b, len(ang):].any()


# ------------------------------------------------------------------------------------------------ non-finite angles
def first_use(col, residue):
    """(residue, atom) of the placement that reads angle column ``col`` of ``residue`` (nerf_ref.PLACEMENTS)."""
    for k, (_, acol, aoff, tcol, toff) in enumerate(R.PLACEMENTS):
        if acol == col:
            return residue - aoff, k
        if tcol == col:
            return residue - toff, k
    raise AssertionError(col)


@pytest.mark.gpu
@pytest.mark.parametrize("nan_col,inf_col", ((1, 2), (0, 4), (3, 7), (5, 0), (6, 3)))
def test_non_finite_angles_stay_in_their_item_and_after_their_first_use(pkg, hip, nan_col, inf_col):
    """B = 6, L = 16; NaN in one angle of residue 5 of item 1, +-inf in one of item 3.  Uncentred: the atoms placed before the
    angle's first use keep the bits of the clean launch, every atom from it on is NaN (an angle of the O placement: that O
    alone).  Centred: the whole item is NaN, its mean is.  The padding stays zero and the other items keep their bits."""
    lens = (16, 16, 9, 12, 1, 16)
    chains = [R.random_chain(n, 500 + b) for b, n in enumerate(lens)]
    clean = padded(chains, 16)
    bad = clean.copy()
    bad[1, 5, nan_col] = np.nan
    bad[3, 5, inf_col] = np.inf if inf_col % 2 else -np.inf
    assert first_use(1, 5) == (6, 0) and first_use(0, 5) == (5, 2) and first_use(3, 5) == (5, 3) and first_use(4, 5) == (6, 2)
    for center in (False, True):
        want, got = launch(pkg, hip, clean, lens, center), launch(pkg, hip, bad, lens, center)
        assert not np.isnan(want).any()
        for b in (0, 2, 4, 5):
            assert got[b].tobytes() == want[b].tobytes(), b
        for b, col in ((1, nan_col), (3, inf_col)):
            n = lens[b]
            res, k = first_use(col, 5)
            flat_got, flat_want = got[b, :n].reshape(-1, 3), want[b, :n].reshape(-1, 3)
            hit = np.zeros(4 * n, dtype=bool)
            if center:
                hit[:] = True
            elif k == 3:
                hit[4 * res + 3] = True
            else:
                hit[4 * res + k:] = True
            assert np.isnan(flat_got[hit]).all(), (b, col, center)
            assert flat_got[~hit].tobytes() == flat_want[~hit].tobytes(), (b, col, center)
            assert not got[b, n:].any()


# ------------------------------------------------------------------------------------------------ host functions
@pytest.mark.gpu
def test_backbone_from_angles_input_forms(pkg, hip):
    from e3diff_amd.structure_model.create_pdb import backbone_from_angles
    chains = [R.random_chain(n, 600 + n) for n in (7, 12, 1)]
    batch = np.zeros((3, 12, 8), dtype=np.float32)
    for b, a in enumerate(chains):
        batch[b, :len(a)] = a
    ang, lens = torch.from_numpy(batch).cuda(), torch.tensor([7, 12, 1], dtype=torch.int32).cuda()
    for center in (True, False):
        plain = backbone_from_angles(ang, lens, center)
        assert plain.dtype == torch.float64 and plain.shape == (3, 12, 4, 3)
        for b, a in enumerate(chains):
            check_chain(plain[b, :len(a)].cpu().numpy(), a, center, f"wrapper item {b}", True)
            assert not plain[b, len(a):].any()
        strided = ang.transpose(0, 1).contiguous().transpose(0, 1)[:, :, ::1]
        assert not strided.is_contiguous()
        for other in (backbone_from_angles(ang.double(), lens, center), backbone_from_angles(strided, lens, center),
                      backbone_from_angles(ang, lens.long(), center), backbone_from_angles(ang, lens.cpu(), center)):
            assert torch.equal(other, plain)
    with pytest.raises(RuntimeError, match="HIP kernel only"):
        backbone_from_angles(ang.cpu(), lens.cpu())
    with pytest.raises(AssertionError):
        backbone_from_angles(ang[:, :, :7], lens)


class Frame:
    """What ``_as_angle_array`` needs of a DataFrame: ``columns`` and ``frame[name]``."""

    def __init__(self, columns):
        self._data = dict(columns)
        self.columns = list(self._data)

    def __getitem__(self, name):
        return self._data[name]


@pytest.mark.gpu
def test_coords_for_chains_pads_trims_and_reads_columns_by_name(pkg, hip):
    from e3diff_amd.structure_model.create_pdb import COLS, backbone_from_angles, coords_for_chains
    chains = [R.random_chain(n, 700 + n) for n in (1, 33, 7, 64)]
    for center in (True, False):
        got = coords_for_chains(chains, center, device="cuda:0")
        for a, g in zip(chains, got):
            n = len(a)
            one = backbone_from_angles(torch.from_numpy(a[None]).cuda(), torch.tensor([n]).cuda(), center)
            assert g.shape == (4 * n, 3) and g.dtype == np.float64
            assert g.tobytes() == one[0].reshape(-1, 3).cpu().numpy().tobytes()
    order = [5, 0, 7, 2, 4, 1, 6, 3]
    frames = [Frame((COLS[j], a[:, j].astype(np.float64)) for j in order) for a in chains]
    for g, f in zip(got, coords_for_chains(frames, False, device="cuda:0")):
        assert g.tobytes() == f.tobytes()
    with pytest.raises(ValueError, match="Unrecognized angle: bogus"):
        coords_for_chains([Frame([(c, chains[2][:, j]) for j, c in enumerate(COLS)] + [("bogus", chains[2][:, 0])])],
                          device="cuda:0")
    with pytest.raises(AssertionError, match="missing dihedral columns"):
        coords_for_chains([Frame((c, chains[2][:, j]) for j, c in enumerate(COLS) if c != "omega")], device="cuda:0")


def parse_atoms(path):
    return np.array([[float(ln[30:38]), float(ln[38:46]), float(ln[46:54])] for ln in open(path) if ln.startswith("ATOM")])


@pytest.mark.gpu
def test_pdb_writers_skip_chains_with_non_finite_angles(pkg, hip, tmp_path):
    from e3diff_amd.structure_model.create_pdb import coords_for_chains, create_new_chain_nerf, write_preds_pdb_folder
    good, other = R.random_chain(12, 801), R.random_chain(5, 802)
    bad = R.random_chain(9, 803)
    bad[4, 2] = np.nan
    assert create_new_chain_nerf(str(tmp_path / "bad.pdb"), bad) == "" and not os.path.exists(tmp_path / "bad.pdb")
    path = create_new_chain_nerf(str(tmp_path / "good.pdb"), good)
    assert path == str(tmp_path / "good.pdb")
    assert np.abs(parse_atoms(path) - coords_for_chains([good])[0]).max() <= 5.0001e-4
    files = write_preds_pdb_folder([good, bad, other], str(tmp_path / "out"))
    assert files[1] == "" and files[0].endswith("generated_0.pdb") and files[2].endswith("generated_2.pdb")
    assert sorted(os.listdir(tmp_path / "out")) == ["generated_0.pdb", "generated_2.pdb"]
    assert np.abs(parse_atoms(files[2]) - coords_for_chains([other])[0]).max() <= 5.0001e-4


def test_load_sampled_angles_takes_trajectories_and_single_steps(pkg, tmp_path):
    from e3diff_amd.structure_model.create_pdb import load_sampled_angles
    a, b = R.random_chain(6, 901), R.random_chain(4, 902)
    traj = np.stack([a * 0.5, a * 0.25, a])
    with open(tmp_path / "output.pkl", "wb") as f:
        pickle.dump([traj, b.astype(np.float64)], f)
    last = load_sampled_angles(str(tmp_path / "output.pkl"))
    assert [x.shape for x in last] == [(6, 8), (4, 8)] and all(x.dtype == np.float32 for x in last)
    assert np.array_equal(last[0], a) and np.array_equal(last[1], b)
    every = load_sampled_angles(str(tmp_path / "output.pkl"), last_step_only=False)
    assert every[0].shape == (3, 6, 8) and np.array_equal(every[0], traj) and np.array_equal(every[1], b)
