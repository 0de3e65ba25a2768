"""The reference side of the NeRF builder's tests can be trusted (tests/nerf_ref.py), before any kernel is judged by it:
``batch_reference`` against the reference's own fixture, ``internal_bound`` as a property of the oracle, ``chain_allowance``
neither vacuous (eight wrong builders are rejected by a factor of 100 or more) nor slack (below the present 1e-4 A at 64
residues of the fixture's distribution); and the fixed columns of ``pdb_text``.  No GPU."""
import os

import numpy as np
import pytest
import torch

import nerf_ref as R
from helpers import GOLDEN
from oracle import nerf as onerf

LENGTHS = (1, 2, 3, 64, 256)


def chains(n):
    return {"random": R.random_chain(n, n), "helix": R.regular_chain(R.HELIX, n), "strand": R.regular_chain(R.STRAND, n),
            "extended": R.regular_chain(R.EXTENDED, n)}


def test_batch_reference_reproduces_the_fixture_exactly():
    """Every case of nerf.pt, alone and in one padded batch whose padding rows are NaN (they must not be read), with the
    clamps: a length beyond L is L, a negative one is 0, and an item of length 0 is all zeros."""
    cases = torch.load(os.path.join(GOLDEN, "nerf.pt"), weights_only=False)["cases"]
    for center in (True, False):
        sel = [c for c in cases if c["center"] == center]
        L = max(c["angles"].shape[0] for c in sel)
        batch = np.full((len(sel) + 2, L, 8), np.nan, dtype=np.float32)
        lens = []
        for i, c in enumerate(sel):
            n = c["angles"].shape[0]
            batch[i, :n] = c["angles"].numpy()
            lens.append(n if n < L else L + 7)
            one = R.batch_reference(c["angles"].numpy()[None], [n], center)
            assert np.array_equal(one[0].reshape(-1, 3), c["coords"].numpy())
        got = R.batch_reference(batch, lens + [0, -3], center)
        assert got.dtype == np.float64 and got.shape == (len(sel) + 2, L, 4, 3) and not np.isnan(got).any()
        for i, c in enumerate(sel):
            n = c["angles"].shape[0]
            assert np.array_equal(got[i, :n].reshape(-1, 3), c["coords"].numpy())
            assert not got[i, n:].any()
        assert not got[-2:].any()


@pytest.mark.parametrize("n", LENGTHS)
def test_internal_bound_holds_for_the_oracle(n):
    """The oracle's coordinates give back their input angles and 1.34, 1.46, 1.54, 1.22 within ``internal_bound``: numpy's
    float32 trigonometry is under the same bound the device's is held to.  Also: every entry the layout defines is checked."""
    worst = {}
    for name, ang in chains(n).items():
        want = R.expected_internal(ang)
        assert np.isfinite(want["length"]).sum() == 4 * n - 3 and np.isnan(want["dihedral"][0, :3]).all()
        for center in (True, False):
            xyz = onerf.backbone_coords(ang, center)
            ratio = R.internal_ratio(xyz, ang)
            worst[name] = max(worst.get(name, 0.0), *ratio.values())
            assert max(ratio.values()) <= 1.0, (name, center, ratio)
    print(f"[nerf_ref] n={n}: worst internal error / internal_bound of the oracle: "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_internal_coordinates_see_one_float32_ulp_times_a_few():
    """The bound is not slack: the oracle's output with one atom moved by 4e-6 A (ten times the length bound) is rejected."""
    ang = R.random_chain(9, 1)
    xyz = onerf.backbone_coords(ang, False).reshape(-1, 4, 3)
    assert max(R.internal_ratio(xyz, ang).values()) <= 1.0
    xyz[4, 1] += np.array([4e-6, 0.0, 0.0])
    assert max(R.internal_ratio(xyz, ang).values()) > 1.0


# ------------------------------------------------------------------------------------------------ mutants
def _swap(a, i, j):
    b = a.copy()
    b[:, [i, j]] = a[:, [j, i]]
    return b


def _from_next(a, cols):
    b = a.copy()
    b[:-1, cols] = a[1:, cols]
    return b


def _negated(a, col):
    b = a.copy()
    b[:, col] = -a[:, col]
    return b


def _swapped_lengths(a, center):
    keep = onerf.N_CA_LENGTH, onerf.CA_C_LENGTH
    try:
        onerf.N_CA_LENGTH, onerf.CA_C_LENGTH = keep[1], keep[0]
        return onerf.backbone_coords(a, center)
    finally:
        onerf.N_CA_LENGTH, onerf.CA_C_LENGTH = keep


def _centred_on_ca(a, center):
    xyz = onerf.backbone_coords(a, False)
    return xyz - xyz[1::4].mean(axis=0)


def _centred_by_padded_length(a, center):
    xyz = onerf.backbone_coords(a, False)
    return xyz - xyz.sum(axis=0) / (len(xyz) + 4)          # the mean over L = len + 1 residues, the closest wrong L


# name: (builder(angles, center) -> [4n,3], centred only, changes the internal coordinates)
MUTANTS = {
    "psi and phi swapped": (lambda a, c: onerf.backbone_coords(_swap(a, 0, 1), c), False, True),
    "omega of residue i, not i-1": (lambda a, c: onerf.backbone_coords(_from_next(a, [2]), c), False, True),
    "bond angles of residue i, not i-1": (lambda a, c: onerf.backbone_coords(_from_next(a, [4, 5, 6]), c), False, True),
    "1.46 and 1.54 swapped": (_swapped_lengths, False, True),
    "CA:C:O and CA:C:1N swapped": (lambda a, c: onerf.backbone_coords(_swap(a, 7, 5), c), False, True),
    "dihedral_o negated": (lambda a, c: onerf.backbone_coords(_negated(a, 3), c), False, True),
    "centred on the CA atoms": (_centred_on_ca, True, False),
    "centred by the mean over L, not len": (_centred_by_padded_length, True, False),
}


@pytest.mark.parametrize("n", (3, 64, 256))
def test_allowance_rejects_every_mutant_by_a_factor_of_100(n):
    """Eight wrong builders on a random chain (on a regular chain the two "residue i" mutants are no change at all): each
    exceeds ``chain_allowance`` by >= 100x, centred and uncentred.  Every mutant that changes a length, an angle or a torsion
    also exceeds ``internal_bound`` by >= 100x.  The two "residue i" mutants keep every length and the multiset of angles; what
    gives them away locally is that the internal coordinates recover omega, or the bond angles, of the wrong residue.  The
    two centring mutants are pure translations: no internal coordinate can see them (asserted: ratio <= 1), only the global
    comparison does."""
    ang = R.random_chain(n, n)
    for center in (True, False):
        ref = onerf.backbone_coords(ang, center)
        allow = R.chain_allowance(ang, center).reshape(-1)
        for name, (build, centred_only, internal) in MUTANTS.items():
            if centred_only and not center:
                continue
            xyz = build(ang, center)
            ratio = float((np.linalg.norm(xyz - ref, axis=-1) / allow).max())
            local = max(R.internal_ratio(xyz, ang).values())
            print(f"[nerf_ref] n={n} center={center} mutant '{name}': {ratio:.3g} x allowance, {local:.3g} x internal_bound")
            assert ratio >= 100.0, (name, center, ratio)
            if internal:
                assert local >= 100.0, (name, center, local)
            else:
                assert local <= 1.0, (name, center, local)


def test_allowance_is_not_slack():
    """``chain_allowance`` at the last atom, lengths 64 and 256 (printed).  At 64 residues of the fixture's distribution it
    is below 1e-4 A, the tolerance of test_next_rows.py, so the new comparison is the tighter one there.  FINDING, printed and
    recorded in DESIGN.md: for REGULAR chains of 64 residues (helix, extended) the same measurement gives 2e-4 .. 6e-4 A --
    a straight chain turns every frame error into the longest lever -- so the flat 1e-4 A of the existing test is not implied
    by the documented accuracy of sinf / cosf there; it is kept on top for every chain of up to 64 residues in
    test_nerf_forms_gpu.py and holds in practice because actual errors are far below the documented bound."""
    for n in (64, 256):
        for name in ("random", "helix", "extended"):
            ang = chains(n)[name]
            for center in (False, True):
                a = R.chain_allowance(ang, center)
                print(f"[nerf_ref] chain_allowance n={n} {name} center={center}: last atom {a[-1, -1]:.3e} A, "
                      f"largest {a.max():.3e} A, smallest {a.min():.3e} A")
                if n == 64 and name == "random":
                    assert a[-1, -1] < 1e-4 and a.max() < 1e-4
                assert a.min() > 0.0


def test_allowance_draws_are_seeded_and_leave_the_oracle_untouched():
    ang = R.random_chain(5, 77)
    first = R.chain_allowance(ang, True).copy()
    R._perturbed.clear()
    R._allowance.clear()
    assert np.array_equal(R.chain_allowance(ang, True), first) and onerf.np is np
    assert np.array_equal(onerf.backbone_coords(ang, False), R.batch_reference(ang[None], [5], False)[0].reshape(-1, 3))
    moved = np.linalg.norm(R.perturbed_coords(ang) - onerf.backbone_coords(ang, False), axis=-1)
    assert not moved[:, :3].any() and moved[:, 3:].all()            # the first frame is given; every placed atom moves


# ------------------------------------------------------------------------------------------------ pdb_text
def _atom_lines(text):
    return [ln for ln in text.splitlines() if ln.startswith("ATOM")]


def test_pdb_text_columns_hold_the_whole_range(pkg):
    from e3diff_amd.structure_model.create_pdb import pdb_text
    edge = [-999.999, -999.9994, -999.5, -100.0, -0.0004, 0.0, 0.0005, 9.9995, 999.9996, 1234.5678, 9999.999, 9999.9994]
    rng = np.random.default_rng(5)
    vals = np.concatenate([edge, rng.uniform(-999.999, 9999.999, 3 * 16 - len(edge))])
    xyz = rng.permutation(vals).reshape(16, 3)
    lines = _atom_lines(pdb_text(xyz))
    assert len(lines) == 16
    for ln, want in zip(lines, xyz):
        assert len(ln) == 78
        got = [float(ln[30:38]), float(ln[38:46]), float(ln[46:54])]
        assert np.abs(np.array(got) - want).max() <= 5.0001e-4
        assert ln[54:60] == "  1.00" and ln[60:66] == "  5.00" and ln[17:20] == "GLY"


@pytest.mark.parametrize("bad", (-1000.0, -999.9996, 9999.9996, 10000.0, -123456.789, 1e10, float("-inf"), float("nan")))
def test_pdb_text_refuses_a_coordinate_its_column_cannot_hold(pkg, bad):
    from e3diff_amd.structure_model.create_pdb import pdb_text
    xyz = np.zeros((8, 3))
    xyz[5, 1] = bad
    with pytest.raises(ValueError) as err:
        pdb_text(xyz)
    assert repr(float(bad)) in str(err.value) and "atom 6" in str(err.value)


def test_pdb_text_refuses_too_many_atoms_or_residues(pkg):
    from e3diff_amd.structure_model.create_pdb import pdb_text
    with pytest.raises(ValueError, match="100000 atoms"):
        pdb_text(np.zeros((100000, 3)))
    with pytest.raises(ValueError, match="10000 residues"):
        pdb_text(np.zeros((40000, 3)))
    lines = _atom_lines(pdb_text(np.zeros((4 * 9999, 3))))
    assert len(lines[-1]) == 78 and lines[-1][6:11] == "39996" and lines[-1][22:26] == "9999"


def test_pdb_text_of_an_uncentred_extended_chain_fits_or_raises(pkg):
    """256 residues, fully extended, uncentred -- the largest coordinates the builder makes at the project's frame (582 A):
    the text has whole columns or there is no text."""
    from e3diff_amd.structure_model.create_pdb import pdb_text
    xyz = onerf.backbone_coords(R.regular_chain(R.EXTENDED, 256), False)
    try:
        lines = _atom_lines(pdb_text(xyz))
    except ValueError:
        assert xyz.min() <= -999.9995 or xyz.max() >= 9999.9995
        return
    assert len(lines) == 1024 and all(len(ln) == 78 for ln in lines)
    got = np.array([[float(ln[30:38]), float(ln[38:46]), float(ln[46:54])] for ln in lines])
    assert np.abs(got - xyz).max() <= 5.0001e-4
