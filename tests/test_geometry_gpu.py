"""GPU: the backbone-geometry kernel (csrc/backbone_geometry.hip) against its float64 restatement (dssp_ref.py), and the
layers on it (evaluate.describe_samples, featurize ... secondary_structure=True).

Letters, clash counts, hydrogen-bond counts and partner indices are compared for EQUALITY.  That is sound because the
reference records how far every threshold decision is from its threshold, and each test first asserts, on the reference
side, that no relative margin is below 1e-9 -- seven orders of magnitude above what float64 rounding can move these
expressions by (dssp_ref's docstring).  Energies and kappa are compared under dssp_ref.energy_bound / kappa_bound, which
are derived from the operations performed, not fitted; two partners whose energies differ by less than that bound may
come out in either order.  The worst observed ratios to the bounds are printed, and recorded in DESIGN.md."""
import numpy as np
import pytest
import torch

import dssp_ref as dr
import featurize_ref as fr

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 3, 5, 6, 63, 64, 65, 257)               # below every window, around the wave, more than one workgroup
SEED = 1
MIN_MARGIN = 1e-9
KEYS = ("ss", "acc_rel", "acc_e", "don_rel", "don_e", "kappa", "clash", "hbonds", "status")


def launch(evaluate, coords, off, is_pro=None, **kw):
    out = evaluate.backbone_geometry(torch.from_numpy(np.asarray(coords, dtype=np.float64)).cuda(),
                                     torch.from_numpy(np.asarray(off, dtype=np.int32)).cuda(),
                                     None if is_pro is None else torch.from_numpy(np.asarray(is_pro)).cuda(), **kw)
    assert set(out) == set(KEYS) and out["ss"].dtype == torch.uint8 and out["acc_e"].dtype == torch.float64
    assert out["acc_rel"].dtype == out["clash"].dtype == out["status"].dtype == torch.int32
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_margins(margins):
    print("smallest relative margins:", {k: f"{v:.3g}" for k, v in margins.items()})
    assert min(margins.values()) >= MIN_MARGIN, margins


def compare(got, want):
    """Equality of every decision, the bounds on every value; returns the worst observed error / bound ratios."""
    for k in ("ss", "clash", "hbonds", "status"):
        assert np.array_equal(got[k], want[k]), k
    worst_e = 0.0
    for side in ("acc", "don"):
        rel, e = got[side + "_rel"], got[side + "_e"]
        wrel, we, wb = want[side + "_rel"], want[side + "_e"], want[side + "_bound"]
        for i in range(len(rel)):
            order = [0, 1]
            if not np.array_equal(rel[i], wrel[i]):               # the one freedom: two partners closer than the bound
                assert abs(we[i, 0] - we[i, 1]) < max(wb[i]) and np.array_equal(rel[i], wrel[i][::-1]), (side, i, rel[i], wrel[i])
                order = [1, 0]
            for k in range(2):
                err, bound = abs(e[i, k] - we[i, order[k]]), wb[i, order[k]]
                assert err <= bound, (side, i, k, err, bound)      # an absent partner: 0.0 against 0.0 under a bound of 0
                if bound > 0:
                    worst_e = max(worst_e, err / bound)
    assert np.array_equal(np.isnan(got["kappa"]), np.isnan(want["kappa"]))
    has = ~np.isnan(want["kappa"])
    err = np.abs(got["kappa"][has] - want["kappa"][has])
    assert (err <= want["kappa_bound"][has]).all()
    worst_k = float((err / want["kappa_bound"][has]).max()) if has.any() else 0.0
    return worst_e, worst_k


@pytest.fixture(scope="module")
def main(pkg, hip):
    """ONE launch over chains of every size, the 65-residue one repeated at the start, in the middle and at the end; the
    reference of each structure, computed once."""
    from e3diff_amd import evaluate
    rng = np.random.default_rng(SEED)
    chain = {n: dr.chain_coords(dr.block_chain_angles(rng, n)) for n in SIZES}
    order = [65, 1, 2, 3, 5, 6, 63, 65, 64, 65, 257, 65]
    coords = np.concatenate([chain[n] for n in order])
    off = np.cumsum([0] + order).astype(np.int32)
    want = dr.describe_call(coords, off, cache={})
    got = launch(evaluate, coords, off)
    return dict(order=order, coords=coords, off=off, want=want, got=got)


# ------------------------------------------------------------------------------- 1. the main launch
def test_the_case_set_is_worth_comparing(main):
    """Asserted on the reference alone: every letter occurs, chains clash, and no decision hangs on rounding."""
    want = main["want"]
    counts = {c: int((want["ss"] == k).sum()) for k, c in enumerate(dr.SS)}
    clashes = int(want["clash"].sum()) // 2
    print("letters:", counts, "clashing pairs:", clashes)
    assert min(counts.values()) >= 5, counts
    assert clashes >= 1
    assert_margins(want["margins"])
    assert not want["status"].any()


def test_letters_counts_partners_and_values_match_the_reference(main):
    worst_e, worst_k = compare(main["got"], main["want"])
    print(f"worst |E - ref| / energy_bound = {worst_e:.3f}, worst |kappa - ref| / kappa_bound = {worst_k:.3f}")
    assert (main["got"]["acc_e"] <= 0.0).all() and (main["got"]["acc_e"] >= -9.9).all()


def test_a_structure_does_not_depend_on_its_place_in_the_call(pkg, hip, main):
    from e3diff_amd import evaluate
    off, got = main["off"], main["got"]
    copies = [s for s, n in enumerate(main["order"]) if n == 65]
    assert copies == [0, 7, 9, 11]
    first = slice(off[0], off[1])
    for s in copies[1:]:
        for k in KEYS:
            assert np.array_equal(got[k][first], got[k][off[s]:off[s + 1]], equal_nan=True), (s, k)
    alone = launch(evaluate, main["coords"][off[10]:off[11]], [0, 257])      # a launch of its own: the same bits
    for k in KEYS:
        assert np.array_equal(alone[k], got[k][off[10]:off[11]], equal_nan=True), k


# ------------------------------------------------------------------------------- 2. edge cases
def test_gap_proline_and_nonfinite_coordinate(pkg, hip):
    from e3diff_amd import evaluate
    X = dr.chain_coords(dr.ANALYTIC["alpha"][0])
    cut = X.copy()                                                   # a 3 A C - N gap inside the helix
    cut[8:] += (cut[8, 0] - cut[7, 2]) * (3.0 / np.linalg.norm(cut[8, 0] - cut[7, 2]) - 1.0)
    bad = X.copy()
    bad[5, 3, 1] = np.nan
    worse = X.copy()
    worse[11, 1, 0] = np.inf
    coords = np.concatenate([X, cut, X, bad, worse])
    off = np.arange(6) * 16
    pro = np.zeros(80, dtype=np.uint8)
    pro[32 + 9] = 1                                                  # a helix donor of the third copy
    want = dr.describe_call(coords, off, pro)
    assert_margins(want["margins"])
    got = launch(evaluate, coords, off, pro)
    compare(got, want)
    letters = ["".join(dr.SS[v] for v in got["ss"][a:a + 16]) for a in off[:-1]]
    assert letters[0] == letters[2] == "-HHHHHHHHHHHHHH-"
    # the gap: no turn, bridge or bend spans it
    assert letters[1] == "-HHHHHH--HHHHHH-" and np.isnan(got["kappa"][16 + 6:16 + 10]).all()
    assert not got["acc_rel"][16 + 8].any() and got["hbonds"][16 + 8] == 0          # not bonded: no amide hydrogen
    # the proline: its hydrogen bond is gone, the rest of the helix keeps its own
    assert got["hbonds"][9] == 1 and got["hbonds"][32 + 9] == 0 and not got["acc_e"][32 + 9].any()
    others = np.arange(16) != 9
    assert np.array_equal(got["hbonds"][32:48][others], got["hbonds"][:16][others])
    assert got["don_rel"][32 + 5, 0] != 4 and got["don_rel"][5, 0] == 4              # the acceptor lost that donor
    # the NaN: status 1, '-', and its neighbours lose only what contiguity takes
    assert got["status"].tolist() == [0] * 48 + [0] * 5 + [1] + [0] * 10 + [0] * 11 + [1] + [0] * 4
    assert letters[3][5] == "-" and got["clash"][48 + 5] == 0 and not got["acc_rel"][48 + 5].any()
    assert np.isnan(got["kappa"][48 + 3:48 + 8]).all() and np.isfinite(got["kappa"][48 + 8:48 + 14]).all()
    assert np.array_equal(got["kappa"][48 + 8:48 + 14], got["kappa"][8:14])
    assert letters[3][9:] == letters[0][9:] and letters[4][:7] == letters[0][:7]
    # a loose peptide-bond test closes the gap; a wide clash cutoff counts more pairs: both reach the kernel
    loose = launch(evaluate, cut, [0, 16], max_peptide_bond=3.5, clash_cutoff=3.4)
    want = dr.describe_call(cut, [0, 16], None, 3.4, 3.5)
    assert_margins(want["margins"])
    compare(loose, want)
    assert loose["clash"].sum() > got["clash"][16:32].sum() and np.isfinite(loose["kappa"][2:14]).all()


@pytest.mark.parametrize("off", [[0, 16, 99, 20, 36], [-3, 16, 36], [0, 16, 36, 20], [0, 16, 20, 37]])
def test_a_bad_offset_touches_nothing_else(pkg, hip, off):
    """An offset past the buffer, below zero or descending: its structure is skipped and nothing is read through it;
    residues no good structure holds get status 3; the good structures are what they are in a launch of their own."""
    from e3diff_amd import evaluate
    X = dr.chain_coords(dr.ANALYTIC["hairpin"][0] + dr.ANALYTIC["alpha"][0][:2])
    assert len(X) == 16
    coords = np.concatenate([X, X[:4], X])
    want = dr.describe_call(coords, off)
    good = [s for s, one in enumerate(want["structures"]) if one is not None]
    held = np.zeros(36, dtype=bool)
    for s in good:
        held[off[s]:off[s + 1]] = True
    assert 0 < len(good) < len(off) - 1
    assert_margins(want["margins"])
    got = launch(evaluate, coords, off)
    compare(got, want)
    assert (got["status"][~held] == 3).all() and not got["status"][held].any()
    assert (got["ss"][~held] == 7).all() and np.isnan(got["kappa"][~held]).all() and not got["clash"][~held].any()
    assert not got["acc_rel"][~held].any() and not got["don_e"][~held].any()
    for s in good:
        alone = launch(evaluate, coords[off[s]:off[s + 1]], [0, off[s + 1] - off[s]])
        for k in KEYS:
            assert np.array_equal(alone[k], got[k][off[s]:off[s + 1]], equal_nan=True), (s, k)


# ------------------------------------------------------------------------------- 3. end to end
def test_describe_samples_end_to_end(pkg, hip):
    """3 pockets x 2 replicates through the device path (one NeRF launch, one geometry call, device sums) against the
    stand-in path of the CPU test, evaluated on the coordinates the device built (captured through the build hook)."""
    from test_geometry_cpu import numpy_geometry, sample_chains
    from e3diff_amd import evaluate
    from e3diff_amd.structure_model.create_pdb import backbone_from_angles
    lengths = (16, 9, 23)
    given = [sample_chains(70 + r, lengths) for r in range(2)]
    seqs = [["A" * n for n in lengths], ["AAP" + "A" * (n - 6) + "PAA" for n in lengths]]
    seen, margins = {}, []

    def build(angles, chain_len):
        seen["coords"] = backbone_from_angles(angles.cuda(), chain_len.cuda(), True)
        return seen["coords"]

    def checked_geometry(coords, off, is_pro, clash_cutoff, max_peptide_bond):
        margins.append(dr.describe_call(coords.numpy(), off.tolist(), is_pro.numpy())["margins"])
        return numpy_geometry(coords, off, is_pro, clash_cutoff, max_peptide_bond)

    rows = evaluate.describe_samples(given, sequences=seqs, convention="labelled", _build=build)
    want = evaluate.describe_samples(given, sequences=seqs, convention="labelled", device="cpu",
                                     _build=lambda a, l: seen["coords"].cpu(), _geometry=checked_geometry)
    assert_margins(margins[0])
    assert len(rows) == 3 and [r.keys() for r in rows] == [w.keys() for w in want]
    for row, ref in zip(rows, want):
        for k in ("index", "ligand_length", "ss", "hbonds", "clashes", "ss_profile"):
            assert row[k] == ref[k], k
        for k in ("helix_fraction", "strand_fraction", "radius_of_gyration", "end_to_end"):
            assert row[k] == pytest.approx(ref[k], rel=1e-12, abs=1e-12), k
    assert len(set("".join(s for r in rows for s in r["ss"]))) >= 4 and sum(sum(r["clashes"]) for r in rows) > 0


def test_featurize_with_secondary_structure(pkg, hip):
    """A two-chain complex and a design-mode job in one call: the record's letters are the reference's on the record's own
    rows (receptor then ligand, one structure), everything else is what the default gives."""
    from e3diff_amd import biolip, featurize
    rec_xyz = dr.chain_coords(dr.ANALYTIC["alpha"][0] + dr.HAIRPIN)
    lig_xyz = dr.chain_coords(dr.ANALYTIC["3-10"][0])
    lig_xyz = lig_xyz + (rec_xyz[22, 1] + np.array([1.0, 2.0, 6.5]) - lig_xyz[6, 1])
    seqs = ["A" * 9 + "P" + "A" * 20, "G" * 5 + "P" + "G" * 6]
    text = fr.pdb_text_for_chains([("A", seqs[0], rec_xyz), ("B", seqs[1], lig_xyz)])
    jobs = [{"path": text, "receptor": "A", "ligand": "B", "pocket": [(20, ""), (21, "")], "pdb_id": "cplx"},
            {"path": text, "receptor": "A", "pocket": [(20, ""), (21, "")], "ligand_length": 7, "pdb_id": "design"}]
    plain = featurize.records_from_pdb_files(jobs, "cuda:0")
    records = featurize.records_from_pdb_files(jobs, "cuda:0", secondary_structure=True)
    chains = featurize.read_pdb(text)
    rows = [np.concatenate([chains["A"].backbone[1:-1], chains["B"].backbone[1:-1]]), chains["A"].backbone[1:-1]]
    pros = [np.array([c == "P" for c in seqs[0][1:-1] + seqs[1][1:-1]]), np.array([c == "P" for c in seqs[0][1:-1]])]
    for rec, base, X, pro in zip(records, plain, rows, pros):
        want = dr.describe(X.astype(np.float64), pro)
        assert_margins(want["margins"])
        n = len(X)
        assert "".join(rec["secondary_structure"][:n]) == want["letters"]
        assert rec["secondary_structure"][n:] == ["-"] * (len(rec["amino_acid"]) - n)      # design-mode placeholders
        assert len(set(want["letters"])) >= 3 and want["hbonds"][8] == 0                  # the proline at row 8 donates nothing
        biolip.validate_record(rec)
        assert base["secondary_structure"] == ["-"] * len(base["amino_acid"]) and not rec["numerical_features"].any()
        for k in rec:
            if k != "secondary_structure":
                assert torch.equal(rec[k], base[k]) if torch.is_tensor(rec[k]) else rec[k] == base[k], k
    one = featurize.record_from_chains(chains["A"], chains["B"], pocket=[(20, ""), (21, "")], pdb_id="cplx", device="cuda:0",
                                       secondary_structure=True)
    assert one["secondary_structure"] == records[0]["secondary_structure"]
