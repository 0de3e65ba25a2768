"""CPU: description of backbones without a native (csrc/backbone_geometry.hip, evaluate.describe_samples) -- the export
and its argument checks, the float64 restatement of the rules (dssp_ref.py) anchored on analytic chains whose secondary
structure is known, its handling of gaps, prolines, non-finite coordinates and bad offsets, the row assembly of
``describe_samples`` with both kernels replaced by their numpy statements, the default-off featurizer path, the tool."""
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dssp_ref as dr
import featurize_ref as fr
from oracle import nerf as onerf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------- 1. the export
def test_geometry_export_and_argument_checks(pkg):
    header = open(os.path.join(ROOT, "include", "e3d_hip.h")).read()
    declared = set(re.findall(r"\b(e3d_[a-z0-9_]+)\s*\(", header))
    lib = pkg.hip.lib()
    assert "e3d_backbone_geometry" in declared and "e3d_backbone_geometry" in pkg.hip.EXPORTS
    assert callable(lib.e3d_backbone_geometry) and lib.e3d_abi_version() == 5 == pkg.hip.ABI_VERSION
    section = header[header.index("backbone geometry: secondary structure"):]
    for words in ("THREE DIFFERENCES FROM DSSP", "not DSSP's two best partners", "|a - d| = 1", "not rounded to 0.001",
                  "mkdssp program has not been measured", "not a standard"):
        assert words in section, words
    source = open(os.path.join(ROOT, "e3-invaraint-diffusion-model_amd", "csrc", "backbone_geometry.hip")).read()
    assert "THREE DIFFERENCES FROM DSSP" in source and "atomic" not in source.replace("no atomics", "")
    # argument validation happens before any launch: callable without a GPU
    d, i = torch.zeros(64, dtype=torch.float64).data_ptr(), torch.zeros(64, dtype=torch.int32).data_ptr()
    good = [d, i, None, i, i, d, i, d, d, i, i, i]              # is_pro may be null
    assert len(good) == 12
    for missing in (0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11):
        args = list(good)
        args[missing] = None
        assert lib.e3d_backbone_geometry(*args, 1, 1, 2.5, 2.5, None) != 0
        assert b"null pointer" in lib.e3d_last_error()
    for counts in ((0, 1), (1, 0), (-1, 1)):
        assert lib.e3d_backbone_geometry(*good, *counts, 2.5, 2.5, None) != 0
        assert b"need all > 0" in lib.e3d_last_error()
    for cutoffs in ((0.0, 2.5), (2.5, 0.0), (-1.0, 2.5), (float("nan"), 2.5), (2.5, float("inf"))):
        assert lib.e3d_backbone_geometry(*good, 1, 1, *cutoffs, None) != 0
        assert b"> 0 and finite" in lib.e3d_last_error()


def test_wrapper_refuses_cpu_tensors(pkg):
    from e3diff_amd import evaluate
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate.backbone_geometry(torch.zeros(5, 4, 3, dtype=torch.float64), torch.tensor([0, 5]))
    sig = inspect.signature(evaluate.backbone_geometry)
    assert sig.parameters["clash_cutoff"].default == 2.5 and sig.parameters["max_peptide_bond"].default == 2.5


# ------------------------------------------------------------------------------- 2. the reference on analytic chains
@pytest.mark.parametrize("name", list(dr.ANALYTIC))
def test_reference_on_analytic_chains(name):
    """Ideal helices, extended chains and a two-residue hairpin built by the oracle's NeRF builder: the letters are known."""
    pp, want = dr.ANALYTIC[name]
    d = dr.describe(dr.chain_coords(pp))
    print(name, d["letters"], "hbonds", d["n_hbonds"], {k: f"{v:.3g}" for k, v in d["margins"].items()})
    assert d["letters"] == want
    assert min(d["margins"].values()) > 1e-3                        # no decision of these chains hangs on rounding
    assert not d["status"].any() and d["hbonds"].sum() == d["n_hbonds"]
    n = len(pp)
    if name in ("extended", "polyproline"):
        assert d["n_hbonds"] == 0 and not set(d["letters"]) & set("HGIEB")
        assert (d["kappa"][2:-2] < 70.0).all()
    step = {"alpha": 4, "3-10": 3, "pi": 5}.get(name)
    if step:                                                          # i -> i + step bonds, and nothing else
        assert {a - dn for (a, dn), e in d["energies"].items() if e < dr.E_HBOND} == {-step}
        assert (d["acc_rel"][step:, 0] == -step).all() and (d["don_rel"][:n - step, 0] == step).all()
        assert not d["acc_rel"][0].any() and not d["acc_e"][0].any()   # no amide hydrogen: absent partners, 0 with 0.0
        assert not d["hbonds"][:step].any() and (d["acc_e"][:step] > dr.E_HBOND).all()
        assert (d["acc_e"] <= 0.0).all() and (d["acc_e"][:, 0] <= d["acc_e"][:, 1]).all()
    if name == "hairpin":
        assert d["letters"][1:6] == "EEEEE" and d["letters"][8:13] == "EEEEE" and d["n_hbonds"] >= 4
    assert np.isnan(d["kappa"][[0, 1, n - 2, n - 1]]).all() and np.isfinite(d["kappa"][2:-2]).all()
    assert d["clash"].sum() % 2 == 0


def test_reference_gap_proline_nonfinite_and_offsets():
    X = dr.chain_coords(dr.ANALYTIC["alpha"][0])
    whole = dr.describe(X)
    # a 3 A C - N gap inside the helix: nothing spans it
    cut = X.copy()
    shift = (cut[8, 0] - cut[7, 2]) * (3.0 / np.linalg.norm(cut[8, 0] - cut[7, 2]) - 1.0)
    cut[8:] += shift
    assert abs(np.linalg.norm(cut[8, 0] - cut[7, 2]) - 3.0) < 1e-12
    g = dr.describe(cut)
    # 4-turns start at 0 .. 3 and 8 .. 11 only: two helices, and neither turn nor bend covers residues 7 and 8
    assert g["letters"] == "-HHHHHH--HHHHHH-" and np.isnan(g["kappa"][6:10]).all() and np.isfinite(g["kappa"][[5, 10]]).all()
    assert (g["acc_e"][8] == 0.0).all()                               # residue 8 has no amide hydrogen: it is not bonded
    # a looser bond test closes the gap again
    assert dr.describe(cut, max_peptide_bond=3.5)["letters"] == whole["letters"]
    # a proline donates nothing
    pro = np.zeros(16, dtype=bool)
    pro[9] = True
    p = dr.describe(X, pro)
    assert whole["hbonds"][9] == 1 and p["hbonds"][9] == 0 and not p["acc_rel"][9].any()
    assert p["n_hbonds"] == whole["n_hbonds"] - 1 and (p["hbonds"][np.arange(16) != 9] == whole["hbonds"][np.arange(16) != 9]).all()
    # a non-finite coordinate
    bad = X.copy()
    bad[5, 3, 1] = np.nan
    b = dr.describe(bad)
    assert b["status"].tolist() == [0] * 5 + [1] + [0] * 10 and b["letters"][5] == "-" and b["clash"][5] == 0
    assert not any(5 in pair for pair in b["energies"]) and not any((a, 6) == pair for pair in b["energies"] for a in range(16))
    # offsets: structures 1 and 2 are bad and are skipped, structure 3 is what it is alone
    coords = np.concatenate([X, X[:4], X])
    out = dr.describe_call(coords, [0, 16, 99, 20, 36])
    assert out["status"].tolist() == [0] * 16 + [3] * 4 + [0] * 16
    assert (out["ss"][:16] == out["ss"][20:]).all() and (out["ss"][16:20] == 7).all() and np.isnan(out["kappa"][16:20]).all()
    assert np.array_equal(out["acc_e"][:16], out["acc_e"][20:]) and out["structures"][1] is None


# ------------------------------------------------------------------------------- 3. describe_samples, row assembly
def numpy_build(angles, lengths):
    """The NeRF builder's contract through the oracle: [B,L,8] + lengths -> centred float64 [B,L,4,3], zero padding."""
    out = torch.zeros(angles.shape[0], angles.shape[1], 4, 3, dtype=torch.float64)
    for b, n in enumerate(lengths.tolist()):
        out[b, :n] = torch.from_numpy(onerf.backbone_coords(angles[b, :n].numpy(), True).reshape(n, 4, 3))
    return out


def numpy_geometry(coords, off, is_pro=None, clash_cutoff=2.5, max_peptide_bond=2.5):
    """The export's contract through dssp_ref."""
    out = dr.describe_call(coords.numpy(), off.tolist(), None if is_pro is None else is_pro.numpy(), clash_cutoff,
                           max_peptide_bond)
    return {k: torch.from_numpy(out[k]) for k in ("ss", "acc_rel", "acc_e", "don_rel", "don_e", "kappa", "clash", "hbonds",
                                                    "status")}


def stored_from_builder(B):
    """The inverse of evaluate.builder_angles_from_stored on the columns a builder reads: omega, theta1, theta3 move to
    the NEXT residue."""
    S = np.zeros_like(B)
    S[:, 1], S[:, 2], S[:, 3], S[:, 5], S[:, 7] = B[:, 0], B[:, 1], B[:, 3], B[:, 5], B[:, 7]
    S[1:, 0], S[1:, 4], S[1:, 6] = B[:-1, 2], B[:-1, 4], B[:-1, 6]
    return S


def sample_chains(seed, lengths):
    rng = np.random.default_rng(seed)
    return [dr.builder_angles(dr.block_chain_angles(rng, n)) for n in lengths]


def check_entry(row, key, r, X, pro=None, cutoff=2.5):
    want = dr.describe(X, pro, cutoff)
    get = (lambda k: row[key][k]) if r is None else (lambda k: row[k][r])
    n = len(X)
    assert get("ss") == want["letters"]
    assert get("helix_fraction") == pytest.approx(sum(c in "HGI" for c in want["letters"]) / n, abs=1e-12)
    assert get("strand_fraction") == pytest.approx(sum(c in "EB" for c in want["letters"]) / n, abs=1e-12)
    assert get("hbonds") == want["n_hbonds"] and isinstance(get("hbonds"), int)
    assert get("clashes") == int(want["clash"].sum()) // 2 and isinstance(get("clashes"), int)
    ca = X[:, 1]
    assert get("radius_of_gyration") == pytest.approx(np.sqrt(((ca - ca.mean(0)) ** 2).sum(-1).mean()), abs=1e-9)
    assert get("end_to_end") == pytest.approx(np.linalg.norm(ca[-1] - ca[0]), abs=1e-9)
    return want


@pytest.mark.parametrize("convention", ["stored", "labelled"])
def test_describe_samples_row_assembly(pkg, convention):
    from e3diff_amd import evaluate
    lengths = (16, 9, 23)
    builder = [sample_chains(60 + r, lengths) for r in range(3)]                     # [R][P] builder-convention angles
    given = [[stored_from_builder(a) if convention == "stored" else a for a in rep] for rep in builder]
    given[1] = [np.stack([np.zeros_like(a), a]) for a in given[1]]                   # [T,l,8]: the last step counts
    hooks = dict(device="cpu", _build=numpy_build, _geometry=numpy_geometry)
    rows = evaluate.describe_samples(given, convention=convention, **hooks)
    assert [r["index"] for r in rows] == [0, 1, 2] and [r["ligand_length"] for r in rows] == list(lengths)
    assert all("structure_ids" not in r and "native" not in r for r in rows)
    letters_seen, clashes = set(), 0
    for i, row in enumerate(rows):
        wants = [check_entry(row, None, r, onerf.backbone_coords(builder[r][i], True).reshape(-1, 4, 3)) for r in range(3)]
        prof = np.array(row["ss_profile"])
        assert prof.shape == (lengths[i], 8) and np.allclose(prof.sum(1), 1.0)
        for p in range(lengths[i]):
            for k in range(8):
                assert prof[p, k] == pytest.approx(sum(w["ss"][p] == k for w in wants) / 3, abs=1e-12)
        letters_seen |= set("".join(row["ss"]))
        clashes += sum(row["clashes"])
    assert len(letters_seen) >= 4 and clashes > 0                    # the assembly was checked on more than coil
    # a different clash cutoff reaches the kernel
    wide = evaluate.describe_samples(given, convention=convention, clash_cutoff=3.2, **hooks)
    check_entry(wide[0], None, 0, onerf.backbone_coords(builder[0][0], True).reshape(-1, 4, 3), cutoff=3.2)
    assert sum(wide[0]["clashes"]) > sum(rows[0]["clashes"])
    with pytest.raises(ValueError, match="convention"):
        evaluate.describe_samples(given, convention="builder", **hooks)
    with pytest.raises(ValueError, match="replicate 1"):
        evaluate.describe_samples([given[0], [a[:-1] for a in given[0]]], convention=convention, **hooks)
    with pytest.raises(ValueError, match="equally long"):
        evaluate.describe_samples([given[0], given[0][:2]], convention=convention, **hooks)
    with pytest.raises(ValueError, match="empty chain"):
        evaluate.describe_samples([[np.zeros((0, 8), dtype=np.float32)]], convention=convention, **hooks)
    assert "mkdssp" in evaluate.describe_samples.__doc__


def test_describe_samples_prolines_and_sequence_checks(pkg):
    from e3diff_amd import evaluate
    helix = dr.builder_angles(dr.ANALYTIC["alpha"][0])
    hooks = dict(device="cpu", _build=numpy_build, _geometry=numpy_geometry)
    seqs = [["A" * 16], ["AAAAAAAAAPAAAAAA"]]                                        # replicate 1: a proline at 9
    rows = evaluate.describe_samples([[helix], [helix]], sequences=seqs, convention="labelled", **hooks)
    X = onerf.backbone_coords(helix, True).reshape(-1, 4, 3)
    pro = np.arange(16) == 9
    plain, with_pro = check_entry(rows[0], None, 0, X), check_entry(rows[0], None, 1, X, pro)
    assert rows[0]["hbonds"] == [plain["n_hbonds"], plain["n_hbonds"] - 1] and with_pro["hbonds"][9] == 0
    for bad in ([["A" * 16], ["A" * 15]], [["A" * 16]], [["A" * 16, "A"], ["A" * 16, "A"]]):
        with pytest.raises(ValueError, match="sequence"):
            evaluate.describe_samples([[helix], [helix]], sequences=bad, convention="labelled", **hooks)


def test_describe_samples_with_a_dataset(pkg):
    from e3diff_amd import biolip, evaluate
    from e3diff_amd.structure_model.dataset import LigandBindingSiteDataset, NoisedAnglesDataset
    records = biolip.synthetic_records(2, seed=5, receptor_len=(20, 30), ligand_len=(6, 9))
    ds = LigandBindingSiteDataset(None, None, max_len=64, records=records)
    native = [d["angle_features"][d["ligand_mask"]].numpy() for d in ds.data]
    rng = np.random.default_rng(3)
    noisy = [a + rng.normal(size=a.shape).astype(np.float32) * 0.3 for a in native]
    hooks = dict(device="cpu", _build=numpy_build, _geometry=numpy_geometry)
    rows = evaluate.describe_samples([native, noisy], NoisedAnglesDataset(ds, timesteps=10), **hooks)
    assert rows == evaluate.describe_samples([native, noisy], ds, **hooks)            # a bare dataset
    for i, row in enumerate(rows):
        d = ds.data[i]
        lig = d["ligand_mask"].tolist()
        pro = np.array([a == "P" for a, m in zip(d["amino_acid"], lig) if m])
        assert row["structure_ids"] == d["structure_ids"] and row["ligand_length"] == native[i].shape[0]
        X = [onerf.backbone_coords(evaluate.builder_angles_from_stored(a), True).reshape(-1, 4, 3) for a in (native[i], noisy[i])]
        check_entry(row, "native", None, X[0], pro)                   # the native's prolines come from the record
        check_entry(row, None, 0, X[0])                               # a replicate without sequences has none
        check_entry(row, None, 1, X[1])
    with pytest.raises(ValueError, match="record's ligand"):
        evaluate.describe_samples([[a[:-1] for a in native]], ds, **hooks)


# ------------------------------------------------------------------------------- 4. the featurizer's default
def test_featurize_default_leaves_records_as_they_were(pkg):
    from e3diff_amd import biolip, featurize
    for fn in (featurize.record_from_chains, featurize.records_from_pdb_files):
        assert inspect.signature(fn).parameters["secondary_structure"].default is False
    rec_xyz = dr.chain_coords(dr.ANALYTIC["alpha"][0] + dr.HAIRPIN)
    lig_xyz = dr.chain_coords(dr.ANALYTIC["3-10"][0]) + 30.0
    chains = featurize.read_pdb(fr.pdb_text_for_chains([("A", "A" * 30, rec_xyz), ("B", "G" * 12, lig_xyz)]))
    angles = [fr.chain_angles(c.backbone.astype(np.float64)).astype(np.float32) for c in (chains["A"], chains["B"])]
    kw = dict(pocket=[(5, ""), (6, "")], angles=angles, pdb_id="x")                   # no kernel is needed
    rec = featurize.record_from_chains(chains["A"], chains["B"], **kw)
    same = featurize.record_from_chains(chains["A"], chains["B"], secondary_structure=False, **kw)
    assert rec["secondary_structure"] == ["-"] * 38 and not rec["numerical_features"].any()
    assert rec.keys() == same.keys()
    for k in rec:
        assert torch.equal(rec[k], same[k]) if torch.is_tensor(rec[k]) else rec[k] == same[k]
    biolip.validate_record(rec)
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # the letters come from the kernel alone
        featurize.record_from_chains(chains["A"], chains["B"], secondary_structure=True, device="cpu", **kw)


# ------------------------------------------------------------------------------- 5. the tools
def load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tools_arguments_tables_and_summary():
    import pandas as pd
    tool = load_tool("describe_samples")
    args = tool.parse_args(["a.pkl", "b.pkl", "-o", "report.json"])
    assert args.samples == ["a.pkl", "b.pkl"] and args.data is None and args.table is None and args.clash_cutoff == 2.5
    args = tool.parse_args(["a.pkl", "--data", "biolip.pt", "--table", "output.pkl", "--convention", "labelled", "-o", "r.json"])
    assert (args.data, args.table, args.convention) == ("biolip.pt", "output.pkl", "labelled")
    table = pd.DataFrame({"structure_ids": ["1abc_B", "2xyz_C"], "true_sequence": ["AAAA", "GGG"],
                          "predict_sequence": ["APAA", "GGP"], "recovery_rate": [0.5, 0.6]})
    assert tool.table_sequences(table, [4, 3]) == ["APAA", "GGP"]                    # by position
    assert tool.table_sequences(table, [3, 4], ["2xyz_C", "1abc_B"]) == ["GGP", "APAA"]   # by id
    with pytest.raises(ValueError, match="residues"):
        tool.table_sequences(table, [4, 4])
    with pytest.raises(ValueError, match="no sequence for"):
        tool.table_sequences(table, [4, 3], ["1abc_B", "9zzz_A"])
    with pytest.raises(ValueError, match="predict_sequence"):
        tool.table_sequences(table.drop(columns="predict_sequence"), [4, 3])
    rows = [{"ss": ["HH", "--"], "helix_fraction": [1.0, 0.0], "strand_fraction": [0.0, 0.0], "hbonds": [2, 0],
             "clashes": [0, 4], "radius_of_gyration": [2.0, 4.0]}]
    assert tool.summarize(rows) == {"pockets": 1, "replicates": 2, "mean_helix_fraction": 0.5, "mean_strand_fraction": 0.0,
                                    "mean_hbonds": 1.0, "mean_clashes": 2.0, "mean_radius_of_gyration": 3.0,
                                    "share_without_clash": 0.5}
    feat = load_tool("featurize_pdb")
    assert feat.parse_args(["c.pdb", "--receptor", "A", "--ligand", "B", "--dssp", "-o", "o.pt"]).dssp is True
    assert feat.parse_args(["c.pdb", "--receptor", "A", "--ligand", "B", "-o", "o.pt"]).dssp is False
