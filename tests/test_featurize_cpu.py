"""CPU: PDB featurization (featurize.py) -- the float64 statement of the eight stored angles against the reference's own
functions, the column map against the NeRF builder, the PDB parser, record assembly with injected angles, the exports."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

import featurize_ref as fr
from helpers import GOLDEN
from oracle import nerf as onerf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def angles_fx():
    return torch.load(os.path.join(GOLDEN, "backbone_angles.pt"), weights_only=False)


def nerf_angles(n, seed):
    rng = np.random.default_rng(seed)
    ang = np.empty((n, 8), dtype=np.float32)
    ang[:, :4] = rng.uniform(-np.pi, np.pi, (n, 4))
    ang[:, 4:] = rng.normal(1.95, 0.1, (n, 4))
    return ang


# ------------------------------------------------------------------------------- 1. the fp64 statement
def test_numpy_statement_matches_the_reference_functions():
    """Both sides are float64 and every fixture dihedral stays >= 1e-3 rad from planar (asserted by the generator), where
    the reference's arccos and sign are exact to ~1e-12: 1e-9 rad, wrapped difference, on every case."""
    fx = angles_fx()
    assert tuple(fx["columns"]) == fr.COLUMNS
    names = [c["name"] for c in fx["cases"]]
    assert {"omega_near_trans", "omega_near_cis", "psi_straddles_pi"} <= set(names)
    assert sorted({c["coords"].shape[0] for c in fx["cases"]}) == [3, 4, 33, 70]
    for c in fx["cases"]:
        assert c["coords"].dtype == torch.float32 and c["angles"].dtype == torch.float64
        want = c["angles"].numpy()
        dih = np.abs(want[1:-1, :4])
        assert dih.min() > 1e-3 and dih.max() < np.pi - 1e-3, c["name"]
        got = fr.chain_angles(c["coords"].numpy())
        err = fr.wrapped(got - want).max()
        print(f"{c['name']}: max wrapped |numpy - reference| = {err:.2e}")
        assert err <= 1e-9, c["name"]
        assert not got[0].any() and not got[-1].any()


# ------------------------------------------------------------------------------- 2. column map
def test_column_map_round_trip_through_the_nerf_builder(pkg):
    """angles -> oracle.nerf coordinates -> featurize_ref recovers the angles under featurize_ref.column_map.  A swapped
    column, a sign or an off-by-one neighbour errs by >= 0.1 rad; float32-cast coordinates cost ~6e-6: assert <= 1e-4."""
    from e3diff_amd import biolip
    assert fr.COLUMNS == biolip.STORED_ANGLE_COLUMNS
    for seed in range(4):
        A = nerf_angles(64, seed)
        for cast in (np.float64, np.float32):
            xyz = onerf.backbone_coords(A, center=bool(seed % 2)).reshape(-1, 4, 3).astype(cast)
            err = fr.wrapped(fr.chain_angles(xyz)[1:-1] - fr.column_map(A)).max()
            print(f"seed {seed} {cast.__name__}: {err:.2e}")
            assert err <= 1e-4


# ------------------------------------------------------------------------------- 3. parser
def _line(rec, serial, name, alt, resname, chain, resseq, icode, xyz, element):
    return "%-6s%5d %-4s%1s%3s %1s%4d%1s   %8.3f%8.3f%8.3f%6.2f%6.2f          %2s" % (
        rec, serial, name, alt, resname, chain, resseq, icode, *xyz, 1.0, 20.0, element)


def _residue(serial, resname, chain, resseq, icode, base):
    """four backbone ATOM lines at distinct three-decimal coordinates derived from ``base``."""
    out = []
    for k, (name, el) in enumerate(((" N  ", "N"), (" CA ", "C"), (" C  ", "C"), (" O  ", "O"))):
        out.append(_line("ATOM", serial + k, name, " ", resname, chain, resseq, icode,
                         (base + k + 0.125, -base - 0.5 * k, 0.001 * (base + k)), el))
    return out


def parser_text():
    lines = ["HEADER    TEST", "MODEL        1"]
    lines += _residue(1, "ALA", "A", 10, " ", 1.0)
    lines += _residue(5, "GLY", "A", 10, "A", 11.0)                      # insertion code
    ser = _residue(9, "SER", "A", 11, " ", 21.0)
    # alternate locations of CA: A first, then B -- the first one seen is kept
    ser[1] = _line("ATOM", 10, " CA ", "A", "SER", "A", 11, " ", (22.125, -21.5, 0.022), "C")
    ser.insert(2, _line("ATOM", 11, " CA ", "B", "SER", "A", 11, " ", (99.0, 99.0, 99.0), "C"))
    lines += ser
    lines.append(_line("ATOM", 14, " CB ", " ", "SER", "A", 11, " ", (23.5, -20.25, 1.75), "C"))
    lines.append(_line("ATOM", 15, " H  ", " ", "SER", "A", 11, " ", (5.0, 5.0, 5.0), "H"))
    lines.append(_line("ATOM", 16, "1HB ", " ", "SER", "A", 11, " ", (6.0, 6.0, 6.0), "")[:66])   # no element column
    lines.append("TER")
    lines += _residue(17, "LYS", "B", 1, " ", 31.0)
    lines += _residue(21, "TRP", "B", 2, " ", 41.0)
    lines.append(_line("HETATM", 25, " O  ", " ", "HOH", "A", 201, " ", (7.0, 7.0, 7.0), "O"))
    lines.append("ENDMDL")
    lines.append("MODEL        2")
    lines += _residue(1, "ALA", "A", 10, " ", 501.0)
    lines += _residue(5, "PRO", "C", 1, " ", 601.0)
    lines += ["ENDMDL", "END"]
    return "\n".join(lines) + "\n"


def _bb(base):
    return np.array([(base + k + 0.125, -base - 0.5 * k, 0.001 * (base + k)) for k in range(4)], dtype=np.float32)


def test_read_pdb(pkg, tmp_path):
    from e3diff_amd import featurize
    text = parser_text()
    chains = featurize.read_pdb(text)
    assert list(chains) == ["A", "B"]                                   # model 2 (and its chain C) is not read
    a, b = chains["A"], chains["B"]
    assert (a.resseq, a.icode, a.resname, a.seq) == ([10, 10, 11], ["", "A", ""], ["ALA", "GLY", "SER"], "AGS")
    assert (b.resseq, b.icode, b.seq) == ([1, 2], ["", ""], "KW")
    assert a.backbone.dtype == np.float32 and a.backbone.shape == (3, 4, 3)
    assert np.array_equal(a.backbone, np.stack([_bb(1.0), _bb(11.0), _bb(21.0)]))      # altloc A of CA, exactly
    assert np.array_equal(b.backbone, np.stack([_bb(31.0), _bb(41.0)]))
    # heavy atoms in file order: hydrogens, the second altloc and the water are gone; CB belongs to residue 2
    assert a.atoms.shape == (13, 3) and a.atom_res.tolist() == [0] * 4 + [1] * 4 + [2] * 5
    assert np.array_equal(a.atoms[-1], np.array([23.5, -20.25, 1.75], dtype=np.float32))
    assert b.atoms.shape == (8, 3) and b.atom_res.dtype == np.int32
    # from a path, restricted to one chain
    p = tmp_path / "x.pdb"
    p.write_text(text)
    only = featurize.read_pdb(str(p), chains=["B"])
    assert list(only) == ["B"] and np.array_equal(only["B"].backbone, b.backbone)
    with pytest.raises(ValueError, match="Z"):
        featurize.read_pdb(text, chains=["Z"])
    # a residue without its O, and a non-standard residue, are named
    no_o = "\n".join(ln for ln in text.splitlines() if not (ln.startswith("ATOM") and ln[12:16] == " O  " and ln[22:27] == "  10A"))
    with pytest.raises(ValueError, match=r"GLY A10A.*\bO\b"):
        featurize.read_pdb(no_o + "\n")
    with pytest.raises(ValueError, match=r"UNK B2"):
        featurize.read_pdb(text.replace("TRP", "UNK"))
    assert list(featurize.read_pdb(text.replace("TRP", "UNK"), chains=["A"])) == ["A"]   # only kept chains are checked
    assert "mmCIF" in featurize.read_pdb.__doc__


def test_read_pdb_inverts_create_pdb_text(pkg):
    from e3diff_amd import featurize
    from e3diff_amd.structure_model.create_pdb import pdb_text
    xyz = onerf.backbone_coords(nerf_angles(17, 5), True)
    chain = featurize.read_pdb(pdb_text(xyz))["A"]
    assert chain.seq == "G" * 17 and chain.resseq == list(range(1, 18))
    assert np.abs(chain.backbone.reshape(-1, 3) - xyz).max() <= 5e-4


# ------------------------------------------------------------------------------- 4. record assembly
@pytest.fixture(scope="module")
def complex_chains(pkg):
    from e3diff_amd import featurize
    rec_xyz = onerf.backbone_coords(nerf_angles(12, 1), True).reshape(-1, 4, 3)
    lig_xyz = onerf.backbone_coords(nerf_angles(8, 2), True).reshape(-1, 4, 3) + 6.0
    text = fr.pdb_text_for_chains([("A", "ACDEFGHIKLMN", rec_xyz), ("B", "PQRSTVWY", lig_xyz)])
    chains = featurize.read_pdb(text)
    return chains["A"], chains["B"], (fr.chain_angles(chains["A"].backbone), fr.chain_angles(chains["B"].backbone))


def test_record_from_chains_with_injected_angles(pkg, complex_chains):
    from e3diff_amd import biolip, featurize
    from e3diff_amd.structure_model.dataset import LigandBindingSiteDataset
    receptor, ligand, angles = complex_chains
    rec = featurize.record_from_chains(receptor, ligand, pocket=[(5, ""), (8, "")], angles=angles, pdb_id="syn")
    assert biolip.validate_record(rec) == 10 + 6
    assert rec["structure_ids"] == {"pdb_id": "syn", "receptor_chain": "A", "ligand_chain": "B"}
    # trimming: first and last residue of each chain are gone, receptor first
    assert "".join(rec["amino_acid"]) == "CDEFGHIKLM" + "QRSTVW"
    assert np.array_equal(rec["coors"].numpy(), np.concatenate([receptor.backbone[1:-1, 1], ligand.backbone[1:-1, 1]]))
    want = np.concatenate([angles[0][1:-1], angles[1][1:-1]]).astype(np.float32)
    assert rec["angle_features"].dtype == torch.float32 and np.array_equal(rec["angle_features"].numpy(), want)
    assert (rec["angle_features"].abs().sum(1) > 0).all()               # no boundary (zero) row survives the trimming
    assert rec["secondary_structure"] == ["-"] * 16 and not rec["numerical_features"].any()
    assert tuple(rec["numerical_features"].shape) == (16, 5)
    assert rec["ligand_idx"].tolist() == list(range(10, 16)) and rec["ligand_idx"].dtype == torch.int32
    # reference_pocket_shift=True: resseq 5 is position 4 of the untrimmed chain, applied to the trimmed arrays = resseq 6
    assert rec["pocket_idx"].tolist() == [4, 7] and [rec["amino_acid"][i] for i in (4, 7)] == ["G", "K"]
    assert rec["edge_index"].dtype == torch.int64 and tuple(rec["edge_index"].shape) == (2, 12)
    assert rec["edge_index"][:, 0].tolist() == [10, 4]
    named = featurize.record_from_chains(receptor, ligand, pocket=[(5, ""), (8, "")], angles=angles,
                                         reference_pocket_shift=False)
    assert named["pocket_idx"].tolist() == [3, 6] and [named["amino_acid"][i] for i in (3, 6)] == ["F", "I"]
    assert torch.equal(named["coors"][3], torch.from_numpy(receptor.backbone[4, 1]))      # resseq 5 itself
    # an empty pocket
    empty = featurize.record_from_chains(receptor, ligand, pocket=[], angles=angles)
    assert tuple(empty["edge_index"].shape) == (2, 0) and empty["edge_index"].dtype == torch.int64
    assert not empty["pocket_mask"].any() and biolip.validate_record(empty) == 16
    # positions that leave the trimmed receptor are dropped with a warning, not marked on the ligand
    with pytest.warns(UserWarning, match="A11"):
        edge = featurize.record_from_chains(receptor, ligand, pocket=[(11, "")], angles=angles)
    assert edge["pocket_idx"].tolist() == []
    with pytest.raises(ValueError, match="A40"):
        featurize.record_from_chains(receptor, ligand, pocket=[(40, "")], angles=angles)
    # the dataset consumes the record
    item = LigandBindingSiteDataset(None, None, max_len=64, records=[rec])[0]
    assert item["ligand_angles"].shape == (64, 8) and item["receptor_angles"].shape == (64, 8)
    assert item["receptor_seq"].shape == (64, 20) and item["ligand_attn_mask"].shape == (64,)
    assert int(item["ligand_length"]) == 6 and int(item["receptor_length"]) == 6     # two pocket residues dilated by 1
    assert torch.equal(item["ligand_angles"][:6], rec["angle_features"][10:])


def test_record_design_mode_and_checks(pkg, complex_chains, tmp_path):
    from e3diff_amd import biolip, featurize
    receptor, ligand, angles = complex_chains
    rec = featurize.record_from_chains(receptor, pocket=[(4, ""), (5, "")], ligand_length=7, angles=(angles[0], None))
    assert biolip.validate_record(rec) == 17
    assert rec["amino_acid"][10:] == ["G"] * 7 and not rec["angle_features"][10:].any() and not rec["coors"][10:].any()
    assert rec["structure_ids"]["ligand_chain"] == "" and rec["pocket_idx"].tolist() == [3, 4]
    with pytest.raises(ValueError, match="ligand_length"):
        featurize.record_from_chains(receptor, pocket=[(4, "")], angles=(angles[0], None))
    with pytest.raises(ValueError, match="pocket"):
        featurize.record_from_chains(receptor, ligand_length=7, angles=(angles[0], None))
    # a ligand of 4 residues after trimming
    short = ligand._replace(resseq=ligand.resseq[:6], icode=ligand.icode[:6], resname=ligand.resname[:6], seq=ligand.seq[:6],
                            backbone=ligand.backbone[:6], atoms=ligand.atoms[:24], atom_res=ligand.atom_res[:24])
    with pytest.raises(ValueError, match="fewer than 5"):
        featurize.record_from_chains(receptor, short, pocket=[], angles=(angles[0], angles[1][:6]))
    # status bits of kept rows: bit 1 raises and names the residue, bit 2 warns and names it
    st = np.zeros(12, dtype=np.int32)
    st[[0, -1]] = featurize.STATUS_NOT_INTERIOR
    bad = st.copy()
    bad[3] |= featurize.STATUS_DEGENERATE
    with pytest.raises(ValueError, match="GLU A4"):
        featurize.record_from_chains(receptor, pocket=[], ligand_length=5, angles=(angles[0], None), status=(bad, None))
    gap = st.copy()
    gap[6] |= featurize.STATUS_CHAIN_BREAK
    with pytest.warns(UserWarning, match="HIS A7"):
        featurize.record_from_chains(receptor, pocket=[], ligand_length=5, angles=(angles[0], None), status=(gap, None))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        featurize.record_from_chains(receptor, pocket=[], ligand_length=5, angles=(angles[0], None), status=(st, None))
    # write(): validates, then saves what biolip.load reads back
    path = featurize.write(str(tmp_path / "biolip.pt"), [rec])
    again = biolip.load(path)
    assert torch.equal(again[0]["angle_features"], rec["angle_features"]) and again[0]["amino_acid"] == rec["amino_acid"]
    with pytest.raises(biolip.BiolipSchemaError):
        featurize.write(str(tmp_path / "bad.pt"), [dict(rec, ligand_mask=~rec["ligand_mask"])])
    assert "featurize" in pkg.__all__


def test_kernel_wrappers_refuse_cpu_tensors(pkg):
    from e3diff_amd import featurize
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        featurize.backbone_angles(torch.zeros(3, 4, 3), torch.zeros(3, dtype=torch.int32))
    z = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        featurize.contact_residues(torch.zeros(1, 3), z[:1], z, torch.zeros(1, 3), z, 1)


def test_featurize_tool_parses_its_arguments(pkg):
    import importlib.util
    spec = importlib.util.spec_from_file_location("featurize_pdb", os.path.join(ROOT, "tools", "featurize_pdb.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = tool.parse_args(["a.pdb", "b.pdb", "--receptor", "A", "--pocket", "45,46,52A,-3", "--ligand-length", "12",
                            "-o", "out.pt"])
    jobs = tool.jobs_from_args(args)
    assert [j["path"] for j in jobs] == ["a.pdb", "b.pdb"]
    assert jobs[0]["pocket"] == [(45, ""), (46, ""), (52, "A"), (-3, "")] and jobs[0]["ligand_length"] == 12
    assert jobs[0]["receptor"] == "A" and jobs[0]["ligand"] is None
    jobs = tool.jobs_from_args(tool.parse_args(["c.pdb", "--receptor", "A", "--ligand", "B", "-o", "out.pt"]))
    assert jobs[0]["ligand"] == "B" and jobs[0]["pocket"] is None


# ------------------------------------------------------------------------------- 5. exports
def test_featurize_exports(pkg):
    header = open(os.path.join(ROOT, "include", "e3d_hip.h")).read()
    declared = set(re.findall(r"\b(e3d_[a-z0-9_]+)\s*\(", header))
    lib = pkg.hip.lib()
    for name in ("e3d_backbone_angles", "e3d_contact_residues"):
        assert name in declared and name in pkg.hip.EXPORTS and callable(getattr(lib, name))
    assert "additions to ABI v5" in header[header.index("featurization of PDB coordinates"):][:200]
    assert lib.e3d_abi_version() == 5 == pkg.hip.ABI_VERSION
    # argument validation happens before any launch: callable without a GPU
    assert lib.e3d_backbone_angles(None, None, None, None, 4, 2.0, None) != 0
    assert b"null pointer" in lib.e3d_last_error()
    assert lib.e3d_contact_residues(None, None, None, None, None, None, 1, 1, 1, 1, 4.0, None) != 0
    assert b"null pointer" in lib.e3d_last_error()
    buf = (torch.zeros(16), torch.zeros(16, dtype=torch.int32))
    f, i = buf[0].data_ptr(), buf[1].data_ptr()
    assert lib.e3d_backbone_angles(f, i, f, i, 0, 2.0, None) != 0 and b"R = 0" in lib.e3d_last_error()
    assert lib.e3d_backbone_angles(f, i, f, i, 1, 0.0, None) != 0 and b"max_peptide_bond" in lib.e3d_last_error()
    assert lib.e3d_contact_residues(f, i, i, f, i, i, 1, 1, 1, 1, 0.0, None) != 0 and b"cutoff" in lib.e3d_last_error()
    assert lib.e3d_contact_residues(f, i, i, f, i, i, 1, 0, 1, 1, 4.0, None) != 0
