"""GPU: the two featurization kernels (csrc/backbone_angles.hip) and the PDB -> record -> sampler -> PDB path.

Tolerance of the angle kernel: 2.5e-7 rad, wrapped difference = one float32 ulp at pi.  The kernel's float64 algebra and
the float64 evaluation it is compared with (the reference's functions in the fixture, or featurize_ref on the same
float32 coordinates) each contribute under 1e-9; the single final rounding to float32 at most half an ulp."""
import os

import numpy as np
import pytest
import torch

import featurize_ref as fr
from helpers import GOLDEN
from oracle import nerf as onerf

pytestmark = pytest.mark.gpu
TOL = 2.5e-7


def nerf_angles(n, seed):
    rng = np.random.default_rng(seed)
    ang = np.empty((n, 8), dtype=np.float32)
    ang[:, :4] = rng.uniform(-np.pi, np.pi, (n, 4))
    ang[:, 4:] = rng.normal(1.95, 0.1, (n, 4))
    return ang


def chain_xyz(n, seed, center=True):
    return onerf.backbone_coords(nerf_angles(n, seed), center).reshape(-1, 4, 3).astype(np.float32)


def run_kernel(featurize, chains, seg_ids=None, **kw):
    """chains: list of [n,4,3] float32 -> (angles [R,8] float64 numpy, status [R] numpy), one launch."""
    seg_ids = seg_ids if seg_ids is not None else range(len(chains))
    coords = torch.from_numpy(np.concatenate(chains))
    seg = torch.from_numpy(np.concatenate([np.full(len(c), s, dtype=np.int32) for c, s in zip(chains, seg_ids)]))
    ang, st = featurize.backbone_angles(coords.cuda(), seg.cuda(), **kw)
    assert ang.dtype == torch.float32 and st.dtype == torch.int32
    return ang.cpu().double().numpy(), st.cpu().numpy()


def interior_mask(lengths):
    m = []
    for n in lengths:
        m += [False] + [True] * max(n - 2, 0) + ([False] if n > 1 else [])
    return np.array(m)


# ------------------------------------------------------------------------------- 6. against the reference fixture
def test_angle_kernel_matches_the_reference(pkg, hip):
    from e3diff_amd import featurize
    fx = torch.load(os.path.join(GOLDEN, "backbone_angles.pt"), weights_only=False)
    chains = [c["coords"].numpy() for c in fx["cases"]]
    want = np.concatenate([c["angles"].numpy() for c in fx["cases"]])
    got, st = run_kernel(featurize, chains)                               # all cases in ONE launch
    inner = interior_mask([len(c) for c in chains])
    err = fr.wrapped(got - want)
    for c, (a, b) in zip(fx["cases"], zip(np.cumsum([0] + [len(c) for c in chains]), np.cumsum([len(c) for c in chains]))):
        print(f"{c['name']}: max wrapped |kernel - reference| = {err[a:b].max():.3e}")
    assert err[inner].max() <= TOL
    assert (st[inner] == 0).all()
    assert not got[~inner].any() and (st[~inner] == featurize.STATUS_NOT_INTERIOR).all()


# ------------------------------------------------------------------------------- 7. indexing
@pytest.mark.parametrize("lengths", [(1,), (2,), (3,), (5, 1, 7, 2, 33, 3, 19), (70, 1, 64, 2, 3, 117)],
                         ids=lambda v: f"R{sum(v)}")
def test_angle_kernel_indexing(pkg, hip, lengths):
    """Chains of 1 and 2 residues between longer ones, different geometry per chain, the same seg id on non-adjacent
    chains: every interior row equals featurize_ref of ITS chain alone (no cross-chain read), every other row is zero."""
    from e3diff_amd import featurize
    assert sum(lengths) in (1, 2, 3, 70, 257)
    chains = [chain_xyz(n, 100 + i, center=bool(i % 2)) for i, n in enumerate(lengths)]
    got, st = run_kernel(featurize, chains, seg_ids=[(7, 3)[i % 2] if i != 4 else -1 for i in range(len(lengths))])
    want = np.concatenate([fr.chain_angles(c) for c in chains])
    inner = interior_mask(lengths)
    assert got.shape == (sum(lengths), 8)
    if inner.any():
        assert fr.wrapped(got - want)[inner].max() <= TOL and (st[inner] == 0).all()
    assert not got[~inner].any() and (st[~inner] == featurize.STATUS_NOT_INTERIOR).all()
    assert st[0] == featurize.STATUS_NOT_INTERIOR and st[-1] == featurize.STATUS_NOT_INTERIOR


def test_angle_kernel_stays_inside_its_buffer(pkg, hip):
    """The rows handed over are the middle of a longer chain whose outer rows carry the SAME seg id and valid atoms: a
    kernel that looked at row -1 or row R would find the first and last row interior."""
    from e3diff_amd import featurize
    for R in (1, 2, 3, 70, 257):
        whole = torch.from_numpy(chain_xyz(R + 2, 200 + R)).cuda()
        seg = torch.zeros(R + 2, dtype=torch.int32, device="cuda")
        ang, st = featurize.backbone_angles(whole[1:-1], seg[1:-1])
        assert whole[1:-1].data_ptr() == whole.data_ptr() + 48 and ang.shape == (R, 8)
        ang, st = ang.cpu().double().numpy(), st.cpu().numpy()
        want = fr.chain_angles(whole[1:-1].cpu().numpy())
        assert st[0] == featurize.STATUS_NOT_INTERIOR and st[-1] == featurize.STATUS_NOT_INTERIOR
        assert not ang[0].any() and not ang[-1].any()
        if R > 2:
            assert fr.wrapped(ang - want)[1:-1].max() <= TOL and (st[1:-1] == 0).all()


# ------------------------------------------------------------------------------- 8. status bits
def test_angle_kernel_status_bits(pkg, hip):
    from e3diff_amd import featurize
    dup = chain_xyz(10, 301)
    dup[4, 1] = dup[4, 0]                         # CA of residue 4 on top of its N: a zero-length bond
    gap = chain_xyz(10, 302)
    gap[5:] += np.float32(5.0)                    # residues 5.. translated by 5 A along each axis: a chain break after 4
    intact = chain_xyz(10, 303)
    bond = np.linalg.norm(intact[1:, 0].astype(np.float64) - intact[:-1, 2], axis=-1)
    assert np.abs(bond - 1.34).max() < 1e-4       # the NeRF builder's peptide bond
    got, st = run_kernel(featurize, [dup, gap, intact])
    with np.errstate(all="ignore"):               # the numpy statement is undefined (NaN) on the degenerate row
        want = np.concatenate([fr.chain_angles(c) for c in (dup, gap, intact)])
    D, B = featurize.STATUS_DEGENERATE, featurize.STATUS_CHAIN_BREAK
    # the duplicated atom: bit 1 on its residue, zeros written; its neighbours stay defined
    assert st[4] & D and not got[4].any()
    assert [int(s) for s in st[1:4]] == [0, 0, 0] and [int(s) for s in st[5:9]] == [0, 0, 0, 0]
    assert fr.wrapped(got - want)[[1, 2, 3, 5, 6, 7, 8]].max() <= TOL
    # the gap: bit 2 on both sides, angles still written
    g = st[10:20]
    assert g[4] == B and g[5] == B and [int(s) for s in g[[1, 2, 3, 6, 7, 8]]] == [0] * 6
    assert fr.wrapped(got - want)[11:19].max() <= TOL and np.abs(got[14]).min() > 0 and np.abs(got[15]).min() > 0
    # the intact chain: neither bit
    assert (st[21:29] == 0).all() and fr.wrapped(got - want)[21:29].max() <= TOL
    # a threshold below the bond length flags every interior row
    _, tight = run_kernel(featurize, [intact], max_peptide_bond=1.0)
    assert (tight[1:-1] == B).all()


# ------------------------------------------------------------------------------- 9. device round trip
def test_device_round_trip_angles_to_coordinates_to_angles(pkg, hip):
    from e3diff_amd import featurize
    from e3diff_amd.structure_model.create_pdb import backbone_from_angles
    B, L = 3, 33
    A = np.stack([nerf_angles(L, 400 + b) for b in range(B)])
    xyz = backbone_from_angles(torch.from_numpy(A).cuda(), torch.full((B,), L).cuda(), center=True).float()
    seg = torch.arange(B, dtype=torch.int32, device="cuda").repeat_interleave(L)
    ang, st = featurize.backbone_angles(xyz.reshape(B * L, 4, 3), seg)
    ang = ang.cpu().double().numpy().reshape(B, L, 8)
    host = xyz.cpu().numpy()
    assert (st.cpu().numpy().reshape(B, L)[:, 1:-1] == 0).all()
    for b in range(B):
        same_coords = fr.wrapped(ang[b] - fr.chain_angles(host[b]))[1:-1].max()
        mapped = fr.wrapped(ang[b, 1:-1] - fr.column_map(A[b])).max()
        print(f"item {b}: vs featurize_ref {same_coords:.3e}, vs the generating angles {mapped:.3e}")
        assert same_coords <= TOL
        assert mapped <= 1e-4           # a swapped column, a sign or an off-by-one neighbour errs by >= 0.1 rad


# ------------------------------------------------------------------------------- 10. contact kernel
CUTOFF = 4.0


def brute_force(rec, rec_row, lig, n_rows, cutoff):
    """float64 from the float32 coordinates -> (hit [n_rows], smallest | distance - cutoff |)."""
    hit = np.zeros(n_rows, dtype=np.int32)
    if len(lig) == 0 or len(rec) == 0:
        return hit, np.inf
    d = np.linalg.norm(rec.astype(np.float64)[:, None] - lig.astype(np.float64)[None], axis=-1)
    np.maximum.at(hit, rec_row, (d.min(1) <= cutoff).astype(np.int32))
    return hit, np.abs(d - cutoff).min()


def make_complex(rng, n_rec, n_lig, near=None):
    """receptor atoms in a 24 A box in residues of 1-9 atoms, ligand atoms in an 8 A box inside it; regenerated until no
    pair lies within 1e-3 A of the cutoff, so float32 against float64 distance arithmetic cannot change a verdict."""
    while True:
        rec = rng.uniform(0, 24, (n_rec, 3)).astype(np.float32)
        lig = rng.uniform(8, 16, (n_lig, 3)).astype(np.float32)
        if near is not None:
            lig = rec[:1] + np.array([3.0 if near else 30.0, 0.0, 0.0], dtype=np.float32)
        row = np.sort(rng.integers(0, max(1, n_rec // 5), n_rec)).astype(np.int32)
        row = np.unique(row, return_inverse=True)[1].astype(np.int32)       # rows 0 .. k-1, every one with an atom
        n_rows = int(row.max()) + 1
        hit, margin = brute_force(rec, row, lig, n_rows, CUTOFF)
        if margin > 1e-3:
            return rec, row, lig, n_rows, hit


def run_contacts(featurize, complexes):
    rec = np.concatenate([c[0] for c in complexes])
    lig = np.concatenate([c[2] for c in complexes])
    row0 = np.cumsum([0] + [c[3] for c in complexes])
    row = np.concatenate([c[1] + row0[i] for i, c in enumerate(complexes)]).astype(np.int32)
    rec_off = np.cumsum([0] + [len(c[0]) for c in complexes]).astype(np.int32)
    lig_off = np.cumsum([0] + [len(c[2]) for c in complexes]).astype(np.int32)
    dev = [torch.from_numpy(a).cuda() for a in (rec, row, rec_off, lig, lig_off)]
    hit = featurize.contact_residues(*dev, n_rows=int(row0[-1]), cutoff=CUTOFF)
    assert hit.dtype == torch.int32 and tuple(hit.shape) == (int(row0[-1]),)
    return hit.cpu().numpy(), np.concatenate([c[4] for c in complexes])


def test_contact_kernel_matches_brute_force(pkg, hip):
    from e3diff_amd import featurize
    rng = np.random.default_rng(5)
    for near in (True, False):                                            # (1, 1): one verdict of each kind
        got, want = run_contacts(featurize, [make_complex(rng, 1, 1, near=near)])
        assert got.tolist() == want.tolist() == [int(near)]
    one = make_complex(rng, 300, 70)
    got, want = run_contacts(featurize, [one])
    assert 0 < want.sum() < len(want) and np.array_equal(got, want)
    # three complexes in one launch in the SAME region of space, the middle one without a ligand: its residues sit
    # among the other complexes' ligand atoms and must stay 0
    batch = [make_complex(rng, 50, 20), make_complex(rng, 120, 0), make_complex(rng, 77, 33)]
    got, want = run_contacts(featurize, batch)
    assert np.array_equal(got, want)
    a, b = batch[0][3], batch[0][3] + batch[1][3]
    assert not got[a:b].any() and got[:a].any() and got[b:].any() and not got.all()
    # no ligand atom at all: zeros, without a zero-sized launch
    got, want = run_contacts(featurize, [make_complex(rng, 40, 0)])
    assert not got.any() and not want.any()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------- 11. end to end
def test_pdb_to_record_to_sampler_to_pdb(pkg, hip, tmp_path):
    """PDB text -> records_from_pdb_files -> biolip.validate -> dataset -> two reverse steps of a tiny structure model ->
    PDB files.  Angles recovered from the three-decimal PDB text: within 1e-2 rad of the generating ones under the column
    map (the rounding of the coordinates costs ~2e-3 rad; any mix-up >= 0.1)."""
    from helpers import seeded_state_dict
    from e3diff_amd import biolip, featurize
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.structure_model.create_pdb import write_preds_pdb_folder
    from e3diff_amd.structure_model.dataset import LigandBindingSiteDataset
    from e3diff_amd.structure_model.model import ConditionalBertForDiffusionBase
    from e3diff_amd.structure_model.sample import p_sample_loop
    from e3diff_amd.structure_model.utils import CosineTables, modulo_with_wrapped_range
    A_rec, A_lig = nerf_angles(40, 501), nerf_angles(10, 502)
    rec_xyz = onerf.backbone_coords(A_rec, True).reshape(-1, 4, 3)
    lig_xyz = onerf.backbone_coords(A_lig, True).reshape(-1, 4, 3)
    lig_xyz = lig_xyz + (rec_xyz[20, 1] + 3.0 - lig_xyz[5, 1])             # beside the receptor: CA 5 at ~5 A of CA 20
    rng = np.random.default_rng(7)
    seqs = ["".join(rng.choice(list(biolip.AA_VOCAB), n)) for n in (40, 10)]
    text = fr.pdb_text_for_chains([("A", seqs[0], rec_xyz), ("B", seqs[1], lig_xyz)])
    path = tmp_path / "cplx.pdb"
    path.write_text(text)
    design = {"path": text, "receptor": "A", "pocket": [(20, ""), (21, "")], "ligand_length": 9, "pdb_id": "design"}
    records = featurize.records_from_pdb_files([{"path": str(path), "receptor": "A", "ligand": "B"}, design], "cuda:0")
    assert biolip.validate(records) == (38 + 8) + (38 + 9)
    rec = records[0]
    assert rec["structure_ids"] == {"pdb_id": "cplx", "receptor_chain": "A", "ligand_chain": "B"}
    assert "".join(rec["amino_acid"]) == seqs[0][1:-1] + seqs[1][1:-1]
    got = rec["angle_features"].double().numpy()
    err = max(fr.wrapped(got[:38] - fr.column_map(A_rec)).max(), fr.wrapped(got[38:] - fr.column_map(A_lig)).max())
    print(f"angles from the PDB text against the generating ones: {err:.3e} rad")
    assert err <= 1e-2
    # the pocket by contact: what a float64 brute force over the parsed atoms finds, shifted as the reference does
    chains = featurize.read_pdb(text)
    d = np.linalg.norm(chains["A"].atoms.astype(np.float64)[:, None] - chains["B"].atoms.astype(np.float64)[None], axis=-1)
    assert np.abs(d - 4.0).min() > 1e-3
    named = sorted(set(chains["A"].atom_res[d.min(1) <= 4.0].tolist()))
    assert named and rec["pocket_idx"].tolist() == [p for p in named if p < 38]
    assert records[1]["pocket_idx"].tolist() == [19, 20] and torch.equal(records[1]["angle_features"][:38], rec["angle_features"][:38])
    featurize.write(str(tmp_path / "biolip.pt"), records)
    # the sampler on the record
    L = 64
    item = LigandBindingSiteDataset(None, None, max_len=L, records=biolip.load(str(tmp_path / "biolip.pt"))[:1])[0]
    c = dict(hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=1, max_position_embeddings=L)
    model = ConditionalBertForDiffusionBase(BertConfig(**c), BertConfig(**c, is_decoder=True, add_cross_attention=True), 8)
    model.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=1))
    model = model.eval().cuda()
    d = {k: item[k][None].cuda() for k in ("ligand_attn_mask", "receptor_seq", "receptor_attn_mask", "receptor_angles")}
    torch.manual_seed(0)
    x_T = modulo_with_wrapped_range(torch.randn(1, L, 8)).cuda()
    traj = p_sample_loop(model, d["ligand_attn_mask"], x_T, d["receptor_seq"], d["receptor_attn_mask"],
                         d["receptor_angles"], 2, CosineTables(2), disable_pbar=True, step=1, use_graph=False)
    assert traj.shape == (2, 1, L, 8) and torch.isfinite(traj).all()
    n_lig = int(item["ligand_length"])
    files = write_preds_pdb_folder([traj[-1, 0, :n_lig].numpy()], str(tmp_path / "out"))
    assert len(files) == 1 and os.path.exists(files[0])
    again = featurize.read_pdb(files[0])["A"]
    assert len(again.seq) == n_lig and np.isfinite(again.backbone).all()
