"""Score sampled peptides on the device: superposition RMSD to the native, ensembles of replicates, clashes.

The step after ``structure_model/sample.py`` and ``create_pdb.py``: the keyed streams make replicates cheap (one seed per
replicate), and a batch of pockets times tens of replicates is 1e5 .. 1e6 structure pairs to superpose.  All pairs of a
call go through ONE launch of ``e3d_superpose_pairs`` (csrc/superpose.hip): float64, one wave per pair, the optimal
PROPER rotation from Horn's quaternion eigenproblem -- a mirror image is never "superposed" by a reflection.

CONVENTION: ``x' = R x + t`` maps the mobile structure onto the reference one (``R`` row-major [3,3]); RMSD is the square
root of the kernel's mean squared deviation.  On near-identical structures the msd is good to ~32 eps64 G / n (G: the two
sets' summed squared radii), which is ~1e-6 Angstrom of RMSD: compare squares when it matters.
Status per pair: 0 ok; 1 atom counts differ; 2 empty; 3 bad index or offset; 4 non-finite coordinate (NaN results).

Angle columns.  A ``biolip.pt`` record STORES (omega, phi, psi, dihedral_o, theta1, theta2, theta3, theta_o) with omega,
theta1 and theta3 on the residue they place (biolip.py); the datasets label these columns (phi, psi, omega, dihedral_o,
tau, CA:C:1N, 1C:N:CA, CA:C:O) and the samplers produce the same columns; the NeRF builder (csrc/nerf.hip) WANTS
the labelled meaning, with omega, tau and 1C:N:CA on the PREVIOUS residue.  ``builder_angles_from_stored`` is the map;
``create_pdb.py`` keeps feeding the columns as labelled, as the reference does.

WITHOUT A NATIVE (design mode) none of the above applies; ``describe_samples`` says what each backbone IS instead --
secondary structure, backbone hydrogen bonds, clashes, size -- through ONE call of ``e3d_backbone_geometry``
(csrc/backbone_geometry.hip: Kabsch & Sander's rules in float64, a thread per residue; its header states the rules and the
three differences from DSSP).  Agreement with the mkdssp program has not been measured.
"""
import numpy as np
import torch

from . import hip
from .featurize import _require_cuda, contact_residues

ATOMS_PER_RESIDUE = {"CA": 1, "backbone": 4}
DEFAULT_CLASH_CUTOFF = 3.0     # Angstrom between a receptor C-alpha and any placed backbone atom


# ------------------------------------------------------------------------------------------------ the kernel
def superpose_msd(xyz, off, mob, ref, transform=True):
    """xyz [n_atoms,3] (all structures back to back), off [n_structs+1] (atom offsets, off[0] = 0), mob / ref [n_pairs]
    (structure indices) -> (msd f64 [n_pairs], R f64 [n_pairs,3,3] or None, t f64 [n_pairs,3] or None, status i32 [n_pairs]).
    The export itself; inputs are converted to contiguous float64 / int32.  ``transform=False`` skips R and t."""
    _require_cuda("superpose", xyz, off, mob, ref)
    n_atoms, n_structs, n_pairs = xyz.shape[0], off.shape[0] - 1, mob.shape[0]
    assert tuple(xyz.shape) == (n_atoms, 3) and off.dim() == 1 and tuple(ref.shape) == (n_pairs,), \
        (xyz.shape, off.shape, mob.shape, ref.shape)
    x = xyz.contiguous().double()
    o, m, r = (t.to(torch.int32).contiguous() for t in (off, mob, ref))
    msd = torch.empty((n_pairs,), device=x.device, dtype=torch.float64)
    status = torch.empty((n_pairs,), device=x.device, dtype=torch.int32)
    R = torch.empty((n_pairs, 3, 3), device=x.device, dtype=torch.float64) if transform else None
    t = torch.empty((n_pairs, 3), device=x.device, dtype=torch.float64) if transform else None
    hip.check(hip.lib().e3d_superpose_pairs(x.data_ptr(), o.data_ptr(), m.data_ptr(), r.data_ptr(), msd.data_ptr(),
                                            R.data_ptr() if transform else None, t.data_ptr() if transform else None,
                                            status.data_ptr(), n_structs, n_atoms, n_pairs,
                                            torch.cuda.current_stream().cuda_stream), "e3d_superpose_pairs")
    return msd, R, t, status


def superpose(xyz, off, mob, ref, transform=True):
    """``superpose_msd`` with the square root taken: (rmsd, R, t, status); ``x' = R x + t`` maps structure mob[p] onto
    structure ref[p].  Pairs with a status other than 0 hold NaN."""
    msd, R, t, status = superpose_msd(xyz, off, mob, ref, transform)
    return msd.sqrt(), R, t, status


# ------------------------------------------------------------------------------------------------ packing (any device)
def select_atoms(coords, atoms="CA"):
    """[B,L,4,3] (N, CA, C, O per residue, what ``backbone_from_angles`` returns) or [B,L,3] (C-alpha only) -> [B,L,k,3]
    with k = 1 (``"CA"``) or 4 (``"backbone"``)."""
    if atoms not in ATOMS_PER_RESIDUE:
        raise ValueError(f"atoms = {atoms!r}: one of {sorted(ATOMS_PER_RESIDUE)}")
    if coords.dim() == 3 and coords.shape[-1] == 3:
        if atoms != "CA":
            raise ValueError("[B,L,3] coordinates hold C-alpha atoms only: atoms must be 'CA'")
        return coords[:, :, None, :]
    if coords.dim() != 4 or tuple(coords.shape[2:]) != (4, 3):
        raise ValueError(f"coordinates must be [B,L,4,3] or [B,L,3], got {tuple(coords.shape)}")
    return coords[:, :, 1:2, :] if atoms == "CA" else coords


def flatten_by_lengths(coords, lengths):
    """Padded [B,L,k,3] + lengths [B] -> (flat [sum(l_i) k, 3], off int32 [B+1]): the first l_i residues of each item, back
    to back -- the layout of ``superpose``."""
    B, L, k = coords.shape[:3]
    lens = torch.as_tensor(lengths, device=coords.device).to(torch.int64).reshape(-1)
    if lens.shape[0] != B or int(lens.min()) < 0 or int(lens.max()) > L:
        raise ValueError(f"lengths must be {B} values in [0, {L}]")
    keep = torch.arange(L, device=coords.device)[None, :] < lens[:, None]
    off = torch.zeros(B + 1, device=coords.device, dtype=torch.int64)
    off[1:] = torch.cumsum(lens * k, 0)
    return coords[keep].reshape(-1, 3), off.to(torch.int32)


def group_pairs(groups, lengths):
    """groups: a sequence of sequences of structure indices; lengths: the structures' lengths (host values) ->
    (mob, ref, bounds): all pairs i < j WITHIN each group in row-major upper-triangle order, never across groups; group g
    owns pairs bounds[g] .. bounds[g+1]-1 (R_g (R_g - 1) / 2 of them).  ValueError if a group mixes lengths."""
    lengths = np.asarray([int(v) for v in lengths], dtype=np.int64)
    mob, ref, bounds, upper = [], [], [0], {}
    for g, members in enumerate(groups):
        members = np.asarray([int(m) for m in members], dtype=np.int32)
        seen = np.unique(lengths[members])
        if len(seen) > 1:
            raise ValueError(f"group {g} mixes structures of lengths {seen.tolist()}: RMSD needs one atom correspondence")
        if len(members) not in upper:
            upper[len(members)] = np.triu_indices(len(members), 1)
        a, b = upper[len(members)]
        mob.append(members[a])
        ref.append(members[b])
        bounds.append(bounds[-1] + len(a))
    empty = np.zeros(0, dtype=np.int32)
    return np.concatenate(mob + [empty]), np.concatenate(ref + [empty]), bounds


# ------------------------------------------------------------------------------------------------ RMSD of padded batches
def rmsd_to_reference(mobile, reference, lengths, atoms="CA", transform=False, _superpose=None):
    """Item b of ``mobile`` against item b of ``reference`` over its first lengths[b] residues, all in one launch.
    Both padded [B,L,4,3] (``backbone_from_angles``' output) or [B,L,3] (C-alpha only); their L may differ.
    -> rmsd f64 [B], or (rmsd, R [B,3,3], t [B,3]) with ``transform`` (``x' = R x + t`` places mobile on reference).
    An item of length 0 gives NaN."""
    sp = _superpose or superpose
    B = mobile.shape[0]
    flat_m, off_m = flatten_by_lengths(select_atoms(mobile, atoms), lengths)
    flat_r, off_r = flatten_by_lengths(select_atoms(reference.to(mobile.device), atoms), lengths)
    xyz = torch.cat([flat_m.double(), flat_r.double()])
    off = torch.cat([off_m, off_r[1:] + off_m[-1]])
    idx = torch.arange(B, device=xyz.device, dtype=torch.int32)
    rmsd, R, t, _ = sp(xyz, off, idx, idx + B, transform)
    return (rmsd, R, t) if transform else rmsd


def pairwise_rmsd(coords, lengths, groups, atoms="CA", _superpose=None):
    """All pairs i < j within each group of structure indices in ONE launch -> a list with one symmetric [R_g, R_g] float64
    RMSD matrix per group (exact zero diagonal; [[0]] for a group of one).  ``lengths`` are read on the host; a group that
    mixes lengths raises ValueError before anything is launched."""
    sp = _superpose or superpose
    lens = torch.as_tensor(lengths).reshape(-1).tolist()
    mob, ref, bounds = group_pairs(groups, lens)
    flat, off = flatten_by_lengths(select_atoms(coords, atoms), lens)
    rmsd = None
    if len(mob):
        dev = flat.device
        rmsd = sp(flat.double(), off, torch.from_numpy(mob).to(dev), torch.from_numpy(ref).to(dev), False)[0]
    out, upper = [], {}
    for g, members in enumerate(groups):
        n = len(members)
        mat = torch.zeros((n, n), device=flat.device, dtype=torch.float64)
        if n > 1:
            if n not in upper:
                upper[n] = torch.triu_indices(n, n, 1, device=flat.device)
            iu = upper[n]
            mat[iu[0], iu[1]] = rmsd[bounds[g]:bounds[g + 1]]
            mat = mat + mat.T
        out.append(mat)
    return out


def medoid(mat):
    """The index with the smallest mean RMSD to the others; ties go to the lowest index (NaN entries count as +inf)."""
    total = torch.nan_to_num(torch.as_tensor(mat, dtype=torch.float64), nan=float("inf")).sum(1)
    return int(torch.nonzero(total == total.min())[0])


def neighbour_counts(mat, cutoff):
    """How many OTHER structures lie within ``cutoff`` RMSD of each one (a torch op on the matrix's device): the size of
    each structure's cluster, the medoid of the largest being the usual representative."""
    return (mat <= cutoff).sum(1) - 1


# ------------------------------------------------------------------------------------------------ angle columns
def builder_angles_from_stored(S):
    """Angles in a record's STORED meaning (biolip.STORED_ANGLE_COLUMNS; also what the samplers emit, since they are
    trained on records) [..., n, 8] -> the NeRF builder's input (create_pdb.COLS), same shape and type:
        B[i] = [S[i,1], S[i,2], S[i+1,0], S[i,3], S[i+1,4], S[i,5], S[i+1,6], S[i,7]]
    omega, theta1 (tau) and theta3 (1C:N:CA) move to the PREVIOUS residue; the missing S[n] entries are 0 and never read
    by the builder.  Pure indexing: torch tensors on any device, or numpy arrays."""
    if torch.is_tensor(S):
        nxt = torch.zeros_like(S)
        stack = torch.stack
    else:
        S = np.asarray(S)
        nxt = np.zeros_like(S)
        stack = np.stack
    nxt[..., :-1, :] = S[..., 1:, :]
    return stack([S[..., 1], S[..., 2], nxt[..., 0], S[..., 3], nxt[..., 4], S[..., 5], nxt[..., 6], S[..., 7]], -1)


# ------------------------------------------------------------------------------------------------ samples against records
def _records_of(dataset):
    return dataset.dset.data if hasattr(dataset, "dset") else dataset.data


def _device_build(angles, lengths, device):
    from .structure_model.create_pdb import backbone_from_angles
    return backbone_from_angles(angles.to(device), lengths.to(device), True)


def evaluate_samples(replicates, dataset, convention="stored", clash_cutoff=DEFAULT_CLASH_CUTOFF, device="cuda",
                     return_placed=False, _superpose=None, _build=None, _contacts=None):
    """Score R replicates of P pockets against their records.

    replicates: a list of R sampler outputs, each a list of P arrays [l_i,8] or [T,l_i,8] (the last step is taken), as
        ``sample()`` / ``create_pdb.load_sampled_angles`` give them; item i belongs to ``dataset.dset.data[i]`` (or
        ``dataset.data[i]`` of a bare ``LigandBindingSiteDataset``): build the dataset as the sampler did
        (``structure_model.sample.get_dataset``), since the dataset shuffles its records.
    convention: ``"stored"`` (default) reads the eight columns as records store them and applies
        ``builder_angles_from_stored`` before building; ``"labelled"`` feeds them to the builder as labelled, which is what
        ``create_pdb.py`` and the reference do.
    Steps, each ONE launch over all pockets and replicates: the NeRF builder on every replicate and on the native angles
    (``angle_features[ligand_mask]``); backbone RMSD of each replicate to the native-BUILT chain (same ideal bond
    lengths on both sides); C-alpha RMSD to the record's ``coors[ligand_mask]`` with its transform; pairwise C-alpha RMSD
    among the replicates of a pocket, their medoid and mean; each replicate placed in the receptor frame by that
    transform; receptor residues whose C-alpha lies within ``clash_cutoff`` of any placed atom
    (``featurize.contact_residues``).

    THE PLACEMENT USES THE KNOWN POSE: a replicate is superposed on the native ligand's C-alphas and then checked against
    the receptor.  That is evaluation of the sampled conformation, not docking -- nothing here predicts where the peptide
    binds.

    Returns one plain dict per pocket: ``index``, ``structure_ids``, ``ligand_length``, ``backbone_rmsd_to_native_built``
    [R], ``ca_rmsd_to_native`` [R], ``pairwise_ca_rmsd`` [R][R], ``medoid``, ``mean_pairwise_ca_rmsd`` (None for R = 1),
    ``clashes`` [R]; with ``return_placed`` also a list [P][R] of placed float64 coordinates [4 l_i, 3]."""
    if convention not in ("stored", "labelled"):
        raise ValueError(f"convention = {convention!r}: 'stored' or 'labelled'")
    sp = _superpose or superpose
    build = _build or (lambda a, l: _device_build(a, l, device))
    contacts = _contacts or contact_residues
    records = _records_of(dataset)
    n_rep, P = len(replicates), len(replicates[0])
    if n_rep < 1 or P < 1 or any(len(r) != P for r in replicates) or P > len(records):
        raise ValueError("replicates must be a non-empty list of equally long sampler outputs, no longer than the dataset")

    # ---- every chain of the call, padded: per pocket the native angles, then its replicates
    per = 1 + n_rep
    chains, lens = [], []
    for i in range(P):
        lig = records[i]["ligand_mask"]
        native = np.asarray(records[i]["angle_features"][lig], dtype=np.float32)
        chains.append(native)
        for r in range(n_rep):
            a = np.asarray(replicates[r][i], dtype=np.float32)
            a = a[-1] if a.ndim == 3 else a
            if a.shape != native.shape:
                raise ValueError(f"pocket {i}, replicate {r}: angles {a.shape}, the record's ligand has {native.shape}")
            chains.append(a)
        lens.append(native.shape[0])
    L = max(lens)
    batch = np.zeros((P * per, L, 8), dtype=np.float32)
    for c, a in enumerate(chains):
        a = builder_angles_from_stored(a) if convention == "stored" else a
        batch[c, :a.shape[0]] = a
    chain_len = torch.tensor([l for l in lens for _ in range(per)], dtype=torch.int32)
    coords = build(torch.from_numpy(batch), chain_len)                       # [P per, L, 4, 3] float64
    dev = coords.device
    natives = torch.arange(P, device=dev) * per
    reps = (natives[:, None] + 1 + torch.arange(n_rep, device=dev)[None, :]).reshape(-1)      # pocket-major
    rep_len = chain_len.to(dev)[reps]

    # ---- backbone RMSD to the native-built chain
    bb_rmsd = rmsd_to_reference(coords[reps], coords[natives.repeat_interleave(n_rep)], rep_len, "backbone", _superpose=sp)
    # ---- C-alpha RMSD to the record's coordinates, with the transform into the complex frame
    nat_ca = torch.zeros((P, L, 3), dtype=torch.float64)
    for i in range(P):
        nat_ca[i, :lens[i]] = records[i]["coors"][records[i]["ligand_mask"]].double()
    nat_ca = nat_ca.to(dev)
    ca_rmsd, R, t = rmsd_to_reference(coords[reps], nat_ca.repeat_interleave(n_rep, 0), rep_len, "CA", True, _superpose=sp)
    # ---- the ensemble of each pocket
    groups = [list(range(i * n_rep, (i + 1) * n_rep)) for i in range(P)]
    mats = pairwise_rmsd(coords[reps], rep_len, groups, "CA", _superpose=sp)
    # ---- placement in the receptor frame (the KNOWN pose) and clashes with receptor C-alphas
    placed = torch.einsum("cjk,clak->claj", R, coords[reps]) + t[:, None, None, :]
    lig_xyz, lig_off = flatten_by_lengths(placed, rep_len)
    rec_ca = [records[i]["coors"][~records[i]["ligand_mask"]].double() for i in range(P)]
    rec_xyz = torch.cat([rec_ca[i] for i in range(P) for _ in range(n_rep)]).to(dev)
    rec_off = np.cumsum([0] + [rec_ca[i].shape[0] for i in range(P) for _ in range(n_rep)])
    n_rows = int(rec_off[-1])
    hit = contacts(rec_xyz, torch.arange(n_rows, device=dev, dtype=torch.int32),
                   torch.from_numpy(rec_off.astype(np.int32)).to(dev), lig_xyz, lig_off, n_rows, clash_cutoff)
    clashes = np.add.reduceat(hit.cpu().numpy().astype(np.int64), rec_off[:-1]) if n_rows else np.zeros(P * n_rep, np.int64)

    bb_rmsd, ca_rmsd = bb_rmsd.cpu().reshape(P, n_rep), ca_rmsd.cpu().reshape(P, n_rep)
    clashes = clashes.reshape(P, n_rep)
    rows = []
    for i in range(P):
        mat = mats[i].cpu()
        rows.append({
            "index": i, "structure_ids": dict(records[i]["structure_ids"]), "ligand_length": lens[i],
            "backbone_rmsd_to_native_built": bb_rmsd[i].tolist(), "ca_rmsd_to_native": ca_rmsd[i].tolist(),
            "pairwise_ca_rmsd": mat.tolist(), "medoid": medoid(mat),
            "mean_pairwise_ca_rmsd": float(mat.sum() / (n_rep * (n_rep - 1))) if n_rep > 1 else None,
            "clashes": [int(v) for v in clashes[i]],
        })
    if not return_placed:
        return rows
    placed = placed.cpu().numpy()
    return rows, [[placed[i * n_rep + r, :lens[i]].reshape(-1, 3) for r in range(n_rep)] for i in range(P)]


# ------------------------------------------------------------------------------------------------ description without a native
SS_HELIX, SS_STRAND = (0, 3, 4), (1, 2)      # H, G, I and B, E as indices into biolip.SS_VOCAB
DEFAULT_CONTACT_CLASH = 2.5    # Angstrom between backbone atoms of residues at least two apart: a choice, not a standard
GEOMETRY_KEYS = ("ss", "acc_rel", "acc_e", "don_rel", "don_e", "kappa", "clash", "hbonds", "status")


def backbone_geometry(coords, off, is_pro=None, clash_cutoff=DEFAULT_CONTACT_CLASH, max_peptide_bond=2.5):
    """coords [R,4,3] (N, CA, C, O per residue, all structures back to back), off [n_structs+1] (residue offsets,
    off[0] = 0), is_pro [R] (non-zero: a proline, no amide hydrogen) or None -> a dict of device tensors, one row per
    residue: ``ss`` u8 (index into ``biolip.SS_VOCAB``), ``acc_rel`` i32 [R,2] / ``acc_e`` f64 [R,2] (the two best
    acceptors of its N-H, relative index and kcal/mol), ``don_rel`` / ``don_e`` (of its C=O), ``kappa`` f64 (degrees, NaN
    where undefined), ``clash`` i32, ``hbonds`` i32 (acceptors of its N-H with E < -0.5), ``status`` i32 (0 ok, 1 a
    non-finite coordinate, 3 held by no structure with good offsets).  The export itself (csrc/backbone_geometry.hip
    states the rules and the three differences from DSSP); inputs are converted to contiguous float64 / int32 / uint8."""
    tensors = (coords, off) + (() if is_pro is None else (is_pro,))
    _require_cuda("backbone_geometry", *tensors)
    R, n_structs = coords.shape[0], off.shape[0] - 1
    assert tuple(coords.shape) == (R, 4, 3) and off.dim() == 1 and (is_pro is None or tuple(is_pro.shape) == (R,)), \
        (coords.shape, off.shape, None if is_pro is None else is_pro.shape)
    x, o = coords.contiguous().double(), off.to(torch.int32).contiguous()
    pro = None if is_pro is None else (is_pro != 0).to(torch.uint8).contiguous()
    new = lambda shape, dtype: torch.empty(shape, device=x.device, dtype=dtype)  # noqa: E731
    out = {"ss": new((R,), torch.uint8), "acc_rel": new((R, 2), torch.int32), "acc_e": new((R, 2), torch.float64),
           "don_rel": new((R, 2), torch.int32), "don_e": new((R, 2), torch.float64), "kappa": new((R,), torch.float64),
           "clash": new((R,), torch.int32), "hbonds": new((R,), torch.int32), "status": new((R,), torch.int32)}
    hip.check(hip.lib().e3d_backbone_geometry(x.data_ptr(), o.data_ptr(), None if pro is None else pro.data_ptr(),
                                              *(out[k].data_ptr() for k in GEOMETRY_KEYS), n_structs, R,
                                              float(clash_cutoff), float(max_peptide_bond),
                                              torch.cuda.current_stream().cuda_stream), "e3d_backbone_geometry")
    return out


def _last_step(a):
    a = np.asarray(a, dtype=np.float32)
    return a[-1] if a.ndim == 3 else a


def describe_samples(replicates, dataset=None, sequences=None, convention="stored", device="cuda",
                     clash_cutoff=DEFAULT_CONTACT_CLASH, max_peptide_bond=2.5, _build=None, _geometry=None):
    """What R replicates of P pockets ARE, without a native: secondary structure, backbone hydrogen bonds, clashes, size.

    replicates: what ``evaluate_samples`` takes, R lists of P arrays [l_i,8] or [T,l_i,8] (the last step is taken).
    dataset: optional.  With one, item i belongs to its record i (as in ``evaluate_samples``), rows carry
        ``structure_ids``, and the native's own description -- built from ``angle_features[ligand_mask]``, prolines from
        ``amino_acid`` -- is added as ``native``.  Design mode has none: leave it out.
    sequences: optional [R][P] strings, e.g. the sequence sampler's designs; a 'P' marks a proline, which donates no
        hydrogen bond.  A string whose length is not its chain's raises ValueError.
    convention: as in ``evaluate_samples``.
    ONE NeRF launch and ONE ``backbone_geometry`` call serve all chains; the sums per chain and the profile per pocket are
    batched index sums on the device, nothing is launched per chain.

    Returns one plain dict per pocket: ``index``, ``ligand_length``, ``structure_ids`` (with a dataset), and per replicate
    [R]: ``ss`` (a string over ``biolip.SS_VOCAB``), ``helix_fraction`` (H + G + I), ``strand_fraction`` (E + B), ``hbonds``
    (pairs with E < -0.5), ``clashes`` (backbone atom pairs of residues at least two apart closer than ``clash_cutoff``),
    ``radius_of_gyration`` and ``end_to_end`` (C-alpha, Angstrom); ``ss_profile`` [l][8], the frequency of each letter
    over the replicates at each position; ``native``, the same seven entries for the native chain.
    The letters follow csrc/backbone_geometry.hip, which differs from DSSP in three stated ways; agreement with mkdssp
    is not measured, and nothing here says whether a sample is GOOD."""
    if convention not in ("stored", "labelled"):
        raise ValueError(f"convention = {convention!r}: 'stored' or 'labelled'")
    from .biolip import SS_VOCAB
    build = _build or (lambda a, l: _device_build(a, l, device))
    geometry = _geometry or backbone_geometry
    n_rep = len(replicates)
    P = len(replicates[0]) if n_rep else 0
    records = _records_of(dataset) if dataset is not None else None
    if n_rep < 1 or P < 1 or any(len(r) != P for r in replicates) or (records is not None and P > len(records)):
        raise ValueError("replicates must be a non-empty list of equally long sampler outputs, no longer than the dataset")
    if sequences is not None and (len(sequences) != n_rep or any(len(s) != P for s in sequences)):
        raise ValueError(f"sequences must be [{n_rep}][{P}] strings, one per replicate and pocket")

    # ---- every chain of the call: the replicates pocket-major, then the natives
    chains, pro, lens = [], [], []
    for i in range(P):
        lens.append(_last_step(replicates[0][i]).shape[0])
        if lens[i] < 1:
            raise ValueError(f"pocket {i}: an empty chain")
        for r in range(n_rep):
            a = _last_step(replicates[r][i])
            if a.shape != (lens[i], 8):
                raise ValueError(f"pocket {i}, replicate {r}: angles {a.shape}, replicate 0 has {(lens[i], 8)}")
            seq = "" if sequences is None else str(sequences[r][i])
            if sequences is not None and len(seq) != lens[i]:
                raise ValueError(f"pocket {i}, replicate {r}: the chain has {lens[i]} residues, the sequence {len(seq)}")
            chains.append(a)
            pro.append(np.frombuffer(seq.encode(), dtype=np.uint8) == ord("P") if seq else np.zeros(lens[i], dtype=bool))
    for i in range(P if records is not None else 0):
        lig = records[i]["ligand_mask"]
        native = np.asarray(records[i]["angle_features"][lig], dtype=np.float32)
        if native.shape != (lens[i], 8):
            raise ValueError(f"pocket {i}: angles {(lens[i], 8)}, the record's ligand has {native.shape}")
        chains.append(native)
        pro.append(np.array([a == "P" for a, m in zip(records[i]["amino_acid"], lig.tolist()) if m], dtype=bool))
    C, L = len(chains), max(lens)
    batch = np.zeros((C, L, 8), dtype=np.float32)
    for c, a in enumerate(chains):
        batch[c, :a.shape[0]] = a
    if convention == "stored":                  # on the padded batch at once: the entries it misses past a chain's end are
        batch = builder_angles_from_stored(batch)    # zeros either way, and rows past the end stay zero
    chain_len = torch.tensor([l for l in lens for _ in range(n_rep)] + (lens if records is not None else []), dtype=torch.int32)
    coords = build(torch.from_numpy(batch), chain_len)                       # [C, L, 4, 3] float64
    dev = coords.device
    flat, atom_off = flatten_by_lengths(coords, chain_len)
    flat, off = flat.reshape(-1, 4, 3), atom_off // 4
    geo = geometry(flat, off, torch.from_numpy(np.concatenate(pro)).to(dev), clash_cutoff, max_peptide_bond)

    # ---- sums per chain and the profile per pocket: index sums over all residues at once
    lens_d = chain_len.to(dev).long()
    chain_of = torch.repeat_interleave(torch.arange(C, device=dev), lens_d)
    first = off[:-1].long()

    def per_chain(values):
        return torch.zeros((C,) + tuple(values.shape[1:]), device=dev, dtype=torch.float64).index_add_(0, chain_of,
                                                                                                       values.double())
    ss = geo["ss"].long()
    onehot = torch.nn.functional.one_hot(ss, len(SS_VOCAB)).double()
    counts = per_chain(onehot)
    n = lens_d.double()
    ca = flat[:, 1]
    spread = ca - (per_chain(ca) / n[:, None])[chain_of]
    rg = (per_chain((spread * spread).sum(-1)) / n).sqrt()
    ends = (ca[first + lens_d - 1] - ca[first]).norm(dim=-1)
    helix, strand = counts[:, list(SS_HELIX)].sum(-1) / n, counts[:, list(SS_STRAND)].sum(-1) / n
    hbonds, clashes = per_chain(geo["hbonds"]), per_chain(geo["clash"]) / 2
    # position p of pocket i, over its replicates: row pocket_first[i] + p of the profile
    pocket_first = np.cumsum([0] + lens)
    n_sampled = n_rep * int(pocket_first[-1])
    pocket_of = torch.repeat_interleave(torch.arange(P, device=dev), torch.tensor(lens, device=dev) * n_rep)
    start = torch.from_numpy(pocket_first[:-1]).to(dev)
    row = start[pocket_of] + (torch.arange(n_sampled, device=dev) - first[chain_of[:n_sampled]])
    profile = torch.zeros((int(pocket_first[-1]), len(SS_VOCAB)), device=dev, dtype=torch.float64)
    profile = (profile.index_add_(0, row, onehot[:n_sampled]) / n_rep).cpu()

    letters = np.frombuffer(SS_VOCAB.encode(), dtype=np.uint8)[geo["ss"].cpu().numpy()].tobytes().decode()
    starts = off.cpu().tolist()
    cols = {"helix_fraction": helix, "strand_fraction": strand, "hbonds": hbonds, "clashes": clashes,
            "radius_of_gyration": rg, "end_to_end": ends}
    cols = {k: v.cpu().tolist() for k, v in cols.items()}

    def entry(c):
        out = {"ss": letters[starts[c]:starts[c + 1]]}
        for k, v in cols.items():
            out[k] = int(round(v[c])) if k in ("hbonds", "clashes") else float(v[c])
        return out

    rows = []
    for i in range(P):
        per = [entry(i * n_rep + r) for r in range(n_rep)]
        row_i = {"index": i, "ligand_length": lens[i]}
        if records is not None:
            row_i["structure_ids"] = dict(records[i]["structure_ids"])
        row_i.update({k: [e[k] for e in per] for k in per[0]})
        row_i["ss_profile"] = profile[pocket_first[i]:pocket_first[i + 1]].tolist()
        if records is not None:
            row_i["native"] = entry(P * n_rep + i)
        rows.append(row_i)
    return rows
