"""PDB files -> ``biolip.pt`` records: the entry of the pipeline that ``create_pdb.py`` leaves.

The reference's producer (clean_data/data_preprocessing.py) needs Biopython, a DSSP binary and the BioLiP downloads.
The models read four things of a record -- ``angle_features``, ``amino_acid``, ``ligand_mask``, ``pocket_mask`` -- and
those need only the backbone coordinates, eight internal angles per residue and a pocket definition.  This module
builds schema-valid records (``biolip.validate_record``) from PDB files with two HIP kernels (csrc/backbone_angles.hip):

    e3d_backbone_angles    N, CA, C, O of all chains of all files -> the eight stored angles (one launch)
    e3d_contact_residues   receptor residues with a heavy atom within ``cutoff`` of a ligand heavy atom (one launch)

What a record built here does NOT carry: DSSP's ``secondary_structure`` (all '-') and ``numerical_features`` (zeros);
no dataset or model of this package reads them.  ``secondary_structure=True`` fills the first from the backbone with
``evaluate.backbone_geometry`` (csrc/backbone_geometry.hip: Kabsch & Sander's rules, three stated differences from DSSP).

The pocket by contact is a CHOICE, not BioLiP's rule: BioLiP's binding-site annotation uses van-der-Waals radii;
here a receptor residue is in the pocket when any of its heavy atoms lies within ``cutoff`` (default 4.0 Angstrom) of
any heavy atom of the ligand chain.  Pass ``pocket=[(resseq, icode), ...]`` to use an annotation instead.

``reference_pocket_shift``: the reference finds ``pocket_idx`` as positions in the UNTRIMMED receptor chain
(data_preprocessing.py:802-820 enumerate ``features[receptor_chain_id]``, all residues) but ``create_data``
(:838-893) applies them to arrays built from ``receptor[1:-1]``.  Position p of the untrimmed chain is position p - 1 of
the trimmed one, so every record the published checkpoints were trained on marks the residue AFTER each annotated
one.  ``True`` (default) reproduces that, for checkpoint compatibility; ``False`` marks the residues actually named.
Positions that fall outside the trimmed receptor either way (the reference would mark a ligand residue or fail) are
dropped with a warning.
"""
import os
import warnings
from collections import namedtuple

import numpy as np
import torch

from . import biolip, hip

DEFAULT_CUTOFF = 4.0        # Angstrom between heavy atoms: a documented choice (see the module docstring)
MAX_PEPTIDE_BOND = 2.0      # Angstrom: a C - N distance above this is reported as a chain break (1.33 in a peptide bond)
MIN_LIGAND_LENGTH = 5       # res_to_dataset (data_preprocessing.py:905) keeps complexes whose ligand has >= 5 residues
STATUS_NOT_INTERIOR, STATUS_DEGENERATE, STATUS_CHAIN_BREAK = 1, 2, 4

THREE_TO_ONE = {"ALA": "A", "CYS": "C", "ASP": "D", "GLU": "E", "PHE": "F", "GLY": "G", "HIS": "H", "ILE": "I", "LYS": "K",
                "LEU": "L", "MET": "M", "ASN": "N", "PRO": "P", "GLN": "Q", "ARG": "R", "SER": "S", "THR": "T", "VAL": "V",
                "TRP": "W", "TYR": "Y"}
_BACKBONE = ("N", "CA", "C", "O")

Chain = namedtuple("Chain", "chain_id resseq icode resname seq backbone atoms atom_res")
Chain.__doc__ = """One parsed chain: ``resseq`` list[int], ``icode`` list[str] ('' = none), ``resname`` list[str] (three-letter),
``seq`` str (one-letter), ``backbone`` f32 [n,4,3] (N, CA, C, O), ``atoms`` f32 [m,3] all heavy atoms in file order,
``atom_res`` i32 [m] the residue index (0 .. n-1) of each heavy atom."""


def _residue_label(chain_id, resseq, icode, resname=None):
    return f"{resname + ' ' if resname else ''}{chain_id}{resseq}{icode}"


def _is_hydrogen(name, element):
    if element:
        return element in ("H", "D")
    stripped = name.strip().lstrip("0123456789")
    return stripped[:1] in ("H", "D")


def read_pdb(path_or_text, chains=None):
    """Fixed-column parser of the ``ATOM`` records of the first ``MODEL`` of a PDB file (a path, or the text itself when
    it holds a newline).  Returns ``{chain_id: Chain}`` in file order, restricted to ``chains`` when given.

    ``HETATM`` records (waters, ions, modified residues) and hydrogens are dropped.  Alternate locations: the blank one,
    or the first one seen per atom, is kept.  A residue of a kept chain that lacks one of N, CA, C, O, or whose name is
    outside the 20 standard ones, raises a ``ValueError`` that names it (the reference drops whole complexes with an
    ``X`` residue).  mmCIF is NOT read: convert to PDB format first."""
    text = path_or_text
    if "\n" not in text:
        with open(text) as f:
            text = f.read()
    wanted = None if chains is None else set(chains)
    order, residues = [], {}        # chain ids in file order; chain -> list of [resseq, icode, resname, {atom: xyz}, [atoms]]
    for line in text.splitlines():
        rec = line[:6]
        if rec == "ENDMDL":
            break
        if rec != "ATOM  ":
            continue
        chain_id = line[21]
        if wanted is not None and chain_id not in wanted:
            continue
        name, resname, icode = line[12:16].strip(), line[17:20].strip(), line[26].strip()
        if _is_hydrogen(line[12:16], line[76:78].strip().upper()):
            continue
        resseq = int(line[22:26])
        xyz = (float(line[30:38]), float(line[38:46]), float(line[46:54]))
        if chain_id not in residues:
            residues[chain_id] = []
            order.append(chain_id)
        res = residues[chain_id]
        if not res or (res[-1][0], res[-1][1]) != (resseq, icode):
            res.append([resseq, icode, resname, {}, []])
        seen = res[-1][3]
        if name in seen:                # a second alternate location of this atom
            continue
        seen[name] = xyz
        res[-1][4].append(xyz)
    if wanted is not None and wanted - set(order):
        raise ValueError(f"chain(s) {sorted(wanted - set(order))} have no ATOM records (found {order})")
    out = {}
    for chain_id in order:
        res = residues[chain_id]
        backbone = np.empty((len(res), 4, 3), dtype=np.float32)
        atoms, atom_res = [], []
        for i, (resseq, icode, resname, seen, heavy) in enumerate(res):
            label = _residue_label(chain_id, resseq, icode, resname)
            if resname not in THREE_TO_ONE:
                raise ValueError(f"residue {label}: not one of the 20 standard amino acids")
            missing = [a for a in _BACKBONE if a not in seen]
            if missing:
                raise ValueError(f"residue {label}: backbone atom(s) {missing} missing")
            backbone[i] = [seen[a] for a in _BACKBONE]
            atoms.extend(heavy)
            atom_res.extend([i] * len(heavy))
        out[chain_id] = Chain(chain_id, [r[0] for r in res], [r[1] for r in res], [r[2] for r in res],
                              "".join(THREE_TO_ONE[r[2]] for r in res), backbone,
                              np.asarray(atoms, dtype=np.float32).reshape(-1, 3), np.asarray(atom_res, dtype=np.int32))
    return out


# ------------------------------------------------------------------------------------------------ kernels
def _require_cuda(what, *tensors):
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"{what} runs on the HIP kernel only: pass GPU tensors (no CPU fallback)")


def backbone_angles(coords, seg, max_peptide_bond=MAX_PEPTIDE_BOND):
    """coords [R,4,3] (N, CA, C, O per residue row; chains back to back), seg [R] (chain of a row) -> (angles f32 [R,8] in
    ``biolip.STORED_ANGLE_COLUMNS`` order, status i32 [R]).  Rows whose two neighbours are not of their chain get zeros and
    STATUS_NOT_INTERIOR; STATUS_DEGENERATE (zeros) and STATUS_CHAIN_BREAK (angles kept) as csrc/backbone_angles.hip says."""
    _require_cuda("backbone_angles", coords, seg)
    R = coords.shape[0]
    assert tuple(coords.shape) == (R, 4, 3) and tuple(seg.shape) == (R,), (coords.shape, seg.shape)
    xyz = coords.contiguous().float()
    sg = seg.to(torch.int32).contiguous()
    angles = torch.empty((R, 8), device=xyz.device, dtype=torch.float32)
    status = torch.empty((R,), device=xyz.device, dtype=torch.int32)
    hip.check(hip.lib().e3d_backbone_angles(xyz.data_ptr(), sg.data_ptr(), angles.data_ptr(), status.data_ptr(), R,
                                            float(max_peptide_bond), torch.cuda.current_stream().cuda_stream),
              "e3d_backbone_angles")
    return angles, status


def contact_residues(rec_xyz, rec_row, rec_off, lig_xyz, lig_off, n_rows, cutoff=DEFAULT_CUTOFF):
    """hit i32 [n_rows]: 1 where a receptor residue row has an atom within ``cutoff`` of a ligand atom of the same complex.
    rec_xyz [n,3] / lig_xyz [m,3]: atoms of complex c at rec_off[c]:rec_off[c+1] / lig_off[c]:lig_off[c+1] (int [C+1]);
    rec_row [n]: the residue row of each receptor atom.  m == 0: all zeros."""
    _require_cuda("contact_residues", rec_xyz, rec_row, rec_off, lig_xyz, lig_off)
    n, m, C = rec_xyz.shape[0], lig_xyz.shape[0], rec_off.shape[0] - 1
    assert tuple(rec_xyz.shape) == (n, 3) and tuple(lig_xyz.shape) == (m, 3) and tuple(rec_row.shape) == (n,), \
        (rec_xyz.shape, lig_xyz.shape, rec_row.shape)
    assert tuple(lig_off.shape) == (C + 1,), (rec_off.shape, lig_off.shape)
    rx, lx = rec_xyz.contiguous().float(), lig_xyz.contiguous().float()
    rr, ro, lo = (t.to(torch.int32).contiguous() for t in (rec_row, rec_off, lig_off))
    hit = torch.empty((n_rows,), device=rx.device, dtype=torch.int32)
    hip.check(hip.lib().e3d_contact_residues(rx.data_ptr(), rr.data_ptr(), ro.data_ptr(), lx.data_ptr() if m else None,
                                             lo.data_ptr(), hit.data_ptr(), C, n, m, int(n_rows), float(cutoff),
                                             torch.cuda.current_stream().cuda_stream), "e3d_contact_residues")
    return hit


# ------------------------------------------------------------------------------------------------ record assembly
def _pocket_positions(receptor, pocket):
    """(resseq, icode) pairs -> positions in the untrimmed receptor chain."""
    index = {(s, i): p for p, (s, i) in enumerate(zip(receptor.resseq, receptor.icode))}
    out = []
    for resseq, icode in pocket:
        key = (int(resseq), str(icode).strip())
        if key not in index:
            raise ValueError(f"pocket residue {_residue_label(receptor.chain_id, *key)} is not in chain {receptor.chain_id}")
        out.append(index[key])
    return out


def _check_rows(chain, status):
    """status of the UNTRIMMED chain's rows -> raise on degenerate kept rows, warn on chain breaks."""
    status = np.asarray(status).reshape(-1)
    assert status.shape[0] == len(chain.seq), (status.shape, len(chain.seq))
    for i in range(1, len(chain.seq) - 1):
        label = _residue_label(chain.chain_id, chain.resseq[i], chain.icode[i], chain.resname[i])
        if status[i] & STATUS_DEGENERATE:
            raise ValueError(f"residue {label}: a zero-length bond or collinear backbone atoms, its angles are undefined")
        if status[i] & STATUS_CHAIN_BREAK:
            warnings.warn(f"residue {label}: peptide bond to a neighbour longer than the chain-break threshold; "
                          "the angles are computed across the gap, as the reference does")


def _assemble(receptor, ligand, rec_angles, lig_angles, positions, ligand_length, reference_pocket_shift, pdb_id):
    """The layout of create_data (data_preprocessing.py:838-893) from untrimmed chains, their [n,8] angles and the
    pocket's positions in the untrimmed receptor."""
    if len(receptor.seq) < 3:
        raise ValueError(f"receptor chain {receptor.chain_id}: {len(receptor.seq)} residues, nothing is left after "
                         "dropping the first and the last")
    n_rec = len(receptor.seq) - 2
    rec_angles = torch.as_tensor(rec_angles, dtype=torch.float32).cpu()
    assert tuple(rec_angles.shape) == (n_rec + 2, 8), rec_angles.shape
    if ligand is not None:
        n_lig = len(ligand.seq) - 2
        if n_lig < MIN_LIGAND_LENGTH:
            raise ValueError(f"ligand chain {ligand.chain_id}: {max(n_lig, 0)} residues after dropping the first and the "
                             f"last, fewer than {MIN_LIGAND_LENGTH}")
        lig_angles = torch.as_tensor(lig_angles, dtype=torch.float32).cpu()
        assert tuple(lig_angles.shape) == (n_lig + 2, 8), lig_angles.shape
        lig_seq, lig_ca, lig_ang = ligand.seq[1:-1], torch.from_numpy(ligand.backbone[1:-1, 1].copy()), lig_angles[1:-1]
    else:
        if ligand_length is None or int(ligand_length) < 1:
            raise ValueError("without a ligand chain (design mode) ligand_length >= 1 is required")
        n_lig = int(ligand_length)     # placeholders: sampling reads only the ligand's length
        lig_seq, lig_ca, lig_ang = "G" * n_lig, torch.zeros(n_lig, 3), torch.zeros(n_lig, 8)
    N = n_rec + n_lig
    shift = 0 if reference_pocket_shift else -1
    kept, dropped = set(), []
    for p in positions:
        (kept.add(p + shift) if 0 <= p + shift < n_rec else dropped.append(p))
    if dropped:
        names = [_residue_label(receptor.chain_id, receptor.resseq[p], receptor.icode[p]) for p in dropped]
        warnings.warn(f"pocket residue(s) {names} fall outside the trimmed receptor "
                      f"(reference_pocket_shift={reference_pocket_shift}) and are dropped")
    pocket_idx = torch.tensor(sorted(kept), dtype=torch.int)
    ligand_idx = torch.arange(n_rec, N, dtype=torch.int)
    pocket_mask = torch.zeros(N, dtype=torch.bool)
    pocket_mask[pocket_idx.long()] = True
    ligand_mask = torch.zeros(N, dtype=torch.bool)
    ligand_mask[n_rec:] = True
    return {
        "structure_ids": {"pdb_id": pdb_id, "receptor_chain": receptor.chain_id,
                          "ligand_chain": ligand.chain_id if ligand is not None else ""},
        "coors": torch.cat([torch.from_numpy(receptor.backbone[1:-1, 1].copy()), lig_ca]).float(),
        "amino_acid": list(receptor.seq[1:-1] + lig_seq),
        "secondary_structure": ["-"] * N,
        "numerical_features": torch.zeros(N, 5),
        "angle_features": torch.cat([rec_angles[1:-1], lig_ang]).contiguous(),
        "edge_index": torch.cartesian_prod(ligand_idx.long(), pocket_idx.long()).reshape(-1, 2).T.contiguous(),
        "ligand_mask": ligand_mask, "ligand_idx": ligand_idx,
        "pocket_mask": pocket_mask, "pocket_idx": pocket_idx,
    }


def _chain_rows(chains):
    """chains -> (coords f32 [R,4,3], seg i32 [R]) with one seg id per chain."""
    coords = np.concatenate([c.backbone for c in chains]).astype(np.float32, copy=False)
    seg = np.concatenate([np.full(len(c.seq), i, dtype=np.int32) for i, c in enumerate(chains)])
    return coords, seg


def _contact_inputs(pairs):
    """[(receptor, ligand)] -> the flat arrays of e3d_contact_residues and each receptor's first row."""
    rec_xyz = np.concatenate([r.atoms for r, _ in pairs])
    lig_xyz = np.concatenate([l.atoms for _, l in pairs])
    row0 = np.cumsum([0] + [len(r.seq) for r, _ in pairs])
    rec_row = np.concatenate([r.atom_res + row0[i] for i, (r, _) in enumerate(pairs)]).astype(np.int32)
    rec_off = np.cumsum([0] + [len(r.atoms) for r, _ in pairs]).astype(np.int32)
    lig_off = np.cumsum([0] + [len(l.atoms) for _, l in pairs]).astype(np.int32)
    return rec_xyz, rec_row, rec_off, lig_xyz, lig_off, row0


def _device_angles(chains, device, max_peptide_bond):
    coords, seg = _chain_rows(chains)
    ang, st = backbone_angles(torch.from_numpy(coords).to(device), torch.from_numpy(seg).to(device), max_peptide_bond)
    ang, st = ang.cpu(), st.cpu().numpy()
    bounds = np.cumsum([0] + [len(c.seq) for c in chains])
    return [(ang[a:b], st[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]


def _device_contacts(pairs, device, cutoff):
    rec_xyz, rec_row, rec_off, lig_xyz, lig_off, row0 = _contact_inputs(pairs)
    hit = contact_residues(*(torch.from_numpy(a).to(device) for a in (rec_xyz, rec_row, rec_off, lig_xyz, lig_off)),
                           n_rows=int(row0[-1]), cutoff=cutoff).cpu().numpy()
    return [np.nonzero(hit[a:b])[0].tolist() for a, b in zip(row0[:-1], row0[1:])]


def _device_secondary_structure(complexes, records, device):
    """Fill ``secondary_structure`` of each record from the backbone of its own rows: ONE ``evaluate.backbone_geometry``
    call over all complexes, each complex one structure -- the receptor's kept rows, then the ligand's, as the record lays
    them out.  Chain ends and gaps are found by the kernel's peptide-bond test, so bridges between the two chains count;
    prolines come from the residue names.  Design-mode placeholders have no coordinates and keep '-'."""
    from .evaluate import backbone_geometry           # evaluate imports this module
    rows = [np.concatenate([c.backbone[1:-1] for c in pair if c is not None]).astype(np.float64) for pair in complexes]
    pro = np.concatenate([np.array([ch == "P" for c in pair if c is not None for ch in c.seq[1:-1]], dtype=np.uint8)
                          for pair in complexes])
    off = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    ss = backbone_geometry(*(torch.from_numpy(a).to(device) for a in (np.concatenate(rows), off, pro)))["ss"].cpu().tolist()
    for rec, a, b in zip(records, off[:-1], off[1:]):
        rec["secondary_structure"][:b - a] = [biolip.SS_VOCAB[v] for v in ss[a:b]]


def record_from_chains(receptor, ligand=None, *, pocket=None, cutoff=DEFAULT_CUTOFF, ligand_length=None,
                       reference_pocket_shift=True, angles=None, status=None, pdb_id="", device="cuda",
                       max_peptide_bond=MAX_PEPTIDE_BOND, secondary_structure=False):
    """One schema-valid BioLiP record from parsed chains, laid out as the reference's ``create_data`` does: the first and
    last residue of each chain dropped, receptor first then ligand, ``coors`` = C-alpha, ``secondary_structure`` all '-',
    ``numerical_features`` zeros, ``angle_features`` in stored column order, ``edge_index`` = ligand x pocket int64 [2,E].

    pocket: a list of ``(resseq, icode)`` naming receptor residues, or None = by contact with the ligand chain
        (heavy atoms within ``cutoff``; see the module docstring).
    reference_pocket_shift: True (default) marks the residue AFTER each pocket residue, as every record the published
        checkpoints were trained on does (the reference indexes the untrimmed chain and applies the positions to the
        trimmed one; module docstring); False marks the residues actually named.
    ligand=None (design mode): ``ligand_length`` placeholder residues 'G' with zero angles and coordinates stand for the
        ligand -- sampling reads only its length -- and ``pocket`` must be given.
    angles: ``(receptor_angles [n,8], ligand_angles [m,8] or None)`` for the UNTRIMMED chains in stored column order,
        instead of the kernel's (``status``: the matching status arrays, optional); with an explicit ``pocket`` no GPU is
        touched.
    secondary_structure: False (default) leaves ``secondary_structure`` all '-', as before.  True fills it with the
        letters of csrc/backbone_geometry.hip (Kabsch & Sander's rules with three stated differences from DSSP; not
        compared with mkdssp), the whole complex being one structure; ``numerical_features`` stays zeros either way
        (relative accessibility needs side chains).  Needs the GPU.
    Raises ValueError for a ligand shorter than 5 residues after trimming (not in design mode) and for a kept residue whose
    angles are undefined (status bit 1); warns for a chain break (status bit 2)."""
    if ligand is None and pocket is None:
        raise ValueError("without a ligand chain (design mode) the pocket must be given explicitly")
    chains = [receptor] + ([ligand] if ligand is not None else [])
    if angles is None:
        per_chain = _device_angles(chains, device, max_peptide_bond)
    else:
        status = status if status is not None else [None] * len(chains)
        per_chain = list(zip(angles, status))
    for chain, (_, st) in zip(chains, per_chain):
        if st is not None:
            _check_rows(chain, st)
    if pocket is not None:
        positions = _pocket_positions(receptor, pocket)
    else:
        positions = _device_contacts([(receptor, ligand)], device, cutoff)[0]
    rec = _assemble(receptor, ligand, per_chain[0][0], per_chain[1][0] if ligand is not None else None, positions,
                    ligand_length, reference_pocket_shift, pdb_id)
    if secondary_structure:
        _device_secondary_structure([(receptor, ligand)], [rec], device)
    biolip.validate_record(rec)
    return rec


def records_from_pdb_files(jobs, device="cuda", *, cutoff=DEFAULT_CUTOFF, reference_pocket_shift=True,
                           max_peptide_bond=MAX_PEPTIDE_BOND, secondary_structure=False):
    """Featurize many files with ONE angle launch and ONE contact launch over all chains of all files; with
    ``secondary_structure`` one more call assigns every record's letters (``record_from_chains``).

    jobs: dicts with ``path`` (or PDB text), ``receptor`` (chain id) and either ``ligand`` (chain id) or ``ligand_length``
    plus ``pocket``; optional ``pocket`` (list of (resseq, icode)) with a ligand too, and ``pdb_id`` (default: the file's
    base name).  Returns one record per job, in order."""
    parsed = []
    for job in jobs:
        ids = [job["receptor"]] + ([job["ligand"]] if job.get("ligand") is not None else [])
        chains = read_pdb(job["path"], chains=ids)
        receptor, ligand = chains[ids[0]], (chains[ids[1]] if len(ids) == 2 else None)
        if ligand is None and job.get("pocket") is None:
            raise ValueError("without a ligand chain (design mode) the pocket must be given explicitly")
        pdb_id = job.get("pdb_id")
        if pdb_id is None:
            pdb_id = "" if "\n" in job["path"] else os.path.splitext(os.path.basename(job["path"]))[0]
        parsed.append((job, receptor, ligand, pdb_id))
    flat = [c for _, r, l, _ in parsed for c in ((r, l) if l is not None else (r,))]
    per_chain = iter(_device_angles(flat, device, max_peptide_bond))
    need = [i for i, (job, _, l, _) in enumerate(parsed) if l is not None and job.get("pocket") is None]
    contacts = dict(zip(need, _device_contacts([parsed[i][1:3] for i in need], device, cutoff))) if need else {}
    records = []
    for i, (job, receptor, ligand, pdb_id) in enumerate(parsed):
        rec_ang, rec_st = next(per_chain)
        _check_rows(receptor, rec_st)
        lig_ang = None
        if ligand is not None:
            lig_ang, lig_st = next(per_chain)
            _check_rows(ligand, lig_st)
        positions = contacts[i] if i in contacts else _pocket_positions(receptor, job["pocket"])
        rec = _assemble(receptor, ligand, rec_ang, lig_ang, positions, job.get("ligand_length"), reference_pocket_shift,
                        pdb_id)
        records.append(rec)
    if secondary_structure:
        _device_secondary_structure([p[1:3] for p in parsed], records, device)
    for i, rec in enumerate(records):
        biolip.validate_record(rec, i)
    return records


def write(path, records):
    """Validate, then ``torch.save`` the list (what ``biolip.load`` and every dataset of this package read)."""
    records = list(records)
    biolip.validate(records)
    torch.save(records, path)
    return path
