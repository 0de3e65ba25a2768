#!/usr/bin/env python3
"""PDB files -> biolip.pt (featurize.py: backbone angles and pocket on the GPU), the input of every train / sample script.

    python tools/featurize_pdb.py complex.pdb --receptor A --ligand B -o biolip.pt        # pocket by contact with chain B
    python tools/featurize_pdb.py target.pdb --receptor A --pocket 45,46,52A --ligand-length 12 -o biolip.pt   # design mode

Several input files give one record each, all in one output file.
The same chain ids and pocket apply to every input.  PDB format only (no mmCIF).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_pocket(text):
    """'45,46,52A' -> [(45, ''), (46, ''), (52, 'A')]"""
    out = []
    for item in text.split(","):
        item = item.strip()
        digits = item.rstrip("ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz")
        out.append((int(digits), item[len(digits):]))
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("pdb", nargs="+", help="PDB files (first MODEL, ATOM records)")
    ap.add_argument("--receptor", required=True, help="receptor chain id")
    ap.add_argument("--ligand", default=None, help="ligand chain id; without it: --pocket and --ligand-length (design mode)")
    ap.add_argument("--pocket", type=parse_pocket, default=None,
                    help="pocket residues as resseq[icode],... ; default: receptor residues in contact with the ligand chain")
    ap.add_argument("--ligand-length", type=int, default=None, help="design mode: residues of the ligand to be sampled")
    ap.add_argument("--cutoff", type=float, default=4.0, help="contact cutoff between heavy atoms in Angstrom (default 4.0)")
    ap.add_argument("--named-pocket", action="store_true",
                    help="mark the pocket residues actually named (default: the reference's shift by one residue, which the "
                         "published checkpoints were trained on; featurize.py)")
    ap.add_argument("--dssp", action="store_true",
                    help="fill secondary_structure from the backbone (featurize.py: Kabsch & Sander's rules on the GPU, not "
                         "the mkdssp program; default: all '-')")
    ap.add_argument("-o", "--output", required=True)
    args = ap.parse_args(argv)
    if args.ligand is None and (args.pocket is None or args.ligand_length is None):
        ap.error("without --ligand both --pocket and --ligand-length are required")
    return args


def jobs_from_args(args):
    return [{"path": p, "receptor": args.receptor, "ligand": args.ligand, "pocket": args.pocket,
             "ligand_length": args.ligand_length} for p in args.pdb]


def main(argv=None):
    args = parse_args(argv)
    import __graft_entry__
    __graft_entry__.load_package()
    from e3diff_amd import featurize
    records = featurize.records_from_pdb_files(jobs_from_args(args), "cuda:0", cutoff=args.cutoff,
                                               reference_pocket_shift=not args.named_pocket, secondary_structure=args.dssp)
    featurize.write(args.output, records)
    for r in records:
        n_lig, n_poc = int(r["ligand_mask"].sum()), int(r["pocket_mask"].sum())
        print(f"{r['structure_ids']}: {len(r['amino_acid']) - n_lig} receptor + {n_lig} ligand residues, {n_poc} in the pocket")
    print(f"wrote {len(records)} record(s) to {args.output}")


if __name__ == "__main__":
    main()
