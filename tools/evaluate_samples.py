#!/usr/bin/env python3
"""Sampled angles -> a report: RMSD to the native, the ensemble of replicates, clashes (evaluate.py, on the GPU).

    python tools/evaluate_samples.py out_seed1.pkl out_seed2.pkl --data biolip.pt -o report.json
    python tools/evaluate_samples.py out_seed*.pkl --data biolip.pt --pdb-dir medoids -o report.json

Each pickle is one replicate: the structure sampler's output for the test pockets of ``--data`` (one seed per replicate).
The dataset is built as the sampler builds it, so item i of a pickle meets its own record.  ``--convention stored``
(default) reads the angle columns as records store them; ``labelled`` feeds them to the backbone builder as
``create_pdb.py`` does.  The placement in the receptor frame uses the native pose: this is evaluation, not docking.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("samples", nargs="+", help="sampler pickles, one per replicate (lists of [T,l,8] or [l,8] arrays)")
    ap.add_argument("--data", required=True, help="the biolip.pt the samples were drawn for")
    ap.add_argument("--convention", choices=("stored", "labelled"), default="stored")
    ap.add_argument("--clash-cutoff", type=float, default=3.0,
                    help="Angstrom between a receptor C-alpha and a placed backbone atom (default 3.0)")
    ap.add_argument("--pdb-dir", default=None, help="write each pocket's medoid, placed in the receptor frame, as a PDB file")
    ap.add_argument("-o", "--output", required=True, help="the JSON report")
    return ap.parse_args(argv)


def summarize(rows, threshold=2.0):
    """Per-pocket rows -> the summary of the report: C-alpha RMSD to the native over all replicates (median), over each
    pocket's best replicate (median), the share of replicates and of pockets' best under ``threshold`` A, mean clashes."""
    every = [v for r in rows for v in r["ca_rmsd_to_native"]]
    best = [min(r["ca_rmsd_to_native"]) for r in rows]
    clashes = [v for r in rows for v in r["clashes"]]
    return {
        "pockets": len(rows), "replicates": len(rows[0]["ca_rmsd_to_native"]),
        "median_ca_rmsd": statistics.median(every), "median_best_of_r_ca_rmsd": statistics.median(best),
        "share_under_2A": sum(v < threshold for v in every) / len(every),
        "share_best_of_r_under_2A": sum(v < threshold for v in best) / len(best),
        "mean_clashes": sum(clashes) / len(clashes),
    }


def main(argv=None):
    args = parse_args(argv)
    import __graft_entry__
    __graft_entry__.load_package()
    from e3diff_amd import evaluate
    from e3diff_amd.structure_model.create_pdb import load_sampled_angles, write_coords_to_pdb
    from e3diff_amd.structure_model.sample import get_dataset
    replicates = [load_sampled_angles(p) for p in args.samples]
    dataset = get_dataset(args.data)
    rows, placed = evaluate.evaluate_samples(replicates, dataset, convention=args.convention,
                                             clash_cutoff=args.clash_cutoff, device="cuda:0", return_placed=True)
    if args.pdb_dir:
        os.makedirs(args.pdb_dir, exist_ok=True)
        for row, chains in zip(rows, placed):
            ids = row["structure_ids"]
            name = f"{row['index']}_{ids.get('pdb_id', '')}_medoid.pdb"
            row["medoid_pdb"] = write_coords_to_pdb(chains[row["medoid"]], os.path.join(args.pdb_dir, name))
    report = {"samples": list(args.samples), "data": args.data, "convention": args.convention,
              "clash_cutoff": args.clash_cutoff, "summary": summarize(rows), "pockets": rows}
    with open(args.output, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report["summary"]))
    print(f"wrote {len(rows)} pocket row(s) to {args.output}")


if __name__ == "__main__":
    main()
