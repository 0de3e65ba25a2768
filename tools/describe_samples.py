#!/usr/bin/env python3
"""Sampled angles -> what the backbones are, without a native: secondary structure, hydrogen bonds, clashes, size
(evaluate.describe_samples, on the GPU).

    python tools/describe_samples.py out_seed1.pkl out_seed2.pkl -o report.json                     # design mode
    python tools/describe_samples.py out_seed*.pkl --data biolip.pt --table output.pkl -o report.json

Each pickle is one replicate: the structure sampler's output, one seed per replicate.  ``--data`` is optional: with it
the rows carry the records' ids and the native ligand's own description (the dataset is built as the sampler builds it,
so item i of a pickle meets its own record).  ``--table`` is the table the sequence sampler's ``run()`` writes; the
prolines of its ``predict_sequence`` column donate no hydrogen bond, in every replicate.  The letters follow Kabsch &
Sander's rules as csrc/backbone_geometry.hip states them -- not the mkdssp program, which they have not been compared
with -- and the report describes the samples; it does not say whether they are good.
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
    ap.add_argument("--data", default=None, help="the biolip.pt the samples were drawn for (optional)")
    ap.add_argument("--table", default=None, help="a table the sequence sampler wrote: its predict_sequence column marks prolines")
    ap.add_argument("--convention", choices=("stored", "labelled"), default="stored")
    ap.add_argument("--clash-cutoff", type=float, default=2.5,
                    help="Angstrom between backbone atoms of residues at least two apart (default 2.5; a choice, not a standard)")
    ap.add_argument("-o", "--output", required=True, help="the JSON report")
    return ap.parse_args(argv)


def table_sequences(table, lengths, ids=None):
    """The ``predict_sequence`` of every pocket, in the pockets' order: rows are met by ``structure_ids`` when ``ids`` (the
    dataset's ``pdbid_chain`` names) are given and the table names each once, else by position.  ValueError for a missing
    column, a missing id, too few rows or a wrong length."""
    for col in ("structure_ids", "predict_sequence"):
        if col not in table.columns:
            raise ValueError(f"the table has no {col!r} column: not a table sample.run() wrote")
    named, seqs = [str(v) for v in table["structure_ids"]], [str(v) for v in table["predict_sequence"]]
    if ids is not None and named[:len(ids)] != list(ids) and len(set(named)) == len(named):
        missing = [i for i in ids if i not in named]
        if missing:
            raise ValueError(f"the table has no sequence for {len(missing)} pocket(s): {', '.join(missing[:5])}")
        seqs = [seqs[named.index(i)] for i in ids]
    if len(seqs) < len(lengths):
        raise ValueError(f"the table has {len(seqs)} rows, the samples {len(lengths)} pockets")
    seqs = seqs[:len(lengths)]
    for i, (s, n) in enumerate(zip(seqs, lengths)):
        if len(s) != n:
            raise ValueError(f"pocket {i}: the sampled chain has {n} residues, the table's sequence {len(s)}")
    return seqs


def summarize(rows):
    """Per-pocket rows -> the summary of the report: means over all replicates of all pockets, and the share of replicates
    without a clash."""
    every = {k: [v for r in rows for v in r[k]] for k in ("helix_fraction", "strand_fraction", "hbonds", "clashes",
                                                            "radius_of_gyration")}
    out = {"pockets": len(rows), "replicates": len(rows[0]["ss"])}
    out.update({f"mean_{k}": statistics.fmean(v) for k, v in every.items()})
    out["share_without_clash"] = sum(v == 0 for v in every["clashes"]) / len(every["clashes"])
    return out


def main(argv=None):
    args = parse_args(argv)
    import __graft_entry__
    __graft_entry__.load_package()
    from e3diff_amd import evaluate
    from e3diff_amd.structure_model.create_pdb import load_sampled_angles
    replicates = [load_sampled_angles(p) for p in args.samples]
    dataset, ids = None, None
    if args.data:
        from e3diff_amd.structure_model.sample import get_dataset
        dataset = get_dataset(args.data)
        records = evaluate._records_of(dataset)[:len(replicates[0])]
        ids = [f'{r["structure_ids"]["pdb_id"]}_{r["structure_ids"]["ligand_chain"]}' for r in records]
    sequences = None
    if args.table:
        import pandas as pd
        one = table_sequences(pd.read_pickle(args.table), [a.shape[0] for a in replicates[0]], ids)
        sequences = [one] * len(replicates)
    rows = evaluate.describe_samples(replicates, dataset, sequences, convention=args.convention, device="cuda:0",
                                     clash_cutoff=args.clash_cutoff)
    report = {"samples": list(args.samples), "data": args.data, "table": args.table, "convention": args.convention,
              "clash_cutoff": args.clash_cutoff, "summary": summarize(rows), "pockets": rows}
    with open(args.output, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report["summary"]))
    print(f"wrote {len(rows)} pocket row(s) to {args.output}")


if __name__ == "__main__":
    main()
