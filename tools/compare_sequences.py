"""Compare designed sequences with the training set and with one another: novelty and diversity.

    python tools/compare_sequences.py --table output.pkl --data biolip.pt [--split-file splits.json] [--split train]
                                      [--group-by structure_ids] -o report.json
    python tools/compare_sequences.py --fasta designs.fa --data biolip.pt -o report.pkl

--table is a table the sequence sampler wrote (its ``predict_sequence`` column), --fasta the alternative.  With --data,
every design gets ``nearest_identity`` (matches of the best local alignment / the shorter length, to the most identical
ligand of the chosen split of --data), ``nearest_index`` (that ligand's place in the split), ``nearest_key`` (its
"pdb_id:receptor_chain:ligand_chain") and ``novelty`` = 1 - nearest_identity.  With --group-by, designs that share the
column's value (the replicates of a pocket) form a group with its mean pairwise identity, diversity = 1 - that, distinct
strings and the largest set of identical ones.  A .pkl output is the table with the new columns (groups in
``.attrs["diversity"]``); a .json output is {"rows": [...], "diversity": [...]}.
Identity is about letters only; nothing here says whether a design binds, and what a trained model reaches is unknown."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def output_path(text):
    if not text.endswith((".json", ".pkl")):
        raise argparse.ArgumentTypeError(f"the output must end in .json or .pkl, got {text!r}")
    return text


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--table", help="a table the sequence sampler wrote: its predict_sequence column is compared")
    src.add_argument("--fasta", help="a FASTA file of designs; the header's first word becomes structure_ids")
    ap.add_argument("--data", help="the biolip.pt whose ligands are the training set for novelty")
    ap.add_argument("--split-file", help="a split file of tools/split_dataset.py (default: the random 80/10/10)")
    ap.add_argument("--split", choices=("train", "validation", "test", "all"), default="train",
                    help="the records of --data to compare with (default train)")
    ap.add_argument("--group-by", default=None, help="column whose equal values form a diversity group, e.g. structure_ids")
    ap.add_argument("--block", type=int, default=1024, help="sequences per side of one launch (default 1024)")
    ap.add_argument("-o", "--output", required=True, type=output_path, help="report.json or report.pkl")
    args = ap.parse_args(argv)
    if args.split_file and not args.data:
        ap.error("--split-file needs --data")
    if not args.data and not args.group_by:
        ap.error("nothing to do: give --data (novelty), --group-by (diversity) or both")
    return args


def read_fasta(path):
    """[(id, sequence)]: the id is the header's first word, the sequence its lines joined, upper case."""
    records, name, lines = [], None, []
    with open(path) as f:
        for n, raw in enumerate(f, 1):
            line = raw.strip()
            if not line:
                continue
            if line.startswith(">"):
                if name is not None:
                    records.append((name, "".join(lines).upper()))
                if not line[1:].split():
                    raise ValueError(f"{path}:{n}: a header without an id")
                name, lines = line[1:].split()[0], []
            elif name is None:
                raise ValueError(f"{path}:{n}: sequence text before the first '>' header")
            else:
                lines.append(line)
    if name is not None:
        records.append((name, "".join(lines).upper()))
    if not records:
        raise ValueError(f"{path}: no FASTA record")
    return records


def groups_of(values):
    """[(value, [row indices])] in the order of first appearance."""
    where = {}
    for i, v in enumerate(values):
        where.setdefault(str(v), []).append(i)
    return list(where.items())


def check_designs(designs, names, source, vocab, max_len):
    """ValueError naming the row for a design that the alignment cannot take."""
    for i, (s, name) in enumerate(zip(designs, names)):
        bad = sorted(set(s) - set(vocab))
        if not s or bad or len(s) > max_len:
            why = "is empty" if not s else f"holds {''.join(bad)!r}, outside {vocab}" if bad else f"has {len(s)} residues, the limit is {max_len}"
            raise ValueError(f"{source}: the design of row {i} ({name}) {why}")


def compare(designs, training=None, training_keys=None, group_values=None, similarity=None, **kw):
    """(per-design columns, per-group rows) -- the arithmetic of the tool, apart from its files."""
    cols, div = {}, []
    if training is not None:
        near = similarity.nearest(designs, training, **kw)
        index = [int(i) for i in near["index"]]
        cols = {"nearest_identity": [float(v) for v in near["identity"]], "nearest_index": index,
                "nearest_key": [training_keys[i] if i >= 0 else None for i in index],
                "novelty": [1.0 - float(v) for v in near["identity"]]}
    if group_values is not None:
        groups = groups_of(group_values)
        rows = similarity.diversity([[designs[i] for i in members] for _, members in groups])
        div = [dict(group=value, rows=members, **row) for (value, members), row in zip(groups, rows)]
    return cols, div


def main(argv=None):
    args = parse_args(argv)
    import pandas as pd
    import __graft_entry__
    __graft_entry__.load_package()
    from e3diff_amd import similarity
    from e3diff_amd.structure_model.dataset import LigandBindingSiteDataset, split_key
    if args.table:
        table = pd.read_pickle(args.table)
        if "predict_sequence" not in table.columns:
            raise ValueError(f"{args.table} has no 'predict_sequence' column: not a table the sequence sampler wrote")
    else:
        fasta = read_fasta(args.fasta)
        table = pd.DataFrame({"structure_ids": [i for i, _ in fasta], "predict_sequence": [s for _, s in fasta]})
    if args.group_by and args.group_by not in table.columns:
        raise ValueError(f"the designs have no {args.group_by!r} column to group by")
    designs = [str(s) for s in table["predict_sequence"]]
    names = list(table["structure_ids"]) if "structure_ids" in table.columns else list(range(len(designs)))
    check_designs(designs, names, args.table or args.fasta, similarity.AA_VOCAB, similarity.MAX_LEN)
    training = keys = None
    if args.data:
        ds = LigandBindingSiteDataset(args.data, None if args.split == "all" else args.split, max_len=1 << 30,
                                      split_file=args.split_file)
        training = ["".join(similarity.AA_VOCAB[int(j)] for j in d["amino_acid"][d["ligand_mask"]].argmax(dim=-1)) for d in ds.data]
        keys = [split_key(d) for d in ds.data]
    cols, div = compare(designs, training, keys, None if not args.group_by else list(table[args.group_by]), similarity,
                        block=args.block)
    res = table.copy()
    for k, v in cols.items():
        res[k] = v
    if args.output.endswith(".pkl"):
        res.attrs["diversity"] = div
        res.to_pickle(args.output)
    else:
        rows = [{k: (None if isinstance(v, float) and v != v else v) for k, v in row.items()}
                for row in res.to_dict(orient="records")]
        with open(args.output, "w") as f:
            json.dump({"rows": rows, "diversity": div}, f, indent=1)
    print(res)
    for g in div:
        print({k: v for k, v in g.items() if k != "rows"})
    print(f"wrote {len(res)} row(s) and {len(div)} group(s) to {args.output}")
    return res, div


if __name__ == "__main__":
    main()
