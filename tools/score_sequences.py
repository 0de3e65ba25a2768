#!/usr/bin/env python3
"""Score peptide sequences under the sequence diffusion model (sequence_model/sample.py::score_sequences, on the GPU).

    python tools/score_sequences.py --data biolip.pt --model seq.ckpt --table output.pkl --seeds 1,2,3 -o scores.pkl
    python tools/score_sequences.py --data biolip.pt --model seq.ckpt --fasta designs.fa --levels 5 -o scores.json
    python tools/score_sequences.py --data biolip.pt --model seq.ckpt --native -o native.json

The sequences come from one of: ``--table``, the pickle ``sample.run()`` writes (its ``predict_sequence`` column, met
with the records by ``structure_ids``); ``--fasta``, one record per ligand whose header's first word is the structure id
(``<pdb_id>_<ligand_chain>``); ``--native``, every record's own ligand.  A sequence must be as long as its record's
ligand.  The output has one row per record of the dataset, in the dataset's order: for ``--table`` the table's own rows
with all their columns, put into that order (rows that name no record of the dataset are dropped), otherwise
``structure_ids`` and ``sequence``.  It gets the columns ``bound`` (nats), ``score`` (nats per residue; lower: the model
likes the sequence better) and ``stderr`` (of the score over the seeds; NaN for one seed).  The score is
the variational score of the sampler's own reverse law, not a certified likelihood bound: see the function's docstring.
The model, the dataset and the number of steps are those of ``sequence_model/sample.py``'s CONFIG.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def vocabulary():
    """The package's residue letters (imported when first needed: parsing the arguments loads no package)."""
    import __graft_entry__
    __graft_entry__.load_package()
    from e3diff_amd.sequence_model.dataset import AA_VOCAB
    return "".join(AA_VOCAB)


def parse_seeds(text):
    try:
        seeds = [int(v, 0) for v in text.split(",") if v.strip()]
    except ValueError:
        raise argparse.ArgumentTypeError(f"seeds must be integers separated by commas, got {text!r}") from None
    if not seeds or any(not 0 <= s < 1 << 64 for s in seeds):
        raise argparse.ArgumentTypeError(f"seeds must be one or more integers in [0, 2^64), got {text!r}")
    if len(set(seeds)) != len(seeds):
        raise argparse.ArgumentTypeError(f"a seed given twice adds no draw: {text!r}")
    return seeds


def positive(text):
    try:
        v = int(text)
    except ValueError:
        v = 0
    if v < 1:
        raise argparse.ArgumentTypeError(f"expected a positive integer, got {text!r}")
    return v


def output_path(text):
    if not text.endswith((".json", ".pkl")):
        raise argparse.ArgumentTypeError(f"the output must end in .json or .pkl, got {text!r}")
    return text


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", required=True, help="the biolip.pt whose records the sequences belong to")
    ap.add_argument("--model", required=True, help="the sequence model's state_dict (reference checkpoint key names)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--table", help="a table sample.run() wrote: score its predict_sequence column by structure_ids; the "
                                      "output is its rows, put into the dataset's order, with the new columns")
    src.add_argument("--fasta", help="a FASTA file, one record per ligand, headers = structure ids")
    src.add_argument("--native", action="store_true", help="score every record's own ligand sequence")
    ap.add_argument("--seeds", type=parse_seeds, default=[0], help="keyed draws to average over, e.g. 1,2,3 (default 0)")
    ap.add_argument("--levels", type=positive, default=None,
                    help="score every K-th step index (and index 0) instead of all of them: T / K forwards per seed")
    ap.add_argument("--transition", choices=("blosum", "uniform"), default="blosum",
                    help="the transition the model was trained and sampled with (default blosum, as sample.py)")
    ap.add_argument("--split", choices=("test", "all"), default="test", help="the records of --data to meet (default test)")
    ap.add_argument("-o", "--output", required=True, type=output_path, help="scores.json or scores.pkl")
    return ap.parse_args(argv)


def read_fasta(path):
    """[(id, sequence)] of a FASTA file: the id is the header's first word, the sequence its lines joined, upper case."""
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


def match_sequences(ids, lengths, records, what="the input"):
    """The sequence of every record of the dataset, in its order: ``records`` [(id, sequence)] are met by id (all of them
    in the dataset's own order: by position, which also serves datasets with repeated ids).  Raises ``ValueError`` for a
    missing or repeated id, a wrong length or a letter outside the vocabulary."""
    records = [(str(i), str(s)) for i, s in records]
    if [i for i, _ in records] == list(ids):
        seqs = [s for _, s in records]
    else:
        by_id = {}
        for i, s in records:
            if i in by_id:
                raise ValueError(f"{what} names {i} twice")
            by_id[i] = s
        if len(set(ids)) != len(ids):
            raise ValueError(f"the dataset holds a structure id twice: {what} must list every record, in the dataset's order")
        missing = [i for i in ids if i not in by_id]
        if missing:
            raise ValueError(f"{what} has no sequence for {len(missing)} record(s): {', '.join(missing[:5])}")
        seqs = [by_id[i] for i in ids]
    vocab = vocabulary()
    for i, n, s in zip(ids, lengths, seqs):
        if len(s) != n:
            raise ValueError(f"{i}: the ligand has {n} residues, the sequence {len(s)}")
        bad = sorted(set(s) - set(vocab))
        if bad:
            raise ValueError(f"{i}: letters {''.join(bad)!r} are outside the vocabulary {vocab}")
    return seqs


def main(argv=None):
    args = parse_args(argv)
    import pandas as pd
    import torch
    from torch.utils.data import DataLoader
    import __graft_entry__
    __graft_entry__.load_package()
    from e3diff_amd.sequence_model import sample as Q
    from e3diff_amd.sequence_model.dataset import LigandBindingSiteDataset
    from e3diff_amd.sequence_model.utils import (BlosumTransition, DiscreteUniformTransition,
                                                 PredefinedNoiseScheduleDiscrete)
    cfg = Q.CONFIG
    dataset = LigandBindingSiteDataset(args.data, None if args.split == "all" else args.split, cfg["max_seq_len"],
                                       cfg["pocket_ext"])
    loader = DataLoader(dataset, batch_size=cfg["batch_size"], shuffle=False)
    ids, lengths = [], []
    for batch in loader:
        sid = batch["structure_ids"]
        ids += [f'{sid["pdb_id"][b]}_{sid["ligand_chain"][b]}' for b in range(len(sid["pdb_id"]))]
        lengths += [int(n) for n in batch["ligand_attn_mask"].sum(dim=1)]
    table = None
    if args.table:
        table = pd.read_pickle(args.table)
        for col in ("structure_ids", "predict_sequence"):
            if col not in table.columns:
                raise ValueError(f"{args.table} has no {col!r} column: not a table sample.run() wrote")
        sequences = match_sequences(ids, lengths, zip(table["structure_ids"], table["predict_sequence"]), args.table)
    elif args.fasta:
        sequences = match_sequences(ids, lengths, read_fasta(args.fasta), args.fasta)
    else:
        sequences = None
    model = Q.get_model(len(loader), args.model)
    dev = next(model.parameters()).device
    schedule = PredefinedNoiseScheduleDiscrete(cfg["noise_schedule"], cfg["timesteps"]).to(dev)
    transition = BlosumTransition(x_classes=20) if args.transition == "blosum" else DiscreteUniformTransition(20)
    cols = {"bound": [], "score": [], "stderr": [], "n": []}
    scored = []
    first = 0
    for batch in loader:
        n = batch["ligand_seq"].shape[0]
        chunk = None if sequences is None else sequences[first:first + n]
        out = Q.score_sequences(batch, model, schedule, transition, chunk, levels=args.levels, seed=args.seeds,
                                item_ids=list(range(first, first + n)))
        for key in cols:
            cols[key] += out[key].tolist()
        if chunk is None:
            idx, mask = batch["ligand_seq"].argmax(dim=-1), batch["ligand_attn_mask"] != 0
            chunk = ["".join(Q.AA_VOCAB[j] for j in idx[b][mask[b]]) for b in range(n)]
        scored += chunk
        first += n
    if table is not None:      # the table's own rows, in the dataset's order (match_sequences met them the same way)
        named = list(table["structure_ids"].astype(str))
        rows = range(len(ids)) if named == ids else [named.index(i) for i in ids]
        res = table.iloc[list(rows)].reset_index(drop=True)
    else:
        res = pd.DataFrame({"structure_ids": ids, "sequence": scored})
    for key in ("bound", "score", "stderr"):
        res[key] = cols[key]
    if args.output.endswith(".pkl"):
        res.to_pickle(args.output)
    else:
        rows = [{k: (None if isinstance(v, float) and v != v else v) for k, v in row.items()}      # NaN -> null
                for row in res.to_dict(orient="records")]
        with open(args.output, "w") as f:
            json.dump(rows, f, indent=1)
    print(res)
    print(f"wrote {len(res)} score row(s) to {args.output}")
    return res


if __name__ == "__main__":
    main()
