#!/usr/bin/env python3
"""Score peptide backbones under the structure diffusion model (structure_model/sample.py::score_structures, on the GPU).

    python tools/score_structures.py --data biolip.pt --model struct.ckpt --samples out_seed1.pkl out_seed2.pkl -o scores.json
    python tools/score_structures.py --data biolip.pt --model struct.ckpt --native --levels 50 --seeds 1,2,3 -o native.pkl

The backbones come from ``--samples``, one or more pickles ``structure_model/sample.py`` wrote -- each a replicate: a list
of [T, l_i, 8] trajectories (their last entry is scored) or [l_i, 8] angle arrays, entry i belonging to record i of the
dataset (a pickle may stop early: ``sample()`` writes the first batch) -- or from ``--native``, every record's own ligand
angles.  An entry must be as long as its record's ligand.  The output has one row per (record, replicate), replicate by
replicate in the dataset's order: ``structure_ids``, ``replicate`` (the pickle's place on the command line, 0 for
``--native``), ``source``, ``bound`` (nats), ``score`` (nats per angle; lower: the model likes the backbone better),
``stderr`` (of the score over the seeds; NaN for one seed), ``n`` (the angles scored), one column per angle feature of the
dataset (``phi`` .. ``CA:C:O``: that feature's share of the bound without the prior, per residue) and ``rank``, the
replicate's place among the replicates of its pocket by score (1: the lowest).  Every replicate of a pocket is scored with
the same keyed draws (the draws are keyed by the record's index), so their scores differ by the backbones alone.  The
score is the variational score of the sampler's own reverse law with wrapped normals read as Gaussians, not a certified
likelihood bound: see the function's docstring.  The dataset, the model and the number of steps are those of
``structure_model/sample.py``'s CONFIG, the arithmetic its ARITHMETIC.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from score_sequences import output_path, parse_seeds, positive  # noqa: E402  (argument types; loads no package)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", required=True, help="the biolip.pt whose records the backbones belong to")
    ap.add_argument("--model", required=True, help="the structure model's state_dict (reference checkpoint key names)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--samples", nargs="+", metavar="PKL",
                     help="pickles structure_model/sample.py wrote, one per replicate; entry i belongs to record i")
    src.add_argument("--native", action="store_true", help="score every record's own ligand angles")
    ap.add_argument("--seeds", type=parse_seeds, default=[0], help="keyed draws to average over, e.g. 1,2,3 (default 0)")
    ap.add_argument("--levels", type=positive, default=None,
                    help="score every K-th timestep (and timestep 0) instead of all of them: T / K forwards per seed")
    ap.add_argument("--split", choices=("test", "all"), default="test", help="the records of --data to meet (default test)")
    ap.add_argument("-o", "--output", required=True, type=output_path, help="scores.json or scores.pkl")
    return ap.parse_args(argv)


def replicate_angles(chains, lengths, ids, pad, n_ft, what):
    """A replicate's angle arrays [l_i, F] as a padded float tensor [len(chains), pad, F]; entry i must be as long as
    record i's ligand."""
    import torch
    if len(chains) > len(lengths):
        raise ValueError(f"{what} holds {len(chains)} backbones, the dataset {len(lengths)} records")
    out = torch.zeros((len(chains), pad, n_ft), dtype=torch.float32)
    for i, c in enumerate(chains):
        if c.ndim != 2 or c.shape[1] != n_ft:
            raise ValueError(f"{what}: entry {i} is {tuple(c.shape)}, expected [l, {n_ft}] angles")
        if c.shape[0] != lengths[i]:
            raise ValueError(f"{ids[i]}: the ligand has {lengths[i]} residues, entry {i} of {what} {c.shape[0]}")
        out[i, :c.shape[0]] = torch.from_numpy(c)
    return out


def ranks_within(groups, scores):
    """1-based rank of each row's score among the rows of its group (ties and NaN: in row order, NaN last)."""
    rank = [0] * len(scores)
    for g in set(groups):
        rows = [i for i, x in enumerate(groups) if x == g]
        rows.sort(key=lambda i: (scores[i] != scores[i], scores[i] if scores[i] == scores[i] else 0.0, i))
        for place, i in enumerate(rows, 1):
            rank[i] = place
    return rank


def main(argv=None):
    args = parse_args(argv)
    import pandas as pd
    import torch
    import __graft_entry__
    __graft_entry__.load_package()
    from e3diff_amd import ops
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.create_pdb import load_sampled_angles
    from e3diff_amd.structure_model.dataset import LigandBindingSiteDataset, NoisedAnglesDataset
    cfg = S.CONFIG
    dataset = NoisedAnglesDataset(LigandBindingSiteDataset(args.data, None if args.split == "all" else args.split,
                                                           cfg["max_seq_len"], cfg["pocket_ext"]), timesteps=cfg["timesteps"])
    records = [dataset.dset[i] for i in range(len(dataset))]
    ids = [f'{r["structure_ids"]["pdb_id"]}_{r["structure_ids"]["ligand_chain"]}' for r in records]
    lengths = [int(r["ligand_attn_mask"].sum()) for r in records]
    names = list(dataset.feature_names)
    pad, n_ft = records[0]["ligand_angles"].shape
    if args.native:
        replicates = [("native", torch.stack([r["ligand_angles"] for r in records]).float())]
    else:
        replicates = [(path, replicate_angles(load_sampled_angles(path), lengths, ids, pad, n_ft, path)) for path in args.samples]
    # one item per (replicate, record), replicate by replicate; the draws are keyed by the record's index
    items = [(rep, i) for rep, (_, ang) in enumerate(replicates) for i in range(ang.shape[0])]
    model = S.load_model(dataset, args.model)
    dev = next(model.parameters()).device
    cols = {k: [] for k in ("bound", "score", "stderr", "n")}
    per_feature = []
    bs = cfg["batch_size"]
    for first in range(0, len(items), bs):
        part = items[first:first + bs]

        def stack(name):
            return torch.stack([records[i][name] for _, i in part]).to(dev)
        angles = torch.stack([replicates[rep][1][i] for rep, i in part])
        with ops.arithmetic(S.ARITHMETIC):
            out = S.score_structures(model, stack("ligand_attn_mask"), angles, stack("receptor_seq"), stack("receptor_attn_mask"),
                                     stack("receptor_angles"), dataset.timesteps, dataset.alpha_beta_terms["betas"],
                                     levels=args.levels, seed=args.seeds, item_ids=[i for _, i in part],
                                     scale=dataset.angular_var_scale)
        for key in cols:
            cols[key] += out[key].tolist()
        residues = torch.tensor([lengths[i] for _, i in part], dtype=torch.float64)
        per_feature += (out["per_feature"] / residues[:, None]).tolist()
    res = pd.DataFrame({"structure_ids": [ids[i] for _, i in items], "replicate": [rep for rep, _ in items],
                        "source": [replicates[rep][0] for rep, _ in items]})
    for key in ("bound", "score", "stderr", "n"):
        res[key] = cols[key]
    for f, name in enumerate(names):
        res[name] = [row[f] for row in per_feature]
    res["rank"] = ranks_within([i for _, i in items], cols["score"])
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
