"""Split a biolip.pt by sequence cluster, so that no validation or test record has a near-copy in training.

Records are clustered on the device (similarity.redundancy_clusters: the connected components of "identity >= threshold",
identity = matches of the best local alignment / the shorter length) by their ligand sequence, their receptor sequence,
or both -- then two records are linked when either their ligands or their receptors reach the threshold.  Whole
clusters are dealt to train / validation / test (similarity.split_by_cluster).  The output is the JSON file that
``LigandBindingSiteDataset(..., split_file=...)`` and ``E3D_SPLIT_FILE`` take:

    python tools/split_dataset.py --data biolip.pt [--by ligand|receptor|both] [--threshold 0.4]
                                  [--fractions 0.8,0.1,0.1] [--seed 0] -o splits.json

It prints the histogram of cluster sizes and, for the dataset's random 80/10/10 and for the new split alike, how many
validation and test records have a training neighbour at or above the threshold (by ligand; exhaustive, block by block).
The first of the two numbers is what a model validated on the random split was flattered by."""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fractions(text):
    try:
        out = tuple(float(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"fractions must be three numbers separated by commas, got {text!r}") from None
    if len(out) != 3 or min(out) < 0 or abs(sum(out) - 1.0) > 1e-9:
        raise argparse.ArgumentTypeError(f"fractions must be three shares >= 0 that sum to 1, got {text!r}")
    return out


def threshold(text):
    v = float(text)
    if not 0.0 < v <= 1.0:
        raise argparse.ArgumentTypeError(f"the threshold is an identity in (0, 1], got {text!r}")
    return v


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", required=True, help="the biolip.pt to split")
    ap.add_argument("--by", choices=("ligand", "receptor", "both"), default="ligand", help="the sequences to cluster on")
    ap.add_argument("--threshold", type=threshold, default=0.4, help="identity at which two records are linked (default 0.4)")
    ap.add_argument("--fractions", type=fractions, default=(0.8, 0.1, 0.1), help="train,validation,test (default 0.8,0.1,0.1)")
    ap.add_argument("--seed", type=int, default=0, help="order in which clusters are dealt (default 0)")
    ap.add_argument("--block", type=int, default=1024, help="sequences per side of one launch (default 1024)")
    ap.add_argument("-o", "--output", required=True, help="splits.json")
    return ap.parse_args(argv)


def record_sequences(records):
    """(ligand strings, receptor strings) of biolip records: ``amino_acid[ligand_mask]`` and the rest."""
    ligands, receptors = [], []
    for r in records:
        mask = [bool(m) for m in r["ligand_mask"].tolist()]
        ligands.append("".join(a for a, m in zip(r["amino_acid"], mask) if m))
        receptors.append("".join(a for a, m in zip(r["amino_acid"], mask) if not m))
    return ligands, receptors


def random_split_names(n, seed=0):
    """The split name of every record under the dataset's own rule: ``random.seed(0); shuffle; 80/10/10``."""
    order = list(range(n))
    random.Random(seed).shuffle(order)
    cut, tenth = int(n * 0.8), int(n * 0.1)
    names = [None] * n
    for pos, i in enumerate(order):
        names[i] = "train" if pos < cut else "validation" if pos < cut + tenth else "test"
    return names


def leaked(names, ligands, level, similarity, **kw):
    """{split: how many of its records have a training ligand at identity >= level} for validation and test."""
    train = [s for s, n in zip(ligands, names) if n == "train"]
    out = {}
    for split in ("validation", "test"):
        held = [s for s, n in zip(ligands, names) if n == split]
        out[split] = (int((similarity.nearest(held, train, **kw)["identity"] >= level).sum()) if held and train else 0, len(held))
    return out


def cluster_histogram(labels):
    sizes = {}
    for lab in set(labels):
        n = labels.count(lab)
        sizes[n] = sizes.get(n, 0) + 1
    return dict(sorted(sizes.items()))


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import __graft_entry__
    __graft_entry__.load_package()
    from e3diff_amd import biolip, similarity
    from e3diff_amd.structure_model.dataset import split_key
    records = biolip.load(args.data)
    ligands, receptors = record_sequences(records)
    for i, (r, lig) in enumerate(zip(records, ligands)):          # (letters and empty ligands: biolip.load refused them)
        if len(lig) > similarity.MAX_LEN:
            raise ValueError(f"{args.data}: the ligand of record {i} ({split_key(r)}) has {len(lig)} residues, "
                             f"the limit is {similarity.MAX_LEN}")
    kw = dict(block=args.block)
    labelings = []
    if args.by in ("ligand", "both"):
        labelings.append(similarity.redundancy_clusters(ligands, args.threshold, **kw))
    if args.by in ("receptor", "both"):
        ok = [i for i, s in enumerate(receptors) if 0 < len(s) <= similarity.MAX_LEN]
        skipped = len(records) - len(ok)
        if skipped:
            print(f"{skipped} record(s) have a receptor of 0 or more than {similarity.MAX_LEN} residues: each is its own "
                  "receptor cluster")
        part = similarity.redundancy_clusters([receptors[i] for i in ok], args.threshold, **kw) if ok else []
        labels = np.arange(len(records), dtype=np.int64) + len(records)          # ids no cluster of ``part`` uses
        for i, lab in zip(ok, part):
            labels[i] = lab
        labelings.append(labels)
    labels = similarity.merge_labels(*labelings).tolist()
    names = similarity.split_by_cluster(labels, args.fractions, args.seed)
    hist = cluster_histogram(labels)
    print(f"{len(records)} records, {len(set(labels))} clusters by {args.by} at identity >= {args.threshold}")
    print("cluster size: clusters   " + "  ".join(f"{size}: {n}" for size, n in hist.items()))
    for s in similarity.SPLIT_NAMES:
        print(f"  {s}: {names.count(s)} records ({names.count(s) / len(names):.3f})")
    report = {}
    for what, split in (("random", random_split_names(len(records))), ("clustered", names)):
        report[what] = leaked(split, ligands, args.threshold, similarity, **kw)
        print(f"{what} split: " + ", ".join(f"{hit} of {n} {s} records have a training ligand at identity >= {args.threshold}"
                                            for s, (hit, n) in report[what].items()))
    out = {"format": "e3d-split-1", "by": args.by, "threshold": args.threshold, "fractions": list(args.fractions),
           "seed": args.seed, "clusters": len(set(labels)),
           "leaked": {w: {s: list(v) for s, v in r.items()} for w, r in report.items()},
           "records": [[split_key(r), n] for r, n in zip(records, names)]}
    with open(args.output, "w") as f:
        json.dump(out, f, indent=0)
    print(f"wrote the split of {len(records)} records to {args.output}")
    return out


if __name__ == "__main__":
    main()
