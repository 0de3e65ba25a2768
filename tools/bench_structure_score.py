"""Time ``score_structures`` against one seeded ``p_sample_loop`` chain of the same batch: B = 64 pockets, L = 64 rows, the
structure module's CONFIG model (hidden 768, 12 layers) with seeded weights, T = 1000, its ARITHMETIC.  Scoring every
``--stride``-th level with one seed makes as many decoder forwards of 64 items as the chain with ``step=--stride`` makes
steps (both run the pocket encoder once), but the score's levels do not wait for one another, so ``--levels-per-launch``
may fold several into one launch.  Host clock around whole calls (both end in a device-to-host copy, which synchronises),
after a warm-up of every form; the forms alternate within each of ``--repeats`` rounds, so that drift on a shared machine
hits them alike.  A record, not a gate:

    python tools/bench_structure_score.py [--out profiles/structure_score_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq-len", type=int, default=64)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--stride", type=int, default=20)
    ap.add_argument("--levels-per-launch", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    __graft_entry__.load_package()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from helpers import seeded_state_dict, synthetic_pockets
    from e3diff_amd import ops
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.model import ConditionalBertForDiffusionBase
    from e3diff_amd.structure_model.utils import CosineTables
    B, L, T, k = a.batch, a.seq_len, a.timesteps, a.stride
    enc, dec = S.build_configs(dict(S.CONFIG, max_seq_len=L))
    model = ConditionalBertForDiffusionBase(enc, dec, 8)
    model.load_state_dict(seeded_state_dict({n: tuple(v.shape) for n, v in model.state_dict().items()}, seed=2))
    model = model.eval().to(DEV)
    pk = {n: v.to(DEV) for n, v in synthetic_pockets(B, L, seed=8).items() if torch.is_tensor(v)}
    tab = CosineTables(T)
    ids = list(range(B))
    args = (model, pk["ligand_attn_mask"])
    pocket = (pk["receptor_seq"], pk["receptor_attn_mask"], pk["receptor_angles"], T, tab)
    x_T = S.keyed_x_T(5, ids, L, 8, device=DEV)

    def chain():
        with ops.arithmetic(S.ARITHMETIC):
            S.p_sample_loop(*args, x_T, *pocket, disable_pbar=True, step=k, seed=5, item_ids=ids)

    forms = {"p_sample_loop_chain": chain}
    for n in a.levels_per_launch:
        def scored(n=n):
            with ops.arithmetic(S.ARITHMETIC):
                S.score_structures(*args, pk["ligand_angles"], *pocket, levels=k, seed=5, item_ids=ids, levels_per_launch=n)
        forms[f"score_levels_per_launch_{n}"] = scored
    for f in forms.values():
        f()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(a.repeats):
        for name, f in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0))
    forwards = len(range(0, T, k))
    res = {"what": f"one whole call, host clock around it (ends in a synchronising copy), milliseconds: a seeded p_sample_loop "
                   f"chain with step={k} against score_structures(levels={k}) with one seed, the same batch and model; both make "
                   f"{forwards} decoder forwards of {B} items and one pocket-encoder pass",
           "device": torch.cuda.get_device_name(0), "B": B, "L": L, "T": T, "stride": k, "forwards_per_call": forwards,
           "arithmetic": S.ARITHMETIC, "repeats": a.repeats,
           "ms_per_call": {name: {"median": statistics.median(v), "min": min(v), "max": max(v)} for name, v in ms.items()}}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
