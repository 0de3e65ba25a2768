"""Time ``score_sequences`` against one ``denoise`` chain of the same batch: B = 64 pockets, L = 64 rows, T = 50 steps, the
module's CONFIG model (hidden 768, 6 layers) with seeded weights, the uniform transition.  Scoring all 50 levels with one
seed makes 50 model forwards of 64 items -- as many as the 50-step chain -- but its levels do not wait for one another, so
``--levels-per-launch`` may fold several into one launch.  Host clock around whole calls (both end in a device-to-host
copy, which synchronises), after a warm-up of every form; the forms alternate within each of ``--repeats`` rounds, so that
drift on a shared machine hits them alike.  A record, not a gate:

    python tools/bench_score.py [--out profiles/score_timing.json]
"""
import argparse
import contextlib
import io
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
    ap.add_argument("--timesteps", type=int, default=50)
    ap.add_argument("--levels-per-launch", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    __graft_entry__.load_package()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from helpers import seeded_state_dict, synthetic_pockets
    from e3diff_amd.sequence_model import sample as Q
    from e3diff_amd.sequence_model.model import PeptideDiff
    from e3diff_amd.sequence_model.utils import DiscreteUniformTransition, PredefinedNoiseScheduleDiscrete
    B, L, T = a.batch, a.seq_len, a.timesteps
    enc, dec = Q.build_configs(dict(Q.CONFIG, max_seq_len=L))
    model = PeptideDiff(enc, dec, feature_names=list(Q.AA_VOCAB), loss_func=torch.nn.CrossEntropyLoss(),
                        noise_schedule="cosine", timesteps=T)
    model.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=2))
    model = model.eval().to(DEV)
    pk = dict(synthetic_pockets(B, L, seed=8, with_ligand_seq=True), structure_ids=None)
    sched, trans = PredefinedNoiseScheduleDiscrete("cosine", T).to(DEV), DiscreteUniformTransition(20)
    ids = list(range(B))

    def chain():
        with contextlib.redirect_stdout(io.StringIO()):
            Q.denoise(pk, model, sched, trans, True, timesteps=T, seed=5, item_ids=ids)

    forms = {"denoise_chain": chain}
    for n in a.levels_per_launch:
        forms[f"score_levels_per_launch_{n}"] = (
            lambda n=n: Q.score_sequences(pk, model, sched, trans, timesteps=T, seed=5, item_ids=ids, levels_per_launch=n))
    for f in forms.values():
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(a.repeats):
        for name, f in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0))
    res = {"what": "one whole call, host clock around it (ends in a synchronising copy), milliseconds: a 50-step seeded denoise "
                   "chain against score_sequences over all levels with one seed, the same batch and model",
           "device": torch.cuda.get_device_name(0), "B": B, "L": L, "T": T, "forwards_per_call": T, "repeats": a.repeats,
           "ms_per_call": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()}}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
