"""Time ``evaluate.describe_samples`` on --pockets x --replicates chains of --length residues (default 256 x 32 x 32:
8192 chains, 262144 residues), split into the NeRF launch, the ``backbone_geometry`` call and everything else (host
packing, the device sums, the copies back and the Python rows).  Random angles: dihedrals ~ U(-pi, pi), bond angles
~ N(1.95, 0.1).  Host clock around parts that end in a device synchronise, after one warm-up call.  A record, not a gate:

    python tools/bench_describe.py [--out profiles/describe_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pockets", type=int, default=256)
    ap.add_argument("--replicates", type=int, default=32)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    __graft_entry__.load_package()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from e3diff_amd import evaluate
    rng = np.random.default_rng(0)

    def chain():
        ang = np.empty((a.length, 8), dtype=np.float32)
        ang[:, :4] = rng.uniform(-np.pi, np.pi, (a.length, 4))
        ang[:, 4:] = rng.normal(1.95, 0.1, (a.length, 4))
        return ang

    replicates = [[chain() for _ in range(a.pockets)] for _ in range(a.replicates)]
    spent = {}

    def timed(name, fn):
        def run(*args):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*args)
            torch.cuda.synchronize()
            spent[name] = time.perf_counter() - t0
            return out
        return run

    hooks = dict(device=DEV, _build=timed("nerf", lambda ang, lens: evaluate._device_build(ang, lens, DEV)),
                 _geometry=timed("geometry", evaluate.backbone_geometry))
    evaluate.describe_samples(replicates, **hooks)                                  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows = evaluate.describe_samples(replicates, **hooks)
    total = time.perf_counter() - t0
    letters = "".join(s for r in rows for s in r["ss"])
    result = {"pockets": a.pockets, "replicates": a.replicates, "length": a.length, "chains": a.pockets * a.replicates,
              "total_ms": 1e3 * total, "nerf_ms": 1e3 * spent["nerf"], "geometry_ms": 1e3 * spent["geometry"],
              "host_ms": 1e3 * (total - spent["nerf"] - spent["geometry"]),
              "letters": {c: letters.count(c) for c in "HBEGITS-"}, "repeats": 1}
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
