#!/usr/bin/env python3
"""Strided (DDIM / respaced) structure sampling against the ancestral chain: one JSON line.

    python tools/bench_strided.py --kernels [--batch 256] [--seq-len 256] [--launches 200]
        # the update kernels (ancestral table form, strided, multistep, known compose; with buffer and keyed draws) launched
        # alternately on one [batch, seq-len, 8] state -- for ``rocprofv3 --kernel-trace --stats``: per-kernel times in one run
    python tools/bench_strided.py --single [--steps 50]
        # tools/bench_single.py's chain (ONE 64-residue pocket) four times in one process: ancestral / strided, torch /
        # keyed draws, eager launches -- under rocprofv3 the same four kernels at that shape; without it ms per step
    python tools/bench_strided.py --chains
        # per-step time of the strided and multistep updates against their own ancestral leg, eager and graph-replayed,
        # and the wall time of the 50-step strided and multistep chains (step = 20, T = 1000) against the 1000-step
        # ancestral chain of one pocket
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_single  # noqa: E402  (loads the package)

pkg = bench_single.pkg
DEV = "cuda:0"


def kernels(batch, seq_len, launches, eta=1.0):
    """Alternate launches of the update kernels on one state; wall time per launch by HIP events as a cross-check."""
    from e3diff_amd import keyed
    from e3diff_amd.structure_model.sample import step_plan
    from e3diff_amd.structure_model.utils import CosineTables, KnownLevels, MultistepTables, StridedTables
    ops = pkg.ops
    tab = CosineTables(1000)
    coef4 = step_plan(tab, DEV, table=True).coef
    coef8 = StridedTables(tab, list(reversed(range(1000))), eta).coef.to(DEV)
    coef_ms = MultistepTables(tab, list(reversed(range(1000)))).coef.to(DEV)      # row 500 extrapolates: c_1 > 0
    g = torch.Generator(device=DEV).manual_seed(0)
    x = (torch.rand(batch, seq_len, 8, device=DEV, generator=g) * 6.28 - 3.14).contiguous()
    e = torch.randn(batch, seq_len, 8, device=DEV, generator=g)
    z = torch.randn(batch, seq_len, 8, device=DEV, generator=g)
    # the two compose legs hold half the positions (whole residues, as a chain's mask does), at level row 500
    x0 = (torch.rand(batch, seq_len, 8, device=DEV, generator=g) * 6.28 - 3.14).contiguous()
    mask = (torch.rand(batch, seq_len, 1, device=DEV, generator=g) < 0.5).expand_as(x).to(torch.uint8).contiguous()
    levels = KnownLevels(tab, list(reversed(range(1000)))).levels.to(DEV)
    out = torch.empty_like(x)
    hist = (torch.rand(batch, seq_len, 8, device=DEV, generator=g) * 6.28 - 3.14).contiguous()   # rewritten by every launch
    keys =keyed.padded_keys(list(range(batch)), seq_len, DEV)
    t = torch.full((1,), 500, device=DEV, dtype=torch.long)
    legs = {"ancestral": lambda: ops.ddpm_step_wrap_table(x, e, z, coef4, t, out=out),
            "keyed_ancestral": lambda: ops.keyed_ddpm_step_wrap(x, e, coef4, t, keys, 7, out=out),
            "strided": lambda: ops.strided_step_wrap(x, e, z, coef8, t, out=out),
            "strided_wrap_x0": lambda: ops.strided_step_wrap(x, e, z, coef8, t, wrap_x0=True, out=out),
            "keyed_strided": lambda: ops.keyed_strided_step_wrap(x, e, coef8, t, keys, 7, out=out),
            "multistep": lambda: ops.multistep_step_wrap(x, e, hist, coef_ms, t, out=out),
            "known_compose": lambda: ops.known_compose_wrap(x, x0, mask, z, levels, t),
            "keyed_known_compose": lambda: ops.keyed_known_compose_wrap(x, x0, mask, levels, t, keys, 7)}
    for f in legs.values():
        f()
    torch.cuda.synchronize()
    ev = {k: [] for k in legs}
    for _ in range(launches):
        for k, f in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    med = {k: sorted(a.elapsed_time(b) for a, b in v)[len(v) // 2] * 1e3 for k, v in ev.items()}
    return {"shape": [batch, seq_len, 8], "launches_each": launches, "eta": eta, "event_us_median": med,
            "bytes_moved": {"unkeyed": 4 * x.numel() * 4, "keyed": 3 * x.numel() * 4, "multistep": 5 * x.numel() * 4}}


def single(steps, graph=0):
    legs = {"ancestral": {}, "ancestral_keyed": {"seed": 7}, "strided_eta1": {"update": "strided", "eta": 1.0},
            "strided_eta1_keyed": {"update": "strided", "eta": 1.0, "seed": 7}}
    return {k: bench_single.run(steps=steps, graph=graph, chains=2, **kw)["ms_per_step"] for k, kw in legs.items()}


def chains():
    out = {"per_step_ms_T50": {}}
    for graph in (0, 1):
        for name, kw in (("ancestral", {}), ("strided_eta0", {"update": "strided"}),
                         ("multistep", {"update": "multistep"}), ("strided_eta1", {"update": "strided", "eta": 1.0}),
                         ("strided_eta1_wrap_x0", {"update": "strided", "eta": 1.0, "wrap_x0": True})):
            out["per_step_ms_T50"][f"{name}_{'graph' if graph else 'eager'}"] = \
                bench_single.run(steps=50, graph=graph, chains=3, **kw)["ms_per_step"]
    t0 = time.perf_counter()
    full = bench_single.run(steps=1000, chains=1)
    strided = bench_single.run(steps=1000, stride=20, chains=3, update="strided")
    multistep = bench_single.run(steps=1000, stride=20, chains=3, update="multistep")
    out["wall_ms_one_pocket_L64"] = {"ancestral_1000_steps": full["ms_per_chain"],
                                     "strided_50_steps_of_T1000": strided["ms_per_chain"],
                                     "multistep_50_steps_of_T1000": multistep["ms_per_chain"],
                                     "ratio": full["ms_per_chain"] / strided["ms_per_chain"],
                                     "graph_replay": "sampler default"}
    out["measured_in_s"] = time.perf_counter() - t0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--single", action="store_true")
    ap.add_argument("--chains", action="store_true")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq-len", type=int, default=256)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    out = {"metric": "strided_structure_sampling"}
    if a.kernels:
        out["kernels"] = kernels(a.batch, a.seq_len, a.launches)
    if a.single:
        out["single_pocket_ms_per_step_eager"] = single(a.steps)
    if a.chains:
        out["chains"] = chains()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
