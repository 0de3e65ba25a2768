"""Time the discrete posterior launch with and without design controls, at the shape of tools/bench_joint.py
(B = 128 pockets, L = 128 rows, C = 20 classes): the launch without controls, the controlled launch with a NULL bias and
the controlled launch reading a [B, L, C] bias, keyed draws in all three (the launches of a seeded chain).  HIP events
around windows of ``--launches`` back-to-back launches on one stream, after a warm-up of every form; the three forms
alternate within each of ``--repeats`` rounds, so that drift on a shared machine hits them alike.  A record, not a gate:

    python tools/bench_design_posterior.py [--out profiles/design_posterior_bias_ab.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seq-len", type=int, default=128)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = __graft_entry__.load_package()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from e3diff_amd import keyed, ops
    from e3diff_amd.design import DesignControls
    from e3diff_amd.sequence_model.utils import DiscreteUniformTransition, PredefinedNoiseScheduleDiscrete
    B, L, C, T = a.batch, a.seq_len, a.classes, 50
    g = torch.Generator().manual_seed(0)
    xt = torch.randint(0, C, (B, L), generator=g).int().to(DEV)
    logits = (2 * torch.randn(B, L, C, generator=g)).to(DEV)
    sched, trans = PredefinedNoiseScheduleDiscrete("cosine", T).to(DEV), DiscreteUniformTransition(C)
    s = torch.full((B, 1), 24.0, device=DEV)
    qsb = trans.get_Qt_bar(sched.get_alpha_bar(t_normalized=s / T), DEV).contiguous()
    qtb = trans.get_Qt_bar(sched.get_alpha_bar(t_normalized=(s + 1) / T), DEV).contiguous()
    keys = keyed.padded_keys(list(range(B)), L, DEV)
    s_dev = torch.full((1,), 24, dtype=torch.long, device=DEV)
    controls = DesignControls.build((B, L, C), temperature=0.7, omit="CM", allow={3: "LIV"}).in_frame(lambda t: t, DEV)
    it = float(controls.inv_temp)
    forms = {
        "no_controls": lambda: ops.keyed_discrete_posterior_sample(xt, logits, qsb, qtb, keys, 5, s_dev),
        "controls_null_bias": lambda: ops.keyed_discrete_posterior_sample_ctl(xt, logits, None, it, qsb, qtb, keys, 5, s_dev),
        "controls_bias": lambda: ops.keyed_discrete_posterior_sample_ctl(xt, logits, controls.bias, it, qsb, qtb, keys, 5, s_dev),
    }
    for f in forms.values():
        for _ in range(50):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in forms}
    for _ in range(a.repeats):
        for name, f in forms.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(a.launches):
                f()
            end.record()
            end.synchronize()
            us[name].append(1e3 * start.elapsed_time(end) / a.launches)
    res = {"what": "keyed discrete posterior launch, HIP events around windows of back-to-back launches (host launch "
                   "path included), microseconds per launch",
           "device": torch.cuda.get_device_name(0), "B": B, "L": L, "C": C, "launches_per_window": a.launches,
           "repeats": a.repeats, "bias_bytes": B * L * C * 4,
           "us_per_launch": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in us.items()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
