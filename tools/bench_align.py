"""Time the alignment kernel (csrc/seq_align.hip, through ops.align_pairs) on three workloads and report cell updates
per second, a cell being one (query residue, target residue) of one pair:

    peptides   4096 queries x 16384 targets, lengths uniform in 5..30 (targets sorted by length, as similarity.align does)
    medium     256 x 256 sequences of 256 residues
    long       64 x 64 sequences of 1024 residues

Uniform random residues, BLOSUM62, gaps (11, 1).  Device events around --repeats back-to-back launches after one warm-up
launch; the median is reported, the minimum and maximum next to it.  A record, not a gate:

    python tools/bench_align.py [--out profiles/seq_align_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402

DEV = "cuda:0"
WORKLOADS = {"peptides": (4096, 16384, (5, 30)), "medium": (256, 256, (256, 256)), "long": (64, 64, (1024, 1024))}


def random_set(rng, n, span, sort):
    lens = rng.integers(span[0], span[1] + 1, n)
    if sort:
        lens = np.sort(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return rng.integers(0, 20, int(off[-1])).astype(np.uint8), off, lens


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default=",".join(WORKLOADS), help="comma-separated subset of " + ", ".join(WORKLOADS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    a.workloads = a.workloads.split(",")
    for w in a.workloads:
        if w not in WORKLOADS:
            ap.error(f"unknown workload {w!r}")
    return a


def main(argv=None):
    a = parse_args(argv)
    __graft_entry__.load_package()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from e3diff_amd import ops, similarity
    subst = similarity.blosum62().to(DEV)
    rng = np.random.default_rng(0)
    result = {"gap_open": 11, "gap_extend": 1, "repeats": a.repeats, "workloads": {}}
    for name in a.workloads:
        n_q, n_t, span = WORKLOADS[name]
        qc, qo, ql = random_set(rng, n_q, span, sort=False)
        tc, to, tl = random_set(rng, n_t, span, sort=True)
        dev = [torch.from_numpy(x).to(DEV) for x in (qc, qo, tc, to)]
        out = tuple(torch.empty((n_q, n_t), dtype=torch.int32, device=DEV) for _ in range(3))
        run = lambda: ops.align_pairs(*dev, subst, 11, 1, out=out, long_queries=int((ql > ops.ALIGN_STRIP).sum()))  # noqa: E731
        run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            run()
            end.record()
            end.synchronize()
            ms.append(start.elapsed_time(end))
        cells = int(ql.sum()) * int(tl.sum())
        med = float(np.median(ms))
        assert int(out[0].min()) >= 0                                  # every pair was computed
        result["workloads"][name] = {"queries": n_q, "targets": n_t, "lengths": list(span), "cells": cells,
                                     "ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
                                     "cell_updates_per_s": cells / (med * 1e-3), "score_sum": int(out[0].sum())}
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
