"""bench.py --dump-outputs: the headline loop's last output on disk, the same from run to run for the same arguments;
what a plain run reports and what --full adds."""
import argparse
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("e3d_bench", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float32_and_samples_fixed_rows_above_the_cap(tmp_path, monkeypatch):
    bench = _bench_module()
    t = torch.arange(10 * 4 * 3, dtype=torch.float64).reshape(10, 4, 3)
    bench.dump_outputs(str(tmp_path / "all"), {"x_next": t})
    a = np.load(tmp_path / "all" / "x_next.npy")
    assert a.dtype == np.float32 and a.shape == (10, 4, 3) and np.array_equal(a, t.float().numpy())
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 * 4 * 3 * 4)        # room for 3 of the 10 rows
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), {"x_next": t})
    s1, s2 = np.load(tmp_path / "s1" / "x_next.npy"), np.load(tmp_path / "s2" / "x_next.npy")
    assert s1.shape == (3, 4, 3) and s1.nbytes <= bench.DUMP_BYTES and np.array_equal(s1, s2)
    rows = [int(r[0, 0]) // 12 for r in s1]
    assert rows == sorted(rows) and len(set(rows)) == 3 and np.array_equal(s1, t.float().numpy()[rows])


def test_headline_line_reports_the_timed_steps_of_all_ranks():
    bench = _bench_module()
    args = argparse.Namespace(batch=4, seq_len=64, steps=5, warmup=2, gemm_mode="f16x3")
    out = bench.headline_line(args, 2, 0.25)       # 5 steps of 2 ranks x 4 pockets in 0.25 s (slowest rank)
    assert out["metric"] == "denoising-steps/sec (batched pocket graphs)" and out["unit"] == "pocket-steps/s"
    assert out["value"] == 4 * 2 * 5 / 0.25 and out["ms_per_step"] == 50.0 and out["higher_is_better"] is True
    assert out["n_gpus"] == 2 and out["steps"] == 5 and out["warmup"] == 2
    assert out["dtype"] == "f32 storage and accumulation, f16x3 products (fp32 grade)"


def test_bench_rejects_zero_timed_steps():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step_identically_for_the_same_arguments(tmp_path):
    """Two runs with the same arguments: K timed steps reported, ms_per_step in the line, and the dumped next state
    [batch, seq-len, 8] of the headline loop's last step agrees between the runs (wrapped angles)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4",
                            "--seq-len", "64", "--headline-only", "--no-cpu-baseline", "--dump-outputs", str(d)],
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        out = json.loads(lines[0])
        assert out["steps"] == 3 and out["ms_per_step"] > 0
        a = np.load(d / "x_next.npy")
        assert a.dtype == np.float32 and a.shape == (4, 64, 8) and np.isfinite(a).all()
        dumps.append(a)
    diff = np.abs(np.remainder(dumps[0] - dumps[1] + math.pi, 2 * math.pi) - math.pi)
    assert diff.max() < 1e-4, diff.max()


@pytest.mark.gpu
def test_plain_bench_run_reports_the_headline_and_full_adds_the_other_figures():
    """A plain run's line holds the headline keys and none of the extra legs' figures; --full prints the same keys and
    adds the other figures (the training, single-pocket, joint and CPU legs left out here: they run at sizes of their own)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    small = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4", "--seq-len", "64"]
    lines = []
    for extra in ([], ["--full", "--no-cpu-baseline", "--no-train-leg"]):
        r = subprocess.run([sys.executable, BENCH] + small + extra, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        found = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(found) == 1, r.stdout
        lines.append(json.loads(found[0]))
    plain, full = lines
    headline = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}
    extras = {"value_by_gemm_mode", "value_encoder_cached", "value_padding_skip", "value_trimmed", "ms_per_step_after_extras",
              "roofline", "roofline_attention", "roofline_gemm_layernorm", "roofline_gemm", "gemm_shapes"}
    assert headline <= set(plain) and not extras & set(plain), sorted(plain)
    assert set(plain) <= set(full) and extras <= set(full), sorted(full)
    assert plain["value"] > 0 and full["value"] > 0 and plain["steps"] == full["steps"] == 2
    assert {"f32", "bf16x3", "bf16x6", "f16x3"} <= set(full["value_by_gemm_mode"])
    assert not {"train", "single_pocket", "joint", "cpu_baseline"} & set(full)
