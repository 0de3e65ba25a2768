"""Packed variable-length sampling against the padded and trimmed frames: one JSON line.

Structure reverse step at bench.py's size (B = 256 pockets, 256-row frame, BioLiP-shaped ligands of 5-30 and pockets
of 20-256 residues, 12 + 12 layers x 768, f16x3): pocket-steps/s of the cached reverse step (pocket encoder and cross
K/V once, as p_sample_loop runs it) on the padded frame, the trimmed frame (p_sample_loop(trim_padding=True)) and the
packed rows (p_sample_loop(pack=True)), eager and replayed from a captured HIP graph; the row counts of each frame; and
the parity of packed against trimmed: one decoder call's predicted noise, and six mid-chain steps with the same injected
noise.  Then the sequence chain at tools/bench_joint.py's size (``sequence_leg``).

    python tools/bench_packed.py [--steps K] [--warmup W]
    python tools/bench_packed.py --leg packed|trimmed --steps K      # only that leg's eager steps (for rocprofv3)
    python tools/bench_packed.py --update strided [--eta E] [--wrap-x0]   # the timed steps run the strided (DDIM) update
    python tools/bench_packed.py --update multistep [--wrap-x0]           # ... the second-order multistep update
    python tools/bench_packed.py --summarize PACKED_STATS.csv TRIMMED_STATS.csv   # attention kernels of two traces

``--summarize`` reads two ``rocprofv3 --kernel-trace --stats`` kernel tables (one run per leg) and prints the attention
kernels' time per step and, for the varlen kernel, the bytes it must move (``varlen_bytes``) over its time as a share
of the HBM peak.
"""
import argparse
import csv
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, L, H, NH, INTER, LAYERS = 256, 256, 768, 12, 1024, 12
HBM_PEAK = 8.0e12          # MI355X HBM3E, bytes/s


def varlen_bytes(q_lengths, k_lengths, rows, relkey, P=L):
    """Bytes one varlen attention call must move at least: Q and the output rows once, each segment's K and V once,
    the distance table once (rel-key), the segment / tile tables (negligible)."""
    hq = H * 4
    b = sum(q_lengths) * hq + rows * hq + 2 * sum(k_lengths) * hq
    if relkey:
        b += (2 * P - 1) * 64 * 4
    return b


def build(device):
    import __graft_entry__
    pkg = __graft_entry__.load_package()
    pkg.hip.lib()
    import torch
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.structure_model.model import ConditionalBertForDiffusionBase
    common = dict(hidden_size=H, num_attention_heads=NH, intermediate_size=INTER, num_hidden_layers=LAYERS,
                  max_position_embeddings=L)
    torch.manual_seed(0)
    model = ConditionalBertForDiffusionBase(BertConfig(**common),
                                            BertConfig(**common, is_decoder=True, add_cross_attention=True), 8)
    with torch.no_grad():   # live adaLN gates, as bench.py
        for se in (model.receptor_emb, model.timestep_emb):
            torch.nn.init.normal_(se.adaLN_modulation[0].weight, std=0.02)
    return model.eval().to(device), pkg


def frames_of(lm, rm):
    """The padded, trimmed and packed frames of a batch, as the samplers build them."""
    from e3diff_amd import packing
    return {"padded": packing.Frame(lm, rm), "trimmed": packing.Frame(lm, rm, trim=True),
            "packed": packing.Frame(lm, rm, pack=True)}


def rows_of(frames):
    """Ligand and pocket rows of each frame."""
    return {k: {"ligand": f.rows, "pocket": f.B * f.Lr if f.layouts is None else f.layouts[1].rows}
            for k, f in frames.items()}


def summarize(packed_csv, trimmed_csv, steps):
    def attn_rows(path):
        out = {}
        with open(path) as f:
            for r in csv.DictReader(f):
                if "attn" in r["Name"] and "bwd" not in r["Name"]:
                    out[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]))
        return out
    p, t = attn_rows(packed_csv), attn_rows(trimmed_csv)
    return {"packed_attention_ns_per_step": sum(v[1] for v in p.values()) / steps,
            "trimmed_attention_ns_per_step": sum(v[1] for v in t.values()) / steps,
            "packed_kernels": {k: {"calls": c, "avg_us": ns / c / 1e3} for k, (c, ns) in p.items()},
            "trimmed_kernels": {k: {"calls": c, "avg_us": ns / c / 1e3} for k, (c, ns) in t.items()}}


def sequence_leg(device, args, B_seq=128, L_seq=128, T_seq=50):
    """The sequence chain at tools/bench_joint.py's size (128 pockets, L = 128, 6 layers, 50 steps, uniform transition,
    categorical draws): pocket-steps/s of ``denoise`` padded / trimmed / packed, the row counts, and an argmax chain
    (T = 6, same initial noise) packed against padded: identical sequences and recovery rates."""
    import contextlib
    import io
    import torch
    from helpers import synthetic_pockets
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.sequence_model.model import PeptideDiff
    from e3diff_amd.sequence_model.sample import denoise, generate_discrete_noise
    from e3diff_amd.sequence_model.utils import DiscreteUniformTransition, PredefinedNoiseScheduleDiscrete
    c = dict(hidden_size=H, num_attention_heads=NH, intermediate_size=INTER, num_hidden_layers=6,
             max_position_embeddings=L_seq, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    torch.manual_seed(0)
    qmodel = PeptideDiff(BertConfig(**c), BertConfig(**c, is_decoder=True, add_cross_attention=True),
                         feature_names=list("ACDEFGHIKLMNPQRSTVWY"), loss_func=torch.nn.CrossEntropyLoss(),
                         noise_schedule="cosine", timesteps=T_seq).eval().to(device)
    pk = dict(synthetic_pockets(B_seq, L_seq, seed=0, with_ligand_seq=True), structure_ids=None)
    sched = PredefinedNoiseScheduleDiscrete("cosine", T_seq).to(device)
    tr = DiscreteUniformTransition(20)
    frames = frames_of(pk["ligand_attn_mask"], pk["receptor_attn_mask"])
    modes = {"padded": {}, "trimmed": {"trim_padding": True}, "packed": {"pack": True}}
    rate = {}
    seeded = {} if args.seed is None else {"seed": args.seed, "item_ids": range(B_seq)}
    quiet = contextlib.redirect_stdout(io.StringIO())    # denoise prints the mean recovery rate
    with quiet:
        for name, kw in modes.items():
            denoise(pk, qmodel, sched, tr, True, timesteps=6, **kw)               # warm-up (first launches, capture)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            denoise(pk, qmodel, sched, tr, True, timesteps=T_seq, **kw, **seeded)
            torch.cuda.synchronize()
            rate[name] = B_seq * T_seq / (time.perf_counter() - t0)
        torch.manual_seed(4)
        x_T = generate_discrete_noise(B_seq, L_seq, 20, device)
        full = denoise(pk, qmodel, sched, tr, False, x_T=x_T, timesteps=6)
        packed = denoise(pk, qmodel, sched, tr, False, x_T=x_T, timesteps=6, pack=True)
    del qmodel
    torch.cuda.empty_cache()
    return {"pockets": B_seq, "frame": L_seq, "steps": T_seq, "layers": 6, "pocket_steps_per_s": rate,
            "speedup_packed_over_trimmed": rate["packed"] / rate["trimmed"],
            "rows": rows_of(frames),
            "argmax_T6_packed_vs_padded_identical_sequences": sum(a == b for a, b in zip(full[2], packed[2])) / B_seq,
            "argmax_T6_packed_vs_padded_identical_recovery": full[3] == packed[3]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--leg", choices=["packed", "trimmed"], default=None)
    ap.add_argument("--summarize", nargs=2, metavar=("PACKED_CSV", "TRIMMED_CSV"), default=None)
    ap.add_argument("--seed", type=int, default=None, help="keyed draws in the timed chains, items keyed 0 .. B-1 "
                    "(default: torch's generator)")
    ap.add_argument("--update", choices=("ancestral", "strided", "multistep"), default="ancestral", help="update kernel of the timed "
                    "structure steps; strided: the DDIM / respaced update, multistep: the second-order multistep update (table of all "
                    "1000 timesteps, as step=1)")
    ap.add_argument("--eta", type=float, default=0.0, help="noise scale of the strided update in [0, 1] (0: deterministic)")
    ap.add_argument("--wrap-x0", action="store_true", help="strided update: wrap the x0 estimate to [-pi, pi)")
    args = ap.parse_args()
    if args.summarize:
        s = summarize(*args.summarize, args.steps)
        import torch  # noqa: F401  (layout of the timed batch: recomputed on the host only)
        from helpers import synthetic_pockets
        pk = synthetic_pockets(B, L, seed=1000)
        ql = [int(n) for n in pk["ligand_length"]]
        kl = [int(n) for n in pk["receptor_length"]]
        rows = max(32, -(-sum(ql) // 32) * 32)
        rows_r = max(32, -(-sum(kl) // 32) * 32)
        # per step: the timestep SELayer's and each decoder layer's self-attention (rel-key) + each layer's cross
        # attention; per run: the pocket encode once (SELayer + 12 encoder layers, rel-key), spread over the steps
        need = ((LAYERS + 1) * varlen_bytes(ql, ql, rows, True) + LAYERS * varlen_bytes(ql, kl, rows, False)
                + (LAYERS + 1) * varlen_bytes(kl, kl, rows_r, True) / args.steps)
        s["varlen_bytes_per_step"] = need
        ns = sum(v["avg_us"] * v["calls"] * 1e3 for k, v in s["packed_kernels"].items() if "varlen" in k) / args.steps
        s["varlen_hbm_share"] = need / (ns * 1e-9) / HBM_PEAK if ns else None
        print(json.dumps(s))
        return

    import torch
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    model, pkg = build(device)
    from helpers import synthetic_pockets
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.utils import CosineTables, MultistepTables, StridedTables, modulo_with_wrapped_range

    pk = {k: v.to(device) for k, v in synthetic_pockets(B, L, seed=1000).items() if torch.is_tensor(v)}
    tab = CosineTables(1000)
    st = StridedTables(tab, list(reversed(range(1000))), args.eta) if args.update == "strided" else None
    ms = MultistepTables(tab, list(reversed(range(1000)))) if args.update == "multistep" else None
    gen = torch.Generator(device=device).manual_seed(0)
    x = modulo_with_wrapped_range(torch.randn(B, L, 8, device=device, generator=gen)).contiguous()
    lm, rm = pk["ligand_attn_mask"], pk["receptor_attn_mask"]
    frames = frames_of(lm, rm)
    lay = frames["packed"].layouts[0]

    def frame(kind):
        """(mask, x, cache, layout) of one frame, as p_sample_loop builds them."""
        f = frames[kind]
        layout, pocket_layout = f.layouts or (None, None)
        if pocket_layout is None:
            cache = model.encode_receptor(f.pocket(pk["receptor_seq"]), f.pocket(pk["receptor_angles"]), f.pocket(rm))
        else:
            cache = model.encode_receptor(pk["receptor_seq"], pk["receptor_angles"], rm, layout=pocket_layout)
        return (None if layout is not None else f.ligand(lm)), f.ligand(x), cache, layout

    mod_table = model.timestep_modulation(torch.arange(1000, device=device)).contiguous()

    def frame_keys(kind):
        """Key table of a frame's rows (--seed), or None."""
        return None if args.seed is None else frames[kind].row_keys(list(range(B)), device)

    def plan_of(kind):
        """The chain's StepPlan on one frame (--update, --eta, --wrap-x0, --seed)."""
        keys = frame_keys(kind)
        return S.step_plan(tab, device, table=True, strided=st, wrap_x0=args.wrap_x0, row_keys=keys,
                           seed=None if keys is None else args.seed, multistep=ms)

    def eager(kind, steps):
        mask, xa, cache, layout = frame(kind)
        plan = plan_of(kind)
        xb = torch.empty_like(xa)
        history = torch.zeros_like(xa) if ms is not None else None      # the multistep chain's x0 history, in the frame
        for k_steps in (args.warmup, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for j in range(k_steps):
                i = 999 - j
                y = S._reverse_step(model, mask, xa, None, None, None, i, tab, None, cache, xb, True,
                                    mod=mod_table[i:i + 1], layout=layout, plan=plan, history=history)
                xa, xb = y, xa
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        return B * steps / dt

    def graphed(kind, steps):
        mask, xa, cache, layout = frame(kind)
        g = S.GraphedReverseStep(model, None if mask is None else mask.contiguous().float(), cache, plan_of(kind), xa,
                                 mod_table=mod_table, layout=layout)
        for k_steps in (args.warmup, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            y = xa
            for j in range(k_steps):
                y = g.step(999 - j, y)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        return B * steps / dt

    if args.leg:
        with torch.no_grad():
            eager(args.leg, args.steps)
        print(json.dumps({"leg": args.leg, "steps": args.steps}))
        return

    out = {"metric": "packed_structure_reverse_step", "unit": "pocket-steps/s", "B": B, "frame": L,
           "update": args.update, "eta": args.eta, "wrap_x0": args.wrap_x0, "rows": rows_of(frames)}
    with torch.no_grad():
        out["eager"] = {k: eager(k, args.steps) for k in ("padded", "trimmed", "packed")}
        out["graph"] = {k: graphed(k, args.steps) for k in ("trimmed", "packed")}
        # parity at the timed size.  (1) The predicted noise of ONE decoder call on every item, packed against trimmed
        # (relative to max |eps|).  (2) Six consecutive steps t = 500 .. 495 of the 1000-step schedule with the same
        # injected noise: mid-chain steps pass an eps difference on with a factor ~beta_t / sqrt(1 - abar_t) < 0.01, so
        # the figure shows packing, not the x100 amplification of the schedule's last step (beta clipped to 0.9999),
        # which makes any two frames of a short T = 6 chain of this random-init model differ by ~0.3 rad.
        t = torch.full((B,), 500, device=device)
        mask_t, xt, cache_t, _ = frame("trimmed")
        eps_t = frames["trimmed"].restore(model.decode(t, xt, mask_t, cache_t))
        _, xp, cache_p, _ = frame("packed")
        eps_p = lay.unpack(model.decode(t, xp, None, cache_p, mod=model.timestep_modulation(t[:1]), layout=lay))
        v = lm.bool()
        out["parity_eps_rel_packed_vs_trimmed"] = ((eps_p - eps_t)[v].abs().max() / eps_t[v].abs().max()).item()
        noises = torch.randn(6, B, L, 8, device=device, generator=gen)

        def chain(kind):
            mask, xa, cache, layout = frame(kind)
            for j in range(6):
                i = 500 - j
                xa = S._reverse_step(model, mask, xa, None, None, None, i, tab, frames[kind].ligand(noises[j]), cache,
                                     None, True, mod=mod_table[i:i + 1], layout=layout)
            return frames[kind].restore(xa)

        d = modulo_with_wrapped_range((chain("packed") - chain("trimmed"))[v]).abs().max().item()
        out["parity_max_wrapped_diff_packed_vs_trimmed_6_steps_t500"] = d
    out["speedup_packed_over_trimmed"] = {"eager": out["eager"]["packed"] / out["eager"]["trimmed"],
                                          "graph": out["graph"]["packed"] / out["graph"]["trimmed"]}
    out["sequence_chain"] = sequence_leg(device, args)
    out["finite"] = all(math.isfinite(v) for v in list(out["eager"].values()) + list(out["graph"].values())
                        + list(out["sequence_chain"]["pocket_steps_per_s"].values()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
