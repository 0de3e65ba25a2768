"""CPU: scoring supplied sequences -- tests/score_ref.py itself (KL >= 0 and == 0 at the true residue, the level sets
and their weight, the prior, the fixed-shape item sum, the keyed forward noising at per-item levels), the three new
C-ABI symbols, the argument checks of ``score_sequences`` (made before any device work: the model is ``None``) and the
command-line tool's parsing."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import sampler_ref as R
import score_ref as SR
from helpers import synthetic_pockets
from test_sampler_ref_cpu import posterior_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("e3d_keyed_discrete_forward_levels", "e3d_discrete_score_rows", "e3d_masked_item_sums")
U = R.U


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("B,L,C", SR.SHAPES)
def test_kl_is_non_negative_and_zero_at_the_true_residue(B, L, C):
    xt, logits, Qsb, Qtb = posterior_case(B, L, C, "blosum" if C == 20 else "random")
    assert SR.spread(logits, C).max() <= SR.MAX_SPREAD             # what tests/test_score_gpu.py's bounds assume
    x0 = SR.score_x0(B, L, C)
    live = x0.reshape(-1) >= 0
    assert live.any() and (~live).any() or B * L == 1
    q, p = SR.q_post(xt, x0, Qsb, Qtb), SR.p_theta(xt, logits, Qsb, Qtb)
    assert np.isnan(q[~live]).all() and np.abs(q[live].sum(-1) - 1).max() < 1e-12 and (q[live] >= 0).all()
    k = SR.kl(q, p)
    assert np.isnan(k[~live]).all() and (k[live] >= -1e-14).all() and k[live].max() > 1e-3      # float64 rounding of C terms
    # the prediction = the one-hot of x0, as far as logits can say it: a +60 gap
    sure = np.zeros((B, L, C), dtype=np.float32)
    np.put_along_axis(sure, np.maximum(x0, 0)[..., None].astype(np.int64), np.float32(60.0), axis=-1)
    p1 = SR.p_theta(xt, sure, Qsb, Qtb)
    k1, bound = SR.kl(q, p1), SR.kl_bound(q, p1, sure, C)
    assert (k1[live] >= -1e-14).all() and (k1[live] <= bound[live]).all(), float((k1[live] / bound[live]).max())
    # and exactly the one-hot: p == q, the KL is 0 to the last bit
    assert np.array_equal(SR.p_theta_from_pred(xt, np.exp(SR.onehot_logits(np.maximum(x0, 0), C)), Qsb, Qtb)[live], q[live])
    assert (SR.kl(q, q)[live] == 0).all()
    # cross-entropy against torch
    ls = torch.log_softmax(torch.from_numpy(logits).double().reshape(-1, C), dim=-1)
    want = -ls[torch.arange(B * L), torch.from_numpy(np.maximum(x0, 0).reshape(-1)).long()].numpy()
    assert np.abs(SR.nll(logits, x0)[live] - want[live]).max() < 1e-12 and np.isnan(SR.nll(logits, x0)[~live]).all()


def test_kl_conventions():
    q = np.array([[0.5, 0.5, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    p = np.array([[0.5, 0.25, 0.25], [0.0, 0.5, 0.5], [0.5, 0.5, 0.0]])
    k = SR.kl(q, p)
    assert abs(k[0] - 0.5 * np.log(2)) < 1e-15 and k[1] == np.inf and abs(k[2] - np.log(2)) < 1e-15
    assert not np.isnan(k).any()


@pytest.mark.parametrize("T", [1, 2, 8, 50])
def test_level_sets_and_their_weight(pkg, T):
    from e3diff_amd.sequence_model.sample import score_levels
    S, w = SR.level_set(T)
    assert S == list(range(T)) and w == (1.0 if T > 1 else 0.0) and score_levels(T) == (S, w)
    for k in sorted({1, 3, T - 1, T} - {0}):
        S, w = SR.level_set(T, k)
        assert score_levels(T, k) == (S, w)
        assert S[0] == 0 and S[1:] == [s for s in range(1, T) if s % k == 0]
        assert w == ((T - 1) / (len(S) - 1) if len(S) > 1 else 0.0)
        assert len(S) == 1 or abs(w * (len(S) - 1) - (T - 1)) < 1e-12       # w x the drawn levels stands for all T - 1
    assert SR.level_set(8, 3) == ([0, 3, 6], 3.5)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="levels"):
            score_levels(8, bad)


def test_prior_against_a_direct_sum(pkg):
    from e3diff_amd.sequence_model.sample import prior_terms
    C = 20
    Q = R.with_exact_zeros(R.row_stochastic(2, C, 3))[0].astype(np.float64)
    x0 = np.array([[0, 5, -1, 19], [7, -1, 3, 3]])
    got = SR.prior(Q, x0)
    for (b, l), c in np.ndenumerate(x0):
        if c < 0:
            assert got[b, l] == 0
            continue
        col = Q[:, c] / Q[:, c].sum()
        want = sum(p * np.log(C * p) for p in col if p > 0)
        assert abs(got[b, l] - want) < 1e-14 and got[b, l] >= 0
    assert (Q == 0).any()
    assert np.abs(prior_terms(torch.from_numpy(Q).float(), torch.from_numpy(x0)).numpy() - SR.prior(Q.astype(np.float32), x0)).max() < 1e-14
    assert np.abs(SR.prior(np.full((C, C), 1.0 / C), x0)).max() < 1e-15           # the uniform law at level 1: nothing
    assert abs(SR.prior(np.eye(C), np.array([3])) - np.log(C)).max() < 1e-15       # no noise at all: log C


@pytest.mark.parametrize("L", [1, 63, 64, 65, 257])
def test_fixed_shape_item_sum(L):
    rng = np.random.default_rng(L)
    v = (rng.standard_normal(L) * 10 ** rng.uniform(-3, 3, L)).astype(np.float32)
    m = rng.random(L) < 0.7
    m[0] = True
    s, n = SR.item_sum_fp32(v, m)
    assert n == int(m.sum()) and s.dtype == np.float32
    assert abs(float(s) - v.astype(np.float64)[m].sum()) <= L * U * np.abs(v[m]).sum()
    # padding to 2 L, whatever stands in the masked-out places
    v2 = np.concatenate([np.where(m, v, np.float32(np.nan)), np.full(L, np.nan, dtype=np.float32)])
    s2, n2 = SR.item_sum_fp32(v2, np.concatenate([m, np.zeros(L, dtype=bool)]))
    assert s2.view(np.int32) == s.view(np.int32) and n2 == n
    assert SR.item_sum_fp32(v, np.zeros(L, dtype=bool)) == (np.float32(0), 0)


def test_forward_levels_reference_is_the_per_step_draw():
    B, L, C = 3, 37, 20
    x0, Qtb = R.discrete_q_inputs(B, L, C)
    ids = R.IDS[:B]
    keys = R.padded_keys(ids, L)
    keys[5] = (9, -1)
    steps = (0, 7, 65535)
    got = SR.forward_levels(x0, Qtb, keys, R.SEEDS[1], steps)
    p32 = R.forward_column(Qtb, x0)
    for b, s in enumerate(steps):
        u = R.keyed_uniforms(keys, R.SEEDS[1], 11, s)
        want = R.pick_fp32(p32, u, 1).reshape(B, L)[b]
        live = (x0[b] >= 0) & (keys.reshape(B, L, 2)[b, :, 1] >= 0)
        assert np.array_equal(got[b][live], want[live]) and (got[b][~live] == 0).all()
    assert got[0, 5] == 0 and (x0 < 0).any() and len(np.unique(got)) > 5


# ------------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_are_declared_bound_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "e3d_hip.h")).read()
    declared = set(re.findall(r"\b(e3d_[a-z0-9_]+)\s*\(", header))
    lib = pkg.hip.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg.hip.EXPORTS, name
        assert getattr(lib, name) is not None
    for name in ("keyed_discrete_forward_levels", "discrete_score_rows", "masked_item_sums"):
        assert callable(getattr(pkg.ops, name))
    assert pkg.hip.ABI_VERSION == 5 and lib.e3d_abi_version() == 5
    assert pkg.score_sequences is __import__("e3diff_amd.sequence_model.sample", fromlist=["x"]).score_sequences
    assert "score_sequences" in pkg.__all__
    # argument validation happens before any launch: callable without a GPU
    x = 16                                                          # a non-null address that is never read
    assert lib.e3d_keyed_discrete_forward_levels(None, None, None, None, 7, 1, None, 1, 4, 20, None) < 0
    assert b"keyed_discrete_forward_levels" in lib.e3d_last_error()
    assert lib.e3d_discrete_score_rows(None, None, None, None, None, None, None, None, None, None, 1, 4, 20, None) < 0
    assert b"discrete_score_rows" in lib.e3d_last_error()
    assert lib.e3d_masked_item_sums(None, None, None, None, 1, 4, None) < 0
    assert b"masked_item_sums" in lib.e3d_last_error()
    for C in (1, 33):
        assert lib.e3d_keyed_discrete_forward_levels(x, x, x, x, 7, 1, x, 1, 4, C, None) < 0
        assert b"keyed_discrete_forward_levels: C must be in [2,32]" in lib.e3d_last_error()
        assert lib.e3d_discrete_score_rows(x, x, x, x, x, x, x, x, None, None, 1, 4, C, None) < 0
        assert b"discrete_score_rows: C must be in [2,32]" in lib.e3d_last_error()
    for step in (65536, -1):
        assert lib.e3d_keyed_discrete_forward_levels(x, x, x, x, step, 1, x, 1, 4, 20, None) < 0
        assert b"steps up to 65535" in lib.e3d_last_error()
    assert lib.e3d_keyed_discrete_forward_levels(x, x, x, x, 7, 1, x, 1, (1 << 24) + 1, 20, None) < 0
    assert b"below 2^24" in lib.e3d_last_error()
    for N, L in ((0, 4), (1, 0)):
        assert lib.e3d_masked_item_sums(x, x, x, x, N, L, None) < 0
        assert lib.e3d_discrete_score_rows(x, x, x, x, x, x, x, x, None, None, N, L, 20, None) < 0
    streams = re.findall(r"#define\s+(\w*STREAM\w*)\s", open(os.path.join(ROOT, "e3-invaraint-diffusion-model_amd", "csrc",
                                                                        "e3d_philox.h")).read())
    assert len(streams) == 12                                        # the score draws stream 11: no stream was added


# ------------------------------------------------------------------------------------------------ score_sequences: argument checks
def test_score_sequences_checks_its_arguments_before_any_device_work(pkg):
    from e3diff_amd.sequence_model.dataset import AA_VOCAB as VOCAB
    from e3diff_amd.sequence_model.sample import score_sequences, sequence_indices
    B, L = 3, 16
    batch = synthetic_pockets(B, L, seed=1, lig_range=(3, 9), with_ligand_seq=True)
    lengths = [int(n) for n in batch["ligand_attn_mask"].sum(dim=1)]
    native = ["".join(VOCAB[j] for j in batch["ligand_seq"][b, :lengths[b]].argmax(-1)) for b in range(B)]
    idx = sequence_indices(native, batch["ligand_attn_mask"])
    assert idx.dtype == torch.int32 and torch.equal(idx >= 0, batch["ligand_attn_mask"] != 0)
    assert torch.equal(idx.clamp_min(0), (batch["ligand_seq"].argmax(-1) * (batch["ligand_attn_mask"] != 0)).int())

    def score(sequences=native, **kw):
        kw.setdefault("timesteps", 8)
        return score_sequences(batch, None, None, None, sequences, **kw)      # no model: nothing below may reach it
    with pytest.raises(ValueError, match=f"item 1 has a ligand of {lengths[1]} residues"):
        score([native[0], native[1] + "A", native[2]], seed=1)
    with pytest.raises(ValueError, match="item 2 has a ligand"):
        score([native[0], native[1], native[2][:-1]], seed=1)
    with pytest.raises(ValueError, match="list of 3 strings"):
        score(native[:2], seed=1)
    with pytest.raises(ValueError, match="list of 3 strings"):
        score("ACD", seed=1)
    with pytest.raises(ValueError, match="item 0: letters 'X' are outside the vocabulary"):
        score(["X" + native[0][1:], native[1], native[2]], seed=1)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        score([native[0].lower(), native[1], native[2]], seed=1)
    with pytest.raises(ValueError, match="item_ids key the seeded draws"):
        score(item_ids=[1, 2, 3])
    with pytest.raises(ValueError, match="either injected us or a seed"):
        score(seed=1, us=torch.zeros(8, B, L))
    with pytest.raises(ValueError, match="us must be a tensor of"):
        score(us=torch.zeros(7, B, L))
    with pytest.raises(ValueError, match="levels"):
        score(seed=1, levels=0)
    with pytest.raises(ValueError, match="details must be a dict"):
        score(seed=1, details=[])
    with pytest.raises(ValueError, match="single seed"):
        score(seed=[1, 2], details={})
    with pytest.raises(ValueError, match="score_mask must be a bool tensor"):
        score(seed=1, score_mask=torch.ones(B, L))
    with pytest.raises(ValueError, match="levels_per_launch"):
        score(seed=1, levels_per_launch=0)
    with pytest.raises(ValueError, match="seed must lie in"):
        score(seed=[1, -2])
    with pytest.raises(AttributeError):                              # every check passed: the model is asked for its device
        score(seed=1)
    import inspect
    params = inspect.signature(score_sequences).parameters
    assert list(params) == ["batch", "model", "noise_schedule", "transition", "sequences", "levels", "seed", "item_ids", "us",
                            "generated_angles", "score_mask", "trim_padding", "timesteps", "levels_per_launch", "details"]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(params)[5:]) and "pack" not in params
    from e3diff_amd.sequence_model import sample_by_generated_angles as J
    assert list(inspect.signature(J.score_sequences).parameters)[:2] == ["batch", "generated_angles"]


# ------------------------------------------------------------------------------------------------ the tool
def load_tool():
    """tools/score_sequences.py as a module (tests/test_score_gpu.py runs its ``main``)."""
    spec = importlib.util.spec_from_file_location("score_sequences_tool", os.path.join(ROOT, "tools", "score_sequences.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tool():
    return load_tool()


def test_tool_parses_its_arguments(tool, capsys):
    base = ["--data", "biolip.pt", "--model", "m.ckpt", "-o", "scores.json"]
    a = tool.parse_args(base + ["--native"])
    assert a.native and a.table is None and a.fasta is None and a.seeds == [0] and a.levels is None
    assert a.transition == "blosum" and a.split == "test"
    a = tool.parse_args(base[:-1] + ["s.pkl", "--table", "out.pkl", "--seeds", "1,2,0x10", "--levels", "5", "--transition", "uniform"])
    assert a.table == "out.pkl" and a.seeds == [1, 2, 16] and a.levels == 5 and a.transition == "uniform" and a.output == "s.pkl"
    for bad, text in ((base, "one of the arguments --table --fasta --native is required"),
                      (base + ["--native", "--fasta", "x.fa"], "not allowed with"),
                      (base + ["--native", "--seeds", "1,x"], "seeds must be integers"),
                      (base + ["--native", "--seeds", ""], "one or more integers"),
                      (base + ["--native", "--seeds", "3,3"], "given twice"),
                      (base + ["--native", "--seeds", "-1"], "one or more integers"),
                      (base + ["--native", "--levels", "0"], "positive integer"),
                      (base[:-1] + ["scores.csv", "--native"], ".json or .pkl"),
                      (["--native", "-o", "s.json", "--model", "m"], "--data")):
        with pytest.raises(SystemExit) as stop:
            tool.parse_args(bad)
        assert stop.value.code == 2 and text in capsys.readouterr().err, bad
    with pytest.raises(SystemExit) as stop:
        tool.parse_args(["--help"])
    text = capsys.readouterr().out
    assert stop.value.code == 0
    for word in ("--table", "--fasta", "--native", "--seeds", "--levels", "nats per residue", "not a certified"):
        assert word in text, word


def test_tool_reads_fasta_and_meets_sequences_with_records(tool, tmp_path):
    fa = tmp_path / "d.fa"
    fa.write_text(">1abc_B first design\nACDE\nfg\n\n>2xyz_C\nKLM\n")
    assert tool.read_fasta(str(fa)) == [("1abc_B", "ACDEFG"), ("2xyz_C", "KLM")]
    for text, msg in (("ACD\n>x\nAC\n", "before the first"), ("", "no FASTA record"), (">\nAC\n", "without an id")):
        fa.write_text(text)
        with pytest.raises(ValueError, match=msg):
            tool.read_fasta(str(fa))
    ids, lengths = ["1abc_B", "2xyz_C"], [6, 3]
    recs = [("2xyz_C", "KLM"), ("1abc_B", "ACDEFG"), ("9zzz_A", "AAAA")]
    assert tool.match_sequences(ids, lengths, recs) == ["ACDEFG", "KLM"]
    assert tool.match_sequences(["a_B", "a_B"], [2, 3], [("a_B", "AC"), ("a_B", "ACD")]) == ["AC", "ACD"]     # by position
    for recs, msg in (([("1abc_B", "ACDEFG")], "no sequence for 1 record"),
                      ([("1abc_B", "ACDEFG"), ("2xyz_C", "KL")], "2xyz_C: the ligand has 3 residues, the sequence 2"),
                      ([("1abc_B", "ACDEFB"), ("2xyz_C", "KLM")], "1abc_B: letters 'B'"),
                      ([("2xyz_C", "KLM"), ("2xyz_C", "KLM"), ("1abc_B", "ACDEFG")], "names 2xyz_C twice")):
        with pytest.raises(ValueError, match=msg):
            tool.match_sequences(ids, lengths, recs)
    with pytest.raises(ValueError, match="holds a structure id twice"):
        tool.match_sequences(["a_B", "a_B"], [2, 2], [("a_B", "AC")])
