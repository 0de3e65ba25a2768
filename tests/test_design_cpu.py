"""CPU: the host side of the sequence design controls -- ``DesignControls`` parsing, the variables the entry points read
at import, the three new C-ABI symbols, tests/design_ref.py itself, and that a chain without controls never touches the
new launches (the product's ``ops`` replaced by a stub that refuses them)."""
import math
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import design_ref as DR
import sampler_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("e3d_discrete_posterior_sample_ctl", "e3d_keyed_discrete_posterior_sample_ctl", "e3d_discrete_final_pick")
VOCAB = "ACDEFGHIKLMNPQRSTVWY"
NEG = -math.inf


def ix(letters):
    return [VOCAB.index(a) for a in letters]


def batch_of(lengths, L=8, C=20):
    mask = (torch.arange(L)[None] < torch.tensor(lengths)[:, None]).float()
    return {"ligand_seq": torch.zeros(len(lengths), L, C), "ligand_attn_mask": mask}


# ------------------------------------------------------------------------------------------------ DesignControls
def test_nothing_set_is_inactive(pkg):
    from e3diff_amd.design import DesignControls
    assert pkg.DesignControls is DesignControls and "design" in pkg.__all__
    for c in (DesignControls.build((2, 8, 20)), DesignControls.build(batch_of([5, 2])),
              DesignControls.build((2, 8, 20), temperature=1.0, omit="", allow="", bias=None),
              DesignControls.build((2, 8, 20), bias=torch.zeros(20)), DesignControls.build((2, 8, 20), allow={})):
        assert c.bias is None and not c.active and c.inv_temp == np.float32(1) and c.inv_temp.dtype == np.float32
    t = DesignControls.build((2, 8, 20), temperature=0.7)
    assert t.active and t.bias is None and t.inv_temp.dtype == np.float32
    assert t.inv_temp == np.float32(1) / np.float32(0.7)


def test_omit(pkg):
    from e3diff_amd.design import DesignControls
    c = DesignControls.build((2, 8, 20), omit="CM")
    assert c.active and c.bias.shape == (2, 8, 20) and c.bias.dtype == torch.float32 and c.bias.is_contiguous()
    closed = torch.zeros(20, dtype=torch.bool)
    closed[ix("CM")] = True
    assert (c.bias[..., closed] == NEG).all() and (c.bias[..., ~closed] == 0).all()
    assert torch.equal(DesignControls.build((2, 8, 20), omit=" mc ").bias, c.bias)          # case and blanks
    with pytest.raises(ValueError, match="'X'"):
        DesignControls.build((2, 8, 20), omit="CX")
    with pytest.raises(TypeError):
        DesignControls.build((2, 8, 20), omit=["C"])


def test_allow_in_its_three_forms(pkg):
    from e3diff_amd.design import DesignControls, parse_allow
    assert parse_allow("") == {} and parse_allow(" 3 : LIV ; 7:DE ") == {3: "LIV", 7: "DE"}
    for bad in ("3", "3:", ":LIV", "x:LIV", "3:LIV;;7:DE", "3:LIV;3:DE", "-1:L"):
        with pytest.raises(ValueError):
            parse_allow(bad)
    batch = batch_of([5, 2])
    forms = ("3:LIV;1:DE", {3: "LIV", 1: "DE"}, lambda i: {3: "LIV", 1: "DE"})
    got = [DesignControls.build(batch, allow=f).bias for f in forms]
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
    b = got[0]
    open3 = torch.zeros(20, dtype=torch.bool)
    open3[ix("LIV")] = True
    assert (b[0, 3, open3] == 0).all() and (b[0, 3, ~open3] == NEG).all()
    assert (b[1, 3] == 0).all(), "position 3 is beyond the second ligand's length: ignored"
    assert (b[:, 1, ix("DE")] == 0).all() and (b[:, 1] == NEG).sum() == 2 * 18
    assert (b[:, [0, 2, 4, 5, 6, 7]] == 0).all()
    # a callable sees the dataset index: first_index + b
    seen = []
    per_item = DesignControls.build(batch, allow=lambda i: seen.append(i) or {0: VOCAB[i % 20]}, first_index=40).bias
    assert seen == [40, 41]
    assert (per_item[0, 0] == 0).nonzero().flatten().tolist() == [0] and (per_item[1, 0] == 0).nonzero().flatten().tolist() == [1]
    # positions beyond every ligand: nothing is set
    assert DesignControls.build(batch, allow="6:A").bias is None and not DesignControls.build(batch, allow="6:A").active
    with pytest.raises(ValueError, match="'Z'"):
        DesignControls.build(batch, allow="1:LZ")
    with pytest.raises(ValueError):
        DesignControls.build(batch, allow={-1: "L"})
    with pytest.raises(TypeError):
        DesignControls.build(batch, allow=3)


def test_bias_forms(pkg):
    from e3diff_amd.design import DesignControls
    B, L, C = 2, 8, 20
    d = DesignControls.build((B, L, C), bias={"A": 1.5, "w": -2.0}).bias
    row = torch.zeros(C)
    row[ix("A")], row[ix("W")] = 1.5, -2.0
    assert torch.equal(d, row.expand(B, L, C))
    g = torch.Generator().manual_seed(0)
    for shape in ((C,), (L, C), (B, L, C)):
        t = torch.randn(shape, generator=g)
        got = DesignControls.build((B, L, C), bias=t.double()).bias
        assert got.dtype == torch.float32 and torch.equal(got, t.expand(B, L, C)) and got.is_contiguous()
    # together with omit and allow: forbidden wins, the rest keeps the bias
    both = DesignControls.build((B, L, C), omit="C", allow={2: "AC"}, bias={"A": 1.5, "C": 3.0}).bias
    assert both[0, 0, ix("A")[0]] == 1.5 and both[0, 0, ix("C")[0]] == NEG
    assert (both[0, 2] != NEG).nonzero().flatten().tolist() == ix("A") and both[0, 2, 0] == 1.5
    # -inf in a bias forbids; NaN and +inf are refused, and so are other shapes and keys
    t = torch.zeros(C)
    t[3] = NEG
    assert (DesignControls.build((B, L, C), bias=t).bias[..., 3] == NEG).all()
    for bad in (torch.full((C,), float("nan")), torch.full((C,), math.inf), torch.zeros(C + 1), torch.zeros(B, C), [0.0] * C,
                {"AC": 1.0}, {"X": 1.0}):
        with pytest.raises(ValueError):
            DesignControls.build((B, L, C), bias=bad)


def test_a_position_left_with_no_class_is_refused_with_item_and_position(pkg):
    from e3diff_amd.design import DesignControls
    batch = batch_of([5, 2])
    with pytest.raises(ValueError, match=r"item 0, position 3\b"):
        DesignControls.build(batch, omit="LIV", allow={3: "LIV"})
    with pytest.raises(ValueError, match=r"item 11, position 1\b"):
        DesignControls.build(batch, omit="DE", allow=lambda i: {1: "DE"} if i == 11 else {}, first_index=10)
    # the same position beyond the ligand's length: ignored, hence fine
    assert DesignControls.build(batch_of([3, 2]), omit="LIV", allow={3: "LIV"}).active
    with pytest.raises(ValueError, match=r"item 0, position 0\b"):
        DesignControls.build(batch, bias=torch.full((20,), NEG))
    with pytest.raises(ValueError, match=r"item 1, position 1\b"):
        t = torch.zeros(2, 8, 20)
        t[1, 1] = NEG
        t[1, 2] = NEG                  # position 2 of a ligand of length 2 is padding: only position 1 counts
        DesignControls.build(batch, bias=t)


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, math.inf, -math.inf, math.nan, 1e-46, 1e39, "warm", None])
def test_bad_temperature(pkg, bad):
    from e3diff_amd.design import DesignControls
    with pytest.raises(ValueError, match="temperature"):
        DesignControls.build((1, 4, 20), temperature=bad)


def test_in_frame_moves_the_bias_like_the_state(pkg):
    from e3diff_amd.design import DesignControls
    c = DesignControls.build((2, 8, 20), temperature=2.0, omit="C")
    f = c.in_frame(lambda t: t[:, :4], "cpu")
    assert f.bias.shape == (2, 4, 20) and f.bias.is_contiguous() and f.inv_temp == c.inv_temp and f.active
    assert DesignControls.build((2, 8, 20), temperature=2.0).in_frame(lambda t: 1 / 0, "cpu").bias is None


# ------------------------------------------------------------------------------------------------ entry points
def test_entry_point_variables_are_read_at_import():
    code = ("import __graft_entry__ as g; g.load_package(); from e3diff_amd.sequence_model import sample as Q; "
            "print(repr((Q.TEMPERATURE, Q.OMIT, Q.ALLOW)))")
    env = {k: v for k, v in os.environ.items() if not k.startswith("E3D_SAMPLE_")}
    for extra, want in (({}, (None, "", "")),
                        ({"E3D_SAMPLE_TEMPERATURE": "0.7", "E3D_SAMPLE_OMIT": "CM", "E3D_SAMPLE_ALLOW": "3:LIV;7:DE"},
                         (0.7, "CM", "3:LIV;7:DE"))):
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, **extra), capture_output=True, text=True,
                             timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.strip().splitlines()[-1] == repr(want)


def test_batch_controls_takes_the_defaults_and_the_keywords(pkg, monkeypatch):
    from e3diff_amd.sequence_model import sample as Q
    batch = batch_of([5, 2])
    for name, value in (("TEMPERATURE", None), ("OMIT", ""), ("ALLOW", "")):
        monkeypatch.setattr(Q, name, value)
    assert Q.batch_controls(batch, 0) is None
    assert Q.batch_controls(batch, 0, temperature=1.0) is None            # nothing to apply
    c = Q.batch_controls(batch, 0, omit="CM")
    assert c.active and (c.bias[..., ix("CM")] == NEG).all() and c.inv_temp == np.float32(1)
    monkeypatch.setattr(Q, "OMIT", "W")
    monkeypatch.setattr(Q, "TEMPERATURE", 0.5)
    monkeypatch.setattr(Q, "ALLOW", "1:DE")
    c = Q.batch_controls(batch, 0)
    assert c.inv_temp == np.float32(2) and (c.bias[..., ix("W")] == NEG).all() and (c.bias[:, 1, ix("DE")] == 0).all()
    c = Q.batch_controls(batch, 0, omit="C", allow=lambda i: {}, temperature=1.0)     # the keywords win
    assert c.inv_temp == np.float32(1) and (c.bias[..., ix("W")] == 0).all() and (c.bias[:, 1, ix("A")] == 0).all()
    import inspect
    params = inspect.signature(Q.run).parameters
    assert [params[k].default for k in ("temperature", "omit", "allow", "scores")] == [None, None, None, False]
    assert "controls" in inspect.signature(Q.denoise).parameters and "details" in inspect.signature(Q.denoise).parameters
    assert "controls" in inspect.signature(Q.sample_p_zs_given_zt_discrete).parameters
    assert "controls" in inspect.signature(Q.GraphedDenoiseStep.__init__).parameters


# ------------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_are_declared_bound_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "e3d_hip.h")).read()
    declared = set(re.findall(r"\b(e3d_[a-z0-9_]+)\s*\(", header))
    lib = pkg.hip.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg.hip.EXPORTS, name
        assert getattr(lib, name) is not None
    for name in ("discrete_posterior_sample_ctl", "keyed_discrete_posterior_sample_ctl", "discrete_final_pick"):
        assert callable(getattr(pkg.ops, name))
    assert pkg.hip.ABI_VERSION == 5 and lib.e3d_abi_version() == 5
    # argument validation happens before any launch: callable without a GPU
    x = 16                                                          # a non-null address that is never read
    assert lib.e3d_discrete_posterior_sample_ctl(None, None, None, 1.0, None, None, None, 0, None, None, 1, 4, 20, None) < 0
    assert b"discrete_posterior_ctl" in lib.e3d_last_error()
    assert lib.e3d_keyed_discrete_posterior_sample_ctl(None, None, None, 1.0, None, None, None, 1, None, None, 1, 4, 20, None) < 0
    assert b"keyed_discrete_posterior_ctl" in lib.e3d_last_error()
    assert lib.e3d_discrete_final_pick(None, None, 1.0, None, None, None, 4, 20, None) < 0
    assert b"discrete_final_pick" in lib.e3d_last_error()
    for C in (0, 33):
        assert lib.e3d_discrete_posterior_sample_ctl(x, x, None, 1.0, x, x, None, 0, x, None, 1, 4, C, None) < 0
        assert b"C must be in [1,32]" in lib.e3d_last_error()
        assert lib.e3d_keyed_discrete_posterior_sample_ctl(x, x, None, 1.0, x, x, x, 1, x, x, 1, 4, C, None) < 0
        assert b"C must be in [1,32]" in lib.e3d_last_error()
        assert lib.e3d_discrete_final_pick(x, None, 1.0, x, None, None, 4, C, None) < 0
        assert b"C must be in [1,32]" in lib.e3d_last_error()
    for bad in (0.0, -1.0, math.inf, math.nan):
        assert lib.e3d_discrete_posterior_sample_ctl(x, x, None, bad, x, x, None, 0, x, None, 1, 4, 20, None) < 0
        assert b"inv_temp" in lib.e3d_last_error()
        assert lib.e3d_keyed_discrete_posterior_sample_ctl(x, x, None, bad, x, x, x, 1, x, x, 1, 4, 20, None) < 0
        assert b"inv_temp" in lib.e3d_last_error()
        assert lib.e3d_discrete_final_pick(x, None, bad, x, None, None, 4, 20, None) < 0
        assert b"inv_temp" in lib.e3d_last_error()
    assert lib.e3d_discrete_posterior_sample_ctl(x, x, None, 1.0, x, x, None, 1, x, None, 1, 4, 20, None) < 0
    assert b"mode 1 needs uniforms" in lib.e3d_last_error()


# ------------------------------------------------------------------------------------------------ the reference itself
def test_effective_logits_are_an_add_then_a_multiply_in_fp32():
    rng = np.random.default_rng(0)
    lg = (3 * rng.standard_normal((50, 20))).astype(np.float32)
    b = DR.bias_inputs(50, 20)
    for T in DR.TEMPERATURES + (0.7,):
        it = DR.inv_temp(T)
        z = DR.effective_logits(lg, b, it)
        assert z.dtype == np.float32 and np.array_equal(np.isneginf(z), np.isneginf(b))
        want = ((lg.astype(np.float64) + b.astype(np.float64)).astype(np.float32).astype(np.float64) * np.float64(it)).astype(np.float32)
        assert np.array_equal(z.view(np.int32), want.view(np.int32))
    assert np.array_equal(DR.effective_logits(lg, None, np.float32(1)).view(np.int32), (lg + np.float32(0)).view(np.int32))
    # a third of the classes closed, never a row
    share = np.isneginf(DR.bias_inputs(1000, 20)).mean()
    assert 0.25 < share < 0.4 and np.abs(b[np.isfinite(b)]).max() <= 4.0


def test_final_pick_reference_against_torch_in_float64():
    for rows, C in ((255, 3), (257, 20), (100, 32)):
        lg, b = DR.pick_inputs(rows, C)
        z = DR.effective_logits(lg, b, DR.inv_temp(0.5))
        z[5] = -np.inf                                              # an all-forbidden row
        idx, logp, ent = DR.final_pick(z)
        t = torch.from_numpy(z).double()
        assert idx[5] == 0 and np.isnan(logp[5]) and np.isnan(ent[5])
        live = np.arange(rows) != 5
        ls = torch.log_softmax(t[live], dim=-1)
        assert np.array_equal(idx[live], t[live].argmax(-1).numpy())
        assert np.abs(logp[live] - ls.gather(1, torch.from_numpy(idx[live])[:, None])[:, 0].numpy()).max() < 1e-12
        want = -torch.where(ls.exp() > 0, ls.exp() * ls, torch.zeros((), dtype=torch.float64)).sum(-1).numpy()
        assert np.abs(ent[live] - want).max() < 1e-12 and (ent[live] >= 0).all() and (ent[live] <= np.log(C) + 1e-12).all()
        # rows with their maximum twice: the first one is picked
        tie = [n for n in range(0, rows, 7) if n != 5 and (z[n] == z[n].max()).sum() >= 2]
        assert len(tie) >= rows // 14 and all(idx[n] == int(np.flatnonzero(z[n] == z[n].max())[0]) for n in tie)
        fin = np.where(np.isfinite(z), z.astype(np.float64), np.nan)
        assert np.array_equal(DR.spread(z)[live], (np.nanmax(fin[live], 1) - np.nanmin(fin[live], 1))) and DR.spread(z)[5] == 0


def test_posterior_reference_takes_forbidden_classes():
    """sampler_ref.posterior fed effective logits with -inf entries: finite, rows summing to 1, and independent of the
    logit under a forbidden class."""
    B, L, C = 2, 5, 20
    xt, logits, Qsb, Qtb = R.posterior_inputs(B, L, C)
    b = DR.bias_inputs(B * L, C).reshape(B, L, C)
    z = DR.effective_logits(logits, b, DR.inv_temp(2.0))
    ref = R.posterior(xt, z, Qsb, Qtb)
    assert np.isfinite(ref).all() and np.abs(ref.sum(-1) - 1).max() < 1e-12
    other = np.where(np.isneginf(b), np.float32(123.0), logits)
    assert np.array_equal(ref, R.posterior(xt, DR.effective_logits(other, b, DR.inv_temp(2.0)), Qsb, Qtb))


# ------------------------------------------------------------------------------------------------ no controls: the old launches
class _Refusing(types.SimpleNamespace):
    """Stands in for the product's ``ops``: the launches a chain without controls makes are served in torch on the CPU,
    every other attribute -- the design-control launches among them -- raises."""

    def __getattr__(self, name):
        raise AssertionError(f"a chain without controls touched ops.{name}")


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, s, x, ang, lmask, rseq, rang, rmask):
        g = torch.Generator().manual_seed(int(s[0, 0]))
        return torch.randn(x.shape, generator=g) + 2 * x


def test_denoise_without_controls_does_not_touch_the_new_ops(pkg, monkeypatch):
    from e3diff_amd.design import DesignControls
    from e3diff_amd.sequence_model import sample as Q
    calls = []

    def posterior(xt_idx, logits, qsb, qtb, u=None, want_prob=False):
        calls.append("discrete_posterior_sample")
        return logits.argmax(dim=-1).to(torch.int32)

    monkeypatch.setattr(Q, "ops", _Refusing(discrete_posterior_sample=posterior))
    B, L, C, T = 2, 8, 20, 3
    g = torch.Generator().manual_seed(1)
    mask = (torch.arange(L)[None] < torch.tensor([5, 2])[:, None]).float()
    batch = {"ligand_seq": torch.nn.functional.one_hot(torch.randint(0, C, (B, L), generator=g), C).float() * mask[..., None],
             "ligand_attn_mask": mask, "ligand_angles": torch.zeros(B, L, 8), "receptor_seq": torch.zeros(B, L, C),
             "receptor_angles": torch.zeros(B, L, 8), "receptor_attn_mask": mask}
    sched = types.SimpleNamespace(get_alpha_bar=lambda t_normalized: t_normalized)
    trans = types.SimpleNamespace(get_Qt_bar=lambda ab, dev: torch.eye(C).expand(B, C, C))
    x_T = torch.nn.functional.one_hot(torch.randint(0, C, (B, L), generator=g), C).float()
    kw = dict(x_T=x_T, timesteps=T, use_graph=False)
    base = Q.denoise(batch, _Model(), sched, trans, False, **kw)
    assert calls == ["discrete_posterior_sample"] * (T - 1)
    assert [len(s) for s in base[2]] == [5, 2]
    for controls in (None, DesignControls.build(batch), DesignControls.build(batch, temperature=1.0, omit="", allow="6:A")):
        got = Q.denoise(batch, _Model(), sched, trans, False, controls=controls, **kw)
        assert got == base
    assert calls == ["discrete_posterior_sample"] * (4 * (T - 1))
    # and with controls the stub is asked for the new launches: the refusal shows that the switch is taken
    with pytest.raises(AssertionError, match="discrete_posterior_sample_ctl"):
        Q.denoise(batch, _Model(), sched, trans, False, controls=DesignControls.build(batch, omit="C"), **kw)
    with pytest.raises(AssertionError, match="discrete_final_pick"):
        Q.denoise(batch, _Model(), sched, trans, False, details={}, **kw)
    with pytest.raises(ValueError, match="details"):
        Q.denoise(batch, _Model(), sched, trans, False, details=[], **kw)
    with pytest.raises(ValueError, match="built for"):
        Q.denoise(batch, _Model(), sched, trans, False, controls=DesignControls.build((B, L + 1, C), omit="C"), **kw)
