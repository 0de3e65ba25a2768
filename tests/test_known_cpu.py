"""CPU: partial redesign (held ligand positions).  ``KnownLevels`` against the float64 statement (tests/known_ref.py), the
``keep`` position-list parser, streams 10 / 11 on both sides of the C-ABI, the four new exports and their argument checks,
and the interface errors of both samplers that need no device."""
import os
import re

import numpy as np
import pytest
import torch

import known_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "e3-invaraint-diffusion-model_amd")
NEW_SYMBOLS = ("e3d_known_compose_wrap", "e3d_keyed_known_compose_wrap", "e3d_discrete_known_compose",
               "e3d_keyed_discrete_known_compose")


# ------------------------------------------------------------------------------------------------ level table
@pytest.mark.parametrize("T", [6, 1000])
@pytest.mark.parametrize("step", [1, 3, 20])
def test_known_levels_against_the_float64_statement(pkg, T, step):
    from e3diff_amd.structure_model.utils import CosineTables, KnownLevels
    tab = CosineTables(T)
    order = list(reversed(range(0, T, step)))
    kl = KnownLevels(tab, order)
    got = kl.levels.numpy()
    assert got.dtype == np.float32 and got.shape == (T, 2) and kl.order == order
    want = KR.levels(tab.betas.numpy(), order)                     # float64, from the same fp32 betas
    visited = np.zeros(T, dtype=bool)
    visited[order] = True
    assert np.isnan(got[~visited]).all() and np.isfinite(got[visited]).all()
    # one fp32 rounding of the float64 value: half an ulp, i.e. 2^-24 relative (entries lie in (0, 1])
    err = np.abs(got[order].astype(np.float64) - want)
    assert (err <= 2.0 ** -24 * np.abs(want)).all(), (err / np.maximum(np.abs(want), 1e-300)).max()
    assert np.array_equal(got, KR.table(tab.betas.numpy(), order), equal_nan=True)
    # the last visited timestep: the state is the sample itself
    assert got[order[-1], 0] == 1.0 and got[order[-1], 1] == 0.0
    # the table names the level AFTER the step: row order[k] is the forward law's pair at order[k + 1]
    ab = np.cumprod(1.0 - tab.betas.double().numpy())
    for k in range(len(order) - 1):
        s = order[k + 1]
        assert got[order[k], 0] == np.float32(np.sqrt(ab[s])) and got[order[k], 1] == np.float32(np.sqrt(1.0 - ab[s]))
        assert got[order[k], 1] != 0.0                              # only the last row is the clean level


def test_known_levels_refuses_a_bad_order(pkg):
    from e3diff_amd.structure_model.utils import CosineTables, KnownLevels
    tab = CosineTables(6)
    for bad in ([], [0, 3], [5, 5, 0], [6, 0], [3, -1]):
        with pytest.raises(ValueError):
            KnownLevels(tab, bad)


def test_the_kernel_tests_fixed_draws_exclude_nothing():
    """tests/test_known_gpu.py leaves out elements whose scale * z lies within 8 u |scale z| of an odd multiple of pi
    (about 2e-8 of standard normals).  On the float64 statement alone: its fixed seed excludes none, at either scale."""
    n_big = 2048 * 256 * 4 + 5
    _, _, z, mask = KR.kernel_inputs(n_big)
    assert 0.49 < mask.mean() < 0.51 and abs(z.mean()) < 5e-3 and abs(z.std() - 1.0) < 5e-3
    for scale in (1.0, 1.5):
        assert not KR.excluded(scale * z.astype(np.float64)).any()
    # the zone itself: an element on a cut is inside, one a little further away is not
    assert KR.excluded(np.array([np.pi, -3 * np.pi, np.pi * (1 + 4 * KR.U)])).all()
    assert not KR.excluded(np.array([0.0, 2 * np.pi, np.pi * (1 + 16 * KR.U), 3.0])).any()


# ------------------------------------------------------------------------------------------------ keep parser
def test_keep_parser(pkg):
    from e3diff_amd import packing
    assert packing.parse_keep("") == [] and packing.parse_keep("  ") == []
    assert packing.parse_keep("7") == [7]
    assert packing.parse_keep("0-3,7") == [0, 1, 2, 3, 7]
    assert packing.parse_keep(" 2 - 4 , 3, 9-9 ") == [2, 3, 4, 9]
    for bad, token in (("0-3,x", "x"), ("1,,2", ""), ("3-1", "3-1"), ("-2", "-2"), ("1-", "1-"), ("1-2-3", "1-2-3"),
                       ("0x3", "0x3"), ("1.5", "1.5")):
        with pytest.raises(ValueError) as e:
            packing.parse_keep(bad)
        assert repr(token) in str(e.value) or token == "", (bad, str(e.value))
    with pytest.raises(TypeError):
        packing.parse_keep(3)
    m = packing.keep_mask("0-3,7", 0, 16, length=6)                 # positions at or beyond the ligand's length: ignored
    assert m.dtype == torch.bool and m.tolist() == [True] * 4 + [False] * 12
    assert packing.keep_mask("0-3,7", 0, 16).nonzero().flatten().tolist() == [0, 1, 2, 3, 7]
    assert packing.keep_mask("40", 0, 16).sum() == 0 and packing.keep_mask("", 5, 16).sum() == 0
    # a callable: dataset index -> bool [L], cut at the length too
    fn = lambda i: torch.arange(16) % 2 == i % 2   # noqa: E731
    assert packing.keep_mask(fn, 1, 16, length=5).nonzero().flatten().tolist() == [1, 3]
    with pytest.raises(ValueError):
        packing.keep_mask(lambda i: torch.zeros(16), 0, 16)
    with pytest.raises(ValueError):
        packing.keep_mask(lambda i: torch.zeros(8, dtype=torch.bool), 0, 16)


def test_entry_points_read_the_same_variable(pkg):
    from e3diff_amd.sequence_model import sample as Q
    from e3diff_amd.structure_model import sample as S
    assert S.KEEP == os.environ.get("E3D_SAMPLE_KEEP", "") == Q.KEEP
    batch = {"ligand_seq": torch.zeros(2, 8, 20), "ligand_attn_mask": torch.tensor([[1.0] * 5 + [0.0] * 3, [1.0] * 2 + [0.0] * 6])}
    assert Q.batch_keep_mask("", batch, 0) is None
    assert Q.batch_keep_mask("1-3", batch, 0).int().tolist() == [[0, 1, 1, 1, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0, 0]]


# ------------------------------------------------------------------------------------------------ streams, exports
def _defines():
    src = open(os.path.join(PKG_DIR, "csrc", "e3d_philox.h")).read()
    return {k: int(v, 0) for k, v in re.findall(r"^#define\s+(E3D_[A-Z0-9_]+)\s+(-?\w+)\s*(?://.*)?$", src, re.M)
            if re.fullmatch(r"-?(0x)?[0-9a-fA-F]+", v)}


def test_streams_10_and_11_agree_and_are_distinct(pkg):
    from e3diff_amd import keyed
    d = _defines()
    assert d["E3D_KNOWN_STREAM_STRUCT"] == keyed.KNOWN_STRUCT == 10
    assert d["E3D_KNOWN_STREAM_SEQ"] == keyed.KNOWN_SEQ == 11
    header_streams = {k: v for k, v in d.items() if "STREAM" in k}
    assert len(header_streams) == 12 and sorted(header_streams.values()) == list(range(12))
    py_streams = [keyed.STRUCT_XT, keyed.STRUCT_STEP, keyed.SEQ_XT, keyed.SEQ_U, keyed.TRAIN_STRUCT_T, keyed.TRAIN_STRUCT_NOISE,
                  keyed.TRAIN_SEQ_T, keyed.TRAIN_SEQ_U, keyed.DROP_LIGAND, keyed.DROP_POCKET, keyed.KNOWN_STRUCT, keyed.KNOWN_SEQ]
    assert sorted(py_streams) == list(range(12))
    # the draw streams keep their count: the new ones are named apart, like the dropout streams
    assert len([k for k in d if k.startswith("E3D_STREAM_")]) == 8


def test_new_symbols_are_declared_bound_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "e3d_hip.h")).read()
    declared = set(re.findall(r"\b(e3d_[a-z0-9_]+)\s*\(", header))
    lib = pkg.hip.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg.hip.EXPORTS, name
        assert getattr(lib, name) is not None
    for name in ("known_compose_wrap", "keyed_known_compose_wrap", "discrete_known_compose", "keyed_discrete_known_compose"):
        assert callable(getattr(pkg.ops, name))
    assert pkg.hip.ABI_VERSION == 5 and lib.e3d_abi_version() == 5
    # argument validation happens before any launch: callable without a GPU
    assert lib.e3d_known_compose_wrap(None, None, None, None, None, None, 10, 1.0, 8, None) < 0
    assert b"known_compose_wrap" in lib.e3d_last_error()
    assert lib.e3d_keyed_known_compose_wrap(None, None, None, None, None, 10, 1.0, None, 1, 4, 8, None) < 0
    assert b"keyed_known_compose_wrap" in lib.e3d_last_error()
    assert lib.e3d_discrete_known_compose(None, None, None, None, None, 1, 1, 4, 20, None) < 0
    assert b"discrete_known_compose" in lib.e3d_last_error()
    assert lib.e3d_keyed_discrete_known_compose(None, None, None, None, None, 1, None, 1, 4, 20, None) < 0
    assert b"keyed_discrete_known_compose" in lib.e3d_last_error()


# ------------------------------------------------------------------------------------------------ interface errors
def test_structure_interface_errors(pkg):
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.utils import CosineTables, KnownLevels
    B, L, T = 2, 32, 3
    x, m = torch.zeros(B, L, 8), torch.ones(B, L)
    betas = torch.full((T,), 0.1)
    held = torch.zeros(B, L, dtype=torch.bool)
    held[:, :3] = True

    def loop(**kw):
        return S.p_sample_loop(None, m, x, None, m, None, T, betas, **kw)

    with pytest.raises(ValueError, match="go together"):
        loop(known=x)
    with pytest.raises(ValueError, match="go together"):
        loop(known_mask=held)
    with pytest.raises(ValueError, match="known_noises"):
        loop(known_noises=torch.zeros(T, B, L, 8))
    with pytest.raises(ValueError, match="bool"):
        loop(known=x, known_mask=held.float())
    with pytest.raises(ValueError, match="known must be"):
        loop(known=torch.zeros(B, L, 4), known_mask=held)
    with pytest.raises(ValueError, match="known_mask must be"):
        loop(known=x, known_mask=held[:, :8])
    with pytest.raises(ValueError, match="known_mask must be"):
        loop(known=x, known_mask=torch.zeros(B, L, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="known_noises must be"):
        loop(known=x, known_mask=held, known_noises=torch.zeros(T + 1, B, L, 8), noises=torch.zeros(T, B, L, 8))
    with pytest.raises(ValueError, match="seed"):
        loop(known=x, known_mask=held, known_noises=torch.zeros(T, B, L, 8), seed=1)
    with pytest.raises(ValueError, match="together"):
        loop(known=x, known_mask=held, known_noises=torch.zeros(T, B, L, 8))
    with pytest.raises(ValueError, match="together"):
        loop(known=x, known_mask=held, noises=torch.zeros(T, B, L, 8))
    # p_sample: the same checks, and the level table it needs
    with pytest.raises(ValueError, match="go together"):
        S.p_sample(None, m, x, None, m, None, 1, betas, known=x)
    with pytest.raises(ValueError, match="seed"):
        S.p_sample(None, m, x, None, m, None, 1, betas, known=x, known_mask=held, known_noise=torch.zeros(B, L, 8), seed=1)
    with pytest.raises(ValueError, match="known_levels"):
        S.p_sample(None, m, x, None, m, None, 1, betas, known=x, known_mask=held)
    assert KnownLevels(CosineTables(T), [2, 1, 0]).levels.shape == (T, 2)


def test_sequence_interface_errors(pkg):
    from e3diff_amd.sequence_model import sample as Q
    B, L, T = 2, 32, 3

    class _Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

    batch = {"ligand_seq": torch.zeros(B, L, 20)}
    held = torch.zeros(B, L, dtype=torch.bool)
    held[:, :3] = True

    def run(**kw):
        return Q.denoise(batch, _Model(), None, None, True, timesteps=T, **kw)

    with pytest.raises(ValueError, match="known_mask"):
        run(known_us=[None] * T)
    with pytest.raises(ValueError, match="bool"):
        run(known_mask=held.float())
    with pytest.raises(ValueError, match="known_mask must be"):
        run(known_mask=held[:, :8])
    with pytest.raises(ValueError, match="seed"):
        run(known_mask=held, known_us=[None] * T, seed=1)
    with pytest.raises(ValueError, match="together"):
        run(known_mask=held, known_us=[None] * T)
    with pytest.raises(ValueError, match="together"):
        run(known_mask=held, us=[None] * T)
    with pytest.raises(ValueError, match="entries"):
        run(known_mask=held, us=[None] * T, known_us=[None] * (T - 1))
