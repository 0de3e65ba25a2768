"""GPU: keyed (seeded) sampling.  The kernels' draws against the numpy restatement (tests/keyed_ref.py); the keyed DDPM
update against the table form fed with those draws; and the property the keys exist for -- a pocket's seeded chain does
not depend on its batch, its place in the batch, the frame (padded / trimmed / packed) or the launch mode, in both
samplers and through the structure entry point."""
import warnings

import numpy as np
import pytest
import torch

import keyed_ref as K
from helpers import synthetic_pockets

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WRAPPED_TOL = 6e-4      # fp32 rounding of other kernel shapes through 6 steps of the amplifying chain (test_packed_gpu)


def key_table():
    """Ids above 2^32, positions up to 255, a sentinel row."""
    ids = [0, 1, (1 << 32) + 5, (1 << 63) + 7, 12345678901]
    rows = [(i, p) for i in ids for p in (0, 1, 2, 31, 128, 255)]
    rows.append((9, -1))
    t = torch.tensor([(i - (1 << 64) if i >= 1 << 63 else i, p) for i, p in rows], dtype=torch.int64)
    return t


@pytest.mark.parametrize("seed", [0, 0xDEADBEEFCAFEF00D])
@pytest.mark.parametrize("t", [0, 1, 999])
def test_keyed_draws_match_the_cpu_restatement(pkg, hip, seed, t):
    ops = pkg.ops
    keys = key_table()
    kd = keys.to(DEV)
    z = ops.keyed_draws(kd, seed, 1, t, ops.KEYED_NORMAL, 8).cpu().double().numpy()
    want = K.normals(keys.numpy(), seed, 1, t, 8)
    assert np.all(np.abs(z - want) <= 2e-6 * np.maximum(1.0, np.abs(want))), np.abs(z - want).max()
    assert (z[-1] == 0).all()
    u = ops.keyed_draws(kd, seed, 3, t, ops.KEYED_UNIFORM).cpu().numpy()
    assert np.array_equal(u, K.uniforms(keys.numpy(), seed, 3, t))
    c = ops.keyed_draws(kd, seed, 2, t, ops.KEYED_CLASS, 20).cpu().numpy()
    assert np.array_equal(c, K.classes(keys.numpy(), seed, 2, t, 20))
    onehot = ops.keyed_draws(kd, seed, 2, t, ops.KEYED_ONEHOT, 20).cpu()
    assert torch.equal(onehot[:-1].argmax(dim=1), torch.from_numpy(c[:-1]).long())
    assert (onehot.sum(dim=1)[:-1] == 1).all() and (onehot[-1] == 0).all()
    # keyed x_T: wrap(scale * z) of stream 0
    from e3diff_amd.structure_model.utils import modulo_with_wrapped_range
    z0 = ops.keyed_draws(kd, seed, 0, 0, ops.KEYED_NORMAL, 8)
    xt = ops.keyed_initial_angles(kd, seed, 8, scale=1.5)
    d = modulo_with_wrapped_range(xt[:-1] - modulo_with_wrapped_range(z0 * 1.5)[:-1]).abs().max().item()
    assert d < 2e-6 and (xt[-1] == 0).all() and xt.abs().max() <= 3.1416


def test_keyed_update_equals_the_table_form_with_the_same_normals(pkg, hip):
    from e3diff_amd.structure_model.utils import CosineTables
    ops = pkg.ops
    tab = CosineTables(1000)
    coef = torch.stack([tab.sqrt_recip_alphas, tab.betas, tab.sqrt_one_minus_alphas_cumprod, tab.sigma],
                       dim=1).float().contiguous().to(DEV)
    keys = key_table().to(DEV)
    rows = keys.shape[0]
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(rows, 8, generator=g) * 6 - 3).to(DEV)
    eps = torch.randn(rows, 8, generator=g).to(DEV)
    seed = 77
    for t in (999, 500, 1, 0):
        t_dev = torch.full((1,), t, dtype=torch.int64, device=DEV)
        for wrap in (True, False):
            got = ops.keyed_ddpm_step_wrap(x, eps, coef, t_dev, keys, seed, wrap=wrap)
            z = ops.keyed_draws(keys, seed, 1, t, ops.KEYED_NORMAL, 8)
            want = ops.ddpm_step_wrap_table(x, eps, z, coef, t_dev, wrap=wrap)
            assert torch.equal(got, want), (t, wrap)
            mean = ops.ddpm_step_wrap_table(x, eps, torch.zeros_like(z), coef, t_dev, wrap=wrap)
            assert torch.equal(got[-1], mean[-1])                      # sentinel row: no noise
            if t == 0:
                assert torch.equal(got, mean)                          # sigma == 0: the mean
            else:
                assert not torch.equal(got[:-1], mean[:-1])
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.keyed_ddpm_step_wrap(x[:, :6].contiguous(), eps[:, :6].contiguous(), coef, t_dev, keys, seed)


# ------------------------------------------------------------------------------------------------ structure chain
def _structure_setup(B=4, L=128, T=6, seed=0):
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.structure_model.model import ConditionalBertForDiffusion as M
    from e3diff_amd.structure_model.utils import CosineTables
    c = dict(hidden_size=768, num_attention_heads=12, intermediate_size=1024, num_hidden_layers=2,
             max_position_embeddings=L, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    torch.manual_seed(seed)
    model = M(BertConfig(**c), BertConfig(**c, is_decoder=True, add_cross_attention=True),
              feature_names=list("abcdefgh"), loss_func=[M.diheral_loss_func] * 8).eval().to(DEV)
    pk = {k: v.to(DEV) for k, v in synthetic_pockets(B, L, seed=3, rec_range=(20, 70)).items() if torch.is_tensor(v)}
    return model, pk, CosineTables(T)


def _chain(S, model, pk, tab, ids, seed, sel=None, **kw):
    """Seeded chain over the items ``sel`` of the batch (default all), keyed x_T; [T, b, L, 8] on the device."""
    sel = list(range(pk["ligand_attn_mask"].shape[0])) if sel is None else sel
    p = {k: v[sel].contiguous() for k, v in pk.items()}
    L = p["ligand_attn_mask"].shape[1]
    x_T = S.keyed_x_T(seed, [ids[i] for i in sel], L, 8, device=DEV)
    return S.p_sample_loop(model, p["ligand_attn_mask"], x_T, p["receptor_seq"], p["receptor_attn_mask"],
                           p["receptor_angles"], tab.timesteps, tab, return_device=True, step=1, seed=seed,
                           item_ids=[ids[i] for i in sel], **kw)


def _wrapped_diff(a, b, valid):
    from e3diff_amd.structure_model.utils import modulo_with_wrapped_range
    return modulo_with_wrapped_range((a - b)[valid]).abs().max().item()


def test_structure_chain_draws_follow_the_item(pkg, hip):
    from e3diff_amd.structure_model import sample as S
    model, pk, tab = _structure_setup()
    B = 4
    ids = [11, (1 << 35) + 2, 7, 123456]
    seed = 2024
    base = _chain(S, model, pk, tab, ids, seed)
    assert base.shape == (tab.timesteps, B, 128, 8) and torch.isfinite(base).all()
    # reversed batch, reversed ids: the same chain per item, bit for bit
    rev = _chain(S, model, pk, tab, ids, seed, sel=list(reversed(range(B))))
    for b in range(B):
        assert torch.equal(rev[:, B - 1 - b], base[:, b]), f"item {b}: reversed order changed its chain"
    # the same seed twice: bit-identical; another seed moves the angles
    assert torch.equal(_chain(S, model, pk, tab, ids, seed), base)
    other = _chain(S, model, pk, tab, ids, seed + 1)
    valid = pk["ligand_attn_mask"].bool()[None, :, :, None].expand_as(base)
    assert _wrapped_diff(other, base, valid) > 0.1
    # one pocket alone vs in the batch (other GEMM shapes: fp32 rounding only)
    one = _chain(S, model, pk, tab, ids, seed, sel=[2])
    assert _wrapped_diff(one[:, 0], base[:, 2], valid[:, 2]) < WRAPPED_TOL
    # padded vs trimmed vs packed frames, on the valid positions
    trim = _chain(S, model, pk, tab, ids, seed, trim_padding=True)
    packed = _chain(S, model, pk, tab, ids, seed, pack=True)
    assert _wrapped_diff(trim, base, valid) < WRAPPED_TOL
    assert _wrapped_diff(packed, base, valid) < WRAPPED_TOL
    assert _wrapped_diff(packed, trim, valid) < WRAPPED_TOL


@pytest.mark.parametrize("frame", [{}, {"pack": True}])
def test_structure_seeded_graph_replay_is_bit_identical_to_eager(pkg, hip, frame):
    from e3diff_amd.structure_model import sample as S
    model, pk, tab = _structure_setup(B=3, L=64, T=8, seed=1)
    ids = [5, 6, 7]
    eager = _chain(S, model, pk, tab, ids, 99, use_graph=False, **frame)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        graph = _chain(S, model, pk, tab, ids, 99, use_graph=True, **frame)
    assert not [str(w.message) for w in caught if "HIP-graph capture" in str(w.message)]
    assert torch.equal(eager, graph)


def test_structure_p_sample_seeded_step(pkg, hip):
    """One seeded p_sample step draws the keyed stream-1 normals of (seed, id, t, position)."""
    from e3diff_amd.structure_model import sample as S
    model, pk, tab = _structure_setup(B=2, L=64, T=6, seed=2)
    x = S.keyed_x_T(3, [4, 9], 64, 8, device=DEV)
    args = (model, pk["ligand_attn_mask"], x, pk["receptor_seq"], pk["receptor_attn_mask"], pk["receptor_angles"], 4, tab)
    got = S.p_sample(*args, seed=3, item_ids=[4, 9])
    keys = pkg.keyed.padded_keys([4, 9], 64, DEV)
    z = pkg.ops.keyed_draws(keys, 3, 1, 4, pkg.ops.KEYED_NORMAL, 8).reshape(2, 64, 8)
    want = S.p_sample(*args, noise=z)
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ sequence chain
def _seq_setup(T=6, B=4, L=128):
    from helpers import seeded_state_dict
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.sequence_model.model import PeptideDiff
    from e3diff_amd.sequence_model.utils import DiscreteUniformTransition, PredefinedNoiseScheduleDiscrete
    common = dict(hidden_size=256, num_attention_heads=4, intermediate_size=1024, num_hidden_layers=2,
                  max_position_embeddings=L)
    model = PeptideDiff(BertConfig(**common), BertConfig(**common, is_decoder=True, add_cross_attention=True),
                        feature_names=list("ACDEFGHIKLMNPQRSTVWY"), loss_func=torch.nn.CrossEntropyLoss(),
                        noise_schedule="cosine", timesteps=T)
    model.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=2))
    pk = dict(synthetic_pockets(B, L, seed=8, with_ligand_seq=True, rec_range=(20, 60)), structure_ids=None)
    return model.eval().to(DEV), pk, PredefinedNoiseScheduleDiscrete("cosine", T).to(DEV), DiscreteUniformTransition(20)


def test_sequence_chain_draws_follow_the_item(pkg, hip):
    from e3diff_amd.sequence_model.sample import denoise
    T, B = 6, 4
    model, pk, sched, tr = _seq_setup(T, B)
    ids = [3, (1 << 40) + 1, 8, 2]
    base = denoise(pk, model, sched, tr, True, timesteps=T, seed=5, item_ids=ids)
    rev_pk = {k: (v.flip(0) if torch.is_tensor(v) else v) for k, v in pk.items()}
    rev = denoise(rev_pk, model, sched, tr, True, timesteps=T, seed=5, item_ids=ids[::-1])
    assert rev[2][::-1] == base[2] and rev[1][::-1] == base[1] and rev[3][::-1] == base[3]
    packed = denoise(pk, model, sched, tr, True, timesteps=T, seed=5, item_ids=ids, pack=True)
    assert packed[2] == base[2] and packed[3] == base[3]
    trim = denoise(pk, model, sched, tr, True, timesteps=T, seed=5, item_ids=ids, trim_padding=True)
    assert trim[2] == base[2]
    again = denoise(pk, model, sched, tr, True, timesteps=T, seed=5, item_ids=ids)
    assert again[2] == base[2]
    other = denoise(pk, model, sched, tr, True, timesteps=T, seed=6, item_ids=ids)
    assert other[2] != base[2]


@pytest.mark.parametrize("frame", [{}, {"pack": True}])
def test_sequence_seeded_graph_replay_is_bit_identical_to_eager(pkg, hip, frame):
    from e3diff_amd.sequence_model.sample import denoise
    T = 8
    model, pk, sched, tr = _seq_setup(T)
    eager = denoise(pk, model, sched, tr, True, timesteps=T, seed=11, use_graph=False, **frame)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        graph = denoise(pk, model, sched, tr, True, timesteps=T, seed=11, use_graph=True, **frame)
    assert not [str(w.message) for w in caught if "HIP-graph capture" in str(w.message)]
    assert graph[2] == eager[2] and graph[3] == eager[3]


def test_keyed_sequence_x_T_is_the_stream_2_one_hot(pkg, hip):
    from e3diff_amd.sequence_model.sample import keyed_discrete_noise
    x = keyed_discrete_noise(4, [1, 2], 64, 20, DEV)
    keys = pkg.keyed.padded_keys([1, 2], 64, "cpu")
    want = torch.from_numpy(K.classes(keys.numpy(), 4, 2, 0, 20)).reshape(2, 64)
    assert x.shape == (2, 64, 20) and torch.equal(x.argmax(dim=-1).cpu(), want) and (x.sum(-1) == 1).all()


# ------------------------------------------------------------------------------------------------ entry point
def test_structure_entry_point_batch_size_does_not_change_a_pocket(pkg, hip, tmp_path, monkeypatch):
    from e3diff_amd import biolip
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.dataset import LigandBindingSiteDataset, NoisedAnglesDataset
    from e3diff_amd.structure_model.model import ConditionalBertForDiffusion as M
    path = biolip.write_synthetic(str(tmp_path / "biolip.pt"), 7, seed=4)
    L = 64
    ds = NoisedAnglesDataset(LigandBindingSiteDataset(path, None, L, 0), timesteps=5)
    c = dict(hidden_size=768, num_attention_heads=12, intermediate_size=1024, num_hidden_layers=2,
             max_position_embeddings=L, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    torch.manual_seed(3)
    model = M(BertConfig(**c), BertConfig(**c, is_decoder=True, add_cross_attention=True),
              feature_names=ds.feature_names, loss_func=[M.diheral_loss_func] * 8).eval().to(DEV)
    runs = {}
    for bs in (4, 3):
        monkeypatch.setitem(S.CONFIG, "batch_size", bs)
        runs[bs] = S.sample(model, ds, all_batches=True, seed=31)
    assert len(runs[4]) == len(runs[3]) == 7
    for a, b in zip(runs[4], runs[3]):
        assert a.shape == b.shape and a.shape[0] == 5 and np.isfinite(a).all()
        d = np.abs(np.mod(a - b + np.pi, 2 * np.pi) - np.pi).max()
        assert d < WRAPPED_TOL, d
    monkeypatch.setitem(S.CONFIG, "batch_size", 4)
    assert all(np.array_equal(a, b) for a, b in zip(S.sample(model, ds, all_batches=True, seed=31), runs[4]))
