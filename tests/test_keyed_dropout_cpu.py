"""CPU: the decision function of keyed dropout ("Keyed sampling streams": streams 8 / 9) as the numpy
restatement states it (tests/keyed_dropout_ref.py; the GPU tests hold the kernels to it bit for bit) -- the keep rate,
the four fields of a group, independence along every coordinate of the key -- and the host-side refusals."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import keyed_dropout_ref as R

IDS = [0, 1, 5, 123456789, (1 << 32) + 9, (1 << 63) + 17, (1 << 64) - 1, 77]
SEED, L, H = 7, 128, 1024                                    # 8 x 128 rows x 1024 columns: 2^20 > 10^6 decisions


def _keep(seed=SEED, ids=IDS, stream=R.LIGAND, epoch=3, site=5, p=0.1):
    return R.hidden_keep(R.row_keys(seed, ids, L, stream, epoch), H, p, site)


def _corr(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    return float(((a - a.mean()) * (b - b.mean())).mean() / (a.std() * b.std()))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate_and_fields(p):
    keep = _keep(p=p)
    n = keep.size
    assert n >= 10 ** 6
    thr = round(p * 65536)
    assert R.threshold(p) == thr and R.scale(p) == np.float32(65536.0 / (65536 - thr))
    sigma = math.sqrt(p * (1 - p) / n)
    rate = 1.0 - keep.mean()
    assert abs(rate - thr / 65536) < 5 * sigma + 1e-6, (rate, thr / 65536)          # the bound of test_dropout_gpu.py
    m = keep.reshape(-1, 4).mean(0)                                                 # per-field keep rates agree
    assert np.abs(m - (1 - thr / 65536)).max() < 6 * math.sqrt(p * (1 - p) / (n // 4)), m
    flat = keep.ravel()
    assert abs(_corr(flat[:-1], flat[1:])) < 5 / math.sqrt(n)                       # neighbouring decisions: uncorrelated
    mult = R.hidden_mult(R.row_keys(SEED, IDS, L, R.LIGAND, 3), H, p, 5)
    assert sorted(np.unique(mult).tolist()) == [0.0, float(R.scale(p))] and np.array_equal(mult != 0, keep)


def test_decisions_are_independent_along_every_coordinate_of_the_key():
    base = _keep()
    grid = base.reshape(len(IDS), L, H)
    pairs = {
        "neighbouring columns": (grid[:, :, :-1], grid[:, :, 1:]),
        "neighbouring groups": (grid[:, :, :-4], grid[:, :, 4:]),
        "neighbouring positions": (grid[:, :-1], grid[:, 1:]),
        "two ids": (grid[:-1], grid[1:]),
        "sites s, s + 1": (base, _keep(site=6)),
        "streams 8, 9": (base, _keep(stream=R.POCKET)),
        "epochs e, e + 1": (base, _keep(epoch=4)),
        "two seeds": (base, _keep(seed=SEED + 1)),
    }
    for name, (a, b) in pairs.items():
        c = _corr(a, b)
        assert abs(c) < 5 / math.sqrt(a.size), (name, c)
        assert not np.array_equal(a, b), name
    assert np.array_equal(base, _keep())                                            # a pure function of its key


def test_attention_decisions_follow_the_query_row_not_the_frame():
    p, site, nh = 0.1, 9, 4
    keys = R.row_keys(SEED, IDS, 64, R.LIGAND, 0)
    full = R.attn_keep(keys, len(IDS), nh, 64, 128, p, site)
    n = full.size
    assert abs((1 - full.mean()) - R.threshold(p) / 65536) < 5 * math.sqrt(p * (1 - p) / n) + 1e-6
    # the trimmed frame: fewer query rows, fewer keys, the same decisions where both exist
    small = R.attn_keep(R.row_keys(SEED, IDS, 32, R.LIGAND, 0), len(IDS), nh, 32, 50, p, site)
    assert np.array_equal(small, full[:, :, :32, :50])
    # one item alone, and two heads of one row
    one = R.attn_keep(R.row_keys(SEED, IDS[3:4], 64, R.LIGAND, 0), 1, nh, 64, 128, p, site)
    assert np.array_equal(one[0], full[3])
    assert abs(_corr(full[:, 0], full[:, 1])) < 5 / math.sqrt(full[:, 0].size)
    assert abs(_corr(full[:, :, :-1], full[:, :, 1:])) < 5 / math.sqrt(full[:, :, 1:].size)       # neighbouring queries
    assert abs(_corr(full[..., :-1], full[..., 1:])) < 5 / math.sqrt(full[..., 1:].size)          # neighbouring keys
    # a hidden-state site and an attention site with the same ordinal share nothing either (head 0, group g coincide
    # only when the ordinals do: the model numbers every call of a step differently)
    assert not np.array_equal(R.attn_keep(keys, len(IDS), nh, 64, 128, p, site + 1), full)


def test_restatement_refuses_what_the_index_cannot_hold():
    keys = R.row_keys(SEED, IDS, 4, R.LIGAND, R.MAX_EPOCH)
    with pytest.raises(ValueError, match="site"):
        R.hidden_keep(keys, 8, 0.1, 1 << 24)
    with pytest.raises(ValueError, match="heads"):
        R.attn_keep(keys, len(IDS), 1 << 16, 4, 4, 0.1, 0)
    with pytest.raises(ValueError, match="epoch"):
        R.row_keys(SEED, IDS, 4, R.LIGAND, R.MAX_EPOCH + 1)
    with pytest.raises(ValueError, match="streams"):
        R.row_keys(SEED, IDS, 4, 7, 0)


def test_host_side_refusals(pkg):
    """Site >= 2^24, heads >= 2^16, epoch > keyed.MAX_EPOCH, another stream: refused on the host, before any launch (the
    library validates its arguments first: callable without a GPU)."""
    from e3diff_amd import keyed, ops
    assert (keyed.DROP_LIGAND, keyed.DROP_POCKET) == (R.LIGAND, R.POCKET) and keyed.MAX_EPOCH == R.MAX_EPOCH
    assert (ops.MAX_DROPOUT_SITES, ops.MAX_DROPOUT_HEADS) == (R.MAX_SITES, R.MAX_HEADS)
    header = open(os.path.join(os.path.dirname(pkg.hip.LIB_PATH), "csrc", "e3d_philox.h")).read()
    defines = dict(re.findall(r"^#define\s+(E3D_DROP_STREAM_[A-Z]+)\s+(\d+)", header, re.M))
    assert defines == {"E3D_DROP_STREAM_LIGAND": str(keyed.DROP_LIGAND), "E3D_DROP_STREAM_POCKET": str(keyed.DROP_POCKET)}
    with pytest.raises(ValueError, match="epochs"):
        keyed.check_epoch(keyed.MAX_EPOCH + 1)
    ids, word = torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="streams"):
        ops.keyed_drop_row_keys(ids, 4, word, 1, keyed.TRAIN_SEQ_U)
    with pytest.raises(ValueError, match="2\\^24"):
        ops.keyed_drop_row_keys(ids, (1 << 24) + 1, word, 1, keyed.DROP_LIGAND)
    # the site counter: ordinals from 0, no torch generator call, refusal at 2^24
    state = torch.get_rng_state()
    with ops.keyed_dropout(3, word, ids) as kd:
        assert ops.keyed_dropout_state() is kd
        assert [ops.next_dropout_seed() for _ in range(3)] == [0, 1, 2]
        keys = torch.zeros(8, dtype=torch.int64)
        assert ops.site_drop(0.1, keys)[:2] == (0.1, 3)
        with pytest.raises(RuntimeError, match="key table"):
            ops.site_drop(0.1)
        kd.site = ops.MAX_DROPOUT_SITES
        with pytest.raises(ValueError, match="sites"):
            ops.next_dropout_seed()
    assert ops.keyed_dropout_state() is None and torch.equal(torch.get_rng_state(), state)
    with pytest.raises(RuntimeError, match="outside"):
        ops.site_drop(0.1, torch.zeros(8, dtype=torch.int64))
    with pytest.raises(ValueError, match="site"):
        ops._keyed_drop((0.1, 1 << 24, torch.zeros(8, dtype=torch.int64)), 8, "test")
    with pytest.raises(ValueError, match="heads"):
        ops._keyed_drop((0.1, 0, torch.zeros(8, dtype=torch.int64)), 8, "test", heads=1 << 16)
    # the C ABI itself
    lib = pkg.hip.lib()
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    assert lib.e3d_dropout_f32_keyed(ptr, 0.1, 1 << 24, ptr, ptr, 4, 4, None) < 0
    assert b"24 bits" in lib.e3d_last_error()
    assert lib.e3d_keyed_attn_dropout_mask(1, 1 << 16, 4, 4, 0.1, 0, ptr, ptr, None) < 0
    assert b"out of range" in lib.e3d_last_error()
    assert lib.e3d_keyed_attn_dropout_mask(1, 2, 4, 4, 0.1, 1 << 24, ptr, ptr, None) < 0
    assert lib.e3d_residual_layernorm_drop_fwd_keyed(ptr, ptr, ptr, ptr, 1e-12, ptr, ptr, 4, 256, 0.1, 1 << 24, ptr, None) < 0
    assert lib.e3d_keyed_drop_row_keys(ptr, 2, 4, ptr, 1, 7, ptr, None) < 0
    assert b"stream" in lib.e3d_last_error()


def test_a_seeded_step_refuses_a_batch_without_item_ids(pkg):
    """Both models' ``training_step`` with keyed dropout on: the "ItemIdDataset" ValueError of the keyed draws, raised
    before anything is launched."""
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.sequence_model.model import PeptideDiff
    from e3diff_amd.structure_model.model import ConditionalBertForDiffusion as M
    c = dict(hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=1, max_position_embeddings=16,
             hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    enc, dec = BertConfig(**c), BertConfig(**c, is_decoder=True, add_cross_attention=True)
    word = torch.zeros(1, dtype=torch.int64)
    models = [M(enc, dec, feature_names=list("abcdefgh"), loss_func=[M.diheral_loss_func] * 8),
              PeptideDiff(enc, dec, feature_names=list("ACDEFGHIKLMNPQRSTVWY"), loss_func=torch.nn.CrossEntropyLoss(),
                          noise_schedule="cosine", timesteps=50)]
    for model in models:
        assert model.keyed_dropout is None
        assert model.use_keyed_dropout(5, word) is word and model.keyed_dropout == (5, word)
        with pytest.raises(ValueError, match="ItemIdDataset"):
            model.train().training_step({"ligand_attn_mask": torch.ones(2, 16)})
        model.use_keyed_dropout(None)
        assert model.keyed_dropout is None
