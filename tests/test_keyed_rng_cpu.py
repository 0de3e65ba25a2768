"""CPU: keyed sampling streams -- the numpy restatement (tests/keyed_ref.py) against Philox4x32-10's known answers and
the distribution of its maps; the row-key tables of the padded, trimmed and packed frames (keyed.py); and the argument
checks of the seeded samplers, which refuse a seed together with injected draws before any launch."""
import numpy as np
import pytest
import torch

import keyed_ref as K


# ------------------------------------------------------------------------------- Philox4x32-10 known answers
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = K.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
    assert [int(v) for v in got] == list(want)


def test_counter_layout():
    """c0, c1 = item id; c2 = stream << 16 | t; c3 = position << 8 | block; key = (seed lo, seed hi)."""
    seed, item = 0x0123456789ABCDEF, 0xFEDCBA9876543210
    got = K.words(seed, item, 3, 999, 255, 7)
    want = K.philox4x32_10(np.array([0x76543210, 0xFEDCBA98, (3 << 16) | 999, (255 << 8) | 7], dtype=np.uint32),
                           np.array([0x89ABCDEF, 0x01234567], dtype=np.uint32))
    assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        K.words(1, 0, 1, 65536, 0, 0)
    with pytest.raises(ValueError):
        K.words(1, 0, 1, 0, 1 << 24, 0)


# ------------------------------------------------------------------------------- maps
def test_normals_uniforms_classes_distribution():
    n = 1 << 20
    rows = n // 8
    keys = np.stack([np.arange(rows) // 64 + (1 << 33), np.arange(rows) % 64], axis=1)
    z = K.normals(keys, 12345, 1, 7, 8).ravel()
    assert z.size == n
    assert abs(z.mean()) < 0.01 and abs(z.var() - 1.0) < 0.01
    assert np.abs(z).max() <= np.sqrt(2 * 24 * np.log(2)) + 1e-12      # u1 >= 2^-24
    u = K.uniforms(keys, 12345, 3, 7)
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    assert abs(float(u.mean()) - 0.5) < 0.01
    c = K.classes(keys, 12345, 2, 0, 20)
    counts = np.bincount(c, minlength=20)
    assert counts.size == 20 and (counts > 0).all()
    assert counts.max() / counts.min() < 1.1                              # near-uniform over 131072 draws


def test_streams_steps_and_seeds_are_distinct():
    keys = np.stack([np.full(64, 5), np.arange(64)], axis=1)
    a = K.normals(keys, 1, 1, 3, 8)
    assert not np.array_equal(a, K.normals(keys, 1, 1, 4, 8))       # another step
    assert not np.array_equal(a, K.normals(keys, 1, 0, 3, 8))       # another stream
    assert not np.array_equal(a, K.normals(keys, 2, 1, 3, 8))       # another seed
    assert np.array_equal(a, K.normals(keys, 1, 1, 3, 8))           # a pure function
    sentinel = np.array([[7, -1], [7, 0]])
    assert (K.normals(sentinel, 1, 1, 3, 8)[0] == 0).all()


# ------------------------------------------------------------------------------- row-key tables
def _mask(lengths, L):
    return (torch.arange(L)[None] < torch.tensor(lengths)[:, None]).float()


def test_row_keys_agree_across_frames(pkg):
    from e3diff_amd import keyed, packing
    from e3diff_amd.structure_model.sample import trimmed_length
    lengths, L = [5, 0, 31, 33, 12], 128
    ids = [3, 1 << 40, 17, (1 << 64) - 1, 0]
    mask = _mask(lengths, L)
    padded = keyed.padded_keys(ids, L, "cpu")
    Lt = trimmed_length(mask)
    assert Lt == 64
    trimmed = keyed.padded_keys(ids, Lt, "cpu")
    lay = packing.PackedLayout.from_mask(mask)
    packed = keyed.packed_keys(lay, ids, "cpu")
    assert padded.shape == (len(ids) * L, 2) and trimmed.shape == (len(ids) * Lt, 2) and packed.shape == (lay.rows, 2)

    def valid(table, frame):
        return [tuple(table[b * frame + l].tolist()) for b, n in enumerate(lengths) for l in range(n)]

    want = [(i - (1 << 64) if i >= 1 << 63 else i, l) for i, n in zip(ids, lengths) for l in range(n)]
    assert valid(padded, L) == want and valid(trimmed, Lt) == want
    assert [tuple(r) for r in packed[:lay.total].tolist()] == want
    assert lay.rows > lay.total and (packed[lay.total:] == keyed.SENTINEL).all()
    # every padded row is keyed (padding positions draw too, as in the unseeded chain)
    assert (padded[:, 1] >= 0).all()


def test_item_ids_and_seed_checks(pkg):
    from e3diff_amd import keyed
    assert keyed.item_ids(None, 3) == [0, 1, 2]
    assert keyed.item_ids(torch.tensor([4, 5]), 2) == [4, 5]
    with pytest.raises(ValueError):
        keyed.item_ids([1, 2], 3)
    with pytest.raises(ValueError):
        keyed.item_ids([-1], 1)
    assert keyed.check_seed(2 ** 64 - 1) == 2 ** 64 - 1
    with pytest.raises(ValueError):
        keyed.check_seed(2 ** 64)
    with pytest.raises(ValueError):
        keyed.check_steps(65537)
    keyed.check_steps(65536)
    with pytest.raises(ValueError):
        keyed.padded_keys([0], (1 << 24) + 1, "cpu")


# ------------------------------------------------------------------------------- samplers refuse seed + injected draws
def test_seed_with_injected_draws_raises(pkg):
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.sequence_model import sample as Q
    B, L, T = 2, 32, 3
    x = torch.zeros(B, L, 8)
    m = torch.ones(B, L)
    with pytest.raises(ValueError, match="seed"):
        S.p_sample_loop(None, m, x, None, m, None, T, torch.full((T,), 0.1), noises=torch.zeros(T, B, L, 8), seed=1)
    with pytest.raises(ValueError, match="seed"):
        S.p_sample(None, m, x, None, m, None, 1, torch.full((T,), 0.1), noise=torch.zeros(B, L, 8), seed=1)
    with pytest.raises(ValueError, match="seed"):
        S.p_sample_loop(None, m, x, None, m, None, T, torch.full((T,), 0.1), item_ids=[0, 1])

    class _Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

    batch = {"ligand_seq": torch.zeros(B, L, 20)}
    with pytest.raises(ValueError, match="seed"):
        Q.denoise(batch, _Model(), None, None, True, x_T=torch.zeros(B, L, 20), seed=1, timesteps=T)
    with pytest.raises(ValueError, match="seed"):
        Q.denoise(batch, _Model(), None, None, True, us=[None] * T, seed=1, timesteps=T)


def test_keyed_kernels_are_declared(pkg):
    for name in ("e3d_keyed_ddpm_step_wrap", "e3d_keyed_discrete_posterior_sample", "e3d_keyed_draws"):
        assert name in pkg.hip.EXPORTS
    lib = pkg.hip.lib()
    # argument validation before any launch: callable without a GPU
    assert lib.e3d_keyed_ddpm_step_wrap(None, None, None, None, None, 1, 1, None, 4, 8, None) < 0
    assert b"keyed_ddpm_step_wrap" in lib.e3d_last_error()
    assert lib.e3d_keyed_draws(None, 1, 0, 0, 0, 8, 0, 1.0, None, 4, None) < 0
