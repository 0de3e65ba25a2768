"""Numpy restatement of the seeded (unkeyed) dropout decisions, written from the prose of include/e3d_hip.h ("dropout
(training)", e3d_dropout_set_epoch_ptr) and csrc/e3d_common.h -- the law of every dropout launch that is not given row keys.

One SplitMix64 output per group of 4 consecutive elements:

    seed_term = (seed + epoch * 0xD1342543DE82EF95) * G + G            (mod 2^64; G = 0x9E3779B97F4A7C15; ``epoch`` is the
                                                                        device word of e3d_dropout_set_epoch_ptr, 0 if none)
    z         = group index + seed_term, then the SplitMix64 finaliser
    element j of the group takes bits 16 j .. 16 j + 15; kept iff that field >= thr = round(65536 p); multiplier
    65536 / (65536 - thr) or 0

Group indices: a flat tensor of n elements: i = element >> 2.  An [M, H] hidden state (H % 4 == 0): r * (H / 4) + column >> 2,
which IS the flat index.  Attention probabilities P[b, h, q, key]: ((b * nh + h) * Lq + q) * ((Lk + 3) >> 2) + key >> 2 --
every query row starts a group of its own, so the last group of a row is cut when Lk % 4 != 0.

At epoch 0, group 0 of the seeds 0, 1, 2, ... hashes G, 2 G, 3 G, ...: the output sequence of SplitMix64 from state 0
(tests/test_dropout_ref_cpu.py asserts the published values).  The tests hold the HIP kernels to this file bit for bit;
the product does not import it."""
import numpy as np

from keyed_dropout_ref import GOLD, MIX1, MIX2, scale, threshold  # noqa: F401  (threshold / scale: the keyed law's, re-used)

EPOCH_MULT = 0xD1342543DE82EF95
MASK64 = (1 << 64) - 1


def seed_term(seed, epoch=0):
    """(seed + epoch * EPOCH_MULT) * G + G mod 2^64, as a numpy uint64 (Python integers: no overflow to think about)."""
    s = (int(seed) + int(epoch) * EPOCH_MULT) & MASK64
    return np.uint64((s * int(GOLD) + int(GOLD)) & MASK64)


def finalise(z):
    """The SplitMix64 finaliser on uint64 (any shape)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * MIX1
        z = (z ^ (z >> np.uint64(27))) * MIX2
        return z ^ (z >> np.uint64(31))


def group(z):
    """uint32 [..., 4]: the fields of the groups whose hash inputs are ``z``; element j takes bits 16 j .. 16 j + 15."""
    h = finalise(z)
    return np.stack([(h >> np.uint64(16 * j)) & np.uint64(0xFFFF) for j in range(4)], axis=-1).astype(np.uint32)


def _fields(index, seed, epoch):
    with np.errstate(over="ignore"):
        return group(np.asarray(index, dtype=np.uint64) + seed_term(seed, epoch))


def _mult(keep, p):
    return np.where(keep, scale(p), np.float32(0)).astype(np.float32)


def elementwise_keep(n, p, seed, epoch=0):
    """bool [n]: element e of a flat tensor is field e & 3 of group e >> 2."""
    f = _fields(np.arange((n + 3) // 4, dtype=np.uint64), seed, epoch)
    return (f >= threshold(p)).reshape(-1)[:n]


def elementwise_mult(n, p, seed, epoch=0):
    return _mult(elementwise_keep(n, p, seed, epoch), p)


def hidden_keep(M, H, p, seed, epoch=0):
    """bool [M, H] (H % 4 == 0): row r, group g has index r * (H / 4) + g."""
    assert H % 4 == 0
    idx = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(H // 4) + np.arange(H // 4, dtype=np.uint64)[None]
    return (_fields(idx, seed, epoch) >= threshold(p)).reshape(M, H)


def hidden_mult(M, H, p, seed, epoch=0):
    return _mult(hidden_keep(M, H, p, seed, epoch), p)


def attn_fields(B, nh, Lq, Lk, seed, epoch=0):
    """uint32 [B, nh, Lq, groups, 4] with groups = (Lk + 3) >> 2: the fields behind ``attn_keep``."""
    groups = (Lk + 3) >> 2
    b = np.arange(B, dtype=np.uint64).reshape(B, 1, 1, 1)
    h = np.arange(nh, dtype=np.uint64).reshape(1, nh, 1, 1)
    q = np.arange(Lq, dtype=np.uint64).reshape(1, 1, Lq, 1)
    row = ((b * np.uint64(nh) + h) * np.uint64(Lq) + q) * np.uint64(groups)
    return _fields(row + np.arange(groups, dtype=np.uint64).reshape(1, 1, 1, groups), seed, epoch)


def attn_keep(B, nh, Lq, Lk, p, seed, epoch=0):
    """bool [B, nh, Lq, Lk]: decisions on the attention probabilities; group = key >> 2 within the query row."""
    f = attn_fields(B, nh, Lq, Lk, seed, epoch)
    return (f >= threshold(p)).reshape(B, nh, Lq, -1)[..., :Lk]


def attn_mult(B, nh, Lq, Lk, p, seed, epoch=0):
    return _mult(attn_keep(B, nh, Lq, Lk, p, seed, epoch), p)
