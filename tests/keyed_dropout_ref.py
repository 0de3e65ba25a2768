"""Numpy restatement of the keyed dropout decisions ("Keyed sampling streams": streams 8 / 9), built on
``keyed_ref.words``.  A frame row's 64-bit key is w0 | w1 << 32 of the Philox words of (seed, item id, stream, epoch,
position, block 0); it seeds the splitmix64 generator of that row's decisions, whose group index is
site << 40 | head << 24 | group (group = column >> 2 or key position >> 2); element j of a group is kept iff the j-th
16-bit field of the hash is >= thr = round(65536 p), kept values are scaled by 65536 / (65536 - thr).  The tests hold the
HIP kernels to it bit for bit; the product does not import it."""
import numpy as np

import keyed_ref as K

LIGAND, POCKET = 8, 9
MAX_EPOCH = 65534
MAX_SITES, MAX_HEADS = 1 << 24, 1 << 16
GOLD = np.uint64(0x9E3779B97F4A7C15)
MIX1, MIX2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def row_keys(seed, ids, L, stream, epoch):
    """uint64 [B * L]: the keys of the rows of a [B, L] frame (row b * L + l = item ids[b] at position l)."""
    if stream not in (LIGAND, POCKET):
        raise ValueError("dropout row keys live on streams 8 (ligand rows) and 9 (pocket rows)")
    if not 0 <= int(epoch) <= MAX_EPOCH:
        raise ValueError(f"epoch outside [0, {MAX_EPOCH}]")
    ids = np.array([int(i) for i in ids], dtype=np.uint64)
    w = K.words(seed, ids[:, None], stream, epoch, np.arange(L)[None], 0)
    return (w[..., 0].astype(np.uint64) | (w[..., 1].astype(np.uint64) << np.uint64(32))).reshape(-1)


def threshold(p):
    t = int(np.rint(np.float32(p) * np.float32(65536.0)))
    return min(max(t, 0), 65535)


def scale(p):
    return np.float32(65536.0) / np.float32(65536 - threshold(p))


def fields(keys, idx4):
    """The four 16-bit fields of the group ``idx4`` under row key ``keys`` (uint64, broadcast) -> uint32 [..., 4]."""
    keys, idx4 = np.asarray(keys, dtype=np.uint64), np.asarray(idx4, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = idx4 + keys * GOLD + GOLD
        z = (z ^ (z >> np.uint64(30))) * MIX1
        z = (z ^ (z >> np.uint64(27))) * MIX2
        z = z ^ (z >> np.uint64(31))
    return np.stack([(z >> np.uint64(16 * j)) & np.uint64(0xFFFF) for j in range(4)], axis=-1).astype(np.uint32)


def _index(site, heads):
    if not 0 <= int(site) < MAX_SITES:
        raise ValueError("site outside [0, 2^24)")
    if not 0 < int(heads) < MAX_HEADS:
        raise ValueError("heads outside [1, 2^16)")
    return np.uint64(int(site) << 40)


def hidden_keep(keys, H, p, site):
    """bool [rows, H]: the decisions of a hidden-state site on rows with these keys (H % 4 == 0)."""
    base = _index(site, 1)
    f = fields(np.asarray(keys, dtype=np.uint64)[:, None], base | np.arange(H // 4, dtype=np.uint64)[None])
    return (f >= threshold(p)).reshape(len(keys), H)


def hidden_mult(keys, H, p, site):
    return np.where(hidden_keep(keys, H, p, site), scale(p), np.float32(0)).astype(np.float32)


def attn_keep(keys, B, nh, Lq, Lk, p, site):
    """bool [B, nh, Lq, Lk]: decisions on the attention probabilities; ``keys`` = the table of the [B, Lq] QUERY frame."""
    base = _index(site, nh)
    keys = np.asarray(keys, dtype=np.uint64).reshape(B, 1, Lq, 1)
    groups = (Lk + 3) // 4
    idx4 = base | (np.arange(nh, dtype=np.uint64).reshape(1, nh, 1, 1) << np.uint64(24)) | \
        np.arange(groups, dtype=np.uint64).reshape(1, 1, 1, groups)
    f = fields(keys, idx4)                                           # [B, nh, Lq, groups, 4]
    return (f >= threshold(p)).reshape(B, nh, Lq, 4 * groups)[..., :Lk]


def attn_mult(keys, B, nh, Lq, Lk, p, site):
    return np.where(attn_keep(keys, B, nh, Lq, Lk, p, site), scale(p), np.float32(0)).astype(np.float32)
