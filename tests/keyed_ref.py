"""Vectorised numpy restatement of the keyed sampling streams ("Keyed sampling streams"): Philox4x32-10,
the counter layout and the maps to uniforms, normals and classes.  The tests hold the HIP kernels to it; the product
does not import it."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr uint32 [..., 4], key uint32 [..., 2] (broadcast) -> uint32 [..., 4]."""
    ctr = np.asarray(ctr, dtype=np.uint32)
    key = np.asarray(key, dtype=np.uint32)
    c0, c1, c2, c3 = (ctr[..., i].astype(np.uint64) for i in range(4))
    k0, k1 = key[..., 0].astype(np.uint32), key[..., 1].astype(np.uint32)
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0, p1 = M0 * c0, M1 * c2
            n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0.astype(np.uint64)
            n1 = p1 & MASK32
            n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1.astype(np.uint64)
            n3 = p0 & MASK32
            c0, c1, c2, c3 = n0, n1, n2, n3
            k0 = k0 + W0
            k1 = k1 + W1
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def words(seed, item, stream, t, position, block):
    """Philox words of (seed, item id, stream, step, position, block); array arguments broadcast."""
    if not 0 <= int(t) <= 65535:
        raise ValueError("step outside [0, 65535]")
    item = np.asarray(item, dtype=np.uint64)
    position = np.asarray(position, dtype=np.uint64)
    if (position >= 1 << 24).any():
        raise ValueError("position outside [0, 2^24)")
    block = np.asarray(block, dtype=np.uint64)
    item, position, block = np.broadcast_arrays(item, position, block)
    ctr = np.stack([item & MASK32, item >> np.uint64(32),
                    np.full(item.shape, (int(stream) << 16) | int(t), dtype=np.uint64),
                    (position << np.uint64(8)) | block], axis=-1).astype(np.uint32)
    seed = int(seed)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    return philox4x32_10(ctr, key)


def uniform(w):
    """[0, 1) from the top 24 bits (exact in fp32)."""
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def klass(w, C):
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.uint64) * np.uint64(C) >> np.uint64(24)).astype(np.int64)


def normal4(w):
    """Box-Muller on (w0, w1), (w2, w3) -> float64 [..., 4] (the device computes it in fp32)."""
    w = np.asarray(w, dtype=np.uint32)
    out = np.empty(w.shape, dtype=np.float64)
    for p in range(2):
        u1 = ((w[..., 2 * p] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (w[..., 2 * p + 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        out[..., 2 * p] = r * np.cos(2 * np.pi * u2)
        out[..., 2 * p + 1] = r * np.sin(2 * np.pi * u2)
    return out


def _split_keys(keys):
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 2)
    return keys[:, 0].astype(np.uint64), keys[:, 1], keys[:, 1] >= 0


def normals(keys, seed, stream, t, F):
    """[rows, F] normals of a key table (rows of no item: 0)."""
    item, pos, valid = _split_keys(keys)
    nb = F // 4
    w = words(seed, item[:, None], stream, t, np.where(valid, pos, 0)[:, None], np.arange(nb)[None])
    z = normal4(w).reshape(len(item), F)
    z[~valid] = 0.0
    return z


def uniforms(keys, seed, stream, t):
    item, pos, valid = _split_keys(keys)
    u = uniform(words(seed, item, stream, t, np.where(valid, pos, 0), 0)[..., 0])
    return np.where(valid, u, np.float32(0))


def classes(keys, seed, stream, t, C):
    item, pos, valid = _split_keys(keys)
    k = klass(words(seed, item, stream, t, np.where(valid, pos, 0), 0)[..., 0], C)
    return np.where(valid, k, 0)
