"""Keyed sampling streams: the row-key tables of seeded chains.

A seeded chain draws every random number from Philox4x32-10 keyed by the seed, with the counter
(item id, stream << 16 | step, position << 8 | block) -- DESIGN.md, "Keyed sampling streams"; csrc/e3d_philox.h.  The
kernels find (item id, position) of a row in a key table, int64 [rows, 2], built here once per chain for the frame the
chain runs in: the padded [B, L] frame, a trimmed frame (the same positions, fewer of them) or a ``packing.PackedLayout``
(position = row - segment start; the zero tail gets ``SENTINEL`` and draws nothing).  The valid rows of one item carry
the same keys in all three, so an item gets the same draws whatever its batch, order or frame.

Training and validation draws (streams 4-7, ``training.fit(seed=)``) put the epoch in the step field -- VALIDATION_EPOCH for
validation -- and need no key table: their frames are padded or trimmed, so the kernels take the batch's item ids and the
epoch from device memory (``epoch_word``), where a captured training step finds the current ones at every replay.
Dropout decisions of a seeded step (streams 8 / 9) are keyed the same way: one 64-bit key per frame row, built inside the
step from the ids and the epoch word (``ops.keyed_drop_row_keys``), seeds the generator of that row's decisions.

Item ids are the caller's (the module entry points use the global dataset index).  Two items with the same id and seed
get the same draws: replicate samples of one pocket take one seed per replicate, or ids that encode (pocket, replicate).
"""
import torch

SENTINEL = -1
MAX_POSITION = 1 << 24          # c3 = position << 8 | block
MAX_STEP = 65535                # c2 = stream << 16 | step

# streams (counter word c2 = stream << 16 | step)
STRUCT_XT, STRUCT_STEP, SEQ_XT, SEQ_U = 0, 1, 2, 3
# training and validation draws: the step field is the epoch (0 .. MAX_EPOCH), VALIDATION_EPOCH for validation
TRAIN_STRUCT_T, TRAIN_STRUCT_NOISE, TRAIN_SEQ_T, TRAIN_SEQ_U = 4, 5, 6, 7
VALIDATION_EPOCH = 65535
MAX_EPOCH = VALIDATION_EPOCH - 1
# dropout decisions of a seeded training step: a frame row's 64-bit key is w0 | w1 << 32 of (seed, item id, stream, epoch,
# position, block 0); an item's ligand position l and pocket position l must not share decisions, hence two streams
DROP_LIGAND, DROP_POCKET = 8, 9
# partial redesign (replacement conditioning): the forward-noised copies of the held ligand positions, drawn at the step
# index of the chain; streams 1 and 3 stay as they are, so the free positions draw what they drew before.
# sample.score_sequences noises a supplied sequence with KNOWN_SEQ too: the same law at the same step field
KNOWN_STRUCT, KNOWN_SEQ = 10, 11
# structure_model.sample.score_structures: the forward noise of a supplied backbone at the level that timestep t READS,
# step field = t.  Stream 10 is not reused for it: KNOWN_STRUCT is drawn at the step whose LANDING level is t - 1 (the step
# field t holds the noise of level t - 1), and it has no draw for level T - 1, the first one a score needs.  A stream of
# its own also keeps streams 0 - 11 untouched: a seeded chain draws what it drew before.
SCORE_STRUCT = 12


def check_seed(seed):
    """The seed as a Python int in [0, 2^64) (the 64-bit Philox key)."""
    if isinstance(seed, bool) or not isinstance(seed, int):
        try:
            seed = int(seed)
        except (TypeError, ValueError):
            raise TypeError(f"seed must be an integer, got {seed!r}") from None
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must lie in [0, 2^64), got {seed}")
    return seed


def check_steps(T):
    if T - 1 > MAX_STEP:
        raise ValueError(f"keyed streams hold steps up to {MAX_STEP}; a chain of {T} steps does not fit")


def check_epoch(epoch):
    """A training epoch as a Python int in [0, MAX_EPOCH]; the value after it is the validation draw's."""
    epoch = int(epoch)
    if not 0 <= epoch <= MAX_EPOCH:
        raise ValueError(f"keyed training streams hold epochs 0 .. {MAX_EPOCH} ({VALIDATION_EPOCH} is the validation "
                         f"draw), got {epoch}")
    return epoch


def epoch_word(device, epoch=0):
    """The int64 scalar in device memory that the training-draw kernels read their epoch from."""
    return torch.full((1,), check_epoch(epoch), dtype=torch.int64, device=device)


def set_epoch(word, epoch):
    """Fill an epoch word in place (a captured step keeps reading the same memory); ``None``: the validation value."""
    word.fill_(VALIDATION_EPOCH if epoch is None else check_epoch(epoch))
    return word


def device_item_ids(ids, B, device):
    """Item ids as the int64 [B] device tensor the training-draw kernels read (ids >= 2^63 as the int64 of the same
    bits).  An int64 tensor -- a batch's ``item_id`` -- is taken as it is."""
    if torch.is_tensor(ids) and ids.dtype == torch.int64:
        if ids.numel() != B:
            raise ValueError(f"{ids.numel()} item ids for a batch of {B}")
        return ids.reshape(B).to(device).contiguous()
    return _as_int64(item_ids(ids, B)).to(device)


def batch_item_ids(batch, B):
    """The ``item_id`` entry of a batch as the int64 [B] tensor the training-draw kernels read."""
    ids = batch.get("item_id")
    if ids is None:
        raise ValueError("seeded training draws are keyed by the batch's 'item_id' (int64 [B], the index in the split's "
                         "dataset) and this batch has none: wrap the dataset in training.ItemIdDataset")
    if not torch.is_tensor(ids) or ids.dtype != torch.int64 or ids.numel() != B:
        raise ValueError(f"batch['item_id'] must be an int64 tensor of {B} ids")
    return ids.reshape(B).contiguous()


def item_ids(ids, B):
    """Item ids as a list of B Python ints in [0, 2^64); ``None`` -> 0 .. B-1."""
    if ids is None:
        return list(range(B))
    ids = [int(i) for i in (ids.tolist() if torch.is_tensor(ids) else ids)]
    if len(ids) != B:
        raise ValueError(f"{len(ids)} item ids for a batch of {B}")
    if any(not 0 <= i < 1 << 64 for i in ids):
        raise ValueError("item ids must lie in [0, 2^64)")
    return ids


def _as_int64(ids):
    """[0, 2^64) -> the int64 of the same bit pattern (the kernels read the word as unsigned)."""
    return torch.tensor([i - (1 << 64) if i >= 1 << 63 else i for i in ids], dtype=torch.int64)


def padded_keys(ids, L, device):
    """Key table of a [B, L] frame: row b * L + l = (ids[b], l).  A trimmed frame is the same with its shorter L."""
    if L > MAX_POSITION:
        raise ValueError(f"keyed streams hold positions below 2^24, got a frame of {L}")
    B = len(ids)
    keys = torch.empty((B, L, 2), dtype=torch.int64)
    keys[:, :, 0] = _as_int64(ids)[:, None]
    keys[:, :, 1] = torch.arange(L, dtype=torch.int64)[None]
    return keys.reshape(B * L, 2).to(device)


def packed_keys(layout, ids, device=None):
    """Key table of a packed buffer: row start_s + l = (ids[s], l) for l < lengths[s]; the tail rows get SENTINEL."""
    if len(ids) != layout.B:
        raise ValueError(f"{len(ids)} item ids for a layout of {layout.B} segments")
    if layout.max_len > MAX_POSITION:
        raise ValueError("keyed streams hold positions below 2^24")
    keys = torch.full((layout.rows, 2), SENTINEL, dtype=torch.int64)
    sid = _as_int64(ids)
    for s, (start, n) in enumerate(zip(layout.starts, layout.lengths)):
        keys[start:start + n, 0] = sid[s]
        keys[start:start + n, 1] = torch.arange(n, dtype=torch.int64)
    return keys.to(layout.device if device is None else device)
