"""Packed variable-length batches: the rows of every item back to back, so that a chain costs the residues it has.

A ``PackedLayout`` is built once per batch from a [B, L] prefix padding mask (the dataset layout: valid positions first).
It holds the segment table the varlen attention kernel reads (``ops.attention_varlen``: int32 starts / lengths and the
(segment, q0) tile table on the device) and the gather index between the padded frame and the packed rows.  Packed
buffers have ``rows`` rows: the valid rows of all items, then a zero tail up to a multiple of 32, so that every GEMM and
row kernel keeps the shapes it is tested on; the attention kernel writes zeros into the tail's output rows.

Every op of the BERT stacks except attention is row-wise, so a packed forward runs the padded-frame executors on
[rows, H] activations (B = 1, L = rows) with the attention calls replaced by the varlen kernel.  Inference only.
"""
import torch

TILE = 32


class NotPackable(Exception):
    """The mask is not a prefix mask: the valid positions of some item are not its first ones."""


def _ceil(n, m=TILE):
    return -(-n // m) * m


def prefix_lengths(mask):
    """Per-item valid lengths of a [B, L] 0/1 mask whose valid positions are a prefix; ``NotPackable`` otherwise.
    (One read-back to the host: layouts are built once per batch, before a chain.)"""
    m = (mask.detach() != 0).to("cpu")
    if m.dim() != 2:
        raise ValueError(f"padding mask must be [B, L], got {tuple(m.shape)}")
    lengths = m.sum(dim=1)
    if m.shape[1] > 1 and not bool((m[:, :-1] >= m[:, 1:]).all()):
        raise NotPackable("padding mask is not a prefix mask: the batch cannot be packed")
    return [int(n) for n in lengths]


class PackedLayout:
    """Segments of ``lengths`` rows.  ``packed`` (default): segment s starts at sum(lengths[:s]) and ``rows`` is the
    total rounded up to a multiple of 32 (at least 32).  ``padded_frame`` = L: the segments sit in a padded [B, L]
    buffer instead (start s * L, ``rows`` = B * L; e.g. a pocket cache kept in its frame)."""

    def __init__(self, lengths, L, device, padded_frame=False):
        self.lengths = [int(n) for n in lengths]
        if any(n < 0 or n > L for n in self.lengths):
            raise ValueError(f"segment lengths must lie in [0, {L}], got {self.lengths}")
        self.B, self.L, self.device = len(self.lengths), int(L), torch.device(device)
        self.padded_frame = bool(padded_frame)
        self.total = sum(self.lengths)
        self.max_len = max(self.lengths, default=0)
        if self.padded_frame:
            self.starts = [s * self.L for s in range(self.B)]
            self.rows = self.B * self.L
        else:
            self.starts, at = [], 0
            for n in self.lengths:
                self.starts.append(at)
                at += n
            self.rows = max(TILE, _ceil(self.total))
        tiles = [(s, q0) for s, n in enumerate(self.lengths) for q0 in range(0, n, TILE)]
        if not self.padded_frame:          # zero the tail's output rows
            tiles += [(-1, r) for r in range(self.total, self.rows, TILE)]
        self.n_tiles = len(tiles)
        dev = self.device
        self.start_dev = torch.tensor(self.starts, dtype=torch.int32, device=dev)
        self.len_dev = torch.tensor(self.lengths, dtype=torch.int32, device=dev)
        self.tiles = torch.tensor(tiles, dtype=torch.int32, device=dev).reshape(-1, 2)
        self._index = {}

    @classmethod
    def from_mask(cls, mask, padded_frame=False):
        """Layout of the valid rows of a [B, L] prefix mask (``NotPackable`` for any other mask)."""
        return cls(prefix_lengths(mask), mask.shape[1], mask.device, padded_frame)

    def index(self, L=None):
        """int64 device index [total]: packed row i <- padded-frame row b * L + l."""
        L = self.L if L is None else int(L)
        idx = self._index.get(L)
        if idx is None:
            flat = [b * L + l for b, n in enumerate(self.lengths) for l in range(n)]
            idx = self._index[L] = torch.tensor(flat, dtype=torch.int64, device=self.device)
        return idx

    def pack(self, x, dim=0):
        """x [.., B, L, ..] (B at ``dim``) -> [.., rows, ..] with the valid rows first and a zero tail."""
        assert not self.padded_frame, "a padded-frame layout has nothing to pack"
        assert x.shape[dim] == self.B, (tuple(x.shape), dim, self.B)
        flat = x.flatten(dim, dim + 1)
        shape = list(flat.shape)
        shape[dim] = self.rows
        out = torch.zeros(shape, dtype=x.dtype, device=x.device)
        out.narrow(dim, 0, self.total).copy_(flat.index_select(dim, self.index(x.shape[dim + 1])))
        return out

    def unpack(self, y, L=None, dim=0):
        """y [.., rows, ..] -> [.., B, L, ..] (L defaults to the mask's frame) with zeros at the padding positions."""
        assert not self.padded_frame, "a padded-frame layout has nothing to unpack"
        L = self.L if L is None else int(L)
        assert y.shape[dim] >= self.total and L >= self.max_len, (tuple(y.shape), L, self.max_len)
        shape = list(y.shape)
        shape[dim] = self.B * L
        out = torch.zeros(shape, dtype=y.dtype, device=y.device)
        out.index_copy_(dim, self.index(L), y.narrow(dim, 0, self.total))
        return out.unflatten(dim, (self.B, L))

    def same_segments(self, other):
        return self.lengths == other.lengths


def check_cross(q_layout, k_layout):
    """Cross-attention pairs segment s of the queries with segment s of the keys: the counts must agree, and a query
    segment with rows needs keys (the reference's fully masked softmax cannot be reproduced without the padding)."""
    if q_layout.B != k_layout.B:
        raise ValueError(f"segment counts differ: {q_layout.B} queries against {k_layout.B} keys")
    empty = [s for s, (nq, nk) in enumerate(zip(q_layout.lengths, k_layout.lengths)) if nq > 0 and nk == 0]
    if empty:
        raise ValueError(f"items {empty} have ligand rows but an empty pocket: a packed batch cannot reproduce the "
                         "fully masked softmax of such an item (run it padded)")


def layouts_or_none(ligand_mask, receptor_mask):
    """(ligand layout, pocket layout) of a batch, or None when a mask is not a prefix mask (the samplers then run the
    trimmed frame instead).  An item with ligand rows and an empty pocket raises ``ValueError``."""
    try:
        lig, rec = PackedLayout.from_mask(ligand_mask), PackedLayout.from_mask(receptor_mask)
    except NotPackable:
        return None
    check_cross(lig, rec)
    return lig, rec
