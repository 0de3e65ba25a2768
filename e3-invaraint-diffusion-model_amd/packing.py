"""Packed variable-length batches: the rows of every item back to back, so that a chain costs the residues it has.

A ``PackedLayout`` is built once per batch from a [B, L] prefix padding mask (the dataset layout: valid positions first).
It holds the segment table the varlen attention kernel reads (``ops.attention_varlen``: int32 starts / lengths and the
(segment, q0) tile table on the device) and the gather index between the padded frame and the packed rows.  Packed
buffers have ``rows`` rows: the valid rows of all items, then a zero tail up to a multiple of 32, so that every GEMM and
row kernel keeps the shapes it is tested on; the attention kernel writes zeros into the tail's output rows.

Every op of the BERT stacks except attention is row-wise, so a packed forward runs the executors of the padded frame on
[rows, H] activations; a ``Rows`` record tells the two attention executors which kernel to call.  Inference only.

A ``Frame`` is the choice both samplers make once per chain between the padded, the trimmed and the packed rows.
"""
import os
import warnings

import torch

from . import keyed

TILE = 32
# ligand rows up to which a sampling chain replays a captured graph by default (B=8 x L=64: 2.05 vs 2.16 ms eager;
# B=16: GPU-bound, eager); E3D_SAMPLE_GRAPH=0/1 overrides
GRAPH_MAX_ROWS = 512


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


def trimmed_length(mask, multiple=TILE):
    """Smallest multiple of ``multiple`` that covers every valid position of a [B,L] 0/1 padding mask whose valid
    positions are a prefix (the dataset layout, dataset.py:119-132); L itself if any row is not a prefix mask."""
    try:
        longest = max(prefix_lengths(mask), default=0)
    except NotPackable:
        return mask.shape[1]
    return max(multiple, min(mask.shape[1], _ceil(longest, multiple)))


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


class Rows:
    """The rows of one activation matrix x [rows, H], as the model layer's executors (``bert.run_*``, ``SELayer.run``)
    take them.  Padded (``from_mask``): the [B, L] frame, its float key mask [B, L] and, in a keyed training step, the
    key table of its rows (``row_keys``; else None).  Packed (``from_layout``): the segments of a ``PackedLayout`` -- a
    ``padded_frame`` one, e.g. a pocket cache kept in its frame, included.  The fields of the other form are None.
    A record of references: nothing is allocated, launched or read back from the device."""

    def __init__(self, rows, B=None, L=None, mask=None, row_keys=None, layout=None):
        self.rows, self.B, self.L, self.mask, self.row_keys, self.layout = rows, B, L, mask, row_keys, layout
        self.packed = layout is not None

    @classmethod
    def from_mask(cls, mask, row_keys=None):
        B, L = mask.shape
        return cls(B * L, B, L, mask, row_keys)

    @classmethod
    def from_layout(cls, layout):
        return cls(layout.rows, layout=layout)


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


class Frame:
    """The rows a sampling chain runs on, chosen once per chain from the batch's [B, L] ligand and pocket masks:

    * padded (default): the dataset's [B, L] frame;
    * trimmed (``trim``): the rows up to the longest ligand / pocket, rounded up to 32 (``trimmed_length``).  Padding
      cannot influence valid positions while a row's attention scores spread over less than ~9900 (its keys carry
      the -10000 bias, whose softmax weight then underflows to exactly 0.0f; every other op is row-wise), so a chain
      needs no other rows.  BioLiP ligands are 5-30 residues in a 64-256 row frame: the decoder then runs on 1/8 of
      the rows;
    * packed (``pack``): every item's valid rows back to back (``layouts``: ligand and pocket ``PackedLayout``).  Masks
      that are not prefix masks cannot be packed: the trimmed frame runs instead, with a warning.  An item with ligand
      rows but an empty pocket raises ``ValueError``.

    The condition.  Trimmed and packed frames equal the padded one on the valid positions while every softmax row's
    scores spread over less than ~9900.  Beyond that the reference's additive -10000 mask lets padded keys win rows of
    the padded frame; a trimmed frame has dropped (some of) those keys, and the packed path computes the absent-keys
    softmax -- keys outside a segment have weight exactly 0, whatever the scores.  That contract is pinned by
    tests/test_varlen_forms_gpu.py::
    test_packed_path_computes_the_absent_keys_softmax_where_the_reference_lets_padded_keys_win.

    ``ligand`` / ``pocket`` move a padded-frame tensor into the frame, ``restore`` moves a ligand-side result back;
    ``row_keys`` is the key table of the frame's ligand rows (keyed.py) and ``rows`` their count."""

    def __init__(self, ligand_mask, receptor_mask, trim=False, pack=False):
        self.B, self.L = ligand_mask.shape
        self.layouts = layouts_or_none(ligand_mask, receptor_mask) if pack else None
        if pack and self.layouts is None:
            warnings.warn("pack=True: a padding mask is not a prefix mask, so the batch cannot be packed; running the "
                          "trimmed frame instead")
            trim = True
        self.Ll, self.Lr = self.L, receptor_mask.shape[1]
        if trim and self.layouts is None:
            self.Ll, self.Lr = min(self.Ll, trimmed_length(ligand_mask)), min(self.Lr, trimmed_length(receptor_mask))
        self.rows = self.B * self.Ll if self.layouts is None else self.layouts[0].rows

    def _move(self, x, dim, n, side):
        if self.layouts is not None:
            return self.layouts[side].pack(x, dim)
        return x if x.shape[dim + 1] == n else x.narrow(dim + 1, 0, n).contiguous()

    def ligand(self, x, dim=0):
        """x [.., B, L, ..] (B at ``dim``) on the ligand rows of the frame: x itself (padded), its first ``Ll`` rows
        (trimmed, contiguous) or the packed rows [.., rows, ..]."""
        return self._move(x, dim, self.Ll, 0)

    def pocket(self, x, dim=0):
        """``ligand`` for a pocket-side tensor (``Lr`` rows when trimmed)."""
        return self._move(x, dim, self.Lr, 1)

    def restore(self, y, dim=0):
        """A ligand-side result in the frame -> [.., B, L, ..], with zeros at the rows the frame dropped."""
        if self.layouts is not None:
            return self.layouts[0].unpack(y, dim=dim)
        if self.Ll == self.L:
            return y
        shape = list(y.shape)
        shape[dim + 1] = self.L
        out = y.new_zeros(shape)
        out.narrow(dim + 1, 0, self.Ll).copy_(y)
        return out

    def row_keys(self, ids, device):
        """Key table of the frame's ligand rows for the item ids ``ids``."""
        if self.layouts is not None:
            return keyed.packed_keys(self.layouts[0], ids, device)
        return keyed.padded_keys(ids, self.Ll, device)


def parse_keep(spec):
    """A position list such as "0-3,7" -> the sorted 0-based positions it names (inclusive ranges; "" -> none).  A
    malformed list raises ``ValueError`` with the offending token."""
    if not isinstance(spec, str):
        raise TypeError(f"keep: expected a position list such as '0-3,7', got {type(spec).__name__}")
    positions = set()
    for token in spec.split(","):
        tok = token.strip()
        if not tok:
            if spec.strip():
                raise ValueError(f"keep: empty entry in position list {spec!r}")
            continue
        lo, dash, hi = tok.partition("-")
        lo, hi = lo.strip(), hi.strip()
        if not (lo.isdigit() and lo.isascii()) or (dash and not (hi.isdigit() and hi.isascii())):
            raise ValueError(f"keep: malformed entry {tok!r} in position list {spec!r} (expected N or N-M)")
        a, b = int(lo), int(hi) if dash else int(lo)
        if b < a:
            raise ValueError(f"keep: descending range {tok!r} in position list {spec!r}")
        positions.update(range(a, b + 1))
    return sorted(positions)


def keep_mask(keep, index, L, length=None):
    """bool [L]: the ligand positions of dataset item ``index`` that a partial redesign holds.  ``keep``: a position list
    (``parse_keep``; applied to every item, positions at or beyond ``length`` -- default L -- ignored) or a callable
    index -> bool [L]."""
    length = L if length is None else min(int(length), L)
    if callable(keep):
        m = torch.as_tensor(keep(index))
        if m.dtype != torch.bool or tuple(m.shape) != (L,):
            raise ValueError(f"keep({index}) must return a bool [{L}] mask, got {m.dtype} {tuple(m.shape)}")
        m = m.clone().cpu()
    else:
        m = torch.zeros(L, dtype=torch.bool)
        pos = [p for p in parse_keep(keep) if p < length]
        if pos:
            m[pos] = True
    m[length:] = False
    return m


def capture_graph(capture, rows, steps, use_graph=None, what="the reverse step"):
    """The captured step ``capture()`` of a chain of ``steps`` steps on ``rows`` ligand rows, or None: eager launches.
    ``use_graph`` None: replay for at most GRAPH_MAX_ROWS rows (E3D_SAMPLE_GRAPH=0/1 overrides); chains of at most 4
    steps never replay.  A capture that fails warns and falls back to eager launches, which are always correct."""
    if use_graph is None:
        env = os.environ.get("E3D_SAMPLE_GRAPH")
        use_graph = env == "1" if env in ("0", "1") else rows <= GRAPH_MAX_ROWS
    if not use_graph or steps <= 4:
        return None
    try:
        return capture()
    except Exception as e:   # noqa: BLE001 -- any capture problem: eager launches are always correct
        warnings.warn(f"HIP-graph capture of {what} failed ({type(e).__name__}: {e}); using eager launches")
        return None


def warm_up_and_capture(body, device, restore_rng=False):
    """``body()`` once on a side stream, off the capture (first-launch attribute calls, caches, the allocator: one eager
    step per chain), then captured into a HIP graph; returns (graph, what the captured ``body()`` returned).
    ``restore_rng``: put the device generator back after the warm-up, so that a chain sees the same random numbers
    whether its steps are replayed or launched one by one (a size threshold decides which)."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    rng = torch.cuda.get_rng_state(device) if restore_rng else None
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream(device).wait_stream(side)
    if restore_rng:
        torch.cuda.synchronize(device)
        torch.cuda.set_rng_state(rng, device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = body()
    return graph, out
