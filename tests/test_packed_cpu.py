"""Packed variable-length layouts (packing.py): segment tables, tile tables, pack / unpack -- host-side, no GPU."""
import pytest
import torch


def _mask(lengths, L):
    return (torch.arange(L)[None, :] < torch.tensor(lengths)[:, None]).float()


def test_layout_from_prefix_mask_starts_lengths_and_tiles(pkg):
    P = pkg.packing
    lengths = [0, 1, 31, 32, 33, 256]
    lay = P.PackedLayout.from_mask(_mask(lengths, 256))
    assert lay.lengths == lengths and lay.B == 6 and lay.L == 256
    assert lay.starts == [0, 0, 1, 32, 64, 97]
    assert lay.start_dev.dtype == torch.int32 and lay.start_dev.tolist() == lay.starts
    assert lay.len_dev.dtype == torch.int32 and lay.len_dev.tolist() == lengths
    assert lay.total == 353 and lay.max_len == 256
    assert lay.rows == 384 and lay.rows % 32 == 0
    want = [(1, 0), (2, 0), (3, 0), (4, 0), (4, 32)] + [(5, q0) for q0 in range(0, 256, 32)] + [(-1, 353)]
    assert [tuple(t) for t in lay.tiles.tolist()] == want and lay.n_tiles == len(want)
    # every valid row is covered by exactly one tile, the tail by the (-1, row0) blocks
    covered = []
    for s, q0 in want:
        if s < 0:
            covered += list(range(q0, min(q0 + 32, lay.rows)))
        else:
            covered += [lay.starts[s] + q0 + i for i in range(min(32, lengths[s] - q0))]
    assert sorted(covered) == list(range(lay.rows))


@pytest.mark.parametrize("lengths,rows", [([5], 32), ([32], 32), ([33], 64), ([0, 0], 32), ([30, 30, 5], 96),
                                          ([64, 64], 128)])
def test_rows_round_up_to_32(pkg, lengths, rows):
    lay = pkg.packing.PackedLayout(lengths, 64, "cpu")
    assert lay.rows == rows
    tail = [t for t in lay.tiles.tolist() if t[0] < 0]
    assert [t[1] for t in tail] == list(range(lay.total, rows, 32))


def test_padded_frame_layout(pkg):
    lay = pkg.packing.PackedLayout([3, 0, 40], 64, "cpu", padded_frame=True)
    assert lay.starts == [0, 64, 128] and lay.rows == 192
    assert [tuple(t) for t in lay.tiles.tolist()] == [(0, 0), (2, 0), (2, 32)]


def test_pack_unpack_round_trip(pkg):
    lengths, L = [7, 0, 30, 1], 32
    mask = _mask(lengths, L)
    lay = pkg.packing.PackedLayout.from_mask(mask)
    x = torch.randn(4, L, 8) * mask[..., None]
    p = lay.pack(x)
    assert p.shape == (lay.rows, 8) and lay.rows == 64
    assert torch.equal(p[:7], x[0, :7]) and torch.equal(p[7:37], x[2, :30]) and torch.equal(p[37], x[3, 0])
    assert (p[lay.total:] == 0).all()
    assert torch.equal(lay.unpack(p), x)
    # a wider frame and a leading (time) dimension
    y = lay.unpack(torch.stack([p, 2 * p]), L=48, dim=1)
    assert y.shape == (2, 4, 48, 8)
    assert torch.equal(y[0, :, :L], x) and torch.equal(y[1, :, :L], 2 * x) and (y[:, :, L:] == 0).all()
    assert torch.equal(lay.pack(y, dim=1)[1], 2 * p)
    # padding values never reach the packed rows
    noisy = x + (1 - mask)[..., None] * 5.0
    assert torch.equal(lay.pack(noisy), p)


def test_non_prefix_mask_is_refused_and_the_sampler_falls_back(pkg):
    P = pkg.packing
    mask = _mask([5, 9], 16)
    holes = mask.clone()
    holes[0, 10] = 1.0
    with pytest.raises(P.NotPackable):
        P.PackedLayout.from_mask(holes)
    rec = _mask([20, 20], 32)
    assert P.layouts_or_none(holes, rec) is None         # p_sample_loop(pack=True) then runs the trimmed frame
    assert P.layouts_or_none(mask, _mask([20, 20], 32)) is not None
    rec_holes = rec.clone()
    rec_holes[1, 25] = 1.0
    assert P.layouts_or_none(mask, rec_holes) is None    # (the pocket's mask counts as well)


def test_ligand_with_an_empty_pocket_raises(pkg):
    P = pkg.packing
    lig, rec = _mask([5, 0, 7], 32), _mask([20, 0, 0], 64)
    with pytest.raises(ValueError, match="empty pocket"):
        P.layouts_or_none(lig, rec)
    # an empty ligand needs no pocket
    lig_ok = _mask([5, 0, 0], 32)
    lay, rec_lay = P.layouts_or_none(lig_ok, rec)
    assert lay.lengths == [5, 0, 0] and rec_lay.lengths == [20, 0, 0]


def test_attention_varlen_is_declared_at_abi_v5(pkg):
    assert pkg.hip.ABI_VERSION == 5 and "e3d_attn_varlen_fwd" in pkg.hip.EXPORTS
    lib = pkg.hip.lib()
    assert lib.e3d_abi_version() == 5
    # argument validation before any launch: callable without a GPU
    rc = lib.e3d_attn_varlen_fwd(None, 64, None, 64, None, 64, None, None, None, None, None, 1, None, 0, None, 32, 1,
                                 1, 1, 6, None)
    assert rc != 0 and b"null pointer" in lib.e3d_last_error()


def test_samplers_default_to_the_unpacked_frame(pkg):
    import inspect
    from e3diff_amd.sequence_model import sample as Q
    from e3diff_amd.structure_model import sample as S
    assert inspect.signature(S.p_sample_loop).parameters["pack"].default is False
    assert inspect.signature(Q.denoise).parameters["pack"].default is False


def test_frames_move_in_restore_and_key_tables(pkg):
    """packing.Frame, the frame of both samplers' chains: its rows, ligand / pocket tensors moved in (the [B, L] axes at
    dim 0 or 1), results restored to the padded frame with zeros where the frame dropped rows, and its key table."""
    P, K = pkg.packing, pkg.keyed
    lig_len, rec_len, L, Lr = [7, 0, 30, 1], [40, 3, 33, 20], 96, 128
    lig, rec = _mask(lig_len, L), _mask(rec_len, Lr)
    ids = [5, 1 << 40, 2, 9]
    x = torch.randn(4, L, 8) * lig[..., None]
    noises = torch.randn(3, 4, L, 8)                     # [T, B, L, F], non-zero at padding
    pocket = torch.randn(4, Lr, 8)
    valid = lig.bool()[None, :, :, None].expand_as(noises)

    padded = P.Frame(lig, rec)
    assert padded.layouts is None and (padded.Ll, padded.Lr, padded.rows) == (L, Lr, 4 * L)
    assert padded.ligand(noises, dim=1) is noises and padded.pocket(pocket) is pocket and padded.restore(x) is x
    assert torch.equal(padded.row_keys(ids, "cpu"), K.padded_keys(ids, L, "cpu"))

    trimmed = P.Frame(lig, rec, trim=True)
    assert trimmed.layouts is None and (trimmed.Ll, trimmed.Lr, trimmed.rows) == (32, 64, 4 * 32)
    t = trimmed.ligand(noises, dim=1)
    assert t.shape == (3, 4, 32, 8) and t.is_contiguous() and torch.equal(t, noises[:, :, :32])
    assert torch.equal(trimmed.pocket(pocket), pocket[:, :64])
    back = trimmed.restore(t, dim=1)
    assert back.shape == noises.shape and torch.equal(back[:, :, :32], t) and (back[:, :, 32:] == 0).all()
    assert torch.equal(trimmed.restore(trimmed.ligand(x)), x)
    assert torch.equal(trimmed.row_keys(ids, "cpu"), K.padded_keys(ids, 32, "cpu"))

    packed = P.Frame(lig, rec, pack=True, trim=True)     # packing wins over trimming
    lay, lay_r = packed.layouts
    assert lay.lengths == lig_len and lay_r.lengths == rec_len and packed.rows == lay.rows == 64
    p = packed.ligand(noises, dim=1)
    assert p.shape == (3, 64, 8) and torch.equal(p, lay.pack(noises, dim=1))
    assert torch.equal(packed.pocket(pocket), lay_r.pack(pocket))
    back = packed.restore(p, dim=1)
    assert back.shape == noises.shape and torch.equal(back[valid], noises[valid]) and (back[~valid] == 0).all()
    assert torch.equal(packed.restore(packed.ligand(x)), x)
    assert torch.equal(packed.row_keys(ids, "cpu"), K.packed_keys(lay, ids, "cpu"))


def test_frame_falls_back_from_packed_to_trimmed(pkg):
    P = pkg.packing
    lig, rec = _mask([5, 9], 64), _mask([20, 40], 96)
    holes = lig.clone()
    holes[0, 40] = 1.0
    assert P.trimmed_length(holes) == 64                # not a prefix mask: trimming keeps every row
    with pytest.warns(UserWarning, match="cannot be packed"):
        f = P.Frame(holes, rec, pack=True)
    assert f.layouts is None and (f.Ll, f.Lr) == (64, 64)
    rec_holes = rec.clone()
    rec_holes[1, 90] = 1.0
    with pytest.warns(UserWarning, match="cannot be packed"):
        f = P.Frame(lig, rec_holes, pack=True)
    assert f.layouts is None and (f.Ll, f.Lr) == (32, 96)
    # an item with ligand rows and an empty pocket cannot be packed; the other frames run it
    empty = _mask([20, 0], 96)
    with pytest.raises(ValueError, match="empty pocket"):
        P.Frame(lig, empty, pack=True)
    assert P.Frame(lig, empty, trim=True).Lr == 32
    # a frame shorter than one 32-row tile has nothing to trim
    short = _mask([5, 3], 16)
    assert P.trimmed_length(short) == 32 and P.Frame(short, short, trim=True).Ll == 16


def test_graph_capture_default_override_and_fallback(pkg, monkeypatch):
    P = pkg.packing
    monkeypatch.delenv("E3D_SAMPLE_GRAPH", raising=False)
    made = []

    def capture():
        made.append(1)
        return "graph"

    assert P.capture_graph(capture, P.GRAPH_MAX_ROWS, 5) == "graph"
    assert P.capture_graph(capture, P.GRAPH_MAX_ROWS + 1, 5) is None
    assert P.capture_graph(capture, 64, 4) is None                        # chains of <= 4 steps never replay
    assert P.capture_graph(capture, 1 << 20, 5, use_graph=True) == "graph"
    assert P.capture_graph(capture, 64, 5, use_graph=False) is None
    monkeypatch.setenv("E3D_SAMPLE_GRAPH", "0")
    assert P.capture_graph(capture, 64, 5) is None
    monkeypatch.setenv("E3D_SAMPLE_GRAPH", "1")
    assert P.capture_graph(capture, 1 << 20, 5) == "graph"
    assert len(made) == 3

    def broken():
        raise RuntimeError("no capture here")

    with pytest.warns(UserWarning, match="HIP-graph capture of the test step failed"):
        assert P.capture_graph(broken, 64, 5, what="the test step") is None
