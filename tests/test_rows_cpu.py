"""The two records the model layer's executors take (packing.Rows, bert.Drop) -- host-side, no GPU."""
import pytest
import torch

LENGTHS, L = (5, 32), 32


def _mask():
    return (torch.arange(L)[None, :] < torch.tensor(LENGTHS)[:, None]).float()


def _encoder(pkg, **rates):
    cfg = pkg.bert.BertConfig(hidden_size=256, num_attention_heads=4, intermediate_size=256, num_hidden_layers=1,
                              max_position_embeddings=L, **rates)
    return pkg.bert.BertEncoder(cfg)


def test_rows_of_a_padded_frame(pkg):
    mask, keys = _mask(), torch.arange(2 * L)
    rows = pkg.packing.Rows.from_mask(mask, keys)
    assert (rows.B, rows.L, rows.rows) == (2, L, 2 * L) and rows.packed is False
    assert rows.mask is mask and rows.row_keys is keys and rows.layout is None
    assert pkg.packing.Rows.from_mask(mask).row_keys is None


def test_rows_of_packed_layouts(pkg):
    P = pkg.packing
    lay = P.PackedLayout.from_mask(_mask())
    rows = P.Rows.from_layout(lay)
    assert rows.rows == 64 and rows.packed is True           # 5 + 32 valid rows, rounded up to 32
    assert rows.layout is lay and rows.mask is None and rows.row_keys is None
    framed = P.PackedLayout.from_mask(_mask(), padded_frame=True)
    rows = P.Rows.from_layout(framed)
    assert rows.rows == framed.rows == 2 * L and rows.packed is True and rows.layout is framed


def test_drop_is_off_in_eval_mode(pkg):
    enc = _encoder(pkg, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.2).eval()
    for rows in (pkg.packing.Rows.from_mask(_mask()), pkg.packing.Rows.from_layout(pkg.packing.PackedLayout.from_mask(_mask()))):
        drop = pkg.bert.Drop.of(enc, rows)
        assert drop.off and (drop.hidden, drop.attention, drop.row_keys) == (0.0, 0.0, None)


def test_drop_in_training_mode_carries_the_rates_and_the_key_table(pkg):
    enc = _encoder(pkg, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.2).train()
    keys = torch.arange(2 * L)
    drop = pkg.bert.Drop.of(enc, pkg.packing.Rows.from_mask(_mask(), keys))
    assert not drop.off and (drop.hidden, drop.attention) == (0.1, 0.2) and drop.row_keys is keys
    assert pkg.bert.Drop.of(enc, pkg.packing.Rows.from_mask(_mask())).row_keys is None
    # a module that trains without dropout drops nothing
    assert pkg.bert.Drop.of(_encoder(pkg, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0).train(),
                            pkg.packing.Rows.from_mask(_mask())).off


@pytest.mark.parametrize("rates", [(0.1, 0.0), (0.0, 0.1), (0.1, 0.1)])
def test_drop_refuses_packed_rows_in_training_mode(pkg, rates):
    enc = _encoder(pkg, hidden_dropout_prob=rates[0], attention_probs_dropout_prob=rates[1]).train()
    packed = pkg.packing.Rows.from_layout(pkg.packing.PackedLayout.from_mask(_mask()))
    with pytest.raises(RuntimeError, match="packed layouts are inference-only"):
        pkg.bert.Drop.of(enc, packed)
    assert pkg.bert.Drop.of(enc.eval(), packed).off
