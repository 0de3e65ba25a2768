"""CPU: tests/dropout_ref.py -- the numpy restatement of the seeded dropout law that tests/test_dropout_forms_gpu.py holds
the kernels to -- tied to something outside this project and to the properties dropout needs.

* Known answers: with seed s and epoch 0, group 0 hashes (s + 1) G, so seeds 0..3 give the first four outputs of
  SplitMix64 from state 0 as published with the generator (Steele, Lea, Flood 2014; the test vector of every port).
* Threshold and scale at the probabilities the project uses and at the ends of the range.
* Independence of the decision fields that must not share decisions -- heads, items, adjacent query rows, neighbouring
  seeds, neighbouring epoch words, the four fields of a group.  Two independent Bernoulli(1 - p') fields agree with
  probability a = (1 - p')^2 + p'^2; over N compared decisions the agreement must lie within 5 sqrt(a (1 - a) / N) of a.
  These are statements about FIXED seeds (chosen below, checked before they were committed): nothing here is random.
* The comparison can fail: a law without the head in its row term fails the head assertion, one with the fields in
  reverse order fails the known answer.
"""
import math

import numpy as np
import pytest

import dropout_ref as D
import keyed_dropout_ref as KD

SPLITMIX64_FROM_0 = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC)
SHAPE = (2, 3, 40, 70)          # B, nh, Lq, Lk: Lk % 4 = 2, so every row's last group is cut
SEED = 20240607


# ------------------------------------------------------------------------------------------------ known answers
def test_group_zero_of_seeds_0_to_3_is_the_published_splitmix64_sequence():
    assert int(D.GOLD) == 0x9E3779B97F4A7C15
    for s, want in enumerate(SPLITMIX64_FROM_0):
        assert int(D.seed_term(s, 0)) == ((s + 1) * 0x9E3779B97F4A7C15) % 2 ** 64
        assert int(D.finalise(D.seed_term(s, 0))) == want, (s, hex(int(D.finalise(D.seed_term(s, 0)))))
    # the group index is ADDED to the seed term, not multiplied in: group i of seed 0 hashes G + i
    z = np.arange(4, dtype=np.uint64) + D.seed_term(0, 0)
    assert [int(v) for v in z] == [0x9E3779B97F4A7C15 + i for i in range(4)]
    assert int(D.finalise(z)[0]) == SPLITMIX64_FROM_0[0] and int(D.finalise(z)[1]) != SPLITMIX64_FROM_0[1]


def test_fields_are_taken_from_the_low_bits_upwards():
    f = D.group(D.seed_term(0, 0))
    assert f.shape == (4,) and f.tolist() == [0xCDAF, 0x7B1D, 0xA839, 0xE220]
    # and the decisions follow them element by element: thr = 0x8000 keeps exactly the fields >= 0x8000
    assert D.elementwise_keep(4, 0.5, 0, 0).tolist() == [True, False, True, True]
    assert D.elementwise_mult(3, 0.5, 0, 0).tolist() == [2.0, 0.0, 2.0]


def test_the_epoch_word_enters_the_seed_before_the_multiplication():
    e, s = 2 ** 40 + 3, 12345
    want = (((s + e * 0xD1342543DE82EF95) % 2 ** 64) * 0x9E3779B97F4A7C15 + 0x9E3779B97F4A7C15) % 2 ** 64
    assert int(D.seed_term(s, e)) == want
    assert int(D.seed_term(s, 0)) == int(D.seed_term(s))                         # no word registered = word 0
    assert int(D.seed_term(s, 1)) == int(D.seed_term((s + 0xD1342543DE82EF95) % 2 ** 64, 0))
    assert np.array_equal(D.elementwise_keep(64, 0.1, s, 1), D.elementwise_keep(64, 0.1, (s + 0xD1342543DE82EF95) % 2 ** 64, 0))


# ------------------------------------------------------------------------------------------------ threshold and scale
def test_threshold_and_scale():
    assert D.threshold is KD.threshold and D.scale is KD.scale
    assert D.threshold(0.1) == 6554 and D.threshold(0.5) == 32768 and D.threshold(0.0) == 0
    assert D.scale(0.0) == np.float32(1.0) and D.scale(0.5) == np.float32(2.0)
    assert D.scale(0.1) == np.float32(65536.0) / np.float32(65536 - 6554)
    assert D.threshold(np.nextafter(np.float32(1), np.float32(0))) == 65535 and D.threshold(0.99999) == 65535
    assert D.scale(0.99999) == np.float32(65536.0)
    assert D.elementwise_keep(4096, 0.0, 7).all() and (D.elementwise_mult(4096, 0.0, 7) == 1).all()


# ------------------------------------------------------------------------------------------------ index laws
def test_the_hidden_law_is_the_elementwise_law_on_the_flat_tensor():
    for M, H in ((1, 256), (5, 768), (33, 1024), (70, 768)):
        for epoch in (0, 2 ** 40 + 3):
            assert np.array_equal(D.hidden_mult(M, H, 0.1, SEED, epoch).reshape(-1), D.elementwise_mult(M * H, 0.1, SEED, epoch))


def test_the_attention_law_starts_a_group_at_every_query_row():
    B, nh, Lq, Lk = SHAPE
    groups = (Lk + 3) >> 2
    assert groups == 18
    keep = D.attn_keep(B, nh, Lq, Lk, 0.1, SEED, 5)
    assert keep.shape == SHAPE
    flat = D.elementwise_keep(B * nh * Lq * groups * 4, 0.1, SEED, 5).reshape(B, nh, Lq, groups * 4)
    assert np.array_equal(keep, flat[..., :Lk])             # rows of 4 * groups flat elements, the last two unused
    # Lk a multiple of 4: the flat law itself
    assert np.array_equal(D.attn_keep(2, 2, 5, 8, 0.5, 3).reshape(-1), D.elementwise_keep(2 * 2 * 5 * 8, 0.5, 3))
    assert D.attn_mult(1, 1, 1, 1, 0.5, 0).tolist() == [[[[2.0]]]]


# ------------------------------------------------------------------------------------------------ independence
def agreement(x, y, p):
    """(observed agreement of two decision fields, a, 5 sigma)."""
    x, y = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
    assert x.shape == y.shape
    pp = D.threshold(p) / 65536.0
    a = (1 - pp) ** 2 + pp ** 2
    return float((x == y).mean()), a, 5 * math.sqrt(a * (1 - a) / x.size)


def assert_independent(x, y, p, what):
    got, a, bound = agreement(x, y, p)
    print(f"{what}: agreement {got:.4f} against {a:.4f} (5 sigma = {bound:.4f}, N = {np.asarray(x).size})")
    assert abs(got - a) < bound, (what, got, a, bound)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_heads_items_and_adjacent_query_rows_share_no_decisions(p):
    B, nh, Lq, Lk = SHAPE
    keep = D.attn_keep(B, nh, Lq, Lk, p, SEED, 0)
    for b in range(B):
        for h0 in range(nh):
            for h1 in range(h0 + 1, nh):
                assert_independent(keep[b, h0], keep[b, h1], p, f"p={p} item {b} heads {h0} / {h1}")
    assert_independent(keep[0], keep[1], p, f"p={p} items 0 / 1")
    assert_independent(keep[:, :, :-1], keep[:, :, 1:], p, f"p={p} query rows q / q + 1")
    rate, pp = 1.0 - keep.mean(), D.threshold(p) / 65536.0
    assert abs(rate - pp) < 5 * math.sqrt(pp * (1 - pp) / keep.size), (rate, pp)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_neighbouring_seeds_and_epoch_words_share_no_decisions(p):
    n = 200003
    base = D.elementwise_keep(n, p, SEED, 7)
    assert_independent(base, D.elementwise_keep(n, p, SEED + 1, 7), p, f"p={p} seeds s / s + 1")
    assert_independent(base, D.elementwise_keep(n, p, SEED, 8), p, f"p={p} epoch words e / e + 1")
    assert_independent(D.elementwise_keep(n, p, SEED, 0), D.elementwise_keep(n, p, SEED, 1), p, f"p={p} epoch words 0 / 1")
    B, nh, Lq, Lk = SHAPE
    assert_independent(D.attn_keep(B, nh, Lq, Lk, p, SEED, 0), D.attn_keep(B, nh, Lq, Lk, p, SEED + 1, 0), p, f"p={p} attention seeds")
    assert_independent(D.attn_keep(B, nh, Lq, Lk, p, SEED, 0), D.attn_keep(B, nh, Lq, Lk, p, SEED, 1), p, f"p={p} attention epochs")


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_the_four_fields_of_a_group_share_no_decisions(p):
    groups = 100000
    keep = D.elementwise_keep(4 * groups, p, SEED, 0).reshape(groups, 4)
    pp = D.threshold(p) / 65536.0
    for i in range(4):
        rate = 1.0 - keep[:, i].mean()
        print(f"p={p} field {i}: drop rate {rate:.4f} against {pp:.4f}")
        assert abs(rate - pp) < 5 * math.sqrt(pp * (1 - pp) / groups), (i, rate, pp)
        for j in range(i + 1, 4):
            assert_independent(keep[:, i], keep[:, j], p, f"p={p} fields {i} / {j}")


# ------------------------------------------------------------------------------------------------ the comparison can fail
def test_a_law_without_the_head_fails_the_head_assertion():
    B, nh, Lq, Lk = SHAPE
    groups = (Lk + 3) >> 2

    def attn_keep_without_head(p, seed, epoch):
        b = np.arange(B, dtype=np.uint64).reshape(B, 1, 1, 1)
        h = np.zeros((1, nh, 1, 1), dtype=np.uint64)                       # <- the head forgotten
        q = np.arange(Lq, dtype=np.uint64).reshape(1, 1, Lq, 1)
        idx = ((b * np.uint64(nh) + h) * np.uint64(Lq) + q) * np.uint64(groups) + np.arange(groups, dtype=np.uint64).reshape(1, 1, 1, groups)
        with np.errstate(over="ignore"):
            f = D.group(idx + D.seed_term(seed, epoch))
        return (f >= D.threshold(p)).reshape(B, nh, Lq, -1)[..., :Lk]

    wrong = attn_keep_without_head(0.1, SEED, 0)
    assert not np.array_equal(wrong, D.attn_keep(B, nh, Lq, Lk, 0.1, SEED, 0))
    got, a, bound = agreement(wrong[0, 0], wrong[0, 1], 0.1)
    assert got == 1.0 and not abs(got - a) < bound
    with pytest.raises(AssertionError):
        assert_independent(wrong[0, 0], wrong[0, 1], 0.1, "heads 0 / 1 of the law without the head")


def test_a_law_with_the_fields_reversed_fails_the_known_answer():
    def group_reversed(z):
        return D.group(z)[..., ::-1]

    assert group_reversed(D.seed_term(0, 0)).tolist() != [0xCDAF, 0x7B1D, 0xA839, 0xE220]
    keep = (group_reversed(D.seed_term(0, 0)) >= D.threshold(0.5)).tolist()
    assert keep != D.elementwise_keep(4, 0.5, 0, 0).tolist()
