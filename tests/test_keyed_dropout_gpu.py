"""GPU: keyed dropout ("Keyed sampling streams": streams 8 / 9).  With a seed every dropout decision of a
training step is a function of (seed, item id, epoch, dropout site, position, head, column or key):
  * the row keys and the multipliers of both kinds of site equal the numpy restatement (tests/keyed_dropout_ref.py) bit for
    bit;
  * fed with the exported multipliers, the kernels equal the plain fp64 statements of test_dropout_gpu.py, forward and
    backward, to that file's bounds;
  * an item's multipliers do not depend on its batch, row or frame;
  * so a seeded ``training_step`` at dropout 0.1 gives the same loss and gradients on the padded batch, on the same items
    permuted and on the trimmed frame, a replayed step equals the eager one, an epoch can be resumed, and a seeded ``fit`` is
    repeatable;
  * without a seed every site draws from torch's generator exactly as before."""
import copy

import numpy as np
import pytest
import torch

import keyed_dropout_ref as R
from helpers import rel_err
from test_dropout_gpu import leaf, ref_attention_dropout
from test_keyed_training_gpu import IDS, MODEL_IDS, _ids, _permuted, _pockets, _word

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 0.1
SCALE = 65536.0 / (65536 - 6554)


def g(seed):
    return torch.Generator().manual_seed(seed)


def _u64(t):
    """An int64 tensor holding uint64 bits -> numpy uint64."""
    return t.cpu().numpy().view(np.uint64)


def _keys(ids, L, stream, epoch, seed):
    from e3diff_amd import ops
    return ops.keyed_drop_row_keys(_ids(ids), L, _word(epoch), seed, stream)


def _hidden_mult(ops, keys, H, site, p=P):
    return ops.dropout(torch.ones(keys.numel(), H, device=DEV), p, site, row_keys=keys)


# ------------------------------------------------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("epoch", [0, 1, 65535])
def test_row_keys_and_multipliers_equal_the_restatement_bit_for_bit(pkg, hip, epoch):
    """(65535 is the validation value of the epoch word: no training step runs there, but the field holds it.)"""
    ops = pkg.ops
    B = len(IDS)
    for seed in (7, 0xDEADBEEFCAFEF00D):
        for stream in (R.LIGAND, R.POCKET):
            for L in (16, 128):
                got = _keys(IDS, L, stream, epoch, seed)
                assert got.dtype == torch.int64 and got.shape == (B * L,)
                w = R.K.words(seed, np.array(IDS, dtype=np.uint64)[:, None], stream, epoch, np.arange(L)[None], 0)
                want = (w[..., 0].astype(np.uint64) | (w[..., 1].astype(np.uint64) << np.uint64(32))).reshape(-1)
                assert np.array_equal(_u64(got), want), (seed, stream, L)
        keys = _keys(IDS, 32, R.LIGAND, epoch, seed)
        kn = _u64(keys)
        for H, site in ((256, 0), (768, 3), (3072, (1 << 24) - 1)):
            got = _hidden_mult(ops, keys, H, site)
            assert np.array_equal(got.cpu().numpy(), R.hidden_mult(kn, H, P, site)), (seed, H, site)
        for (Lq, Lk), nh, site in (((16, 16), 2, 0), ((50, 64), 3, 11), ((128, 128), 2, 5), ((32, 128), 12, (1 << 24) - 1)):
            kq = _keys(IDS, Lq, R.LIGAND, epoch, seed)
            got = ops.keyed_attn_dropout_mask(B, nh, Lq, Lk, P, site, kq)
            assert np.array_equal(got.cpu().numpy(), R.attn_mult(_u64(kq), B, nh, Lq, Lk, P, site)), (seed, Lq, Lk)
    with pytest.raises(ValueError, match="row keys"):
        ops.dropout(torch.ones(4, 256, device=DEV), P, 0, row_keys=keys)


# ----------------------------------------------------------------------- 2. kernels, fed with the exported multipliers
@pytest.mark.parametrize("M,H", [(70, 768), (4096, 768), (33, 256)])
def test_keyed_residual_layernorm_pair_against_fp64_and_the_unfused_kernels(pkg, hip, M, H):
    """LayerNorm(dropout(x) + r), keyed: forward and every gradient against the fp64 statement fed with the exported
    multipliers (2e-5: fp32 LayerNorm arithmetic, the bound test_dropout_gpu.py gives its fp32-grade paths), and
    dx = ds * multipliers exactly.  Against the keyed dropout launch followed by the plain kernels the decisions are the
    same ones and the values agree to 2e-6 of the largest element: the keyed kernels are instantiations of their own, and
    the compiler is free to fuse other multiply-add pairs of the same fp32 formula in them than in the plain ones (a few
    ulp, 2^-23 = 1.2e-7 each, on values up to ~10x the typical one) -- the unkeyed pair, whose code is the one it always
    was, stays bit-identical (test_dropout_folded_into_the_residual_layernorm_kernels)."""
    from e3diff_amd import autograd as AG, ops
    from e3diff_amd.autograd import functional as F
    gen = g(5)
    x, r = torch.randn(M, H, generator=gen), torch.randn(M, H, generator=gen)
    ga, be = 1 + 0.1 * torch.randn(H, generator=gen), torch.randn(H, generator=gen)
    dy = torch.randn(M, H, generator=gen)
    ids = [1000 + i for i in range((M + 15) // 16)]
    with ops.keyed_dropout(9, _word(2), _ids(ids)) as kd:
        keys = kd.row_keys(R.POCKET, 16)[:M].contiguous()
        ops.next_dropout_seed()                                        # (the site under test is not the first of its step)
        site = kd.site
        xd, rd, gd, bd = leaf(x, DEV), leaf(r, DEV), leaf(ga, DEV), leaf(be, DEV)
        out = F.residual_layernorm(xd, rd, gd, bd, 1e-12, P, row_keys=keys)
        assert kd.site == site + 1
    out.backward(dy.to(DEV))
    mult = _hidden_mult(ops, keys, H, site)
    assert abs((mult == 0).float().mean().item() - 0.1) < 0.02
    xr, rr, gr, br = (leaf(t, dtype=torch.double) for t in (x, r, ga, be))
    ref = torch.nn.functional.layer_norm(xr * mult.cpu().double() + rr, (H,), gr, br, 1e-12)
    ref.backward(dy.double())
    for name, a, b in (("out", out, ref), ("dx", xd.grad, xr.grad), ("dr", rd.grad, rr.grad), ("dgamma", gd.grad, gr.grad),
                       ("dbeta", bd.grad, br.grad)):
        e = rel_err(a, b.float())
        print(f"M={M} H={H} {name}: {e:.3e} (2e-5)")
        assert e < 2e-5, (name, e)
    assert torch.equal(xd.grad, rd.grad * mult)                                      # the forward's decisions
    # the folded form against the separate launches
    drop = (P, site, keys)
    xg, rg, gg, bg = x.to(DEV), r.to(DEV), ga.to(DEV), be.to(DEV)
    out_f, s_f = ops.residual_layernorm(xg, rg, gg, bg, 1e-12, want_s=True, drop=drop)
    out_u, s_u = ops.residual_layernorm(ops.dropout(xg, P, site, row_keys=keys), rg, gg, bg, 1e-12, want_s=True)
    assert torch.equal(out_f, out.detach())
    ds_f, _, _, dsd = AG.layernorm_bwd(dy.to(DEV), s_f, gg, 1e-12, drop=drop)
    ds_u = AG.layernorm_bwd(dy.to(DEV), s_u, gg, 1e-12)[0]
    assert torch.equal(dsd, ds_f * mult)
    for name, a, b in (("out", out_f, out_u), ("s", s_f, s_u), ("ds", ds_f, ds_u)):
        e = rel_err(a, b)
        print(f"M={M} H={H} folded against separate launches, {name}: {e:.3e} (2e-6)")
        assert e <= 2e-6, (name, e)


ATTN_CASES = [  # B, nh, Lq, Lk, P (max_position_embeddings), kind
    (2, 2, 16, 16, 16, "relkey"), (2, 2, 50, 50, 64, "relkey"), (1, 3, 128, 128, 128, "relkey"), (1, 2, 256, 256, 256, "relkey"),
    (2, 2, 16, 16, 16, "self"), (2, 2, 50, 50, 64, "self"), (1, 3, 128, 128, 128, "self"), (1, 2, 256, 256, 256, "self"),
    (2, 2, 32, 128, 0, "cross"), (2, 2, 50, 64, 0, "cross"), (1, 2, 128, 256, 0, "cross"),
]


@pytest.mark.parametrize("B,nh,Lq,Lk,Pm,kind", ATTN_CASES)
def test_keyed_attention_dropout_forward_and_backward(pkg, hip, B, nh, Lq, Lk, Pm, kind):
    """Every mode of test_attention_probability_dropout_forward_and_backward at its tolerance, rel-key / plain self-attention
    and cross-attention (Lq != Lk); L <= 128 takes the fused backward in bf16x3, L = 256 the two-launch backward, bf16x6 and
    f32 the fp32 MFMA backward."""
    from e3diff_amd.autograd import functional as F
    ops = pkg.ops
    H = nh * 64
    cross = kind == "cross"
    q_src = torch.randn(B * Lq, H if cross else 3 * H, generator=g(Lq))
    kv_src = torch.randn(B * Lk, 2 * H, generator=g(Lk + 1)) if cross else None
    E = torch.randn(2 * Pm - 1, 64, generator=g(Pm)) if kind == "relkey" else None
    lens = torch.randint(1, Lk + 1, (B,), generator=g(3))
    lens[0] = Lk
    mask = (torch.arange(Lk)[None] < lens[:, None]).float()
    go = torch.randn(B * Lq, H, generator=g(9))
    sp = lambda x, L: x.reshape(B, L, nh, 64).permute(0, 2, 1, 3)  # noqa: E731
    ids = IDS[:B]
    for mode, tol in (("bf16x6", 2e-5), ("bf16x3", 1e-4), ("f32", 2e-5)):
        prev = ops.set_attn_mode(mode)
        try:
            with ops.keyed_dropout(21, _word(4), _ids(ids)) as kd:
                keys = kd.row_keys(R.LIGAND, Lq)
                for _ in range(3):
                    ops.next_dropout_seed()
                site = kd.site
                qd = leaf(q_src, DEV)
                kvd = leaf(kv_src, DEV) if cross else None
                Ed = leaf(E, DEV) if E is not None else None
                out = F.attention(qd, kvd, B, nh, Lq, Lk, key_mask=mask.to(DEV), dist_emb=Ed, max_pos=Pm, drop_p=P, row_keys=keys)
            out.backward(go.to(DEV))
        finally:
            ops.set_attn_mode(prev)
        mult = ops.keyed_attn_dropout_mask(B, nh, Lq, Lk, P, site, keys).cpu()
        assert torch.unique(mult).tolist() == [0.0, pytest.approx(SCALE)]
        assert abs((mult == 0).float().mean().item() - 0.1) < 0.02
        qr = leaf(q_src, dtype=torch.double)
        kvr = leaf(kv_src, dtype=torch.double) if cross else None
        Er = leaf(E, dtype=torch.double) if E is not None else None
        if cross:
            ref = ref_attention_dropout(sp(qr, Lq), sp(kvr[:, :H], Lk), sp(kvr[:, H:], Lk), mask.double(), None, Pm, mult.double())
        else:
            ref = ref_attention_dropout(sp(qr[:, :H], Lq), sp(qr[:, H:2 * H], Lk), sp(qr[:, 2 * H:], Lk), mask.double(), Er, Pm,
                                        mult.double())
        ref2d = ref.permute(0, 2, 1, 3).reshape(B * Lq, H)
        ref2d.backward(go.double())
        figures = [("out", out, ref2d)]
        if cross:
            figures += [("dq", qd.grad, qr.grad), ("dk", kvd.grad[:, :H], kvr.grad[:, :H]), ("dv", kvd.grad[:, H:], kvr.grad[:, H:])]
        else:
            figures += [(name, qd.grad[:, part], qr.grad[:, part])
                        for part, name in ((slice(0, H), "dq"), (slice(H, 2 * H), "dk"), (slice(2 * H, 3 * H), "dv"))]
        if E is not None:
            figures.append(("dE", Ed.grad, Er.grad))
        for name, a, b in figures:
            e = rel_err(a, b.float())
            print(f"{kind} {B}x{nh}x{Lq}x{Lk} {mode} {name}: {e:.3e} ({tol})")
            assert e < tol, (mode, name, e)


# --------------------------------------------------------------------------------------------- 3. invariance of decisions
def _all_multipliers(ops, ids, L, Lk, epoch=3, seed=11, site=4, stream=R.LIGAND, nh=4, H=256):
    keys = _keys(ids, L, stream, epoch, seed)
    B = len(ids)
    return dict(hidden=_hidden_mult(ops, keys, H, site).view(B, L, H),
                attn=ops.keyed_attn_dropout_mask(B, nh, L, Lk, P, site, keys))


def _same_items(full, part, rows, Lp=None, Lkp=None):
    h, a = full["hidden"][rows], full["attn"][rows]
    if Lp is not None:
        h, a = h[:, :Lp], a[:, :, :Lp, :Lkp]
    assert torch.equal(part["hidden"], h) and torch.equal(part["attn"], a)


def test_an_items_multipliers_do_not_depend_on_batch_row_or_frame(pkg, hip):
    ops = pkg.ops
    B, L = len(IDS), 128
    full = _all_multipliers(ops, IDS, L, L)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    _same_items(full, _all_multipliers(ops, [IDS[i] for i in perm], L, L), perm)
    for b in range(B):                                                               # any single item alone
        _same_items(full, _all_multipliers(ops, IDS[b:b + 1], L, L), [b])
    _same_items(full, _all_multipliers(ops, IDS[:3], L, L), [0, 1, 2])
    _same_items(full, _all_multipliers(ops, IDS, 32, 32), list(range(B)), Lp=32, Lkp=32)        # the 32-row frame
    _same_items(full, _all_multipliers(ops, IDS, 32, 64), list(range(B)), Lp=32, Lkp=64)        # ... against 64 keys
    again = _all_multipliers(ops, IDS, L, L)
    assert all(torch.equal(again[k], full[k]) for k in full)
    for other in (dict(epoch=4), dict(site=5), dict(seed=12), dict(stream=R.POCKET)):
        got = _all_multipliers(ops, IDS, L, L, **other)
        for k in full:
            assert not torch.equal(got[k], full[k]), (other, k)
            agree = ((got[k] != 0) == (full[k] != 0)).float().mean().item()           # two independent Bernoulli(0.9) fields
            assert abs(agree - 0.82) < 0.01, (other, k, agree)


# --------------------------------------------------------------------------------------------------- 4. the property
def _small_sequence_model(dropout, learning_rate=1e-4, seed=0):
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.sequence_model.model import PeptideDiff
    c = dict(hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=2, max_position_embeddings=64,
             hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout)
    torch.manual_seed(seed)
    return PeptideDiff(BertConfig(**c), BertConfig(**c, is_decoder=True, add_cross_attention=True),
                       feature_names=list("ACDEFGHIKLMNPQRSTVWY"), loss_func=torch.nn.CrossEntropyLoss(), noise_schedule="cosine",
                       timesteps=50, l2_lambda=0.1, learning_rate=learning_rate).train().to(DEV)


def _small_model(which, dropout):
    from test_training_gpu import _small_structure_model
    return _small_sequence_model(dropout) if which == "sequence" else _small_structure_model(dropout)


@pytest.mark.parametrize("which", ["sequence", "structure"])
def test_seeded_step_with_dropout_is_the_same_on_a_permuted_and_on_a_trimmed_batch(pkg, hip, which):
    """``training_step`` at hidden and attention dropout 0.1, seeded, on the padded batch, the same items permuted and
    the trimmed frame: identical per-item arithmetic -- every decision follows the item -- so loss and parameter gradients
    agree to the bounds of test_seeded_*_step_is_the_same_on_a_permuted_and_on_a_trimmed_batch at dropout 0 (2e-6 of the
    loss, 2e-4 of each gradient's largest element: only the order of the fp32 sums differs)."""
    from test_training_gpu import _assert_same_gradients, _grads_of
    from e3diff_amd import keyed, ops, training
    from e3diff_amd.structure_model.dataset import noise_batch_on_device
    from e3diff_amd.structure_model.utils import CosineTables
    model, plain = _small_model(which, 0.1), _small_model(which, 0.0)
    assert all(torch.equal(a, b) for a, b in zip(model.parameters(), plain.parameters()))
    pk = _pockets(5 if which == "sequence" else 21, MODEL_IDS, which == "sequence", rec_range=(20, 30))
    word = keyed.epoch_word(DEV)
    tab = CosineTables(100)

    def prepared(b):
        if which == "sequence":
            return b
        return dict(b, **noise_batch_on_device(b["ligand_angles"], tab, seed=13, item_ids=b["item_id"], epoch=2))

    for m in (model, plain):
        if which == "sequence":
            m.use_keyed_draws(13, word)
        assert m.use_keyed_dropout(13, word) is word
    batch, small, perm = prepared(pk), prepared(training.trim_batch(pk)), [5, 2, 7, 0, 3, 6, 1, 4]
    assert small["ligand_attn_mask"].shape[1] == 32 and small["receptor_angles"].shape[1] == 32
    state = torch.get_rng_state()
    with ops.arithmetic("bf16x3"):
        la, ga = _grads_of(model, lambda: model.training_step(batch))
        assert la == la and abs(la) < 1e4, la
        lb, gb = _grads_of(model, lambda: model.training_step(prepared(_permuted(pk, perm))))
        lc, gc = _grads_of(model, lambda: model.training_step(small))
        l0, _ = _grads_of(plain, lambda: plain.training_step(batch))
        keyed.set_epoch(word, 1)
        ld, _ = _grads_of(model, lambda: model.training_step(batch))
    assert torch.equal(torch.get_rng_state(), state)                                 # no site drew from torch's generator
    print(f"seeded {which} step at dropout 0.1: padded {la!r} permuted {lb!r} trimmed {lc!r}; dropout 0 {l0!r}; epoch 1 {ld!r}")
    print(f"  loss: permuted {abs(la - lb) / abs(la):.3e} trimmed {abs(la - lc) / abs(la):.3e} (2e-6)")
    assert abs(la - lb) <= 2e-6 * abs(la), (la, lb)
    assert abs(la - lc) <= 2e-6 * abs(la), (la, lc)
    _assert_same_gradients(ga, gb, 2e-4)
    _assert_same_gradients(ga, gc, 2e-4)
    assert abs(la - l0) > 1e-3 * abs(la), (la, l0)                                   # dropout acted
    assert ld != la                                                                  # another epoch: other decisions
    with pytest.raises(ValueError, match="ItemIdDataset"):
        model.training_step({k: v for k, v in batch.items() if k != "item_id"})
    model.use_keyed_dropout(None)
    assert model.keyed_dropout is None


# ------------------------------------------------------------------------------------- 5. launch mode and resumption
@pytest.mark.parametrize("which", ["sequence", "structure"])
def test_seeded_graphed_step_with_dropout_matches_the_eager_loop_and_an_epoch_resumes(pkg, hip, which):
    """2 epochs x 3 batches at dropout 0.1 through training.GraphedStep (two eager steps, capture, replays) against eager
    steps (``training.EagerStep``) on a twin model: per-step losses within the 2e-5 of
    test_seeded_graphed_step_matches_the_seeded_eager_loop -- eager and replayed steps take the same decisions.  Then epoch 1
    alone, on a fresh model and optimizer that took the weights and moments of the start of epoch 1 and never saw epoch 0:
    the same losses."""
    from e3diff_amd import keyed, ops, training
    from e3diff_amd.structure_model.dataset import noise_batch_on_device
    from e3diff_amd.structure_model.utils import CosineTables
    tab = CosineTables(100)
    batches = [_pockets(30 + i, [1000 * i + 17 * j + 3 for j in range(8)], which == "sequence") for i in range(3)]

    def setup():
        word = keyed.epoch_word(DEV)
        model = _small_model(which, 0.1)
        if which == "sequence":
            model.use_keyed_draws(29, word)
        model.use_keyed_dropout(29, word)
        optim = model.configure_optimizers()["optimizer"]
        return word, model, optim, [p for p in model.parameters() if p.requires_grad]

    def run_epoch(word, epoch, step):
        keyed.set_epoch(word, epoch)
        out = []
        for batch in batches:
            if which == "structure":
                batch = dict(batch, **noise_batch_on_device(batch["ligand_angles"], tab, seed=29, item_ids=batch["item_id"],
                                                            epoch=word))
            out.append(float(step(batch)))
        return out

    results, snapshot = [], None
    with ops.arithmetic("bf16x3"):
        for graphed in (False, True):
            word, model, optim, params = setup()
            if graphed:
                stepper = training.GraphedStep(model, optim, params, 1.0)
                step = stepper.step
            else:
                step = training.EagerStep(model, optim, params, 1.0).step
            losses = run_epoch(word, 0, step)
            if not graphed:
                snapshot = copy.deepcopy(model.state_dict()), copy.deepcopy(optim.state_dict())
            losses += run_epoch(word, 1, step)
            if graphed:
                assert stepper.graph is not None and stepper.failed is None and len(stepper.graphs) == 1
            results.append(losses)
        word, model, optim, params = setup()
        model.load_state_dict(snapshot[0])
        optim.load_state_dict(snapshot[1])
        resumed = run_epoch(word, 1, training.EagerStep(model, optim, params, 1.0).step)
    la, lb = results
    print(f"{which} at dropout 0.1: eager {la} graphed {lb} epoch 1 resumed {resumed}")
    assert all(l == l and abs(l) < 1e4 for l in la)
    worst = max(abs(a - b) / abs(a) for a, b in zip(la, lb))
    print(f"  graphed against eager: {worst:.3e} (2e-5); resumed: {max(abs(a - b) / abs(a) for a, b in zip(la[3:], resumed)):.3e}")
    assert all(abs(a - b) <= 2e-5 * abs(a) for a, b in zip(la, lb)), (la, lb)
    assert all(abs(a - b) <= 2e-5 * abs(a) for a, b in zip(la[3:], resumed)), (la[3:], resumed)
    assert all(abs(la[i] - la[i + 3]) > 1e-4 * abs(la[i]) for i in range(3))        # the second epoch decided again


# -------------------------------------------------------------------------------------------------------------- 6. fit
def _fit_setup(which, monkeypatch, tmp_path):
    """The entry points' own models at dropout 0.1 and learning rate 0, over their seeded loaders -- the training loader
    without shuffling, so that torch's generator decides nothing but (unkeyed) dropout."""
    from test_training_gpu import SMALL, _records
    if which == "sequence":
        from e3diff_amd.sequence_model import train_model as T
        from e3diff_amd.sequence_model.model import PeptideDiff as M
        model_kw = dict(feature_names=list("ACDEFGHIKLMNPQRSTVWY"), loss_func=torch.nn.CrossEntropyLoss(),
                        noise_schedule="cosine", timesteps=50, l2_lambda=0.1, learning_rate=0.0)
    else:
        from e3diff_amd.structure_model import train_model as T
        from e3diff_amd.structure_model.model import ConditionalBertForDiffusion as M
        model_kw = dict(feature_names=list("abcdefgh"), loss_func=[M.diheral_loss_func] * 4 + [M.angle_loss_func] * 4,
                        l2_lambda=0.1, learning_rate=0.0)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(T, "NUM_THREAD", 0)
    monkeypatch.setattr(T, "CONFIG", dict(T.CONFIG, **dict(SMALL, dropout_p=0.1), timesteps=50 if which == "sequence" else 100))
    train_dl, _ = T.get_dataloader(None, records=_records(), seed=41)
    train_dl = torch.utils.data.DataLoader(train_dl.dataset, batch_size=8, shuffle=False)
    enc, dec = T.build_configs()
    assert enc.hidden_dropout_prob == 0.1 and dec.attention_probs_dropout_prob == 0.1
    torch.manual_seed(0)
    model = M(enc, dec, **model_kw)
    if which == "structure":
        with torch.no_grad():
            for se in (model.receptor_emb, model.timestep_emb):
                torch.nn.init.normal_(se.adaLN_modulation[0].weight, std=0.02)
    return model, train_dl


@pytest.mark.parametrize("which", ["sequence", "structure"])
def test_a_seeded_fit_with_dropout_is_repeatable(pkg, hip, monkeypatch, tmp_path, which):
    """Learning rate 0: the weights never move.  Two seeded fits of two epochs from the same weights, with torch's generator
    in two different states, give identical ``train_loss`` lists; with ``keyed_dropout=False`` dropout draws from that
    generator and they do not (the ``!=`` shows that the ``==`` can fail)."""
    from e3diff_amd import training
    runs = {}
    for keyed_dropout in (None, False):
        for torch_seed in (1, 2):
            model, train_dl = _fit_setup(which, monkeypatch, tmp_path)
            torch.manual_seed(torch_seed)
            h = training.fit(model, train_dl, None, max_epochs=2, device=DEV, checkpoint_path=None, log=lambda *a: None, seed=41,
                             keyed_dropout=keyed_dropout)
            assert h["steps"] == 2 * len(train_dl) and len(h["train_loss"]) == 2
            assert all(v == v and abs(v) < 1e4 for v in h["train_loss"]), h
            assert model.keyed_dropout is None                                       # fit switched it off again
            runs[(keyed_dropout, torch_seed)] = h["train_loss"]
            print(f"{which} keyed_dropout={keyed_dropout} torch seed {torch_seed}: train_loss {h['train_loss']}")
    assert runs[(None, 1)] == runs[(None, 2)]
    assert runs[(False, 1)] != runs[(False, 2)]
    assert runs[(None, 1)][0] != runs[(None, 1)][1]                                  # epochs decide again


# ------------------------------------------------------------------------------------------------- 7. the unseeded path
def test_unseeded_sites_draw_from_torchs_generator_as_before(pkg, hip):
    """After ``torch.manual_seed(s)`` each functional site equals the ``ops`` call given the seed ``next_dropout_seed()``
    returns after the same ``manual_seed``, and leaves the generator where that one draw leaves it; inside the keyed
    context the generator does not move."""
    from e3diff_amd import ops
    from e3diff_amd.autograd import functional as F
    M, H, B, nh, L = 64, 256, 2, 4, 32
    gen = g(4)
    x, r = torch.randn(M, H, generator=gen).to(DEV), torch.randn(M, H, generator=gen).to(DEV)
    ga, be = torch.randn(H, generator=gen).to(DEV), torch.randn(H, generator=gen).to(DEV)
    qkv = torch.randn(B * L, 3 * H, generator=gen).to(DEV)
    mask = torch.ones(B, L, device=DEV)
    sites = [
        (lambda: F.dropout(x, P), lambda s: ops.dropout(x, P, s)),
        (lambda: F.residual_layernorm(x, r, ga, be, 1e-12, p_drop=P), lambda s: ops.residual_layernorm(x, r, ga, be, 1e-12, drop=(P, s))),
        (lambda: F.attention(qkv, None, B, nh, L, L, key_mask=mask, drop_p=P),
         lambda s: ops.attention(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], B, nh, L, L, key_mask=mask, drop=(P, s))),
    ]
    for s in (0, 123):
        for functional, direct in sites:
            torch.manual_seed(s)
            seed = ops.next_dropout_seed()
            after = torch.get_rng_state()
            torch.manual_seed(s)
            got = functional()
            assert torch.equal(torch.get_rng_state(), after)
            assert torch.equal(got, direct(seed))
    torch.manual_seed(5)
    state = torch.get_rng_state()
    with ops.keyed_dropout(3, _word(0), _ids(IDS[:B])) as kd:
        hk, ak = kd.row_keys(R.LIGAND, M // B), kd.row_keys(R.LIGAND, L)
        a = F.dropout(x, P, row_keys=hk)
        b = F.residual_layernorm(x, r, ga, be, 1e-12, p_drop=P, row_keys=hk)
        c = F.attention(qkv, None, B, nh, L, L, key_mask=mask, drop_p=P, row_keys=ak)
        assert kd.site == 3
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(a, ops.dropout(x, P, 0, row_keys=hk))
    assert torch.equal(b, ops.residual_layernorm(x, r, ga, be, 1e-12, drop=(P, 1, hk)))
    assert torch.equal(c, ops.attention(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], B, nh, L, L, key_mask=mask, drop=(P, 2, ak)))
