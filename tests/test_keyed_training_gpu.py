"""GPU: keyed training and validation draws ("Keyed sampling streams": streams 4-7, the epoch in the step
field).  The three kernels against the numpy restatement (tests/keyed_ref.py) and against the buffer-fed kernels they
share their arithmetic with; the property the keys exist for -- what an item is noised with depends on (seed, item id,
epoch, position) and on nothing else: not the batch, the row, the frame, eager / graph launches; the two models'
seeded steps; a seeded ``fit`` whose validation loss is a function of the weights; and the unseeded path, which draws
from torch's generator exactly as before."""
import numpy as np
import pytest
import torch

import keyed_ref as K
from helpers import synthetic_pockets

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDS = [0, 1, 5, 123456789, (1 << 32) + 9, (1 << 63) + 17, (1 << 64) - 1, 77]      # one >= 2^63, one above 2^32
VALIDATION = 65535


def _word(epoch):
    from e3diff_amd import keyed
    return keyed.set_epoch(keyed.epoch_word(DEV), None if epoch == VALIDATION else epoch)


def _ids(ids):
    from e3diff_amd import keyed
    return keyed.device_item_ids(ids, len(ids), DEV)


def _keys(ids, L):
    """The [B * L, 2] key table of a padded frame, for the restatement."""
    from e3diff_amd import keyed
    return keyed.padded_keys(keyed.item_ids(ids, len(ids)), L, "cpu").numpy()


def _wrap(x):
    from e3diff_amd.structure_model.utils import modulo_with_wrapped_range
    return modulo_with_wrapped_range(x)


def _sequence_inputs(B, L, t_int, seed=0):
    """int32 class indices [B, L] with a padding tail (-1) per row and the Qt_bar of the items' timesteps [B, 20, 20]."""
    from e3diff_amd.sequence_model.utils import BlosumTransition, PredefinedNoiseScheduleDiscrete
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, 20, (B, L), generator=g, dtype=torch.int32)
    lengths = torch.randint(5, 31, (B,), generator=g)
    idx[torch.arange(L)[None] >= lengths[:, None]] = -1
    sched = PredefinedNoiseScheduleDiscrete("cosine", 50).to(DEV)
    ab = sched.get_alpha_bar(t_normalized=t_int.reshape(B, 1).float().to(DEV) / 50)
    return idx.to(DEV), BlosumTransition(x_classes=20).get_Qt_bar(ab, device=DEV).contiguous()


# ------------------------------------------------------------------------------------- kernels against the restatement
@pytest.mark.parametrize("epoch", [0, 1, VALIDATION])
def test_timesteps_equal_the_restatement(pkg, hip, epoch):
    from e3diff_amd import keyed
    ops = pkg.ops
    for stream, C in ((keyed.TRAIN_STRUCT_T, 1000), (keyed.TRAIN_SEQ_T, 51)):
        for seed in (7, 0xDEADBEEFCAFEF00D):
            got = ops.keyed_timesteps(_ids(IDS), _word(epoch), seed, stream, C)
            assert got.dtype == torch.int64 and got.shape == (len(IDS),)
            want = K.classes(_keys(IDS, 1), seed, stream, epoch, C)
            assert np.array_equal(got.cpu().numpy(), want), (stream, seed, got.tolist(), want.tolist())
    with pytest.raises(ValueError, match="timestep stream"):
        ops.keyed_timesteps(_ids(IDS), _word(0), 7, keyed.TRAIN_SEQ_U, 51)


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("epoch", [0, 1, VALIDATION])
def test_structure_noise_matches_the_restatement_and_x_t_the_buffer_kernel(pkg, hip, scale, epoch):
    """known_noise = wrap(scale * z) within 2e-6 on the circle of the fp64 restatement (the tolerance of the sampler
    streams' fp32 normals and of test_q_sample_wrap); x_t BIT-identical to e3d_q_sample_wrap fed with that noise: the two
    kernels share the device function of the update (the compiler emits the same multiply / multiply / add / add for
    both instantiations)."""
    from e3diff_amd import keyed
    from e3diff_amd.structure_model.utils import CosineTables
    ops = pkg.ops
    B, L, F, seed = len(IDS), 128, 8, 7
    tab = CosineTables(1000)
    sa, s1 = tab.sqrt_alphas_cumprod.to(DEV), tab.sqrt_one_minus_alphas_cumprod.to(DEV)
    g = torch.Generator().manual_seed(2)
    x0 = (torch.rand(B, L, F, generator=g) * 6.28 - 3.14).to(DEV)
    t = torch.tensor([0, 1, 17, 250, 500, 875, 998, 999], device=DEV)
    noise, x_t = ops.keyed_q_sample_wrap(x0, t, sa, s1, scale, _ids(IDS), _word(epoch), seed)
    want = _wrap(torch.from_numpy(scale * K.normals(_keys(IDS, L), seed, keyed.TRAIN_STRUCT_NOISE, epoch, F))).reshape(B, L, F)
    d = _wrap(noise.cpu().double() - want).abs().max().item()
    print(f"scale {scale} epoch {epoch}: max wrapped |known_noise - restatement| = {d:.3e} (2e-6)")
    assert d <= 2e-6, d
    assert noise.abs().max() <= 3.1416 and noise.std() > 0.4 * scale
    assert torch.equal(x_t, ops.q_sample_wrap(x0, noise, t, sa, s1))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.keyed_q_sample_wrap(x0[..., :6].contiguous(), t, sa, s1, scale, _ids(IDS), _word(epoch), seed)


@pytest.mark.parametrize("epoch", [0, 1, VALIDATION])
def test_sequence_noising_equals_the_buffer_kernel_fed_with_the_restated_uniforms(pkg, hip, epoch):
    """Same kernel arithmetic, bit-equal uniforms: every position's class equals e3d_discrete_q_sample's, none left out."""
    from e3diff_amd import keyed
    ops = pkg.ops
    B, L, seed = len(IDS), 128, 7
    t_int = torch.tensor([0, 1, 10, 25, 33, 49, 50, 50])
    idx, qtb = _sequence_inputs(B, L, t_int)
    got = ops.keyed_discrete_q_sample(idx, qtb, _ids(IDS), _word(epoch), seed)
    u = torch.from_numpy(K.uniforms(_keys(IDS, L), seed, keyed.TRAIN_SEQ_U, epoch)).reshape(B, L).to(DEV)
    want = ops.discrete_q_sample(idx, qtb, u)
    assert got.dtype == torch.int32 and torch.equal(got, want)
    assert (got[idx < 0] == 0).all() and (idx < 0).any()                          # padding rows: class 0
    assert (got != idx)[idx >= 0].any()                                           # and residues are noised


# ------------------------------------------------------------------------------------------------------- invariance
def _draw_all(ops, ids, x0, idx, epoch_word, seed=11):
    """Every training draw of a batch: both timesteps, structure noise and x_t, sequence classes."""
    from e3diff_amd import keyed
    from e3diff_amd.structure_model.utils import CosineTables
    from e3diff_amd.sequence_model.utils import BlosumTransition, PredefinedNoiseScheduleDiscrete
    tab = CosineTables(1000)
    d = _ids(ids)
    B = len(ids)
    t4 = ops.keyed_timesteps(d, epoch_word, seed, keyed.TRAIN_STRUCT_T, 1000)
    t6 = ops.keyed_timesteps(d, epoch_word, seed, keyed.TRAIN_SEQ_T, 51)
    noise, x_t = ops.keyed_q_sample_wrap(x0.contiguous(), t4, tab.sqrt_alphas_cumprod.to(DEV),
                                         tab.sqrt_one_minus_alphas_cumprod.to(DEV), 1.0, d, epoch_word, seed)
    sched = PredefinedNoiseScheduleDiscrete("cosine", 50).to(DEV)
    qtb = BlosumTransition(x_classes=20).get_Qt_bar(sched.get_alpha_bar(t_normalized=t6.reshape(B, 1).float() / 50),
                                                    device=DEV).contiguous()
    cls = ops.keyed_discrete_q_sample(idx.contiguous(), qtb, d, epoch_word, seed)
    return dict(t4=t4, t6=t6, noise=noise, x_t=x_t, cls=cls)


def _same_items(full, part, rows, Lp=None):
    """Items ``rows`` of ``full`` equal the items of ``part`` (its frame: the first ``Lp`` positions), bit for bit."""
    for k, v in part.items():
        want = full[k][rows]
        if v.dim() > 1 and Lp is not None:
            want = want[:, :Lp]
        assert torch.equal(v, want), k


def test_an_items_draws_do_not_depend_on_batch_row_or_frame(pkg, hip):
    from e3diff_amd import keyed
    ops = pkg.ops
    B, L = 8, 128
    g = torch.Generator().manual_seed(5)
    x0 = (torch.rand(B, L, 8, generator=g) * 6.28 - 3.14).to(DEV)
    idx, _ = _sequence_inputs(B, L, torch.zeros(B), seed=6)
    word = _word(3)
    full = _draw_all(ops, IDS, x0, idx, word)
    assert len(set(full["t4"].tolist())) > 1 and len(set(full["t6"].tolist())) > 1
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    _same_items(full, _draw_all(ops, [IDS[i] for i in perm], x0[perm], idx[perm], word), perm)
    for b in range(B):                                                               # any single item alone
        _same_items(full, _draw_all(ops, IDS[b:b + 1], x0[b:b + 1], idx[b:b + 1], word), [b])
    _same_items(full, _draw_all(ops, IDS[:3], x0[:3], idx[:3], word), [0, 1, 2])
    _same_items(full, _draw_all(ops, IDS, x0[:, :32], idx[:, :32], word), list(range(B)), Lp=32)   # the trimmed frame
    # the same epoch twice: identical; another epoch: other draws
    again = _draw_all(ops, IDS, x0, idx, _word(3))
    assert all(torch.equal(again[k], full[k]) for k in full)
    other = _draw_all(ops, IDS, x0, idx, _word(4))
    assert not torch.equal(other["t4"], full["t4"]) and not torch.equal(other["t6"], full["t6"])
    assert not torch.equal(other["noise"], full["noise"]) and not torch.equal(other["cls"], full["cls"])
    # validation: the same draws whatever the training epoch was before, and no training epoch's
    vals = []
    for before in (0, 9):
        keyed.set_epoch(word, before)
        _draw_all(ops, IDS, x0, idx, word)
        keyed.set_epoch(word, None)
        vals.append(_draw_all(ops, IDS, x0, idx, word))
    assert all(torch.equal(vals[0][k], vals[1][k]) for k in full)
    assert not torch.equal(vals[0]["noise"], full["noise"]) and not torch.equal(vals[0]["t4"], full["t4"])


def test_captured_kernels_replay_with_the_ids_and_epoch_in_device_memory(pkg, hip):
    """The three kernels in one graph: ids and epoch are read at replay time, so changing the static tensors in place
    gives the eager launches' results for the new values."""
    from e3diff_amd import keyed
    from e3diff_amd.structure_model.utils import CosineTables
    ops = pkg.ops
    B, L, seed = 8, 64, 21
    tab = CosineTables(1000)
    sa, s1 = tab.sqrt_alphas_cumprod.to(DEV), tab.sqrt_one_minus_alphas_cumprod.to(DEV)
    g = torch.Generator().manual_seed(8)
    x0 = (torch.rand(B, L, 8, generator=g) * 6.28 - 3.14).to(DEV)
    idx, qtb = _sequence_inputs(B, L, torch.full((B,), 40), seed=9)

    def launch(ids, word):
        t4 = ops.keyed_timesteps(ids, word, seed, keyed.TRAIN_STRUCT_T, 1000)
        t6 = ops.keyed_timesteps(ids, word, seed, keyed.TRAIN_SEQ_T, 51)
        noise, x_t = ops.keyed_q_sample_wrap(x0, t4, sa, s1, 1.0, ids, word, seed)
        return t4, t6, noise, x_t, ops.keyed_discrete_q_sample(idx, qtb, ids, word, seed)

    ids, word = _ids(IDS), _word(0)
    launch(ids, word)                                    # (code objects loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = launch(ids, word)
    seen = []
    for new_ids, epoch in ((IDS, 0), (IDS[::-1], 0), (IDS, 5), ([3, 1 << 40, 9, 27, 81, 243, 729, (1 << 63) + 1], VALIDATION)):
        ids.copy_(_ids(new_ids))
        keyed.set_epoch(word, None if epoch == VALIDATION else epoch)
        graph.replay()
        torch.cuda.synchronize()
        want = launch(_ids(new_ids), _word(epoch))
        assert all(torch.equal(a, b) for a, b in zip(outs, want)), (new_ids, epoch)
        seen.append(outs[2].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[0], seen[2]) and not torch.equal(seen[2], seen[3])


# ----------------------------------------------------------------------------------------------------------- models
MODEL_IDS = [101, 7, (1 << 40) + 3, 55, 900, 13, 4242, 31]


def _small_sequence_model(learning_rate=1e-4, seed=0):
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.sequence_model.model import PeptideDiff
    c = dict(hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=2, max_position_embeddings=64,
             hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    torch.manual_seed(seed)
    return PeptideDiff(BertConfig(**c), BertConfig(**c, is_decoder=True, add_cross_attention=True),
                       feature_names=list("ACDEFGHIKLMNPQRSTVWY"), loss_func=torch.nn.CrossEntropyLoss(), noise_schedule="cosine",
                       timesteps=50, l2_lambda=0.1, learning_rate=learning_rate).train().to(DEV)


def _pockets(seed, ids, with_ligand_seq, **kw):
    pk = {k: v.to(DEV) for k, v in synthetic_pockets(8, 64, seed=seed, with_ligand_seq=with_ligand_seq, **kw).items()
          if torch.is_tensor(v)}
    pk["item_id"] = _ids(ids)
    return pk


def _permuted(batch, perm):
    return {k: v[perm].contiguous() for k, v in batch.items()}


def test_seeded_sequence_step_is_the_same_on_a_permuted_and_on_a_trimmed_batch(pkg, hip):
    """``training_step`` itself on the padded batch, the same items permuted and the trimmed frame: with keyed draws the
    three see the same timesteps and noised residues, so loss and parameter gradients agree as
    test_trimmed_sequence_batch_has_the_padded_batchs_loss_and_gradients demands of one pre-noised input (2e-6 of the
    loss; 2e-4 of each gradient's largest element)."""
    from test_training_gpu import _assert_same_gradients, _grads_of
    from e3diff_amd import keyed, ops, training
    model = _small_sequence_model()
    batch = _pockets(5, MODEL_IDS, True, rec_range=(20, 30))
    small = training.trim_batch(batch)
    assert small["ligand_seq"].shape[1] == 32 and small["receptor_angles"].shape[1] == 32 and torch.equal(small["item_id"], batch["item_id"])
    word = model.use_keyed_draws(13)
    assert word.tolist() == [0]
    with ops.arithmetic("bf16x3"):
        la, ga = _grads_of(model, lambda: model.training_step(batch))
        assert la == la and abs(la) < 1e4, la                                        # the batch has noised positions
        lb, gb = _grads_of(model, lambda: model.training_step(_permuted(batch, [5, 2, 7, 0, 3, 6, 1, 4])))
        lc, gc = _grads_of(model, lambda: model.training_step(small))
        keyed.set_epoch(word, 1)
        ld, _ = _grads_of(model, lambda: model.training_step(batch))
    print(f"seeded sequence step: padded {la!r} permuted {lb!r} trimmed {lc!r}; next epoch {ld!r}")
    assert abs(la - lb) <= 2e-6 * abs(la), (la, lb)
    assert abs(la - lc) <= 2e-6 * abs(la), (la, lc)
    _assert_same_gradients(ga, gb, 2e-4)
    _assert_same_gradients(ga, gc, 2e-4)
    assert abs(la - ld) > 1e-4 * abs(la)                                             # another epoch: other draws
    with pytest.raises(ValueError, match="ItemIdDataset"):
        model.training_step({k: v for k, v in batch.items() if k != "item_id"})
    with pytest.raises(ValueError, match="not both"):
        model.apply_aa_noise(batch["ligand_seq"], torch.ones(8, 1, device=DEV), u=torch.rand(8, 64, device=DEV),
                             keyed_draw=(batch["item_id"], word, 13))
    model.use_keyed_draws(None)
    assert model.keyed_draws is None


def test_seeded_structure_noising_gives_the_same_step_on_a_permuted_and_on_a_trimmed_batch(pkg, hip):
    """``noise_batch_on_device(seed=)`` on each frame, then ``training_step``: the comparison of
    test_trimmed_structure_batch_has_the_padded_batchs_loss_and_gradients without handing both frames one pre-noised batch."""
    from test_training_gpu import _assert_same_gradients, _grads_of, _small_structure_model
    from e3diff_amd import ops, training
    from e3diff_amd.structure_model.dataset import noise_batch_on_device
    from e3diff_amd.structure_model.utils import CosineTables
    model, tab = _small_structure_model(), CosineTables(100)
    pk = _pockets(21, MODEL_IDS, False, rec_range=(20, 30))

    def noised(b, epoch=2):
        out = noise_batch_on_device(b["ligand_angles"], tab, seed=13, item_ids=b["item_id"], epoch=epoch)
        assert out["timestep"].shape == (8, 1) and out["timestep"].dtype == torch.int64
        return dict(b, **out)

    batch, small, perm = noised(pk), noised(training.trim_batch(pk)), [5, 2, 7, 0, 3, 6, 1, 4]
    assert small["noised_ligand_angle"].shape[1] == 32 and torch.equal(small["timestep"], batch["timestep"])
    assert torch.equal(small["known_noise"], batch["known_noise"][:, :32])
    assert len(set(batch["timestep"].flatten().tolist())) > 1
    with ops.arithmetic("bf16x3"):
        la, ga = _grads_of(model, lambda: model.training_step(batch))
        assert la == la and abs(la) < 1e4, la
        lb, gb = _grads_of(model, lambda: model.training_step(noised(_permuted(pk, perm))))
        lc, gc = _grads_of(model, lambda: model.training_step(small))
    print(f"seeded structure step: padded {la!r} permuted {lb!r} trimmed {lc!r}")
    assert abs(la - lb) <= 2e-6 * abs(la), (la, lb)
    assert abs(la - lc) <= 2e-6 * abs(la), (la, lc)
    _assert_same_gradients(ga, gb, 2e-4)
    _assert_same_gradients(ga, gc, 2e-4)
    assert not torch.equal(noised(pk, epoch=3)["known_noise"], batch["known_noise"])


@pytest.mark.parametrize("which", ["sequence", "structure"])
def test_seeded_graphed_step_matches_the_seeded_eager_loop(pkg, hip, which):
    """2 epochs x 3 batches through training.GraphedStep (two eager steps, capture, replays: the epoch word changes between
    replays of ONE graph; the sequence model's draws are kernels inside it) against eager steps on a twin model: per-step
    losses within the 2e-5 DESIGN.md section 4 states for graph vs eager training."""
    from test_training_gpu import _small_structure_model
    from e3diff_amd import autograd, keyed, ops, training
    from e3diff_amd.structure_model.dataset import noise_batch_on_device
    from e3diff_amd.structure_model.utils import CosineTables
    tab = CosineTables(100)
    batches = [_pockets(30 + i, [1000 * i + 17 * j + 3 for j in range(8)], which == "sequence") for i in range(3)]
    results = []
    for graphed in (False, True):
        word = keyed.epoch_word(DEV)
        if which == "sequence":
            model = _small_sequence_model()
            model.use_keyed_draws(29, word)
        else:
            model = _small_structure_model()
        optim = model.configure_optimizers()["optimizer"]
        params = [p for p in model.parameters() if p.requires_grad]
        stepper = training.GraphedStep(model, optim, params, 1.0) if graphed else None
        losses = []
        with ops.arithmetic("bf16x3"):
            for epoch in range(2):
                keyed.set_epoch(word, epoch)
                for batch in batches:
                    if which == "structure":
                        batch = dict(batch, **noise_batch_on_device(batch["ligand_angles"], tab, seed=29,
                                                                    item_ids=batch["item_id"], epoch=word))
                    if graphed:
                        losses.append(float(stepper.step(batch)))
                    else:
                        loss = model.training_step(batch)
                        optim.zero_grad(set_to_none=True)
                        with autograd.deferred_weight_grads():
                            loss.backward()
                        training.clip_and_step(params, optim, 1.0)
                        losses.append(float(loss))
        if graphed:
            assert stepper.graph is not None and stepper.failed is None and len(stepper.graphs) == 1
        results.append(losses)
    la, lb = results
    print(f"{which}: eager {la} graphed {lb}")
    assert all(l == l and abs(l) < 1e4 for l in la)
    assert all(abs(a - b) <= 2e-5 * abs(a) for a, b in zip(la, lb)), (la, lb)
    assert all(abs(la[i] - la[i + 3]) > 1e-4 * abs(la[i]) for i in range(3))        # the second epoch drew again


# -------------------------------------------------------------------------------------------------------------- fit
def _fit_setup(which, monkeypatch, tmp_path, seed):
    from test_training_gpu import SMALL, _records
    if which == "sequence":
        from e3diff_amd.sequence_model import train_model as T
        model_kw = dict(feature_names=list("ACDEFGHIKLMNPQRSTVWY"), loss_func=torch.nn.CrossEntropyLoss(),
                        noise_schedule="cosine", timesteps=50, l2_lambda=0.1, learning_rate=0.0)
        from e3diff_amd.sequence_model.model import PeptideDiff as M
    else:
        from e3diff_amd.structure_model import train_model as T
        from e3diff_amd.structure_model.model import ConditionalBertForDiffusion as M
        model_kw = dict(feature_names=list("abcdefgh"), loss_func=[M.diheral_loss_func] * 4 + [M.angle_loss_func] * 4,
                        l2_lambda=0.1, learning_rate=0.0)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(T, "NUM_THREAD", 0)
    monkeypatch.setattr(T, "CONFIG", dict(T.CONFIG, **SMALL, timesteps=50 if which == "sequence" else 100))
    train_dl, val_dl = T.get_dataloader(None, records=_records(), seed=seed)
    enc, dec = T.build_configs()
    torch.manual_seed(0)
    model = M(enc, dec, **model_kw)
    if which == "structure":
        with torch.no_grad():       # adaLN_modulation[0] is zero-initialised: give the timestep a say in the output
            for se in (model.receptor_emb, model.timestep_emb):
                torch.nn.init.normal_(se.adaLN_modulation[0].weight, std=0.02)
    return model, train_dl, val_dl


@pytest.mark.parametrize("which", ["sequence", "structure"])
def test_validation_loss_of_a_seeded_fit_is_a_function_of_the_weights(pkg, hip, monkeypatch, tmp_path, which):
    """Learning rate 0, no schedule, dropout 0: the weights never move.  Seeded, the validation loss of epoch 0 IS that of
    epoch 1; unseeded it is another draw every epoch (the ``!=`` shows that the ``==`` can fail).  The loaders are the
    entry points' own: with a seed their items carry ``item_id`` (and the structure items skip the CPU noising)."""
    from e3diff_amd import training
    results = {}
    for seed in (41, None):
        model, train_dl, val_dl = _fit_setup(which, monkeypatch, tmp_path, seed)
        first = next(iter(val_dl))
        assert ("item_id" in first) == (seed is not None)
        if seed is not None and which == "structure":
            assert not first["known_noise"].any() and not first["noised_ligand_angle"].any()
        before = [p.detach().clone() for p in model.parameters()]
        torch.manual_seed(1)
        h = training.fit(model, train_dl, val_dl, max_epochs=2, device=DEV, checkpoint_path=None, log=lambda *a: None, seed=seed)
        assert all(torch.equal(a.to(DEV), b) for a, b in zip(before, model.parameters()))
        assert h["steps"] == 2 * len(train_dl) and len(h["val_loss"]) == 2
        assert all(v == v and abs(v) < 1e4 for v in h["val_loss"] + h["train_loss"]), h
        results[seed] = h
        print(f"{which} seed={seed}: val_loss {h['val_loss']} train_loss {h['train_loss']}")
    assert results[41]["val_loss"][0] == results[41]["val_loss"][1]
    assert results[None]["val_loss"][0] != results[None]["val_loss"][1]
    assert results[41]["train_loss"][0] != results[41]["train_loss"][1]              # training epochs draw again
    if which == "sequence":
        assert model.keyed_draws is None                                             # fit switched the keyed draws off again


def test_seeded_fit_refuses_a_batch_without_item_ids(pkg, hip, monkeypatch, tmp_path):
    from e3diff_amd import training
    model, train_dl, val_dl = _fit_setup("sequence", monkeypatch, tmp_path, None)
    with pytest.raises(ValueError, match="ItemIdDataset"):
        training.fit(model, train_dl, val_dl, max_epochs=1, device=DEV, checkpoint_path=None, log=lambda *a: None, seed=3)
    assert model.keyed_draws is None


# ----------------------------------------------------------------------------------------------------- default path
def test_unseeded_sequence_step_consumes_torchs_generator_as_before(pkg, hip):
    """seed=None: ``training_step`` makes the two generator calls it always made, in the same order -- restated here after
    the same ``manual_seed`` and fed to the injected-uniform path -- and returns the identical loss."""
    from e3diff_amd import ops
    model = _small_sequence_model()
    batch = {k: v for k, v in _pockets(5, MODEL_IDS, True).items() if k != "item_id"}
    B, L, T = 8, 64, model.timesteps
    with ops.arithmetic("bf16x3"):
        for s in (0, 123):
            torch.manual_seed(s)
            t_int = torch.randint(0, T + 1, (B, 1), device=DEV).float()
            u = torch.rand(B, L, device=DEV)
            want = model.get_loss(batch, t_int / T, model.apply_aa_noise(batch["ligand_seq"], t_int, u=u))[0]
            torch.manual_seed(s)
            got = model.training_step(batch)
            assert want == want and torch.equal(got, want), (s, float(got), float(want))
            # ... and a batch that carries ids draws the same without a seed
            torch.manual_seed(s)
            assert torch.equal(model.training_step(dict(batch, item_id=_ids(MODEL_IDS))), want)
