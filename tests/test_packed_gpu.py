"""GPU: packed variable-length batches -- the varlen attention kernel (ops.attention_varlen) against fp64 statements and
the padded-frame kernel; the packed structure decoder / reverse chain and the packed sequence forward / denoising chain
against the padded and trimmed frames."""
import warnings

import pytest
import torch

from helpers import FULL_STRUCT, rel_err, seeded_state_dict, synthetic_pockets
from oracle import bert as obert, structure as ostr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-4
MODES = [("f32", 1e-5), ("bf16x6", 1e-5), ("bf16x3", 1e-4), ("f16x3", 1e-5)]
LENGTHS = [1, 5, 31, 32, 33, 64, 256]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ref_segment(q, k, v, E=None, P=0):
    """fp64 attention of one segment: q [Lq,nh,64], k / v [Lk,nh,64] -> [Lq, nh*64]."""
    q, k, v = (t.permute(1, 0, 2)[None].double() for t in (q, k, v))
    s = q @ k.transpose(-1, -2)
    if E is not None:
        s = s + obert.relkey_scores_literal(q, E.double(), P)
    p = torch.softmax(s / 8.0, dim=-1)
    return (p @ v)[0].permute(1, 0, 2).reshape(q.shape[2], -1)


def packed_rows(x, lengths, nh):
    """[rows, nh*64] slices of the segments (packed back to back) as [L, nh, 64] views."""
    out, at = [], 0
    for n in lengths:
        out.append(x[at:at + n].reshape(n, nh, 64))
        at += n
    return out


@pytest.mark.parametrize("mode,tol", MODES)
def test_attention_varlen_self_relkey_against_fp64(pkg, hip, mode, tol):
    nh, P = 12, 256
    H = nh * 64
    lay = pkg.packing.PackedLayout(LENGTHS, P, DEV)
    qkv = torch.randn(lay.rows, 3 * H, generator=gen(1))
    qkv[lay.total:] = float("nan")          # the tail is no segment's: never read into a softmax
    E = torch.randn(2 * P - 1, 64, generator=gen(2))
    d = qkv.to(DEV)
    with torch.no_grad():
        got = pkg.ops.attention_varlen(d[:, :H], d[:, H:2 * H], d[:, 2 * H:], lay, lay, nh, dist_emb=E.to(DEV),
                                       max_pos=P, mode=mode).cpu()
    assert got.shape == (lay.rows, H)
    assert (got[lay.total:] == 0).all()      # tail rows are exactly zero
    qs, ks, vs = (packed_rows(qkv[:, i * H:(i + 1) * H], LENGTHS, nh) for i in range(3))
    want = torch.cat([ref_segment(q, k, v, E, P) for q, k, v in zip(qs, ks, vs)]).float()
    assert rel_err(got[:lay.total], want) < tol


@pytest.mark.parametrize("mode,tol", MODES)
@pytest.mark.parametrize("padded_keys", [False, True])
def test_attention_varlen_cross_against_fp64(pkg, hip, mode, tol, padded_keys):
    """q_len != k_len per segment; keys packed or a padded [B, Lr] cache (k_start = s * Lr) whose padding rows hold NaN."""
    nh, Lr = 12, 256
    H = nh * 64
    P = pkg.packing
    k_lengths = [7, 40, 256, 1, 64, 100, 33]
    q_lay = P.PackedLayout(LENGTHS, 256, DEV)
    k_lay = P.PackedLayout(k_lengths, Lr, DEV, padded_frame=padded_keys)
    q = torch.randn(q_lay.rows, H, generator=gen(3))
    kv_seg = [torch.randn(n, 2 * H, generator=gen(10 + s)) for s, n in enumerate(k_lengths)]
    kv = torch.full((k_lay.rows, 2 * H), float("nan"))
    for s, n in enumerate(k_lengths):
        kv[k_lay.starts[s]:k_lay.starts[s] + n] = kv_seg[s]
    dq, dkv = q.to(DEV), kv.to(DEV)
    with torch.no_grad():
        got = pkg.ops.attention_varlen(dq, dkv[:, :H], dkv[:, H:], q_lay, k_lay, nh, mode=mode).cpu()
    assert (got[q_lay.total:] == 0).all()
    want = torch.cat([ref_segment(qq, kk[:, :H].reshape(-1, nh, 64), kk[:, H:].reshape(-1, nh, 64))
                      for qq, kk in zip(packed_rows(q, LENGTHS, nh), kv_seg)]).float()
    assert rel_err(got[:q_lay.total], want) < tol


def test_attention_varlen_matches_the_padded_kernel_per_item(pkg, hip):
    """Each segment against ops.attention on that item alone in its own frame (bf16x6: both run the per-wave
    kernel's arithmetic): fp32-rounding agreement."""
    nh, P = 12, 256
    H = nh * 64
    lay = pkg.packing.PackedLayout(LENGTHS, P, DEV)
    d = torch.randn(lay.rows, 3 * H, generator=gen(4)).to(DEV)
    E = torch.randn(2 * P - 1, 64, generator=gen(5)).to(DEV)
    with torch.no_grad():
        got = pkg.ops.attention_varlen(d[:, :H], d[:, H:2 * H], d[:, 2 * H:], lay, lay, nh, dist_emb=E, max_pos=P,
                                       mode="bf16x6")
        for s, n in enumerate(LENGTHS):
            x = d[lay.starts[s]:lay.starts[s] + n]
            want = pkg.ops.attention(x[:, :H], x[:, H:2 * H], x[:, 2 * H:], 1, nh, n, n, dist_emb=E, max_pos=P,
                                     mode="bf16x6")
            assert rel_err(got[lay.starts[s]:lay.starts[s] + n], want) < 1e-5, n


def test_attention_varlen_refuses_grad_and_bad_layouts(pkg, hip):
    H = 64
    lay = pkg.packing.PackedLayout([5, 9], 16, DEV)
    other = pkg.packing.PackedLayout([9, 5], 16, DEV)
    x = torch.randn(lay.rows, 3 * H, device=DEV, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference-only"):
        pkg.ops.attention_varlen(x[:, :H], x[:, H:2 * H], x[:, 2 * H:], lay, lay, 1)
    E = torch.randn(31, 64, device=DEV)
    with torch.no_grad(), pytest.raises(ValueError, match="q_len == k_len"):
        pkg.ops.attention_varlen(x[:, :H], x[:, H:2 * H], x[:, 2 * H:], lay, other, 1, dist_emb=E, max_pos=16)


# ------------------------------------------------------------------------------------------------ structure model
def build(pkg, L, seed, layers=2):
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.structure_model.model import ConditionalBertForDiffusionBase
    common = dict(hidden_size=FULL_STRUCT["hidden_size"], num_attention_heads=FULL_STRUCT["num_heads"],
                  intermediate_size=FULL_STRUCT["intermediate_size"], num_hidden_layers=layers, max_position_embeddings=L)
    model = ConditionalBertForDiffusionBase(BertConfig(**common),
                                            BertConfig(**common, is_decoder=True, add_cross_attention=True), 8)
    sd = seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=seed)
    model.load_state_dict(sd, strict=True)
    return model.eval().to(DEV), sd


def packed_decode(pkg, model, t, x_t, d):
    P = pkg.packing
    lay, lay_r = P.layouts_or_none(d["ligand_attn_mask"], d["receptor_attn_mask"])
    cache = model.encode_receptor(d["receptor_seq"], d["receptor_angles"], d["receptor_attn_mask"], layout=lay_r)
    mod = model.timestep_modulation(t[:1].to(DEV))
    eps = model.decode(None, lay.pack(x_t.to(DEV)), None, cache, mod=mod, layout=lay)
    assert eps.shape == (lay.rows, 8)
    return lay.unpack(eps), lay


def test_structure_decode_packed_against_padded_trimmed_and_oracle(pkg, hip):
    B, L = 3, 64
    model, sd = build(pkg, L, seed=31)
    pk = synthetic_pockets(B, L, seed=8)
    d = {k: v.to(DEV) for k, v in pk.items() if torch.is_tensor(v)}
    x_t = ostr.modulo_with_wrapped_range(torch.randn(B, L, 8, generator=gen(6)))
    t = torch.full((B,), 517)
    args = (d["ligand_attn_mask"], d["receptor_seq"], d["receptor_angles"], d["receptor_attn_mask"])
    with torch.no_grad():
        got, lay = packed_decode(pkg, model, t, x_t, d)
        full = model(t.to(DEV), x_t.to(DEV), *args)
        Ll = 32                                                     # ligands are 5-30 residues: the trimmed frame
        trim = model(t.to(DEV), x_t[:, :Ll].to(DEV), d["ligand_attn_mask"][:, :Ll].contiguous(), *args[1:])
    valid = d["ligand_attn_mask"].bool()
    assert (got[~valid] == 0).all()
    want = ostr.forward(sd, {"num_heads": 12, "max_pos": L}, t, x_t, pk["ligand_attn_mask"], pk["receptor_seq"],
                        pk["receptor_angles"], pk["receptor_attn_mask"])
    assert rel_err(got[valid], want.to(DEV)[valid]) < TOL
    assert rel_err(got[valid], full[valid]) < 2e-5
    assert rel_err(got[:, :Ll][valid[:, :Ll]], trim[valid[:, :Ll]]) < 2e-5


def _chain_setup(pkg, B, L, T, seed=0):
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.structure_model.model import ConditionalBertForDiffusion as M
    from e3diff_amd.structure_model.utils import CosineTables, modulo_with_wrapped_range
    c = dict(hidden_size=768, num_attention_heads=12, intermediate_size=1024, num_hidden_layers=2,
             max_position_embeddings=L, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    torch.manual_seed(seed)
    model = M(BertConfig(**c), BertConfig(**c, is_decoder=True, add_cross_attention=True),
              feature_names=list("abcdefgh"), loss_func=[M.diheral_loss_func] * 8).eval().to(DEV)
    pk = {k: v.to(DEV) for k, v in synthetic_pockets(B, L, seed=3, rec_range=(20, 70)).items() if torch.is_tensor(v)}
    g = gen(5)
    x_T = modulo_with_wrapped_range(torch.randn(B, L, 8, generator=g)).to(DEV)
    noises = torch.randn(T, B, L, 8, generator=g).to(DEV)
    args = (model, pk["ligand_attn_mask"], x_T, pk["receptor_seq"], pk["receptor_attn_mask"], pk["receptor_angles"], T,
            CosineTables(T))
    return args, noises, pk


def test_packed_sampling_chain_equals_the_trimmed_one_on_valid_positions(pkg, hip):
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.utils import modulo_with_wrapped_range
    B, L, T = 3, 128, 6
    args, noises, pk = _chain_setup(pkg, B, L, T)
    trim = S.p_sample_loop(*args, noises=noises, return_device=True, step=1, trim_padding=True)
    packed = S.p_sample_loop(*args, noises=noises, return_device=True, step=1, pack=True)
    assert packed.shape == trim.shape == (T, B, L, 8)
    valid = pk["ligand_attn_mask"].bool()[None, :, :, None].expand_as(packed)
    # fp32-level rounding differences (other kernels by shape) through 6 steps of the amplifying reverse chain
    d = modulo_with_wrapped_range((packed - trim)[valid])
    assert d.abs().max() < 6e-4, d.abs().max()
    assert (packed[~valid] == 0).all()
    # a mask that is not a prefix cannot be packed: the chain runs the trimmed frame and says so
    holes = pk["ligand_attn_mask"].clone()
    holes[0, 100] = 1.0
    with pytest.warns(UserWarning, match="cannot be packed"):
        fb = S.p_sample_loop(args[0], holes, *args[2:], noises=noises, return_device=True, step=1, pack=True)
    assert torch.isfinite(fb).all()


def test_packed_chain_graph_replay_is_bit_identical_to_eager(pkg, hip):
    from e3diff_amd.structure_model import sample as S
    B, L, T = 3, 64, 8
    args, noises, _ = _chain_setup(pkg, B, L, T, seed=1)
    eager = S.p_sample_loop(*args, noises=noises, return_device=True, step=1, use_graph=False, pack=True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        graph = S.p_sample_loop(*args, noises=noises, return_device=True, step=1, use_graph=True, pack=True)
    assert not _capture_fallbacks(caught)    # a silent fall-back to eager launches would make this test vacuous
    assert torch.equal(eager, graph)
    free = S.p_sample_loop(*args, return_device=True, step=1, use_graph=True, pack=True)
    assert torch.isfinite(free).all() and free.abs().max() <= 3.1416


def _capture_fallbacks(caught):
    return [str(w.message) for w in caught if "HIP-graph capture" in str(w.message)]


def test_baseline_size_packed_step(pkg, hip):
    """B = 256 pockets in a 256-row frame with BioLiP-shaped lengths, the full 12 + 12 layers: the packed step is
    finite everywhere and its first items match the oracle."""
    B, L, NS = 256, 256, 2
    model, sd = build(pkg, L, seed=21, layers=FULL_STRUCT["num_hidden_layers"])
    pk = synthetic_pockets(B, L, seed=77)
    d = {k: v.to(DEV) for k, v in pk.items() if torch.is_tensor(v)}
    x_t = ostr.modulo_with_wrapped_range(torch.randn(B, L, 8, generator=gen(5)))
    t = torch.full((B,), 731)
    with torch.no_grad():
        got, lay = packed_decode(pkg, model, t, x_t, d)
    assert lay.rows < B * 32 and torch.isfinite(got).all()
    want = ostr.forward(sd, {"num_heads": 12, "max_pos": L}, t[:NS], x_t[:NS], pk["ligand_attn_mask"][:NS],
                        pk["receptor_seq"][:NS], pk["receptor_angles"][:NS], pk["receptor_attn_mask"][:NS])
    valid = pk["ligand_attn_mask"][:NS].bool()
    assert rel_err(got[:NS].cpu()[valid], want[valid]) < TOL


# ------------------------------------------------------------------------------------------------- sequence model
def build_seq(pkg, L, seed, layers=2, hidden=768, heads=12, wrapper=False, T=6):
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.sequence_model.model import ConditionalBertForDiffusionBase, PeptideDiff
    common = dict(hidden_size=hidden, num_attention_heads=heads, intermediate_size=1024, num_hidden_layers=layers,
                  max_position_embeddings=L)
    enc, dec = BertConfig(**common), BertConfig(**common, is_decoder=True, add_cross_attention=True)
    if wrapper:
        model = PeptideDiff(enc, dec, feature_names=list("ACDEFGHIKLMNPQRSTVWY"), loss_func=torch.nn.CrossEntropyLoss(),
                            noise_schedule="cosine", timesteps=T)
    else:
        model = ConditionalBertForDiffusionBase(enc, dec, 20)
    sd = seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=seed)
    model.load_state_dict(sd, strict=True)
    return model.eval().to(DEV), sd


def test_sequence_forward_packed_against_padded_trimmed_and_oracle(pkg, hip):
    import torch.nn.functional as TF
    from oracle import sequence as oseq
    B, L = 3, 64
    model, sd = build_seq(pkg, L, seed=41)
    pk = synthetic_pockets(B, L, seed=9, with_ligand_seq=True)
    d = {k: v.to(DEV) for k, v in pk.items() if torch.is_tensor(v)}
    x_t = TF.one_hot(torch.randint(0, 20, (B, L), generator=gen(3)), 20).float() * pk["ligand_attn_mask"][..., None]
    t = torch.full((B, 1), 17.0)
    lay, lay_r = pkg.packing.layouts_or_none(d["ligand_attn_mask"], d["receptor_attn_mask"])
    with torch.no_grad():
        got = model.forward_packed(t[:1].to(DEV), lay.pack(x_t.to(DEV)), lay.pack(d["ligand_angles"]),
                                   lay_r.pack(d["receptor_seq"]), lay_r.pack(d["receptor_angles"]), lay, lay_r)
        assert got.shape == (lay.rows, 20) and torch.isfinite(got).all()
        got = lay.unpack(got)
        args = (d["ligand_attn_mask"], d["receptor_seq"], d["receptor_angles"], d["receptor_attn_mask"])
        full = model(t.to(DEV), x_t.to(DEV), d["ligand_angles"], *args)
        Ll = 32
        trim = model(t.to(DEV), x_t[:, :Ll].contiguous().to(DEV), d["ligand_angles"][:, :Ll].contiguous(),
                     d["ligand_attn_mask"][:, :Ll].contiguous(), *args[1:])
        with pytest.raises(ValueError, match="one timestep"):
            model.forward_packed(t.to(DEV), lay.pack(x_t.to(DEV)), lay.pack(d["ligand_angles"]),
                                 lay_r.pack(d["receptor_seq"]), lay_r.pack(d["receptor_angles"]), lay, lay_r)
    valid = d["ligand_attn_mask"].bool()
    want = oseq.forward(sd, {"num_heads": 12, "max_pos": L}, t, x_t, pk["ligand_angles"], pk["ligand_attn_mask"],
                        pk["receptor_seq"], pk["receptor_angles"], pk["receptor_attn_mask"])
    assert rel_err(got[valid], want.to(DEV)[valid]) < TOL
    assert rel_err(got[valid], full[valid]) < 2e-5
    assert rel_err(got[:, :Ll][valid[:, :Ll]], trim[valid[:, :Ll]]) < 2e-5


def _seq_chain_setup(pkg, B=4, L=128, T=6, seed=2):
    from e3diff_amd.sequence_model.utils import DiscreteUniformTransition, PredefinedNoiseScheduleDiscrete
    qmodel, _ = build_seq(pkg, L, seed=seed, hidden=256, heads=4, wrapper=True, T=T)
    pk = dict(synthetic_pockets(B, L, seed=8, with_ligand_seq=True, rec_range=(20, 60)), structure_ids=None)
    sched = PredefinedNoiseScheduleDiscrete("cosine", T).to(DEV)
    return qmodel, pk, sched, DiscreteUniformTransition(20)


def test_packed_sequence_chain_gives_the_same_sequences(pkg, hip):
    """denoise(pack=True), argmax chain: the same predicted sequences and recovery rates as the padded chain."""
    from e3diff_amd.sequence_model.sample import denoise, generate_discrete_noise
    T = 6
    qmodel, pk, sched, tr = _seq_chain_setup(pkg, T=T)
    torch.manual_seed(4)
    x_T = generate_discrete_noise(4, 128, 20, DEV)
    full = denoise(pk, qmodel, sched, tr, False, x_T=x_T, timesteps=T)
    packed = denoise(pk, qmodel, sched, tr, False, x_T=x_T, timesteps=T, pack=True)
    assert packed[2] == full[2] and packed[1] == full[1] and packed[3] == full[3]
    # a mask that is not a prefix: the trimmed frame runs instead, and says so
    holes = dict(pk, ligand_attn_mask=pk["ligand_attn_mask"].clone())
    holes["ligand_attn_mask"][0, 100] = 1.0
    with pytest.warns(UserWarning, match="cannot be packed"):
        denoise(holes, qmodel, sched, tr, False, x_T=x_T, timesteps=T, pack=True)


def test_packed_sequence_chain_graph_replay_is_bit_identical_to_eager(pkg, hip):
    """GraphedDenoiseStep on packed rows against eager launches, injected uniforms (diverse chain): identical
    sequences; the capture does not fall back."""
    from e3diff_amd.sequence_model.sample import denoise, generate_discrete_noise
    T = 8
    qmodel, pk, sched, tr = _seq_chain_setup(pkg, T=T, seed=3)
    torch.manual_seed(5)
    x_T = generate_discrete_noise(4, 128, 20, DEV)
    us = [torch.rand(4, 128, generator=gen(100 + n)).to(DEV) for n in range(T)]
    eager = denoise(pk, qmodel, sched, tr, True, x_T=x_T, us=us, timesteps=T, pack=True, use_graph=False)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        graph = denoise(pk, qmodel, sched, tr, True, x_T=x_T, us=us, timesteps=T, pack=True, use_graph=True)
    assert not _capture_fallbacks(caught)
    assert graph[2] == eager[2] and graph[3] == eager[3]
