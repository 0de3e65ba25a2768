"""SELayer conditioning on one-hot rows: the modulation computed once per distinct row (``blocks.onehot_modulation``).

The pocket's ``receptor_seq`` rows are one-hot residue types or all-zero padding rows, so the per-token modulation
``adaLN_modulation(receptor_seq_emb(receptor_seq))`` takes at most F + 1 = 21 distinct values.  The table path classifies
the rows on the device, runs the embedding and both modulation GEMMs on the 21 canonical rows (padded to one 256-row
block, in the kernel form of the M-row launch), keeps the M-row launches behind a device flag that only a non-one-hot row
raises, and lets the gates look their row up.  Nothing of this may change a bit of the result:

* ``test_classification``: exact ``idx`` per row kind, the flag with and without rows that are neither one-hot nor zero;
* ``test_indexed_gate``: the looked-up gate against the dense-``mod`` gate fed the gathered rows, both chunk selections;
* ``test_encode_receptor_*``: ``encoder_states`` of the table path against the dense path (``blocks.ADALN_TABLE = False``:
  the launches of the parent commit), one-hot input and input with one soft row (the fallback), padded and packed frames;
* ``test_row_block_independent_of_m``: M = 256, N = 4608, K = 768 on the persistent 256x256 form (the form of the
  workload's M = 65 536 launch) against the same rows inside an M = 512 launch -- the smallest shape at which "a row
  block does not depend on M" can fail (a second row block on another workgroup, 18 against 36 tiles);
* ``test_gated_launches_*``: a zero flag leaves the outputs untouched, a raised one gives the ungated results.

Kernel forms in the end-to-end tests: at B = 2, L = 32 (M = 64) ``ops.gemm`` sends plain launches to the skinny (split-K)
kernels, whose K slicing depends on M, so no 256-row launch can reproduce their rows; the table path therefore applies
only where the M-row launch runs the tiled kernels (``ops.gemm_is_tiled``), as every batch of more than 512 rows does.
The tests reach that dispatch at M = 64 by setting ``ops.SKINNY_GEMM_MAX_M = 0`` (the E3D_GEMM_SKINNY_MAX_M switch) for
BOTH paths: dense and table GEMMs then share a kernel form (128x64 tiles at N = 768, 128x128 on eight waves at N = 4608),
and bit-equality is asserted for (a) and (b) alike.
"""
import pytest
import torch

from helpers import seeded_state_dict, synthetic_pockets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F_IN, H = 20, 768


def g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ classification
def _rows():
    """64 rows: the 20 one-hot rows, an all-zero row, a row with -0.0 beside its one, an all -0.0 row, then one-hot / zero
    filler -- and the four rows that are neither (two ones, a single 0.5, a one plus 1e-30 elsewhere, NaN) at the end."""
    x = torch.zeros(64, F_IN)
    want = torch.empty(64, dtype=torch.int32)
    for k in range(F_IN):
        x[k, k] = 1.0
        want[k] = k
    want[20] = F_IN                                   # all zero
    x[21] = -0.0
    x[21, 7] = 1.0
    want[21] = 7                                      # -0.0 elsewhere
    x[22] = -0.0
    want[22] = F_IN                                   # all -0.0
    for r in range(23, 60):
        if r % 3:
            x[r, (5 * r) % F_IN] = 1.0
            want[r] = (5 * r) % F_IN
        else:
            want[r] = F_IN
    good = (x.clone(), want.clone())
    x[60, 3] = x[60, 11] = 1.0                        # two ones
    x[61, 4] = 0.5                                    # a single 0.5
    x[62] = 1e-30
    x[62, 9] = 1.0                                    # a one, 1e-30 elsewhere
    x[63, 0] = 1.0
    x[63, 19] = float("nan")                          # NaN
    want[60:] = -1
    good[0][60:] = 0.0
    good[1][60:] = F_IN
    return good, (x, want)


@pytest.mark.parametrize("aligned", [True, False], ids=["float4", "scalar"])
def test_classification(pkg, hip, aligned):
    """Exact idx for every row kind; the flag stays zero without the four other rows and is raised with them.  ``scalar``:
    the same rows at a 4-byte offset (the kernel then reads them float by float)."""
    for case, (x, want) in zip(("one-hot only", "with other rows"), _rows()):
        if aligned:
            xd = x.to(DEV)
        else:
            buf = torch.zeros(x.numel() + 1)
            buf[1:] = x.reshape(-1)
            xd = buf.to(DEV)[1:].view(64, F_IN)
            assert xd.data_ptr() % 16 == 4
        idx, flag = pkg.ops.classify_onehot_rows(xd)
        assert idx.dtype == torch.int32 and torch.equal(idx.cpu(), want), (case, idx.cpu().tolist())
        assert (int(flag) != 0) == (case == "with other rows"), (case, int(flag))


# ------------------------------------------------------------------------------------------------ indexed gate
@pytest.mark.parametrize("branch", [0, 1])
def test_indexed_gate(pkg, hip, branch):
    """M = 64, H = 768: rows with idx >= 0 read the table, rows with idx = -1 (every fifth) read ``mod`` -- bit-equal to the
    dense gate on the gathered rows.  ``mod`` rows that must not be read hold NaN."""
    M = 64
    x, y = torch.randn(M, H, generator=g(1)).to(DEV), torch.randn(M, H, generator=g(2)).to(DEV)
    table = torch.randn(256, 6 * H, generator=g(3)).to(DEV)
    mod = torch.randn(M, 6 * H, generator=g(4)).to(DEV)
    idx = torch.randint(0, F_IN + 1, (M,), generator=g(5)).int()
    idx[::5] = -1
    idx = idx.to(DEV)
    gathered = torch.where((idx >= 0)[:, None], table[idx.clamp_min(0).long()], mod).contiguous()
    mod[idx >= 0] = float("nan")
    want = pkg.ops.adaln_gate(x, y, gathered, branch, 1)
    got = pkg.ops.adaln_gate_indexed(x, y, idx, table, mod, branch)
    assert torch.isfinite(want).all() and torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ gated launches
def test_gated_launches_skip_and_run(pkg, hip):
    """``run_if`` = 0: the output keeps its NaN fill; ``run_if`` != 0: bit-equal to the ungated launch.  One case per kernel
    family that takes the word: the general tiles (plan_m = 1024), the 256x256 tiles (64 rows planned as 65 536) and the
    persistent 256x256 form (256 rows planned as 65 536); then the two forms of the embedding (few rows, many rows), which
    must also agree with each other on the rows they share: the table's embedding runs the first, the M-row launch of a
    large batch the second."""
    ops = pkg.ops
    off, on = torch.zeros(1, dtype=torch.int32, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)
    a = torch.randn(256, H, generator=g(1)).to(DEV)
    for M, plan_m in ((64, 1024), (64, 65536), (256, 65536)):
        for N, act in ((H, ops.ACT_SILU), (6 * H, ops.ACT_NONE)):
            w, b = (torch.randn(N, H, generator=g(2)) / 28).to(DEV), torch.randn(N, generator=g(3)).to(DEV)
            want = ops.gemm(a[:M], w, b, act, plan_m=plan_m)
            out = torch.full((M, N), float("nan"), device=DEV)
            ops.gemm(a[:M], w, b, act, out=out, run_if=off, plan_m=plan_m)
            assert torch.isnan(out).all(), (M, plan_m, N)
            ops.gemm(a[:M], w, b, act, out=out, run_if=on, plan_m=plan_m)
            assert torch.isfinite(want).all() and torch.equal(out, want), (M, plan_m, N)
    xs = torch.randn(640, F_IN, generator=g(4)).to(DEV)
    xs[:21] = 0.0
    xs[:20] += torch.eye(F_IN, device=DEV)          # the canonical rows first
    w, b = torch.randn(H, F_IN, generator=g(5)).to(DEV), torch.randn(H, generator=g(6)).to(DEV)
    gamma, beta = torch.rand(H, generator=g(7)).to(DEV) + 0.5, torch.randn(H, generator=g(8)).to(DEV)
    many = ops.embed_layernorm(xs, w, b, gamma, beta, 1e-12)            # M > 512: W^T staged in LDS
    few = ops.embed_layernorm(xs[:64], w, b, gamma, beta, 1e-12)        # one wave per row
    assert torch.isfinite(many).all() and torch.equal(few, many[:64])
    assert torch.equal(ops.embed_layernorm(xs, w, b, gamma, beta, 1e-12, run_if=on), many)
    assert torch.equal(ops.embed_layernorm(xs[:64], w, b, gamma, beta, 1e-12, run_if=on), few)
    # (a skipped embedding leaves a fresh output buffer unwritten: nothing to observe through ops; the end-to-end tests
    #  below run it skipped and not skipped)


# ------------------------------------------------------------------------------------------------ workload form
def test_row_block_independent_of_m(pkg, hip):
    """The persistent 256x256 form (``plan_m`` = 65 536 selects it, as the workload's launch does): rows 0..255 and
    256..511 of an M = 512, N = 4608, K = 768 launch against the same rows as launches of their own.  Bit-equal."""
    ops = pkg.ops
    N, K = 4608, 768
    a = torch.randn(512, K, generator=g(1)).to(DEV)
    w, b = (torch.randn(N, K, generator=g(2)) / 28).to(DEV), torch.randn(N, generator=g(3)).to(DEV)
    for mode in ("f16x3", "bf16x3"):
        both = ops.gemm(a, w, b, mode=mode, plan_m=65536)
        for r0 in (0, 256):
            alone = ops.gemm(a[r0:r0 + 256], w, b, mode=mode, plan_m=65536)
            assert torch.equal(alone, both[r0:r0 + 256]), (mode, r0)
        ref = a.double().cpu() @ w.double().cpu().t() + b.double().cpu()
        assert ((both.cpu() - ref).abs().max() / ref.abs().max()).item() < (5e-6 if mode == "f16x3" else 3e-5)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def small_model(pkg):
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.structure_model.model import ConditionalBertForDiffusionBase
    L = 32
    common = dict(hidden_size=H, num_attention_heads=12, intermediate_size=1024, num_hidden_layers=2,
                  max_position_embeddings=L)
    model = ConditionalBertForDiffusionBase(BertConfig(**common),
                                            BertConfig(**common, is_decoder=True, add_cross_attention=True), 8)
    model.load_state_dict(seeded_state_dict({k: v.shape for k, v in model.state_dict().items()}, seed=1))
    pk = {k: v.to(DEV) for k, v in synthetic_pockets(2, L, seed=2).items() if torch.is_tensor(v)}
    return model.eval().to(DEV), pk


def _encode(pkg, monkeypatch, model, pk, table, receptor_seq=None, layout=None):
    """encoder_states of one ``encode_receptor`` call on the dense (parent) or the table path, plus what
    ``onehot_modulation`` returned."""
    from e3diff_amd.structure_model import model as model_module
    seen = []
    real = pkg.blocks.onehot_modulation

    def spy(*args):
        seen.append(real(*args))
        return seen[-1]

    monkeypatch.setattr(pkg.ops, "SKINNY_GEMM_MAX_M", 0)      # M = 64 on the tiled kernels, both paths (module docstring)
    monkeypatch.setattr(pkg.blocks, "ADALN_TABLE", table)
    monkeypatch.setattr(model_module, "onehot_modulation", spy)
    with torch.no_grad():
        rec = model.encode_receptor(pk["receptor_seq"] if receptor_seq is None else receptor_seq, pk["receptor_angles"],
                                    pk["receptor_attn_mask"], project_cross_kv=False, layout=layout)
    return rec.encoder_states, seen[0]


def test_encode_receptor_onehot(pkg, hip, small_model, monkeypatch):
    """(a) one-hot input: table path == dense path, bit for bit; the flag stays zero and every row has a table index."""
    model, pk = small_model
    want, none = _encode(pkg, monkeypatch, model, pk, table=False)
    got, mod = _encode(pkg, monkeypatch, model, pk, table=True)
    assert none is None and mod is not None
    assert int(mod.other_rows) == 0 and int(mod.idx.min()) >= 0 and int(mod.idx.max()) <= F_IN
    assert torch.isfinite(want).all() and torch.equal(got, want)


def test_encode_receptor_other_row_falls_back(pkg, hip, small_model, monkeypatch):
    """(b) one row replaced by a soft (non-one-hot) row: the flag is raised, the M-row launches run, that row reads its own
    modulation -- bit-equal to the dense path again."""
    model, pk = small_model
    seq = pk["receptor_seq"].clone()
    seq[1, 3] = 0.0
    seq[1, 3, 2] = seq[1, 3, 15] = 0.5
    want, _ = _encode(pkg, monkeypatch, model, pk, table=False, receptor_seq=seq)
    got, mod = _encode(pkg, monkeypatch, model, pk, table=True, receptor_seq=seq)
    assert int(mod.other_rows) != 0 and (mod.idx < 0).nonzero().flatten().tolist() == [1 * 32 + 3]
    assert torch.isfinite(want).all() and torch.equal(got, want)
    one_hot, _ = _encode(pkg, monkeypatch, model, pk, table=False)
    assert not torch.equal(one_hot, want)      # the soft row does change the result: the fallback was needed


def test_encode_receptor_packed_frame(pkg, hip, small_model, monkeypatch):
    """The packed frame (``layout=``): valid rows only, same statement."""
    model, pk = small_model
    layout = pkg.packing.PackedLayout.from_mask(pk["receptor_attn_mask"])
    want, _ = _encode(pkg, monkeypatch, model, pk, table=False, layout=layout)
    got, mod = _encode(pkg, monkeypatch, model, pk, table=True, layout=layout)
    assert mod is not None and int(mod.other_rows) == 0
    assert torch.isfinite(want).all() and torch.equal(got, want)


def test_training_and_grad_keep_the_dense_path(pkg, hip, small_model, monkeypatch):
    """Grad mode on with parameters that require grad: ``onehot_modulation`` declines (the autograd path is unchanged)."""
    model, pk = small_model
    monkeypatch.setattr(pkg.ops, "SKINNY_GEMM_MAX_M", 0)
    x2d = pkg.blocks.flat2d(pk["receptor_seq"])
    assert pkg.blocks.onehot_modulation(model.receptor_emb, model.receptor_seq_emb, x2d) is None
    with torch.no_grad():
        assert pkg.blocks.onehot_modulation(model.receptor_emb, model.receptor_seq_emb, x2d) is not None
