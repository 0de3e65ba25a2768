"""GPU: partial redesign -- chosen ligand positions held fixed in both samplers (replacement conditioning).
``e3d_known_compose_wrap`` against the numpy float64 statement (tests/known_ref.py) evaluated from the same fp32 table
row; its keyed form against the buffer form fed the keyed draws of stream 10; ``e3d_discrete_known_compose`` against
``discrete_q_sample`` + ``torch.where``; and chains: an empty mask changes nothing, held positions follow the forward law
and end on the known values bit for bit, eager against graph replay, seeded chains that follow the item through batch,
frame and launch mode, padding, the sequence chain, and the structure entry point.

Error bound of one composed element (u = 2^-24), counting the fp32 roundings of the expression as the kernel writes it,
    n = wrap_pi(scale * z);  v = a * x0 + s1m * n;  x = wrap_pi(v),      G = |a x0| + |s1m n|:
  * the product scale * z: u |scale z|, carried through the inner wrap unchanged and scaled by s1m;
  * the inner wrap_pi's two additions: 4 u (|scale z| + pi), scaled by s1m (the allowance test_strided_gpu.py makes for a
    wrap: the shift by pi, the shift back and the fp32 value of 2 pi against the float64 one);
  * two products and a sum: each at most u of G to first order, 5 u G covers second order;
  * the outer wrap_pi: 4 u (|v| + pi), compared by circular distance.
So |got - ref|_circ <= s1m (u |sz| + 4 u (|sz| + pi)) + 5 u G + 4 u (|v| + pi), sz = scale z.  Elements whose float64 sz
lies within 8 u |sz| of an odd multiple of pi are excluded: there a legitimate rounding moves n by 2 pi, which s1m < 1 does
not map onto the circle again.  For standard normals that is about 2e-8 of the elements; the fixed seed excludes none
(checked on the float64 statement alone in ``data``), and the test requires the share to stay below 0.1 %.

Where a chain test compares held positions against tests/keyed_ref.py, the reference normals are float64 Box-Muller
values and the device's are fp32: test_keyed_sampling_gpu.py holds them to 2e-6 max(1, |z|), and that allowance, scaled by
s1m * scale, is added to the bound (and to the exclusion margin) there -- nowhere else.
"""
import warnings

import numpy as np
import pytest
import torch

import keyed_ref as K
import known_ref as KR
from test_keyed_sampling_gpu import WRAPPED_TOL, _seq_setup, _structure_setup, _wrapped_diff, key_table

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
N_BIG = 2048 * 256 * 4 + 5                 # more float4 groups than the capped grid has threads, plus a tail
SIZES = (1, 3, 4, 5, 8 * 37, N_BIG)
TIMESTEPS = (999, 980, 500, 20, 0)         # 999 is not visited at step 20: its row is NaN
T_FULL, STEP = 1000, 20
Z_TOL = 2e-6                               # fp32 Box-Muller against keyed_ref's float64 (test_keyed_sampling_gpu.py)


def _t(t):
    return torch.full((1,), t, dtype=torch.int64, device=DEV)


_excluded = KR.excluded


def _bound(row, parts, z_err=0.0):
    s1m = float(row[1])
    asz = np.abs(parts["sz"])
    return s1m * (U * asz + 4 * U * (asz + np.pi) + z_err) + 5 * U * parts["G"] + 4 * U * (np.abs(parts["v"]) + np.pi)


@pytest.fixture(scope="module")
def data(pkg, hip):
    """Inputs shared by the kernel tests (smaller sizes are prefixes of the largest) and the level table."""
    from e3diff_amd.structure_model.utils import CosineTables, KnownLevels
    x, x0, z, mask = KR.kernel_inputs(N_BIG)
    # the exclusion zone on the float64 statement alone, for both scales the tests use: the fixed seed excludes nothing
    # (test_known_cpu.py makes the same check where no GPU is needed)
    for scale in (1.0, 1.5):
        assert not _excluded(scale * z.astype(np.float64)).any()
    kl = KnownLevels(CosineTables(T_FULL), list(reversed(range(0, T_FULL, STEP))))
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in (("x", x), ("x0", x0), ("z", z), ("mask", mask))}
    return {"x": x, "x0": x0, "z": z, "mask": mask, "dev": dev, "kl": kl, "levels": kl.levels.to(DEV)}


# ------------------------------------------------------------------------------------------------ structure kernel
@pytest.mark.parametrize("scale", [1.0, 1.5])
def test_compose_against_the_float64_ref(pkg, hip, data, scale):
    ops, d = pkg.ops, data["dev"]
    rows = data["kl"].levels.numpy()
    worst = 0.0
    for t in TIMESTEPS:
        for n in SIZES:
            x_in = d["x"][:n].clone()
            got_t = ops.known_compose_wrap(x_in, d["x0"][:n], d["mask"][:n], d["z"][:n], data["levels"], _t(t), scale)
            assert got_t is x_in
            held = d["mask"][:n] != 0
            assert torch.equal(got_t[~held], d["x"][:n][~held]), (t, n, "a free element was written")
            if t == 999:                                            # not visited: NaN where held, the rest untouched
                assert np.isnan(rows[t]).all() and torch.isnan(got_t[held]).all()
                continue
            if t == 0:                                              # the clean level: x0, a copy
                assert rows[t, 0] == 1.0 and rows[t, 1] == 0.0 and torch.equal(got_t[held], d["x0"][:n][held])
                continue
            ref, parts = KR.compose(rows[t], data["x"][:n], data["x0"][:n], data["mask"][:n], data["z"][:n], scale)
            h = held.cpu().numpy()
            keep = h & ~_excluded(parts["sz"])
            assert 1.0 - keep.sum() / max(h.sum(), 1) < 1e-3, (t, n, "excluded share")
            got = got_t.cpu().numpy().astype(np.float64)
            assert np.abs(got[h]).max(initial=0.0) <= np.pi + 1e-6
            err, bound = KR.circ(got, ref)[keep], _bound(rows[t], parts)[keep]
            ratio = (err / bound).max(initial=0.0)
            worst = max(worst, ratio)
            print(f"known compose scale={scale} t={t} n={n}: worst |got - ref| / bound = {ratio:.3f}")
            assert (err <= bound).all(), (t, n, scale, "worst |got - ref| / bound", ratio)
    print(f"known compose scale={scale}: worst |got - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("bad", [-1, T_FULL])
def test_step_index_outside_the_table_and_missing_draws_give_nan(pkg, hip, data, bad):
    ops, d = pkg.ops, data["dev"]
    n = 4 * 300 + 3
    held = d["mask"][:n] != 0
    x = d["x"][:n].clone()
    ops.known_compose_wrap(x, d["x0"][:n], d["mask"][:n], d["z"][:n], data["levels"], _t(bad))
    assert torch.isnan(x[held]).all() and torch.equal(x[~held], d["x"][:n][~held])
    # no draws: fine at the clean level, NaN at a noisy one
    x = d["x"][:n].clone()
    ops.known_compose_wrap(x, d["x0"][:n], d["mask"][:n], None, data["levels"], _t(0))
    assert torch.equal(x[held], d["x0"][:n][held])
    ops.known_compose_wrap(x, d["x0"][:n], d["mask"][:n], None, data["levels"], _t(500))
    assert torch.isnan(x[held]).all() and torch.equal(x[~held], d["x"][:n][~held])
    # the clean level reads nothing through noise
    x = d["x"][:n].clone()
    ops.known_compose_wrap(x, d["x0"][:n], d["mask"][:n], torch.full((n,), float("nan"), device=DEV), data["levels"], _t(0))
    assert torch.equal(x[held], d["x0"][:n][held])
    with pytest.raises(ValueError):
        ops.known_compose_wrap(x, d["x0"][:n - 1], d["mask"][:n], None, data["levels"], _t(0))
    with pytest.raises(TypeError):
        ops.known_compose_wrap(x, d["x0"][:n], held, None, data["levels"], _t(0))


def test_keyed_compose_equals_the_buffer_form_with_the_keyed_draws(pkg, hip, data):
    ops = pkg.ops
    keys = key_table().to(DEV)
    rows = keys.shape[0]
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(rows, 8, generator=g) * 6 - 3).to(DEV)
    x0 = (torch.rand(rows, 8, generator=g) * 6 - 3).to(DEV)
    mask = (torch.rand(rows, 8, generator=g) < 0.5).to(torch.uint8)
    mask[3] = 0                                                     # a free row, a held row, the sentinel row held
    mask[4] = 1
    mask[-1] = 1
    mask = mask.to(DEV)
    held = mask != 0
    seed = 77
    for scale in (1.0, 1.5):
        for t in (980, 500, 20, 0):
            z = ops.keyed_draws(keys, seed, 10, t, ops.KEYED_NORMAL, 8)
            assert not torch.equal(z, ops.keyed_draws(keys, seed, 1, t, ops.KEYED_NORMAL, 8))       # a stream of its own
            got = ops.keyed_known_compose_wrap(x.clone(), x0, mask, data["levels"], _t(t), keys, seed, scale)
            want = ops.known_compose_wrap(x.clone(), x0, mask, z, data["levels"], _t(t), scale)
            assert torch.equal(got[:-1], want[:-1]), (scale, t)
            assert torch.equal(got[-1], x[-1])                                                      # sentinel row: untouched
            assert torch.equal(got[~held], x[~held])
            if t == 0:
                assert torch.equal(got[:-1][held[:-1]], x0[:-1][held[:-1]])
            else:
                assert torch.isfinite(got).all() and not torch.equal(got[:-1][held[:-1]], x0[:-1][held[:-1]])
    got = ops.keyed_known_compose_wrap(x.clone(), x0, mask, data["levels"], _t(999), keys, seed)
    assert torch.isnan(got[:-1][held[:-1]]).all() and torch.equal(got[-1], x[-1]) and torch.equal(got[~held], x[~held])
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.keyed_known_compose_wrap(x[:, :6].contiguous(), x0[:, :6].contiguous(), mask[:, :6].contiguous(), data["levels"],
                                     _t(0), keys, seed)


# ------------------------------------------------------------------------------------------------ sequence kernel
def _transition(name):
    from e3diff_amd.sequence_model.utils import BlosumTransition, DiscreteUniformTransition
    return BlosumTransition(x_classes=20) if name == "blosum" else DiscreteUniformTransition(20)


@pytest.mark.parametrize("trans_name", ["blosum", "uniform"])
@pytest.mark.parametrize("B,L", [(1, 1), (1, 5), (3, 5), (1, 64), (3, 64), (1, 96)])     # (1, 96): a packed buffer's shape
def test_discrete_compose_equals_q_sample_and_where(pkg, hip, trans_name, B, L):
    from e3diff_amd import keyed
    from e3diff_amd.sequence_model.utils import PredefinedNoiseScheduleDiscrete
    ops, C, T = pkg.ops, 20, 50
    sched, trans = PredefinedNoiseScheduleDiscrete("cosine", T).to(DEV), _transition(trans_name)
    g = torch.Generator().manual_seed(B * 100 + L)
    idx = torch.randint(0, C, (B, L), generator=g).int().to(DEV)
    x0 = torch.randint(0, C, (B, L), generator=g).int()
    if L >= 5:
        x0[:, 3] = -1                                               # an all-zero (padding) row: untouched
    x0 = x0.to(DEV)
    mask = (torch.rand(B, L, generator=g) < 0.5).to(torch.uint8)
    mask[:, 0] = 1
    if L >= 5:
        mask[:, 3] = 1
        mask[:, 4] = 0
    mask = mask.to(DEV)
    u = torch.rand(B, L, generator=g).to(DEV)
    ids = [5, (1 << 40) + 3, 9][:B]
    keys = keyed.padded_keys(ids, L, DEV)
    if (B, L) == (1, 96):                                           # packed: two segments and a tail of no item
        keys = keys.clone()
        keys[40:80, 0], keys[40:80, 1] = 11, torch.arange(40, device=DEV)
        keys[80:] = -1
    valid = (keys[:, 1] >= 0).reshape(B, L)
    touch = (mask != 0) & (x0 >= 0)
    for s_int in (1, 24, 48):
        qsb = trans.get_Qt_bar(sched.get_alpha_bar(t_normalized=torch.full((B, 1), s_int / T, device=DEV)), DEV).contiguous()
        for diverse in (True, False):
            uu = u if diverse else None
            want = torch.where(touch, ops.discrete_q_sample(x0, qsb, uu), idx)
            got = ops.discrete_known_compose(idx.clone(), x0, mask, qsb, uu)
            assert got.dtype == torch.int32 and torch.equal(got, want), (s_int, diverse)
        ku = ops.keyed_draws(keys, 21, 11, s_int, ops.KEYED_UNIFORM).reshape(B, L)
        assert not torch.equal(ku, ops.keyed_draws(keys, 21, 3, s_int, ops.KEYED_UNIFORM).reshape(B, L))
        want = torch.where(touch & valid, ops.discrete_q_sample(x0, qsb, ku), idx)
        got = ops.keyed_discrete_known_compose(idx.clone(), x0, mask, qsb, keys, 21, _t(s_int))
        assert torch.equal(got, want), (s_int, "keyed")


@pytest.mark.parametrize("C", [2, 20, 32])
def test_the_three_column_draws_agree(pkg, hip, C):
    """discrete_q_sample, discrete_known_compose (full mask) and keyed_discrete_forward_levels draw a row from column x0 of
    its item's table: fed the same tables, x0 and uniforms -- the keyed stream 11 of one step -- they return the same
    classes wherever a row has a clean class and an item.  B = 2 items with tables of their own (some entries zero),
    L = 257: one row past a 256-thread block.  Elsewhere each keeps its own rule: a padding row (x0 = -1) is class 0 for
    q_sample and forward_levels and left alone by the compose; a row of no item (key position < 0) is class 0 for
    forward_levels, while the two buffer forms know no keys and draw with the u = 0 that keyed_draws gives such a row."""
    from e3diff_amd import keyed
    ops, B, L, seed, step, base = pkg.ops, 2, 257, 21, 17, 99
    g = torch.Generator().manual_seed(C)
    q = torch.rand(B, C, C, generator=g)
    q[q < 0.25] = 0.0
    x0 = torch.randint(0, C, (B, L), generator=g).int()
    x0[:, 3::11] = -1
    keys = keyed.padded_keys([5, (1 << 40) + 3], L, "cpu").clone()
    keys[7::13, 1] = -1
    q, x0, keys = q.to(DEV).contiguous(), x0.to(DEV), keys.to(DEV)
    item, clean = (keys[:, 1] >= 0).reshape(B, L), x0 >= 0
    assert bool((~item & clean).any()) and bool((item & ~clean).any()) and bool((~item & ~clean).any())
    u = ops.keyed_draws(keys, seed, 11, step, ops.KEYED_UNIFORM).reshape(B, L)
    assert bool((u[~item] == 0).all())
    drawn = ops.discrete_q_sample(x0, q, u)
    composed = ops.discrete_known_compose(torch.full((B, L), base, dtype=torch.int32, device=DEV), x0,
                                          torch.ones(B, L, dtype=torch.uint8, device=DEV), q, u)
    forward = ops.keyed_discrete_forward_levels(x0, q, keys, torch.full((B,), step, dtype=torch.long, device=DEV), seed, 49)
    both = item & clean
    assert torch.equal(drawn[both], composed[both]) and torch.equal(drawn[both], forward[both])
    assert len(torch.unique(drawn[both])) > 1 and not torch.equal(drawn[0], drawn[1])
    assert bool((drawn[~clean] == 0).all()) and bool((forward[~clean] == 0).all()) and bool((composed[~clean] == base).all())
    assert bool((forward[~item] == 0).all()) and torch.equal(drawn[~item & clean], composed[~item & clean])


# ------------------------------------------------------------------------------------------------ structure chains
T_CHAIN, B_CHAIN, L_CHAIN = 6, 4, 128
IDS = [11, (1 << 35) + 2, 7, 123456]
SCALE = 1.0


@pytest.fixture(scope="module")
def setup(pkg, hip):
    from e3diff_amd.structure_model.utils import modulo_with_wrapped_range
    model, pk, tab = _structure_setup(B=B_CHAIN, L=L_CHAIN, T=T_CHAIN)
    g = torch.Generator().manual_seed(5)
    x_T = modulo_with_wrapped_range(torch.randn(B_CHAIN, L_CHAIN, 8, generator=g)).to(DEV)
    noises = torch.randn(T_CHAIN, B_CHAIN, L_CHAIN, 8, generator=g).to(DEV)
    known_noises = torch.randn(T_CHAIN, B_CHAIN, L_CHAIN, 8, generator=g).to(DEV)
    valid = pk["ligand_attn_mask"].bool()
    assert int(valid.sum(dim=1).min()) >= 5
    res = torch.zeros(B_CHAIN, L_CHAIN, dtype=torch.bool, device=DEV)
    res[:, 1:4] = True                                              # an anchor: residues 1-3 (every ligand has >= 5)
    res[:, 100] = True                                              # a bit on padding: ignored
    elem = torch.zeros(B_CHAIN, L_CHAIN, 8, dtype=torch.bool, device=DEV)
    elem[:, 0:3, :4] = True                                         # the dihedrals of residues 0-2, their bond angles free
    elem[:, 2, 5] = True
    return {"model": model, "pk": pk, "tab": tab, "x_T": x_T, "noises": noises, "known_noises": known_noises,
            "known": pk["ligand_angles"].clone(), "res": res, "elem": elem, "valid": valid}


def _args(s, sel=None, x_T=None):
    pk = s["pk"] if sel is None else {k: v[sel].contiguous() for k, v in s["pk"].items()}
    x_T = s["x_T"] if x_T is None else x_T
    x_T = x_T if sel is None else x_T[sel].contiguous()
    return (s["model"], pk["ligand_attn_mask"], x_T, pk["receptor_seq"], pk["receptor_attn_mask"], pk["receptor_angles"],
            T_CHAIN, s["tab"])


def _held3(s, mask):
    """The effective [B, L, F] mask: and-ed with the padding mask."""
    m = mask if mask.dim() == 3 else mask[..., None].expand(-1, -1, 8)
    return m & s["valid"][..., None]


def _order(step):
    return list(reversed(range(0, T_CHAIN, step)))


def _graphed_chain(S, s, step=1, strided_eta=None, noises=None, known_noises=None, seed=None, known=None, mask=None):
    """The padded chain with every step replayed from one captured GraphedReverseStep (p_sample_loop itself never
    replays chains of up to four steps)."""
    from e3diff_amd import keyed
    from e3diff_amd.structure_model.utils import KnownLevels, StridedTables
    model, pk, order = s["model"], s["pk"], _order(step)
    st = None if strided_eta is None else StridedTables(s["tab"], order, strided_eta)
    cache = model.encode_receptor(pk["receptor_seq"], pk["receptor_angles"], pk["receptor_attn_mask"])
    mod_rows = model.timestep_modulation(torch.tensor(order, device=DEV, dtype=torch.long))
    mod_table = torch.zeros((T_CHAIN, mod_rows.shape[1]), device=DEV)
    mod_table[order] = mod_rows
    keys = None if seed is None else keyed.padded_keys(IDS, L_CHAIN, DEV)
    kn = None
    if known is not None:
        kn = (known.contiguous(), _held3(s, mask).to(torch.uint8).contiguous(), KnownLevels(s["tab"], order), SCALE)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        g = S.GraphedReverseStep(model, pk["ligand_attn_mask"].contiguous().float(), cache, s["tab"], s["x_T"],
                                 draw=noises is None, mod_table=mod_table, row_keys=keys, seed=seed, strided=st, known=kn)
    out, x = [], s["x_T"]
    for n, i in enumerate(order):
        x = g.step(i, x, None if noises is None else noises[n], None if known_noises is None else known_noises[n])
        out.append(x.clone())
    return torch.stack(out)


def test_an_empty_mask_changes_nothing(pkg, hip, setup):
    from e3diff_amd.structure_model import sample as S
    s = setup
    none = torch.zeros(B_CHAIN, L_CHAIN, dtype=torch.bool, device=DEV)
    pad_only = none.clone()
    pad_only[:, 100] = True                                         # and-ed with the padding mask: nothing is held
    for use_graph in (False, True):
        for draws in (dict(noises=s["noises"]), dict(seed=9, item_ids=IDS)):
            kw = dict(return_device=True, step=1, use_graph=use_graph, **draws)
            base = S.p_sample_loop(*_args(s), **kw)
            for m in (none, pad_only):
                assert torch.equal(S.p_sample_loop(*_args(s), known=s["known"], known_mask=m, **kw), base)
    # no generator use either: default draws, the same torch seed, the same chain
    torch.manual_seed(3)
    base = S.p_sample_loop(*_args(s), return_device=True, step=1, use_graph=False)
    state = torch.cuda.get_rng_state(DEV)
    torch.manual_seed(3)
    got = S.p_sample_loop(*_args(s), return_device=True, step=1, use_graph=False, known=s["known"], known_mask=none)
    assert torch.equal(got, base) and torch.equal(torch.cuda.get_rng_state(DEV), state)


@pytest.mark.parametrize("which", ["res", "elem"])
def test_held_positions_follow_the_forward_law(pkg, hip, setup, which):
    """Independent of the model: every entry's held elements are the float64 compose of ``known`` at that entry's level
    with the keyed_ref normals of stream 10; the last entry is ``known``; the conditioning reaches the decoder."""
    from e3diff_amd import keyed
    from e3diff_amd.structure_model import sample as S
    s, seed = setup, 2024
    held = _held3(s, s[which])
    kw = dict(return_device=True, step=1, seed=seed, item_ids=IDS, use_graph=False)
    free_chain = S.p_sample_loop(*_args(s), **kw)
    traj = S.p_sample_loop(*_args(s), known=s["known"], known_mask=s[which], known_scale=SCALE, **kw)
    assert traj.shape == (T_CHAIN, B_CHAIN, L_CHAIN, 8) and torch.isfinite(traj).all()
    assert torch.equal(traj[-1][held], s["known"][held])                           # bit for bit
    assert torch.equal(traj[0][~held], free_chain[0][~held])                       # x_T is uncomposed: the first update agrees
    free_valid = ~held & s["valid"][..., None]
    assert not torch.equal(traj[1][free_valid], free_chain[1][free_valid])         # the decoder read the held content
    rows = KR.table(s["tab"].betas.numpy(), _order(1))
    keys = keyed.padded_keys(IDS, L_CHAIN, "cpu").numpy()
    h = held.cpu().numpy().reshape(-1, 8)
    known = s["known"].cpu().numpy().reshape(-1, 8)
    worst = 0.0
    for n, t in enumerate(_order(1)[:-1]):
        z = K.normals(keys, seed, 10, t, 8)
        ref, parts = KR.compose(rows[t], np.zeros_like(known), known, h, z, SCALE)
        z_err = SCALE * Z_TOL * np.maximum(1.0, np.abs(z))
        keep = h & ~_excluded(parts["sz"], z_err)
        assert keep.sum() >= 0.999 * h.sum()
        got = traj[n].cpu().numpy().reshape(-1, 8).astype(np.float64)
        err, bound = KR.circ(got, ref)[keep], _bound(rows[t], parts, z_err)[keep]
        worst = max(worst, (err / bound).max())
        assert (err <= bound).all(), (which, t, (err / bound).max())
    print(f"held positions ({which}): worst |got - ref| / bound = {worst:.3f}")


CHAINS = [dict(step=1), dict(step=3), dict(step=1, update="strided", eta=0.0), dict(step=1, update="strided", eta=1.0)]


@pytest.mark.parametrize("chain", CHAINS, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_eager_chain_equals_the_graphed_chain(pkg, hip, setup, chain):
    from e3diff_amd.structure_model import sample as S
    s, step = setup, chain["step"]
    n = len(_order(step))
    eta = chain.get("eta") if chain.get("update") == "strided" else None
    held = _held3(s, s["elem"])
    for draws in ("injected", "seeded"):
        if draws == "injected":
            kw = dict(noises=s["noises"][:n], known_noises=s["known_noises"][:n])
            gkw = dict(noises=s["noises"][:n], known_noises=s["known_noises"][:n])
        else:
            kw = dict(seed=41, item_ids=IDS)
            gkw = dict(seed=41)
        with torch.no_grad():
            eager = S.p_sample_loop(*_args(s), return_device=True, use_graph=False, known=s["known"], known_mask=s["elem"],
                                    known_scale=SCALE, **chain, **kw)
            graph = _graphed_chain(S, s, step=step, strided_eta=eta, known=s["known"], mask=s["elem"], **gkw)
        assert eager.shape == (n, B_CHAIN, L_CHAIN, 8) and torch.isfinite(eager).all() and eager.abs().max() <= 3.1416
        assert torch.equal(eager, graph), (chain, draws)
        assert torch.equal(eager[-1][held], s["known"][held])
        if n > 1:
            assert not torch.equal(eager[0][held], s["known"][held])
    if step == 1:       # and through p_sample_loop's own capture (six steps: long enough to replay)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            own = S.p_sample_loop(*_args(s), return_device=True, use_graph=True, known=s["known"], known_mask=s["elem"],
                                  known_scale=SCALE, **chain, seed=41, item_ids=IDS)
        assert torch.equal(own, eager)
        # default draws inside the graph: the held positions still end on the known values
        torch.manual_seed(0)
        own = S.p_sample_loop(*_args(s), return_device=True, use_graph=True, known=s["known"], known_mask=s["elem"], **chain)
        assert torch.isfinite(own).all() and torch.equal(own[-1][held], s["known"][held])


def _seeded(S, s, seed, mask, sel=None, **kw):
    sel = list(range(B_CHAIN)) if sel is None else sel
    ids = [IDS[i] for i in sel]
    args = list(_args(s, sel))
    args[2] = S.keyed_x_T(seed, ids, L_CHAIN, 8, device=DEV)
    return S.p_sample_loop(*args, return_device=True, step=1, seed=seed, item_ids=ids, known=s["known"][sel].contiguous(),
                           known_mask=mask[sel].contiguous(), known_scale=SCALE, **kw)


def test_seeded_chain_with_held_positions_follows_the_item(pkg, hip, setup):
    from e3diff_amd.structure_model import sample as S
    s, seed, mask = setup, 2024, setup["elem"] | setup["res"][..., None]
    held = _held3(s, mask)[None].expand(T_CHAIN, -1, -1, -1)
    free = (~_held3(s, mask) & s["valid"][..., None])[None].expand(T_CHAIN, -1, -1, -1)
    base = _seeded(S, s, seed, mask)
    assert torch.isfinite(base).all() and torch.equal(_seeded(S, s, seed, mask), base)
    assert _wrapped_diff(_seeded(S, s, seed + 1, mask)[:-1], base[:-1], held[:-1]) > 0.1
    rev = _seeded(S, s, seed, mask, sel=[3, 2, 1, 0])
    for b in range(B_CHAIN):
        assert torch.equal(rev[:, 3 - b], base[:, b])
    one = _seeded(S, s, seed, mask, sel=[2])
    assert torch.equal(one[:, 0][held[:, 2]], base[:, 2][held[:, 2]])
    assert _wrapped_diff(one[:, 0], base[:, 2], free[:, 2]) < WRAPPED_TOL
    for frame in (dict(trim_padding=True), dict(pack=True)):
        got = _seeded(S, s, seed, mask, **frame)
        assert torch.equal(got[held], base[held]), frame
        assert _wrapped_diff(got, base, free) < WRAPPED_TOL, frame
        # padding comes back as without a mask: zeros at the rows the frame dropped (trimmed: beyond the longest ligand
        # rounded up to 32; packed: every padding row)
        dropped = ~s["valid"] if "pack" in frame else torch.arange(L_CHAIN, device=DEV)[None].expand(B_CHAIN, -1) >= S.trimmed_length(s["pk"]["ligand_attn_mask"])
        assert dropped.any() and (got[:, dropped] == 0).all(), frame
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert torch.equal(_seeded(S, s, seed, mask, use_graph=True, **frame), _seeded(S, s, seed, mask, use_graph=False, **frame))
    # mask bits on padding are ignored: the chain with them is the chain without them
    no_pad_bits = mask & s["valid"][..., None]
    assert not torch.equal(no_pad_bits, mask) and torch.equal(_seeded(S, s, seed, no_pad_bits), base)


def test_p_sample_takes_the_held_positions(pkg, hip, setup):
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.utils import KnownLevels
    s = setup
    kl = KnownLevels(s["tab"], _order(1))
    a = list(_args(s))[:6] + [4, s["tab"]]
    held = _held3(s, s["res"])
    plain = S.p_sample(*a, noise=s["noises"][0], wrap=True)
    got = S.p_sample(*a, noise=s["noises"][0], wrap=True, known=s["known"], known_mask=s["res"], known_noise=s["known_noises"][0],
                     known_levels=kl)
    assert torch.equal(got[~held], plain[~held]) and not torch.equal(got[held], plain[held])
    want = pkg.ops.known_compose_wrap(plain.clone(), s["known"], held.to(torch.uint8).contiguous(), s["known_noises"][0],
                                      kl.levels.to(DEV), _t(4))
    assert torch.equal(got, want)
    keyed_got = S.p_sample(*a, seed=5, item_ids=IDS, wrap=True, known=s["known"], known_mask=s["res"], known_levels=kl)
    z = pkg.ops.keyed_draws(pkg.keyed.padded_keys(IDS, L_CHAIN, DEV), 5, 10, 4, pkg.ops.KEYED_NORMAL, 8).reshape(B_CHAIN, L_CHAIN, 8)
    plain = S.p_sample(*a, seed=5, item_ids=IDS, wrap=True)
    assert torch.equal(keyed_got, pkg.ops.known_compose_wrap(plain.clone(), s["known"], held.to(torch.uint8).contiguous(), z,
                                                             kl.levels.to(DEV), _t(4)))
    last = S.p_sample(*a[:6], 0, s["tab"], wrap=True, known=s["known"], known_mask=s["res"], known_levels=kl)
    assert torch.equal(last[held], s["known"][held])


# ------------------------------------------------------------------------------------------------ sequence chain
@pytest.fixture(scope="module")
def seq(pkg, hip):
    T = 8                                                            # long enough for denoise's own graph capture
    model, pk, sched, tr = _seq_setup(T, B_CHAIN)
    valid = pk["ligand_attn_mask"].bool()
    mask = torch.zeros(B_CHAIN, 128, dtype=torch.bool)
    mask[:, 1:4] = True
    mask[:, 100] = True                                              # padding: ignored
    mask[3] = valid[3]                                               # an item with no free position
    return {"T": T, "model": model, "pk": pk, "sched": sched, "tr": tr, "mask": mask, "valid": valid,
            "lengths": [int(n) for n in valid.sum(dim=1)]}


def _recovery_over(pred, true, cols):
    return float(np.float32(sum(pred[c] == true[c] for c in cols)) / np.float32(len(cols))) if cols else float("nan")


def test_sequence_chain_holds_the_true_residues(pkg, hip, seq):
    from e3diff_amd.sequence_model.sample import denoise
    q, T = seq, seq["T"]
    kw = dict(timesteps=T, seed=5, item_ids=IDS)
    base = denoise(q["pk"], q["model"], q["sched"], q["tr"], True, **kw)
    got = denoise(q["pk"], q["model"], q["sched"], q["tr"], True, known_mask=q["mask"], use_graph=False, **kw)
    assert len(got) == 4 and got[0] == base[0] and got[1] == base[1]
    assert got[2] != base[2]
    for b in range(B_CHAIN):
        true, pred, n = got[1][b], got[2][b], q["lengths"][b]
        assert len(pred) == n
        held_cols = list(range(n)) if b == 3 else [c for c in (1, 2, 3) if c < n]
        assert all(pred[c] == true[c] for c in held_cols), b
        free_cols = [c for c in range(n) if c not in held_cols]
        want = _recovery_over(pred, true, free_cols)
        assert (np.isnan(got[3][b]) and np.isnan(want)) or abs(got[3][b] - want) < 1e-6, (b, got[3][b], want)
    assert np.isnan(got[3][3])
    # an empty mask: the chain without the argument
    empty = torch.zeros_like(q["mask"])
    empty[:, 100] = True
    assert denoise(q["pk"], q["model"], q["sched"], q["tr"], True, known_mask=empty, **kw)[2:] == base[2:]
    # eager equals graph, seeded and with injected uniforms, diverse and argmax
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        graph = denoise(q["pk"], q["model"], q["sched"], q["tr"], True, known_mask=q["mask"], use_graph=True, **kw)
    assert not [str(w.message) for w in caught if "HIP-graph capture" in str(w.message)]
    assert graph[2] == got[2] and [repr(r) for r in graph[3]] == [repr(r) for r in got[3]]
    g = torch.Generator().manual_seed(4)
    x_T = torch.nn.functional.one_hot(torch.randint(0, 20, (B_CHAIN, 128), generator=g), 20).float()
    us = [torch.rand(B_CHAIN, 128, generator=g) for _ in range(T)]
    kus = [torch.rand(B_CHAIN, 128, generator=g) for _ in range(T)]
    for diverse in (True, False):
        inj = dict(timesteps=T, x_T=x_T, known_mask=q["mask"], **(dict(us=us, known_us=kus) if diverse else {}))
        e = denoise(q["pk"], q["model"], q["sched"], q["tr"], diverse, use_graph=False, **inj)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            r = denoise(q["pk"], q["model"], q["sched"], q["tr"], diverse, use_graph=True, **inj)
        assert e[2] == r[2]
        for b in range(B_CHAIN):
            assert all(e[2][b][c] == e[1][b][c] for c in (1, 2, 3) if c < q["lengths"][b])
    # the three frames and another batch order: the allowance of test_sequence_chain_draws_follow_the_item, no more
    packed = denoise(q["pk"], q["model"], q["sched"], q["tr"], True, known_mask=q["mask"], pack=True, **kw)
    assert packed[2] == got[2] and [repr(r) for r in packed[3]] == [repr(r) for r in got[3]]
    trim = denoise(q["pk"], q["model"], q["sched"], q["tr"], True, known_mask=q["mask"], trim_padding=True, **kw)
    assert trim[2] == got[2]
    rev_pk = {k: (v.flip(0) if torch.is_tensor(v) else v) for k, v in q["pk"].items()}
    rev = denoise(rev_pk, q["model"], q["sched"], q["tr"], True, known_mask=q["mask"].flip(0), timesteps=T, seed=5,
                  item_ids=IDS[::-1])
    assert rev[2][::-1] == got[2] and rev[1][::-1] == got[1]


# ------------------------------------------------------------------------------------------------ entry point
def test_structure_entry_point_holds_the_native_angles(pkg, hip, tmp_path, monkeypatch):
    from e3diff_amd import biolip
    from e3diff_amd.bert import BertConfig
    from e3diff_amd.structure_model import sample as S
    from e3diff_amd.structure_model.dataset import LigandBindingSiteDataset, NoisedAnglesDataset
    from e3diff_amd.structure_model.model import ConditionalBertForDiffusion as M
    path = biolip.write_synthetic(str(tmp_path / "biolip.pt"), 3, seed=4)
    L = 64
    ds = NoisedAnglesDataset(LigandBindingSiteDataset(path, None, L, 0), timesteps=5)
    c = dict(hidden_size=768, num_attention_heads=12, intermediate_size=1024, num_hidden_layers=2,
             max_position_embeddings=L, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    torch.manual_seed(3)
    model = M(BertConfig(**c), BertConfig(**c, is_decoder=True, add_cross_attention=True),
              feature_names=ds.feature_names, loss_func=[M.diheral_loss_func] * 8).eval().to(DEV)
    monkeypatch.setitem(S.CONFIG, "batch_size", 3)
    free = S.sample(model, ds, seed=31)
    monkeypatch.setenv("E3D_SAMPLE_KEEP", "0-2")
    monkeypatch.setattr(S, "KEEP", "0-2")                            # the module reads the variable when it is imported
    kept = S.sample(model, ds, seed=31)
    assert len(kept) == len(free) == 3
    for i, (a, f) in enumerate(zip(kept, free)):
        native = ds[i]["ligand_angles"][:a.shape[1]].numpy()
        assert a.shape == f.shape and a.shape[0] == 5 and a.shape[1] >= 3 and np.isfinite(a).all()
        assert np.array_equal(a[-1, :3], native[:3]), i
        assert not np.array_equal(a[-1, 3:], native[3:]) and not np.array_equal(a[-1], f[-1])
        assert not np.array_equal(a[0, :3], native[:3])              # on the way the held residues carry their level's noise
    # the keyword wins over the variable; a callable picks per dataset index
    by_kw = S.sample(model, ds, seed=31, keep=lambda i: torch.arange(L) == i)
    for i, a in enumerate(by_kw):
        native = ds[i]["ligand_angles"][:a.shape[1]].numpy()
        assert np.array_equal(a[-1, i], native[i]) and not np.array_equal(a[-1, :3], native[:3])
    with pytest.raises(ValueError, match="'x'"):
        S.sample(model, ds, seed=31, keep="0-2,x")
