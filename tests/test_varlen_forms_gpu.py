"""GPU: the varlen attention kernel (csrc/attn_varlen.hip, ``attn_varlen_kernel``, entry point ``e3d_attn_varlen_fwd``,
wrapper ``ops.attention_varlen``) in every branch, against the fp64 statement of tests/varlen_ref.py, at the segment
edges where its tiling can go wrong.  tests/test_attention_edges_gpu.py covers the padded kernels only; the three kernel
tests of tests/test_packed_gpu.py run one shape (nh = 12, P = 256).

Branches (K = csrc/attn_varlen.hip, F = csrc/attn_split_frag.h) and the test that reaches each:

======  ====================================================  ==========================================================
line    branch / condition                                    reached by
======  ====================================================  ==========================================================
K30     ``unit >= n_units``: an idle wave beside working ones test_self_relkey[P16] (18 units), [P33] (7), cross packed (27)
K32     ``h = unit % nh``, ``entry = unit / nh``, nh % 4 != 0 every test: nh = 1, 3, 5; one workgroup spans entries
K36     ``seg < 0``: tail entry, zero rows                    every packed case but [P96]; with segment entries in one
                                                              workgroup [P33]; alone test_only_tail_layout
K40     ``row < out_rows`` false in the last tail block       test_guarded_direct_calls (rows behind ``out_rows`` stay NaN)
K47     ``Lk <= 0``: queries without keys, zero rows          test_cross[*] (item 5), test_guarded_direct_calls[cross-*]
K48     ``q0 + qi < Lq`` in that branch                       the same (5 rows of a 32-row tile)
K56     ``lq = min(q0 + qi, Lq - 1)``: partial query tile     every case (lengths 1, 3, 5, 7, 13, 31, 33, 97 ...)
K70     ``RELKEY`` true / false                               test_self_relkey / test_cross
K72     first table block: fast / clamped HIGH (q0 > P - 33)  fast [P256], [P64] q0 = 0; high every other rel-key case
K85     key tile: fast / clamped to ``Lk - 1``                full tiles [P96], [P64]; partial last tile everywhere else
K86     table block in the k loop: fast / clamped LOW         low [P16] [P33] [P40] [P100]; fast only [P64] [P96] [P256]
        (P % 32 != 0 and Lk > 32 (P // 32))
K87     ``-inf`` bias on keys behind ``Lk``                   every partial key tile; Lk = 1: test_self_relkey[P16|P33|P256], cross
K99     ring rotation ``rot ^= 32``, 1 / 2 / 3 / 4 key tiles  [P96] 1, 2, 3; [P33] 2; [P100] 4; cross 1, 2, 3
K112    ``v_load``: fast / gathered rows (F121)               as K85; 8-byte V rows (v_rs % 4 == 2) test_cross
K157    ``q0 + qi < Lq`` at the store                         every partial query tile; test_guarded_direct_calls
K179    launch ``<NS, true>`` / ``<NS, false>``               test_self_relkey / test_cross
K213    ``terms`` 19 / 3 / else (6 and 0)                     every test: f16x3, bf16x3, bf16x6 and f32
ops     ``torch.zeros`` for a padded-frame query layout       test_cross[padded_queries_and_keys],
                                                              test_placement_independence, the contract test
ops     ``n_tiles == 0`` returns the zero buffer              test_only_tail_layout (padded frame of empty segments)
======  ====================================================  ==========================================================

``E3D_REQUIRE`` lines of ``e3d_attn_varlen_fwd``:

======  ====================================================  ==========================================================
K195    null pointer                                          tests/test_packed_cpu.py (no device memory needed)
K196    nh, n_tiles, out_rows > 0                             test_host_refusals: n_tiles = 0, out_rows = 0
K198    row strides: % 4 (q, k), % 2 (v), >= nh x 64          test_host_refusals: q_rs = H + 2, k_rs = H - 4, v_rs = H + 1
K200    16-byte pointers                                      test_host_refusals: q at + 4 bytes
K202    terms in {0, 3, 6, 19}                                test_host_refusals: terms = 5
K204    max_k_len x row stride < 2^30                         test_host_refusals: max_k_len as a scalar only
K206    n_tiles x nh < 2^30                                   not run: without the check the launch would read past the
                                                              tile table (no refusal test may depend on its own check)
K208    rel-key: lengths <= P                                 test_host_refusals: max_q_len = P + 1 as a scalar only
K210    rel-key: 16-byte table                                test_host_refusals: dist_emb at + 4 bytes
======  ====================================================  ==========================================================

Every broken argument of test_host_refusals stays inside the test's own allocations even if its check were missing.

Checks.  Every mode (f32 runs the bf16x6 form here) with the bounds of tests/test_packed_gpu.py -- ``rel_err`` below 1e-5,
1e-5, 1e-4 (bf16x3), 1e-5 -- over all segment rows and, per segment, 4x the bound against that segment's own max |ref|
(varlen_ref.figures).  Inputs hold NaN in every row of no segment and in every stride gap; through the op, rows of no
segment must be exactly 0 (a NaN-filled tensor of the output's size is allocated and freed first, so that a stale zero
page cannot pass); through the C entry point ``out`` is NaN-prefilled with 64 guard rows: the packed tail must be exactly
0, rows of no segment of a padded-frame query layout and the guard rows still NaN.

Placement.  One segment computes the same bits alone, among others and in a padded frame: each (tile, head) is one wave's
work on the same values in the same order -- no atomics, no cross-wave sums.

Contract at large scores.  The kernel gives absent keys weight 0 (K87); the reference's additive -10000 mask lets padded
keys win rows once a row's scores spread over more than ~9900.  test_packed_path_computes_the_absent_keys_softmax_...
pins the former and shows the two apart.

Measured on an MI355X, largest figure per mode f32 / bf16x6 / bf16x3 / f16x3 (f32 runs the bf16x6 form: equal bits):
  test_self_relkey, all rows [1e-5 / 1e-5 / 1e-4 / 1e-5]      4.8e-7 / 4.8e-7 / 7.4e-6 / 3.9e-7   ([P96], [P96], [P256], [P100])
  test_self_relkey, per segment [4e-5 / 4e-5 / 4e-4 / 4e-5]   6.1e-7 / 6.1e-7 / 9.0e-6 / 5.1e-7
  test_cross, all rows (the three layouts: equal bits)        1.9e-7 / 1.9e-7 / 5.8e-6 / 1.5e-7
  test_cross, per segment                                     3.9e-7 / 3.9e-7 / 1.1e-5 / 3.5e-7
  test_sharp_softmax_rows [2e-4 / 2e-4 / 4e-3 / 2e-4]         5.6e-6 / 5.6e-6 / 4.5e-4 / 5.6e-6
  contract, against absent keys [2e-3 / 2e-3 / 5e-2 / 2e-3]   7.4e-8 / 7.4e-8 / 4.1e-6 / 9.0e-8;  against the additive mask 1.25
The closest to its bound is the sharp case in bf16x3, at 0.11 of it.  Every test prints its figures; the file runs in 3 s.
"""
import pytest
import torch

import varlen_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                   # NaN rows behind every output of a direct call
IN_GUARD = 8                 # NaN rows behind every input of a direct call
MODES = R.MODES


# ----------------------------------------------------------------------------------------------------- buffers
def _qkv(inp, lay, guard=0):
    """Fused [rows + guard, 3H] buffer: the segments at the layout's rows, NaN everywhere else."""
    buf = R.nan_rows(lay.rows + guard, 3 * inp.H)
    for i, segs in enumerate((inp.q, inp.k, inp.v)):
        R.place(buf, segs, lay.starts, i * inp.H)
    d = buf.to(DEV)
    H, n = inp.H, lay.rows
    return d, (d[:n, :H], d[:n, H:2 * H], d[:n, 2 * H:])


def _separate(inp, q_lay, k_lay, guard=0):
    """q, k and v in three buffers of row strides H + 4, H + 8, H + 2 (NaN in the gaps and in every row of no segment)."""
    bufs, views = [], []
    for name, segs, lay in (("q", inp.q, q_lay), ("k", inp.k, k_lay), ("v", inp.v, k_lay)):
        d = R.place(R.nan_rows(lay.rows + guard, inp.H + R.CROSS_PAD[name]), segs, lay.starts).to(DEV)
        assert d.data_ptr() % 16 == 0
        bufs.append(d)
        views.append(d[:lay.rows, :inp.H])
    assert len({v.stride(0) for v in views}) == 3 and views[2].stride(0) % 4 == 2
    return bufs, tuple(views)


def _member(lay):
    """bool [rows]: the row belongs to a segment."""
    m = torch.zeros(lay.rows, dtype=torch.bool)
    for at, n in zip(lay.starts, lay.lengths):
        m[at:at + n] = True
    return m


def _poison(rows, width):
    """Leave NaN in the block the allocator hands out next for a [rows, width] tensor."""
    t = torch.full((rows, width), R.NAN, device=DEV)
    torch.cuda.synchronize()
    del t


def _op(pkg, views, q_lay, k_lay, inp, mode):
    _poison(q_lay.rows, inp.H)
    with torch.no_grad():
        out = pkg.ops.attention_varlen(*views, q_lay, k_lay, inp.nh, dist_emb=None if inp.E is None else inp.E.to(DEV),
                                       max_pos=inp.P, mode=mode)
    assert out.shape == (q_lay.rows, inp.H)
    return out


def _op_figures(out, q_lay, inp, tol, what):
    out = out.cpu()
    assert bool((out[~_member(q_lay)] == 0).all()), f"{what}: a row of no segment is not exactly zero"
    return R.figures(R.cut(out, q_lay.starts, q_lay.lengths), inp.ref, tol, what)


def _bits(t):
    return t.view(torch.int32).clone()


class _Call:
    """The arguments of one ``e3d_attn_varlen_fwd`` call on (views of) the test's own buffers; ``run(name=value)`` breaks
    chosen ones."""
    ORDER = ("q", "q_rs", "k", "k_rs", "v", "v_rs", "q_start", "q_len", "k_start", "k_len", "tiles", "n_tiles", "dist_emb",
             "P", "out", "out_rows", "nh", "max_q_len", "max_k_len", "terms", "stream")

    def __init__(self, pkg, lib, views, q_lay, k_lay, inp):
        self.pkg, self.lib, self.q_lay = pkg, lib, q_lay
        q, k, v = views
        self.E = None if inp.E is None else torch.cat([inp.E, R.nan_rows(1, R.D)]).to(DEV)     # (a spare row behind the table)
        self.out = torch.full((q_lay.rows + GUARD, inp.H), R.NAN, device=DEV)
        self.keep = (views, q_lay, k_lay)
        self.args = dict(q=q.data_ptr(), q_rs=q.stride(0), k=k.data_ptr(), k_rs=k.stride(0), v=v.data_ptr(), v_rs=v.stride(0),
                         q_start=q_lay.start_dev.data_ptr(), q_len=q_lay.len_dev.data_ptr(),
                         k_start=k_lay.start_dev.data_ptr(), k_len=k_lay.len_dev.data_ptr(), tiles=q_lay.tiles.data_ptr(),
                         n_tiles=q_lay.n_tiles, dist_emb=pkg.ops._p(self.E), P=inp.P, out=self.out.data_ptr(),
                         out_rows=q_lay.rows, nh=inp.nh, max_q_len=q_lay.max_len, max_k_len=k_lay.max_len, terms=6,
                         stream=torch.cuda.current_stream().cuda_stream)
        assert tuple(self.args) == self.ORDER

    def run(self, **broken):
        a = dict(self.args, **broken)
        rc = self.lib.e3d_attn_varlen_fwd(*(a[n] for n in self.ORDER))
        torch.cuda.synchronize()
        return rc

    def refill(self):
        self.out.fill_(R.NAN)


def _guarded_figures(call, inp, tol, what):
    """After a direct call: segments against fp64, the packed tail exactly 0, every other row still NaN."""
    lay, out = call.q_lay, call.out.cpu()
    member = _member(lay)
    loose = out[:lay.rows][~member]
    if lay.padded_frame:
        assert bool(torch.isnan(loose).all()), f"{what}: a row of no segment of the padded query frame was written"
    else:
        assert bool((loose == 0).all()), f"{what}: the packed tail is not exactly zero"
    assert bool(torch.isnan(out[lay.rows:]).all()), f"{what}: written behind out_rows"
    return R.figures(R.cut(out, lay.starts, lay.lengths), inp.ref, tol, what)


# ----------------------------------------------------------------------------------------------------- cases
@pytest.mark.parametrize("case", R.RELKEY_CASES, ids=lambda c: c.name)
def test_self_relkey(pkg, hip, case):
    """Rel-key self-attention on views of one fused qkv buffer, ``q_layout is k_layout``."""
    inp = R.relkey_inputs(case)
    lay = pkg.packing.PackedLayout(case.lengths, case.P, DEV)
    _, views = _qkv(inp, lay)
    figs = []
    for mode, tol in MODES:
        figs += _op_figures(_op(pkg, views, lay, lay, inp, mode), lay, inp, tol, f"{case.name} {mode}")
    R.report(figs)


def _cross_layouts(pkg, name):
    q_padded, k_padded = R.CROSS_LAYOUTS[name]
    P = pkg.packing.PackedLayout
    return P(R.CROSS_Q, R.CROSS_FRAME, DEV, padded_frame=q_padded), P(R.CROSS_K, R.CROSS_FRAME, DEV, padded_frame=k_padded)


@pytest.mark.parametrize("name", list(R.CROSS_LAYOUTS))
def test_cross(pkg, hip, name):
    """No table; q, k and v in three buffers of pairwise different row strides (v rows 8-byte aligned only).  Item 5 has
    queries and no keys: its rows are exactly zero (varlen_ref.figures) and its key rows -- NaN, or none at all -- are
    never read; item 1 has keys and no queries.  In the padded query frame the rows of no segment are exactly 0."""
    inp = R.cross_inputs()
    q_lay, k_lay = _cross_layouts(pkg, name)
    _, views = _separate(inp, q_lay, k_lay)
    figs = []
    for mode, tol in MODES:
        figs += _op_figures(_op(pkg, views, q_lay, k_lay, inp, mode), q_lay, inp, tol, f"{name} {mode}")
    R.report(figs)


@pytest.mark.parametrize("name", ["relkey-P40"] + ["cross-" + n for n in R.CROSS_LAYOUTS])
def test_guarded_direct_calls(pkg, hip, name):
    """``e3d_attn_varlen_fwd`` on buffers of the test's own: NaN-prefilled ``out`` with 64 guard rows, inputs with NaN in
    every row of no segment (tail, padding, 8 guard rows)."""
    if name.startswith("relkey"):
        case = R.RELKEY_BY_NAME[name[7:]]
        inp = R.relkey_inputs(case)
        q_lay = k_lay = pkg.packing.PackedLayout(case.lengths, case.P, DEV)
        bufs, views = _qkv(inp, q_lay, IN_GUARD)
    else:
        inp = R.cross_inputs()
        q_lay, k_lay = _cross_layouts(pkg, name[6:])
        bufs, views = _separate(inp, q_lay, k_lay, IN_GUARD)
    call = _Call(pkg, hip, views, q_lay, k_lay, inp)
    figs = []
    for mode, tol in MODES:
        call.refill()
        pkg.hip.check(call.run(terms=pkg.ops.GEMM_MODES[mode]), "e3d_attn_varlen_fwd")
        figs += _guarded_figures(call, inp, tol, f"{name} {mode}")
    R.report(figs)


def test_only_tail_layout(pkg, hip):
    """``PackedLayout([0, 0], 32)``: 32 rows, one tail entry, no segment -- 32 zero rows, whatever the (NaN) inputs hold,
    with and without a table, through the op and through the entry point.  A padded frame of empty segments has no tile
    at all: the op returns zeros without a launch."""
    nh, P = 3, 32
    H = nh * 64
    lay = pkg.packing.PackedLayout([0, 0], P, DEV)
    assert (lay.rows, lay.n_tiles, lay.total) == (32, 1, 0) and lay.tiles.tolist() == [[-1, 0]]
    inp = R.Inputs([torch.zeros(0, H)] * 2, [torch.zeros(0, H)] * 2, [torch.zeros(0, H)] * 2, nh, torch.randn(2 * P - 1, 64), P)
    d, views = _qkv(inp, lay, IN_GUARD)
    before = _bits(d)
    for mode, _ in MODES:
        for E in (inp.E, None):
            inp.E = E
            out = _op(pkg, views, lay, lay, inp, mode)
            assert out.shape == (32, H) and bool((out == 0).all()), (mode, E is None)
    inp.E = None
    call = _Call(pkg, hip, views, lay, lay, inp)
    pkg.hip.check(call.run(), "e3d_attn_varlen_fwd")
    assert bool((call.out[:32] == 0).all()) and bool(torch.isnan(call.out[32:]).all())
    assert torch.equal(_bits(d), before)
    frame = pkg.packing.PackedLayout([0, 0], P, DEV, padded_frame=True)
    assert frame.n_tiles == 0 and frame.rows == 64
    fd = torch.full((64, 3 * H), R.NAN, device=DEV)
    out = _op(pkg, (fd[:, :H], fd[:, H:2 * H], fd[:, 2 * H:]), frame, frame, inp, "bf16x6")
    assert out.shape == (64, H) and bool((out == 0).all())


@pytest.mark.parametrize("mode,tol", MODES)
def test_placement_independence(pkg, hip, mode, tol):
    """One 33-row segment (rel-key, P = 40, nh = 3) alone, as the third of five packed segments and in a padded frame;
    each twice.  Bit-identical everywhere."""
    c = R.PLACEMENT
    one = R.placement_inputs()
    q1, k1, v1 = one.q[0], one.k[0], one.v[0]
    mk = pkg.packing.PackedLayout

    def run(lengths, at, padded=False):
        others = R.Inputs.randn(lengths, lengths, c["nh"], seed=50 + len(lengths))
        others.q[at], others.k[at], others.v[at], others.E, others.P = q1, k1, v1, one.E, c["P"]
        lay = mk(lengths, c["P"], DEV, padded_frame=padded)
        _, views = _qkv(others, lay)
        first, second = (_op(pkg, views, lay, lay, others, mode) for _ in range(2))
        assert torch.equal(first, second), "two consecutive calls differ"
        return first[lay.starts[at]:lay.starts[at] + c["L"]]

    alone = run([c["L"]], 0)
    packed = run(c["packed"], c["at_packed"])
    framed = run(c["frame"], c["at_frame"], padded=True)
    R.report(R.figures([alone.cpu()], one.ref, tol, f"alone {mode}"))
    assert torch.equal(alone, packed), "alone against third of five packed segments"
    assert torch.equal(alone, framed), "alone against the padded frame"


def test_sharp_softmax_rows(pkg, hip):
    """The construction of test_attention_sharp_softmax_rows_match_fp64 on segments: Q, K x 16, scores of std ~256, rows
    all but one-hot (tests/test_varlen_ref_cpu.py: 97 % of the rows above 0.99, no tie at the top).  A score carries an
    absolute error of ~|s| 2^-24 (fp32 grade) or ~|s| 2^-17 (bf16x3), the relative error of its probability: the bounds of
    that test, 2e-4 and 4e-3."""
    c = R.SHARP
    inp = R.sharp_inputs()
    lay = pkg.packing.PackedLayout(c["lengths"], c["P"], DEV)
    _, views = _qkv(inp, lay)
    figs = []
    for mode, _ in MODES:
        out = _op(pkg, views, lay, lay, inp, mode).cpu()
        assert bool((out[lay.total:] == 0).all())
        figs.append((f"sharp {mode}", R.rel_err(torch.cat(R.cut(out, lay.starts, lay.lengths)), torch.cat(inp.ref)), R.SHARP_TOL[mode]))
    R.report(figs)


def test_packed_path_computes_the_absent_keys_softmax_where_the_reference_lets_padded_keys_win(pkg, hip):
    """THE PACKED PATH'S CONTRACT, and where it departs from the reference.  Keys outside a segment do not exist for its
    rows: weight exactly 0, whatever they hold.  The reference model masks additively (-10000), so once a row's scores
    spread over more than ~9900 its padded keys win the row
    (test_attention_padded_keys_reach_the_softmax_when_scores_exceed_the_mask pins the padded kernels to that).  Here
    that test's construction sits in a padded [2, 64] frame with prefix lengths [16, 64]; the padding rows of the short
    item hold keys that lead by ~6000 under the additive mask.  The varlen kernel must match the absent-keys fp64
    statement within that test's bounds (2e-3; 5e-2 for bf16x3) and differ from the additive-mask statement by more than
    0.1: packed, and trimmed, chains equal the padded one only below that spread (packing.Frame)."""
    inp, (qf, kf, vf) = R.contract_case()
    L, lens = R.CONTRACT["L"], R.CONTRACT["lengths"]
    H = inp.H
    lay = pkg.packing.PackedLayout(lens, L, DEV, padded_frame=True)
    d = torch.cat([qf, kf, vf], -1).reshape(len(lens) * L, 3 * H).to(DEV)                  # padding rows included
    valid = lambda x: torch.cat([x.reshape(len(lens), L, H)[b, :n] for b, n in enumerate(lens)])  # noqa: E731
    additive = valid(R.additive_mask_statement(qf, kf, vf, lens, inp.nh, inp.E, inp.P))
    absent = torch.cat(inp.ref)
    assert R.rel_err(absent, additive) > 0.1
    figs = []
    for mode, _ in MODES:
        out = _op(pkg, (d[:, :H], d[:, H:2 * H], d[:, 2 * H:]), lay, lay, inp, mode).cpu()
        assert bool((out[~_member(lay)] == 0).all())
        got = valid(out)
        figs.append((f"contract {mode}: against absent keys", R.rel_err(got, absent), R.CONTRACT_TOL[mode]))
        apart = R.rel_err(got, additive)
        print(f"contract {mode}: against the additive mask {apart:.3f} (> 0.1)")
        assert apart > 0.1, mode
    R.report(figs)


# ----------------------------------------------------------------------------------------------------- refusals
def test_host_refusals(pkg, hip):
    """Every refused call returns non-zero with the message of its check and leaves the NaN-filled output untouched.  The
    buffers are real and roomy: each broken argument would stay inside them if its check were missing."""
    lib = hip
    inp = R.cross_inputs()
    q_lay, k_lay = _cross_layouts(pkg, "packed")
    _, views = _separate(inp, q_lay, k_lay, IN_GUARD)
    cross = _Call(pkg, lib, views, q_lay, k_lay, inp)
    case = R.RELKEY_BY_NAME["P40"]
    rinp = R.relkey_inputs(case)
    lay = pkg.packing.PackedLayout(case.lengths, case.P, DEV)
    _, rviews = _qkv(rinp, lay, IN_GUARD)
    relkey = _Call(pkg, lib, rviews, lay, lay, rinp)
    H, a = inp.H, cross.args
    broken = [
        (cross, dict(q_rs=H + 2), b"row strides"),                              # q_rs % 4 != 0
        (cross, dict(k_rs=H - 4), b"row strides"),                              # k_rs < nh * 64
        (cross, dict(v_rs=H + 1), b"row strides"),                              # v_rs odd
        (cross, dict(q=a["q"] + 4), b"pointers must be 16B"),
        (cross, dict(terms=5), b"terms must be"),
        (cross, dict(n_tiles=0), b"bad shape"),
        (cross, dict(out_rows=0), b"bad shape"),
        (cross, dict(max_k_len=(1 << 30) // a["k_rs"] + 1), b"2^30"),           # a scalar only: the kernel never sees it
        (relkey, dict(max_q_len=case.P + 1), b"relative_key needs"),            # a scalar only
        (relkey, dict(dist_emb=relkey.args["dist_emb"] + 4), b"dist_emb must be 16B"),
    ]
    for call, bad, message in broken:
        rc = call.run(**bad)
        assert rc != 0 and message in lib.e3d_last_error(), (bad, rc, lib.e3d_last_error())
        assert bool(torch.isnan(call.out).all()), bad
    for call in (cross, relkey):                                                # the unbroken calls are accepted
        pkg.hip.check(call.run(), "e3d_attn_varlen_fwd")
        assert bool(torch.isfinite(call.out[:call.q_lay.total]).all())
    # through the op
    q, k, v = views
    with torch.no_grad():
        with pytest.raises(ValueError, match="rows q"):
            pkg.ops.attention_varlen(q[:-1], k, v, q_lay, k_lay, inp.nh)
        with pytest.raises(ValueError, match="rows q"):
            pkg.ops.attention_varlen(q, k, v[:-32], q_lay, k_lay, inp.nh)
        more = pkg.packing.PackedLayout(R.CROSS_K + [3], R.CROSS_FRAME, DEV)
        assert more.rows == k_lay.rows and more.B == k_lay.B + 1
        with pytest.raises(ValueError, match="query segments against"):
            pkg.ops.attention_varlen(q, k, v, q_lay, more, inp.nh)
