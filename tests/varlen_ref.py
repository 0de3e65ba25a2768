"""The varlen attention kernel (csrc/attn_varlen.hip, ``ops.attention_varlen``) stated plainly: the cases
tests/test_varlen_forms_gpu.py runs, their inputs, the fp64 statement of one segment, the additive-mask statement of the
padded frame it is compared with on the CPU, mirrors of the host arithmetic that decides which kernel branch a case
reaches, and the error figures both test modules use.

Statement.  Segment s: out = softmax((q k^T + relkey) / 8) v over the segment's OWN keys, the rel-key term
``oracle.bert.relkey_scores_literal`` with positions measured from the segment start.  A segment without keys gives zero
rows.  Rows of no segment are zero (a packed buffer's tail) or stay as they were (a padded-frame query layout).

The reference model masks additively instead: softmax over the whole padded frame of (scores / 8 - 10000 on padded keys).
While a row's scores spread over less than ~9900 the two agree to fp64 rounding (exp(-10000 + spread) underflows to 0);
beyond that padded keys win rows of the additive statement and the two part (``contract_case``).
tests/test_varlen_ref_cpu.py asserts both.

Figures.  ``figures`` gives the project's ``rel_err`` over all segment rows against the mode's bound (``MODES``, the bounds
of tests/test_packed_gpu.py) and, per segment, max |got - ref| / max |ref of that segment| against 4x the bound -- the
per-block rule of tests/test_gemm_forms_gpu.py: a segment with small outputs cannot hide behind one with large ones.
"""
import torch

from oracle import bert as obert

F64 = torch.float64
NAN = float("nan")
D = 64
TILE = 32
MODES = (("f32", 1e-5), ("bf16x6", 1e-5), ("bf16x3", 1e-4), ("f16x3", 1e-5))      # tests/test_packed_gpu.MODES
SEGMENT_FACTOR = 4                                                                   # tests/test_gemm_forms_gpu.py, per block
# tests/test_kernels_gpu.py: test_attention_sharp_softmax_rows_match_fp64 / ..._padded_keys_reach_the_softmax_...
SHARP_TOL = {"f32": 2e-4, "bf16x6": 2e-4, "f16x3": 2e-4, "bf16x3": 4e-3}
CONTRACT_TOL = {"f32": 2e-3, "bf16x6": 2e-3, "f16x3": 2e-3, "bf16x3": 5e-2}


# ----------------------------------------------------------------------------------------------------- cases
class RelkeyCase:
    """Self-attention with the rel-key table [2P - 1, 64]; ``low`` / ``high``: a table block of the case starts below
    row 0 / ends above row 2P - 2 (marked by hand; tests/test_varlen_ref_cpu.py computes them from ``table_blocks``)."""

    def __init__(self, P, lengths, nh, low, high):
        self.name, self.P, self.lengths, self.nh, self.low, self.high = f"P{P}", P, lengths, nh, low, high


RELKEY_CASES = [
    RelkeyCase(16, [16, 1, 7, 16, 0, 3], 3, True, True),       # every block clamped; empty segment; units % 4 != 0
    RelkeyCase(33, [33, 32, 1, 33], 1, True, True),            # low clamp at r0 = 32; 2 key tiles; tail shares a workgroup
    RelkeyCase(40, [40, 31, 0, 0, 34], 5, True, True),         # adjacent empty segments
    RelkeyCase(100, [97, 100, 5], 3, True, True),              # low clamp at r0 = 96; 4 key tiles; 3 query tiles
    RelkeyCase(64, [64, 33, 64], 1, False, True),              # P % 32 == 0: high clamp only; total 161
    RelkeyCase(256, [5, 40, 1], 5, False, False),              # no clamp: the fast path of every table load
    RelkeyCase(96, [96, 32, 64], 3, False, True),              # total % 32 == 0: no tail entry; 1, 2, 3 key tiles
]
RELKEY_BY_NAME = {c.name: c for c in RELKEY_CASES}

CROSS_Q = [1, 0, 33, 32, 70, 5]
CROSS_K = [70, 9, 1, 64, 31, 0]            # the last item: queries and no keys; the second: keys and no queries
CROSS_NH = 3
CROSS_FRAME = 96                           # L of a padded query frame, Lr of a padded key frame
CROSS_PAD = {"q": 4, "k": 8, "v": 2}       # row stride - nh * 64: v rows are 8-byte, not 16-byte, aligned
CROSS_LAYOUTS = {"packed": (False, False), "padded_keys": (False, True), "padded_queries_and_keys": (True, True)}

PLACEMENT = dict(P=40, L=33, nh=3, packed=[5, 40, 33, 0, 17], frame=[7, 33, 20], at_packed=2, at_frame=1)
SHARP = dict(P=64, lengths=[64, 13, 40], nh=3, scale=16.0, seed=22)   # the seed: test_varlen_ref_cpu.py
CONTRACT = dict(L=64, lengths=[16, 64], nh=3)


# ----------------------------------------------------------------------------------------------------- host arithmetic
def layout(lengths, L, padded_frame=False):
    """packing.PackedLayout's (starts, rows, total): segments back to back and rows rounded up to 32 (at least 32), or
    segment s at row s * L of a [B, L] frame."""
    total = sum(lengths)
    if padded_frame:
        return [s * L for s in range(len(lengths))], len(lengths) * L, total
    starts = [sum(lengths[:s]) for s in range(len(lengths))]
    return starts, max(TILE, -(-total // TILE) * TILE), total


def table_blocks(P, L):
    """First rows of the 32-row distance-table blocks a segment of L rows loads: per query tile q0 the block above the
    diagonal (``q0 + 1 + P - 1``, before the k loop) and one per key tile r0 (``q0 - r0 - 31 + P - 1``)."""
    blocks = []
    for q0 in range(0, L, TILE):
        blocks.append(q0 + P)
        blocks += [q0 - r0 - 32 + P for r0 in range(0, L, TILE)]
    return blocks


def clamps(P, lengths):
    """(a block starts below row 0, a block ends above row 2P - 2): ``tile_load`` then takes its per-row clamp path."""
    blocks = [b for L in lengths for b in table_blocks(P, L)]
    return any(b < 0 for b in blocks), any(b + TILE - 1 > 2 * P - 2 for b in blocks)


def units(q_lengths, nh, padded_frame=False):
    """(tile entries, waves with work, workgroups): one wave per (entry, head), 4 waves per workgroup."""
    _, rows, total = layout(q_lengths, 0, padded_frame)
    entries = sum(-(-n // TILE) for n in q_lengths) + (0 if padded_frame else len(range(total, rows, TILE)))
    return entries, entries * nh, -(-entries * nh // 4)


# ----------------------------------------------------------------------------------------------------- inputs
def gen(seed):
    return torch.Generator().manual_seed(seed)


class Inputs:
    """Per segment q [nq, H], k and v [nk, H] (fp32, CPU), the table E [2P - 1, 64] or None, and -- computed once,
    never changed -- the fp64 statement of every segment (``ref``)."""

    def __init__(self, q, k, v, nh, E=None, P=0):
        self.q, self.k, self.v, self.nh, self.E, self.P = q, k, v, nh, E, P
        self.H = nh * D
        self.q_lengths, self.k_lengths = [len(x) for x in q], [len(x) for x in k]
        self._ref = None

    @classmethod
    def randn(cls, q_lengths, k_lengths, nh, P=0, seed=0, qk_scale=1.0):
        g, H = gen(seed), nh * D
        q = [torch.randn(n, H, generator=g) * qk_scale for n in q_lengths]
        k = [torch.randn(n, H, generator=g) * qk_scale for n in k_lengths]
        v = [torch.randn(n, H, generator=g) for n in k_lengths]
        return cls(q, k, v, nh, torch.randn(2 * P - 1, D, generator=g) if P else None, P)

    @property
    def ref(self):
        if self._ref is None:
            self._ref = [segment_statement(q, k, v, self.nh, self.E, self.P) for q, k, v in zip(self.q, self.k, self.v)]
        return self._ref


_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def relkey_inputs(case):
    return _once(case.name, lambda: Inputs.randn(case.lengths, case.lengths, case.nh, case.P, seed=100 + case.P))


def cross_inputs():
    return _once("cross", lambda: Inputs.randn(CROSS_Q, CROSS_K, CROSS_NH, seed=7))


def placement_inputs():
    c = PLACEMENT
    return _once("placement", lambda: Inputs.randn([c["L"]], [c["L"]], c["nh"], c["P"], seed=41))


def sharp_inputs():
    c = SHARP
    return _once("sharp", lambda: Inputs.randn(c["lengths"], c["lengths"], c["nh"], c["P"], c["seed"], c["scale"]))


def contract_case():
    """(Inputs of the valid rows, frames (q, k, v) [B, L, H]): the construction of
    test_attention_padded_keys_reach_the_softmax_when_scores_exceed_the_mask as a padded [B, L] frame with prefix
    lengths.  Queries and PADDED keys share a direction u (q . k / 8 ~ +8192), valid keys point the other way (~ -8192):
    under the additive mask the padded keys lead by ~6000 and win every row of the short item.  Small-integer operands:
    the products are exact in every arithmetic."""
    def make():
        L, lens, nh = CONTRACT["L"], CONTRACT["lengths"], CONTRACT["nh"]
        B, H = len(lens), nh * D
        u = torch.where(torch.rand(D, generator=gen(31)) < 0.5, -1.0, 1.0)
        noise = lambda seed, *shape, sd=8.0: torch.round(torch.randn(*shape, generator=gen(seed)) * sd).clamp(-60, 60)  # noqa: E731
        valid = torch.arange(L)[None] < torch.tensor(lens)[:, None]
        q = (32.0 * u + noise(34, B, L, nh, D)).reshape(B, L, H)
        k = (torch.where(valid[:, :, None, None], -32.0 * u, 32.0 * u) + noise(35, B, L, nh, D)).reshape(B, L, H)
        v = torch.randn(B, L, nh, D, generator=gen(33)).reshape(B, L, H)
        E = noise(36, 2 * L - 1, D, sd=2.0)
        cut = lambda x: [x[b, :n].clone() for b, n in enumerate(lens)]  # noqa: E731
        return Inputs(cut(q), cut(k), cut(v), nh, E, L), (q, k, v)
    return _once("contract", make)


def nan_rows(rows, width):
    return torch.full((rows, width), NAN)


def place(buf, segs, starts, col0=0):
    """Segment s into rows starts[s] .. of ``buf``, columns col0 ..; everything else keeps what it held (NaN)."""
    for x, at in zip(segs, starts):
        buf[at:at + x.shape[0], col0:col0 + x.shape[1]] = x
    return buf


def frames(inp, Lq, Lk, seed=1):
    """Padded frames (q [B, Lq, H], k and v [B, Lk, H]) of ``inp``: the segments first, randn rows as padding (any
    finite padding does: the additive statement gives it weight exp(-10000 + spread))."""
    g, B, H = gen(seed), len(inp.q), inp.H
    out = []
    for segs, L in ((inp.q, Lq), (inp.k, Lk), (inp.v, Lk)):
        f = torch.randn(B * L, H, generator=g)
        out.append(place(f, segs, [b * L for b in range(B)]).reshape(B, L, H))
    return tuple(out)


# ----------------------------------------------------------------------------------------------------- statements
def _heads(x, nh):
    return x.reshape(x.shape[0], -1, nh, D).permute(0, 2, 1, 3).to(F64)            # [B, L, H] -> [B, nh, L, 64]


def segment_statement(q, k, v, nh, E=None, P=0, want_scores=False):
    """q [Lq, H], k and v [Lk, H] -> fp64 [Lq, H] (and the scaled scores [nh, Lq, Lk]); no key: zero rows."""
    Lq, Lk = q.shape[0], k.shape[0]
    if Lq == 0 or Lk == 0:
        out = torch.zeros(Lq, nh * D, dtype=F64)
        return (out, torch.zeros(nh, Lq, Lk, dtype=F64)) if want_scores else out
    qq, kk, vv = _heads(q[None], nh), _heads(k[None], nh), _heads(v[None], nh)
    s = qq @ kk.transpose(-1, -2)
    if E is not None:
        s = s + obert.relkey_scores_literal(qq, E.to(F64), P)
    s = s / 8.0
    out = (torch.softmax(s, -1) @ vv)[0].permute(1, 0, 2).reshape(Lq, nh * D)
    return (out, s[0]) if want_scores else out


def additive_mask_statement(qf, kf, vf, k_lengths, nh, E=None, P=0):
    """The padded frame as the reference model computes it (tests/test_attention_edges_gpu.py, ``Case.reference``):
    (scores + rel-key) / 8 + (1 - mask) * -10000, softmax over the whole frame, @ v.  [B, L, H] in, fp64 [B, Lq, H] out."""
    q, k, v = _heads(qf, nh), _heads(kf, nh), _heads(vf, nh)
    s = q @ k.transpose(-1, -2)
    if E is not None:
        s = s + obert.relkey_scores_literal(q, E.to(F64), P)
    mask = (torch.arange(kf.shape[1])[None] < torch.tensor(k_lengths)[:, None]).to(F64)
    s = s / 8.0 + ((1.0 - mask) * -10000.0)[:, None, None, :]
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(qf.shape[0], qf.shape[1], nh * D)


# ----------------------------------------------------------------------------------------------------- figures
def rel_err(a, b):
    """helpers.rel_err for fp64 references: max |a - b| / max |b|."""
    a, b = a.detach().to(F64).cpu(), b.detach().to(F64).cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def cut(x, starts, lengths):
    """The segments' rows of x [rows, H]."""
    return [x[at:at + n] for at, n in zip(starts, lengths)]


def figures(got, ref, tol, what, segment_factor=SEGMENT_FACTOR):
    """[(what, figure, bound)] of per-segment results ``got`` against ``ref`` (lists of [n, H]): ``rel_err`` over all rows
    against ``tol``, then every segment with rows and a non-zero reference against its own largest |ref| at
    ``segment_factor`` x ``tol``.  A segment whose reference is zero (no keys) must be exactly zero."""
    rows = [s for s, r in enumerate(ref) if r.shape[0]]
    out = [(f"{what} all", rel_err(torch.cat([got[s] for s in rows]), torch.cat([ref[s] for s in rows])), tol)]
    for s in rows:
        if float(ref[s].abs().max()) == 0.0:
            out.append((f"{what} segment {s} (no keys) max |got|", float(got[s].detach().abs().max().cpu()), 1e-45))
        else:
            out.append((f"{what} segment {s}", rel_err(got[s], ref[s]), segment_factor * tol))
    return out


def report(figs):
    """Print every figure, then assert them all (NaN fails: ``not e < bound``)."""
    for what, e, bound in figs:
        print(f"{what}: {e:.3e} ({bound:g})")
    bad = [f for f in figs if not f[1] < f[2]]
    assert not bad, bad
