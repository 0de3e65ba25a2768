"""The batched weight-gradient launches (csrc/gemm_split.hip: e3d_gemm_wgrad_grouped_f32_split, e3d_gemm_wgrad_ragged_f32_split)
stated in fp64, the cases tests/test_wgrad_forms_gpu.py launches, a restatement of both launchers' staging predicate, the
memory layout of a test launch and the comparison.  tests/test_wgrad_ref_cpu.py checks all of it without a GPU.

Statement.  Problem p of a launch over M tokens has dz_p [M, N_p] and x_p [M, K_p] (row strides ldz_p, ldx_p) and writes
    dW_p [N_p, K_p] = dz_p^T x_p        db_p [N_p] = sum_m dz_p[m, :]
each added to what the output held before where accumulate bit p is set; db_p may be absent.  terms = 1 multiplies the
operands rounded to bf16 (round to nearest even), as tests/test_gemm_forms_gpu.py states the plain-bf16 kernels; the column
sums are taken of the fp32 values in every arithmetic.

Kernel cells.  (entry point, NS, TR): NS = bf16 terms per operand (terms 1 -> 1, 3 -> 2, 6 and 19 -> 3), TR = the transposing
float4 / buffer-descriptor staging, chosen by ``grouped_tr`` / ``ragged_tr`` below for the WHOLE launch; its alternative is
the dword staging.  The workgroup tile is 256 (N) x 128 (K) x 32 (tokens); ``nk`` = k-tiles of the reduction.

Bounds.  dW: the GEMM forms file's own -- ``TOL`` of max |ref| and every 32 x 32 block within 4x that of its own largest
|ref|, floored at 1e-3 max |ref|.  db, derived: |got - ref| <= (M + 8) 2^-24 (sum_m |dz[m, n]| + |old|) per column, the worst
case of any fp32 summation order of M terms in eight partials (+ the old contents when accumulating).  The two 2^19-token
launches (``long_reduction_bound``): (M + 64) 2^-24 sum_m |dz| |x| per element plus the arithmetic's TOL max |ref| -- the
forms bounds were never stated for reductions that long, and those launches exist to catch a wrapped descriptor.
"""
import dataclasses
import math

import torch
import torch.nn.functional as F

BM, BN, BK = 256, 128, 32                    # workgroup tile: dW rows (N), dW columns (K), tokens per k-tile
TOL = {1: 5e-6, 3: 3e-5, 6: 5e-6, 19: 5e-6}
NS = {1: 1, 3: 2, 6: 3, 19: 3}
MODES = {1: "bf16", 3: "bf16x3", 6: "bf16x6", 19: "f16x3"}
ENTRIES = ("grouped", "ragged")
NAN = float("nan")
SENTINEL = -7777.25
ZC0, XC0 = 8, 4                              # first column of dz_p / x_p inside its NaN-filled buffer (16-byte aligned)
TAIL = 32                                    # NaN rows after row M - 1 of every input
G_ROWS, G_WORDS = 16, 64                     # guards on each side: rows of a dW block (never under 64 words), words of a db block
F64 = torch.float64


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def ceil4(n):
    return -(-n // 4) * 4


# ----------------------------------------------------------------------------------------------------- problems and cases
@dataclasses.dataclass(frozen=True)
class P:
    """One problem of a launch.  ``ldz`` / ``ldx`` default to whole quads wider than the column block; ``zoff`` / ``xoff``
    move the operand's first column (floats: 1 = a pointer 4 bytes off 16-byte alignment); ``seed`` names the data (default:
    the problem's index in the launch), so the same (N, K, M, seed) is the same data under any stride or offset.  ``positive``:
    operands in [0.5, 1.5) instead of standard normals -- every product counts in the sum, so a reduction that loses rows
    leaves even the wide derived bound of the long reductions."""
    N: int
    K: int
    ldz: int = 0
    ldx: int = 0
    zoff: int = 0
    xoff: int = 0
    bias: bool = True
    acc: bool = False
    seed: int = -1
    positive: bool = False

    def __post_init__(self):
        object.__setattr__(self, "ldz", self.ldz or ceil4(self.N) + 16)
        object.__setattr__(self, "ldx", self.ldx or ceil4(self.K) + 8)

    @property
    def tiles(self):
        return -(-self.N // BM) * -(-self.K // BN)


@dataclasses.dataclass(frozen=True)
class Case:
    """``tr``, ``tiles``, ``nk``: what the case CLAIMS (its id carries them); test_wgrad_ref_cpu.py holds the claims to the
    predicate and the shapes.  ``flip`` = (predicate term, "all" | "first" | "last"): the one term the case turns, alone.
    ``big``: dz lives in the shared 2 GiB buffer (the e3d_tr_span_ok cases)."""
    name: str
    entry: str
    terms: int
    M: int
    probs: tuple
    tr: bool
    tiles: int
    nk: int
    db_null: bool = False
    flip: tuple = None
    big: bool = False

    @property
    def id(self):
        return f"{self.name}-{self.entry}-{MODES[self.terms]}-{'tr' if self.tr else 'dword'}-t{self.tiles}-nk{self.nk}"

    @property
    def cell(self):
        return (self.entry, NS[self.terms], self.tr)

    @property
    def bits(self):
        return sum(1 << i for i, p in enumerate(self.probs) if p.acc)

    def seeded(self):
        return tuple(dataclasses.replace(p, seed=i) if p.seed < 0 else p for i, p in enumerate(self.probs))


# ----------------------------------------------------------------------------------------------------- the launchers' predicate
PREDICATE_TERMS = ("N%4", "K%4", "ldz%4", "ldx%4", "dz+4B", "x+4B", "ld>=2^24", "M*ld*4>=2^31")


def tr_span_ok(k_len, ld):
    """e3d_tr_span_ok: the buffer descriptors of the transposing stager count bytes in 32 bits."""
    return k_len > 0 and 0 < ld < (1 << 24) and k_len * ld * 4 < (1 << 31)


def grouped_tr(M, N, K, ldz, ldx, dz_ptrs, x_ptrs):
    """e3d_gemm_wgrad_grouped_f32_split: one shape, every problem's pointers."""
    tr = N % 4 == 0 and K % 4 == 0 and ldz % 4 == 0 and ldx % 4 == 0 and tr_span_ok(M, ldz) and tr_span_ok(M, ldx)
    return tr and all(a % 16 == 0 and b % 16 == 0 for a, b in zip(dz_ptrs, x_ptrs))


def ragged_tr(M, Ns, Ks, ldzs, ldxs, dz_ptrs, x_ptrs):
    """e3d_gemm_wgrad_ragged_f32_split: ONE problem that is not in whole quads, aligned and in span turns the whole launch."""
    return all(n % 4 == 0 and k % 4 == 0 and lz % 4 == 0 and lx % 4 == 0 and a % 16 == 0 and b % 16 == 0
               and tr_span_ok(M, lz) and tr_span_ok(M, lx) for n, k, lz, lx, a, b in zip(Ns, Ks, ldzs, ldxs, dz_ptrs, x_ptrs))


def failing_terms(M, p):
    """The predicate terms problem ``p`` fails, by name (operand buffers start 16-byte aligned: ``in_layout``)."""
    lds = (p.ldz, p.ldx)
    bad = {"N%4": p.N % 4, "K%4": p.K % 4, "ldz%4": p.ldz % 4, "ldx%4": p.ldx % 4, "dz+4B": (ZC0 + p.zoff) % 4,
           "x+4B": (XC0 + p.xoff) % 4, "ld>=2^24": any(ld >= 1 << 24 for ld in lds),
           "M*ld*4>=2^31": any(ld < 1 << 24 and M * ld * 4 >= 1 << 31 for ld in lds)}
    return {k for k, v in bad.items() if v}


def launch_tr(case, base=0):
    """The staging ``case`` takes under the launcher of its entry point, from operand pointers laid out by ``in_layout``."""
    zo, xo, _ = in_layout(case)
    dzp, xp = [base + 4 * o for o in zo], [base + 4 * o for o in xo]
    ps = case.probs
    if case.entry == "grouped":
        return grouped_tr(case.M, ps[0].N, ps[0].K, ps[0].ldz, ps[0].ldx, dzp, xp)
    return ragged_tr(case.M, [p.N for p in ps], [p.K for p in ps], [p.ldz for p in ps], [p.ldx for p in ps], dzp, xp)


# ----------------------------------------------------------------------------------------------------- memory layout
def in_layout(case):
    """(dz offsets, x offsets, total): float offsets of each problem's first operand element in ONE flat NaN-filled input
    buffer.  Every operand is a column block (first column ZC0 + zoff / XC0 + xoff) of an [M + TAIL, ld] buffer that starts
    on a 64-byte boundary.  ``big`` cases keep dz elsewhere (offset of its column only)."""
    zo, xo, at = [], [], 0
    for p in case.probs:
        if case.big:
            zo.append(ZC0 + p.zoff)
        else:
            assert ZC0 + p.zoff + p.N <= p.ldz, p
            zo.append(at + ZC0 + p.zoff)
            at += -(-(case.M + TAIL) * p.ldz // 16) * 16
        assert XC0 + p.xoff + p.K <= p.ldx, p
        xo.append(at + XC0 + p.xoff)
        at += -(-(case.M + TAIL) * p.ldx // 16) * 16
    return zo, xo, at


def out_layout(case):
    """(dW offsets, db offsets, total) in one flat sentinel-filled arena: every dW_p is an [N, K] block with >= G_ROWS guard
    rows (>= G_WORDS words) before and after it, every db_p an [N] block between >= G_WORDS guard words -- also where the
    problem has no bias (the block then has to keep the sentinel)."""
    wo, bo, at = [], [], 0
    for p in case.probs:
        g = max(G_ROWS * p.K, G_WORDS)
        wo.append(at + g)
        at += g + p.N * p.K + g
    for p in case.probs:
        bo.append(at + G_WORDS)
        at += G_WORDS + p.N + G_WORDS
    return wo, bo, at


# ----------------------------------------------------------------------------------------------------- data and reference
_DATA, _REF = {}, {}


def operands(M, p):
    """(dz [M, N], x [M, K]) of problem ``p`` (seeded): fp32 standard normals (``positive``: uniform in [0.5, 1.5))."""
    key = (M, p.N, p.K, p.seed, p.positive)
    if key not in _DATA:
        assert p.seed >= 0
        draw = (lambda *a, **k: 0.5 + torch.rand(*a, **k)) if p.positive else torch.randn
        _DATA[key] = (draw(M, p.N, generator=gen(M, p.N, p.K, p.seed, 1)), draw(M, p.K, generator=gen(M, p.N, p.K, p.seed, 2)))
    return _DATA[key]


def old_contents(M, p):
    """What dW_p / db_p hold before a launch that accumulates into them."""
    return (torch.randn(p.N, p.K, generator=gen(M, p.N, p.K, p.seed, 3)), torch.randn(p.N, generator=gen(M, p.N, p.K, p.seed, 4)))


def statement(dz, x, terms, old_w=None, old_b=None):
    """(dW, db) in fp64."""
    a, b = (dz.bfloat16(), x.bfloat16()) if terms == 1 else (dz, x)
    dW, db = a.to(F64).t() @ b.to(F64), dz.to(F64).sum(0)
    return (dW if old_w is None else dW + old_w.to(F64)), (db if old_b is None else db + old_b.to(F64))


def reference(M, p, terms):
    """(dW, db) of a seeded problem, with its old contents where it accumulates (db also where the case passes none)."""
    key = (M, p.N, p.K, p.seed, p.positive, p.acc, terms == 1)
    if key not in _REF:
        old = old_contents(M, p) if p.acc else (None, None)
        _REF[key] = statement(*operands(M, p), terms, *old)
    return _REF[key]


def db_bound(M, dz, old_b=None):
    s = dz.to(F64).abs().sum(0)
    return (M + 8) * 2.0 ** -24 * (s if old_b is None else s + old_b.to(F64).abs())


def long_reduction_bound(M, dz, x, ref, terms):
    return (M + 64) * 2.0 ** -24 * (dz.to(F64).abs().t() @ x.to(F64).abs()) + TOL[terms] * float(ref.abs().max())


# ----------------------------------------------------------------------------------------------------- comparison
def block_errors(got, ref):
    """(max |got - ref| / max |ref|, worst 32 x 32 block: its max error / max(its max |ref|, 1e-3 max |ref|))."""
    got, ref = got.detach().to(F64).cpu(), ref.detach().to(F64).cpu()
    assert got.shape == ref.shape and got.dim() == 2, (got.shape, ref.shape)
    err, scale = (got - ref).abs(), float(ref.abs().max())
    if scale == 0.0:
        return (0.0, 0.0) if float(err.max()) == 0.0 else (math.inf, math.inf)
    R, C = got.shape
    pr, pc = -R % 32, -C % 32
    eb = F.pad(err, (0, pc, 0, pr)).view((R + pr) // 32, 32, (C + pc) // 32, 32).amax((1, 3))
    rb = F.pad(ref.abs(), (0, pc, 0, pr)).view((R + pr) // 32, 32, (C + pc) // 32, 32).amax((1, 3))
    return float(err.max()) / scale, float((eb / rb.clamp_min(1e-3 * scale)).max())


def check_close(got, ref, tol, what):
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    whole, block = block_errors(got, ref)
    assert whole <= tol, f"{what}: rel err {whole:.3g} > {tol:g}"
    assert block <= 4 * tol, f"{what}: a 32x32 block is off by {block:.3g} of its own magnitude (> {4 * tol:g})"
    return whole, block


def check_within(got, ref, bound, what):
    """Element-wise derived bound (a tensor of the same shape)."""
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got.detach().to(F64).cpu() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    assert bool((err <= bound).all()), f"{what}: {worst:.3g} x its derived bound"
    return worst


# ----------------------------------------------------------------------------------------------------- the case table
NK = {1: 1, 31: 1, 32: 1, 33: 2, 64: 2, 65: 3, 96: 3, 97: 4, 128: 4, 129: 5}      # tokens -> k-tiles, as the issue lists them
STAGINGS = (True, False)
CELLS = [(e, t, tr) for e in ENTRIES for t in (1, 3, 6) for tr in STAGINGS]


def cell_id(entry, terms, tr):
    return f"{entry}-{MODES[terms]}-{'tr' if tr else 'dword'}"


def reduction_cases(entry, terms, tr):
    """M = 1 .. 129: nk = 1 .. 5 with a full and a partial last k-tile (NS = 3: the single-buffer loop; NS <= 2: two buffers,
    and under TR the two-register-set pipeline whose prologue special-cases nk = 1, 2, 3).  260 x 132 (257 x 129) has a second
    tile row of 4 rows (1 row) and a second tile column."""
    big = P(260, 132) if tr else P(257, 129)
    probs, tiles = ((big, big), 8) if entry == "grouped" else ((big, P(4, 128)), 5)
    return [Case(f"red{M}", entry, terms, M, probs, tr, tiles, nk) for M, nk in NK.items()]


# (N, K, tiles of ONE problem)
EDGE_GROUPED = {True: [(4, 4, 1), (252, 124, 1), (256, 128, 1), (260, 132, 4), (260, 4, 2), (4, 132, 2)],
                False: [(1, 1, 1), (255, 127, 1), (257, 129, 4), (1, 132, 2), (260, 129, 4), (255, 4, 1)]}
EDGE_N = {True: (4, 252, 256, 260), False: (1, 4, 252, 255, 256, 257, 260)}
EDGE_K = {True: (4, 124, 128, 132), False: (1, 4, 124, 127, 128, 129, 132)}
EDGE_RAGGED_TILES = {True: 25, False: 81}    # (1 + 1 + 1 + 2)^2 and (5 x 1 + 2 x 2)^2


def edge_cases(entry, terms, tr):
    """Output edges at M = 33 (nk = 2, a partial last k-tile).  Ragged: every N x K of the issue's lists as the problems of ONE
    launch (16 under TR, 49 under the dword staging); grouped: two problems per shape."""
    if entry == "ragged":
        probs = tuple(P(N, K) for N in EDGE_N[tr] for K in EDGE_K[tr])
        return [Case("edges", entry, terms, 33, probs, tr, EDGE_RAGGED_TILES[tr], 2)]
    return [Case(f"edge{N}x{K}", entry, terms, 33, (P(N, K), P(N, K)), tr, 2 * t, 2) for N, K, t in EDGE_GROUPED[tr]]


FLIP_BASE = P(260, 132)      # 2 x 2 tiles; 3 problems, M = 65: 12 tiles, nk = 3
FLIPPED = {"N%4": P(258, 132), "K%4": P(260, 130), "ldz%4": P(260, 132, ldz=277), "ldx%4": P(260, 132, ldx=141),
           "dz+4B": P(260, 132, zoff=1), "x+4B": P(260, 132, xoff=1)}
SAME_DATA_FLIPS = ("ldz%4", "ldx%4", "dz+4B", "x+4B")      # the flipped launch multiplies the base case's data


def flip_base(entry, terms):
    return Case("flipbase", entry, terms, 65, (FLIP_BASE,) * 3, True, 12, 3)


def flip_cases():
    """One predicate term turned at a time from ``flip_base``.  Grouped: the shape terms hold for every problem, the pointer
    terms for the first / the last one; ragged: every term on the first / the last problem only."""
    out, i = [], 0
    for entry in ENTRIES:
        for term, odd in FLIPPED.items():
            wheres = ("all",) if entry == "grouped" and not term.endswith("4B") else ("first", "last")
            for where in wheres:
                probs = {"all": (odd,) * 3, "first": (odd, FLIP_BASE, FLIP_BASE), "last": (FLIP_BASE, FLIP_BASE, odd)}[where]
                slug = term.replace("%", "mod").replace("+", "_plus_")
                out.append(Case(f"flip_{slug}_{where}", entry, (1, 3, 6)[i % 3], 65, probs, False, 12, 3, flip=(term, where)))
                i += 1
    return out


def span_cases():
    """e3d_tr_span_ok, both clauses, N = 8, K = 4 (one tile): a row stride of 2^24 at M = 2, and ldz = 1024 at M = 2^19 - 1
    (2^31 - 4096 bytes: TR) and M = 2^19 (2^31: dword), the latter two on positive operands."""
    out, wide = [], P(8, 4, ldz=1024, positive=True)
    for entry in ENTRIES:
        out.append(Case("span_ld", entry, 3, 2, (P(8, 4, ldz=1 << 24),), False, 1, 1, flip=("ld>=2^24", "all"), big=True))
        out.append(Case("span_under", entry, 3, (1 << 19) - 1, (wide,), True, 1, 16384, big=True))
        out.append(Case("span_bytes", entry, 3, 1 << 19, (wide,), False, 1, 16384, flip=("M*ld*4>=2^31", "all"), big=True))
    return out


ONE, TWO, FOUR, FIVE, SIX = P(36, 20), P(260, 20), P(260, 132), P(4, 516), P(260, 260)      # shapes by their tile count
ACC_AT = (0, 31, 32, 63)


def _acc(probs, at=ACC_AT):
    return tuple(dataclasses.replace(p, acc=i in at) for i, p in enumerate(probs))


def table_cases():
    """The problem table: counts, tile totals (xcd_remap with n < 8 and n % 8 != 0), bisection boundaries, accumulate bits at
    0 / 31 / 32 / 63 (together, and the low and the high pair apart: a bit index taken modulo 32 shows), absent bias gradients."""
    out = []
    for count in (1, 2, 7, 8, 9, 63, 64):
        out.append(Case(f"count{count}", "grouped", 3, 33, _acc((ONE,) * count), True, count, 2))
    for name, at in (("count64lo", ACC_AT[:2]), ("count64hi", ACC_AT[2:])):      # (0, 31, 32, 63 together look the same modulo 32)
        out.append(Case(name, "grouped", 3, 33, _acc((ONE,) * 64, at), True, 64, 2))
        out.append(Case(name, "ragged", 3, 33, _acc((ONE, TWO) * 32, at), True, 96, 2))
    out.append(Case("count13x5", "grouped", 3, 33, (FIVE,) * 13, True, 65, 2))
    out.append(Case("nodb", "grouped", 6, 33, _acc((TWO,) * 2, (1,)), True, 4, 2, db_null=True))
    out.append(Case("count1", "ragged", 3, 33, (ONE,), True, 1, 2))
    singles = (ONE, P(8, 4), P(256, 128), P(4, 124))
    out.append(Case("count64x1", "ragged", 3, 33, _acc(tuple(singles[i % 4] for i in range(64))), True, 64, 2))
    cyc = tuple(dataclasses.replace((ONE, TWO, FOUR)[i % 3], bias=i % 3 != 1) for i in range(64))
    for terms in (1, 3, 6):
        out.append(Case("count64cyc", "ragged", terms, 33, _acc(cyc), True, 148, 2))
    odd_last = cyc[:63] + (dataclasses.replace(ONE, zoff=1),)
    out.append(Case("count64cyc_oddlast", "ragged", 3, 33, _acc(odd_last), False, 148, 2))
    out.append(Case("big_then_one", "ragged", 3, 33, (SIX, ONE), True, 7, 2))
    out.append(Case("ones_then_big", "ragged", 3, 33, (ONE, ONE, SIX), True, 8, 2))
    out.append(Case("big_then_ones", "ragged", 3, 33, (SIX, ONE, ONE, ONE), True, 9, 2))
    lone = tuple(dataclasses.replace(TWO if i == 0 else ONE, bias=i in (0, 17)) for i in range(64))
    out.append(Case("lone_db", "ragged", 3, 33, lone, True, 65, 2))
    out.append(Case("nodb", "ragged", 6, 33, _acc((TWO, ONE, FOUR), (1,)), True, 7, 2, db_null=True))
    return out


def all_cases():
    out = []
    for cell in CELLS:
        out += reduction_cases(*cell) + edge_cases(*cell)
    return out + flip_cases() + [flip_base(e, t) for e in ENTRIES for t in (1, 3, 6)] + span_cases() + table_cases()


REFUSALS = ("count0", "count65", "terms2", "ldz_below_N", "ldx_below_K", "null_dz", "null_x", "null_dw", "M0")
