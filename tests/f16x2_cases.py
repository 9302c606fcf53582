"""Exact cases for the two-plane fp16 GEMM family (include/pd_gemm.h: pd_gemm_tn_f16x2, pd_gemm_tn_f16x2_bf16out, pd_conv3x3_nhwc_f16x2,
pd_gemm_wgrad_acc_f16x2_ws, pd_gemm_wgrad_f16x2_grouped, pd_conv3x3_wgrad_nhwc_f16x2, pd_row_amax_f32, pd_cast_bf16_f32_amax;
csrc/gemm_f16x2.hip, the H2 kernels of csrc/gemm_x3.hip, csrc/f16x2.h).  The instrument (Guarded, bits, the sentinels) is tests/smallgemm_cases.py's,
imported by the tests, not copied.

The split is deterministic (f16x2.h): with e the biased exponent of a row's maximum clamped to [20, 250], s = 2^(141 - e), inv = 2^(e - 141),
x' = s x, hi = fp16(x') (nearest even), lo = fp16(x' - hi); a product is hi_a hi_b + hi_a lo_b + lo_a hi_b accumulated in fp32 and the epilogue
is acc (inv_a inv_b) + bias.  `row_scale()` and `split()` restate that with torch.half casts.

Operands (`operand()`): scaled elements are x' = +-2^shift (4096 a + b), a in {1..amag}, b from `bset`, kept with probability `d` and
exactly 0 otherwise (a is never 0: a lone b would land in the hi plane; b counts away from zero).  One element per row (column row % cols) is 4096 amag + max(bset), the
known row maximum, which `shift` puts into [2^14, 2^15).  Then hi = 2^shift 4096 a and lo = 2^shift b exactly, under any power-of-two scale that
stays inside fp16's range, so every term of the three-product sum is a multiple of 2^(2 shift + 12) and every partial sum, in any order (the
MFMAs', a persistent kernel's, the column sums' atomics), is exact in fp32 as long as sum |terms| stays below 2^24 units.  The result must
then equal the float64 value of the THREE-product formula bit for bit; tests/test_f16x2_cases_cpu.py proves the conditions for every case and
that the value differs from the full product's rounding and from the sums that miss a product.  Rows are multiplied by their own power of
two 2^r (`rpow`: r in [-30, 30]) wherever nothing ties the rows of a launch to a common unit (no bias, no column sums).

Column sums (mode 2) run over all M rows: sum |terms| < 2^24 units with hi hi terms of 2^12 units each leaves fewer than 2^13 / M terms per
output, i.e. fewer than one at the 8 192-row shapes.  The mode-2 operands are therefore SPARSE (`SPARSE_A`, `SPARSE_B`: amag = 1, b = 1
and b = 2, all positive: with one to three terms per output, signed cross products would cancel in every eighth; the dense cases carry the
signs), and their sensitivity is taken over the outputs that
have a term at all; what a mode-2 launch can get wrong that a mode-0 launch cannot is the mask's order, which shows on every such output.

Which body a table reaches (the GPU test asserts it with pd_gemm_tn_f16x2_which):
  TILE128 x TILE128_DEBUG, TILE128_OPTIONS, BF16OUT   gemm_tn_f16x2<128, 128, 64, 16, MODE 0 | 1, NRS 1 | 2, FAST 0 | 1>
  TILE256 x TILE256_DEBUG, RELU_PAIRS_TILED            gemm_tn_f16x2<256, 256, 128, 16, MODE 0 | 1 | 2, ..>
  ROWS, RELU_PAIRS_ROWS, BITS_CONTRACT                 gemm_rows_f16x2_k256<AM, MODE 0 | 1 | 2>
  KPC                                                  gemm_kpc_f16x2<AM>
  CONV x CONV_DEBUG                                    gemm_tn_f16x2<128 | 256, .., MODE 0, CONV> (pd_conv3x3_nhwc_f16x2)
  WGRAD_NARROW, WGRAD_WIDE, WGRAD_GROUPED_*, CONV_WGRAD  the H2 weight-gradient bodies of csrc/gemm_x3.hip (128-tile and 256-tile, single and grouped)"""
import collections

import torch

F32, F64 = torch.float32, torch.float64
E_UNIT = 141                       # the biased exponent at which row_scale gives s = inv = 1: maxima in [2^14, 2^15)


# ------------------------------------------------------------------------------------------------ the oracle of f16x2.h
def row_scale(amax):
    """fp32 maxima -> (s, inv) fp32, as pdh2::row_scale"""
    e = ((amax.to(F32).contiguous().view(torch.int32) >> 23) & 0xFF).clamp(20, 250)
    return ((268 - e) << 23).view(F32), ((e - 14) << 23).view(F32)


def split(x, amax=None):
    """x fp32 [rows, cols], amax [rows] or None (unit scale) -> hi, lo (the fp16 planes, as float64), inv [rows] fp32"""
    if amax is None:
        s = inv = torch.ones(x.shape[0], dtype=F32, device=x.device)
    else:
        s, inv = row_scale(amax)
    xs = x.to(F32) * s[:, None]
    hi = xs.half().float()
    lo = (xs - hi).half().float()
    return hi.double(), lo.double(), inv


def scaled(x, amax=None):
    """x' = s x in float64 (what hi + lo must add up to)"""
    s = torch.ones(x.shape[0], dtype=F32, device=x.device) if amax is None else row_scale(amax)[0]
    return x.double() * s.double()[:, None]


# ------------------------------------------------------------------------------------------------ operands
Op = collections.namedtuple("Op", "x amax")        # x fp32 [rows, cols]; amax fp32 [rows]: the true absolute row maxima

DENSE = dict(amag=3, bset=(-1, 0, 1))
SPARSE_A = dict(amag=1, bset=(1,), signed=False)
SPARSE_B = dict(amag=1, bset=(2,), signed=False, even=True)


def operand(rows, cols, seed, d=1.0, amag=3, bset=(-1, 0, 1), r=0, even=False, signed=True):
    """r: an int, or an int tensor [rows] — the power of two of each row relative to the scaled form (r = 0: x == x', an O(1) operand that
    needs no maxima).  even: every row keeps the same number of elements, ceil(d cols) (a column sum of a product scales with the number of
    elements of the weight row: drawn independently it would vary by +-70 % at 13 elements per row)"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(1, amag + 1, (rows, cols), generator=g)
    sign = torch.randint(0, 2, (rows, cols), generator=g) * 2 - 1 if signed else 1
    b = torch.tensor(bset)[torch.randint(0, len(bset), (rows, cols), generator=g)]
    keep = torch.rand((rows, cols), generator=g)
    keep = (keep.argsort(1).argsort(1) < -(-d * cols // 1)) if even else (keep < d)
    v = torch.where(keep, sign * (4096 * a + b), torch.zeros_like(a))      # b counts away from zero: 4096 - 2 would fit the hi plane whole
    top = 4096 * amag + max(bset)
    if cols:
        v[torch.arange(rows), torch.arange(rows) % cols] = top
    shift = 14 - (top.bit_length() - 1)
    rr = torch.as_tensor(r, dtype=F64).expand(rows) if not torch.is_tensor(r) else r.double()
    x = (v.double() * 2.0 ** shift * torch.exp2(rr)[:, None]).float()
    amax = (torch.full((rows,), float(top * 2 ** shift), dtype=F64) * torch.exp2(rr)).float()
    if not cols:
        amax = torch.zeros(rows)
    return Op(x, amax)


def row_powers(rows, seed, lo=-30, hi=30):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, (rows,), generator=g)


def block_powers(rows, block, seed, lo=-30, hi=30):
    """one power per `block` rows: a stale inverse scale carried from one block of a persistent kernel to the next shows"""
    p = row_powers(-(-rows // block), seed, lo, hi)
    return p.repeat_interleave(block)[:rows]


# ------------------------------------------------------------------------------------------------ the cases
# amax: which operands come with row maxima ("both" | "none" | "a" | "b"); over: the maxima are over-stated by 2^over; rpow: rows of the operands
# that have maxima carry their own power of two; bias: None | "int" (multiples of the unit) | "half" (odd multiples of half the unit: no
# pre-activation is exactly zero); mode 0 | 1; special: None | "tiny" (row 0 all zero, row 1 with biased exponent 15: below the clamp at 20) |
# "huge" (row 1 with biased exponent 251: above the clamp at 250.  252 cannot be built: its scaled maximum 1.5 x 2^16 leaves fp16's range)
# indexing: the case is too small for the percentages of the CPU proof (both planes, sensitivity); it keeps every exactness condition
Tn = collections.namedtuple("Tn", "M N K seed d amax over rpow bias mode special indexing", defaults=(1.0, "both", 0, True, None, 0, None, False))


def tn_id(c):
    parts = [f"{c.M}x{c.N}x{c.K}", c.amax]
    parts += [f"over{c.over}"] * bool(c.over) + ["bias" + (c.bias or "")] * bool(c.bias) + [f"mode{c.mode}"] * bool(c.mode) + [c.special or ""] * bool(c.special)
    return "-".join(parts)


# 128 x 128 tiles: one row; one interior tile on the interleaved step + three guarded ones; K % 32 != 0 (every tile guarded); 1, 2, 2, 3, 5
# steps of 16 (the register-stage prologue and both parities); K = 0 (the result is the bias)
TILE128_DEBUG = (0, 70, 4, 14)
TILE128 = [Tn(1, 4, 4, 2101, indexing=True), Tn(130, 132, 64, 2102), Tn(130, 132, 68, 2103), Tn(257, 64, 16, 2104), Tn(257, 64, 20, 2105), Tn(257, 64, 32, 2106),
           Tn(257, 64, 48, 2107), Tn(257, 64, 80, 2108), Tn(33, 12, 0, 2109, amax="none", rpow=False, bias="int", indexing=True)]
TILE128_OPTIONS_DEBUG = (0, 70)
TILE128_OPTIONS = [
    Tn(130, 132, 68, 2201, amax="none", rpow=False), Tn(130, 132, 68, 2202, amax="a"), Tn(130, 132, 68, 2203, amax="b"),
    Tn(130, 132, 68, 2204, over=3), Tn(257, 64, 48, 2205, over=7),
    Tn(130, 132, 68, 2206, rpow=False, bias="int"), Tn(130, 132, 68, 2207, rpow=False, bias="half", mode=1),
    Tn(257, 64, 48, 2208, amax="none", rpow=False, bias="half", mode=1),
    Tn(130, 132, 64, 2209, rpow=False, special="tiny"), Tn(130, 132, 64, 2210, rpow=False, special="huge"),
]
BF16OUT = TILE128[:3]
# 256 x 256 tiles: forced (debug 3: one register stage, 13: two), a ragged last row tile, one step of 16
TILE256_DEBUG = (3, 13)
TILE256 = [Tn(1024, 256, 64, 2301), Tn(1030, 512, 96, 2302), Tn(1281, 256, 16, 2303)]
# the row stream: one tile per row group (the second prefetch is clamped); a ragged last tile and unequal groups; four tiles per group (the
# double buffer wraps)
ROWS_DEBUG = (0, 61)
ROWS = [Tn(8192, 256, 256, 2401), Tn(8197, 256, 256, 2402), Tn(8200, 1024, 256, 2403),
        Tn(8192, 256, 256, 2404, amax="none", rpow=False), Tn(8197, 256, 256, 2405, amax="none", rpow=False),
        Tn(8200, 1024, 256, 2406, amax="none", rpow=False, bias="int")]
# producer / consumer wavefronts (K >= 512: d = 0.5 keeps the sums exact); 17 chunks and a ragged last block; KPC_MANY(cus): more work
# items than CUs, a different magnitude in every 192-row block
KPC_BLOCK = 192
KPC = [Tn(8192, 256, 512, 2501, d=0.5), Tn(8195, 512, 544, 2502, d=0.5), Tn(8192, 256, 512, 2503, d=0.5, amax="none", rpow=False),
       Tn(8195, 512, 544, 2504, d=0.5, amax="none", rpow=False, bias="int"), Tn(8192, 256, 512, 2505, d=0.5, rpow=False, bias="int")]


def kpc_many(cus):
    return Tn(KPC_BLOCK * (cus // 2) + KPC_BLOCK + 5, 512, 512, 2506, d=0.5, rpow="blocks")


# ReLU pairs: a mode-1 launch (dense operands, "half" bias) writes the sign bits, a mode-2 launch with OTHER, sparse operands reads them.
# (shape, seed, density of the mode-2 operands: M K d^2 / 2 x 2^12 < 2^24)
Pair = collections.namedtuple("Pair", "M N K seed d2")
RELU_PAIRS_TILED_DEBUG = (0, 13, 62)
RELU_PAIRS_TILED = [Pair(1024, 256, 64, 2601, 0.2), Pair(1030, 512, 96, 2602, 0.17), Pair(1281, 256, 16, 2603, 0.33)]
RELU_PAIRS_ROWS = [Pair(8197, 512, 256, 2701, 0.052), Pair(8200, 1024, 256, 2702, 0.052)]
BITS_CONTRACT = Pair(8192, 512, 256, 2801, 0.052)
COLSUM_UNIT = 2.0 ** 20            # the column sums' pre-fill: integers in [-64, 64] times this (a multiple of every term's unit)

ALL_TN = TILE128 + TILE128_OPTIONS + TILE256 + ROWS + KPC + [kpc_many(256)]
ALL_PAIRS = RELU_PAIRS_TILED + RELU_PAIRS_ROWS + [BITS_CONTRACT]

# pd_row_amax_f32: (rows, cols, ld, element offset of the base: 4 = 16-byte aligned, 1 = the scalar path)
ROW_AMAX = [(1, 4, 8, 4), (3, 36, 40, 4), (5, 260, 264, 4), (1027, 1024, 1028, 4), (5, 7, 9, 1), (3, 36, 37, 4)]
CAST_AMAX = [(1, 8), (5, 264), (1027, 1024)]


def tn_operands(c):
    """A [M, K], B [N, K] as Op, bias [N] fp32 or None.  Operands without maxima are O(1) (r = 0)."""
    has_a, has_b = c.amax in ("both", "a"), c.amax in ("both", "b")
    if c.rpow == "blocks":
        ra, rb = block_powers(c.M, KPC_BLOCK, c.seed + 10), row_powers(c.N, c.seed + 11)
    else:
        ra = row_powers(c.M, c.seed + 10) if (c.rpow and has_a) else 0
        rb = row_powers(c.N, c.seed + 11) if (c.rpow and has_b) else 0
    if c.special == "tiny":
        ra, rb = torch.zeros(c.M, dtype=torch.int64), 20
        ra[1] = 15 - E_UNIT
    if c.special == "huge":
        ra, rb = torch.zeros(c.M, dtype=torch.int64), -30
        ra[1] = 251 - E_UNIT
    a = operand(c.M, c.K, c.seed, c.d, r=ra, **DENSE)
    b = operand(c.N, c.K, c.seed + 1, c.d, r=rb, **DENSE)
    if c.special == "tiny":
        a.x[0] = 0.0
        a.amax[0] = 0.0
    return a, b, tn_bias(c)


def tn_bias(c):
    """multiples of 2^14 (the terms' unit at r = 0), or odd multiples of 2^13"""
    if c.bias is None:
        return None
    g = torch.Generator().manual_seed(c.seed + 2)
    k = torch.randint(-512, 513, (c.N,), generator=g).double()
    return (k * 2.0 ** 14 if c.bias == "int" else (2 * k + 1) * 2.0 ** 13).float()


def given(op, over):
    """the maxima a launch is handed: the true ones, over-stated by 2^over"""
    return op.amax * 2.0 ** over


def tn_maxima(c, a, b):
    return (given(a, c.over) if c.amax in ("both", "a") else None), (given(b, c.over) if c.amax in ("both", "b") else None)


def pair_operands(p, maxima=True):
    """forward: A1 [M, K], B1 [N, K] dense, bias1 "half"; backward: A2 [M, K'], B2 [N, K'] sparse (K' = K), the column sums' pre-fill [N].
    maxima False: every operand is O(1) already (r = 0); True: r = 3 for A and -2 for B, one power per operand (the column sums tie the rows)"""
    ra, rb = (3, -2) if maxima else (0, 0)
    a1 = operand(p.M, p.K, p.seed, r=ra, **DENSE)
    b1 = operand(p.N, p.K, p.seed + 1, r=rb, **DENSE)
    g = torch.Generator().manual_seed(p.seed + 2)
    bias1 = ((2 * torch.randint(-512, 513, (p.N,), generator=g).double() + 1) * 2.0 ** (13 + ra + rb)).float()
    a2 = operand(p.M, p.K, p.seed + 3, p.d2, r=ra, **SPARSE_A)
    b2 = operand(p.N, p.K, p.seed + 4, p.d2, r=rb, **SPARSE_B)
    pre = (torch.randint(-64, 65, (p.N,), generator=g).double() * COLSUM_UNIT).float()
    return a1, b1, bias1, a2, b2, pre


# ------------------------------------------------------------------------------------------------ float64 references
Products = collections.namedtuple("Products", "hh hl lh ll scale")       # the four plane products [M, N] float64 and inv_a inv_b (fp32 product)


def products(a, b, a_amax=None, b_amax=None, absolute=False):
    ha, la, ia = split(a, a_amax)
    hb, lb, ib = split(b, b_amax)
    if absolute:
        ha, la, hb, lb = ha.abs(), la.abs(), hb.abs(), lb.abs()
    return Products(ha @ hb.t(), ha @ lb.t(), la @ hb.t(), la @ lb.t(), (ia[:, None] * ib[None, :]).double())


def finish(acc, scale, bias=None, relu=False):
    r = acc * scale
    if bias is not None:
        r = r + bias.double()
    if relu:
        r = r.relu()
    return r + 0.0                                 # the kernels accumulate onto +0.0


def ref_tn(a, b, a_amax=None, b_amax=None, bias=None, relu=False):
    """the kernel's formula in float64: (hi hi + hi lo + lo hi) (inv_a inv_b) + bias"""
    p = products(a, b, a_amax, b_amax)
    return finish(p.hh + p.hl + p.lh, p.scale, bias, relu)


def ref_masked(a, b, a_amax, b_amax, fwd, colsum_prefill):
    """mode 2: the product where the forward result was > 0, 0 elsewhere; prefill + column sums"""
    r = ref_tn(a, b, a_amax, b_amax)
    r = torch.where(fwd > 0, r, torch.zeros_like(r))
    return r, colsum_prefill.double() + r.sum(0)


def ref_c_amax(ref, prefill):
    """atomic max into a pre-filled buffer"""
    return torch.maximum(prefill.double(), ref.abs().amax(1)) if ref.shape[1] else prefill.double()


def exact_in_fp32(r):
    return bool((r.float().double() == r).all()) and bool(torch.isfinite(r.float()).all())


def lowbit(x):
    """float64 -> the largest power of two dividing each element (inf for 0)"""
    m, e = torch.frexp(x.abs())
    mi = (m * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).double() * torch.exp2((e - 53).double())
    return torch.where(x == 0, torch.full_like(low, float("inf")), low)


def row_unit(plane):
    """[rows]: the largest power of two dividing every element of a row (inf for a row of zeros)"""
    return lowbit(plane).amin(1) if plane.shape[1] else torch.full((plane.shape[0],), float("inf"), dtype=F64)


def term_unit(a, b, a_amax=None, b_amax=None):
    """[M, N]: a power of two dividing every term hi hi, hi lo, lo hi of an output, in the scaled domain"""
    ha, la, _ = split(a, a_amax)
    hb, lb, _ = split(b, b_amax)
    uha, ula, uhb, ulb = row_unit(ha), row_unit(la), row_unit(hb), row_unit(lb)

    def outer(p, q):
        return p[:, None] * q[None, :]
    u = torch.minimum(outer(uha, uhb), torch.minimum(outer(uha, ulb), outer(ula, uhb)))
    return u


# ------------------------------------------------------------------------------------------------ two-plane weight gradients
# pd_gemm_wgrad_acc_f16x2_ws / pd_gemm_wgrad_f16x2_grouped (csrc/gemm_x3.hip): dW[N, K] += dY[M, N]^T X[M, K], dB[N] += column sums of dY.
# The contraction runs over the rows and a workgroup scales its slab of rows by the slab's largest maximum, so these operands carry ONE power
# of two each (not one per row): exactness must not depend on how the launch cuts the rows into slabs.  amax: which operands bring maxima
# ("both" | "none" | "y" | "x"); d keeps M d^2 below 2^10 (sum |terms| < 2^24 units) and the column sums of dY below 2^24 of its units.
Wg = collections.namedtuple("Wg", "M N K seed d amax indexing", defaults=(1.0, "both", False))      # indexing: as for Tn (one row: one term per output)
WG_RY, WG_RX = 5, -3
# the 128-tile transpose-read body: one row; ragged in both directions; many slabs, one ragged tile
WGRAD_NARROW = [Wg(1, 128, 128, 2901, indexing=True), Wg(31, 132, 260, 2902, amax="none"), Wg(2100, 72, 40, 2903, d=0.5, amax="y"), Wg(31, 132, 260, 2904, amax="x")]
# the 256-tile body (and, with pd_debug_set("wgrad_wide", 0), the 128-tile body on the first): ragged in both directions; fewer rows than a chunk
WGRAD_WIDE = [Wg(300, 1024, 132, 2911), Wg(1100, 132, 1028, 2912, d=0.7, amax="none"), Wg(40, 1024, 256, 2913, amax="x")]
WGRAD_GROUPED_NARROW = [Wg(70, 72, 40, 2921), Wg(1, 128, 128, 2922, amax="none", indexing=True), Wg(333, 132, 260, 2923, amax="y")]
WGRAD_GROUPED_MIXED = [WGRAD_WIDE[0], WGRAD_NARROW[1], WGRAD_WIDE[2]]
ALL_WG = WGRAD_NARROW + WGRAD_WIDE + WGRAD_GROUPED_NARROW


def wg_id(c):
    return f"wg{c.M}x{c.N}x{c.K}-{c.amax}"


def wg_operands(c):
    """dY [M, N], X [M, K] as Op, the maxima handed over (or None), the pre-fills of dW [N, K] and dB [N] (multiples of the terms' units)"""
    has_y, has_x = c.amax in ("both", "y"), c.amax in ("both", "x")
    ry, rx = (WG_RY if has_y else 0), (WG_RX if has_x else 0)
    dy = operand(c.M, c.N, c.seed, c.d, r=ry, **DENSE)
    x = operand(c.M, c.K, c.seed + 1, c.d, r=rx, **DENSE)
    g = torch.Generator().manual_seed(c.seed + 2)
    dw0 = (torch.randint(-64, 65, (c.N, c.K), generator=g).double() * 2.0 ** (14 + ry + rx)).float()
    db0 = (torch.randint(-64, 65, (c.N,), generator=g).double() * 2.0 ** (1 + ry)).float()
    return dy, x, (dy.amax if has_y else None), (x.amax if has_x else None), dw0, db0


def wg_products(dy, x, y_amax=None, x_amax=None, absolute=False):
    """the plane products of dY^T X, [N, K] float64, and the one inverse scale (the maxima of a case are the same in every row: every slab
    arrives at the same power of two)"""
    hy, ly, iy = split(dy, y_amax)
    hx, lx, ix = split(x, x_amax)
    assert bool((iy == iy[0]).all()) and bool((ix == ix[0]).all())
    if absolute:
        hy, ly, hx, lx = hy.abs(), ly.abs(), hx.abs(), lx.abs()
    return Products(hy.t() @ hx, hy.t() @ lx, ly.t() @ hx, ly.t() @ lx, (iy[0] * ix[0]).double())


def ref_wgrad(dy, x, y_amax, x_amax, dw0):
    p = wg_products(dy, x, y_amax, x_amax)
    return (p.hh + p.hl + p.lh) * p.scale + dw0.double() + 0.0


def ref_db(dy, db0):
    return dy.double().sum(0) + db0.double() + 0.0


# ------------------------------------------------------------------------------------------------ 3 x 3 convolution (pd_conv3x3_nhwc_f16x2)
# X [B, H, W, Ci], Wk [Co][3][3][Ci], stride 1, pad 1.  Row m of the implicit GEMM is output pixel m, its K = 9 Ci elements the (tap, channel)
# patch around it (zeros outside the image), and the kernel scales that whole row by the LARGEST of the maxima of the up to nine in-image
# pixels it reads: `patches()` gathers the rows and `patch_maxima()` those maxima, after which the oracle is ref_tn on them.  Pixels carry
# their own power of two 2^r, r in {0, 1, 2}: a pixel up to 2^2 below its neighbourhood's maximum still splits exactly, and the terms' unit
# falls by at most 2^2, which the densities d leave room for (9 Ci d^2 <= 144).  amax: "both" | "none" | "x" | "w"; bias ties the rows to one unit,
# so the case that has one has O(1) pixels.
Conv = collections.namedtuple("Conv", "B H W Ci Co seed d amax bias", defaults=("both", None))
CONV_DEBUG = (0, 70, 21, 3)
# every up / down tap outside (H = 1); W = 1; 288 pixels: interior tiles on the interleaved step, a tile across the boundary of two images; 260 filters
CONV = [Conv(2, 5, 7, 16, 8, 3301, 1.0), Conv(3, 1, 9, 32, 132, 3302, 0.7, amax="x"), Conv(2, 9, 1, 48, 64, 3303, 0.55, amax="w"),
        Conv(2, 12, 12, 32, 128, 3304, 0.7), Conv(1, 3, 3, 64, 260, 3305, 0.5, amax="none", bias="int")]
# the input gradient is the same call on dY with the flipped, transposed filter: CONV_DGRAD's Wk IS that filter ([32][3][3][48], the gradient of a
# 32 -> 48 channel convolution), `forward_filter()` the forward filter it came from; the CPU test proves with autograd that the product is the gradient
CONV_DGRAD = Conv(2, 6, 7, 48, 32, 3306, 0.55)
CONV.append(CONV_DGRAD)


def forward_filter(c, wk):
    """[c.Co, 9 c.Ci] (the filter the input-gradient call is handed: [ci][3][3][co] of the forward convolution, taps flipped) -> the forward
    filter [co][3][3][ci]"""
    return wk.view(c.Co, 3, 3, c.Ci).flip(1, 2).permute(3, 1, 2, 0).contiguous()


def conv_id(c):
    return f"{c.B}x{c.H}x{c.W}-{c.Ci}to{c.Co}-{c.amax}" + ("-bias" if c.bias else "")


def conv_operands(c):
    """X [B H W, Ci] and Wk [Co, 9 Ci] as Op (amax: per pixel / per filter), bias [Co] or None"""
    has_x, has_w = c.amax in ("both", "x"), c.amax in ("both", "w")
    M = c.B * c.H * c.W
    x = operand(M, c.Ci, c.seed, c.d, r=row_powers(M, c.seed + 10, 0, 2) if has_x else 0, **DENSE)
    w = operand(c.Co, 9 * c.Ci, c.seed + 1, c.d, r=row_powers(c.Co, c.seed + 11) if has_w else 0, **DENSE)
    bias = tn_bias(Tn(M, c.Co, 9 * c.Ci, c.seed, bias=c.bias))
    return x, w, bias


def _neighbours(c):
    """for every output pixel and tap: the input pixel's row index and whether it lies inside the image"""
    dev_b, dev_y, dev_x = torch.meshgrid(torch.arange(c.B), torch.arange(c.H), torch.arange(c.W), indexing="ij")
    idx, ok = [], []
    for tap in range(9):
        yy, xx = dev_y + tap // 3 - 1, dev_x + tap % 3 - 1
        inside = (yy >= 0) & (yy < c.H) & (xx >= 0) & (xx < c.W)
        idx.append(((dev_b * c.H + yy.clamp(0, c.H - 1)) * c.W + xx.clamp(0, c.W - 1)).reshape(-1))
        ok.append(inside.reshape(-1))
    return torch.stack(idx, 1), torch.stack(ok, 1)                 # [M, 9]


def patches(c, x, into_next_image=False):
    """[M, 9 Ci]: the GEMM rows.  into_next_image: the planted defect — taps are taken from the flat pixel index m + dy W + dx, across image
    borders and row ends"""
    idx, ok = _neighbours(c)
    if into_next_image:
        M = x.shape[0]
        m = torch.arange(M)[:, None]
        flat = m + torch.tensor([(t // 3 - 1) * c.W + t % 3 - 1 for t in range(9)])[None, :]
        idx, ok = flat.clamp(0, M - 1), (flat >= 0) & (flat < M)
    idx, ok = idx.to(x.device), ok.to(x.device)
    return (x[idx] * ok[:, :, None]).reshape(x.shape[0], -1)


def patch_maxima(c, x_amax):
    idx, ok = _neighbours(c)
    return (x_amax[idx.to(x_amax.device)] * ok.to(x_amax.device)).amax(1)


# pd_conv3x3_wgrad_nhwc_f16x2: dWk[co][tap][ci] += sum_p dY[p][co] X[p + off(tap)][ci], dB[co] += sum_p dY[p][co]: the weight gradient above
# with `patches(X)` as its second operand (one power of two per operand, as there).  wide: pd_gemm_wgrad_f16x2_takes_wide_tiles(Co, 9 Ci) and
# Ci % 256 == 0
ConvWg = collections.namedtuple("ConvWg", "B H W Ci Co seed amax wide indexing", defaults=("both", False, False))
CONV_WGRAD = [ConvWg(2, 5, 7, 128, 8, 3401), ConvWg(1, 3, 20, 128, 132, 3402, amax="y"), ConvWg(2, 6, 6, 256, 132, 3403, amax="x", wide=True),
              ConvWg(1, 1, 5, 128, 4, 3404, amax="none", indexing=True)]          # (five pixels: at most five terms per output)


def conv_wg_id(c):
    return f"convwg{c.B}x{c.H}x{c.W}-{c.Ci}to{c.Co}-{c.amax}"


def conv_wg_operands(c):
    """dY [B H W, Co], X [B H W, Ci] as Op, the maxima handed over, the pre-fills of dWk [Co, 9 Ci] and dB [Co]"""
    M = c.B * c.H * c.W
    dy, x, ya, xa, dw0, db0 = wg_operands(Wg(M, c.Co, c.Ci, c.seed, amax=c.amax))
    g = torch.Generator().manual_seed(c.seed + 3)
    scale = float(dw0.abs()[dw0 != 0].min())
    dw0 = (torch.randint(-64, 65, (c.Co, 9 * c.Ci), generator=g).double() * scale).float()
    return dy, x, ya, xa, dw0, db0


def wg_narrow_plan(c):
    """(output tiles, row slices) of the 128-tile weight gradient (wgrad_x3_launch in csrc/gemm_x3.hip): one round of 512 workgroups, slices of
    at least 64 rows in stages of 16.  With two slices or more and tiles x slices x 128 x 128 workspace floats the partial tiles go
    through the workspace and a reduce kernel; with fewer floats, or none, through atomics."""
    tiles = -(-c.K // 128) * -(-c.N // 128)
    splits = 1 if tiles >= 512 else (512 + tiles // 2) // tiles
    chunk = max(-(-(-(-c.M // splits)) // 16) * 16, 64)
    return tiles, -(-c.M // chunk)
