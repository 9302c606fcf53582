"""Exact cases for the bf16 implicit-GEMM family and its weight gradients (include/pd_igemm.h: pd_igemm_bf16, pd_igemm_bf16_seq,
pd_filter_transpose_grouped, pd_wgrad_bf16, pd_wgrad_bf16_seq).  The instrument is tests/smallgemm_cases.py's (imported, not copied).

Operands are integer-valued bf16 in [-8, 8] (`operand()`: magnitudes 5..8 with a random sign, so that a contraction of 64 terms already
leaves the range bf16 holds exactly), bias / res / res2 / the dB base integers in [-128, 128], scale / row_scale drawn from
{-2, -1, -0.5, 0.5, 1, 2}.  Every product and every partial sum is exact in fp32 in any order (the largest contraction is
9 x 320 = 2 880 terms: |sum| <= 184 320, x 2 + 3 x 128 < 2^24), so the only rounding a kernel performs is the final fp32 -> bf16 one
and the result must equal the float64 reference rounded once, `expected(ref64)`, bit for bit; -0.0 sums are normalised (`+ 0.0`) as
smallgemm_cases does (pd_wgrad_bf16's row_scale multiplies the finished sum: a zero sum times a negative scale is the -0.0 IEEE
gives, in the kernel and in the reference).  The references are float64 on the CPU: F.conv2d in double and its autograd for the input gradient.
`gemm_view()` is a second, tap-by-tap float64 form of the same sums (the header's GEMM view); tests/test_igemm_cases_cpu.py proves that
it equals the first and plants the defects a loose tolerance hides into it.

GELU and GELU' results cannot be exact.  They must satisfy
    |got - ref64| <= GELU_REL |ref64| + GELU_ABS max(|x|, 1),      GELU_REL = 2^-8, GELU_ABS = 2e-6,
x the pre-activation (the gate value for GELU'; the larger of the two when a launch has both).  The first term is the one rounding to
bf16.  The second is derived, not measured: csrc/gelu.h documents an absolute error of 1.5e-7 of its erfc (Abramowitz & Stegun
7.1.26); the reciprocal (rcpf) and the exponential (__expf) it is built from each add a few fp32 ulps (6e-8) to a value of at most 1;
Phi and phi are then multiplied by x.  2e-6 is about ten times 1.5e-7 and covers both.  `out_pre` of the same launch stays bit-exact.

Which kernel body a case reaches (csrc/igemm_bf16.hip, csrc/wgrad_bf16.hip; the GPU test forces the schedule with pd_debug_set):
  PLAIN x PLAIN_SCHEDULES   igemm_bf16<64 | 128, 1 | 2 | 3, P1 = true>: KT = 1, 2, 3, 5 K-steps under every ring depth
  SPLIT                     the same + splitk_seam<1> (64-wide tiles) and splitk_seam<2> (128-wide), forced and automatic
  FWD, DGRAD                igemm_bf16<64 | 128, 1 | 2 | 3, P1 = false>: the gathered forward (3 x 3 / 1 x 1 stride 2, 3 x 3 stride 1 under
                            ig_patch = 0; the 3 x 3 ones over 128 channels also split: splitk_seam behind a gathered contraction) and input
                            gradient (1 x 1, stride-2 1 x 1, the nine-tap walk on an odd grid and under ig_pcls = 0)
  PCLS                      igemm_bf16<64 | 128, 1 | 2 | 3, false> with parity classes (a.pcls = 1)
  PATCH                     igemm3x3_bf16 forward and input gradient, one chunk .. five chunks, + splitk_seam<1> over the channel chunks
  EPILOGUES                 igemm_epilogue.inc in igemm_bf16<64, 1, true>, <128, 1, true> (EPI_PIPE == false), the parity classes, igemm3x3_bf16
                            and behind splitk_seam<2>; out_col_slab on (130, 64, 256)
  SEQ                       pd_igemm_bf16_seq: a split plain-rows problem, a chunk-split patch problem, a parity-class problem
  TRANSPOSES                filter_transpose_grouped
  WGRAD x wg_nst x wg_splits   wgrad_bf16<1 | 2>, wgrad_bf16_reduce; WGRAD_SEQ: wgrad_bf16_reduce_grouped"""
import collections
import math

import torch
import torch.nn.functional as F

from smallgemm_cases import ADDEND, EXACT_LIMIT, expected, ints, relu_mask_operand

NAN32 = 0x7FC00000          # fp32 quiet NaN: what surrounds scale / bias / row_scale
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
GATE_NONE, GATE_RELU, GATE_GELU = 0, 1, 2
RES_DENSE, RES_UP2 = 0, 1
SCALES = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)
GELU_REL, GELU_ABS = 2.0 ** -8, 2e-6
BM, KSTEP, TILE, STAGE_ROWS = 128, 64, 128, 64      # igemm: rows per tile, channels per K-step; wgrad: tile edge, rows per stage

# H, W: the grid of the convolution's INPUT (the result grid of an input gradient); ci / co: its input / output channels
Geo = collections.namedtuple("Geo", "name B H W ci co k stride dgrad seed")


def rows(M, K, N, seed):
    """a Linear over M tokens: the plain-rows case"""
    return Geo(f"rows{M}x{K}x{N}", 1, M, 1, K, N, 1, 1, 0, seed)


def conv(B, H, W, ci, co, k, stride, dgrad, seed):
    return Geo(f"{'dgrad' if dgrad else 'fwd'}{k}x{k}s{stride}-{B}x{H}x{W}-{ci}to{co}", B, H, W, ci, co, k, stride, dgrad, seed)


def dims(g):
    """the PdIgemm geometry fields"""
    pad = g.k // 2
    Ho, Wo = (g.H + 2 * pad - g.k) // g.stride + 1, (g.W + 2 * pad - g.k) // g.stride + 1
    if g.dgrad:
        return dict(batch=g.B, hs=Ho, ws=Wo, cs=g.co, ho=g.H, wo=g.W, n=g.ci, k=g.k, stride=g.stride, pad=pad, dgrad=1)
    return dict(batch=g.B, hs=g.H, ws=g.W, cs=g.ci, ho=Ho, wo=Wo, n=g.co, k=g.k, stride=g.stride, pad=pad, dgrad=0)


def rows_of(g):
    d = dims(g)
    return d["batch"] * d["ho"] * d["wo"]


def contraction(g):
    d = dims(g)
    return d["k"] * d["k"] * d["cs"]


# ------------------------------------------------------------------------------------------------ the cases
# 1. plain rows (M, K, N): KT = 1, 2, 3, 5; one row, ragged tiles, three row tiles; 1, 2, 3, 4 column tiles of 64
PLAIN = [rows(1, 64, 64, 1101), rows(127, 128, 64, 1102), rows(130, 192, 128, 1103), rows(257, 320, 192, 1104), rows(130, 64, 256, 1105)]


def plain_schedules(g):
    return [dict(ig_bn=bn, ig_nst=nst) for bn in (64, 128) if bn == 64 or g.co % 128 == 0 for nst in (1, 2, 3)]


# 2. split-K seam: (case, knobs, the splits the plan must arrive at).  (130, 320, 128): KT = 5 -> 3 | 2 and 2 | 2 | 1; KT = 2 under 3 splits: clipped
SPLIT_GEO = rows(130, 320, 128, 1201)
SPLIT = [(SPLIT_GEO, dict(ig_splits=2, ig_bn=64), 2), (SPLIT_GEO, dict(ig_splits=2, ig_bn=128), 2), (SPLIT_GEO, dict(ig_splits=3, ig_bn=64), 3),
         (SPLIT_GEO, dict(ig_splits=3, ig_bn=128), 3), (rows(127, 128, 64, 1202), dict(ig_splits=3), 2), (rows(130, 128, 128, 1203), dict(ig_splits=3, ig_bn=128), 2),
         (rows(130, 1024, 64, 1204), dict(), 2)]

# 3. gathered forward, B = 2 (a row tile spans two images)
FWD = [conv(2, H, W, c, c, k, s, 0, 1300 + i) for i, (H, W, k, s, c) in enumerate(
    [(9, 11, 3, 2, 64), (10, 12, 3, 2, 64), (9, 11, 1, 2, 64), (10, 12, 1, 2, 64), (9, 17, 3, 1, 64),
     (9, 11, 3, 2, 128), (10, 12, 3, 2, 128), (9, 11, 1, 2, 128), (10, 12, 1, 2, 128), (9, 17, 3, 1, 128)])]


def gathered_knobs(g):
    """(3 x 3 stride 1: the gathered kernel; stride-2 3 x 3 input gradient on an even grid: the nine-tap walk)"""
    kn = {}
    if g.k == 3 and g.stride == 1:
        kn["ig_patch"] = 0
    if g.dgrad and g.k == 3 and g.stride == 2 and g.H % 2 == 0 and g.W % 2 == 0:
        kn["ig_pcls"] = 0
    return kn


def fwd_schedules(g):
    """64 channels: the plan's own schedule; 128: every ring depth under both tile widths"""
    if g.ci != 128:
        return [gathered_knobs(g)]
    return [dict(gathered_knobs(g), ig_bn=bn, ig_nst=nst) for bn in (64, 128) for nst in (1, 2, 3)]


# 4. gathered input gradient: co = 128 source channels -> ci = 64
DGRAD = [conv(2, 9, 11, 64, 128, 1, 1, 1, 1401), conv(2, 9, 11, 64, 128, 1, 2, 1, 1402), conv(2, 10, 12, 64, 128, 1, 2, 1, 1403),
         conv(2, 9, 11, 64, 128, 3, 2, 1, 1404), conv(2, 10, 12, 64, 128, 3, 2, 1, 1405), conv(2, 9, 17, 64, 128, 3, 1, 1, 1406)]

# 5. parity classes: 90 rows per class over two images | 144 rows per class: two tiles, the second ragged
PCLS = [conv(2, 10, 18, 128, 64, 3, 2, 1, 1501), conv(1, 24, 24, 128, 64, 3, 2, 1, 1502)]
PCLS_SCHEDULES = [dict(ig_bn=bn, ig_nst=nst) for bn in (64, 128) for nst in (1, 2, 3)]

# 6. patch form: every grid with every channel count, n alternating; forward AND input gradient of each
PATCH_GRIDS = [(1, 1, 1), (1, 8, 16), (1, 3, 40), (2, 9, 17)]
PATCH = [(conv(B, H, W, cs, (64, 128)[(i + j) % 2], 3, 1, 0, 1600 + 10 * i + j), conv(B, H, W, (64, 128)[(i + j) % 2], cs, 3, 1, 1, 1650 + 10 * i + j))
         for i, (B, H, W) in enumerate(PATCH_GRIDS) for j, cs in enumerate((64, 128, 192, 320))]
# forced chunk splits: (source channels, ig_splits, chunks per split the plan must arrive at)
PATCH_SPLIT = [(320, 2, (3, 2)), (320, 3, (2, 2, 1)), (192, 5, (1, 1, 1))]
PATCH_SPLIT_GRID = (2, 9, 17)


def patch_split_pair(cs, seed):
    B, H, W = PATCH_SPLIT_GRID
    return conv(B, H, W, cs, 64, 3, 1, 0, seed), conv(B, H, W, 128, cs, 3, 1, 1, seed + 50)


# 7. epilogue options.  bias: None | "f32" | "bf16"; res: None | "dense" | "up2"
Epi = collections.namedtuple("Epi", "scale bias res res2 pre act gate")
NO_EPI = Epi(False, None, None, False, False, ACT_NONE, GATE_NONE)
EPILOGUES = [
    Epi(True, "f32", "dense", True, True, ACT_RELU, GATE_RELU),
    Epi(True, "bf16", "up2", True, True, ACT_GELU, GATE_GELU),
    Epi(True, "f32", "up2", True, True, ACT_GELU, GATE_GELU),
    Epi(True, "bf16", "dense", True, True, ACT_RELU, GATE_RELU),
    Epi(True, "f32", "dense", True, True, ACT_GELU, GATE_GELU),
    Epi(True, "bf16", "up2", True, True, ACT_RELU, GATE_RELU),
    Epi(True, "f32", "dense", False, True, ACT_RELU, GATE_GELU),
    Epi(False, "bf16", "up2", True, False, ACT_GELU, GATE_RELU),
    Epi(False, "f32", None, False, False, ACT_NONE, GATE_NONE),
    Epi(False, None, "dense", False, False, ACT_NONE, GATE_NONE),
    Epi(False, None, "up2", False, False, ACT_RELU, GATE_NONE),
    Epi(False, None, None, True, False, ACT_NONE, GATE_NONE),
    Epi(False, None, None, False, False, ACT_NONE, GATE_RELU),
    Epi(True, None, None, False, True, ACT_GELU, GATE_NONE),
]


def epi_id(e):
    parts = ["scale"] * e.scale + ["bias" + (e.bias or "")] * bool(e.bias) + ["res" + (e.res or "")] * bool(e.res) + ["res2"] * e.res2 + ["pre"] * e.pre
    parts += [("", "relu", "gelu")[e.act]] * bool(e.act) + [("", "gaterelu", "gategelu")[e.gate]] * bool(e.gate)
    return "-".join(parts) or "bare"


def epi_options(e):
    """the options an epilogue has switched on (what must appear with every other at least once)"""
    return {o for o, on in (("scale", e.scale), ("bias_f32", e.bias == "f32"), ("bias_bf16", e.bias == "bf16"), ("res_dense", e.res == "dense"),
                            ("res_up2", e.res == "up2"), ("res2", e.res2), ("pre", e.pre), ("act_relu", e.act == ACT_RELU), ("act_gelu", e.act == ACT_GELU),
                            ("gate_relu", e.gate == GATE_RELU), ("gate_gelu", e.gate == GATE_GELU)) if on}


EXCLUSIVE = [{"bias_f32", "bias_bf16"}, {"res_dense", "res_up2"}, {"act_relu", "act_gelu"}, {"gate_relu", "gate_gelu"}]

# the problems the epilogues run on: (name, case, its sibling on an even grid for PD_IG_RES_UP2 — 130 rows have no even x even grid —, knobs)
_E_ROWS, _E_ROWS_EVEN = rows(130, 192, 128, 1701), conv(1, 6, 22, 192, 128, 1, 1, 0, 1702)
_E_SPLIT, _E_SPLIT_EVEN = rows(130, 320, 128, 1703), conv(1, 6, 22, 320, 128, 1, 1, 0, 1704)
EPI_BASES = [
    ("rows-bn64-nst1", _E_ROWS, _E_ROWS_EVEN, dict(ig_bn=64, ig_nst=1)),
    ("rows-bn128-nst1", _E_ROWS, _E_ROWS_EVEN, dict(ig_bn=128, ig_nst=1)),
    ("pcls", PCLS[0], PCLS[0], dict()),
    ("patch", conv(2, 9, 17, 128, 64, 3, 1, 0, 1705), conv(2, 10, 18, 128, 64, 3, 1, 0, 1706), dict()),
    ("split3-bn128", _E_SPLIT, _E_SPLIT_EVEN, dict(ig_splits=3, ig_bn=128)),
]
SLAB_GEO, SLABS = rows(130, 64, 256, 1707), (128, 256)


def epi_geo(base, e):
    return base[2] if e.res == "up2" else base[1]


# 8. one pd_igemm_bf16_seq call: a split plain-rows problem, a chunk-split patch problem, a parity-class problem (default schedule: the automatic splits)
SEQ = [(rows(130, 1024, 64, 1801), NO_EPI), (conv(2, 9, 17, 320, 64, 3, 1, 0, 1802), Epi(True, "f32", "dense", False, False, ACT_RELU, GATE_NONE)),
       (conv(2, 10, 18, 128, 64, 3, 2, 1, 1803), Epi(False, None, "dense", True, False, ACT_NONE, GATE_RELU))]

# 9. one pd_filter_transpose_grouped launch: (co, taps, ci, with scale)
TRANSPOSES = [(64, 9, 192, True), (192, 1, 64, False), (128, 9, 64, True), (64, 1, 64, False)]

# weight gradients (M, N, K): one row; a ragged stage; one row into the second stage; three stages, three column tiles of N; five stages, three of K
Wg = collections.namedtuple("Wg", "M N K seed")
WGRAD = [Wg(1, 8, 8, 1901), Wg(63, 72, 136, 1902), Wg(65, 136, 72, 1903), Wg(129, 264, 8, 1904), Wg(257, 64, 264, 1905)]
WG_NST, WG_SPLITS = (1, 2), (1, 2, 3, 7)
# (row_scale, db, dw_f32): each option on and off with each other one
WG_OPTIONS = [(False, False, False), (True, True, False), (True, False, True), (False, True, True)]
# pd_wgrad_bf16_seq: (case, wg-independent) five problems under wg_splits = 2: (1, 8, 8) and (63, ..) stay unsliced, the others are cut; both result types
WGRAD_SEQ = [(Wg(257, 64, 264, 1911), False), (Wg(1, 8, 8, 1912), True), (Wg(129, 264, 8, 1913), True), (Wg(63, 72, 136, 1914), False), (Wg(65, 136, 72, 1915), False)]
WGRAD_SEQ_SPLITS = 2

# cases whose products need too little rounding to say anything about it: they test indexing.  Contraction <= 64 (or a handful of results).
INDEXING_ONLY = {"rows1x64x64", "fwd3x3s1-1x1x1-64to64", "dgrad3x3s1-1x1x1-64to64", "wg1x8x8", "wg63x72x136"}


def wg_id(c):
    return f"wg{c.M}x{c.N}x{c.K}"


def wg_plan(c, wg_splits):
    """(slices, rows per slice) csrc/wgrad_bf16.hip's wg_plan arrives at under a forced wg_splits: slices beyond the 64-row stages collapse"""
    per = (-(-c.M // wg_splits) + STAGE_ROWS - 1) // STAGE_ROWS * STAGE_ROWS
    return -(-c.M // per), per


def wg_tiles(c):
    return -(-c.N // TILE) * -(-c.K // TILE)


# ------------------------------------------------------------------------------------------------ operands
def operand(shape, seed):
    """integer-valued bf16 in [-8, 8]: magnitude 5..8, random sign (variance 43.5: 64 products already sum to ~350, beyond the 256 up to which
    bf16 holds every integer)"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.randint(5, 9, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sign).to(torch.bfloat16)


def scales(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(SCALES, dtype=torch.float32)[torch.randint(0, len(SCALES), (n,), generator=g)]


def conv_operands(g):
    """src [batch, hs, ws, cs] (the input, or dz for an input gradient), w [co, k, k, ci] (the forward filter), wk: the filter as the kernel
    wants it ([n][taps][cs]: w itself, or its [ci][k][k][co] transpose for an input gradient)"""
    d = dims(g)
    src = operand((d["batch"], d["hs"], d["ws"], d["cs"]), g.seed)
    w = operand((g.co, g.k, g.k, g.ci), g.seed + 1000)
    return src, w, (w.permute(3, 1, 2, 0).contiguous() if g.dgrad else w)


def epi_operands(g, e):
    d = dims(g)
    M, n = rows_of(g), d["n"]
    o = {}
    if e.scale:
        o["scale"] = scales(n, g.seed + 2000)
    if e.bias:
        o["bias"] = ints((n,), ADDEND, g.seed + 3000).to(torch.float32 if e.bias == "f32" else torch.bfloat16)
    if e.res == "dense":
        o["res"] = ints((M, n), ADDEND, g.seed + 4000)
    if e.res == "up2":
        o["res"] = ints((d["batch"] * (d["ho"] // 2) * (d["wo"] // 2), n), ADDEND, g.seed + 4000)
    if e.res2:
        o["res2"] = ints((M, n), ADDEND, g.seed + 5000)
    if e.gate:
        o["gate"] = relu_mask_operand((M, n), g.seed + 6000)
    return o


def wg_operands(c):
    """dy [M, N], x [M, K], row_scale [N], the dB base [N]"""
    return (operand((c.M, c.N), c.seed), operand((c.M, c.K), c.seed + 1000), scales(c.N, c.seed + 2000),
            ints((c.N,), ADDEND, c.seed + 3000).float())


def transpose_operands(i):
    co, taps, ci, sc = TRANSPOSES[i]
    return ints((co, taps, ci), 8, 2001 + i), (scales(co, 2101 + i) if sc else None)


# ------------------------------------------------------------------------------------------------ float64 references
def ref_conv(g, src, w):
    """[rows, n] float64: F.conv2d in double, or its autograd for the input gradient"""
    pad = g.k // 2
    wd = w.double().permute(0, 3, 1, 2)
    if not g.dgrad:
        r = F.conv2d(src.double().permute(0, 3, 1, 2), wd, None, g.stride, pad)
    else:
        x = torch.zeros((g.B, g.ci, g.H, g.W), dtype=torch.float64, requires_grad=True)
        (r,) = torch.autograd.grad(F.conv2d(x, wd, None, g.stride, pad), x, src.double().permute(0, 3, 1, 2))
    return r.permute(0, 2, 3, 1).reshape(rows_of(g), -1) + 0.0


def gemm_view(g, src, wk, absolute=False, defect=None):
    """the header's GEMM view, tap by tap in float64: out[m][n] = sum_{tap, c} src[pixel(m, tap)][c] wk[n][tap][c];
    forward pixel = (oy stride + dy - pad, ..), input gradient pixel = ((iy + pad - dy) / stride, ..) where divisible.
    absolute: of |src| and |wk| (the bound of every partial sum).  defect (planted by the CPU test): ("tap", t) that tap dropped |
    "noflip" the input gradient walks the taps like a forward pass | "parity" the input gradient's divisibility taken from the other coordinate |
    "kstep" the last 64 channels of the last tap dropped"""
    d = dims(g)
    s, p, k = d["stride"], d["pad"], d["k"]
    S, Wk = src.double(), wk.double()
    if absolute:
        S, Wk = S.abs(), Wk.abs()
    oy, ox = torch.arange(d["ho"]), torch.arange(d["wo"])
    out = torch.zeros((d["batch"], d["ho"], d["wo"], d["n"]), dtype=torch.float64)
    for tap in range(k * k):
        if defect == ("tap", tap):
            continue
        dy, dx = divmod(tap, k)
        if d["dgrad"]:
            ey, ex = (k - 1 - dy, k - 1 - dx) if defect == "noflip" else (dy, dx)
            ty, tx = oy + p - ey, ox + p - ex
            sy, sx = torch.div(ty, s, rounding_mode="floor"), torch.div(tx, s, rounding_mode="floor")
            if defect == "parity":
                # (the rows' taps chosen by the parity of x and the columns' by that of y, as a class (cy, cx) read as (cx, cy) would)
                oky, okx = ((ox + p - ey) % s == 0)[None, :] & (ty >= 0)[:, None], ((oy + p - ex) % s == 0)[:, None] & (tx >= 0)[None, :]
            else:
                oky, okx = ((ty % s == 0) & (ty >= 0))[:, None], ((tx % s == 0) & (tx >= 0))[None, :]
        else:
            sy, sx = oy * s + dy - p, ox * s + dx - p
            oky, okx = (sy >= 0)[:, None], (sx >= 0)[None, :]
        ok = oky & okx & (sy < d["hs"])[:, None] & (sx < d["ws"])[None, :]
        patch = S[:, sy.clamp(0, d["hs"] - 1)][:, :, sx.clamp(0, d["ws"] - 1)] * ok[None, :, :, None]
        wt = Wk[:, dy, dx, :] if Wk.dim() == 4 else Wk[:, tap, :]
        if defect == "kstep" and tap == k * k - 1:
            patch, wt = patch[..., :-KSTEP], wt[:, :-KSTEP]
        out += patch @ wt.t()
    return out.reshape(rows_of(g), d["n"]) + 0.0


def gelu64(x):
    return x * 0.5 * torch.erfc(-x / math.sqrt(2.0))


def gelu_grad64(x):
    return 0.5 * torch.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def upsampled(g, res, everywhere=False):
    """the compact [batch, ho / 2, wo / 2, n] addend on the result grid: at even (y, x), zero elsewhere (everywhere: the planted defect)"""
    d = dims(g)
    r = res.double().view(d["batch"], d["ho"] // 2, d["wo"] // 2, d["n"])
    if everywhere:
        return r.repeat_interleave(2, 1).repeat_interleave(2, 2).reshape(-1, d["n"])
    up = torch.zeros((d["batch"], d["ho"], d["wo"], d["n"]), dtype=torch.float64)
    up[:, ::2, ::2] = r
    return up.reshape(-1, d["n"])


def ref_epilogue(g, e, acc, o, defect=None):
    """acc [rows, n] float64 -> dict(out, pre (the value before the activation), x (what the GELU tolerance scales with))
    defect: "res_odd" | "no_res2" | "gate_first" | "scale_after_bias" """
    v = acc
    bias = o["bias"].double() if e.bias else 0.0
    scale = o["scale"].double() if e.scale else 1.0
    v = (v + bias) * scale if defect == "scale_after_bias" else v * scale + bias
    if e.res == "dense":
        v = v + o["res"].double()
    if e.res == "up2":
        v = v + upsampled(g, o["res"], everywhere=defect == "res_odd")
    if e.res2 and defect != "no_res2":
        v = v + o["res2"].double()
    pre = v + 0.0

    def act(t):
        return t.relu() if e.act == ACT_RELU else gelu64(t) if e.act == ACT_GELU else t

    def gate(t):
        if e.gate == GATE_RELU:
            return torch.where(o["gate"].double() > 0, t, torch.zeros_like(t))
        return t * gelu_grad64(o["gate"].double()) if e.gate == GATE_GELU else t
    out = act(gate(pre)) if defect == "gate_first" else gate(act(pre))
    x = torch.ones_like(pre)
    if e.act == ACT_GELU:
        x = torch.maximum(x, pre.abs())
    if e.gate == GATE_GELU:
        x = torch.maximum(x, o["gate"].double().abs())
    return dict(out=out + 0.0, pre=pre, x=x)


def is_exact(e):
    return e.act != ACT_GELU and e.gate != GATE_GELU


def gelu_bound(ref, x):
    return GELU_REL * ref.abs() + GELU_ABS * x


def slabbed(ref, S, swapped=False):
    """[M, N] -> the [N / S, M, S] layout of out_col_slab (swapped: the planted defect, slab index and row exchanged)"""
    M, N = ref.shape
    r = ref.view(M, N // S, S)
    return r.contiguous() if swapped else r.permute(1, 0, 2).contiguous()


def ref_wgrad(c, dy, x, row_scale=None, drop_last_stage_of_slice=None):
    """dw [N, K] float64.  drop_last_stage_of_slice = wg_splits: the planted defect — the last 64-row stage of the first slice is not summed"""
    dyd, xd = dy.double(), x.double()
    if drop_last_stage_of_slice is not None:
        _, per = wg_plan(c, drop_last_stage_of_slice)
        end = min(per, c.M)
        keep = torch.ones(c.M, dtype=torch.bool)
        keep[(end - 1) // STAGE_ROWS * STAGE_ROWS:end] = False
        dyd = dyd[keep]
        xd = xd[keep]
    r = dyd.t() @ xd + 0.0                                   # the sum: accumulated onto +0.0
    if row_scale is not None:
        r = r * row_scale.double()[:, None]                    # a product, not a sum: a zero sum times a negative scale is -0.0, as IEEE has it
    return r


def ref_db(dy, base=None):
    r = dy.double().sum(0)
    return (r + base.double() if base is not None else r) + 0.0


def ref_transpose(w, scale):
    """[co, taps, ci] -> [ci, taps, co] (x scale[co]), bf16: a permutation, the products by +-0.5 / 1 / 2 are exact (no -0.0 normalisation:
    the kernel multiplies, it does not accumulate)"""
    r = w.double() if scale is None else w.double() * scale.double()[:, None, None]
    return expected(r.permute(2, 1, 0).contiguous())


def magnitude(g, e=None):
    """the largest sum of |a||b| (x the largest |scale|, + the addends) of the case: bounds every partial sum in any order"""
    src, _, wk = conv_operands(g)
    return float(gemm_view(g, src, wk, absolute=True).max()) * 2.0 + 3 * ADDEND


def wg_magnitude(c):
    dy, x, _, _ = wg_operands(c)
    return 2.0 * float((dy.double().abs().t() @ x.double().abs()).max()) + float(dy.double().abs().sum(0).max()) + ADDEND


def all_geos():
    """every distinct convolution / Linear problem the GPU test launches"""
    geos = list(PLAIN) + [s[0] for s in SPLIT] + FWD + DGRAD + PCLS + [g for pair in PATCH for g in pair]
    for cs, _, _ in PATCH_SPLIT:
        geos += list(patch_split_pair(cs, 1680 + cs))
    geos += list(patch_split_pair(320, 1690))
    for b in EPI_BASES:
        geos += [b[1], b[2]]
    geos += [SLAB_GEO] + [g for g, _ in SEQ]
    seen, out = set(), []
    for g in geos:
        if g not in seen:
            seen.add(g)
            out.append(g)
    return out


assert EXACT_LIMIT == 1 << 24
