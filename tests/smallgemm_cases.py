"""Exact cases for the skinny-activation bf16 GEMMs (include/pd_smallgemm.h).

Operands are integer-valued bf16 (uniform integers in [-8, 8]; bias and accumulate-base in [-128, 128]), so every product and
every partial sum is an integer below 2^24: exact in fp32 in ANY summation order (the MFMA's, the split forms' slice order,
wgrad_reduce's).  The only rounding a kernel performs is the final fp32 -> bf16 one, and the expected result is the float64
reference rounded once, `expected(ref64)`, which the kernel must match bit for bit (`bits()`).
tests/test_smallgemm_cases_cpu.py proves that each case rounds (and ties) often enough for that to mean something and that
planted defects change the expected bits; tests/test_smallgemm_exact_gpu.py runs the kernels on them.

Every matrix the GPU test hands to a kernel is a window of a larger allocation (`Guarded`): leading dimension larger than the
width, rows after it, a block in front of it.  Inputs are surrounded by bf16 NaN (one missing bounds guard or zero-fill turns the
output into NaN instead of slightly wrong), outputs by a sentinel bit pattern that is compared afterwards."""
import collections

import torch

OPERAND = 8                 # operands: integers in [-OPERAND, OPERAND]
ADDEND = 128                # bias / accumulate-base: integers in [-ADDEND, ADDEND]
EXACT_LIMIT = 1 << 24       # integers below this are exact in fp32

NAN16 = 0x7FC0              # bf16 quiet NaN
SENTINEL16 = 0x5A5B         # a finite bf16 (about 1.5e16) no exact case can produce
SENTINEL32 = 0x5A5B5C5D     # the same idea for fp32 / int32 buffers (about 1.5e16 as fp32)

Case = collections.namedtuple("Case", "kind form M N K seed")

# kind tn: Y[M,N] = X[M,K] W[N,K]^T, contraction K.  `form` is the kernel body the dispatcher of smallgemm.hip picks for the shape:
#   K <= 256 -> sgemm_tn_k256; otherwise chunked sgemm_tn (K / 64 chunks: 5 = odd, last chunk in LDS buffer 0; 6 = even);
#   splitk (K % 256 == 0, >= 512) is a separate entry point: 2 and 3 slices.
# Shapes: ragged 32-row tile (33, 65, 7), ragged 128-column tile that ends on 4 and not on 8 (132, 260), more than one tile each way.
TN = [
    Case("tn", "k256", 33, 132, 192, 101),
    Case("tn", "k256", 7, 16, 64, 112),
    Case("tn", "k256", 33, 132, 256, 103),
    Case("tn", "chunked", 33, 132, 320, 104),
    Case("tn", "chunked", 33, 132, 384, 105),
    Case("tn", "splitk", 33, 132, 512, 106),
    Case("tn", "splitk", 65, 260, 768, 107),
]
# kind nn: dX[M,K] (+)= dY[M,N] W[N,K], contraction N.  N <= 256 -> sgemm_nn_n256; otherwise chunked sgemm_nn; splitn as above.
NN = [
    Case("nn", "n256", 33, 192, 132, 201),
    Case("nn", "n256", 7, 64, 24, 212),
    Case("nn", "chunked", 33, 320, 132, 203),
    Case("nn", "chunked", 33, 384, 260, 204),
    Case("nn", "splitn", 33, 512, 132, 205),
    Case("nn", "splitn", 65, 768, 260, 206),
]
# kind wgrad: dW[N,K] = dY[M,N]^T X[M,K], dB[N] = column sums of dY, contraction M.
WGRAD = [
    Case("wgrad", "single", 70, 40, 264, 301),
    Case("wgrad", "single", 65, 36, 132, 302),
    Case("wgrad", "single", 1, 8, 8, 303),
    Case("wgrad", "single", 0, 36, 132, 304),
]
# pd_sgemm_wgrad_split_bf16: N % 64 == 0 -> the 64-wide tile kernel, otherwise the 32-wide one.  (257, 64, 136): two slices of 192 and
# 65 rows, the second slice's last 64-row chunk holds one row.  (257, 72, 4): N tail of 8, K = 4.
WGRAD_SPLIT = [
    Case("wgrad", "split64", 257, 64, 136, 311),
    Case("wgrad", "split32", 257, 72, 4, 312),
    Case("wgrad", "split32", 513, 36, 132, 313),
    Case("wgrad", "split64", 1, 64, 136, 314),
]
# the 130 small problems of the grouped launch (one seed each, 400 + i) are built by wgrad_operands(Case("wgrad", "grouped", 5, 8, 8, 400 + i))
GROUPED_SMALL = [Case("wgrad", "grouped", 5, 8, 8, 400 + i) for i in range(130)]
# pd_sgemm_tn_batched_bf16 (per problem seeds 600 + b) and pd_sgemm_tn_multi_bf16 (four problems, one K = 192)
BATCHED = [Case("tn", "batched", 33, 132, 192, 600 + b) for b in range(3)]
MULTI = [Case("tn", "multi", 33, 132, 192, 611), Case("tn", "multi", 0, 64, 192, 612), Case("tn", "multi", 200, 516, 192, 613),
         Case("tn", "multi", 7, 16, 192, 614)]
MULTI_BIAS = (True, False, True, False)

ALL = TN + NN + WGRAD + WGRAD_SPLIT + GROUPED_SMALL[:2] + BATCHED + MULTI
INDEXING_ONLY = {(1, 8, 8), (1, 64, 136)}      # one-row weight gradients: they test indexing, their products need no rounding


def case_id(c):
    return f"{c.form}-{c.M}x{c.N}x{c.K}"


def contraction(c):
    return {"tn": c.K, "nn": c.N, "wgrad": c.M}[c.kind]


# ------------------------------------------------------------------------------------------------ operands
def ints(shape, bound, seed):
    """integer-valued bf16, uniform in [-bound, bound], from a seeded CPU generator"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-bound, bound + 1, shape, generator=g).to(torch.bfloat16)


def tn_operands(c):
    """x [M,K], w [N,K], bias [N]"""
    return ints((c.M, c.K), OPERAND, c.seed), ints((c.N, c.K), OPERAND, c.seed + 1000), ints((c.N,), ADDEND, c.seed + 2000)


def relu_mask_operand(shape, seed):
    """what the ReLU whose gradient is taken produced or saw: negative and positive values and both +0.0 and -0.0 (every second zero),
    which are masked.  No subnormals."""
    h = ints(shape, 3, seed).flatten()
    z = (h == 0).nonzero().flatten()
    h[z[1::2]] = -0.0
    return h.view(shape)


def nn_operands(c):
    """dy [M,N], w [N,K], base [M,K] (what accumulate adds to), mask operand [M,K]"""
    return (ints((c.M, c.N), OPERAND, c.seed), ints((c.N, c.K), OPERAND, c.seed + 1000), ints((c.M, c.K), ADDEND, c.seed + 2000),
            relu_mask_operand((c.M, c.K), c.seed + 3000))


def wgrad_operands(c):
    """dy [M,N], x [M,K]"""
    return ints((c.M, c.N), OPERAND, c.seed), ints((c.M, c.K), OPERAND, c.seed + 1000)


# ------------------------------------------------------------------------------------------------ float64 references
# `+ 0.0` turns a -0.0 of the float64 product into +0.0: the kernels accumulate onto +0.0, which no sum of products leaves.
def ref_tn(x, w, bias=None, relu=False):
    r = x.double() @ w.double().t()
    if bias is not None:
        r = r + bias.double()
    if relu:
        r = r.relu()
    return r + 0.0


def ref_nn(dy, w, base=None, mask=None, mask_ge=False):
    """masked entries are exactly 0, base included (the gradient of a ReLU that was off).  mask_ge: the planted `>= 0` defect."""
    r = dy.double() @ w.double()
    if base is not None:
        r = r + base.double()
    if mask is not None:
        on = (mask.double() >= 0) if mask_ge else (mask.double() > 0)
        r = torch.where(on, r, torch.zeros_like(r))
    return r + 0.0


def ref_wgrad(dy, x):
    return dy.double().t() @ x.double() + 0.0


def ref_db(dy):
    return dy.double().sum(0) + 0.0


def magnitude(c):
    """the largest sum of |a||b| (+ |addend|) of the case: every partial sum, in any order, is bounded by it"""
    if c.kind == "tn":
        x, w, b = tn_operands(c)
        return float((x.double().abs() @ w.double().abs().t() + b.double().abs()).max()) if c.M else 0.0
    if c.kind == "nn":
        dy, w, base, _ = nn_operands(c)
        return float((dy.double().abs() @ w.double().abs() + base.double().abs()).max())
    dy, x = wgrad_operands(c)
    return max(float((dy.double().abs().t() @ x.double().abs()).max()), float(dy.double().abs().sum(0).max())) if c.M else 0.0


# ------------------------------------------------------------------------------------------------ the one rounding, and wrong ones
def expected(ref64):
    """float64 reference -> bf16, rounded once to nearest, ties to even"""
    return ref64.float().to(torch.bfloat16)


def bits(t):
    """bf16 -> int16 bit patterns (fp32 -> int32): comparisons are bit for bit"""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _from_hi16(hi):
    return hi.to(torch.int16).view(torch.bfloat16)        # hi: the sign-extended upper half of the fp32 pattern, in [-2^15, 2^15)


def truncated(ref64):
    """planted defect: fp32 -> bf16 by dropping the low 16 bits"""
    return _from_hi16(ref64.float().view(torch.int32).to(torch.int64) >> 16)


def half_away(ref64):
    """planted defect: ties away from zero (add half an ulp to the magnitude, truncate)"""
    return _from_hi16((ref64.float().view(torch.int32).to(torch.int64) + 0x8000) >> 16)


def is_tie(ref64):
    """exactly half way between two bf16 neighbours"""
    return (ref64.float().view(torch.int32) & 0xFFFF) == 0x8000


def is_rounded(ref64):
    return expected(ref64).double() != ref64


# ------------------------------------------------------------------------------------------------ guarded buffers
class Guarded:
    """`batch` windows [rows, cols] inside one larger allocation: leading dimension ld = cols rounded up to 8, + pad (pad % 8 == 0: a multiple of 8 above the width;
    pad % 8 == 4 for the one operand whose ld may be a multiple of 4 only, the weight gradient),
    window b at row b * (rows + gap), at least `tail` rows after the last one, a guard block of `front` elements in front of the base
    (which stays 16-byte aligned).  Everything outside the windows holds `fill` (a bit pattern); intact() compares it bit for bit.
      .t / .w[b]  the window(s) as tensors of `dtype` (stride(0) == ld)      .ptr   address of window 0      .stride   elements per problem"""

    def __init__(self, rows, cols, dtype, fill, device, pad=8, tail=32, front=64, batch=1, gap=8):
        size = torch.empty((), dtype=dtype).element_size()
        assert size in (2, 4) and pad % 4 == 0 and pad > 0 and (front * size) % 16 == 0
        idt = torch.int16 if size == 2 else torch.int32
        if fill >= 1 << (8 * size - 1):
            fill -= 1 << (8 * size)
        self.fill, self.rows, self.cols, self.batch = fill, rows, cols, batch
        self.ld = (cols + 7) // 8 * 8 + pad
        self.stride = (rows + gap) * self.ld
        total_rows = batch * (rows + gap) + tail
        self.raw = torch.full((front + total_rows * self.ld,), fill, dtype=idt, device=device)
        body = self.raw[front:].view(total_rows, self.ld)
        inside = torch.zeros(self.raw.shape, dtype=torch.bool, device=device)
        ins = inside[front:].view(total_rows, self.ld)
        self.w = []
        for b in range(batch):
            r0 = b * (rows + gap)
            ins[r0:r0 + rows, :cols] = True
            self.w.append(body[r0:r0 + rows, :cols].view(dtype))
        self.outside = ~inside
        self.t = self.w[0]
        self.ptr = self.raw.data_ptr() + front * size
        assert self.ptr % 16 == 0

    @classmethod
    def of(cls, value, fill, device, **kw):
        """a window holding `value` ([rows, cols], or [batch, rows, cols] with batch=...)"""
        if kw.get("batch", 1) > 1:
            g = cls(value.shape[1], value.shape[2], value.dtype, fill, device, **kw)
            for w, v in zip(g.w, value):
                w.copy_(v)
        else:
            g = cls(value.shape[0], value.shape[1], value.dtype, fill, device, **kw)
            g.t.copy_(value)
        return g

    def intact(self):
        """nothing outside the windows was written"""
        return bool((self.raw[self.outside] == self.fill).all())

    def untouched(self):
        """nothing at all was written, the windows included"""
        return bool((self.raw == self.fill).all())

    def snapshot(self):
        return self.raw.clone()

    def same_as(self, snap):
        return torch.equal(self.raw, snap)
