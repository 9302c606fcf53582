"""Cases for the masked-attention kernels (include/pd_attention.h): an fp64 reference that defines the blocked-row semantics, named
structured masks that kill whole tiles / key halves / chunks / rows, and inputs whose logits span far more than exp() can hold in fp32.
tests/test_attention_cases_cpu.py proves each case has the property it is named for; tests/test_attention_edges_gpu.py runs them.

Layouts are the kernels': q [Lq, B, H*32], k / v [Lk, B, H*32], mask bool [B, Lq, Lk] with True = blocked, lse [B, H, Lq]."""
import math

import torch

D = 32
SCALE = D ** -0.5
TILE = 32                  # keys per score tile of the matrix-core kernels (the scalar kernels stage 64 and give each key half of 32 to a thread)


def reference(q, k, v, mask, H, scale=SCALE):
    """fp64 attention on the inputs as given (bf16 inputs are upcast: the operand rounding is shared with the kernel).
    Returns (o [Lq, B, H*32], lse [B, H, Lq]).  A row with every key blocked — or with no key at all — is DEFINED as o = 0, lse = -inf and
    contributes nothing to any gradient; gradients come from autograd through this function."""
    Lq, B, C = q.shape
    Lk, d = k.shape[0], C // H
    qh = q.double().reshape(Lq, B, H, d).permute(1, 2, 0, 3)
    kh = k.double().reshape(Lk, B, H, d).permute(1, 2, 0, 3)
    vh = v.double().reshape(Lk, B, H, d).permute(1, 2, 0, 3)
    s = qh @ kh.transpose(-1, -2) * scale
    if mask is not None:
        s = s.masked_fill(mask[:, None], float("-inf"))
    if Lk > 0:
        m = s.detach().amax(-1, keepdim=True)
    else:
        m = s.new_full((B, H, Lq, 1), float("-inf"))
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)          # the shift is a constant: the result does not depend on it
    e = torch.exp(s - m)                                             # blocked: exp(-inf) = 0, with a zero derivative
    l = e.sum(-1, keepdim=True)
    live = l > 0
    l1 = torch.where(live, l, torch.ones_like(l))
    p = e / l1                                                       # a blocked row: all zeros
    o = (p @ vh).permute(2, 0, 1, 3).reshape(Lq, B, C)
    lse = torch.where(live, m + torch.log(l1), torch.full_like(l, float("-inf"))).squeeze(-1)
    return o, lse


# ------------------------------------------------------------------------------------------------ structured masks
# Every builder returns bool [B, Lq, Lk], True = blocked.  `t` is the tile size (32), `kc` the chunk size where the pattern has one.

def _rows(B, Lq, row):
    return row[None, None, :].expand(B, Lq, -1).clone()


def only_last_key(B, Lq, Lk, t=TILE, kc=None):
    """only key Lk-1 is open: every earlier tile and chunk is dead, and the first open key sits in the last (partial) tile"""
    row = torch.ones(Lk, dtype=torch.bool)
    row[Lk - 1] = False
    return _rows(B, Lq, row)


def only_first_key(B, Lq, Lk, t=TILE, kc=None):
    """everything after key 0 is blocked: the running maximum is set by the first tile and every later tile and chunk is dead"""
    row = torch.ones(Lk, dtype=torch.bool)
    row[0] = False
    return _rows(B, Lq, row)


def upper_half_of_tiles(B, Lq, Lk, t=TILE, kc=None):
    """only keys 32..63 of each 64-key tile are open: in the scalar kernels the first key half is dead in every tile"""
    return _rows(B, Lq, (torch.arange(Lk) % (2 * t)) < t)


def hi_lanes(B, Lq, Lk, t=TILE, kc=None):
    """only keys 4..7 of every group of 8 are open: the hh = 1 lanes of the matrix-core score tile"""
    return _rows(B, Lq, (torch.arange(Lk) % 8) < 4)


def alternate_chunks(B, Lq, Lk, t=TILE, kc=256):
    """chunks of kc keys alternately dead and open; even rows start dead, odd rows start open (all rows open where Lk <= kc: one chunk)"""
    dead_first = ((torch.arange(Lk) // kc) % 2) == 0
    m = _rows(B, Lq, dead_first)
    m[:, 1::2] = ~dead_first
    if Lk <= kc:
        m[:] = False
    return m


def dead_then_live(B, Lq, Lk, t=TILE, kc=None):
    """the first ceil(Lk / 2) keys are blocked"""
    return _rows(B, Lq, torch.arange(Lk) < (Lk + 1) // 2)


def live_then_dead(B, Lq, Lk, t=TILE, kc=None):
    """the first ceil(Lk / 2) keys are the only open ones"""
    return _rows(B, Lq, torch.arange(Lk) >= (Lk + 1) // 2)


def blocked_row(B, Lq, Lk, t=TILE, kc=None):
    """every key blocked"""
    return torch.ones(B, Lq, Lk, dtype=torch.bool)


def grid_of(Lk):
    """(h, w) with h * w = Lk and h the largest divisor <= sqrt(Lk) (a prime Lk is a 1 x Lk strip)"""
    h = max(a for a in range(1, int(math.isqrt(Lk)) + 1) if Lk % a == 0)
    return h, Lk // h


def image_like(B, Lq, Lk, t=TILE, kc=None, seed=0):
    """one random axis-aligned rectangle open per row on the h x w key grid (h * w = Lk): the decoder's `mask_logit < 0` on an image is
    spatially coherent like this — runs of open keys one grid row apart, everything else (most chunks) dead"""
    h, w = grid_of(Lk)
    g = torch.Generator().manual_seed(1000 + seed)
    y0 = torch.randint(0, h, (B, Lq), generator=g)
    x0 = torch.randint(0, w, (B, Lq), generator=g)
    hh = torch.randint(1, max(2, h // 2 + 1), (B, Lq), generator=g)
    ww = torch.randint(1, max(2, w // 4 + 1), (B, Lq), generator=g)
    ys, xs = torch.arange(h)[None, None, :, None], torch.arange(w)[None, None, None, :]
    y0, x0, hh, ww = (a[:, :, None, None] for a in (y0, x0, hh, ww))
    open_ = (ys >= y0) & (ys < y0 + hh) & (xs >= x0) & (xs < x0 + ww)         # clipped at the border, never empty: (y0, x0) is inside
    return ~open_.reshape(B, Lq, Lk)


BUILDERS = {f.__name__: f for f in (only_last_key, only_first_key, upper_half_of_tiles, hi_lanes, alternate_chunks, dead_then_live,
                                    live_then_dead, blocked_row, image_like)}
NAMES = tuple(BUILDERS)


def pattern_of(b, i):
    """the builder whose row (b, i) the mixed mask takes: consecutive rows carry consecutive patterns, images start at different ones"""
    return NAMES[(i + 4 * b) % len(NAMES)]


def mixed(B, Lq, Lk, kc=256, t=TILE):
    """row (b, i) of the mask is row (b, i) of the builder pattern_of(b, i): one call carries every pattern (from 9 rows on)"""
    full = {n: f(B, Lq, Lk, t=t, kc=kc) for n, f in BUILDERS.items()}
    m = torch.empty(B, Lq, Lk, dtype=torch.bool)
    for b in range(B):
        for i in range(Lq):
            m[b, i] = full[pattern_of(b, i)][b, i]
    return m


def blocked_rows_of(B, Lq):
    """bool [B, Lq]: the rows of mixed() that are fully blocked"""
    return torch.tensor([[pattern_of(b, i) == "blocked_row" for i in range(Lq)] for b in range(B)])


# ------------------------------------------------------------------------------------------------ wide-range inputs
WIDE = ("ascending", "descending", "scrambled")
LOGIT_STD = 6.0


def tile_offsets(kind, Lk, t=TILE):
    """fp64 [ceil(Lk / t)]: what the logit of every key of a 32-key tile gains"""
    n = (Lk + t - 1) // t
    if kind == "ascending":                                     # every tile dominates everything before it
        return torch.linspace(-90.0, 90.0, n, dtype=torch.float64) if n > 1 else torch.tensor([90.0], dtype=torch.float64)
    if kind == "descending":                                    # the first tile dominates; later tiles shrink to nothing
        return tile_offsets("ascending", Lk, t).flip(0)
    if kind == "scrambled":                                     # the running maximum goes up several times, by 30 or 60 each time
        return 30.0 * ((7 * torch.arange(n, dtype=torch.float64)) % 5 - 2)
    raise ValueError(kind)


def wide_inputs(kind, Lq, Lk, B, H, dtype, seed=0):
    """q, k, v, d_o (CPU, already rounded to `dtype`): randn scaled so that q.k * 32**-0.5 has a standard deviation of ~6, then channel 0 of
    every query is sqrt(32) and channel 0 of key j is off[j // 32], so the scaled logit of key j gains the offset of its tile."""
    g = torch.Generator().manual_seed(77 + seed)
    C = H * D
    amp = math.sqrt(LOGIT_STD)
    q = torch.randn(Lq, B, C, generator=g) * amp
    k = torch.randn(Lk, B, C, generator=g) * amp
    v = torch.randn(Lk, B, C, generator=g)
    d_o = torch.randn(Lq, B, C, generator=g)
    off = tile_offsets(kind, Lk)[torch.arange(Lk) // TILE].float()
    q.view(Lq, B, H, D)[..., 0] = math.sqrt(D)
    k.view(Lk, B, H, D)[..., 0] = off[:, None, None]
    return tuple(a.to(dtype) for a in (q, k, v, d_o))


def unit_inputs(Lq, Lk, B, H, dtype, seed=0):
    """q, k, v, d_o (CPU, rounded to `dtype`): unit randn, the existing tests' inputs"""
    g = torch.Generator().manual_seed(5 + seed)
    C = H * D
    return tuple(torch.randn(n, B, C, generator=g).to(dtype) for n in (Lq, Lk, Lk, Lq))


def scaled_logits(q, k, H, scale=SCALE):
    """fp64 [B, H, Lq, Lk]"""
    Lq, B, C = q.shape
    Lk = k.shape[0]
    qh = q.double().reshape(Lq, B, H, D).permute(1, 2, 0, 3)
    kh = k.double().reshape(Lk, B, H, D).permute(1, 2, 0, 3)
    return qh @ kh.transpose(-1, -2) * scale


# ------------------------------------------------------------------------------------------------ properties (used by the CPU tests)
def dead_chunk_rows(mask, kc):
    """bool [B, Lq]: rows with at least one chunk of kc keys fully blocked although the row as a whole is not"""
    B, Lq, Lk = mask.shape
    n = (Lk + kc - 1) // kc
    pad = torch.ones(B, Lq, n * kc, dtype=torch.bool)
    pad[:, :, :Lk] = mask
    dead = pad.view(B, Lq, n, kc).all(-1)
    return dead.any(-1) & ~dead.all(-1)


def first_open_key(mask):
    """int64 [B, Lq]: index of the first open key, Lk for a fully blocked row"""
    Lk = mask.shape[-1]
    idx = torch.where(mask, torch.full((1,), Lk), torch.arange(Lk))
    return idx.amin(-1) if Lk else torch.zeros(mask.shape[:2], dtype=torch.long)


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic in plain torch
def working_precision(q, k, v, d_o, mask, H, scale=SCALE, matrix_core=False):
    """The same formulas at the precision the kernels work at, in plain torch: fp32 throughout, results rounded to the inputs' dtype, the
    backward recomputing p = exp(s - lse) and taking delta = rowsum(dO * O) from the ROUNDED o as every flash-style backward does; with
    `matrix_core`, P and dS are rounded to bf16 before the second products.  Its deviation from reference() is the error the number
    formats themselves force on these inputs — what a tolerance for them is derived from.  Returns dict(o, lse, dq, dk, dv)."""
    Lq, B, C = q.shape
    Lk, dt = k.shape[0], q.dtype
    heads = lambda a, n: a.float().reshape(n, B, H, D).permute(1, 2, 0, 3)              # noqa: E731
    back = lambda a, n: a.permute(2, 0, 1, 3).reshape(n, B, C)                          # noqa: E731
    rnd = (lambda a: a.bfloat16().float()) if matrix_core else (lambda a: a)
    qh, kh, vh, gh = heads(q, Lq), heads(k, Lk), heads(v, Lk), heads(d_o, Lq)
    s = qh @ kh.transpose(-1, -2) * scale
    if mask is not None:
        s = s.masked_fill(mask[:, None], float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    live = l > 0
    l1 = torch.where(live, l, torch.ones_like(l))
    o = ((rnd(e) @ vh) / l1).to(dt)
    lse = torch.where(live, m + torch.log(l1), torch.full_like(l, float("inf")))       # +inf: p = exp(s - inf) = 0 for a blocked row
    p = torch.exp(s - lse)
    delta = (gh * o.float()).sum(-1, keepdim=True)
    ds = p * (gh @ vh.transpose(-1, -2) - delta)
    p, ds = rnd(p), rnd(ds)
    dq, dk, dv = ds @ kh * scale, ds.transpose(-1, -2) @ qh * scale, p.transpose(-1, -2) @ gh
    lse = torch.where(live, lse, torch.full_like(l, float("-inf"))).squeeze(-1)
    return dict(o=back(o, Lq), lse=lse, dq=back(dq, Lq).to(dt), dk=back(dk, Lk).to(dt), dv=back(dv, Lk).to(dt))
