"""Cases for the Swin window-attention kernels (include/pd_window_attention.h): an fp64 oracle of one launch written from the reference's
formulas (modeling/backbone/swin.py:110-125 the relative_position_index, :146-173 the attention body, :425-441 the shifted-window mask, added
as -100), the magnitude companions that turn "bf16 rounding" into a bound for EVERY element, the same math with the kernels' documented
roundings inserted (to prove the bounds can be met), and the named, seeded inputs of tests/test_window_attention_edges_gpu.py.
tests/test_window_attention_cases_cpu.py proves the oracle, the bounds and each case's named property without a GPU.

Layouts are the kernels': qkv [B_, 144, 3 C] (q of head h at column 32 h, k at C + 32 h, v at 2 C + 32 h), out / d_out [B_, 144, C],
table / dtable [529, heads], lse [B_, heads, 144] in BASE 2, window of row b is b % nW.

Bounds, with u = 2^-8 the bf16 unit roundoff.  The kernels round: P to bf16 before P.V and before P^T.dO; scale * dS to bf16 before the dQ and
dK products; delta = rowsum(dO * out) is formed from the bf16 `out`; every output once to bf16; dtable comes from the unrounded fp32 dS;
everything else is fp32.  With E_i = sum_d |dO_id| |out_id| (what an error of u in `out` does to delta) and W = scale * (P o E + |dS|):
    out  : (1 + 2^-4) u (P |V| + |out|)            dV : (1 + 2^-4) u (P^T |dO| + |dV|)
    dQ   : (1 + 2^-4) u (W |K| + |dQ|)             dK : (1 + 2^-4) u (W^T |Q| + |dK|)
    dT[t]: u sum_{idx = t} P_ij E_i + 2^-20 sum_{idx = t} |dS_ij|
    lse  : 2^-18 (log2(e) max_j (scale sum_d |q_d| |k_jd| + |T| + |M|) + 1)
each + 1e-30 where the result may be flushed to zero.  The 2^-4 covers the u^2 terms and the fp32 accumulation; 2^-18 is 64 fp32 ulps of the
score magnitude (a 32-term dot product, two roundings of the table, exp2 / log2, the final add)."""
import math

import torch

WS, N, D, TBL = 12, 144, 32, 529
SCALE = D ** -0.5
LOG2E = 1.0 / math.log(2.0)
U = 2.0 ** -8
HEADROOM = 1.0 + 2.0 ** -4
FLOOR = 1e-30
TENSORS = ("out", "lse", "dq", "dk", "dv", "dt")


# ------------------------------------------------------------------------------------------------ the reference's index and mask
def relative_position_index():
    """int64 [144, 144], built step by step as the reference builds its buffer (:114-124)"""
    coords = torch.stack(torch.meshgrid(torch.arange(WS), torch.arange(WS), indexing="ij")).flatten(1)       # 2, 144
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()                            # 144, 144, 2
    rel[:, :, 0] += WS - 1
    rel[:, :, 1] += WS - 1
    rel[:, :, 0] *= 2 * WS - 1
    return rel.sum(-1)


def n_windows(H, W):
    return (-(-H // WS)) * (-(-W // WS))


def reference_mask(H, W, shift):
    """fp64 [nW, 144, 144], 0 / -100: the padded grid painted with nine region labels, cut into windows, labels subtracted (:425-441)"""
    Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS
    img = torch.zeros((1, Hp, Wp, 1), dtype=torch.float64)
    cnt = 0
    for hs in (slice(0, -WS), slice(-WS, -shift), slice(-shift, None)):
        for wsl in (slice(0, -WS), slice(-WS, -shift), slice(-shift, None)):
            img[:, hs, wsl, :] = cnt
            cnt += 1
    mw = img.view(1, Hp // WS, WS, Wp // WS, WS, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1, N)
    am = mw.unsqueeze(1) - mw.unsqueeze(2)
    return am.masked_fill(am != 0, -100.0).masked_fill(am == 0, 0.0)


# ------------------------------------------------------------------------------------------------ the fp64 oracle
def _heads_of(x, heads):                                    # [B_, 144, heads * 32] -> [B_, heads, 144, 32]
    return x.double().reshape(x.shape[0], N, heads, D).transpose(1, 2)


def _rows_of(x):                                            # back
    return x.transpose(1, 2).reshape(x.shape[0], N, -1)


def _table_sum(x):
    """[B_, heads, 144, 144] -> [529, heads]: entry t = the sum over windows and over the pairs whose relative_position_index is t"""
    heads = x.shape[1]
    out = torch.zeros(heads, TBL, dtype=torch.float64)
    out.index_add_(1, relative_position_index().view(-1), x.sum(0).reshape(heads, N * N))
    return out.t().contiguous()


def scores(qkv, table, H, W, shift, scale=SCALE, mask_value=-100.0):
    """q, k, v [B_, heads, 144, 32], the raw scores scale q k^T + T[idx] and the additive mask (both [B_, heads, 144, 144] or broadcastable),
    |T[idx]| — all fp64, natural units"""
    heads = table.shape[1]
    B_, nW = qkv.shape[0], n_windows(H, W)
    assert B_ % nW == 0 and qkv.shape[2] == 3 * heads * D
    q, k, v = (_heads_of(t, heads) for t in qkv.double().view(B_, N, 3, heads * D).unbind(2))
    bias = table.double()[relative_position_index().view(-1)].view(N, N, heads).permute(2, 0, 1)
    raw = scale * (q @ k.transpose(-1, -2)) + bias.unsqueeze(0)
    if shift:
        m = reference_mask(H, W, shift)
        if mask_value != -100.0:
            m = torch.where(m != 0, torch.full_like(m, mask_value), m)
        m = m.repeat(B_ // nW, 1, 1).unsqueeze(1)                                   # window of row b is b % nW
    else:
        m = torch.zeros(1, 1, N, N, dtype=torch.float64)
    return q, k, v, raw, m, bias.abs().unsqueeze(0)


def oracle(qkv, table, d_out, H, W, shift, scale=SCALE, mask_value=-100.0):
    """fp64 results of one launch and their magnitude companions (module docstring): out, lse (base 2), dq, dk, dv, dt and c_out, c_lse,
    c_dq, c_dk, c_dv, c_dt, a_dt, all in the kernels' layouts.  `mask_value` is the reference's -100; -inf gives the hard mask."""
    heads = table.shape[1]
    q, k, v, raw, m, abs_bias = scores(qkv, table, H, W, shift, scale, mask_value)
    s = raw + m
    p = torch.softmax(s, -1)
    out = p @ v
    lse = LOG2E * torch.logsumexp(s, -1)
    do = _heads_of(d_out, heads)
    dv = p.transpose(-1, -2) @ do
    delta = (do * out).sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(-1, -2) - delta)
    dq = scale * (ds @ k)
    dk = scale * (ds.transpose(-1, -2) @ q)
    e = (do.abs() * out.abs()).sum(-1, keepdim=True)
    w = scale * (p * e + ds.abs())
    finite_m = torch.where(torch.isinf(m), torch.full_like(m, 100.0), m.abs())
    c_lse = LOG2E * (scale * (q.abs() @ k.abs().transpose(-1, -2)) + abs_bias + finite_m).amax(-1) + 1.0
    return dict(out=_rows_of(out), lse=lse, dq=_rows_of(dq), dk=_rows_of(dk), dv=_rows_of(dv), dt=_table_sum(ds),
                c_out=_rows_of(p @ v.abs() + out.abs()), c_lse=c_lse, c_dv=_rows_of(p.transpose(-1, -2) @ do.abs() + dv.abs()),
                c_dq=_rows_of(w @ k.abs() + dq.abs()), c_dk=_rows_of(w.transpose(-1, -2) @ q.abs() + dk.abs()),
                c_dt=_table_sum(p * e), a_dt=_table_sum(ds.abs()))


def bounds(ref):
    """the per-element bound of every tensor of TENSORS"""
    b = {n: HEADROOM * U * ref["c_" + n] + FLOOR for n in ("out", "dq", "dk", "dv")}
    b["dt"] = U * ref["c_dt"] + 2.0 ** -20 * ref["a_dt"] + FLOOR
    b["lse"] = 2.0 ** -18 * ref["c_lse"]
    return b


def ratios(got, ref, extra=None):
    """{tensor: max over its elements of |got - ref| / bound} (inf for a non-finite result); `extra` adds to the bound of named tensors"""
    r = {}
    for n, bound in bounds(ref).items():
        g = got[n].double().cpu()
        assert g.shape == ref[n].shape, (n, g.shape, ref[n].shape)
        if extra and n in extra:
            bound = bound + extra[n]
        r[n] = ((g - ref[n]).abs() / bound).max().item() if torch.isfinite(g).all() else float("inf")
    return r


def split_dqkv(dqkv):
    """dq, dk, dv [B_, 144, C] of a [B_, 144, 3 C] gradient"""
    return dqkv.view(dqkv.shape[0], N, 3, -1).unbind(2)


# ------------------------------------------------------------------------------------------------ the kernels' roundings in fp64
def _bf(x):
    return x.float().bfloat16().double()


def emulate(qkv, table, d_out, H, W, shift, scale=SCALE):
    """The oracle's math in fp64 with the kernels' documented roundings inserted and nothing else: the forward rounds exp(s - max) to bf16
    for the P.V product (normalising by the unrounded sum afterwards) and `out` to bf16; the backward recomputes P from lse, takes delta from
    the bf16 `out`, rounds P (for dV) and scale * dS (for dQ, dK) to bf16, sums the unrounded dS into dtable, and rounds dq, dk, dv to bf16.
    -> dict(out, lse, dq, dk, dv, dt)"""
    heads = table.shape[1]
    q, k, v, raw, m, _ = scores(qkv, table, H, W, shift, scale)
    s = raw + m
    mx = s.amax(-1, keepdim=True)
    e = torch.exp(s - mx)
    l = e.sum(-1, keepdim=True)
    out = _bf((_bf(e) @ v) / l)
    lse = mx + torch.log(l)
    p = torch.exp(s - lse)
    do = _heads_of(d_out, heads)
    delta = (do * out).sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(-1, -2) - delta)
    dsb = _bf(scale * ds)
    return dict(out=_rows_of(out), lse=(LOG2E * lse.squeeze(-1)).float().double(), dq=_rows_of(_bf(dsb @ k)),
                dk=_rows_of(_bf(dsb.transpose(-1, -2) @ q)), dv=_rows_of(_bf(_bf(p).transpose(-1, -2) @ do)), dt=_table_sum(ds))


# ------------------------------------------------------------------------------------------------ the named cases
#                 heads images  H   W  shift  q,k std  table std
CASES = {
    "one_window":        (1, 1, 12, 12, 0, 1.0, 0.5),        # B_ = 1, no mask: every table entry, the four corners (one pair each) included
    "mixed_flags":       (3, 1, 24, 24, 6, 1.0, 0.5),        # nW = 4: window 0 has one region (unflagged), the other three are flagged
    "ragged_masked":     (2, 2, 25, 40, 6, 1.0, 0.5),        # padded 36 x 48 grid, nW = 12, B_ = 24
    "wide_masked":       (2, 1, 24, 24, 6, 3.0, 4.0),        # + constructed rows whose best cross-region score beats every same-region one by > 100
    "peaky":             (4, 1, 12, 12, 0, 6.0, 8.0),        # |lse| > 150, near one-hot rows
    "bias_only_plain":   (2, 1, 24, 24, 0, 0.0, 4.0),        # q = k = 0: P is the softmax of the gathered table alone
    "bias_only_shifted": (2, 1, 24, 24, 6, 0.0, 4.0),
    "heads48":           (48, 1, 24, 24, 6, 1.0, 0.5),       # Swin-L stage-4 width, C = 1536
    "chunk_plain":       (2, 7, 12, 12, 0, 1.0, 0.5),        # B_ = 7, nW = 1 (the chunk sweep)
    "chunk_masked":      (2, 3, 24, 24, 6, 1.0, 0.5),        # B_ = 12, nW = 4 (the chunk sweep)
}
WIDE_FACTOR = 8.0                                            # the planted key is this multiple of its query


def wide_rows(heads=2):
    """(window, head, query, key) of the rows `wide_masked` constructs: in every flagged window of the 24 x 24, shift 6 grid and every head,
    a query and a key of ANOTHER region (different queries and keys per head and window, so that they land in different lanes and tiles)"""
    m = reference_mask(24, 24, 6)
    rows = []
    for w in range(m.shape[0]):
        if not (m[w] != 0).any():
            continue
        for h in range(heads):
            i = 5 + 37 * w + 16 * h
            cross = torch.nonzero(m[w, i] != 0).view(-1)
            rows.append((w, h, i, int(cross[-1 - 3 * h])))
    return rows


def build(name):
    """-> dict(qkv bf16 [B_, 144, 3 C], table fp32 [529, heads], d_out bf16 [B_, 144, C], heads, images, H, W, shift, nW, scale), on the CPU,
    seeded by the case's position in CASES"""
    heads, images, H, W, shift, std, tstd = CASES[name]
    g = torch.Generator().manual_seed(4100 + list(CASES).index(name))
    nW = n_windows(H, W)
    B_, C = images * nW, heads * D
    qkv = torch.randn(B_, N, 3, C, generator=g)
    qkv[:, :, :2] *= std
    table = torch.randn(TBL, heads, generator=g) * tstd
    d_out = torch.randn(B_, N, C, generator=g).bfloat16()
    qkv = qkv.bfloat16()
    if name == "wide_masked":
        for w, h, i, j in wide_rows(heads):
            qkv[w, j, 1, h * D:(h + 1) * D] = WIDE_FACTOR * qkv[w, i, 0, h * D:(h + 1) * D]                  # (a power of two: exact in bf16)
    return dict(qkv=qkv.view(B_, N, 3 * C).contiguous(), table=table.contiguous(), d_out=d_out, heads=heads, images=images, H=H, W=W,
                shift=shift, nW=nW, scale=SCALE)


def oracle_of(case, **kw):
    return oracle(case["qkv"], case["table"], case["d_out"], case["H"], case["W"], case["shift"], case["scale"], **kw)
