"""A numpy restatement of the WINDOW RULE of the LDS-window MSDA backward kernels (partdistillation_amd/csrc/msda.hip:
msda_bwd_owner4_d32, msda_bwd_tiled_d32) and the inputs of tests/test_msda_windows_gpu.py — test infrastructure only.

The kernels cut the unit square into G x G tiles, G = min(16, ceil(max level dimension / 16)).  Tile (ty, tx) owns, at a level of
H x W pixels, the queries of rows [ty H / G, (ty + 1) H / G) and columns [tx W / G, (tx + 1) W / G) (integer division), and caches
of every destination level the window of rows [max(0, ty H / G - 5), min(H, (ty + 1) H / G + 5)), clipped to 26 cells — likewise
in x.  A sample point whose 2 x 2 bilinear footprint is not wholly inside its tile's window is a MISS: the launch gate of
pd_msda_backward counts them.  Nothing here reads the kernels; the numerical reference of the gradients is the C oracle."""
import numpy as np
import torch

TILE, GMAX, HALO5, WIN5, CELLS5, HALO9, WIN9, CELLS9 = 16, 16, 5, 26, 1200, 9, 34, 2330
D, P = 32, 4


def grid(shapes):
    return min(GMAX, (max(max(int(h), int(w)) for h, w in shapes) + TILE - 1) // TILE)


def level_starts(shapes):
    out, s = [], 0
    for h, w in shapes:
        out.append(s)
        s += int(h) * int(w)
    return out, s


def window(n, t, G, halo=HALO5, win=WIN5):
    """-> (first cell, number of cells) of tile row / column t's window along an axis of n cells"""
    lo = max(0, t * n // G - halo)
    return lo, max(0, min(min(n, (t + 1) * n // G + halo) - lo, win))


def windows_fit(shapes, halo=HALO5, win=WIN5, cells=CELLS5):
    """every tile's windows of all levels fit the kernel's LDS budget (otherwise a level gets no window: every sample at it misses)"""
    G = grid(shapes)
    return all(sum(window(int(h), ty, G, halo, win)[1] * window(int(w), tx, G, halo, win)[1] for h, w in shapes) <= cells
               for ty in range(G) for tx in range(G))


def query_tiles(shapes):
    """-> (tile [S] = ty * G + tx of every query, claims [S] = how many tiles claim it: the kernels need exactly one)"""
    G = grid(shapes)
    starts, S = level_starts(shapes)
    tile = np.full(S, -1, dtype=np.int64)
    claims = np.zeros(S, dtype=np.int64)
    for (h, w), s0 in zip(shapes, starts):
        h, w = int(h), int(w)
        for ty in range(G):
            for tx in range(G):
                ys, xs = np.arange(ty * h // G, (ty + 1) * h // G), np.arange(tx * w // G, (tx + 1) * w // G)
                q = (s0 + ys[:, None] * w + xs[None, :]).reshape(-1)
                tile[q] = ty * G + tx
                claims[q] += 1
    return tile, claims


def _low_corner(loc, shapes):
    """fp32, as the kernels: -> in_range [N, S, M, L, P], h_low, w_low (int64; meaningful where in_range)"""
    loc = np.asarray(loc, dtype=np.float32)
    H = np.asarray([h for h, _ in shapes], dtype=np.float32).reshape(1, 1, 1, -1, 1)
    W = np.asarray([w for _, w in shapes], dtype=np.float32).reshape(1, 1, 1, -1, 1)
    with np.errstate(invalid="ignore"):
        h_im, w_im = loc[..., 1] * H - np.float32(0.5), loc[..., 0] * W - np.float32(0.5)
        ok = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
    h_low = np.floor(np.where(ok, h_im, 0)).astype(np.int64)
    w_low = np.floor(np.where(ok, w_im, 0)).astype(np.int64)
    return ok, h_low, w_low


def count_misses(shapes, loc):
    """loc [N, S, M, L, P, 2] (x, y), num_query == S -> (missed, looked-at): the sample points inside the map whose 2 x 2 footprint
    (what of it lies on the map) leaves the halo-5 window of their query's tile, among all N S M L P.  Exactly what a gated launch
    publishes when every sample has four corners inside the map and four non-zero bilinear weights (a corner outside the map, or
    one of weight zero, is treated differently by the halo-5 and the halo-9 kernel) and every tile's windows fit the LDS budget
    (windows_fit)."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    G = grid(shapes)
    tile, _ = query_tiles(shapes)
    ok, h_low, w_low = _low_corner(loc, shapes)
    N, S, M, L, Pn = ok.shape
    ty, tx = tile // G, tile % G
    inside = np.zeros_like(ok)
    for l, (h, w) in enumerate(shapes):
        wy = np.asarray([window(h, t, G) for t in range(G)])          # [G, 2]
        wx = np.asarray([window(w, t, G) for t in range(G)])
        y0, hh = wy[ty, 0].reshape(1, S, 1, 1), wy[ty, 1].reshape(1, S, 1, 1)
        x0, ww = wx[tx, 0].reshape(1, S, 1, 1), wx[tx, 1].reshape(1, S, 1, 1)
        hl, wl = h_low[:, :, :, l], w_low[:, :, :, l]
        ins = np.ones_like(ok[:, :, :, l])
        for dy in (0, 1):
            for dx in (0, 1):
                y, x = hl + dy, wl + dx
                exists = (y >= 0) & (y < h) & (x >= 0) & (x < w)          # a corner outside the map is never added anywhere
                ins &= ~exists | ((y >= y0) & (y < y0 + hh) & (x >= x0) & (x < x0 + ww))
        inside[:, :, :, l] = ins
    return int((ok & ~inside).sum()), int(ok.size)


def touched_cells(shapes, loc, queries=None, head=None):
    """-> bool [N, S]: the value cells (pixels of the concatenated levels) that a corner, inside the map, of a sample of the given
    queries (bool [S]; default all) lands on, over all heads or for one head"""
    shapes = [(int(h), int(w)) for h, w in shapes]
    starts, S = level_starts(shapes)
    ok, h_low, w_low = _low_corner(loc if head is None else np.asarray(loc)[:, :, head:head + 1], shapes)
    N = ok.shape[0]
    out = np.zeros((N, S), dtype=bool)
    sel = np.ones(S, dtype=bool) if queries is None else np.asarray(queries, dtype=bool)
    for l, (h, w) in enumerate(shapes):
        for dy in (0, 1):
            for dx in (0, 1):
                y, x = h_low[:, :, :, l][:, sel] + dy, w_low[:, :, :, l][:, sel] + dx          # [N, selected, M, P]
                m = ok[:, :, :, l][:, sel] & (y >= 0) & (y < h) & (x >= 0) & (x < w)
                for b in range(N):
                    out[b, starts[l] + (y[b][m[b]] * w + x[b][m[b]])] = True
    return out


# ----------------------------------------------------------------------------------------------------------------- test inputs
def _ref_points(shapes):
    """the encoder's reference points: the normalised pixel centre of every query, [S, 2] (x, y), float64"""
    pts = []
    for h, w in shapes:
        ys, xs = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij")
        pts.append(np.stack((xs.reshape(-1), ys.reshape(-1)), -1))
    return np.concatenate(pts)


def _pack(shapes, N, M, value, off, logits, gout):
    """-> the raw form pd_msda_fused_* takes (oa = offsets in pixels | logits, reference points) with value and grad_out"""
    starts, S = level_starts(shapes)
    L = len(shapes)
    ref = torch.from_numpy(_ref_points(shapes)).float()[None, :, None, :].expand(N, S, L, 2).reshape(N * S, L, 2).contiguous()
    oa = torch.cat([off.reshape(N * S, -1), logits.reshape(N * S, -1)], 1).contiguous()
    return dict(value=value, shapes=torch.as_tensor(shapes, dtype=torch.long), lvl=torch.as_tensor(starts, dtype=torch.long), oa=oa,
                ref=ref, gout=gout, dims=(N, S, M, D, L, P))


def loc_attn(case):
    """sampling locations and attention probabilities the raw form stands for (tests/test_msda_gpu.py:_loc_attn)"""
    from test_msda_gpu import _loc_attn
    return _loc_attn(case["oa"], case["ref"], case["shapes"], case["dims"])


# section A: (shapes, N, M); two offset regimes each, (spread in cells, seed)
BRANCH_CASES = [
    ([(16, 16), (8, 8), (4, 4)], 1, 3),              # 3 (6) active workgroups: the block decode that is not XCD-chunked
    ([(16, 16), (8, 8), (4, 4)], 3, 4),              # batch > 1, 12 workgroups
    ([(24, 20), (12, 10), (6, 5)], 2, 8),            # other sizes, G = 2, chunked decode
    ([(40, 40), (40, 40), (40, 40)], 1, 2),          # the windows exceed the LDS budget: levels without a window
    ([(272, 4), (136, 2), (68, 1)], 1, 1),           # G capped at 16; tiles that own no query of a level
    ([(2, 3), (1, 1), (1, 2)], 2, 5),                # degenerate levels
]
REGIMES = [(1.0, 0), (12.0, 1)]
TILED_LEVELS = {1: [(8, 8)], 2: [(8, 8), (4, 4)], 4: [(8, 8), (8, 8), (4, 4), (2, 2)], 8: [(8, 8), (8, 8), (4, 4), (4, 4), (2, 2), (2, 2), (1, 1), (1, 1)]}
NONFINITE_SHAPES = [(24, 24), (12, 12), (6, 6)]


def case_seed(i, regime):
    """seeds for which the fp32 oracle meets the fp64 oracle at the tests' tolerances with no element left out
    (tests/test_msda_window_oracle_cpu.py).  On the 272-row map y * H is rounded to 3e-5 cells in fp32, which alone moves grad_attn
    by up to the tolerance: seed 1041 leaves one element out there, 3041 stays at 0.43 of it."""
    return {(4, 1): 3041}.get((i, regime), 1000 + 10 * i + regime)


def random_case(shapes, N, M, spread, seed):
    """offsets ~ N(0, spread) cells of the destination level around the query's own pixel centre (so they leave [0, 1] near the
    borders and, at 12 cells, nearly everywhere on small maps), softmax attention.  A sample closer than 1e-3 cells to a cell
    border is moved 4e-3 cells: there grad_loc is a one-sided derivative and the side depends on the last bit."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    _, S = level_starts(shapes)
    L = len(shapes)
    g = torch.Generator().manual_seed(seed)
    value = torch.randn(N, S, M, D, generator=g)
    off = torch.randn(N * S, M, L, P, 2, generator=g, dtype=torch.float64) * spread
    logits = torch.randn(N * S, M, L * P, generator=g) * 2.0
    gout = torch.randn(N, S, M * D, generator=g)
    wh = torch.as_tensor([(w, h) for h, w in shapes], dtype=torch.float64).view(1, 1, L, 1, 2)
    ref = torch.from_numpy(_ref_points(shapes)).repeat(N, 1).view(N * S, 1, 1, 1, 2)
    im = ref * wh + off - 0.5
    fr = im - im.floor()
    off = torch.where((fr < 1e-3) | (fr > 1 - 1e-3), off + 4e-3, off).float()
    return _pack(shapes, N, M, value, off, logits, gout)


def grad_misses(name, got, want):
    """the tolerances of test_backward_config2_geometry_offset_distributions_vs_c_oracle -> fraction of elements outside them:
    grad_value within 2e-5 of the tensor's maximum; grad_loc / grad_attn within rtol 1e-4 + 1e-5 of the maximum"""
    want = want.to(got.device)
    scale = want.abs().max()
    bound = (2e-5 if name == "grad_value" else 1e-5) * scale + (0.0 if name == "grad_value" else 1e-4) * want.abs()
    return (~((got - want).abs() <= bound)).double().mean().item()


def assert_grads(got3, want3, what=""):
    for name, got, want in zip(("grad_value", "grad_loc", "grad_attn"), got3, want3):
        frac = grad_misses(name, got, want)
        # grad_loc is a one-sided derivative for samples within rounding distance of a cell border: 1e-5 of them may differ
        assert frac <= (1e-5 if name == "grad_loc" else 0.0), (what, name, frac, (got - want.to(got.device)).abs().max().item(), want.abs().max().item())


# ------------------------------------------------------------------------------------------------ section B: exact inputs
PYR, EQ3 = [(16, 16), (8, 8), (4, 4)], [(16, 16), (16, 16), (16, 16)]
FIXED_POINT_CASES = ["a3", "unit12", "eq768", "eq768_wide", "onehot336", "mixed"]
FIXED_POINT_FUSED = ["eq768", "eq768_wide", "onehot336"]        # what a softmax can express


def precondition(attn):
    """attn [1, S, M, L, P] of a one-tile case -> (max |a|, the largest sum |a| over a head's samples): the kernels keep their
    fixed-point windows while the first is <= 1 and the second <= 511 (include/pd_msda.h)"""
    return attn.abs().max().item(), attn.abs().sum((0, 1, 3, 4)).max().item()


def fixed_point_case(name, M=2):
    """grad_out in {+-1, +-0.5} (x 1.75 in eq768_wide), every sample on a pixel centre (one bilinear weight 1, three 0), weights
    that are small dyadic numbers: every sum of the reference is exact in fp32.  One image; both pyramids have G = 1, i.e. one tile.
      a3         weight 3 on one sample per query, 0 elsewhere; targets spread over the maps
      unit12     weight 1 on all 12 samples; the 4 level-0 samples of all 336 queries on ONE cell (1344 unit weights)
      eq768      three 16 x 16 levels, one-hot weights, all 768 queries on one cell of level 0
      eq768_wide the same with |grad_out| in {1.75, 0.875}: the largest scaled contribution, 0.875 x 2^22 (a maximum of exactly
                 1 leaves a factor 2 of headroom in the scale, which hides a bound exceeded by less than that)
      onehot336  one-hot weights on 16 / 8 / 4, all 336 queries on one cell: inside the bound
      mixed      weights in {0, +-1/32, +-1/16, +-1/8} on all samples (they sum to ~250 in absolute value per head: inside the
                 bound, so negative weights go through the int32 windows), random signs of grad_out, targets spread
    -> the raw form (logits = None where a softmax cannot produce the weights), loc, attn"""
    shapes = EQ3 if name.startswith("eq768") else PYR
    starts, S = level_starts(shapes)
    L, N = 3, 1
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    value = torch.randn(N, S, M, D, generator=g)
    q = torch.arange(S).view(S, 1, 1, 1)
    l = torch.arange(L).view(1, 1, L, 1)
    p = torch.arange(P).view(1, 1, 1, P)
    hw = torch.as_tensor(shapes).view(1, 1, L, 1, 2)
    t = (q * 7 + p * 3 + l + torch.arange(M).view(1, M, 1, 1) * 5) % (hw[..., 0] * hw[..., 1])
    cy, cx = t // hw[..., 1], t % hw[..., 1]
    if name != "a3" and name != "mixed":
        cy[:, :, 0], cx[:, :, 0] = 5, 9
    ref = torch.from_numpy(_ref_points(shapes)).view(S, 1, 1, 1, 2)
    wh = torch.stack((hw[..., 1], hw[..., 0]), -1).double()
    off = (torch.stack((cx, cy), -1).double() + 0.5 - ref * wh).float()       # pixels; ref + off / (W, H) is the target's centre, exactly
    attn = torch.zeros(S, M, L, P)
    if name == "a3":
        attn[:, :, 0, 0] = 3.0
    elif name == "unit12":
        attn[:] = 1.0
    elif name == "mixed":
        k = torch.randint(0, 7, (S, M, L, P), generator=g) - 3
        attn = k.sign() * torch.tensor([0.0, 1 / 32, 1 / 16, 1 / 8])[k.abs()]
    else:
        attn[:, :, 0, 0] = 1.0
    c = torch.arange(M * D).view(1, M * D)
    mag = torch.where((torch.arange(S).view(S, 1) + c) % 8 == 0, 0.5, 1.0)
    sign = torch.where(c % 3 == 0, -1.0, 1.0).expand(S, M * D)
    if name == "mixed":
        sign = torch.randint(0, 2, (S, M * D), generator=g).float() * 2 - 1
    gout = (mag * sign * (1.75 if name == "eq768_wide" else 1.0)).view(N, S, M * D).contiguous()
    logits = torch.where(attn > 0, 0.0, -1.0e4) if name in FIXED_POINT_FUSED else torch.zeros(S, M, L, P)
    case = _pack(shapes, N, M, value, off, logits, gout)
    loc, a_soft = loc_attn(case)
    im = loc.double() * wh.view(1, 1, 1, L, 1, 2) - 0.5
    assert (im == im.round()).all() and (im >= 0).all() and (im < wh.view(1, 1, 1, L, 1, 2)).all()      # pixel centres inside the maps, exactly
    if name in FIXED_POINT_FUSED:
        assert torch.equal(a_soft, attn.view(N, S, M, L, P))
    else:
        case["oa"] = None
    return case, loc, attn.view(N, S, M, L, P).contiguous()


# ------------------------------------------------------------------------------------------------ section C: gate inputs
def aimed_case(shapes, N, M, aim, seed):
    """every sample at pixel centre + (0.25, 0.25) cells of a cell whose 2 x 2 footprint is inside the map (all four corners exist,
    all four weights are non-zero: the halo-5 and the halo-9 kernel count the same misses).
      aim = "home": the cell under the query's own reference point — zero offsets up to that quarter cell: no sample leaves a window
      aim = "far" : the far corner (H - 2, W - 2) of every level: all but the last tiles' samples leave their windows"""
    shapes = [(int(h), int(w)) for h, w in shapes]
    _, S = level_starts(shapes)
    L = len(shapes)
    g = torch.Generator().manual_seed(seed)
    value = torch.randn(N, S, M, D, generator=g)
    logits = torch.randn(N * S, M, L * P, generator=g)
    gout = torch.randn(N, S, M * D, generator=g)
    ref = torch.from_numpy(_ref_points(shapes)).view(S, 1, 1, 1, 2)
    wh = torch.as_tensor([(w, h) for h, w in shapes], dtype=torch.float64).view(1, 1, L, 1, 2)
    if aim == "home":
        cell = torch.minimum((ref * wh).floor(), wh - 2).clamp_min(0)
    else:
        cell = (wh - 2).expand(S, 1, L, 1, 2)
    off = (cell + 0.75 - ref * wh).expand(S, M, L, P, 2).float()
    return _pack(shapes, N, M, value, off.repeat(N, 1, 1, 1, 1).contiguous(), logits, gout)
