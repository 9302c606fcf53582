"""Python faces of the set criterion's kernels (include/pd_criterion.h, csrc/criterion.hip): the Hungarian cost matrices of all (image,
head) problems in one pass, the BCE / dice losses of the matched masks at their points (with their gradient), and the selection of the
most uncertain oversampled points.  GPU only; the callers keep the plain torch expressions for CPU tensors (the oracle-side tests)."""
import os

import torch
from torch.autograd import Function

from .. import lib as _lib

_DT = {torch.float32: 0, torch.bfloat16: 2}
MAX_K = _lib.const("PD_UNCERTAIN_MAX_K")
ENABLED = __import__("os").environ.get("PD_CRITERION_KERNELS", "1") != "0"      # 0: the torch expressions (tools/ A/B runs)


def _stream():
    return _lib.current_stream()


def matcher_costs_supported(x, t, prob, labels):
    return (ENABLED and x.is_cuda and x.dtype in _DT and x.is_contiguous() and t.dtype == torch.float32 and t.stride(-1) == 1
            and prob.dtype == torch.float32 and labels.dtype == torch.int64)


def matcher_costs(x, t, prob, labels, heads, w_mask, w_class, w_dice):
    """x [B * heads, Q, n] point logits (bf16 / fp32), t [B, n_targets, heads, n] fp32 VIEW of the sampled target masks (any strides with a
    unit last one), prob [B * heads, Q, classes] fp32, labels [B, n_targets] int64 -> cost [B * heads, Q, n_targets] fp32
    (reference matcher.py:108-158)"""
    if not x.is_cuda:
        raise RuntimeError("pd_matcher_costs runs on the GPU only (no CPU fallback in partdistillation_amd)")
    problems, Q, n = x.shape
    B, nt = t.shape[0], t.shape[1]
    assert problems == B * heads and t.shape == (B, nt, heads, n) and t.stride(3) == 1 and labels.shape == (B, nt), (x.shape, t.shape, labels.shape)
    prob = prob.contiguous()
    labels = labels.contiguous()
    cost = torch.empty((problems, Q, nt), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().pd_matcher_costs(x.data_ptr(), _DT[x.dtype], t.data_ptr(), t.stride(0), t.stride(2), t.stride(1), prob.data_ptr(),
                                            labels.data_ptr(), cost.data_ptr(), problems, heads, Q, n, nt, prob.shape[-1], float(w_mask),
                                            float(w_class), float(w_dice), _stream()))
    return cost


MATCH_FUSED = os.environ.get("PD_MATCH_FUSED", "1") != "0"      # 0: sampler + batched product as two launches (A/B)


def match_point_logits_supported(mfeat, coords, emb):
    """mfeat [B, C, H, W] fp32 in channels-last memory, coords [B, heads * points, 2] fp32, emb [B * heads, Q, C] bf16 contiguous"""
    if not (ENABLED and MATCH_FUSED and mfeat.is_cuda and mfeat.dim() == 4 and emb.dim() == 3 and emb.dtype == torch.bfloat16 and emb.is_contiguous()):
        return False
    B, C, H, W = mfeat.shape
    if mfeat.dtype != torch.float32 or not mfeat.permute(0, 2, 3, 1).is_contiguous() or C != 256 or emb.shape[2] != C or emb.shape[1] > 128:
        return False
    heads = emb.shape[0] // max(B, 1)
    return heads * B == emb.shape[0] and coords.shape[0] == B and coords.shape[1] % heads == 0 and (coords.shape[1] // heads) % 4 == 0


def match_point_logits(mfeat, coords, emb):
    """-> [B * heads, Q, points] bf16: the logits of all Q masks of every (image, head) problem at its points, = emb . point_sample(mfeat)
    (pd_match_point_logits: reference matcher.py:108-125 through the linearity of point sampling; the sampled features stay on the CU).
    GPU only, no fallback."""
    if not mfeat.is_cuda:
        raise RuntimeError("pd_match_point_logits runs on the GPU only (no CPU fallback in partdistillation_amd)")
    B, C, H, W = mfeat.shape
    BH, Q, _ = emb.shape
    heads = BH // B
    coords = coords.float().contiguous()
    Pm = coords.shape[1] // heads
    out = torch.empty((BH, Q, Pm), dtype=torch.bfloat16, device=mfeat.device)
    _lib.check(_lib.load().pd_match_point_logits(mfeat.data_ptr(), coords.data_ptr(), emb.data_ptr(), out.data_ptr(), B, heads, Q, Pm, H, W, C, _stream()))
    return out


class MaskPointLosses(Function):
    """pl, labels [N, P] fp32 -> (bce [N] = mean over the points of BCE-with-logits, dice [N]); gradient with respect to pl only
    (reference criterion.py:25-69)"""

    @staticmethod
    def forward(ctx, pl, labels):
        if not pl.is_cuda:
            raise RuntimeError("pd_mask_point_losses runs on the GPU only (no CPU fallback in partdistillation_amd)")
        pl, labels = pl.contiguous(), labels.contiguous()
        N, P = pl.shape
        out = torch.empty((2, N), dtype=torch.float32, device=pl.device)
        stats = torch.empty((N, 3), dtype=torch.float32, device=pl.device)
        _lib.check(_lib.load().pd_mask_point_losses_fwd(pl.data_ptr(), labels.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), stats.data_ptr(),
                                                        N, P, _stream()))
        ctx.save_for_backward(pl, labels, stats)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, d_bce, d_dice):
        pl, labels, stats = ctx.saved_tensors
        N, P = pl.shape
        dx = torch.empty_like(pl)
        gb = d_bce.contiguous().float() if d_bce is not None else None
        gd = d_dice.contiguous().float() if d_dice is not None else None
        _lib.check(_lib.load().pd_mask_point_losses_bwd(pl.data_ptr(), labels.data_ptr(), stats.data_ptr(), gb.data_ptr() if gb is not None else None,
                                                        gd.data_ptr() if gd is not None else None, dx.data_ptr(), N, P, _stream()))
        return dx, None


def mask_point_losses_supported(pl, labels):
    return ENABLED and pl.is_cuda and pl.dtype == torch.float32 and labels.dtype == torch.float32 and pl.dim() == 2 and pl.shape == labels.shape and pl.shape[1] > 0


def mask_point_losses(pl, labels):
    return MaskPointLosses.apply(pl, labels)


def uncertain_points_supported(logits, coords, k):
    return (ENABLED and logits.is_cuda and logits.dtype == torch.float32 and coords.dtype == torch.float32 and logits.dim() == 2
            and 1 <= k <= logits.shape[1] <= MAX_K)


def uncertain_points(logits, coords, k, random_coords=None):
    """logits [N, K] fp32, coords [N, K, 2], random_coords [N, R, 2] | None -> [N, k + R, 2]: the coordinates of the k points with the
    smallest |logit| (a fixed order; ties at the threshold: a fixed choice), then the random ones (reference criterion.py:181-189; no gradient)"""
    if not logits.is_cuda:
        raise RuntimeError("pd_uncertain_points runs on the GPU only (no CPU fallback in partdistillation_amd)")
    logits, coords = logits.contiguous(), coords.contiguous()
    N, K = logits.shape
    R = 0 if random_coords is None else random_coords.shape[1]
    rnd = random_coords.contiguous().float() if R else None
    out = torch.empty((N, k + R, 2), dtype=torch.float32, device=logits.device)
    _lib.check(_lib.load().pd_uncertain_points(logits.data_ptr(), coords.data_ptr(), rnd.data_ptr() if rnd is not None else None, out.data_ptr(),
                                               N, K, k, R, _stream()))
    return out


def point_sample_masks_supported(masks, coords):
    return (ENABLED and masks.is_cuda and masks.dtype in (torch.bool, torch.uint8) and masks.is_contiguous() and masks.dim() >= 3
            and coords.dtype == torch.float32 and coords.dim() == 3 and coords.shape[2] == 2)


def point_sample_masks(masks, coords, map_idx=None, coords_div=1):
    """masks bool / uint8 [..., H, W] (M maps), coords [R_c, P, 2] in [0, 1], map_idx int64 [rows] | None (rows = M, row r reads map r)
    -> fp32 [rows, P]: bilinear samples (zeros padding, align_corners=False) of map map_idx[r] at coords[r // coords_div]; no gradient"""
    if not masks.is_cuda:
        raise RuntimeError("pd_point_sample_u8 runs on the GPU only (no CPU fallback in partdistillation_amd)")
    H, W = masks.shape[-2:]
    M = masks.numel() // max(H * W, 1)
    rows = M if map_idx is None else map_idx.numel()
    coords = coords.contiguous()
    P = coords.shape[1]
    assert coords.shape[0] * coords_div >= rows, (coords.shape, coords_div, rows)
    mi = None if map_idx is None else map_idx.contiguous()
    out = torch.empty((rows, P), dtype=torch.float32, device=masks.device)
    _lib.check(_lib.load().pd_point_sample_u8(masks.data_ptr(), mi.data_ptr() if mi is not None else None, coords.data_ptr(), out.data_ptr(), rows, P,
                                              H, W, coords_div, _stream()))
    return out


PAIR_LOGITS = __import__("os").environ.get("PD_PAIR_LOGITS", "1") != "0"     # 0: one library GEMM per image (tools/ A/B runs)
_IMG_START = {}


def _img_start(counts):
    key = tuple(int(c) for c in counts)
    if key not in _IMG_START:
        import ctypes
        if len(_IMG_START) >= 4096:
            _IMG_START.clear()
        acc = [0]
        for c in key:
            acc.append(acc[-1] + c)
        _IMG_START[key] = (ctypes.c_int32 * len(acc))(*acc)
    return _IMG_START[key]


def pair_logits_supported(tok, e):
    return (ENABLED and PAIR_LOGITS and tok.is_cuda and tok.dtype == torch.float32 and e.dtype == torch.float32 and tok.dim() == 3 and tok.is_contiguous()
            and tok.shape[2] == 256 and tok.shape[0] <= 32 and e.dim() == 2 and e.shape[1] == 256 and e.shape[0] > 0)


class PairLogits(Function):
    """tok [B, T, 256] fp32 (channels-last mask features as tokens), e [N, 256] fp32 (the matched pairs' mask embeddings, grouped by image:
    counts[b] rows for image b), out_row int64 [N] (row of the result that pair i of e lands in) -> [N, T]: the mask logits of the matched
    pairs only (reference: the rows src_masks = pred_masks[src_idx] of the decoder's einsum, criterion.py:147-160).  Both gradients."""

    @staticmethod
    def forward(ctx, tok, e, out_row, counts):
        if not tok.is_cuda:
            raise RuntimeError("pd_pair_logits runs on the GPU only (no CPU fallback in partdistillation_amd)")
        e = e.contiguous()
        B, T, C = tok.shape
        N = e.shape[0]
        assert sum(counts) == N and len(counts) == B and out_row.shape == (N,) and out_row.dtype == torch.int64
        out = torch.empty((N, T), dtype=torch.float32, device=tok.device)
        _lib.check(_lib.load().pd_pair_logits_fwd(tok.data_ptr(), e.data_ptr(), _img_start(counts), out_row.data_ptr(), out.data_ptr(), B, T, C, N,
                                                  _stream()))
        ctx.save_for_backward(tok, e, out_row)
        ctx.counts = counts
        return out

    @staticmethod
    def backward(ctx, g):
        tok, e, out_row = ctx.saved_tensors
        B, T, C = tok.shape
        N = e.shape[0]
        g = g.contiguous()
        lib, start = _lib.load(), _img_start(ctx.counts)
        d_tok = d_e = None
        if ctx.needs_input_grad[0]:
            d_tok = torch.empty_like(tok)
            _lib.check(lib.pd_pair_logits_bwd_tok(g.data_ptr(), e.data_ptr(), start, out_row.data_ptr(), d_tok.data_ptr(), B, T, C, N, _stream()))
        if ctx.needs_input_grad[1]:
            d_e = torch.empty_like(e)
            ws = torch.empty((lib.pd_pair_logits_workspace_floats(T, C, N),), dtype=torch.float32, device=tok.device)
            _lib.check(lib.pd_pair_logits_bwd_rows(g.data_ptr(), tok.data_ptr(), start, out_row.data_ptr(), d_e.data_ptr(), ws.data_ptr(), B, T, C, N,
                                                   _stream()))
        return d_tok, d_e, None, None


def pair_logits(tok, e, out_row, counts):
    return PairLogits.apply(tok, e, out_row, list(counts))


LOSS_VECTORS = __import__("os").environ.get("PD_LOSS_VECTORS", "1") != "0"    # 0: the torch expressions (tools/ A/B runs)


def loss_vectors_supported(logits_bd, tclass, class_weight):
    return (ENABLED and LOSS_VECTORS and logits_bd.is_cuda and logits_bd.dtype == torch.float32 and logits_bd.dim() == 4 and tclass.dtype == torch.int64
            and tclass.is_contiguous() and class_weight.dtype == torch.float32 and torch.is_grad_enabled())


class LossVectors(Function):
    """logits [B, H, Q, K1] fp32 (any image / head strides), tclass int64 [B, H, Q], class_weight [K1], d_of_h int64 [H], bce / dice [H * Nh]
    (criterion order), num_masks (device scalar) -> [3, H]: loss_ce, loss_mask, loss_dice of every head in criterion order
    (reference criterion.py:126-145, 203-206).  Gradients with respect to logits, bce, dice."""

    @staticmethod
    def forward(ctx, logits, tclass, class_weight, d_of_h, bce, dice, num_masks):
        if not logits.is_cuda:
            raise RuntimeError("pd_loss_vectors runs on the GPU only (no CPU fallback in partdistillation_amd)")
        if logits.stride(3) != 1 or logits.stride(2) != logits.shape[3]:
            logits = logits.contiguous()
        B, H, Q, K1 = logits.shape
        bce, dice = bce.contiguous().float(), dice.contiguous().float()
        assert bce.numel() % H == 0 and dice.numel() == bce.numel()
        Nh = bce.numel() // H
        nm = num_masks if num_masks.dtype == torch.float32 else num_masks.float()
        vec = torch.empty((3, H), dtype=torch.float32, device=logits.device)
        lse = torch.empty((B, H, Q), dtype=torch.float32, device=logits.device)
        den = torch.empty((H,), dtype=torch.float32, device=logits.device)
        _lib.check(_lib.load().pd_loss_vectors_fwd(logits.data_ptr(), logits.stride(0), logits.stride(1), tclass.data_ptr(), class_weight.data_ptr(),
                                                   d_of_h.data_ptr(), bce.data_ptr(), dice.data_ptr(), nm.data_ptr(), vec.data_ptr(), lse.data_ptr(),
                                                   den.data_ptr(), B, H, Q, K1, Nh, _stream()))
        ctx.save_for_backward(logits, tclass, class_weight, d_of_h, nm, lse, den)
        ctx.Nh = Nh
        return vec

    @staticmethod
    def backward(ctx, dvec):
        logits, tclass, class_weight, d_of_h, nm, lse, den = ctx.saved_tensors
        B, H, Q, K1 = logits.shape
        dvec = dvec.contiguous()
        d_logits = torch.empty_strided(logits.shape, logits.stride(), dtype=torch.float32, device=logits.device)
        d_bd = torch.empty((2, H * ctx.Nh), dtype=torch.float32, device=logits.device)
        _lib.check(_lib.load().pd_loss_vectors_bwd(logits.data_ptr(), logits.stride(0), logits.stride(1), tclass.data_ptr(), class_weight.data_ptr(),
                                                   d_of_h.data_ptr(), nm.data_ptr(), lse.data_ptr(), den.data_ptr(), dvec.data_ptr(), d_logits.data_ptr(),
                                                   d_bd[0].data_ptr(), d_bd[1].data_ptr(), B, H, Q, K1, ctx.Nh, _stream()))
        return d_logits, None, None, None, d_bd[0], d_bd[1], None


def loss_vectors(logits, tclass, class_weight, d_of_h, bce, dice, num_masks):
    return LossVectors.apply(logits, tclass, class_weight, d_of_h, bce, dice, num_masks)
