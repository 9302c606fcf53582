"""The device input pipeline's launchers (include/pd_input.h, csrc/input_pipeline.hip): Pillow's coefficient and index tables on the host,
the Pillow-exact two-pass bilinear resample of a uint8 image (`resample_u8`, and the base stage built on it: `base_canvas`, `base_image`),
the masks sampled straight from their run lengths (`rle_sample`, `rle_sample_groups`), and the uploads they share.  The mappers
(data/*.py) decide windows, flips and groups; every pd_input.h call is made here.  GPU only; there is no fallback."""
import math

import numpy as np
import torch

from .. import lib as _lib

PRECISION_BITS = 32 - 8 - 2


def resample_coeffs(in_size, out_size, first, count):
    """Pillow Resample.c precompute_coeffs + normalize_coeffs_8bpc (bilinear) for output indices [first, first + count),
    vectorised with the same double-precision operation order (the weight sum is a sequential cumsum)."""
    if in_size == out_size:                                   # Pillow skips the pass: identity taps
        idx = np.arange(first, first + count, dtype=np.int32)
        return idx, np.ones(count, dtype=np.int32), np.full((count, 1), 1 << PRECISION_BITS, dtype=np.int32)
    scale = filterscale = (float(in_size) - 0.0) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = 0.0 + (np.arange(first, first + count, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    arg = np.abs(((x + xmin[:, None]) - center[:, None] + 0.5) * ss)
    w = np.where((x < xmax[:, None]) & (arg < 1.0), 1.0 - arg, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]
    k = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    v = k * (1 << PRECISION_BITS)
    kk = np.where(v < 0, np.trunc(v - 0.5), np.trunc(v + 0.5)).astype(np.int32)
    return xmin.astype(np.int32), xmax.astype(np.int32), kk


def nearest_index(in_size, out_size):
    """Pillow NEAREST resize positions (Geometry.c ImagingScaleAffine): tabulated by repeated addition in double precision"""
    scale = float(in_size) / float(out_size)
    steps = np.full(out_size, scale, dtype=np.float64)
    steps[0] = 0.0 + scale * 0.5
    return np.clip(np.cumsum(steps).astype(np.int64), 0, in_size - 1).astype(np.int32)


def base_canvas(h, w, base, square):
    """ResizeScale(1.0, 1.0, base, base) [+ FixedSizeCrop((base, base)) when `square`] of an h x w image
    -> ((bh, bw) resized, (ch, cw) canvas)"""
    scale = min(base * 1.0 / h, base * 1.0 / w)
    bh, bw = int(np.round(h * scale)), int(np.round(w * scale))
    return (bh, bw), ((base, base) if square else (bh, bw))


def to_device(array, device):
    return torch.from_numpy(np.ascontiguousarray(array)).to(device, non_blocking=True)


def upload_image(image, device):
    """decoded uint8 [H, W, 3] (numpy or tensor) -> contiguous on the device"""
    if torch.device(device).type != "cuda":
        raise RuntimeError("the device input pipeline runs on the GPU only (no CPU fallback in partdistillation_amd)")
    img = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image))
    assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3, img.shape
    return img.to(device, non_blocking=True).contiguous()


def pack_tables(tables):
    """integer host tables -> ONE flat int32 vector and the split points between them"""
    parts = [np.asarray(t, dtype=np.int32).reshape(-1) for t in tables]
    return np.concatenate(parts), np.cumsum([len(p) for p in parts])[:-1]


def upload_tables(tables, device):
    """`pack_tables` sent as one upload -> the tables' device views, int32"""
    table, cuts = pack_tables(tables)
    return torch.tensor_split(to_device(table, device), cuts.tolist())


def resample_u8(img, xtab, ytab, canvas=None, *, row0=0, x0=0, flip=False, pad_value=0, planar=True):
    """img uint8 [H, W, 3] on the device; xtab / ytab: `resample_coeffs`' host triples for the vw columns and vh rows of the resize that
    survive -> uint8 [3, oh, ow] ([oh, ow, 3] when not `planar`), canvas = (oh, ow), the window itself when None: the horizontal pass
    over the source rows the surviving rows need, then the vertical pass into the top-left corner of the canvas, the rest = pad_value.
    The tables address the source through its first crop (row0, x0), mirrored when `flip`: source row row0 + i, column x0 + j or
    W - 1 - (x0 + j).  An empty window gives a canvas of pad_value."""
    H, W = int(img.shape[0]), int(img.shape[1])
    vw, vh = len(xtab[0]), len(ytab[0])
    oh, ow = (vh, vw) if canvas is None else (int(canvas[0]), int(canvas[1]))
    r0, r1 = (int(ytab[0].min()), int((ytab[0] + ytab[1]).max())) if vh else (0, 0)
    tmp = torch.empty((r1 - r0, vw, 3), dtype=torch.uint8, device=img.device)
    out = torch.empty((3, oh, ow) if planar else (oh, ow, 3), dtype=torch.uint8, device=img.device)
    d = upload_tables(tuple(xtab) + tuple(ytab), img.device)              # held until both launches are enqueued
    L, st = _lib.load(), _lib.current_stream()
    _lib.check(L.pd_resample_rows_u8(img.data_ptr(), H, W, row0 + r0, r1 - r0, x0, int(flip), d[0].data_ptr(), d[1].data_ptr(),
                                     d[2].data_ptr(), xtab[2].shape[1], vw, tmp.data_ptr(), st))
    _lib.check(L.pd_resample_cols_canvas_u8(tmp.data_ptr(), r1 - r0, vw, r0, d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(),
                                            ytab[2].shape[1], vh, vw, oh, ow, int(pad_value), int(planar), out.data_ptr(), st))
    return out


def base_image(image, base, square, pad_value, planar, device):
    """image uint8 [H, W, 3] -> the base canvas uint8 [ch, cw, 3] ([3, ch, cw] when `planar`) on the device: Pillow BILINEAR resize
    to base_canvas(H, W), the rest of the canvas = pad_value"""
    assert base > 0, "base_image needs base_size > 0"
    img = upload_image(image, device)
    H, W = int(img.shape[0]), int(img.shape[1])
    (bh, bw), canvas = base_canvas(H, W, base, square)
    return resample_u8(img, resample_coeffs(W, bw, 0, bw), resample_coeffs(H, bh, 0, bh), canvas, pad_value=pad_value, planar=planar)


def rle_sample(starts, offsets, H, W, flip, sx, sy, S):
    """pd_rle_sample_u8 on device int32 tensors: the n = len(offsets) - 1 masks of an H x W image from their run starts, sampled at the
    source columns sx (mirrored when `flip`) and rows sy into the top-left corner of S x S planes, the rest 0
    -> (masks uint8 [n, S, S], area int32 [n]); n = 0 launches nothing"""
    n = int(offsets.numel()) - 1
    masks = torch.empty((n, S, S), dtype=torch.uint8, device=offsets.device)
    area = torch.zeros(n, dtype=torch.int32, device=offsets.device)     # the kernel adds to it
    if n:
        _lib.check(_lib.load().pd_rle_sample_u8(starts.data_ptr(), offsets.data_ptr(), n, H, W, int(flip), sx.data_ptr(), sy.data_ptr(),
                                                int(sy.numel()), int(sx.numel()), S, masks.data_ptr(), area.data_ptr(),
                                                _lib.current_stream()))
    return masks, area


def rle_sample_groups(starts, offsets, H, W, src_x, src_y, group_offsets, group_members, out=None, member_area=None, group_area=None,
                      uploaded=None, canvas=None):
    """pd_rle_sample_groups_u8 on device tensors (int32 tables; the group table may be host numpy: its member indices are range-checked
    here, before upload) -> (planes uint8 [G, out_h, out_w], member_area int32 [n], group_area int32 [G]); nothing is pre-zeroed.
    `uploaded`: device int32 copies (group_offsets, group_members padded by one entry) of the host group table the caller has already
    sent with another upload; the host table is still what is checked.
    `canvas` = (out_h, out_w): pd_rle_sample_groups_canvas_u8 — the tables span the window len(src_y) x len(src_x) in the top-left corner
    of each plane and the rest of the plane is 0 (ValueError when the window does not fit)"""
    dev = src_x.device
    n, G = int(offsets.numel()) - 1, len(group_offsets) - 1
    go, gm = (np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype=np.int64).reshape(-1) for a in (group_offsets, group_members))
    if G < 0 or go[0] != 0 or (np.diff(go) < 0).any() or go[-1] != len(gm):
        raise ValueError("rle_sample_groups: group_offsets is not a CSR offset vector of group_members")
    if len(gm) and (gm.min() < 0 or gm.max() >= n):
        raise ValueError(f"rle_sample_groups: member index outside [0, {n})")
    if uploaded is not None:
        d_go, d_gm = uploaded
        assert d_go.dtype == torch.int32 and d_gm.dtype == torch.int32 and d_go.numel() == len(go) and d_gm.numel() > len(gm)
    else:
        d_go = torch.from_numpy(go.astype(np.int32)).to(dev, non_blocking=True)
        d_gm = torch.from_numpy(np.concatenate((gm, [0])).astype(np.int32)).to(dev, non_blocking=True)  # never a null pointer
    vh, vw = int(src_y.numel()), int(src_x.numel())
    out_h, out_w = (vh, vw) if canvas is None else (int(canvas[0]), int(canvas[1]))
    if vh > out_h or vw > out_w:
        raise ValueError(f"rle_sample_groups: the window {vh} x {vw} does not fit the canvas {out_h} x {out_w}")
    out = torch.empty((G, out_h, out_w), dtype=torch.uint8, device=dev) if out is None else out
    member_area = torch.empty(n, dtype=torch.int32, device=dev) if member_area is None else member_area
    group_area = torch.empty(G, dtype=torch.int32, device=dev) if group_area is None else group_area
    assert out.is_contiguous() and tuple(out.shape) == (G, out_h, out_w) and member_area.numel() == n and group_area.numel() == G
    tail = (d_go.data_ptr(), d_gm.data_ptr(), G, out.data_ptr() if G else None, member_area.data_ptr() if n else None,
            group_area.data_ptr() if G else None, _lib.current_stream())
    if canvas is None:
        _lib.check(_lib.load().pd_rle_sample_groups_u8(starts.data_ptr() if n else None, offsets.data_ptr() if n else None, n, H, W,
                                                       src_x.data_ptr(), src_y.data_ptr(), out_h, out_w, *tail))
    else:
        _lib.check(_lib.load().pd_rle_sample_groups_canvas_u8(starts.data_ptr() if n else None, offsets.data_ptr() if n else None, n, H, W,
                                                              src_x.data_ptr() if vw else None, src_y.data_ptr() if vh else None, vh, vw,
                                                              out_h, out_w, *tail))
    return out, member_area, group_area
