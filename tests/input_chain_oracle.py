"""Test helper (not collected): the base stage of the dataset mappers composed from the oracle's pieces (oracle/input_pipeline_ref.py).

Reference part_distillation_dataset_mapper.py:59-67 / proposal_dataset_mapper.py:54-60 put ResizeScale(1.0, 1.0, base, base) — and, with
SET_IMAGE_SQUARE, FixedSizeCrop((base, base)) — in front of the augmentations: the image is resized (Pillow BILINEAR) so that its longer side
is `base`, padded right / bottom with 128 to base x base, and only then flipped / cropped / rescaled.  Every Pillow pass rounds to 8 bits, so
the chain is base resize THEN `apply`, never one resize."""
import numpy as np

from oracle import input_pipeline_ref as R


def base_shape(h, w, base):
    """ResizeScale._get_resize with scale 1.0: both sides times min(base / h, base / w), rounded with np.round"""
    scale = min(base * 1.0 / h, base * 1.0 / w)
    return int(np.round(h * scale)), int(np.round(w * scale))


def base_image_ref(img, base, square, pad_value=128):
    """uint8 [H, W, 3] -> the base canvas uint8 [bh, bw, 3], or [base, base, 3] when `square`"""
    bh, bw = base_shape(img.shape[0], img.shape[1], base)
    out = R.resize_bilinear_u8(img, bh, bw)
    if not square:
        return out
    canvas = np.full((base, base, 3), pad_value, dtype=np.uint8)
    canvas[:bh, :bw] = out
    return canvas


def base_draws(rng, base, square):
    """what base_aug draws from the global RNG in every _forward: ResizeScale's uniform(1.0, 1.0), FixedSizeCrop's uniform(0.0, 1.0)"""
    if base > 0:
        rng.uniform(1.0, 1.0)
        if square:
            rng.uniform(0.0, 1.0)


def chain_ref(img, masks, base, square, p):
    """masks bool [n, ch, cw] at the canvas size -> R.apply on the base canvas"""
    return R.apply(base_image_ref(img, base, square), masks, p)


def random_image(rng, H, W):
    return rng.randint(0, 256, (H, W, 3)).astype(np.uint8)


def part_masks(rng, h, w, n):
    """n disjoint Voronoi cells inside an ellipse, bool [n, h, w] — pseudo-labels at the canvas size"""
    ys, xs = np.mgrid[0:h, 0:w]
    seeds = rng.rand(n, 2) * [h, w]
    lab = np.argmin((ys[None] - seeds[:, 0, None, None]) ** 2 + (xs[None] - seeds[:, 1, None, None]) ** 2, axis=0)
    inside = ((ys - h / 2) ** 2 / (0.17 * h * h) + (xs - w / 2) ** 2 / (0.12 * w * w)) < 1.0
    return np.stack([(lab == i) & inside for i in range(n)])
