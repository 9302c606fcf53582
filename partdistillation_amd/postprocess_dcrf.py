"""Dense-CRF clean-up of generated part proposals: the loop body of the reference's continuously_postprocess_dcrf.py:127-153 with the
mean field on the device (functions/dense_crf.py).  The image is brought to size x size the way the reference does (ResizeScale(1, 1, size,
size) + FixedSizeCrop(size), padded with 128) through the mappers' Pillow-exact base stage (functions/input_pipeline.py `base_image`)."""
import numpy as np
import torch

from .functions import dense_crf as _dcrf
from .functions.input_pipeline import base_image
from .utils import rle

MASK_KEYS = ("part_masks", "part_mask")          # the reference's key; the key ProposalGenerationModel._result writes


def resize_image(image, size=640, device="cuda"):
    """uint8 [H, W, 3] (numpy or tensor) -> uint8 [size, size, 3] on the device"""
    return base_image(image, size, True, 128, False, device)


def refine_proposals(data, image, size=640, device="cuda", **crf):
    """data: the dict a proposal-generation run saved per image, its RLE masks (each size x size) under "part_masks" or "part_mask";
    image: the decoded RGB image, uint8 [H, W, 3].  Returns `data` with the masks replaced by the dense-CRF result, under the key found:
    cmask = sum_c mask_c * (c + 1) -> dense_crf(image at size x size, cmask, num_c + 1, **crf) -> one mask per non-zero label that
    survives.  A missing, None or empty mask list passes through untouched."""
    key = next((k for k in MASK_KEYS if k in data), None)
    if key is None or data[key] is None or len(data[key]) == 0:
        return data
    if torch.device(device).type == "cuda":
        # the masks stay run tables on the bus: strings -> run starts (host) -> label map (device) -> dense_crf -> run table -> strings
        from .functions import rle as device_rle
        num_c = len(data[key])
        cmask = device_rle.decode_label_map(data[key], (size, size), device)         # ValueError "... do not match ..." on another size
        img = resize_image(image, size, device)
        out = _dcrf.dense_crf(img, cmask, num_c + 1, **crf)
        data[key], _ = device_rle.encode_label_map(out)                               # one mask per non-zero label that survives
        return data
    bmask = np.stack([rle.decode(m["segmentation"]) for m in data[key]])
    if tuple(bmask.shape[1:]) != (size, size):
        raise ValueError(f"tensor shapes do not match. ({(size, size)} != {tuple(bmask.shape[1:])})")
    num_c = bmask.shape[0]
    cmask = (bmask.astype(np.int64) * (np.arange(num_c, dtype=np.int64) + 1)[:, None, None]).sum(0)
    img = resize_image(image, size, device)
    out = _dcrf.dense_crf(img, torch.from_numpy(cmask).to(img.device), num_c + 1, **crf)
    out = np.asarray(out.cpu())
    present = [c for c in np.unique(out) if c != 0]
    data[key] = rle.masks_to_coco_json(np.stack([out == c for c in present]) if present else np.zeros((0, size, size), dtype=bool))
    return data
