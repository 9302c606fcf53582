"""``DeviceProposalGenerationMapper`` / ``DeviceImagenetPartRankingMapper``: the reference's ProposalGenerationMapper
(data/dataset_mappers/proposal_generation_mapper.py) and ImagenetPartRankingDatasetMapper
(data/dataset_mappers/imagenet_part_ranking_dataset_mapper.py), the mappers of the two ImageNet stages around proposal learning:
stage 1 (ProposalGenerationModel: an image and, with PROPOSAL_GENERATION.WITH_GIVEN_MASK, the Detic object mask) and part ranking in its
"imagenet" modes (PartRankingModel: an image on the padded square canvas and ONE object mask = the union of the parts stage 1 saved).
The record builders `imagenet_record` / `imagenet_proposal_record` turn one image path, or one saved stage-1 file, into the dict the
reference's dataset registration (register_imagenet.py, register_imagenet_with_proposals.py) hands its mapper; the directory walks
and the catalogs stay out.

Both augmentation lists are fixed: [ResizeScale(1, 1, S, S)] for proposal generation, [ResizeScale(1, 1, S, S)] then
[FixedSizeCrop((S, S))] for part ranking — exactly the base stage of DeviceProposalMapper: the same `base_canvas` / `base_image`
(functions/input_pipeline.py).  Host side: the two draws the transforms consume, the run-length parse and, for proposal generation,
which masks are empty and the boxes of the others, both straight from the run lengths (no device readback).  Device side: the
Pillow-exact two-pass resize (`resample_u8`), the mask decode of stage 1 (pd_rle_decode) and, for part ranking, ONE
`rle_sample_groups(canvas=)` launch (include/pd_input.h) that ORs every part straight from its run lengths into the window of the
S x S plane the resized image occupies and zeroes the rest — the reference's `FixedSizeCrop` pad of n dense masks followed by
`gt_masks.tensor.sum(0)[None]`, without the n dense planes.  Nothing is read back and nothing synchronises.

UNPINNED: detectron2 is not available to test against; the order of the draws (ResizeScale's uniform(1.0, 1.0), then FixedSizeCrop's
uniform(0.0, 1.0)), FixedSizeCrop's pad values (128 for the image, 0 for masks) and the float32 box dtype are restated from detectron2
0.6, like the other mappers'."""
import logging
import os

import numpy as np
import torch

from ..compat import BitMasks, Instances
from ..functions.input_pipeline import base_canvas, base_image, pack_tables, rle_sample_groups, to_device
from ..utils.rle import run_lengths, segmentations_to_starts
from .device_mapper import load_saved, read_image

_logger = logging.getLogger("part_distillation")


# ---------------------------------------------------------------------------------------------------- host: run lengths
def run_area(counts):
    """set pixels of a mask = the sum of its odd-indexed run lengths"""
    return int(np.asarray(counts)[1::2].sum())


def run_box(counts, h):
    """BitMasks.get_bounding_boxes of one mask from its run lengths (column-major, height h): float32 [x0, y0, x1 + 1, y1 + 1], zeros for
    an empty mask.  A 1-run [s, e) covers the columns s // h .. (e - 1) // h; the rows s % h .. (e - 1) % h when it stays in one column,
    every row otherwise."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    ends = np.cumsum(counts)
    s, e = (ends - counts)[1::2], ends[1::2]
    s, e = s[e > s], e[e > s]                                               # zero-length runs cover nothing
    if len(s) == 0:
        return np.zeros(4, dtype=np.float32)
    c0, c1 = s // h, (e - 1) // h
    one = c0 == c1
    y0 = np.where(one, s % h, 0).min()
    y1 = np.where(one, (e - 1) % h, h - 1).max()
    return np.asarray([c0.min(), y0, c1.max() + 1, y1 + 1], dtype=np.float32)


# ---------------------------------------------------------------------------------------------------- host: records
def imagenet_record(dataset_path, class_code, image_name, class_code_to_class_id, class_name=None, object_mask_path=None):
    """the dict of the reference's register_imagenet.py:43-57 for dataset_path/class_code/image_name.  With `object_mask_path`
    (PROPOSAL_GENERATION.WITH_GIVEN_MASK) the Detic file object_mask_path/class_code/image_name gives the single pseudo-annotation: its
    first, most confident object mask; None when that file is missing or holds no mask"""
    data = {"file_path": os.path.join(dataset_path, class_code, image_name), "file_name": image_name, "class_code": class_code,
            "gt_object_class": class_code_to_class_id[class_code], "class_name": class_name}
    if object_mask_path is not None:
        path = os.path.join(object_mask_path, class_code, image_name)
        if not os.path.exists(path):
            return None
        object_data = load_saved(path, _logger)
        if object_data is None or len(object_data["object_masks"]) == 0:
            return None
        data["pseudo_annotations"] = [{"segmentation": object_data["object_masks"][0]["segmentation"]}]
    return data


def imagenet_proposal_record(path_tuple, class_code_to_class_id, min_object_area_ratio=-1.0):
    """the dict of the reference's register_imagenet_with_proposals.py:54-75 from the file (dataset_path, class_code, name) that
    ProposalGenerationModel saved; None when the file is corrupted, `object_ratio` is not above the threshold or `part_mask` is empty"""
    ann = load_saved(os.path.join(*path_tuple), _logger)
    if ann is None or not ann["object_ratio"] > min_object_area_ratio or not ann["part_mask"]:
        return None
    h, w = ann["part_mask"][-1]["segmentation"]["size"]
    return {"file_name": ann["file_path"], "image_id": ann["file_name"], "class_code": path_tuple[1],
            "gt_object_class": class_code_to_class_id[path_tuple[1]], "height": int(h), "width": int(w),
            "pseudo_annotations": [{"segmentation": m["segmentation"]} for m in ann["part_mask"]]}


# ---------------------------------------------------------------------------------------------------- the mappers
class DeviceProposalGenerationMapper:
    """reference ProposalGenerationMapper: the image resized so that its longer side is `image_size` (no pad), planar, and with
    `with_given_mask` the record's object masks AT THEIR STORED SIZE (the reference hands them an empty transform list): masks of another
    size than the resized image are not refused, because the reference does not refuse them — but ProposalGenerationModel needs them at
    the mapper's output resolution, which is what Detic saved when it ran behind the same resize.  Returns None for an unreadable image
    and, with `with_given_mask`, when no non-empty mask is left (logged).  The output is a new dict (the input is not modified) without
    `pseudo_annotations`."""

    def __init__(self, image_size, with_given_mask=False, device="cuda", rng=None):
        self.image_size, self.with_given_mask, self.device = int(image_size), bool(with_given_mask), torch.device(device)
        self.rng = rng if rng is not None else np.random                     # detectron2 draws from the global numpy RNG
        self.square_base, self.pad_value = False, 128                       # no canvas beyond the resized image: nothing is padded
        self.logger = _logger

    @classmethod
    def from_config(cls, cfg, device=None):
        """reference :33-48"""
        return cls(cfg.INPUT.IMAGE_SIZE, cfg.PROPOSAL_GENERATION.WITH_GIVEN_MASK, device or cfg.MODEL.DEVICE)

    def draw(self):
        """ResizeScale(1.0, 1.0, S, S) draws its scale"""
        self.rng.uniform(1.0, 1.0)

    def masks(self, record):
        """the host half of `_transform_annotations` (:79-106): the non-empty masks' segmentations, classes (-1 when absent) and float32
        boxes, all from the run lengths -> (segmentations, classes int64 [k], boxes float32 [k, 4])"""
        segs, classes, boxes = [], [], []
        for obj in record.get("pseudo_annotations", ()):
            seg = obj["segmentation"]
            counts = run_lengths(seg)
            if run_area(counts) == 0:                                       # filter_empty_instances(by_box=False)
                continue
            segs.append(seg)
            classes.append(int(obj.get("category_id", -1)))
            boxes.append(run_box(counts, int(seg["size"][0])))
        return segs, np.asarray(classes, dtype=np.int64), np.asarray(boxes, dtype=np.float32).reshape(-1, 4)

    def __call__(self, record):
        """record: `imagenet_record`'s dict, with "image" (decoded uint8 HWC) or a "file_path" readable by Pillow -> the reference
        mapper's output dict, tensors on the device: image uint8 [3, h, w], height / width = h, w and, with `with_given_mask`,
        instances (gt_masks BitMasks, gt_classes int64, gt_boxes float32 [k, 4])"""
        image = record.get("image")
        if image is None:
            try:
                image = read_image(record, "file_path")
            except Exception:                                               # the reference: a bare `except: return`
                return None
        if "width" in record or "height" in record:                         # detection_utils.check_image_size
            if (record.get("height"), record.get("width")) != (image.shape[0], image.shape[1]):
                raise ValueError(f"Mismatched image shape for {record.get('file_path')}: got {(image.shape[0], image.shape[1])}, "
                                 f"expect {(record.get('height'), record.get('width'))}")
        self.draw()
        out = {k: v for k, v in record.items() if k not in ("pseudo_annotations", "image")}
        if self.with_given_mask:
            segs, classes, boxes = self.masks(record)
            if not segs:
                self.logger.info("No mask detected on {}.".format(record.get("file_path")))
                return None
        img = base_image(image, self.image_size, self.square_base, self.pad_value, True, self.device)
        h, w = int(img.shape[1]), int(img.shape[2])
        out.update(image=img, height=h, width=w)
        if self.with_given_mask:
            from ..functions import rle as device_rle
            inst = Instances((h, w))
            inst.gt_masks = BitMasks(device_rle.decode_masks(segs, segs[0]["size"], self.device))
            inst.gt_classes = to_device(classes, self.device)
            inst.gt_boxes = to_device(boxes, self.device)
            out["instances"] = inst
        return out


class DeviceImagenetPartRankingMapper:
    """reference ImagenetPartRankingDatasetMapper: the image on the S x S canvas (resize, then pad right / bottom with `pad_value`) and
    ONE object mask, the union of the record's part masks, zero-padded to S x S; gt_classes = [class_code_to_class_index[class_code]].
    The part masks must have the size of the RESIZED image — what stage 1 saved — or the reference's plane would not be S x S:
    ValueError.  An empty `pseudo_annotations` is a ValueError too (the reference raises AttributeError there).  The output is a new
    dict without `pseudo_annotations`; the input is not modified."""

    def __init__(self, image_size, class_code_to_class_index, device="cuda", rng=None, pad_value=128):
        self.image_size, self.device = int(image_size), torch.device(device)
        self.class_code_to_class_index = class_code_to_class_index
        self.rng = rng if rng is not None else np.random                     # detectron2 draws from the global numpy RNG
        self.square_base, self.pad_value = True, int(pad_value)

    @classmethod
    def from_config(cls, cfg, class_code_to_class_index, device=None):
        """reference :36-53"""
        if cfg.INPUT.MASK_FORMAT != "bitmask":
            raise NotImplementedError(f"INPUT.MASK_FORMAT '{cfg.INPUT.MASK_FORMAT}': the saved part proposals are COCO RLE; this mapper "
                                      "maps 'bitmask' only")
        return cls(cfg.INPUT.IMAGE_SIZE, class_code_to_class_index, device or cfg.MODEL.DEVICE)

    def draw(self):
        """base_aug's ResizeScale draws its scale, then aug's FixedSizeCrop its offset fraction (times a zero range): the order
        DeviceProposalMapper.draw consumes them in for its base stage"""
        self.rng.uniform(1.0, 1.0)
        self.rng.uniform(0.0, 1.0)

    def tables(self, segmentations, bh, bw):
        """everything the sampling launch reads, as ONE int32 vector and its split points: the run starts and their offsets, the identity
        index tables of the bh x bw window, and the group table of the single plane that holds every member (padded by one entry)"""
        n = len(segmentations)
        starts, offsets = segmentations_to_starts(segmentations, (bh, bw))
        parts = (starts, offsets, np.arange(bw, dtype=np.int32), np.arange(bh, dtype=np.int32), np.asarray([0, n], dtype=np.int32),
                 np.arange(n + 1, dtype=np.int32) % max(n, 1))
        return pack_tables(parts)

    def __call__(self, record):
        """record: `imagenet_proposal_record`'s dict, with "image" (decoded uint8 HWC) or a "file_name" readable by Pillow -> the
        reference mapper's output dict, tensors on the device: image uint8 [3, S, S], height = width = S, instances (gt_masks BitMasks
        [1, S, S], gt_classes int64 [1])"""
        S = self.image_size
        image = read_image(record)
        self.draw()
        (bh, bw), _ = base_canvas(int(image.shape[0]), int(image.shape[1]), S, self.square_base)
        segs = [part["segmentation"] for part in record["pseudo_annotations"]]
        name = record.get("file_name")
        if not segs:
            raise ValueError(f"{name}: no pseudo_annotations (the reference mapper raises AttributeError on such a record)")
        for seg in segs:
            if tuple(int(v) for v in seg["size"]) != (bh, bw):
                raise ValueError(f"{name}: a part mask of size {tuple(int(v) for v in seg['size'])} on an image resized to {(bh, bw)}: "
                                 f"the part masks must have the size of the resized image")
        class_index = self.class_code_to_class_index[record["class_code"]]
        img = base_image(image, self.image_size, self.square_base, self.pad_value, True, self.device)
        table, cuts = self.tables(segs, bh, bw)
        d = to_device(table, self.device)                                        # one upload
        starts, offsets, sx, sy, d_go, d_gm = torch.tensor_split(d, cuts.tolist())
        n = len(segs)
        plane = rle_sample_groups(starts, offsets, bh, bw, sx, sy, [0, n], np.arange(n), uploaded=(d_go, d_gm), canvas=(S, S))[0]
        inst = Instances((S, S))
        inst.gt_masks = BitMasks(plane.view(torch.bool))
        inst.gt_classes = to_device(np.asarray([class_index], dtype=np.int64), self.device)
        out = {k: v for k, v in record.items() if k not in ("pseudo_annotations", "image")}
        out.update(image=img, height=S, width=S, instances=inst)
        return out
