"""``DeviceProposalMapper``: the reference's ProposalDatasetMapper (data/dataset_mappers/proposal_dataset_mapper.py:24-235)
with the pixel work on the GPU (include/pd_input.h) — SURVEY §8 f3.

Host side (cheap, data-dependent control flow): the random draws of detectron2's RandomFlip / RandomCrop / ResizeScale /
FixedSizeCrop in the order the reference builds them (:64-88; restated from detectron2 0.6, which is not in this image),
the COCO RLE string -> run lengths parse, Pillow's coefficient tables for the region that survives the crops.
Device side: the Pillow-exact two-pass bilinear resample of the image with flip / crops / pad folded into the addressing,
and every pseudo-label mask sampled straight from its run lengths (decode + flip + crop + nearest resize + crop + pad in
one kernel, no dense full-resolution mask), plus the mask areas for the reference's area-ratio filter (:225-235).
The uploaded image is the decoded uint8 HWC array; the result is what the reference's mapper returns
({"image" [3,S,S] uint8, "padding_mask", "instances" (gt_masks BitMasks, gt_classes), "height", "width"}), on the device.

Base stage (`base_size > 0`, reference :54-60 and :174-175; CUSTOM_DATASETS.BASE_SIZE 640 in every shipped training script): the image is
first resized so that its longer side is `base_size` — the resolution the pseudo-labels were generated at — and, for the part-distillation
mapper with PART_DISTILLATION.SET_IMAGE_SQUARE, padded right / bottom with 128 to base x base.  Pillow rounds to 8 bits after every pass,
so the base resize cannot be folded into the augmentation's resize: it is its own two passes (pd_resample_rows_u8, then
pd_resample_cols_canvas_u8 writing the HWC canvas the next pd_resample_rows_u8 reads), done once per image, not once per attempt.

``DevicePartDistillationMapper`` is the same for the reference's PartDistillationDatasetMapper
(data/dataset_mappers/part_distillation_dataset_mapper.py), train and test; both mappers read the saved pseudo-label dicts of the
PATH_ONLY datasets through `load_annotation`."""
import logging
import os

import numpy as np
import torch

from ..compat import BitMasks, Instances
from ..functions.input_pipeline import (base_canvas, base_image, nearest_index, resample_coeffs, resample_u8, rle_sample, upload_image,
                                        upload_tables)
from ..utils import rle as _rle


def read_image(record, key="file_name"):
    """the record's decoded "image", else the file record[key] through Pillow -> uint8 [H, W, 3]"""
    image = record.get("image")
    if image is None:
        from PIL import Image
        image = np.asarray(Image.open(record[key]).convert("RGB"))
    return image


def load_cpu(path):
    return torch.load(path, map_location="cpu", weights_only=False)          # pickled Python objects (dicts, numpy arrays), not tensors only


def load_saved(path, logger):
    """`load_cpu`; None (logged) when the file is corrupted — a missing or unreadable file is not a corrupted one"""
    try:
        return load_cpu(path)
    except OSError:
        raise
    except Exception:
        logger.info("%s is corrupted.", path)
        return None


def random_crop(rng, h, w, crop_type, crop_size):
    """detectron2 0.6 RandomCrop.get_transform of an h x w image: get_crop_size's draws, then the row and the column offset
    -> (x0, y0, cw, ch)"""
    if crop_type == "relative":
        ch, cw = int(h * crop_size[0] + 0.5), int(w * crop_size[1] + 0.5)
    elif crop_type == "relative_range":
        cs = np.asarray(crop_size, dtype=np.float32)
        chf, cwf = cs + rng.rand(2) * (1 - cs)
        ch, cw = int(h * chf + 0.5), int(w * cwf + 0.5)
    elif crop_type == "absolute":
        ch, cw = min(crop_size[0], h), min(crop_size[1], w)
    else:
        raise NotImplementedError(crop_type)
    y0 = rng.randint(h - ch + 1)
    x0 = rng.randint(w - cw + 1)
    return int(x0), int(y0), int(cw), int(ch)


class DeviceProposalMapper:
    def __init__(self, image_size, min_scale=0.1, max_scale=2.0, crop_type=None, crop_size=None, flip=True, min_area_ratio=0.0,
                 min_object_area_ratio=0.0, device="cuda", rng=None, pad_value=128, num_repeats=100, base_size=-1, square_base=False,
                 class_code_to_class_id=None):
        self.image_size, self.min_scale, self.max_scale = int(image_size), float(min_scale), float(max_scale)
        self.crop_type, self.crop_size, self.flip = crop_type, crop_size, flip
        self.min_area_ratio, self.min_object_area_ratio = min_area_ratio, min_object_area_ratio
        self.device, self.pad_value, self.num_repeats = torch.device(device), int(pad_value), num_repeats
        self.rng = rng if rng is not None else np.random                 # detectron2 draws from the global numpy RNG
        self.base_size, self.square_base = int(base_size), bool(square_base)
        self.class_code_to_class_id = class_code_to_class_id if class_code_to_class_id is not None else {}   # no MetadataCatalog here
        self.logger = logging.getLogger("part_distillation")

    @staticmethod
    def _augmentation_args(cfg):
        """the AUG_NAME_LIST / INPUT.* keys both mappers read (reference :62-97) -> the first six constructor arguments"""
        names = list(cfg.CUSTOM_DATASETS.AUG_NAME_LIST)
        for n in names:
            if n not in ("flip", "crop", "scale"):
                raise NotImplementedError(f"augmentation '{n}' (reference :68-72: colour jitter / rotation) is not in the device pipeline")
        scale = "scale" in names
        return (cfg.INPUT.IMAGE_SIZE, cfg.INPUT.MIN_SCALE if scale else 1.0, cfg.INPUT.MAX_SCALE if scale else 1.0,
                cfg.INPUT.CROP.TYPE if "crop" in names else None, tuple(cfg.INPUT.CROP.SIZE) if "crop" in names else None, "flip" in names)

    @classmethod
    def from_config(cls, cfg, is_train=True, device=None, base_size=-1, class_code_to_class_id=None):
        """reference :49-60: the caller passes cfg.CUSTOM_DATASETS.BASE_SIZE as `base_size` (part_proposal_train_net.py:73)"""
        return cls(*cls._augmentation_args(cfg), cfg.PROPOSAL_LEARNING.MIN_AREA_RATIO, cfg.PROPOSAL_LEARNING.MIN_OBJECT_AREA_RATIO,
                   device or cfg.MODEL.DEVICE, base_size=base_size, class_code_to_class_id=class_code_to_class_id)

    # ------------------------------------------------------------------ host: saved pseudo-labels of the PATH_ONLY datasets
    def load_annotation(self, path_tuple):
        """reference :113-139: the dict ProposalGenerationModel._result saves -> dataset dict, or None when the file is corrupted, the
        object is not larger than min_object_area_ratio of the image, or there are no part masks"""
        ann = load_saved(os.path.join(*path_tuple), self.logger)
        if ann is None or not ann["object_ratio"] > self.min_object_area_ratio or not ann["part_mask"]:
            return None
        h, w = ann["part_mask"][-1]["segmentation"]["size"]
        return {"file_name": ann["file_path"], "image_id": ann["file_name"], "class_code": path_tuple[1], "height": h, "width": w,
                "pseudo_annotations": [{"segmentation": m["segmentation"], "category_id": 0} for m in ann["part_mask"]],   # class-agnostic
                "gt_object_class": self.class_code_to_class_id[ann["class_code"]]}

    # ------------------------------------------------------------------ host: parameter draws (detectron2 0.6 augmentation_impl.py)
    def base_canvas(self, h, w):
        """ResizeScale(1.0, 1.0, base, base) [+ FixedSizeCrop((base, base))] of an h x w image -> ((bh, bw) resized, (ch, cw) canvas)"""
        return base_canvas(h, w, self.base_size, self.square_base)

    def draw(self, in_h, in_w, weak=False):
        """in_h, in_w: the size the augmentations see — the base canvas when the base stage is on"""
        rng, S = self.rng, self.image_size
        if self.base_size > 0:
            # the reference applies base_aug inside every _forward (:174-175): its ResizeScale draws its scale, uniform(1.0, 1.0), and
            # its FixedSizeCrop its offset fraction, uniform(0.0, 1.0) (times a zero range), ahead of the augmentations' own draws
            rng.uniform(1.0, 1.0)
            if self.square_base:
                rng.uniform(0.0, 1.0)
        p = {"in_h": in_h, "in_w": in_w, "size": S, "flip": bool(self.flip and rng.uniform() < 0.5)}
        h, w = in_h, in_w
        p["crop1"] = (0, 0, w, h)
        if self.crop_type is not None and not weak:
            p["crop1"] = random_crop(rng, h, w, self.crop_type, self.crop_size)
            h, w = p["crop1"][3], p["crop1"][2]
        s = rng.uniform(1.0, 1.0) if weak else rng.uniform(self.min_scale, self.max_scale)
        out_scale = min(S * s / h, S * s / w)
        rh, rw = int(np.round(h * out_scale)), int(np.round(w * out_scale))
        p["resize"] = (rh, rw)
        off = np.round(np.multiply(np.maximum(np.array([rh, rw]) - S, 0), rng.uniform(0.0, 1.0))).astype(int)
        p["crop2"] = (int(off[1]), int(off[0]))
        return p

    # ------------------------------------------------------------------ device: pixels
    def base_image(self, image, planar=False):
        """image uint8 [H, W, 3] -> the base canvas uint8 [ch, cw, 3] ([3, ch, cw] when `planar`) on the device"""
        return base_image(image, self.base_size, self.square_base, self.pad_value, planar, self.device)

    def transform(self, image, segmentations, p):
        """image uint8 [H, W, 3] (numpy or tensor), segmentations = list of COCO RLE dicts {"size": [H, W], "counts": str}
        -> (image uint8 [3,S,S], masks bool [n,S,S], padding_mask bool [S,S], areas int32 [n]) on the device"""
        img = upload_image(image, self.device)
        S, H, W = p["size"], int(img.shape[0]), int(img.shape[1])
        (x0, y0, cw, ch), (rh, rw), (ox, oy), flip = p["crop1"], p["resize"], p["crop2"], p["flip"]
        vh, vw = min(rh - oy, S), min(rw - ox, S)
        # image: horizontal pass over the source rows the surviving output rows need, then vertical pass + crop + pad
        out = resample_u8(img, resample_coeffs(cw, rw, ox, vw), resample_coeffs(ch, rh, oy, vh), (S, S), row0=y0, x0=x0, flip=flip,
                          pad_value=self.pad_value)
        padding = torch.ones((S, S), dtype=torch.bool, device=self.device)
        padding[:vh, :vw] = False
        for seg in segmentations:
            assert tuple(seg["size"]) == (H, W), (seg["size"], (H, W))
        masks, area = torch.empty((0, S, S), dtype=torch.uint8, device=self.device), torch.zeros(0, dtype=torch.int32, device=self.device)
        if segmentations:                                                    # masks: straight from the run lengths, one upload
            sx = x0 + nearest_index(cw, rw)[ox:ox + vw]
            sy = y0 + nearest_index(ch, rh)[oy:oy + vh]
            d = upload_tables(_rle.segmentations_to_starts(segmentations, (H, W)) + (sx, sy), self.device)
            masks, area = rle_sample(d[0], d[1], H, W, flip, d[2], d[3], S)
        return out, masks.view(torch.bool), padding, area

    def select(self, masks, area):
        """reference :217-235: drop empty masks (filter_empty_instances(by_box=False)), then masks whose share of the total
        mask area is <= min_area_ratio -> indices kept"""
        a = area.float()
        nonempty = (area > 0).nonzero().flatten()
        if nonempty.numel() == 0:
            return nonempty
        ratio = a[nonempty] / a[nonempty].sum()
        return nonempty[ratio > self.min_area_ratio]

    def _output(self, dataset_dict, image, padding, masks, classes, size):
        inst = Instances(size)
        inst.gt_masks = BitMasks(masks)
        inst.gt_classes = classes
        out = {k: v for k, v in dataset_dict.items() if k not in ("pseudo_annotations", "image")}
        out.update(image=image, padding_mask=padding, instances=inst, height=size[0], width=size[1])
        return out

    def __call__(self, dataset_dict):
        """dataset_dict: {"image": decoded uint8 HWC array (or "file_name" readable by Pillow), "pseudo_annotations":
        [{"segmentation": COCO RLE dict, "category_id"?}], ...}, or the (dataset_path, class_code, file) tuple of a PATH_ONLY dataset
        -> the reference mapper's output dict, tensors on the device (None when load_annotation drops the image).  With the base
        stage on, the masks' RLE size is the base canvas, not the decoded image (`transform` asserts it)."""
        if isinstance(dataset_dict, tuple):
            dataset_dict = self.load_annotation(dataset_dict)
            if dataset_dict is None:
                return None
        image = read_image(dataset_dict)
        if self.base_size > 0:
            image = self.base_image(image)                                   # once: it does not depend on the draws
        annos = dataset_dict["pseudo_annotations"]
        segs = [a["segmentation"] for a in annos]
        classes = torch.tensor([int(a.get("category_id", -1)) for a in annos], dtype=torch.int64)
        H, W = int(image.shape[0]), int(image.shape[1])
        repeats = self._repeats(annos)
        for attempt in range(repeats + 1):
            p = self.draw(H, W, weak=attempt == self.num_repeats)            # last resort: the weak augmentation (:160-164)
            img, masks, padding, area = self.transform(image, segs, p)
            keep = self.select(masks, area)
            if keep.numel() > 0 or attempt == repeats:
                break
        return self._output(dataset_dict, img, padding, masks[keep], classes.to(self.device)[keep], (self.image_size, self.image_size))

    def _repeats(self, annos):
        return self.num_repeats


class DevicePartDistillationMapper(DeviceProposalMapper):
    """the reference's PartDistillationDatasetMapper, which part_distillation_train_net.py builds for its train AND its test loader:
    the base stage always on, part labels as gt_classes, a score filter on the saved parts, and `is_train=False` = the reference's
    `test_aug = []` — the base canvas itself with the decoded masks, no augmentation and no draws."""

    def __init__(self, *args, is_train=True, min_score=-1.0, **kw):
        super().__init__(*args, **kw)
        if self.base_size <= 0:
            raise ValueError("DevicePartDistillationMapper: base_size (CUSTOM_DATASETS.BASE_SIZE) must be positive, the reference's "
                             "mapper always resizes to it")
        self.is_train, self.min_score = bool(is_train), min_score

    @classmethod
    def from_config(cls, cfg, is_train=True, device=None, class_code_to_class_id=None):
        """reference part_distillation_dataset_mapper.py:52-126"""
        pd = cfg.PART_DISTILLATION
        return cls(*cls._augmentation_args(cfg), pd.MIN_AREA_RATIO, pd.MIN_OBJECT_AREA_RATIO, device or cfg.MODEL.DEVICE,
                   base_size=cfg.CUSTOM_DATASETS.BASE_SIZE, square_base=pd.SET_IMAGE_SQUARE, class_code_to_class_id=class_code_to_class_id,
                   is_train=is_train, min_score=pd.MIN_SCORE)

    def load_annotation(self, path_tuple):
        """reference :130-164: the dict save_generated_part_labels / save_part_segmentation write (part_labels a tensor, part_scores a
        numpy array, part_ratios a tensor or absent) -> dataset dict with the parts that pass the ratio and score filters, or None"""
        ann = load_saved(os.path.join(*path_tuple), self.logger)
        if ann is None or not ann["object_ratio"] >= self.min_object_area_ratio or not ann["part_masks"]:
            return None
        parts = []
        for i, (lbl, m) in enumerate(zip(ann["part_labels"], ann["part_masks"])):
            if "part_ratios" in ann and not ann["part_ratios"][i] >= self.min_area_ratio:
                continue
            if "part_scores" in ann and not ann["part_scores"][i] >= self.min_score:
                continue
            parts.append({"segmentation": m["segmentation"], "category_id": int(lbl)})
        if not parts:
            return None
        h, w = parts[-1]["segmentation"]["size"]
        return {"file_name": ann["file_name"], "image_id": ann["image_id"], "class_code": path_tuple[1], "height": h, "width": w,
                "pseudo_annotations": parts, "gt_object_class": self.class_code_to_class_id[ann["class_code"]]}

    def _repeats(self, annos):
        return self.num_repeats if len(annos) else 0                         # nothing to retry for: one pass, zero-length instances

    def __call__(self, dataset_dict):
        if self.is_train:
            return super().__call__(dataset_dict)
        if isinstance(dataset_dict, tuple):
            dataset_dict = self.load_annotation(dataset_dict)
            if dataset_dict is None:
                return None
        from ..functions import rle as device_rle
        image = self.base_image(read_image(dataset_dict), planar=True)
        size = (int(image.shape[1]), int(image.shape[2]))
        annos = dataset_dict["pseudo_annotations"]
        classes = torch.tensor([int(a.get("category_id", -1)) for a in annos], dtype=torch.int64, device=self.device)
        masks = device_rle.decode_masks([a["segmentation"] for a in annos], size, self.device)
        keep = self.select(masks, masks.flatten(1).sum(1, dtype=torch.int32))
        padding = torch.zeros(size, dtype=torch.bool, device=self.device)
        return self._output(dataset_dict, image, padding, masks[keep], classes[keep], size)
