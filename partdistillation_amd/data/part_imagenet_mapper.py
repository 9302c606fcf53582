"""``DevicePartImageNetMapper``: the reference's PartImageNetMapper (data/dataset_mappers/part_imagenet_mapper.py), which six drivers build
for a `part_imagenet` test set and supervised_train_net.py also for training, with the pixel work on the GPU.  Unlike its two siblings
(gt_part_mapper.py) the ground truth is POLYGONS: every annotation of the COCO record is a part, the polygons go through the resize and
the flip as vertices and are rasterised AT THE OUTPUT RESOLUTION, so nothing about the masks can be prepared once per image — the
rasterisation itself is the per-image device work (include/pd_poly.h, functions/polygon.py: pycocotools' rleFrPoly restated).

The augmentation list is [ResizeShortestEdge(MIN_SIZE_TRAIN, MAX_SIZE_TRAIN, MIN_SIZE_TRAIN_SAMPLING)] in BOTH modes, + RandomFlip in
train mode.  Host side: the draws, the vertex transform in float64, the float32 boxes of PolygonMasks.get_bounding_boxes and the box half of
filter_empty_instances (for PolygonMasks the mask half is always true, so SURVIVAL IS DECIDED BY BOXES ALONE: the retry loop launches
nothing and nothing is read back), the exact table offsets and the group table.  Device side, once per image: the Pillow-exact image
resample (pd_resample_rows_u8, pd_resample_cols_canvas_u8), ONE pd_poly_crossings_i32 for the polygons of the surviving parts and ONE
`rle_sample_groups` with identity index tables that ORs them into planes: plane 0 = all members (the object), then one plane per
unique class (USE_MERGED_GT) or per surviving part.  One small upload carries the vertices and every table; there is no synchronisation.

UNPINNED: pycocotools and detectron2 are not available to test against; the rasteriser and the draw order are restatements
(tests/poly_oracle.py pins the restatement against an independent even-odd test).  REFUSED: INPUT.CROP.ENABLED in train mode
(detectron2's CropTransform.apply_polygons clips with shapely, which is absent and whose output cannot be restated bit for bit; no shipped
script or YAML enables the crop for this mapper) and INPUT.COLOR_AUG_SSD."""
import os

import numpy as np
import torch

from ..compat import BitMasks, Instances
from ..functions import polygon as _poly
from ..functions.input_pipeline import rle_sample_groups, upload_image
from .device_mapper import load_cpu, read_image
from .gt_part_mapper import DeviceGTPartMapper, boxes_nonempty

MAPPING_22K = "metadata/imagenet1k_to_22k_mapping.pkl"


def correct_part_imagenet_path(file_name):
    """dir/n0123_456.JPEG -> (dir/n0123/n0123_456.JPEG, "n0123"): PartImageNet's records name the image without its class folder.  The
    reference rewrites its input dict in place; here both values are returned and the input stays as it is."""
    parts = file_name.split("/")
    code = parts[-1].split("_")[0]
    return os.path.join("/".join(parts[:-1]), code, parts[-1]), code


def polygon_boxes(parts):
    """PolygonMasks.get_bounding_boxes: per part the min / max over all vertices of all its polygons, taken in float32, unclipped
    parts: list of lists of float64 [k, 2] -> float32 [n, 4] XYXY"""
    out = np.zeros((len(parts), 4), dtype=np.float32)
    for i, polys in enumerate(parts):
        pts = np.concatenate(polys).astype(np.float32)
        out[i, :2], out[i, 2:] = pts.min(axis=0), pts.max(axis=0)
    return out


class DevicePartImageNetMapper(DeviceGTPartMapper):
    """reference PartImageNetMapper.  __call__ returns None in test mode when no annotation has iscrowd == 0 (as the reference does); in
    train mode the reference crashes on that None — here a ValueError names the file.  Where every part is filtered out the reference's
    merged branch crashes in torch.stack([]); here the result has zero part planes and an empty object mask in both branches."""
    num_repeats = 20             # attempts before the pass with the EMPTY augmentation list: no resize, no flip, no draw

    def __init__(self, is_train, min_size, max_size, sample_style="choice", use_merged_gt=True, device="cuda", rng=None,
                 class_code_to_class_id=None):
        super().__init__(is_train, min_size, max_size, sample_style, None, None, use_merged_gt, device, rng)
        self.class_code_to_class_id = class_code_to_class_id if class_code_to_class_id is not None else {}   # no MetadataCatalog here

    @classmethod
    def from_config(cls, cfg, is_train=True, class_code_to_class_id=None):
        """class_code_to_class_id: the imagenet_1k_meta_train table (class code -> class id) the reference reads from its MetadataCatalog;
        with "22k" in DATASETS.TRAIN[0] the ids go through metadata/imagenet1k_to_22k_mapping.pkl, as in the reference"""
        if is_train and cfg.INPUT.COLOR_AUG_SSD:
            raise NotImplementedError("INPUT.COLOR_AUG_SSD (ColorAugSSDTransform, an OpenCV route) is not in the device pipeline")
        if is_train and cfg.INPUT.CROP.ENABLED:
            raise NotImplementedError("INPUT.CROP.ENABLED with polygon ground truth: detectron2's CropTransform.apply_polygons clips with "
                                      "shapely, which is not available and not restated; PartImageNet is mapped without the crop")
        table = dict(class_code_to_class_id) if class_code_to_class_id is not None else {}
        train = cfg.DATASETS.TRAIN
        if len(train) and "22k" in train[0]:
            if not os.path.exists(MAPPING_22K):
                raise FileNotFoundError(f"{MAPPING_22K} is needed to map the ImageNet-1k class ids to the 22k vocabulary of "
                                        f"DATASETS.TRAIN[0] = '{train[0]}'")
            to_22k = load_cpu(MAPPING_22K)
            table = {k: to_22k[i] for k, i in table.items()}
        return cls(is_train, *cls._resize_args(cfg, is_train), cfg.CUSTOM_DATASETS.USE_MERGED_GT, cfg.MODEL.DEVICE,
                   class_code_to_class_id=table)

    # ------------------------------------------------------------------ host: the record
    def parse(self, dataset_dict):
        """the parts of the record: annotations without `iscrowd`, their classes and polygons as float64 [k, 2]
        ValueError for a polygon with an odd number of coordinates or fewer than 6 (PolygonMasks)"""
        annos = [a for a in dataset_dict["annotations"] if a.get("iscrowd", 0) == 0]
        polys = []
        for a in annos:
            seg = a["segmentation"]
            if isinstance(seg, dict) or len(seg) == 0:
                raise ValueError("PartImageNet parts are lists of polygons; RLE parts belong to DeviceVOCPartsMapper / DeviceCityscapesPartMapper")
            mine = []
            for p in seg:
                p = np.asarray(p, dtype=np.float64).reshape(-1)
                if p.size % 2 != 0 or p.size < 6:
                    raise ValueError(f"Cannot create a polygon from {p.size} coordinates.")
                mine.append(p.reshape(-1, 2))
            polys.append(mine)
        return {"part_cls": np.asarray([int(a["category_id"]) for a in annos], dtype=np.int64), "part_polys": polys}

    @staticmethod
    def identity(in_h, in_w):
        """the pass with the empty augmentation list"""
        return {"in_h": in_h, "in_w": in_w, "resize": (in_h, in_w), "flip": False, "crop": (0, 0, in_w, in_h)}

    @staticmethod
    def transform_polygons(polys, p):
        """ResizeTransform.apply_coords then HFlipTransform.apply_coords on the vertices, float64"""
        rh, rw = p["resize"]
        out = []
        for q in polys:
            q = q.copy()
            q[:, 0] = q[:, 0] * (rw * 1.0 / p["in_w"])
            q[:, 1] = q[:, 1] * (rh * 1.0 / p["in_h"])
            if p["flip"]:
                q[:, 0] = rw - q[:, 0]
            out.append(q)
        return out

    def plan(self, rec, p):
        """what one attempt decides on the host: the transformed polygons, the float32 boxes and which parts survive them"""
        parts = [self.transform_polygons(polys, p) for polys in rec["part_polys"]]
        boxes = polygon_boxes(parts)
        return parts, boxes, boxes_nonempty(boxes)

    @staticmethod
    def group_table(part_cls, poly_part, merged):
        """members = the polygons of the surviving parts (poly_part[m] = the part of polygon m, parts numbered over the survivors);
        plane 0 = every member (the object), then one plane per unique class ascending (`merged`) or per part
        -> (group_offsets int32 [G + 1], group_members int32, the part planes' classes int64)"""
        poly_part = np.asarray(poly_part, dtype=np.int64)
        groups = [np.arange(len(poly_part))]
        if merged:
            classes = np.unique(part_cls)
            groups += [np.flatnonzero(part_cls[poly_part] == c) for c in classes]
        else:
            classes = part_cls
            groups += [np.flatnonzero(poly_part == i) for i in range(len(part_cls))]
        offsets = np.concatenate(([0], np.cumsum([len(g) for g in groups]))).astype(np.int32)
        return offsets, np.concatenate(groups).astype(np.int32), np.asarray(classes, dtype=np.int64)

    # ------------------------------------------------------------------ device: the masks
    def rasterize(self, polys, h, w, group_offsets, group_members):
        """polys: the member polygons at the h x w output -> planes uint8 [G, h, w].  One upload (vertices, polygon offsets, table offsets,
        identity index tables, group table), pd_poly_crossings_i32, `rle_sample_groups`; nothing comes back (the two pixel-count
        vectors the sampling also writes are not read: survival was decided by the boxes)"""
        if self.device.type != "cuda":
            raise RuntimeError("the device input pipeline runs on the GPU only (no CPU fallback in partdistillation_amd)")
        extra = (np.arange(w, dtype=np.int32), np.arange(h, dtype=np.int32), group_offsets, np.concatenate((group_members, [0])))
        starts, offsets, (sx, sy, d_go, d_gm) = _poly.rasterize_polygons(polys, h, w, self.device, extra)
        return rle_sample_groups(starts, offsets, h, w, sx, sy, group_offsets, group_members, uploaded=(d_go, d_gm))[0]

    # ------------------------------------------------------------------ the call
    def __call__(self, dataset_dict):
        """dataset_dict: a COCO record {"file_name": dir/n0123_456.JPEG, "image"?: decoded uint8 HWC array (else the corrected file_name is
        read with Pillow), "annotations": the parts ("category_id", "segmentation" = list of flat polygons, "iscrowd"?; "bbox" is
        ignored: the reference overwrites it), ...} -> the reference mapper's output dict on the device, or None (test mode, no
        annotation); the input is not modified"""
        file_name, class_code = correct_part_imagenet_path(dataset_dict["file_name"])
        rec = self.parse(dataset_dict)
        if len(rec["part_cls"]) == 0:
            if self.is_train:
                raise ValueError(f"{file_name}: no annotation with iscrowd == 0 (the reference mapper crashes on such a record in train mode)")
            return None
        object_class = self.class_code_to_class_id[class_code]
        img = upload_image(read_image(dict(dataset_dict, file_name=file_name)), self.device)
        H, W = int(img.shape[0]), int(img.shape[1])
        attempts = self.num_repeats if self.is_train else 1
        for attempt in range(attempts + (1 if self.is_train else 0)):
            p = self.draw(H, W) if attempt < attempts else self.identity(H, W)
            parts, boxes, ok = self.plan(rec, p)
            if ok.any() or not self.is_train:
                break
        keep = np.flatnonzero(ok)
        members = [q for i in keep for q in parts[i]]
        poly_part = [k for k, i in enumerate(keep) for _ in parts[i]]
        g_off, g_mem, classes = self.group_table(rec["part_cls"][keep], poly_part, self.use_merged_gt)
        rh, rw = p["resize"]
        planes = self.rasterize(members, rh, rw, g_off, g_mem).view(torch.bool)
        inst = Instances((rh, rw))
        inst.gt_masks = BitMasks(planes[:1])
        inst.gt_classes = self._dev(np.asarray([object_class], dtype=np.int64))
        part_inst = Instances((rh, rw))
        part_inst.gt_masks = BitMasks(planes[1:])
        part_inst.gt_classes = self._dev(classes)
        if not self.use_merged_gt:
            part_inst.gt_boxes = self._dev(boxes[keep])
        out = {k: v for k, v in dataset_dict.items() if k not in ("annotations", "image")}
        out.update(file_name=file_name, class_code=class_code, height=rh, width=rw, image=self.transform_image(img, p), instances=inst,
                   part_instances=part_inst)
        return out
