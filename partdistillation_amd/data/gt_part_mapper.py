"""``DeviceVOCPartsMapper`` / ``DeviceCityscapesPartMapper``: the reference's ground-truth part mappers
(data/dataset_mappers/voc_parts_mapper.py, cityscapes_part_mapper.py), which every driver builds for its test loader and
supervised_train_net.py also for its train loader, with the pixel work on the GPU (include/pd_input.h).  They produce the two fields
every evaluation branch reads: ``instances`` (the objects) and ``part_instances`` (their parts, merged per object and class when
CUSTOM_DATASETS.USE_MERGED_GT).

The augmentation list is [ResizeShortestEdge, RandomFlip (train), RandomCrop (train, INPUT.CROP.ENABLED)]: unlike the pseudo-label mappers
(device_mapper.py) the resize comes FIRST, so the flip and the crop select columns and rows of the resized image.
Host side (cheap, data-dependent control flow, vectorised numpy): the draws in detectron2's call order (restated from detectron2 0.6, which
is not in this image), ResizeShortestEdge.get_output_shape, the box transform and the box half of filter_empty_instances, the run-length
parse, Pillow's coefficient tables for the surviving window and the group table.  Device side: Pillow's two-pass bilinear resample for the
rows and columns that survive the crop (pd_resample_rows_u8 with the column tables reversed when flipped, pd_resample_cols_canvas_u8
planar) and ONE `rle_sample_groups` launch per attempt for every mask: the members are the object masks followed by all part masks, the
planes each object alone followed by the part planes (one per object and class, or one per part), and the two small count vectors that
come back decide survival — no dense full-resolution mask, no per-object / per-class loop over planes."""
import numpy as np
import torch

from ..compat import BitMasks, Instances
from ..functions.input_pipeline import nearest_index, resample_coeffs, resample_u8, rle_sample_groups, to_device, upload_image
from ..utils import rle as _rle
from .cityscapes_part_record import load_object_and_parts
from .device_mapper import random_crop, read_image

XYXY_ABS, XYWH_ABS = 0, 1                                                    # detectron2 BoxMode values


def get_output_shape(oldh, oldw, short_edge_length, max_size):
    """detectron2 0.6 ResizeShortestEdge.get_output_shape: the short edge becomes `short_edge_length` unless the long edge would pass
    `max_size`, both sides rounded with int(x + 0.5)"""
    h, w = oldh, oldw
    size = short_edge_length * 1.0
    scale = size / min(h, w)
    if h < w:
        newh, neww = size, scale * w
    else:
        newh, neww = scale * h, size
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * scale, neww * scale
    return int(newh + 0.5), int(neww + 0.5)


def transform_boxes(boxes, p):
    """XYXY boxes [k, 4] through ResizeTransform, HFlipTransform, CropTransform (apply_box: the four corners, then min / max) and
    transform_instance_annotations' clip to the output image, in float64"""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    (rh, rw), (x0, y0, cw, ch) = p["resize"], p["crop"]
    xs = b[:, [0, 2, 0, 2]] * (rw * 1.0 / p["in_w"])
    ys = b[:, [1, 1, 3, 3]] * (rh * 1.0 / p["in_h"])
    if p["flip"]:
        xs = rw - xs
    xs, ys = xs - x0, ys - y0
    out = np.stack([xs.min(1), ys.min(1), xs.max(1), ys.max(1)], axis=1)
    return np.minimum(np.maximum(out, 0.0), np.array([cw, ch, cw, ch], dtype=np.float64))


def boxes_nonempty(boxes, threshold=1e-5):
    """detectron2 Boxes.nonempty"""
    return ((boxes[:, 2] - boxes[:, 0]) > threshold) & ((boxes[:, 3] - boxes[:, 1]) > threshold)


def group_table(n_obj, part_obj, part_cls, part_ok, merged):
    """members = the n_obj object masks followed by the parts; planes = each object alone, then the part planes: with `merged` one per
    (object in order, class ascending) that has a part with part_ok, else one per part (empty when not part_ok)
    -> (group_offsets int32 [G + 1], group_members int32, part planes' object index [G - n_obj], their class [G - n_obj])"""
    part_obj, part_cls, part_ok = (np.asarray(a).reshape(-1) for a in (part_obj, part_cls, part_ok))
    groups = [[i] for i in range(n_obj)]
    g_obj, g_cls = [], []
    if merged:
        for o in range(n_obj):
            mine = np.flatnonzero((part_obj == o) & part_ok)
            for c in np.unique(part_cls[mine]):
                groups.append((n_obj + mine[part_cls[mine] == c]).tolist())
                g_obj.append(o)
                g_cls.append(int(c))
    else:
        for i in range(len(part_obj)):
            groups.append([n_obj + i] if part_ok[i] else [])
            g_obj.append(int(part_obj[i]))
            g_cls.append(int(part_cls[i]))
    offsets = np.concatenate(([0], np.cumsum([len(g) for g in groups]))).astype(np.int32)
    members = np.asarray([m for g in groups for m in g], dtype=np.int32)
    return offsets, members, np.asarray(g_obj, dtype=np.int64), np.asarray(g_cls, dtype=np.int64)


class DeviceGTPartMapper:
    """the work the two reference mappers share; the subclasses hold exactly what differs between them"""
    num_repeats = 100            # attempts with the crop before the pass without it
    min_parts = 1                # an attempt succeeds with at least this many part masks
    filter_by_box = True         # filter_empty_instances(by_box=...) on objects and parts
    part_class_key = "category_id"

    def __init__(self, is_train, min_size, max_size, sample_style="choice", crop_type=None, crop_size=None, use_merged_gt=True,
                 device="cuda", rng=None, mask_format="bitmask"):
        if mask_format != "bitmask":
            raise NotImplementedError(f"INPUT.MASK_FORMAT '{mask_format}': polygon ground truth is DevicePartImageNetMapper's "
                                      "(part_imagenet_mapper.py); this mapper maps RLE segmentations only")
        self.is_train = bool(is_train)
        self.min_size = tuple(int(s) for s in (min_size if isinstance(min_size, (tuple, list)) else (min_size, min_size)))
        self.max_size, self.sample_style = int(max_size), sample_style
        if sample_style not in ("choice", "range") or (sample_style == "range" and len(self.min_size) != 2):
            raise ValueError(f"ResizeShortestEdge: sample_style '{sample_style}' with sizes {self.min_size}")
        self.crop_type = crop_type if self.is_train else None
        self.crop_size = tuple(crop_size) if crop_size is not None else None
        self.use_merged_gt, self.device = bool(use_merged_gt), torch.device(device)
        self.rng = rng if rng is not None else np.random                     # detectron2 draws from the global numpy RNG

    @classmethod
    def _resize_args(cls, cfg, is_train):
        return cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN, cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING

    @classmethod
    def from_config(cls, cfg, is_train=True):
        if is_train and cfg.INPUT.COLOR_AUG_SSD:
            raise NotImplementedError("INPUT.COLOR_AUG_SSD (ColorAugSSDTransform, an OpenCV route) is not in the device pipeline")
        crop = is_train and cfg.INPUT.CROP.ENABLED
        return cls(is_train, *cls._resize_args(cfg, is_train), cfg.INPUT.CROP.TYPE if crop else None,
                   tuple(cfg.INPUT.CROP.SIZE) if crop else None, cfg.CUSTOM_DATASETS.USE_MERGED_GT, cfg.MODEL.DEVICE)

    # ------------------------------------------------------------------ host: parameter draws (detectron2 0.6 augmentation_impl.py)
    def draw(self, in_h, in_w, crop=True):
        """one attempt's draws in list order: ResizeShortestEdge's size, RandomFlip's uniform (train), RandomCrop's (train, enabled,
        and `crop`: the pass after the last attempt runs the list without it)"""
        rng = self.rng
        if self.sample_style == "range":
            size = rng.randint(self.min_size[0], self.min_size[1] + 1)
        else:
            size = rng.choice(self.min_size)
        rh, rw = (in_h, in_w) if size == 0 else get_output_shape(in_h, in_w, int(size), self.max_size)    # size 0: NoOpTransform
        p = {"in_h": in_h, "in_w": in_w, "resize": (rh, rw), "flip": bool(self.is_train and rng.uniform() < 0.5), "crop": (0, 0, rw, rh)}
        if self.crop_type is not None and crop:
            p["crop"] = random_crop(rng, rh, rw, self.crop_type, self.crop_size)
        return p

    # ------------------------------------------------------------------ host: tables
    @staticmethod
    def index_tables(p):
        """source column of every output column and source row of every output row: Pillow NEAREST resize, then flip, then crop"""
        (rh, rw), (x0, y0, cw, ch) = p["resize"], p["crop"]
        cols = x0 + np.arange(cw)
        if p["flip"]:
            cols = rw - 1 - cols
        return nearest_index(p["in_w"], rw)[cols].astype(np.int32), nearest_index(p["in_h"], rh)[y0:y0 + ch].astype(np.int32)

    def _dev(self, a):
        return to_device(a, self.device)

    # ------------------------------------------------------------------ device: pixels
    def transform_image(self, img, p):
        """img uint8 [H, W, 3] on the device -> uint8 [3, ch, cw]: the window of the Pillow BILINEAR full-size resize that survives
        the crop, mirrored when flipped.  The coefficient tables cover only that window; flipped, they are handed over in reverse."""
        H, W = int(img.shape[0]), int(img.shape[1])
        (rh, rw), (x0, y0, cw, ch) = p["resize"], p["crop"]
        xtab = resample_coeffs(W, rw, rw - x0 - cw if p["flip"] else x0, cw)
        if p["flip"]:
            xtab = tuple(t[::-1] for t in xtab)
        return resample_u8(img, xtab, resample_coeffs(H, rh, y0, ch))

    # ------------------------------------------------------------------ host: the record
    @staticmethod
    def _xyxy(anno):
        mode = anno.get("bbox_mode", XYXY_ABS)
        mode = int(getattr(mode, "value", mode))
        b = [float(v) for v in anno["bbox"]]
        if mode == XYWH_ABS:
            return [b[0], b[1], b[0] + b[2], b[1] + b[3]]
        if mode != XYXY_ABS:
            raise NotImplementedError(f"bbox_mode {mode}: only XYXY_ABS (0) and XYWH_ABS (1) boxes are mapped")
        return b

    def from_tuple(self, pair):
        """the (dict, part_file) records of a PATH_ONLY dataset: CityscapesPartMapper's alone"""
        raise NotImplementedError(f"{type(self).__name__}: a (dict, part_file) tuple is the input of DeviceCityscapesPartMapper only "
                                  "(CUSTOM_DATASETS.CITYSCAPES_PART.PATH_ONLY); pass a record with annotations / part_annotations")

    def parse(self, dataset_dict):
        """the static part of a record: objects without `iscrowd`, their parts flattened, boxes, classes, segmentations"""
        objs = [(i, o) for i, o in enumerate(dataset_dict["annotations"]) if o.get("iscrowd", 0) == 0]
        parts = [(k, part) for k, (i, _) in enumerate(objs) for part in dataset_dict["part_annotations"][i]]
        segs = [o["segmentation"] for _, o in objs] + [part["segmentation"] for _, part in parts]
        for s in segs:
            if not isinstance(s, dict):
                raise NotImplementedError("polygon segmentations (INPUT.MASK_FORMAT 'polygon') are not mapped by this mapper: they are "
                                          "DevicePartImageNetMapper's (part_imagenet_mapper.py); encode the masks as COCO RLE")
        rec = {"obj_index": np.asarray([i for i, _ in objs], dtype=np.int64),
               "obj_cls": np.asarray([int(o["category_id"]) for _, o in objs], dtype=np.int64),
               "obj_box": np.asarray([self._xyxy(o) for _, o in objs], dtype=np.float64).reshape(-1, 4),
               "part_obj": np.asarray([k for k, _ in parts], dtype=np.int64),
               "part_cls": np.asarray([int(part[self.part_class_key]) for _, part in parts], dtype=np.int64),
               "part_segs": [part["segmentation"] for _, part in parts], "segs": segs}
        if self.filter_by_box:
            rec["part_box"] = np.asarray([self._xyxy(part) for _, part in parts], dtype=np.float64).reshape(-1, 4)
        return rec

    def plan(self, rec, p):
        """what one attempt decides before the launch: the transformed object boxes, which objects / parts pass the box half of
        filter_empty_instances, and the group table"""
        n_obj, n_part = len(rec["obj_index"]), len(rec["part_obj"])
        obj_box = transform_boxes(rec["obj_box"], p)
        obj_ok = boxes_nonempty(obj_box) if self.filter_by_box else np.ones(n_obj, dtype=bool)
        part_ok = boxes_nonempty(transform_boxes(rec["part_box"], p)) if self.filter_by_box else np.ones(n_part, dtype=bool)
        return (obj_box, obj_ok, part_ok) + group_table(n_obj, rec["part_obj"], rec["part_cls"], part_ok, self.use_merged_gt)

    # ------------------------------------------------------------------ the call
    def __call__(self, dataset_dict):
        """dataset_dict: {"image": decoded uint8 HWC array (or "file_name" readable by Pillow), "annotations": the objects (RLE
        "segmentation", "bbox" [+ "bbox_mode", XYXY_ABS when absent], "category_id"), "part_annotations": per object a list of parts (RLE
        "segmentation", the part class, and for the Pascal flavour "bbox"), ...} -> the reference mapper's output dict, on the device.
        A (dict, part_file) tuple goes through `from_tuple` first (the Cityscapes mapper's PATH_ONLY records; None when it has no objects)"""
        if isinstance(dataset_dict, tuple):
            dataset_dict = self.from_tuple(dataset_dict)
            if dataset_dict is None:
                return None
        rec = self.parse(dataset_dict)
        img = upload_image(read_image(dataset_dict), self.device)
        H, W = int(img.shape[0]), int(img.shape[1])
        starts, offsets = _rle.segmentations_to_starts(rec["segs"], (H, W))
        runs = (self._dev(starts), self._dev(offsets))                       # once per image: the runs do not depend on the draws
        attempts = self.num_repeats if self.is_train else 0
        for attempt in range(attempts + 1):
            p = self.draw(H, W, crop=attempt < attempts)                      # after the last attempt: the list without the crop
            res = self.sample(rec, runs, p)
            if len(res["part_classes"]) >= self.min_parts or attempt == attempts:
                break
        return self._output(dataset_dict, self.transform_image(img, p), rec, res, p)

    def sample(self, rec, runs, p):
        """one launch for every mask of the attempt, one readback of the two count vectors, then the mask half of
        filter_empty_instances and the index-select of the surviving planes"""
        H, W, n_obj = p["in_h"], p["in_w"], len(rec["obj_index"])
        obj_box, obj_ok, part_ok, g_off, g_mem, g_obj, g_cls = self.plan(rec, p)
        sx, sy = (self._dev(t) for t in self.index_tables(p))
        planes, m_area, g_area = rle_sample_groups(runs[0], runs[1], H, W, sx, sy, g_off, g_mem)
        counts = torch.cat([m_area, g_area]).cpu().numpy()                   # the one synchronisation of the attempt
        m_area, g_area = counts[:len(m_area)], counts[len(m_area):]
        obj_keep = obj_ok & (m_area[:n_obj] > 0)
        of_kept = obj_keep[rec["part_obj"]]                                  # parts_list: the parts of the surviving objects
        part_keep = part_ok & of_kept & (m_area[n_obj:] > 0)
        plane_keep = obj_keep[g_obj] & (g_area[n_obj:] > 0)                  # merged: a plane lives when one of its parts does
        idx = np.concatenate((np.flatnonzero(obj_keep), n_obj + np.flatnonzero(plane_keep)))
        kept = planes[self._dev(idx)] if len(idx) else planes[:0]
        k = int(obj_keep.sum())
        return {"obj_masks": kept[:k], "part_masks": kept[k:], "obj_keep": obj_keep, "obj_box": obj_box[obj_keep], "part_keep": part_keep,
                "part_classes": g_cls[plane_keep],
                "part_obj_mapping": (np.cumsum(obj_keep) - 1)[rec["part_obj"][part_keep]],          # re-enumerated over parts_list
                "part_mapping": (np.cumsum(of_kept) - 1)[part_keep]}                                # over the flattened parts_list

    def _output(self, dataset_dict, image, rec, res, p):
        size = (p["crop"][3], p["crop"][2])
        inst = Instances(size)
        inst.gt_masks = BitMasks(res["obj_masks"].view(torch.bool))
        inst.gt_classes = self._dev(rec["obj_cls"][res["obj_keep"]])
        inst.gt_boxes = self._dev(res["obj_box"].astype(np.float32))
        inst.obj_mapping = self._dev(rec["obj_index"][res["obj_keep"]])
        parts = Instances(size)
        parts.gt_masks = BitMasks(res["part_masks"].view(torch.bool))
        parts.gt_classes = self._dev(res["part_classes"])
        if not self.use_merged_gt:
            parts.obj_mapping = self._dev(res["part_obj_mapping"])
            parts.part_mapping = self._dev(res["part_mapping"])
        out = {k: v for k, v in dataset_dict.items() if k not in ("annotations", "part_annotations", "image")}
        out.update(image=image, instances=inst, part_instances=parts,
                   orig_part_maps=[s for s, keep in zip(rec["part_segs"], res["part_keep"]) if keep])
        return out


class DeviceVOCPartsMapper(DeviceGTPartMapper):
    """reference VOCPartsMapper: the TRAIN sizes in both modes, 100 attempts that need MORE THAN ONE part mask, the box and the mask
    filter, the class of a part = its `orig_part_category_id`"""
    num_repeats = 100
    min_parts = 2
    filter_by_box = True
    part_class_key = "orig_part_category_id"


class DeviceCityscapesPartMapper(DeviceGTPartMapper):
    """reference CityscapesPartMapper: ResizeShortestEdge(MIN_SIZE_TEST, MAX_SIZE_TEST, "choice") in test mode, 20 attempts that need at
    least one part mask, the mask filter only (its parts carry the whole image as their box), the class of a part = `part_category_id`"""
    num_repeats = 20
    min_parts = 1
    filter_by_box = False
    part_class_key = "part_category_id"

    @classmethod
    def _resize_args(cls, cfg, is_train):
        if is_train:
            return super()._resize_args(cfg, is_train)
        return cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, "choice"

    def from_tuple(self, pair):
        """reference :201-211: (record, gtFinePanopticParts.tif path or int32 uid map) -> the record with the objects and parts of
        `load_object_and_parts` (cityscapes_part_record.py), a copy: the reference writes them into its input; None when the record has no
        annotation with a segmentation.  The panoptic_parts decoding exists as a device kernel only: a mapper that is not on a GPU
        refuses the tuple before it looks at the record or the file."""
        if self.device.type != "cuda":
            raise NotImplementedError("the (dict, part_file) input of CityscapesPartMapper reads the part ids with panoptic_parts, which is "
                                      "restated here as a device kernel only (pd_pp_decode_uids): on a mapper that is not on a GPU pass "
                                      "records whose annotations / part_annotations are already RLE")
        record, part_file = pair
        objects, parts = load_object_and_parts(record, part_file, self.device)
        if objects is None:
            return None
        return dict(record, annotations=objects, part_annotations=parts)
