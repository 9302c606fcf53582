"""Cityscapes-Part ground truth from the dataset's own files, with the pixel work on the GPU: the reference's `load_object_and_parts`
(data/dataset_mappers/cityscapes_part_mapper.py:40-87, run by its mapper for every (dict, part_file) tuple of a PATH_ONLY dataset) and
the per-image part of its registration (data/datasets/register_cityscapes_part.py:128-142).

The reference decodes the 1024 x 2048 int32 panoptic-parts TIFF, runs panoptic_parts.decode_uids, one np.where and np.unique per object
and one pycocotools encode per object and per part, all on the host.  Here the uid map is uploaded once, `decode_uids` turns it into ONE
uint8 part-label map, the object planes come from the existing decoders (`decode_masks` for COCO RLE, `rasterize_polygons` +
`rle_sample_groups` with identity tables for detectron2's polygon lists: the OR of an object's polygons, as polygons_to_bitmask makes
it), and two run-table reads finish the image: `plane_runs` (binary) for the objects' own RLE and `encode_plane_labels` for "the part ids
under each object's mask" — no dense per-part plane and no per-object label plane is written.

A "segmentation" produced here is exactly utils.rle.encode(mask) ({"size", "counts" bytes}), this project's stand-in for
mask_util.encode.  panoptic_parts, pycocotools and detectron2 are not available to test against: parity with them is UNPINNED.
Left out: walking the Cityscapes directory tree, the shapely overlap resolution inside detectron2's load_cityscapes_instances, and
`label_percentage` (all of them belong to the caller that produces the instance records)."""
import copy

import numpy as np
import torch

from ..functions import panoptic_parts as _pp
from ..functions import rle as _drle
from ..functions.input_pipeline import rle_sample_groups, to_device
from ..functions.polygon import rasterize_polygons
from ..utils import rle as _rle

PART_CLASSES = (
    "person-torso", "person-head", "person-arm", "person-leg",
    "rider-torso", "rider-head", "rider-arm", "rider-leg",
    "car-window", "car-wheel", "car-light", "car-license plate", "car-chassis",
    "truck-window", "truck-wheel", "truck-light", "truck-license plate", "truck-chassis",
    "bus-window", "bus-wheel", "bus-light", "bus-license plate", "bus-chassis",
)
PART_BASE_ID = {0: 0, 1: 4, 2: 8, 3: 13, 4: 18}
OBJECT_CLASSES = ("person", "rider", "car", "truck", "bus")


def read_part_map(part, height, width):
    """a gtFinePanopticParts.tif path (read with Pillow), or an int32 array / tensor -> the uid map, int32 [height, width] (numpy, or the
    tensor itself).  ValueError when it is anything else: the reference would broadcast or fail somewhere inside np.where."""
    if isinstance(part, (str, bytes)) or hasattr(part, "__fspath__"):
        from PIL import Image
        with Image.open(part) as im:
            part = np.array(im)
    dtype, shape = (part.dtype, tuple(part.shape)) if torch.is_tensor(part) else (np.asarray(part).dtype, np.asarray(part).shape)
    if dtype not in (torch.int32, np.dtype(np.int32)) or tuple(shape) != (int(height), int(width)):
        raise ValueError(f"panoptic-parts map: int32 [{int(height)}, {int(width)}] expected, got {dtype} {list(shape)}")
    return part if torch.is_tensor(part) else np.ascontiguousarray(part)


def _object_planes(segmentations, height, width, device):
    """the kept objects' segmentations (COCO RLE dicts or lists of polygons, detectron2's annotations_to_instances with "bitmask")
    -> uint8 / bool [n, height, width] on the device"""
    rle_at = [i for i, s in enumerate(segmentations) if isinstance(s, dict)]
    poly_at = [i for i, s in enumerate(segmentations) if isinstance(s, list)]
    if len(rle_at) + len(poly_at) != len(segmentations):
        bad = next(s for s in segmentations if not isinstance(s, (dict, list)))
        raise ValueError(f"Cannot convert segmentation of type '{type(bad)}' to BitMasks! Supported here: COCO-style RLE as a dict, "
                         "or a list of polygons")
    from_rle = _drle.decode_masks([segmentations[i] for i in rle_at], (height, width), device).view(torch.uint8) if rle_at else None
    from_poly = None
    if poly_at:
        polys = [p for i in poly_at for p in segmentations[i]]
        starts, offsets = rasterize_polygons(polys, height, width, device)
        sx, sy = to_device(np.arange(width, dtype=np.int32), device), to_device(np.arange(height, dtype=np.int32), device)
        g_off = np.concatenate(([0], np.cumsum([len(segmentations[i]) for i in poly_at]))).astype(np.int32)
        from_poly = rle_sample_groups(starts, offsets, height, width, sx, sy, g_off, np.arange(len(polys), dtype=np.int32))[0]
    if from_poly is None or from_rle is None:
        return from_rle if from_poly is None else from_poly
    planes = torch.empty((len(segmentations), height, width), dtype=torch.uint8, device=device)
    planes[to_device(np.asarray(rle_at, dtype=np.int64), device)] = from_rle
    planes[to_device(np.asarray(poly_at, dtype=np.int64), device)] = from_poly
    return planes


def _part_labels(uids, device):
    """the uid map -> (part-label map uint8 [H, W] on the device: the pid where it is > 0, else 0; the decode's `check`)"""
    if torch.device(device).type != "cuda":
        raise RuntimeError("load_object_and_parts runs on the GPU only (no CPU fallback in partdistillation_amd)")
    d = _pp.decode_uids(uids.to(device) if torch.is_tensor(uids) else to_device(uids, device), want=("part_label",))
    return d["part_label"], d.check


def _rle_of_runs(starts, first_value, size):
    """utils.rle.encode(mask) from the mask's run starts"""
    counts = np.diff(np.asarray(starts, dtype=np.int64), append=size[0] * size[1])
    if len(counts) and first_value:
        counts = np.concatenate(([0], counts))
    return {"size": [int(size[0]), int(size[1])], "counts": _rle.counts_to_string(counts)}


def load_object_and_parts(record, part, device="cuda"):
    """record: a detectron2 Cityscapes instance record ("height", "width", "annotations" with "category_id", "bbox", "bbox_mode",
    "segmentation"); part: see `read_part_map` -> (object_instances, part_instances) as the reference builds them: the objects with
    category_id < 5 in order, each with its possibly empty list of parts; (None, None) when there is no annotation with a segmentation.
    The record is not modified."""
    annos = record["annotations"]
    if not len(annos) or "segmentation" not in annos[0]:                      # annotations_to_instances sets no gt_masks
        return None, None
    height, width = int(record["height"]), int(record["width"])
    uids = read_part_map(part, height, width)
    kept = [a for a in annos if int(a["category_id"]) < 5]
    if not kept:
        return [], []
    planes = _object_planes([a["segmentation"] for a in kept], height, width, device)
    labels, check = _part_labels(uids, device)
    offsets, starts, values, _ = _drle.plane_runs(planes, binary=True)                       # run-table read 1: the objects
    parts, _ = _drle.encode_plane_labels(planes, labels)                                     # run-table read 2: the labels under them
    check()                                                                                  # after the blocking reads: no wait of its own
    object_instances, part_instances = [], []
    for i, a in enumerate(kept):
        cat = int(a["category_id"])
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        object_instances.append({"object_category": OBJECT_CLASSES[cat], "object_category_id": cat, "category_id": cat,
                                 "bbox": a["bbox"], "bbox_mode": a["bbox_mode"],
                                 "segmentation": _rle_of_runs(starts[lo:hi], hi > lo and values[lo], (height, width))})
        mine = []
        for pid, entry in parts[i]:
            part_id = PART_BASE_ID[cat] + pid - 1
            seg = entry["segmentation"]
            mine.append({"part_category": PART_CLASSES[part_id], "part_category_id": part_id, "category_id": part_id, "object_index": i,
                         "segmentation": {"size": seg["size"], "counts": seg["counts"].encode("ascii")}})
        part_instances.append(mine)
    return object_instances, part_instances


def cityscapes_part_records(record, part, for_segmentation, device="cuda"):
    """the per-image part of the reference's registration without PATH_ONLY (register_cityscapes_part.py:128-142): with
    `for_segmentation` one deep copy of the record per object that has parts, holding that object alone; otherwise the record (a shallow
    copy) with "annotations" / "part_annotations" when there is any object.  The reference's own `if len(part_dict) > 0` (:84) keeps
    every object once the image has had one part and is a NameError before; here every object is kept."""
    object_instances, part_instances = load_object_and_parts(record, part, device)
    if not part_instances:
        return
    if for_segmentation:
        for obj, parts in zip(object_instances, part_instances):
            if len(parts) > 0:
                one = copy.deepcopy(record)
                one["annotations"], one["part_annotations"] = [obj], [parts]
                yield one
    else:
        yield dict(record, annotations=object_instances, part_annotations=part_instances)
