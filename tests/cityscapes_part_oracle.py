"""Test helper (not collected): the reference's Cityscapes-Part ground truth restated in numpy — the published panoptic-parts uid table
(panoptic_parts.decode_uids), `load_object_and_parts` of data/dataset_mappers/cityscapes_part_mapper.py:40-87 and of
data/datasets/register_cityscapes_part.py:37-88, literally (np.where(mask, pids, -1), np.unique, > 0, one encode per object and part),
and the per-image part of the registration (:128-142).  utils.rle.encode stands in for mask_util.encode, poly_oracle.mask for
polygons_to_bitmask.  panoptic_parts, pycocotools and detectron2 are absent: parity with them is UNPINNED."""
import copy

import numpy as np

import poly_oracle as P
from partdistillation_amd.utils import rle

PART_CLASSES = (
    "person-torso", "person-head", "person-arm", "person-leg",
    "rider-torso", "rider-head", "rider-arm", "rider-leg",
    "car-window", "car-wheel", "car-light", "car-license plate", "car-chassis",
    "truck-window", "truck-wheel", "truck-light", "truck-license plate", "truck-chassis",
    "bus-window", "bus-wheel", "bus-light", "bus-license plate", "bus-chassis",
)
PART_BASE_ID = {0: 0, 1: 4, 2: 8, 3: 13, 4: 18}
OBJECT_CLASSES = ("person", "rider", "car", "truck", "bus")
# uid, sid, iid, pid: written by hand from the format's description
HAND_TABLE = ((0, 0, -1, -1), (1, 1, -1, -1), (99, 99, -1, -1), (100, 0, 100, -1), (999, 0, 999, -1), (1000, 1, 0, -1),
              (24012, 24, 12, -1), (99999, 99, 999, -1), (100000, 1, 0, 0), (2401203, 24, 12, 3), (2600000, 26, 0, 0),
              (9999999, 99, 999, 99))
MAX_UID = 9999999


# ------------------------------------------------------------------------------------------------ the uid table
def decode_uids(uids):
    """int array -> (sids, iids, pids) int32; ValueError on a uid outside [0, 9 999 999]"""
    u = np.asarray(uids).astype(np.int64)
    if ((u < 0) | (u > MAX_UID)).any():
        raise ValueError("uid outside the encoding")
    short, mid = u <= 99, (u >= 100) & (u <= 99999)
    sids = np.where(short, u, np.where(mid, u // 1000, u // 100000))
    iids = np.where(short, -1, np.where(mid, u % 1000, (u // 100) % 1000))
    pids = np.where(short | mid, -1, u % 100)
    return sids.astype(np.int32), iids.astype(np.int32), pids.astype(np.int32)


def part_label(uids):
    pids = decode_uids(uids)[2]
    return np.where(pids > 0, pids, 0).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ run tables
def runs_table(vplanes):
    """[n, H, W] -> (offsets int32 [n + 1], starts int32, values uint8, nonzero int64 [n]): the runs of every plane's column-major
    flattening, a plain loop over the pixels' changes"""
    offsets, starts, values, nonzero = [0], [], [], []
    for v in vplanes:
        flat = np.asarray(v).T.ravel()
        at = [0] + [i for i in range(1, flat.size) if flat[i] != flat[i - 1]] if flat.size else []
        starts += at
        values += [int(flat[i]) for i in at]
        offsets.append(len(starts))
        nonzero.append(int(np.count_nonzero(flat)))
    return (np.asarray(offsets, dtype=np.int32), np.asarray(starts, dtype=np.int32), np.asarray(values, dtype=np.uint8),
            np.asarray(nonzero, dtype=np.int64))


def plane_label_runs(planes, labels):
    return runs_table([np.where(p, labels, 0) for p in np.asarray(planes)])


def encode_plane_labels(planes, labels):
    out, counts = [], np.zeros((len(planes), 256), dtype=np.int64)
    for i, p in enumerate(np.asarray(planes)):
        v = np.where(p, labels, 0)
        counts[i] = np.bincount(v.ravel(), minlength=256)
        present = [int(l) for l in np.unique(v) if l > 0]
        out.append(list(zip(present, rle.labels_to_coco_json(v, present))))
    return out, counts


# ------------------------------------------------------------------------------------------------ the reference's functions
def object_mask(segmentation, h, w):
    """annotations_to_instances(mask_format="bitmask") of one annotation: an RLE dict decoded, a list of polygons OR-ed"""
    if isinstance(segmentation, dict):
        return rle.decode(segmentation)
    out = np.zeros((h, w), dtype=bool)
    for poly in segmentation:
        out |= P.mask(poly, h, w)
    return out


def load_object_and_parts(record, uids, registration=False):
    """the mapper's version; `registration`: register_cityscapes_part.py's, whose `if len(part_dict) > 0` is taken as always true"""
    annos = record["annotations"]
    h, w = record["height"], record["width"]
    if not (len(annos) and "segmentation" in annos[0]):
        return None, None
    classes = np.asarray([a["category_id"] for a in annos])
    masks = np.stack([object_mask(a["segmentation"], h, w) for a in annos])
    obj_classes, obj_masks = classes[classes < 5], masks[classes < 5]
    kept = [annos[i] for i in range(len(classes)) if classes[i] < 5]
    pids = decode_uids(uids)[2]
    object_instances, part_instances = [], []
    for instance_id, object_category_id in enumerate(obj_classes):
        object_category_id = int(object_category_id)
        object_dict = {"object_category": OBJECT_CLASSES[object_category_id],
                       "object_category_id": object_category_id,
                       "category_id": object_category_id,
                       "bbox": kept[instance_id]["bbox"],
                       "bbox_mode": kept[instance_id]["bbox_mode"],
                       "segmentation": rle.encode(obj_masks[instance_id])}
        part_map = np.where(obj_masks[instance_id], pids, -1)
        part_instances_per_object = []
        for _pid in np.unique(part_map):
            if _pid > 0:
                part_id = PART_BASE_ID[object_category_id] + int(_pid) - 1
                part_instances_per_object.append({"part_category": PART_CLASSES[part_id],
                                                  "part_category_id": part_id,
                                                  "category_id": part_id,
                                                  "object_index": instance_id,
                                                  "segmentation": rle.encode(np.where(part_map == _pid, True, False))})
        object_instances.append(object_dict)
        part_instances.append(part_instances_per_object)
    return object_instances, part_instances


def records(record, uids, for_segmentation):
    """register_cityscapes_part.py:128-142 for one image -> list of records"""
    loaded = load_object_and_parts(record, uids, registration=True)
    out = []
    if loaded[0] is None:
        return out
    object_instances, part_instances = loaded
    if for_segmentation:
        if len(part_instances) > 0:
            for object_annotation, part_annotations in zip(object_instances, part_instances):
                if len(part_annotations) > 0:
                    new = copy.deepcopy(record)
                    new["annotations"] = [object_annotation]
                    new["part_annotations"] = [part_annotations]
                    out.append(new)
    elif len(part_instances) > 0:
        out.append(dict(record, annotations=object_instances, part_annotations=part_instances))
    return out


# ------------------------------------------------------------------------------------------------ scenes
# (category, polygons in fractions of (W, H)): a car, a class-6 object (dropped), a person over pixels without a part id, a bus and a
# rider of two polygons that overlap
OBJECTS = ((2, [[0.05, 0.10, 0.45, 0.12, 0.40, 0.55, 0.08, 0.50]]),
           (6, [[0.50, 0.05, 0.70, 0.05, 0.60, 0.30]]),
           (0, [[0.75, 0.10, 0.95, 0.10, 0.95, 0.45, 0.75, 0.45]]),
           (4, [[0.10, 0.60, 0.60, 0.60, 0.60, 0.95, 0.10, 0.95]]),
           (1, [[0.40, 0.50, 0.80, 0.55, 0.70, 0.90], [0.82, 0.60, 0.97, 0.60, 0.90, 0.97]]))


def scene(rng, H, W, polygons):
    """-> (record with five objects as polygon lists or as the RLE of the same masks, uid map int32 [H, W] mixing all three uid forms)"""
    annos, masks = [], []
    for cat, polys in OBJECTS:
        polys = [(np.asarray(p).reshape(-1, 2) * [W, H] + 0.3).reshape(-1).tolist() for p in polys]
        m = object_mask(polys, H, W)
        ys, xs = np.nonzero(m)
        annos.append({"category_id": cat, "iscrowd": 0, "bbox": [float(xs.min()), float(ys.min()), float(xs.max() + 1), float(ys.max() + 1)],
                      "bbox_mode": 0, "segmentation": polys if polygons else rle.encode(m)})
        masks.append(m)
    ys, xs = np.mgrid[0:H, 0:W]
    band = (xs * 8) // W                                                      # eight vertical bands
    sid, iid, pid = 24 + band % 5, (band * 7 + ys // 5) % 1000, (ys // 3 + band) % 6
    uids = np.where(band % 3 == 0, sid, np.where(band % 3 == 1, sid * 1000 + iid, sid * 100000 + iid * 100 + pid))
    uids = np.where(ys % 4 == 3, sid * 100000 + iid * 100 + pid, uids)      # rows with part ids cross every band
    uids = np.where(masks[2], np.where(xs % 2 == 0, 24012, 2401200), uids)   # the person: no pid, or pid 0
    image = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    record = {"file_name": "aachen_000000_000019_leftImg8bit.png", "image_id": "aachen_000000_000019", "height": H, "width": W,
              "annotations": annos, "image": image}
    return record, uids.astype(np.int32)
