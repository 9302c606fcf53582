"""DevicePartImageNetMapper end to end on the device against the reference's mapper restated on the literal rasteriser and the
Pillow-exact image chain (tests/poly_oracle.py).  Everything is integer arithmetic or float32 boxes computed the same way: every comparison
is exact equality."""
import copy
import types

import numpy as np
import pytest
import torch

import poly_oracle as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
CLASS_MAP = {"n0123": 7, "n0456": 3}
H, W, SIZES, MAX_SIZE = 40, 56, (32,), 60                                  # 40 x 56 -> 32 x 45


def _mapper(is_train, merged, rng, sizes=SIZES):
    from partdistillation_amd.data import DevicePartImageNetMapper
    return DevicePartImageNetMapper(is_train, sizes, MAX_SIZE, "choice", use_merged_gt=merged, device=DEV, rng=rng,
                                    class_code_to_class_id=CLASS_MAP)


def _record(parts, seed=0, h=H, w=W, code="n0123", **extra):
    """parts: [(class, [flat polygons])] -> a COCO record with the decoded image attached"""
    image = np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    rec = {"file_name": f"data/val/{code}_77.JPEG", "image_id": 77, "height": h, "width": w, "image": image,
           "annotations": [{"category_id": c, "bbox": [0.0, 0.0, 1.0, 1.0], "bbox_mode": 1, "segmentation": [list(map(float, q)) for q in polys]}
                           for c, polys in parts]}
    rec.update(extra)
    return rec


def _scene():
    """four parts: class 5 twice (merging has work to do), one part made of two polygons, float vertices; they overlap a little"""
    return [(5, [[3.2, 4.1, 25.7, 3.3, 22.4, 18.9, 6.5, 21.0]]),
            (2, [[20.5, 10.5, 50.0, 8.0, 53.5, 30.2, 30.0, 36.6, 18.0, 25.0]]),
            (5, [[5.0, 24.0, 16.0, 24.0, 16.0, 37.0, 5.0, 37.0], [40.2, 1.0, 54.9, 2.0, 47.0, 7.5]]),
            (1, [[28.0, 30.0, 44.4, 31.3, 36.1, 39.8]])]


def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[2] == sb[2] and np.array_equal(sa[1], sb[1])


def _assert_output(out, want, record, merged):
    assert "annotations" not in out and out["image_id"] == record["image_id"]
    assert out["file_name"] == want["file_name"] and out["class_code"] == want["class_code"]
    assert (out["height"], out["width"]) == want["size"]
    inst, parts = out["instances"], out["part_instances"]
    assert out["image"].dtype == torch.uint8 and out["image"].is_cuda and np.array_equal(out["image"].cpu().numpy(), want["image"])
    assert inst.image_size == want["size"] == parts.image_size == tuple(out["image"].shape[1:])
    for t in (inst.gt_masks.tensor, inst.gt_classes, parts.gt_masks.tensor, parts.gt_classes):
        assert t.is_cuda
    assert inst.gt_masks.tensor.dtype == torch.bool and parts.gt_masks.tensor.dtype == torch.bool
    assert inst.gt_classes.dtype == torch.int64 and parts.gt_classes.dtype == torch.int64
    assert tuple(inst.gt_masks.tensor.shape) == (1,) + want["size"] and np.array_equal(inst.gt_masks.tensor.cpu().numpy(), want["obj_masks"])
    assert inst.gt_classes.tolist() == want["obj_classes"] and not inst.has("gt_boxes")
    assert tuple(parts.gt_masks.tensor.shape) == want["part_masks"].shape
    assert np.array_equal(parts.gt_masks.tensor.cpu().numpy(), want["part_masks"]) and parts.gt_classes.tolist() == want["part_classes"]
    if merged:
        assert not parts.has("gt_boxes")
    else:
        assert parts.gt_boxes.dtype == torch.float32 and parts.gt_boxes.is_cuda
        assert np.array_equal(parts.gt_boxes.cpu().numpy(), want["part_boxes"])


@pytest.mark.parametrize("merged", [True, False])
@pytest.mark.parametrize("is_train", [True, False])
def test_mapper_against_the_oracle(is_train, merged):
    record = _record(_scene(), extra_key="kept")
    before = copy.deepcopy(record)
    flips = set()
    for seed in range(3 if is_train else 1):
        mine, theirs = np.random.RandomState(seed), np.random.RandomState(seed)
        want, attempts, fallback = P.call(record, record["image"], theirs, is_train, SIZES, MAX_SIZE, "choice", merged, CLASS_MAP)
        out = _mapper(is_train, merged, mine)(record)
        _assert_output(out, want, record, merged)
        assert _same_state(mine, theirs) and not fallback and attempts == int(is_train) and out["extra_key"] == "kept"
        assert want["size"] == (32, 45) and want["obj_masks"].any() and want["part_classes"] == ([1, 2, 5] if merged else [5, 2, 5, 1])
        draws = np.random.RandomState(seed)                                # the first attempt succeeds: its draws are the size, then the flip
        draws.choice(SIZES)
        flips.add(bool(is_train and draws.uniform() < 0.5))
    assert flips == ({False, True} if is_train else {False})               # one case is flipped and one is not
    assert record["file_name"] == before["file_name"] and "class_code" not in record                     # the input is not modified
    assert np.array_equal(record["image"], before["image"]) and record["annotations"] == before["annotations"]


def test_part_of_two_polygons_is_their_or():
    record = _record(_scene())
    p = {"in_h": H, "in_w": W, "resize": (32, 45), "flip": False, "crop": (0, 0, 45, 32)}
    out = _mapper(False, False, np.random.RandomState(0))(record)
    both = [P.mask(P.transform_polygon(q, p).reshape(-1), 32, 45) for q in record["annotations"][2]["segmentation"]]
    got = out["part_instances"].gt_masks.tensor[2].cpu().numpy()
    assert both[0].any() and both[1].any() and not (both[0] & both[1]).any() and np.array_equal(got, both[0] | both[1])
    assert out["part_instances"].gt_boxes[2].tolist() == [np.float32(5.0 * (45 / 56)), np.float32(1.0 * 0.8), np.float32(54.9 * (45 * 1.0 / 56)),
                                                          np.float32(37.0 * 0.8)]


def test_part_with_an_empty_box_is_dropped():
    """collinear, axis-aligned vertices: a box of zero width (or height) fails filter_empty_instances; the part leaves part_instances and
    the object mask is the OR of the others"""
    scene = _scene()
    scene.insert(1, (9, [[30.0, 5.0, 30.0, 12.0, 30.0, 33.0]]))            # zero width
    scene.append((8, [[4.0, 20.5, 50.0, 20.5, 33.0, 20.5, 12.0, 20.5]]))   # zero height
    record = _record(scene)
    for merged in (True, False):
        for is_train in (False, True):
            mine, theirs = np.random.RandomState(1), np.random.RandomState(1)
            want, _, fallback = P.call(record, record["image"], theirs, is_train, SIZES, MAX_SIZE, "choice", merged, CLASS_MAP)
            out = _mapper(is_train, merged, mine)(record)
            _assert_output(out, want, record, merged)
            assert not fallback and _same_state(mine, theirs)
            classes = out["part_instances"].gt_classes.tolist()
            assert 9 not in classes and 8 not in classes and len(classes) == (3 if merged else 4)
            assert np.array_equal(out["instances"].gt_masks.tensor[0].cpu().numpy(), want["part_masks"].any(axis=0))
    clean = _mapper(False, True, np.random.RandomState(1))(_record(_scene()))
    with_dropped = _mapper(False, True, np.random.RandomState(1))(record)
    assert torch.equal(clean["instances"].gt_masks.tensor, with_dropped["instances"].gt_masks.tensor)    # nothing of the dropped parts


@pytest.mark.parametrize("merged", [True, False])
def test_all_parts_degenerate_takes_the_identity_pass(merged):
    """train mode, every part filtered out in every attempt: 20 attempts draw (size, flip) each, then the pass with the EMPTY augmentation
    list: no draw, no resize, the output at the input size with the image as decoded.  (Here the reference's merged branch would crash in
    torch.stack([]); the mapper returns zero part planes and an empty object mask.)"""
    record = _record([(9, [[30.0, 5.0, 30.0, 12.0, 30.0, 33.0]]), (8, [[4.0, 20.5, 50.0, 20.5, 33.0, 20.5]])])
    mine, theirs, count = np.random.RandomState(4), np.random.RandomState(4), np.random.RandomState(4)
    want, attempts, fallback = P.call(record, record["image"], theirs, True, SIZES, MAX_SIZE, "choice", merged, CLASS_MAP)
    out = _mapper(True, merged, mine)(record)
    assert fallback and attempts == 20 and want["size"] == (H, W)
    _assert_output(out, want, record, merged)
    assert np.array_equal(out["image"].cpu().numpy(), record["image"].transpose(2, 0, 1))
    assert tuple(out["part_instances"].gt_masks.tensor.shape) == (0, H, W) and len(out["part_instances"]) == 0
    assert out["part_instances"].gt_classes.shape == (0,) and not out["instances"].gt_masks.tensor.any()
    if not merged:
        assert tuple(out["part_instances"].gt_boxes.shape) == (0, 4)
    for _ in range(20):
        count.choice(SIZES)
        count.uniform()
    assert _same_state(mine, theirs) and _same_state(mine, count)
    # test mode makes its one pass and returns the same empty result at the resized size
    out = _mapper(False, merged, np.random.RandomState(4))(record)
    assert tuple(out["part_instances"].gt_masks.tensor.shape) == (0, 32, 45) and (out["height"], out["width"]) == (32, 45)


def test_record_without_annotations_and_class_lookup():
    record = _record([])
    assert _mapper(False, True, np.random.RandomState(0))(record) is None
    with pytest.raises(ValueError, match="n0123/n0123_77.JPEG"):
        _mapper(True, True, np.random.RandomState(0))(record)
    for code, cls in CLASS_MAP.items():
        out = _mapper(False, True, np.random.RandomState(0))(_record(_scene(), code=code))
        assert out["instances"].gt_classes.tolist() == [cls] and out["class_code"] == code
        assert out["file_name"] == f"data/val/{code}/{code}_77.JPEG"
    with pytest.raises(KeyError):
        _mapper(False, True, np.random.RandomState(0))(_record(_scene(), code="n0999"))


def test_test_mode_output_feeds_the_models_target_preparation():
    """a batch of two test-mode outputs of different sizes goes through SupervisedModel.prepare_targets and inference.prepare_gt_targets
    as it is"""
    from partdistillation_amd import inference
    from partdistillation_amd.supervised_model import SupervisedModel
    batch, wants = [], []
    for (h, w), size, seed in (((H, W), 32, 1), ((52, 36), 24, 2)):
        scene = _scene() if (h, w) == (H, W) else [(4, [[2.0, 3.0, 30.5, 6.0, 20.0, 45.5]]), (6, [[10.0, 30.0, 33.0, 28.0, 25.0, 50.0]])]
        record = _record(scene, seed=seed, h=h, w=w)
        wants.append(P.call(record, record["image"], np.random.RandomState(0), False, (size,), MAX_SIZE, "choice", True, CLASS_MAP)[0])
        batch.append(_mapper(False, True, np.random.RandomState(0), sizes=(size,))(record))
    assert wants[0]["size"] != wants[1]["size"]
    model = types.SimpleNamespace(device=torch.device(DEV), class_agnostic_learning=False)
    images = types.SimpleNamespace(tensor=torch.zeros((2, 3, 48, 48), device=DEV))
    for targets in (SupervisedModel.prepare_targets(model, batch, images), inference.prepare_gt_targets(model, batch, images)):
        for t, want in zip(targets, wants):
            h, w = want["size"]
            assert tuple(t["masks"].shape) == (len(want["part_classes"]), 48, 48) and t["masks"].dtype == torch.bool
            assert np.array_equal(t["masks"][:, :h, :w].cpu().numpy(), want["part_masks"]) and int(t["masks"].sum()) == want["part_masks"].sum()
            assert np.array_equal(t["object_masks"][:, :h, :w].cpu().numpy(), want["obj_masks"])
            assert t["labels"].tolist() == want["part_classes"] and t["labels"].is_cuda
