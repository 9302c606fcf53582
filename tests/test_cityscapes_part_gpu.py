"""Cityscapes-Part ground truth on the device: pd_pp_decode_uids and pd_rle_masked_label_runs alone against numpy, then the record
builder and DeviceCityscapesPartMapper's (record, part_file) input against the reference's functions restated in
cityscapes_part_oracle.py.  Integers, bytes and dicts: every comparison is exact equality."""
import copy

import numpy as np
import pytest
import torch
from PIL import Image

import cityscapes_part_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
LABELS = np.asarray([0, 1, 2, 5, 99], dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ decode_uids
def _uid_map(rng):
    u = np.concatenate(([row[0] for row in O.HAND_TABLE], rng.randint(0, 100, 20), rng.randint(100, 100000, 30),
                        rng.randint(100000, 10000000, 3 * 37 - 62)))
    return u.astype(np.int32).reshape(3, 37)


def test_decode_uids_all_outputs_and_each_alone():
    from partdistillation_amd.functions.panoptic_parts import OUTPUTS, decode_uids
    uids = _uid_map(np.random.RandomState(0))
    sids, iids, pids = O.decode_uids(uids)
    want = {"sids": sids, "iids": iids, "pids": pids, "part_label": O.part_label(uids)}
    d = torch.from_numpy(uids).to(DEV)
    got = decode_uids(d).check()
    assert tuple(got) == OUTPUTS
    for k in OUTPUTS:
        assert got[k].is_cuda and got[k].cpu().numpy().dtype == want[k].dtype and np.array_equal(got[k].cpu().numpy(), want[k]), k
        alone = decode_uids(d, want=(k,)).check()
        assert list(alone) == [k] and np.array_equal(alone[k].cpu().numpy(), want[k]), k
    # a view that is not 16-byte aligned takes the one-uid-per-thread kernel; one pixel; nothing
    flat = torch.from_numpy(np.concatenate(([0], uids.ravel())).astype(np.int32)).to(DEV)
    off = decode_uids(flat[1:].view(3, 37)).check()
    for k in OUTPUTS:
        assert np.array_equal(off[k].cpu().numpy(), want[k]), k
    assert decode_uids(d[:1, :1]).check()["pids"].tolist() == [[-1]]
    assert decode_uids(d[:0]).check()["sids"].shape == (0, 37)


def test_decode_uids_invalid_uids_and_bad_arguments():
    from partdistillation_amd.functions.panoptic_parts import decode_uids
    uids = _uid_map(np.random.RandomState(1))
    for bad, at in ((-1, (2, 36)), (10000000, (0, 0)), (-2 ** 31, (1, 17)), (2 ** 31 - 1, (2, 35))):
        broken = uids.copy()
        broken[at] = bad
        with pytest.raises(ValueError, match="outside"):
            decode_uids(torch.from_numpy(broken).to(DEV)).check()
        decode_uids(torch.from_numpy(uids).to(DEV)).check()                   # the flag starts clear
    d = torch.from_numpy(uids).to(DEV)
    for wrong in (d.long(), d.float(), d[0], d[None]):
        with pytest.raises(ValueError, match="int32"):
            decode_uids(wrong)
    with pytest.raises(ValueError, match="want"):
        decode_uids(d, want=("sids", "uids"))
    with pytest.raises(RuntimeError, match="GPU only"):
        decode_uids(torch.from_numpy(uids))


# ------------------------------------------------------------------------------------------------ plane_label_runs
def _assert_runs(planes, labels, d_planes=None):
    from partdistillation_amd.functions.rle import plane_label_runs
    d_planes = torch.from_numpy(planes).to(DEV) if d_planes is None else d_planes
    got = plane_label_runs(d_planes, torch.from_numpy(labels).to(DEV))
    want = O.plane_label_runs(planes, labels)
    for g, w, what in zip(got, want, ("offsets", "starts", "values", "nonzero")):
        assert g.dtype == w.dtype and np.array_equal(g, w), what
    return got


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 70), (9, 1), (8, 64), (13, 67), (17, 130)])
def test_plane_label_runs_against_numpy(H, W, n):
    rng = np.random.RandomState(H * 131 + W + n)
    labels = LABELS[rng.randint(0, 5, (H, W))]
    planes = (rng.rand(n, H, W) < 0.6).astype(np.uint8) * rng.randint(1, 256, (n, H, W)).astype(np.uint8)   # any non-zero byte selects
    _assert_runs(planes, labels)
    _assert_runs(planes.astype(bool), labels)


def test_plane_label_runs_particular_planes():
    H, W = 13, 67
    rng = np.random.RandomState(5)
    labels = LABELS[rng.randint(0, 5, (H, W))]
    zero, ones = np.zeros((1, H, W), dtype=np.uint8), np.ones((1, H, W), dtype=np.uint8)
    got = _assert_runs(zero, labels)
    assert got[0].tolist() == [0, 1] and got[2].tolist() == [0] and got[3].tolist() == [0]
    got = _assert_runs(ones, np.full((H, W), 5, dtype=np.uint8))               # one run across every column end
    assert got[1].tolist() == [0] and got[2].tolist() == [5] and got[3].tolist() == [H * W]
    flat = np.full(H * W, 5, dtype=np.uint8)
    flat[:3 * H], flat[3 * H:5 * H + 4] = 1, 2                                 # one change exactly at a column end, one inside a column
    got = _assert_runs(ones, np.ascontiguousarray(flat.reshape(W, H).T))
    assert got[1].tolist() == [0, 3 * H, 5 * H + 4] and got[2].tolist() == [1, 2, 5]
    # planes that are a strided view: every second plane of a larger tensor, plane stride 2 H W
    big = (rng.rand(6, H, W) < 0.5).astype(np.uint8)
    d_big = torch.from_numpy(big).to(DEV)
    view = d_big[::2]
    assert view.stride(0) == 2 * H * W and not view.is_contiguous()
    _assert_runs(big[::2], labels, view)


def test_plane_label_runs_grow_path():
    """a 300 x 300 plane of ones over a checkerboard of labels 1 / 2: a run per pixel but for the 299 column ends the colour carries
    across, more than the 65 536 runs the buffers start with (the buffers of earlier tests are dropped first)"""
    from partdistillation_amd.functions import rle as drle
    ys, xs = np.mgrid[0:300, 0:300]
    labels = (1 + (ys + xs) % 2).astype(np.uint8)
    drle._buffers.clear()
    assert drle._MIN_CAPACITY == 65536
    got = drle.plane_label_runs(torch.ones((1, 300, 300), dtype=torch.uint8, device=DEV), torch.from_numpy(labels).to(DEV))
    flat = labels.T.ravel()
    starts = np.concatenate(([0], np.flatnonzero(flat[1:] != flat[:-1]) + 1))
    assert len(starts) == 90000 - 299 and got[0].tolist() == [0, len(starts)]
    assert np.array_equal(got[1], starts) and np.array_equal(got[2], flat[starts]) and got[3].tolist() == [90000]
    assert got[1].dtype == np.int32 and got[2].dtype == np.uint8 and next(iter(drle._buffers.values())).capacity >= len(starts)


def test_plane_label_runs_checks_its_arguments():
    from partdistillation_amd.functions.rle import plane_label_runs
    planes, labels = torch.ones((2, 4, 5), dtype=torch.uint8, device=DEV), torch.ones((4, 5), dtype=torch.uint8, device=DEV)
    for bad in (labels.int(), labels[:3], labels[None]):
        with pytest.raises(ValueError, match="labels uint8"):
            plane_label_runs(planes, bad)
    with pytest.raises(RuntimeError, match="GPU only"):
        plane_label_runs(planes, labels.cpu())
    got = plane_label_runs(planes[:0], labels)
    assert got[0].tolist() == [0] and got[1].size == 0 and got[3].size == 0


# ------------------------------------------------------------------------------------------------ encode_plane_labels
@pytest.mark.parametrize("H,W", [(13, 67), (17, 130)])
def test_encode_plane_labels(H, W):
    from partdistillation_amd.functions.rle import encode_plane_labels
    from partdistillation_amd.utils import rle
    rng = np.random.RandomState(H)
    labels = LABELS[rng.randint(0, 5, (H, W))]
    planes = rng.rand(4, H, W) < 0.5
    planes[1] = False                                                          # no label under it
    planes[2] &= labels == 99                                                  # one label
    got, counts = encode_plane_labels(torch.from_numpy(planes).to(DEV), torch.from_numpy(labels).to(DEV))
    assert counts.shape == (4, 256) and counts.dtype == np.int64 and len(got) == 4
    for i in range(4):
        v = np.where(planes[i], labels, 0)
        present = [int(l) for l in np.unique(v) if l > 0]
        assert got[i] == list(zip(present, rle.labels_to_coco_json(v, present))), i
        assert np.array_equal(counts[i], np.bincount(v.ravel(), minlength=256)), i
    assert got[1] == [] and [l for l, _ in got[2]] == [99] and [l for l, _ in got[0]] == [1, 2, 5, 99]


# ------------------------------------------------------------------------------------------------ the record builder
@pytest.mark.parametrize("polygons", [False, True])
@pytest.mark.parametrize("H,W", [(37, 53), (64, 128)])
def test_load_object_and_parts(H, W, polygons):
    from partdistillation_amd.data.cityscapes_part_record import cityscapes_part_records, load_object_and_parts
    record, uids = O.scene(np.random.RandomState(H), H, W, polygons)
    before = copy.deepcopy(record)
    want = O.load_object_and_parts(record, uids)
    assert len(want[0]) == 4 and want[1][1] == [] and min(len(want[1][i]) for i in (0, 2, 3)) >= 2     # class 6 dropped; the person has no part
    bus, rider = (O.object_mask(record["annotations"][i]["segmentation"], H, W) for i in (3, 4))
    assert (bus & rider).any() and {int(u) for u in np.unique(uids)} & set(range(100)) and ((uids >= 100) & (uids < 100000)).any()
    for part in (uids, torch.from_numpy(uids), torch.from_numpy(uids).to(DEV)):
        got = load_object_and_parts(record, part, DEV)
        assert got[0] == want[0] and got[1] == want[1]
    assert load_object_and_parts(dict(record, annotations=[]), uids, DEV) == (None, None)
    for for_segmentation in (True, False):
        mine, theirs = list(cityscapes_part_records(record, uids, for_segmentation, DEV)), O.records(record, uids, for_segmentation)
        assert len(mine) == len(theirs) == (3 if for_segmentation else 1)
        for a, b in zip(mine, theirs):
            assert {k: v for k, v in a.items() if k != "image"} == {k: v for k, v in b.items() if k != "image"}
    assert record["annotations"] == before["annotations"] and sorted(record) == sorted(before)
    broken = uids.copy()
    broken[H - 1, W - 1] = -7
    with pytest.raises(ValueError, match="outside"):
        load_object_and_parts(record, broken, DEV)


def test_load_object_and_parts_mixed_segmentations():
    """RLE and polygon objects in one record: each goes through its own decoder"""
    from partdistillation_amd.data.cityscapes_part_record import load_object_and_parts
    H, W = 37, 53
    as_rle, uids = O.scene(np.random.RandomState(9), H, W, False)
    as_poly, _ = O.scene(np.random.RandomState(9), H, W, True)
    mixed = dict(as_rle, annotations=[(as_poly if i % 2 else as_rle)["annotations"][i] for i in range(5)])
    assert load_object_and_parts(mixed, uids, DEV) == O.load_object_and_parts(as_rle, uids)


# ------------------------------------------------------------------------------------------------ the mapper
def _mapper(cls, is_train, merged, rng):
    crop = ("relative_range", (0.6, 0.6)) if is_train else (None, None)
    return cls(is_train, (48, 64), 200, "choice", crop[0], crop[1], use_merged_gt=merged, device=DEV, rng=rng)


def _assert_same_output(a, b, merged):
    assert sorted(a) == sorted(b) and "annotations" not in a and "part_annotations" not in a
    assert torch.equal(a["image"], b["image"]) and a["orig_part_maps"] == b["orig_part_maps"] and len(a["orig_part_maps"]) > 0
    for key in ("instances", "part_instances"):
        x, y = a[key], b[key]
        assert x.image_size == y.image_size and torch.equal(x.gt_masks.tensor, y.gt_masks.tensor) and torch.equal(x.gt_classes, y.gt_classes)
    assert torch.equal(a["instances"].gt_boxes, b["instances"].gt_boxes) and torch.equal(a["instances"].obj_mapping, b["instances"].obj_mapping)
    if not merged:
        for key in ("obj_mapping", "part_mapping"):
            assert torch.equal(getattr(a["part_instances"], key), getattr(b["part_instances"], key))
    assert len(a["part_instances"]) > 0


@pytest.mark.parametrize("merged", [True, False])
@pytest.mark.parametrize("is_train", [True, False])
def test_mapper_takes_the_record_and_part_file(tmp_path, is_train, merged):
    from partdistillation_amd.data import DeviceCityscapesPartMapper
    H, W = 64, 128
    record, uids = O.scene(np.random.RandomState(7), H, W, polygons=is_train)
    path = str(tmp_path / "aachen_000000_000019_gtFinePanopticParts.tif")
    Image.fromarray(uids).save(path)
    objects, parts = O.load_object_and_parts(record, uids)
    built = dict(record, annotations=objects, part_annotations=parts)
    before = copy.deepcopy(record)
    for seed in range(2):
        mine, theirs = np.random.RandomState(seed), np.random.RandomState(seed)
        out = _mapper(DeviceCityscapesPartMapper, is_train, merged, mine)((record, path))
        want = _mapper(DeviceCityscapesPartMapper, is_train, merged, theirs)(built)
        _assert_same_output(out, want, merged)
        assert mine.get_state()[2] == theirs.get_state()[2] and np.array_equal(mine.get_state()[1], theirs.get_state()[1])
    assert record["annotations"] == before["annotations"] and "part_annotations" not in record


def test_mapper_tuple_without_annotations_and_the_pascal_mapper():
    from partdistillation_amd.data import DeviceCityscapesPartMapper, DeviceVOCPartsMapper
    record, uids = O.scene(np.random.RandomState(8), 37, 53, False)
    empty = dict(record, annotations=[])
    assert _mapper(DeviceCityscapesPartMapper, False, True, np.random.RandomState(0))((empty, uids)) is None
    with pytest.raises(NotImplementedError, match="DeviceCityscapesPartMapper only"):
        _mapper(DeviceVOCPartsMapper, False, True, np.random.RandomState(0))((record, uids))
