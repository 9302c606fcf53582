"""Ground-truth part mappers on the device: pd_rle_sample_groups_u8 (include/pd_input.h) alone against a numpy loop, then
DeviceVOCPartsMapper / DeviceCityscapesPartMapper end to end against the reference's mappers restated on the Pillow-exact oracle pieces
(tests/gt_part_oracle.py).  Everything is integer arithmetic: every comparison is exact equality."""
import types

import numpy as np
import pytest
import torch

import gt_part_oracle as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------------------------------------ the kernel alone
def _sample(masks, sx, sy, groups, garbage=7):
    """masks bool [n, H, W] (or (H, W) with n = 0) -> the kernel's three outputs as numpy; the outputs are pre-filled with garbage"""
    from partdistillation_amd.functions.input_pipeline import rle_sample_groups
    from partdistillation_amd.utils import rle
    if isinstance(masks, tuple):
        (H, W), segs = masks, []
    else:
        (H, W), segs = masks.shape[1:], [rle.encode(m) for m in masks]
    starts, offsets = rle.segmentations_to_starts(segs, (H, W))
    n, ng = len(segs), len(groups)
    d = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV) for a in (starts, offsets, sx, sy)]
    out = torch.full((ng, len(sy), len(sx)), garbage, dtype=torch.uint8, device=DEV)
    m_area = torch.full((n,), garbage, dtype=torch.int32, device=DEV)
    g_area = torch.full((ng,), garbage, dtype=torch.int32, device=DEV)
    g_off = np.concatenate(([0], np.cumsum([len(g) for g in groups]))).astype(np.int32)
    g_mem = np.asarray([m for g in groups for m in g], dtype=np.int32)
    rle_sample_groups(d[0], d[1], H, W, d[2], d[3], g_off, g_mem, out, m_area, g_area)
    return out.cpu().numpy(), m_area.cpu().numpy(), g_area.cpu().numpy()


def _sample_ref(masks, sx, sy, groups):
    n = 0 if isinstance(masks, tuple) else len(masks)
    sampled = np.zeros((n, len(sy), len(sx)), dtype=np.uint8)
    for m in range(n):
        for y in range(len(sy)):
            sampled[m, y] = masks[m][sy[y], sx]
    planes = np.zeros((len(groups), len(sy), len(sx)), dtype=np.uint8)
    for g, members in enumerate(groups):
        for m in members:
            planes[g] |= sampled[m]
    return planes, sampled.sum(axis=(1, 2)).astype(np.int32), planes.sum(axis=(1, 2)).astype(np.int32)


def _check(masks, sx, sy, groups):
    got, want = _sample(masks, sx, sy, groups), _sample_ref(masks, sx, sy, groups)
    for g, w, what in zip(got, want, ("planes", "member_area", "group_area")):
        assert g.dtype == w.dtype and np.array_equal(g, w), what
    return got


def _special_masks(rng, H, W):
    """random blobs, then: starts with ones (COCO's leading zero count), empty, full"""
    m = np.zeros((6, H, W), dtype=bool)
    m[:3] = rng.rand(3, H, W) < 0.35
    m[3] = rng.rand(H, W) < 0.5
    m[3, 0, 0] = True
    m[5] = True
    return m


def test_sample_groups_one_pixel():
    for value in (False, True):
        got = _check(np.full((1, 1, 1), value), [0], [0], [[0]])
        assert got[0].tolist() == [[[int(value)]]] and got[1].tolist() == [int(value)] == got[2].tolist()


@pytest.mark.parametrize("out_h", [1, 3])
@pytest.mark.parametrize("out_w", [5, 63, 64, 65, 257])
def test_sample_groups_odd_pitches_and_wave_edges(out_w, out_h):
    rng = np.random.RandomState(out_w * 4 + out_h)
    masks = _special_masks(rng, 11, 13)
    # an empty group, member 2 in no group, member 0 in two groups, overlapping members 0 and 1 in one group
    groups = [[0, 1], [], [0], [3], [4], [5, 1]]
    got = _check(masks, rng.randint(0, 13, out_w), rng.randint(0, 11, out_h), groups)
    assert not got[0][1].any() and got[2][1] == 0 and got[2][4] == 0 and got[1][4] == 0     # empty group, empty mask
    assert got[0][5].all() and got[2][5] == out_w * out_h == got[1][5]                       # full mask
    assert got[0].max() == 1 and got[2][0] <= got[1][0] + got[1][1]                          # values 0 / 1; the union is counted once


@pytest.mark.parametrize("kind", ["descending", "repeats_7_to_20", "gaps_40_to_9"])
def test_sample_groups_index_tables(kind):
    from partdistillation_amd.functions.input_pipeline import nearest_index
    rng = np.random.RandomState(len(kind))
    W = {"descending": 23, "repeats_7_to_20": 7, "gaps_40_to_9": 40}[kind]
    H = 17
    masks = _special_masks(rng, H, W)
    sx = {"descending": np.arange(W)[::-1], "repeats_7_to_20": nearest_index(7, 20), "gaps_40_to_9": nearest_index(40, 9)}[kind]
    if kind == "repeats_7_to_20":
        assert len(set(sx.tolist())) == 7 and len(sx) == 20
    if kind == "gaps_40_to_9":
        assert (np.diff(sx) > 1).all()
    sy = nearest_index(H, 29)[::-1] if kind == "descending" else nearest_index(H, 12)
    _check(masks, sx, sy, [[0], [1, 2], [3, 4, 5], [2]])


def test_sample_groups_without_groups_and_without_members():
    rng = np.random.RandomState(3)
    masks = _special_masks(rng, 9, 10)[:3]
    got = _check(masks, np.arange(10), np.arange(9), [])                   # n_groups = 0, n = 3: member_area is still filled
    assert got[0].shape == (0, 9, 10) and got[1].tolist() == masks.reshape(3, -1).sum(1).tolist()
    got = _check((9, 10), np.arange(10), np.arange(9), [[], []])           # n = 0: zero planes
    assert not got[0].any() and got[2].tolist() == [0, 0]
    _sample((9, 10), np.arange(10), np.arange(9), [])                      # nothing at all: PD_OK without a launch
    torch.cuda.synchronize()


def _striped_masks(rng, n, H, W, runs):
    """n masks of about `runs` runs each in the column-major order"""
    out = np.zeros((n, H * W), dtype=bool)
    for i in range(n):
        cuts = np.sort(rng.choice(np.arange(1, H * W), runs - 1, replace=False))
        vals = (np.arange(runs) + i) % 2 == 1
        out[i] = np.repeat(vals, np.diff(np.concatenate(([0], cuts, [H * W]))))
    return np.ascontiguousarray(out.reshape(n, W, H).transpose(0, 2, 1))


def test_sample_groups_many_members_in_one_group():
    """70 members of ~40 runs in one group on a 33 x 70 source: more members than a wave has lanes, more runs than one pass of a small
    tile; every member also counted on its own"""
    rng = np.random.RandomState(70)
    masks = _striped_masks(rng, 70, 33, 70, 40)
    masks &= rng.rand(70, 33, 70) < 0.02                                   # sparse, so that the union is not simply everything
    got = _check(masks, np.arange(70), np.arange(33), [list(range(70)), [69, 0]])
    assert 0 < got[2][0] < 33 * 70 and (got[1] > 0).sum() > 60


def test_sample_groups_long_run_table_and_many_tiles():
    """a member with more runs than the kernel stages on chip (searched in place), next to short ones, on an output of several tiles per
    plane; then more tiles than the launch has blocks, so that blocks take a second tile"""
    rng = np.random.RandomState(9)
    masks = _striped_masks(rng, 3, 70, 70, 40)
    masks[1] = (np.add.outer(np.arange(70), np.arange(70)) % 2).astype(bool)              # 4900 runs
    from partdistillation_amd.utils import rle
    assert len(rle.mask_to_counts(masks[1])) > 2048
    _check(masks, rng.randint(0, 70, 131), rng.randint(0, 70, 67), [[0, 1], [1], [2, 0], [1, 2]])
    many = _striped_masks(rng, 70, 33, 70, 40)
    got = _check(many, rng.randint(0, 70, 400), rng.randint(0, 33, 300), [[5, 6]])        # 71 units x 59 tiles > 4096 blocks
    assert got[0].shape == (1, 300, 400)


# ------------------------------------------------------------------------------------------------ the mappers end to end
def _mapper(flavour, is_train, merged, rng, sizes=(48, 64, 96), max_size=140, style="choice", crop=("relative_range", (0.6, 0.6))):
    from partdistillation_amd.data import DeviceCityscapesPartMapper, DeviceVOCPartsMapper
    cls = DeviceVOCPartsMapper if flavour == "voc" else DeviceCityscapesPartMapper
    ctype, csize = crop if crop is not None else (None, None)
    return cls(is_train, sizes, max_size, style, ctype, csize, use_merged_gt=merged, device=DEV, rng=rng)


def _assert_output(out, want, record, merged):
    assert "annotations" not in out and "part_annotations" not in out
    for key in ("file_name", "image_id", "height", "width"):
        assert out[key] == record[key]                                     # height / width stay the record's
    inst, parts, size = out["instances"], out["part_instances"], want["size"]
    assert out["image"].dtype == torch.uint8 and out["image"].is_cuda and np.array_equal(out["image"].cpu().numpy(), want["image"])
    assert inst.image_size == size == parts.image_size == tuple(out["image"].shape[1:])
    for t in (inst.gt_masks.tensor, inst.gt_classes, inst.gt_boxes, inst.obj_mapping, parts.gt_masks.tensor, parts.gt_classes):
        assert t.is_cuda
    assert inst.gt_masks.tensor.dtype == torch.bool and parts.gt_masks.tensor.dtype == torch.bool
    assert inst.gt_classes.dtype == torch.int64 and parts.gt_classes.dtype == torch.int64 and inst.obj_mapping.dtype == torch.int64
    assert np.array_equal(inst.gt_masks.tensor.cpu().numpy(), want["obj_masks"])
    assert inst.gt_classes.tolist() == want["obj_classes"] and inst.obj_mapping.tolist() == want["obj_mapping"]
    assert inst.gt_boxes.dtype == torch.float32 and np.array_equal(inst.gt_boxes.cpu().numpy(), want["obj_boxes"].astype(np.float32))
    assert tuple(parts.gt_masks.tensor.shape) == want["part_masks"].shape
    assert np.array_equal(parts.gt_masks.tensor.cpu().numpy(), want["part_masks"]) and parts.gt_classes.tolist() == want["part_classes"]
    if merged:
        assert not parts.has("obj_mapping") and not parts.has("part_mapping")
    else:
        assert parts.obj_mapping.tolist() == want["part_obj_mapping"] and parts.part_mapping.tolist() == want["part_mapping"]
        assert parts.obj_mapping.dtype == torch.int64 and parts.part_mapping.dtype == torch.int64
    assert out["orig_part_maps"] == want["orig_part_maps"]
    assert all(a is b for a, b in zip(out["orig_part_maps"], want["orig_part_maps"]))        # the untouched RLE dicts of the record


def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[2] == sb[2] and np.array_equal(sa[1], sb[1])


@pytest.mark.parametrize("merged", [True, False])
@pytest.mark.parametrize("is_train", [True, False])
@pytest.mark.parametrize("flavour", ["voc", "city"])
def test_mappers_against_the_oracle(flavour, is_train, merged):
    rng = np.random.RandomState(11 + is_train)
    H, W = 90, 120
    image = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    record = G.record(*G.scene(rng, H, W), flavour, image=image)
    record["annotations"][1]["iscrowd"] = 1                                # skipped with its parts; the mapping keeps the record's indices
    sizes, max_size = (48, 64, 96), 140
    test_sizes = sizes if flavour == "voc" or is_train else (96, 96)       # Cityscapes reads MIN_SIZE_TEST in test mode
    seen_flip = 0
    for seed in range(3):
        mine, theirs = np.random.RandomState(seed), np.random.RandomState(seed)
        mapper = _mapper(flavour, is_train, merged, mine, test_sizes, max_size)
        want, attempts, fallback = G.call(record, image, flavour, theirs, is_train, test_sizes, max_size, "choice",
                                          ("relative_range", (0.6, 0.6)), merged)
        out = mapper(record)
        _assert_output(out, want, record, merged)
        assert _same_state(mine, theirs) and not fallback
        assert len(want["part_classes"]) >= 2 and want["obj_mapping"] in ([0, 2], [0], [2])
        assert "image" in record and len(record["annotations"]) == 3       # the input is not modified
    if merged:
        assert len(want["part_classes"]) < len(want["part_mapping"])       # merging had work to do


def _fixed(mapper, p):
    mapper.draw = lambda h, w, crop=True: dict(p)
    return mapper


def test_one_pixel_wide_part_pascal_drops_it_cityscapes_keeps_it():
    rng = np.random.RandomState(4)
    H, W = 60, 80
    image = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    obj = np.zeros((H, W), dtype=bool)
    obj[10:50, 10:70] = True
    line, left, right = np.zeros_like(obj), obj.copy(), obj.copy()
    line[10:50, 40] = True                                                 # one pixel wide: a tight box of zero width
    left[:, 40:] = False
    right[:, :41] = False
    p = {"in_h": H, "in_w": W, "resize": (60, 80), "flip": False, "crop": (0, 0, 80, 60)}
    for flavour, kept in (("voc", [0, 2]), ("city", [0, 1, 2])):
        record = G.record([obj], [3], [[left, line, right]], [[1, 5, 2]], flavour, image=image)
        for merged in (False, True):
            out = _fixed(_mapper(flavour, False, merged, None), p)(record)
            _assert_output(out, G.forward(record, image, flavour, p, merged), record, merged)
            assert out["orig_part_maps"] == [record["part_annotations"][0][k]["segmentation"] for k in kept]
            assert sorted(out["part_instances"].gt_classes.tolist()) == sorted([1, 5, 2][k] for k in kept)
            if not merged:
                assert out["part_instances"].part_mapping.tolist() == kept


def test_object_cropped_away_takes_its_parts_and_renumbers():
    rng = np.random.RandomState(6)
    H, W = 90, 120
    image = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    scene = G.scene(rng, H, W)
    n0 = len(scene[2][0])
    for flavour in ("voc", "city"):
        record = G.record(*scene, flavour, image=image)
        for flip in (False, True):
            # 72 x 96 after the resize; the window is the right 60 columns (flipped: the mirror image's, i.e. the source's LEFT ones)
            p = {"in_h": H, "in_w": W, "resize": (72, 96), "flip": flip, "crop": (36, 0, 60, 72)}
            gone = 2 if flip else 0
            for merged in (False, True):
                out = _fixed(_mapper(flavour, True, merged, None), p)(record)
                want = G.forward(record, image, flavour, p, merged)
                _assert_output(out, want, record, merged)
                assert out["instances"].obj_mapping.tolist() == [i for i in range(3) if i != gone]
                if not merged:
                    om, pm = out["part_instances"].obj_mapping.tolist(), out["part_instances"].part_mapping.tolist()
                    assert set(om) == {0, 1} and max(pm) < sum(len(scene[2][i]) for i in range(3) if i != gone)
                    flat = [part for i in range(3) if i != gone for part in record["part_annotations"][i]]   # the survivors' parts
                    assert all(seg is flat[k]["segmentation"] for seg, k in zip(out["orig_part_maps"], pm)) and n0 > 0


def _corner_scene(H, W):
    """one small object in the top-left corner with two parts"""
    obj = np.zeros((H, W), dtype=bool)
    obj[2:10, 2:12] = True
    a, b = obj.copy(), obj.copy()
    a[:, 7:] = False
    b[:, :7] = False
    return [obj], [1], [[a, b]], [[0, 1]]


@pytest.mark.parametrize("flavour", ["voc", "city"])
def test_retry_and_fallback_without_the_crop(flavour):
    """an absolute 8 x 8 crop of the bottom-right region can never hold the corner object: every cropped attempt fails, the attempt loop
    (num_repeats lowered to 2 on the instance) ends in the pass without the crop, which draws the size and the flip but no crop"""
    H, W = 60, 80
    rng = np.random.RandomState(8)
    image = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    record = G.record(*_corner_scene(H, W), flavour, image=image)
    crop = ("absolute", (8, 8))
    found = 0
    for seed in range(6):
        mine, theirs = np.random.RandomState(seed), np.random.RandomState(seed)
        want, attempts, fallback = G.call(record, image, flavour, theirs, True, (48,), 140, "choice", crop, True, num_repeats=2)
        mapper = _mapper(flavour, True, True, mine, (48,), 140, crop=crop)
        mapper.num_repeats = 2
        out = mapper(record)
        _assert_output(out, want, record, True)
        assert _same_state(mine, theirs)
        if fallback:
            found += 1
            assert attempts == 2 and want["size"] == (48, 64) and len(want["part_classes"]) == 2
    assert found >= 3                                                      # most seeds miss the corner twice in a row


def test_pascal_needs_more_than_one_part_cityscapes_one():
    """exactly one surviving part and no crop: Pascal's `> 1` fails every attempt and takes the extra pass (three draws of size and flip
    with num_repeats = 2), Cityscapes' `> 0` returns after the first"""
    H, W = 60, 80
    rng = np.random.RandomState(2)
    image = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    objs, ocls, parts, pcls = _corner_scene(H, W)
    for flavour, draws in (("voc", 3), ("city", 1)):
        record = G.record(objs, ocls, [parts[0][:1]], [pcls[0][:1]], flavour, image=image)
        mine, theirs, count = np.random.RandomState(1), np.random.RandomState(1), np.random.RandomState(1)
        want, attempts, fallback = G.call(record, image, flavour, theirs, True, (48, 64), 140, "choice", None, True, num_repeats=2)
        mapper = _mapper(flavour, True, True, mine, (48, 64), 140, crop=None)
        mapper.num_repeats = 2
        out = mapper(record)
        _assert_output(out, want, record, True)
        assert len(out["part_instances"]) == 1 and fallback == (flavour == "voc")
        for _ in range(draws):
            count.choice((48, 64))
            count.uniform()
        assert _same_state(mine, theirs) and _same_state(mine, count)


@pytest.mark.parametrize("flavour", ["voc", "city"])
def test_zero_part_result_shape(flavour):
    H, W = 60, 80
    image = np.random.RandomState(0).randint(0, 256, (H, W, 3)).astype(np.uint8)
    objs, ocls, _, _ = _corner_scene(H, W)
    record = G.record(objs, ocls, [[]], [[]], flavour, image=image)
    for merged in (True, False):
        for is_train in (False, True):
            mapper = _mapper(flavour, is_train, merged, np.random.RandomState(0), (48,), 140, crop=None)
            mapper.num_repeats = 2
            out = mapper(record)
            parts = out["part_instances"]
            assert tuple(parts.gt_masks.tensor.shape) == (0, 48, 64) and parts.gt_masks.tensor.dtype == torch.bool
            assert parts.gt_classes.shape == (0,) and parts.gt_classes.dtype == torch.int64 and out["orig_part_maps"] == []
            assert len(out["instances"]) == 1 and len(parts) == 0
    empty = dict(record, annotations=[], part_annotations=[])              # no objects at all
    out = _mapper(flavour, False, True, np.random.RandomState(0), (48,), 140)(empty)
    assert tuple(out["instances"].gt_masks.tensor.shape) == (0, 48, 64) and tuple(out["instances"].gt_boxes.shape) == (0, 4)
    assert tuple(out["part_instances"].gt_masks.tensor.shape) == (0, 48, 64)


# ------------------------------------------------------------------------------------------------ closing the loop
def test_test_mode_output_feeds_the_models_target_preparation():
    """a batch of two test-mode outputs of different sizes goes through SupervisedModel.prepare_targets and inference.prepare_gt_targets
    as it is"""
    from partdistillation_amd import inference
    from partdistillation_amd.supervised_model import SupervisedModel
    rng = np.random.RandomState(12)
    batch, wants = [], []
    for (H, W), size in (((90, 120), 48), ((100, 70), 64)):
        image = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        record = G.record(*G.scene(rng, H, W), "voc", image=image)
        theirs = np.random.RandomState(0)
        wants.append(G.call(record, image, "voc", theirs, False, (size,), 140, "choice", None, True)[0])
        batch.append(_mapper("voc", False, True, np.random.RandomState(0), (size,), 140)(record))
    model = types.SimpleNamespace(device=torch.device(DEV), class_agnostic_learning=False)
    images = types.SimpleNamespace(tensor=torch.zeros((2, 3, 96, 96), device=DEV))
    for targets in (SupervisedModel.prepare_targets(model, batch, images), inference.prepare_gt_targets(model, batch, images)):
        for t, want in zip(targets, wants):
            h, w = want["size"]
            assert tuple(t["masks"].shape) == (len(want["part_classes"]), 96, 96) and t["masks"].dtype == torch.bool
            assert np.array_equal(t["masks"][:, :h, :w].cpu().numpy(), want["part_masks"]) and int(t["masks"].sum()) == want["part_masks"].sum()
            assert np.array_equal(t["object_masks"][:, :h, :w].cpu().numpy(), want["obj_masks"])
            assert t["labels"].tolist() == want["part_classes"] and t["labels"].is_cuda
