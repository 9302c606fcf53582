"""The ImageNet stage mappers on the device: pd_rle_sample_groups_canvas_u8 (include/pd_input.h) alone against a numpy loop, then
DeviceProposalGenerationMapper / DeviceImagenetPartRankingMapper end to end against the reference's mappers restated on the Pillow-pinned
oracle pieces (tests/imagenet_stage_oracle.py), then stage 1 -> saved files -> part-ranking input as one chain.  Everything is integer
arithmetic: every comparison is exact equality."""
import os
from unittest import mock

import numpy as np
import pytest
import torch

import imagenet_stage_oracle as O
import input_chain_oracle as B

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 64
TILE = 2048                                                                # SG_TILE of csrc/input_pipeline.hip
LDS_RUNS = 2048                                                            # SG_LDS_RUNS


# ------------------------------------------------------------------------------------------------ the kernel alone
def _sample(masks, sx, sy, groups, canvas, garbage=7):
    """masks bool [n, H, W] -> the three outputs as numpy, pre-filled with garbage so that an unwritten byte shows; canvas None = the
    existing entry pd_rle_sample_groups_u8"""
    from partdistillation_amd.functions.input_pipeline import rle_sample_groups
    from partdistillation_amd.utils import rle
    (H, W), segs = masks.shape[1:], [rle.encode(m) for m in masks]
    starts, offsets = rle.segmentations_to_starts(segs, (H, W))
    n, ng = len(segs), len(groups)
    d = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV) for a in (starts, offsets, sx, sy)]
    shape = (len(sy), len(sx)) if canvas is None else canvas
    out = torch.full((ng,) + tuple(shape), garbage, dtype=torch.uint8, device=DEV)
    m_area = torch.full((n,), garbage, dtype=torch.int32, device=DEV)
    g_area = torch.full((ng,), garbage, dtype=torch.int32, device=DEV)
    g_off = np.concatenate(([0], np.cumsum([len(g) for g in groups]))).astype(np.int32)
    g_mem = np.asarray([m for g in groups for m in g], dtype=np.int32)
    rle_sample_groups(d[0], d[1], H, W, d[2], d[3], g_off, g_mem, out, m_area, g_area, canvas=canvas)
    return out.cpu().numpy(), m_area.cpu().numpy(), g_area.cpu().numpy()


def _blobs(rng, n, H, W, density=0.35):
    m = rng.rand(n, H, W) < density
    m[0, 0, 0] = True                                                      # starts with ones: COCO's leading zero count
    return m


def _case(name):
    """-> (masks, src_x, src_y, groups, canvas)"""
    rng = np.random.RandomState(len(name) * 7 + 1)
    if name == "partial_last_tile":
        masks, canvas = _blobs(rng, 3, 33, 70), (50, 259)
        sx, sy = rng.randint(0, 70, 66), rng.randint(0, 33, 47)
        assert -(-canvas[0] * canvas[1] // TILE) == 7 and canvas[0] * canvas[1] % TILE != 0      # 7 tiles, the last one partial
        assert len(sy) < canvas[0] and len(sx) < canvas[1]                                           # both pads
        return masks, sx, sy, [[0, 1], [2]], canvas
    if name == "window_equals_canvas":
        return _blobs(rng, 2, 8, 8), np.arange(8), np.arange(8), [[0], [0, 1]], (8, 8)
    if name == "one_pixel":
        return np.ones((1, 1, 1), dtype=bool), [0], [0], [[0]], (1, 1)
    if name == "vh_0":
        return _blobs(rng, 2, 9, 20), np.arange(20), [], [[0, 1], [1]], (12, 300)
    if name == "vw_0":
        return _blobs(rng, 2, 9, 20), [], np.arange(9), [[0, 1], [1]], (12, 300)
    if name == "groups_and_overlap":
        masks = _blobs(rng, 5, 20, 30)
        masks[1, :10] |= masks[0, :10]                                     # members 0 and 1 overlap
        groups = [[0, 1], [1, 2], [], [0, 1, 2]]                           # three groups over overlapping members, one empty; member 3, 4 in none
        assert (masks[0] & masks[1]).sum() > 20 and not any(m in g for g in groups for m in (3, 4))
        return masks, np.arange(30), np.arange(20), groups, (24, 40)
    if name == "long_run_table":
        from partdistillation_amd.functions.input_pipeline import nearest_index
        from partdistillation_amd.utils import rle
        masks = (np.add.outer(np.arange(48), np.arange(64)) % 2).astype(bool)[None]
        assert len(rle.mask_to_counts(masks[0])) > LDS_RUNS               # searched in place, not staged on chip
        return masks, np.arange(64), nearest_index(48, 46), [[0]], (64, 64)
    if name == "shuffled_tables":
        masks = _blobs(rng, 3, 17, 23)
        sx, sy = rng.randint(0, 23, 40), rng.randint(0, 17, 29)
        assert len(set(sx.tolist())) < len(sx) and len(set(sy.tolist())) < len(sy) and (np.diff(sx) < 0).any() and (np.diff(sy) < 0).any()
        return masks, sx, sy, [[0, 2], [1]], (31, 45)
    raise KeyError(name)


CASES = ["partial_last_tile", "window_equals_canvas", "one_pixel", "vh_0", "vw_0", "groups_and_overlap", "long_run_table", "shuffled_tables"]


@pytest.mark.parametrize("name", CASES)
def test_canvas_kernel_against_a_numpy_loop(name):
    masks, sx, sy, groups, canvas = _case(name)
    sx, sy = np.asarray(sx, dtype=np.int64), np.asarray(sy, dtype=np.int64)
    got = _sample(masks, sx, sy, groups, canvas)
    want = O.canvas_ref(masks, sx, sy, groups, canvas)
    for g, w, what in zip(got, want, ("planes", "member_area", "group_area")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), what
    planes, m_area, g_area = got
    vh, vw = len(sy), len(sx)
    assert planes.max(initial=0) <= 1 and not planes[:, vh:].any() and not planes[:, :, vw:].any()      # no garbage left, the pad is 0
    if name in ("vh_0", "vw_0"):
        assert not planes.any() and not m_area.any() and not g_area.any() and planes.shape == (2, 12, 300)
        return
    assert m_area.sum() > 0 and g_area.sum() > 0
    if name == "one_pixel":
        assert planes.tolist() == [[[1]]] and m_area.tolist() == [1] == g_area.tolist()
    if name == "groups_and_overlap":
        assert g_area[0] < m_area[0] + m_area[1] and g_area[2] == 0 and not planes[2].any() and m_area[3] > 0 and m_area[4] > 0
        assert g_area[3] == (planes[0] | planes[1]).sum()                                                  # the union is counted once
    # the existing entry on the same inputs, and the new one with canvas == window: byte-equal
    old = _sample(masks, sx, sy, groups, None)
    new = _sample(masks, sx, sy, groups, (vh, vw))
    for a, b, w in zip(old, new, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    assert np.array_equal(old[0], want[0][:, :vh, :vw]) and np.array_equal(old[1], want[1]) and np.array_equal(old[2], want[2])


# ------------------------------------------------------------------------------------------------ the mappers end to end
# source -> resized at S = 64 (ResizeScale rounds with np.round).  A 30 x 300 source resizes to 6 x 64; the 14 x 64 window is a 66 x 300
# source's: both narrow windows are kept.
SOURCES = {(40, 56): (46, 64), (56, 40): (64, 46), (64, 64): (64, 64), (30, 300): (6, 64), (66, 300): (14, 64)}
CLASS_INDEX = {"n0123": 7, "n0456": 3}


def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[2] == sb[2] and np.array_equal(sa[1], sb[1])


def _segs(masks):
    from partdistillation_amd.utils import rle
    out = []
    for m in masks:
        r = rle.encode(m)
        r["counts"] = r["counts"].decode("utf-8")
        out.append({"segmentation": r})
    return out


def _ranking_parts(rng, bh, bw, n):
    """n part masks at the resized size; from three parts on, part 1 overlaps part 0 and part 2 is empty"""
    parts = B.part_masks(rng, bh, bw, n)
    if n >= 3:
        parts[0, bh // 2, bw // 4:bw // 2] = True                          # wide enough to meet its own shift
        parts[1] |= np.roll(parts[0], 1, axis=1)
        parts[2] = False
        assert (parts[0] & parts[1]).any() and not parts[2].any()
    assert parts.any()
    return parts


@pytest.mark.parametrize("n_parts", [1, 3, 8])
@pytest.mark.parametrize("source", list(SOURCES))
def test_part_ranking_mapper_against_the_oracle(source, n_parts):
    from partdistillation_amd.data import DeviceImagenetPartRankingMapper
    bh, bw = SOURCES[source]
    assert B.base_shape(*source, S) == (bh, bw)
    rng = np.random.RandomState(source[0] + n_parts)
    image = B.random_image(rng, *source)
    parts = _ranking_parts(rng, bh, bw, n_parts)
    record = {"file_name": "imagenet/n0123/n0123_5.JPEG", "image_id": "n0123_5.JPEG", "class_code": "n0123", "gt_object_class": 11,
              "height": bh, "width": bw, "pseudo_annotations": _segs(parts), "image": image}
    before = dict(record)
    mine, theirs = np.random.RandomState(5), np.random.RandomState(5)
    want = O.part_ranking_ref(record, image, theirs, S, CLASS_INDEX)
    with mock.patch("torch.cuda.synchronize") as sync:
        out = DeviceImagenetPartRankingMapper(S, CLASS_INDEX, device=DEV, rng=mine)(record)
    assert not sync.called                                                 # reading the outputs below is the first synchronisation
    inst = out["instances"]
    assert out["image"].dtype == torch.uint8 and out["image"].is_cuda and tuple(out["image"].shape) == (3, S, S)
    assert np.array_equal(out["image"].cpu().numpy(), want["image"])
    assert (out["height"], out["width"]) == (S, S) == inst.image_size
    assert inst.gt_masks.tensor.dtype == torch.bool and inst.gt_masks.tensor.is_cuda and tuple(inst.gt_masks.tensor.shape) == (1, S, S)
    assert np.array_equal(inst.gt_masks.tensor.cpu().numpy(), want["mask"]) and want["mask"].any()
    assert not want["mask"][0, bh:].any() and not want["mask"][0, :, bw:].any()
    assert inst.gt_classes.dtype == torch.int64 and inst.gt_classes.is_cuda and inst.gt_classes.tolist() == want["classes"] == [7]
    assert len(inst) == 1 and _same_state(mine, theirs)
    assert "pseudo_annotations" not in out and "pseudo_annotations" in record and all(record[k] is before[k] for k in before)
    assert {k: out[k] for k in ("file_name", "image_id", "class_code", "gt_object_class")} == \
        {k: record[k] for k in ("file_name", "image_id", "class_code", "gt_object_class")}


def _object_masks(kind, bh, bw):
    """the pseudo-annotations of a proposal-generation record at the resized size"""
    obj = np.zeros((bh, bw), dtype=bool)
    obj[bh // 8:bh - bh // 6, bw // 7:bw - bw // 9] = True
    small = np.zeros((bh, bw), dtype=bool)
    small[bh - 1, 0] = small[0, bw - 1] = True
    empty = np.zeros((bh, bw), dtype=bool)
    if kind == "one":
        return _segs([obj])
    if kind == "only_empty":
        return _segs([empty])
    annos = _segs([empty, obj, small])                                     # "several": the empty one is dropped, one has a class
    annos[2]["category_id"] = 4
    return annos


@pytest.mark.parametrize("kind", ["off", "one", "only_empty", "several"])
@pytest.mark.parametrize("source", [s for s in SOURCES if s != (66, 300)])
def test_proposal_generation_mapper_against_the_oracle(source, kind):
    from partdistillation_amd.data import DeviceProposalGenerationMapper
    bh, bw = SOURCES[source]
    rng = np.random.RandomState(source[1] + len(kind))
    image = B.random_image(rng, *source)
    record = {"file_path": "imagenet/n0456/n0456_1.JPEG", "file_name": "n0456_1.JPEG", "class_code": "n0456", "gt_object_class": 3,
              "class_name": "hen", "image": image}
    if kind != "off":
        record["pseudo_annotations"] = _object_masks(kind, bh, bw)
    keys = set(record)
    mine, theirs = np.random.RandomState(9), np.random.RandomState(9)
    want = O.proposal_generation_ref(record, image, theirs, S, kind != "off")
    with mock.patch("torch.cuda.synchronize") as sync:
        out = DeviceProposalGenerationMapper(S, kind != "off", device=DEV, rng=mine)(record)
    assert not sync.called and _same_state(mine, theirs) and set(record) == keys
    if kind == "only_empty":
        assert want is None and out is None
        return
    assert out["image"].dtype == torch.uint8 and out["image"].is_cuda and tuple(out["image"].shape) == (3, bh, bw)
    assert np.array_equal(out["image"].cpu().numpy(), want["image"]) and (out["height"], out["width"]) == (bh, bw) == want["size"]
    assert "pseudo_annotations" not in out and out["file_path"] == record["file_path"] and out["class_name"] == "hen"
    if kind == "off":
        assert "instances" not in out
        return
    inst = out["instances"]
    assert inst.image_size == (bh, bw) and len(inst) == {"one": 1, "several": 2}[kind]
    assert inst.gt_masks.tensor.dtype == torch.bool and inst.gt_masks.tensor.is_cuda
    assert np.array_equal(inst.gt_masks.tensor.cpu().numpy(), want["masks"])
    assert inst.gt_classes.dtype == torch.int64 and inst.gt_classes.is_cuda and inst.gt_classes.tolist() == want["classes"]
    assert want["classes"] == {"one": [-1], "several": [-1, 4]}[kind]
    assert torch.is_tensor(inst.gt_boxes) and inst.gt_boxes.dtype == torch.float32 and inst.gt_boxes.is_cuda
    assert np.array_equal(inst.gt_boxes.cpu().numpy(), want["boxes"]) and want["boxes"].dtype == np.float32
    assert want["boxes"][0].tolist() == [bw // 7, bh // 8, bw - bw // 9, bh - bh // 6]
    if kind == "several":
        assert want["boxes"][1].tolist() == [0.0, 0.0, float(bw), float(bh)]


def test_masks_of_another_stored_size_are_passed_through():
    """the reference hands the masks an empty transform list: they stay at their stored size, whatever the image is resized to"""
    from partdistillation_amd.data import DeviceProposalGenerationMapper
    image = B.random_image(np.random.RandomState(1), 40, 56)
    m = np.zeros((40, 56), dtype=bool)
    m[3:30, 10:50] = True
    out = DeviceProposalGenerationMapper(S, True, device=DEV, rng=np.random.RandomState(0))({"file_path": "x", "image": image,
                                                                                               "pseudo_annotations": _segs([m])})
    assert tuple(out["image"].shape) == (3, 46, 64) and out["instances"].image_size == (46, 64)
    assert np.array_equal(out["instances"].gt_masks.tensor.cpu().numpy(), m[None])
    assert out["instances"].gt_boxes.tolist() == [[10.0, 3.0, 50.0, 30.0]]


# ------------------------------------------------------------------------------------------------ the stage chain
def _stage1_model(feats, init, save_path, K=4):
    """ProposalGenerationModel on a stub backbone that returns fixed features (as tests/test_propgen_gpu.py::_model)"""
    from partdistillation_amd.proposal_generation_model import ProposalGenerationModel

    class Stub(torch.nn.Module):
        size_divisibility = 32

        def forward(self, x):
            return {k: v.to(x.device) for k, v in feats.items()}
    m = ProposalGenerationModel(backbone=Stub(), size_divisibility=32, dataset_name="synthetic", pixel_mean=[123.675, 116.28, 103.53],
                                pixel_std=[58.395, 57.12, 57.375], distance_metric="dot", backbone_feature_key_list=["res3", "res4"],
                                num_superpixel_clusters=K, feature_normalize=False, save_path=save_path)
    m.init_centroids = lambda i: init.to(DEV)
    return m.to(DEV).eval()


def test_stage_chain_detic_masks_to_part_ranking_input(tmp_path):
    """image files + Detic-format object masks -> imagenet_record -> DeviceProposalGenerationMapper -> ProposalGenerationModel (saving) ->
    imagenet_proposal_record -> DeviceImagenetPartRankingMapper: the object mask part ranking sees is stage 1's (labels > 0), padded"""
    from PIL import Image
    from partdistillation_amd.data import (DeviceImagenetPartRankingMapper, DeviceProposalGenerationMapper, imagenet_proposal_record,
                                           imagenet_record)
    from partdistillation_amd.utils import rle
    K, table = 4, {"n0123": 0, "n0456": 1}
    data, detic, stage1 = (str(tmp_path / d) for d in ("imagenet", "detic", "stage1"))
    rng = np.random.RandomState(21)
    items = [("n0123", "n0123_1.png", (40, 56)), ("n0456", "n0456_2.png", (56, 40))]
    images, objects = {}, {}
    for code, name, (h, w) in items:
        bh, bw = SOURCES[(h, w)]
        images[name] = B.random_image(rng, h, w)
        os.makedirs(os.path.join(data, code))
        Image.fromarray(images[name]).save(os.path.join(data, code, name))                              # lossless
        obj = np.zeros((bh, bw), dtype=bool)
        obj[3:bh - 4, 5:bw - 3] = True
        obj[3:9, 5:12] = False
        assert obj.mean() >= 0.5
        objects[name] = obj
        second = np.zeros_like(obj)
        second[:5, :5] = True                                                                           # a less confident mask: not used
        os.makedirs(os.path.join(detic, code))
        torch.save({"file_name": name, "file_path": os.path.join(data, code, name), "class_code": code, "class_name": code,
                    "object_masks": rle.masks_to_coco_json(np.stack([obj, second])), "object_boxes": torch.zeros(2, 4),
                    "object_scores": torch.tensor([0.9, 0.2]), "height": bh, "width": bw, "pred_names": [code, code]},
                   os.path.join(detic, code, name))
    gen = DeviceProposalGenerationMapper(S, True, device=DEV, rng=np.random.RandomState(0))
    batch = []
    for code, name, _ in items:
        rec = imagenet_record(data, code, name, table, class_name=code, object_mask_path=detic)
        assert "image" not in rec                                                                       # read from file_path with Pillow
        batch.append(gen(rec))
    assert [tuple(b["image"].shape) for b in batch] == [(3, 46, 64), (3, 64, 46)]
    g = torch.Generator().manual_seed(3)
    centres = torch.randn(K, 40, generator=g)                                                           # four well separated blobs
    which = torch.randint(0, K, (2, 8, 8), generator=g)
    field = centres[which].permute(0, 3, 1, 2) * 2.0 + 0.3 * torch.randn(2, 40, 8, 8, generator=g)       # [2, 40, 8, 8]
    feats = {"res3": field[:, :16].contiguous(), "res4": field[:, 16:, ::2, ::2].contiguous()}
    model = _stage1_model(feats, centres * 2.0, stage1, K)
    results = model(batch)
    assert all(r is not None for r in results)                                                          # both objects have more than K feature pixels
    rank = DeviceImagenetPartRankingMapper(S, table, device=DEV, rng=np.random.RandomState(0))
    for (code, name, (h, w)), r in zip(items, results):
        bh, bw = SOURCES[(h, w)]
        assert os.path.exists(os.path.join(stage1, code, name)) and tuple(r["labels"].shape) == (bh, bw)
        rec = imagenet_proposal_record((stage1, code, name), table)
        assert rec is not None and rec["file_name"] == os.path.join(data, code, name) and (rec["height"], rec["width"]) == (bh, bw)
        assert len(rec["pseudo_annotations"]) == len(r["present_labels"]) >= 1
        out = rank(rec)
        want = np.zeros((1, S, S), dtype=bool)
        want[0, :bh, :bw] = (r["labels"] > 0).cpu().numpy()
        assert np.array_equal(want[0, :bh, :bw], objects[name])                                         # stage 1 labels exactly the object
        assert np.array_equal(out["instances"].gt_masks.tensor.cpu().numpy(), want)
        assert np.array_equal(out["image"].cpu().numpy(), B.base_image_ref(images[name], S, True).transpose(2, 0, 1))
        assert out["instances"].gt_classes.tolist() == [table[code]] and out["gt_object_class"] == table[code]
        assert (out["height"], out["width"]) == (S, S) and "pseudo_annotations" not in out
