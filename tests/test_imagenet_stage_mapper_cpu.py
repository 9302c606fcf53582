"""Host side of the ImageNet stage mappers (partdistillation_amd/data/imagenet_stage_mapper.py): the argument checks of
pd_rle_sample_groups_canvas_u8, the config surface, the refusals, the draws, the boxes from run lengths and the record builders.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import imagenet_stage_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "partdistillation_amd", "configs")
NAME = "pd_rle_sample_groups_canvas_u8"


def _cfg(yaml, extra=()):
    from partdistillation_amd.config import setup_cfg
    return setup_cfg(os.path.join(CONFIGS, yaml), ["MODEL.DEVICE", "cpu"] + list(extra))


# ------------------------------------------------------------------------------------------------ C-ABI
def test_canvas_entry_rejects_bad_arguments_before_any_launch():
    """the argument checks come before the memsets and the launch, so they answer without a device"""
    from partdistillation_amd import lib
    L = lib.load()
    limit = 1 << 20                                                        # PD_SAMPLE_GROUPS_MAX (include/pd_input.h)
    good = dict(n=3, H=33, W=70, vh=10, vw=7, out_h=12, out_w=9, n_groups=2)
    bad = {"negative n": dict(n=-1), "negative n_groups": dict(n_groups=-1), "n_groups above the limit": dict(n_groups=limit + 1),
           "H 0": dict(H=0), "W negative": dict(W=-5), "H * W over int32": dict(H=65536, W=32768), "out_h 0": dict(out_h=0),
           "out_w 0": dict(out_w=0), "out_h too large": dict(out_h=65536), "out_w too large": dict(out_w=65536),
           "vh negative": dict(vh=-1), "vw negative": dict(vw=-1), "vh > out_h": dict(vh=13), "vw > out_w": dict(vw=10),
           "null pointers": {}, "null pointers without groups": dict(n_groups=0), "null pointers without members": dict(n=0),
           "null pointers with an empty window": dict(vh=0)}
    for what, change in bad.items():
        a = dict(good, **change)
        rc = L.pd_rle_sample_groups_canvas_u8(None, None, a["n"], a["H"], a["W"], None, None, a["vh"], a["vw"], a["out_h"], a["out_w"], None,
                                              None, a["n_groups"], None, None, None, None)
        assert rc == -1 and L.pd_last_error().decode().startswith(NAME + ":"), what
        with pytest.raises(lib.PdHipError, match="null pointer" if what.startswith("null") else "bad sizes"):
            lib.check(rc)
    # each pointer on its own: everything else non-null (never dereferenced: the call returns before any launch)
    buf = (ctypes.c_int32 * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p).value
    names = ["starts", "offsets", "src_x", "src_y", "group_offsets", "group_members", "out", "member_area", "group_area"]

    def call(v, vh, vw):
        return L.pd_rle_sample_groups_canvas_u8(v["starts"], v["offsets"], 3, 33, 70, v["src_x"], v["src_y"], vh, vw, 12, 9,
                                                v["group_offsets"], v["group_members"], 2, v["out"], v["member_area"], v["group_area"], None)
    for missing in names:
        for vh, vw in ((10, 7), (0, 7), (10, 0)):
            if (vh == 0 or vw == 0) and missing in ("src_x", "src_y"):
                continue                                                   # not read with an empty window: the call would launch
            rc = call({k: (None if k == missing else ptr) for k in names}, vh, vw)
            assert rc == -1 and L.pd_last_error().decode() == NAME + ": null pointer", (missing, vh, vw)
    assert L.pd_rle_sample_groups_canvas_u8(None, None, 0, 33, 70, None, None, 10, 7, 12, 9, None, None, 0, None, None, None, None) == 0
    assert L.pd_rle_sample_groups_canvas_u8(None, None, 0, 33, 70, None, None, 13, 7, 12, 9, None, None, 0, None, None, None, None) == -1
    res, args = lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == 18 and [i for i, a in enumerate(args) if a is ctypes.c_int] == [2, 3, 4, 7, 8, 9, 10, 13]
    fn = L.pd_cmd_fn_index(NAME.encode())
    assert fn >= 0 and fn != L.pd_cmd_fn_index(b"pd_rle_sample_groups_u8")


def test_wrapper_refuses_a_window_larger_than_the_canvas():
    from partdistillation_amd.functions.input_pipeline import rle_sample_groups
    z = torch.zeros(4, dtype=torch.int32)
    offsets = torch.tensor([0, 1, 2], dtype=torch.int32)
    for canvas in ((3, 9), (9, 3)):
        with pytest.raises(ValueError, match="does not fit"):
            rle_sample_groups(z, offsets, 4, 4, z, z, [0, 2], [0, 1], canvas=canvas)


# ------------------------------------------------------------------------------------------------ config
def test_from_config_on_the_shipped_yamls():
    from partdistillation_amd.data import DeviceImagenetPartRankingMapper, DeviceProposalGenerationMapper
    for yaml in ("proposal_generation/r50.yaml", "proposal_generation/swinl.yaml"):
        cfg = _cfg(yaml)
        m = DeviceProposalGenerationMapper.from_config(cfg)
        assert (m.image_size, m.with_given_mask, m.device.type) == (cfg.INPUT.IMAGE_SIZE, False, "cpu")
        assert (m.image_size, m.square_base) == (cfg.INPUT.IMAGE_SIZE, False)
        m = DeviceProposalGenerationMapper.from_config(_cfg(yaml, ["INPUT.IMAGE_SIZE", "640", "PROPOSAL_GENERATION.WITH_GIVEN_MASK", "True"]))
        assert (m.image_size, m.with_given_mask) == (640, True)
    table = {"n01": 3}
    cfg = _cfg("part_ranking/r50_mask2former.yaml")
    assert cfg.MODEL.META_ARCHITECTURE == "PartRankingModel" and cfg.INPUT.MASK_FORMAT == "bitmask"
    m = DeviceImagenetPartRankingMapper.from_config(cfg, table)
    assert (m.image_size, m.device.type, m.class_code_to_class_index) == (640, "cpu", table)
    assert (m.image_size, m.square_base, m.pad_value) == (640, True, 128)
    assert DeviceImagenetPartRankingMapper.from_config(cfg, table, device="cuda").device.type == "cuda"


# ------------------------------------------------------------------------------------------------ refusals
def _parts(h, w, n=2):
    from partdistillation_amd.utils import rle
    m = np.zeros((n, h, w), dtype=bool)
    for i in range(n):
        m[i, i:h - 1, 2 * i:w // 2 + i] = True
    return [{"segmentation": rle.encode(x)} for x in m]


def test_refusals_come_before_any_device_work():
    from partdistillation_amd.data import DeviceImagenetPartRankingMapper, DeviceProposalGenerationMapper
    with pytest.raises(NotImplementedError, match="MASK_FORMAT 'polygon'"):
        DeviceImagenetPartRankingMapper.from_config(_cfg("part_ranking/r50_mask2former.yaml", ["INPUT.MASK_FORMAT", "polygon"]), {})
    image = np.zeros((40, 56, 3), dtype=np.uint8)                          # resized to 46 x 64
    m = DeviceImagenetPartRankingMapper(64, {"n01": 3}, device="cpu", rng=np.random.RandomState(0))
    base = {"file_name": "a/n01/x.JPEG", "class_code": "n01", "image": image}
    with pytest.raises(ValueError, match="no pseudo_annotations"):
        m(dict(base, pseudo_annotations=[]))
    with pytest.raises(ValueError, match=r"\(40, 56\).*\(46, 64\)"):
        m(dict(base, pseudo_annotations=_parts(46, 64) + _parts(40, 56)))
    with pytest.raises(KeyError):
        m(dict(base, class_code="n02", pseudo_annotations=_parts(46, 64)))
    with pytest.raises(RuntimeError, match="GPU only"):                    # no CPU fallback
        m(dict(base, pseudo_annotations=_parts(46, 64)))
    g = DeviceProposalGenerationMapper(64, True, device="cpu", rng=np.random.RandomState(0))
    assert g({"file_path": os.path.join(ROOT, "no", "such.JPEG")}) is None                   # unreadable: the reference's bare except
    assert g({"file_path": "x", "image": image, "pseudo_annotations": []}) is None           # no mask
    with pytest.raises(ValueError, match="Mismatched image shape"):
        g({"file_path": "x", "image": image, "height": 41, "width": 56})
    with pytest.raises(RuntimeError, match="GPU only"):
        g({"file_path": "x", "image": image, "pseudo_annotations": _parts(46, 64)})


# ------------------------------------------------------------------------------------------------ draws
def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[2] == sb[2] and np.array_equal(sa[1], sb[1])


def test_draws_are_consumed_in_the_reference_order():
    """proposal generation: ResizeScale's uniform(1.0, 1.0), one draw; part ranking: that, then FixedSizeCrop's uniform(0.0, 1.0), two
    draws — through `draw` and through the calls themselves (which stop at the device on this machine, after the draws)"""
    from partdistillation_amd.data import DeviceImagenetPartRankingMapper, DeviceProposalGenerationMapper
    image = np.zeros((40, 56, 3), dtype=np.uint8)
    for seed in (0, 7):
        mine, theirs = np.random.RandomState(seed), np.random.RandomState(seed)
        g = DeviceProposalGenerationMapper(64, True, device="cpu", rng=mine)
        g.draw()
        theirs.uniform(1.0, 1.0)
        assert _same_state(mine, theirs)
        assert g({"file_path": "x", "image": image, "pseudo_annotations": []}) is None
        O.proposal_generation_ref({"pseudo_annotations": []}, image, theirs, 64, True)
        assert _same_state(mine, theirs)
        assert g({"file_path": os.path.join(ROOT, "no", "such.JPEG")}) is None and _same_state(mine, theirs)   # no image, no draw
        r = DeviceImagenetPartRankingMapper(64, {"n01": 3}, device="cpu", rng=mine)
        r.draw()
        theirs.uniform(1.0, 1.0)
        theirs.uniform(0.0, 1.0)
        assert _same_state(mine, theirs)
        with pytest.raises(RuntimeError, match="GPU only"):
            r({"file_name": "x", "class_code": "n01", "image": image, "pseudo_annotations": _parts(46, 64)})
        theirs.uniform(1.0, 1.0)
        theirs.uniform(0.0, 1.0)
        assert _same_state(mine, theirs)
        one = np.random.RandomState(seed)
        one.uniform()
        assert not _same_state(mine, one)


# ------------------------------------------------------------------------------------------------ boxes
def test_boxes_and_areas_from_run_lengths_equal_the_dense_ones():
    from oracle import input_pipeline_ref as R
    from partdistillation_amd.data.imagenet_stage_mapper import run_area, run_box, run_lengths
    from partdistillation_amd.utils import rle
    rng = np.random.RandomState(3)
    masks = []
    for h, w in ((1, 1), (5, 9), (9, 5), (12, 12), (7, 1), (1, 7)):
        for density in (0.05, 0.5, 0.95):
            masks += [rng.rand(h, w) < density for _ in range(6)]
        masks += [np.zeros((h, w), dtype=bool), np.ones((h, w), dtype=bool)]
    spans = np.zeros((6, 8), dtype=bool)                                   # one run from the bottom of column 2 into the top of column 3
    spans[4:, 2] = True
    spans[:2, 3] = True
    masks.append(spans)
    corner = np.zeros((6, 8), dtype=bool)                                  # starts with ones: COCO's leading zero-length run
    corner[0, 0] = corner[5, 7] = True
    masks.append(corner)
    seen_empty = seen_span = 0
    for m in masks:
        h, w = m.shape
        for seg in (rle.encode(m), {"size": [h, w], "counts": rle.mask_to_counts(m).tolist()}):
            counts = run_lengths(seg)
            assert np.array_equal(R.rle_decode(counts, h, w), m)
            box = run_box(counts, h)
            assert box.dtype == np.float32 and np.array_equal(box, O.dense_box(m)), (m.astype(int), box)
            assert run_area(counts) == int(m.sum())
        seen_empty += not m.any()
        ends = np.cumsum(counts)
        seen_span += bool(((ends[1::2] - 1) // h > (ends - counts)[1::2] // h)[counts[1::2] > 0].any())
    assert seen_empty >= 6 and seen_span >= 20
    assert run_box(run_lengths(rle.encode(spans)), 6).tolist() == [2.0, 0.0, 4.0, 6.0]       # every row, although rows 2..3 are unset
    assert run_box([3, 0, 2, 1], 6).tolist() == [0.0, 5.0, 1.0, 6.0]                           # a zero-length run of ones covers nothing


# ------------------------------------------------------------------------------------------------ record builders
def test_imagenet_record(tmp_path):
    from partdistillation_amd.data import imagenet_record
    from partdistillation_amd.utils import rle
    table = {"n01": 5, "n02": 9}
    data, masks = str(tmp_path / "imagenet"), str(tmp_path / "detic")
    rec = imagenet_record(data, "n02", "n02_3.JPEG", table, class_name="tench")
    assert rec == {"file_path": os.path.join(data, "n02", "n02_3.JPEG"), "file_name": "n02_3.JPEG", "class_code": "n02",
                   "gt_object_class": 9, "class_name": "tench"}
    assert imagenet_record(data, "n02", "n02_3.JPEG", table, object_mask_path=masks) is None             # no Detic file
    os.makedirs(os.path.join(masks, "n02"))
    m = np.zeros((2, 46, 64), dtype=bool)
    m[0, 5:40, 3:60] = True
    m[1, 1:4, 1:4] = True
    saved = {"file_name": "n02_3.JPEG", "file_path": rec["file_path"], "class_code": "n02", "class_name": "tench",           # labeling_detic.py:99-110
             "object_masks": rle.masks_to_coco_json(m), "object_boxes": torch.zeros(2, 4), "object_scores": torch.tensor([0.9, 0.4]),
             "height": 46, "width": 64, "pred_names": ["tench", "tench"]}
    torch.save(saved, os.path.join(masks, "n02", "n02_3.JPEG"))
    got = imagenet_record(data, "n02", "n02_3.JPEG", table, "tench", masks)
    assert got == dict(rec, pseudo_annotations=[{"segmentation": saved["object_masks"][0]["segmentation"]}])   # the most confident mask only
    assert np.array_equal(O.decode(got["pseudo_annotations"][0]["segmentation"]), m[0])
    torch.save(dict(saved, object_masks=[]), os.path.join(masks, "n02", "n02_4.JPEG"))
    assert imagenet_record(data, "n02", "n02_4.JPEG", table, "tench", masks) is None                      # a file without masks
    with open(os.path.join(masks, "n02", "n02_5.JPEG"), "wb") as f:
        f.write(b"not a pickle")
    assert imagenet_record(data, "n02", "n02_5.JPEG", table, "tench", masks) is None                      # a corrupted file
    with pytest.raises(KeyError):
        imagenet_record(data, "n03", "n03_1.JPEG", table)


def test_imagenet_proposal_record(tmp_path):
    from partdistillation_amd.data import imagenet_proposal_record
    from partdistillation_amd.utils import rle
    table = {"n01": 5, "n02": 9}
    root = str(tmp_path / "stage1")
    os.makedirs(os.path.join(root, "n01"))
    labels = np.zeros((46, 64), dtype=np.uint8)
    labels[4:30, 5:40], labels[30:44, 5:40] = 1, 3
    saved = {"file_name": "n01_7.JPEG", "file_path": "imagenet/n01/n01_7.JPEG", "class_code": "n01", "class_name": "tench",   # _result
             "part_mask": rle.labels_to_coco_json(labels, [1, 3]), "object_ratio": float((labels > 0).mean()), "height": 46, "width": 64,
             "class_index": 5}

    def write(name, d):
        torch.save(d, os.path.join(root, "n01", name))
        return (root, "n01", name)
    got = imagenet_proposal_record(write("a", saved), table)
    assert got == {"file_name": "imagenet/n01/n01_7.JPEG", "image_id": "n01_7.JPEG", "class_code": "n01", "gt_object_class": 5, "height": 46,
                   "width": 64, "pseudo_annotations": [{"segmentation": p["segmentation"]} for p in saved["part_mask"]]}
    assert [int(O.decode(a["segmentation"]).sum()) for a in got["pseudo_annotations"]] == [26 * 35, 14 * 35]
    ratio = saved["object_ratio"]
    assert imagenet_proposal_record(write("a", saved), table, min_object_area_ratio=ratio - 1e-6) is not None
    assert imagenet_proposal_record(write("a", saved), table, min_object_area_ratio=ratio) is None          # not ABOVE the threshold
    assert imagenet_proposal_record(write("b", dict(saved, part_mask=[])), table) is None
    assert imagenet_proposal_record(write("c", dict(saved, part_mask=None)), table) is None
    with open(os.path.join(root, "n01", "d"), "wb") as f:
        f.write(b"\x80\x04truncated")
    assert imagenet_proposal_record((root, "n01", "d"), table) is None                                      # corrupted
    with pytest.raises(OSError):
        imagenet_proposal_record((root, "n01", "missing"), table)                                           # missing is not corrupted
