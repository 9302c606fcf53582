"""Host side of the ground-truth part mappers (partdistillation_amd/data/gt_part_mapper.py): the oracle helper of the GPU tests
(tests/gt_part_oracle.py) against Pillow itself, ResizeShortestEdge's output shape, the draw order, the box transform, the group table,
the config surface, the refusals and the argument checks of pd_rle_sample_groups_u8.  No GPU."""
import os

import numpy as np
import pytest

import gt_part_oracle as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "partdistillation_amd", "configs")


# ------------------------------------------------------------------------------------------------ helper against Pillow
@pytest.mark.parametrize("H,W,short", [(37, 53, 64), (90, 61, 33)])
def test_oracle_chain_equals_the_same_steps_done_with_pillow(H, W, short):
    """resize -> flip -> crop of the image (BILINEAR) and of a mask (NEAREST), each step written directly with Pillow / numpy"""
    from PIL import Image
    rng = np.random.RandomState(H + short)
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    mask = rng.rand(H, W) < 0.4
    rh, rw = G.output_shape(H, W, short, 1000)
    assert min(rh, rw) == short and (rh, rw) != (H, W)
    for flip in (False, True):
        for crop in ((0, 0, rw, rh), (3, 5, rw - 7, rh - 9), (rw - 4, rh - 2, 4, 2)):
            p = {"in_h": H, "in_w": W, "resize": (rh, rw), "flip": flip, "crop": crop}
            a = np.asarray(Image.fromarray(img).resize((rw, rh), Image.BILINEAR))
            m = np.asarray(Image.fromarray(mask.astype(np.uint8)).resize((rw, rh), Image.NEAREST)).astype(bool)
            if flip:
                a, m = a[:, ::-1], m[:, ::-1]
            x0, y0, cw, ch = crop
            assert np.array_equal(G.chain_image(img, p), a[y0:y0 + ch, x0:x0 + cw])
            assert np.array_equal(G.chain_mask(mask, p), m[y0:y0 + ch, x0:x0 + cw])


# ------------------------------------------------------------------------------------------------ ResizeShortestEdge
def test_get_output_shape_hand_computed():
    from partdistillation_amd.data.gt_part_mapper import DeviceVOCPartsMapper, get_output_shape
    assert get_output_shape(480, 640, 800, 1333) == (800, 1067)            # the short edge governs: 640 * 800 / 480 = 1066.67
    assert get_output_shape(640, 480, 800, 1333) == (1067, 800)
    assert get_output_shape(400, 1000, 800, 1333) == (533, 1333)           # (800, 2000) -> times 1333 / 2000: the MAX_SIZE clamp
    assert get_output_shape(10, 25, 5, 100) == (5, 13)                     # 12.5 -> int(12.5 + 0.5) = 13, where np.round gives 12
    assert get_output_shape(25, 10, 5, 100) == (13, 5)
    assert get_output_shape(64, 64, 64, 64) == (64, 64)
    for case in [(480, 640, 800, 1333), (400, 1000, 800, 1333), (10, 25, 5, 100), (90, 61, 33, 40)]:
        assert get_output_shape(*case) == G.output_shape(*case)
    # size 0 is detectron2's NoOpTransform: the image keeps its size, and the draw is still made
    m = DeviceVOCPartsMapper(False, (0,), 1333, device="cpu", rng=np.random.RandomState(0))
    assert m.draw(37, 53) == {"in_h": 37, "in_w": 53, "resize": (37, 53), "flip": False, "crop": (0, 0, 53, 37)}


# ------------------------------------------------------------------------------------------------ draws
class RecordingRNG:
    def __init__(self, seed):
        self.state, self.calls = np.random.RandomState(seed), []

    def __getattr__(self, name):
        fn = getattr(self.state, name)

        def call(*a, **k):
            self.calls.append(name)
            return fn(*a, **k)
        return call


@pytest.mark.parametrize("flavour", ["voc", "city"])
@pytest.mark.parametrize("is_train,crop", [(True, True), (True, False), (False, True), (False, False)])
def test_draw_order_and_count(flavour, is_train, crop):
    """per attempt, in list order: the short edge (choice, or randint(lo, hi + 1) for "range"), then in train mode the flip's uniform(),
    then the crop's rand(2) + two randint when it is enabled; nothing else, and the values of the oracle's restatement"""
    from partdistillation_amd.data import DeviceCityscapesPartMapper, DeviceVOCPartsMapper
    cls = DeviceVOCPartsMapper if flavour == "voc" else DeviceCityscapesPartMapper
    ctype, csize = ("relative_range", (0.6, 0.7)) if crop else (None, None)
    for style, sizes in (("choice", (48, 64, 80)), ("range", (40, 90))):
        rec = RecordingRNG(5)
        m = cls(is_train, sizes, 100, style, ctype, csize, device="cpu", rng=rec)
        want_rng = np.random.RandomState(5)
        first = "randint" if style == "range" else "choice"
        per_attempt = [first] + (["uniform"] if is_train else []) + (["rand", "randint", "randint"] if is_train and crop else [])
        for _ in range(12):
            rec.calls.clear()
            got = m.draw(90, 61)
            assert rec.calls == per_attempt
            assert got == G.draw(want_rng, 90, 61, sizes, 100, style, is_train, (ctype, csize) if is_train and crop else None)
        rec.calls.clear()
        got = m.draw(90, 61, crop=False)                                   # the pass after the last attempt: the list without the crop
        assert rec.calls == [first] + (["uniform"] if is_train else [])
        assert got == G.draw(want_rng, 90, 61, sizes, 100, style, is_train, None) and got["crop"] == (0, 0) + got["resize"][::-1]


# ------------------------------------------------------------------------------------------------ boxes
def test_box_transform_against_corner_by_corner_arithmetic():
    from partdistillation_amd.data.gt_part_mapper import boxes_nonempty, transform_boxes
    rng = np.random.RandomState(2)
    H, W = 90, 120
    boxes = np.concatenate([np.sort(rng.rand(40, 2) * W, axis=1)[:, [0]], np.sort(rng.rand(40, 2) * H, axis=1)[:, [0]],
                            rng.rand(40, 1) * W, rng.rand(40, 1) * H], axis=1)
    boxes[:, 2:] = np.maximum(boxes[:, 2:], boxes[:, :2])
    boxes[0] = [10, 20, 10, 60]                                            # zero width: empty before and after
    boxes[1] = [0, 0, W, H]
    flips = 0
    for _ in range(10):
        p = G.draw(rng, H, W, (48, 64, 80), 100, "choice", True, ("relative_range", (0.5, 0.5)))
        flips += p["flip"]
        got = transform_boxes(boxes, p)
        want = np.asarray([G.box_ref(b, p) for b in boxes])
        assert got.dtype == np.float64 and np.array_equal(got, want)
        assert boxes_nonempty(got).tolist() == [G._nonempty_box(b) for b in want] and not boxes_nonempty(got)[0]
        assert got[1].tolist() == [0.0, 0.0, float(p["crop"][2]), float(p["crop"][3])]
        assert not boxes_nonempty(got).all()                               # the half crop pushes some boxes out of the window
    assert 0 < flips < 10
    assert transform_boxes(np.zeros((0, 4)), p).shape == (0, 4)


# ------------------------------------------------------------------------------------------------ group table
def test_group_table_assembly():
    from partdistillation_amd.data.gt_part_mapper import group_table
    # 3 objects; parts (object, class, passes the box filter): object 1 has no surviving part, object 2 has two parts of class 4
    part_obj = [0, 0, 0, 1, 2, 2, 2]
    part_cls = [5, 2, 5, 3, 4, 1, 4]
    part_ok = [True, True, True, False, True, True, True]
    off, mem, g_obj, g_cls = group_table(3, part_obj, part_cls, part_ok, merged=True)
    groups = [mem[a:b].tolist() for a, b in zip(off[:-1], off[1:])]
    assert off.dtype == np.int32 and mem.dtype == np.int32
    assert groups == [[0], [1], [2], [3 + 1], [3 + 0, 3 + 2], [3 + 5], [3 + 4, 3 + 6]]      # objects alone, then (object, class ascending)
    assert g_obj.tolist() == [0, 0, 2, 2] and g_cls.tolist() == [2, 5, 1, 4]
    part_ok[2] = False                                                     # a box-filtered part leaves its plane
    off, mem, g_obj, g_cls = group_table(3, part_obj, part_cls, part_ok, merged=True)
    assert [mem[a:b].tolist() for a, b in zip(off[:-1], off[1:])][3:5] == [[4], [3]]
    off, mem, g_obj, g_cls = group_table(3, part_obj, part_cls, part_ok, merged=False)   # one plane per part, empty when filtered
    assert [mem[a:b].tolist() for a, b in zip(off[:-1], off[1:])] == [[0], [1], [2], [3], [4], [], [], [7], [8], [9]]
    assert g_obj.tolist() == part_obj and g_cls.tolist() == part_cls
    off, mem, g_obj, g_cls = group_table(0, [], [], [], merged=True)
    assert off.tolist() == [0] and len(mem) == 0 and len(g_obj) == 0


# ------------------------------------------------------------------------------------------------ config
class RecordingCfg:
    """reads through to a config node and records the dotted paths of the leaves that were read"""

    def __init__(self, node, seen, path=""):
        self.__dict__.update(_node=node, _seen=seen, _path=path)

    def __getattr__(self, name):
        v = getattr(self._node, name)
        path = f"{self._path}.{name}" if self._path else name
        if hasattr(v, "keys"):
            return RecordingCfg(v, self._seen, path)
        self._seen.add(path)
        return v


def _cfg(extra):
    from partdistillation_amd.config import setup_cfg
    return setup_cfg(os.path.join(CONFIGS, "proposal_learning/r50_mask2former.yaml"), ["MODEL.DEVICE", "cpu"] + list(extra))


def test_from_config_reads_its_keys():
    from partdistillation_amd.data import DeviceCityscapesPartMapper, DeviceVOCPartsMapper
    allowed = {"INPUT.MIN_SIZE_TRAIN", "INPUT.MAX_SIZE_TRAIN", "INPUT.MIN_SIZE_TRAIN_SAMPLING", "INPUT.MIN_SIZE_TEST", "INPUT.MAX_SIZE_TEST",
               "INPUT.CROP.ENABLED", "INPUT.CROP.TYPE", "INPUT.CROP.SIZE", "INPUT.COLOR_AUG_SSD", "CUSTOM_DATASETS.USE_MERGED_GT", "MODEL.DEVICE"}
    cfg = _cfg(["INPUT.MIN_SIZE_TRAIN", "(480, 512)", "INPUT.MAX_SIZE_TRAIN", "900", "INPUT.MIN_SIZE_TRAIN_SAMPLING", "range",
                "INPUT.MIN_SIZE_TEST", "640", "INPUT.MAX_SIZE_TEST", "1000", "INPUT.CROP.ENABLED", "True", "INPUT.CROP.TYPE", "absolute",
                "INPUT.CROP.SIZE", "(384, 400)", "CUSTOM_DATASETS.USE_MERGED_GT", "False"])
    seen = set()
    for cls in (DeviceVOCPartsMapper, DeviceCityscapesPartMapper):
        m = cls.from_config(RecordingCfg(cfg, seen), is_train=True)
        assert (m.is_train, m.min_size, m.max_size, m.sample_style) == (True, (480, 512), 900, "range")
        assert (m.crop_type, m.crop_size, m.use_merged_gt, m.device.type) == ("absolute", (384, 400), False, "cpu")
    t = DeviceVOCPartsMapper.from_config(RecordingCfg(cfg, seen), is_train=False)       # Pascal: the TRAIN sizes in test mode too
    assert (t.is_train, t.min_size, t.max_size, t.sample_style, t.crop_type) == (False, (480, 512), 900, "range", None)
    t = DeviceCityscapesPartMapper.from_config(RecordingCfg(cfg, seen), is_train=False)
    assert (t.is_train, t.min_size, t.max_size, t.sample_style, t.crop_type) == (False, (640, 640), 1000, "choice", None)
    assert seen == allowed
    d = DeviceVOCPartsMapper.from_config(_cfg([]))                         # the defaults: merged ground truth, no crop
    assert d.use_merged_gt and d.crop_type is None and d.min_size == (800,) and d.sample_style == "choice"
    assert (DeviceVOCPartsMapper.num_repeats, DeviceVOCPartsMapper.min_parts, DeviceVOCPartsMapper.filter_by_box,
            DeviceVOCPartsMapper.part_class_key) == (100, 2, True, "orig_part_category_id")
    assert (DeviceCityscapesPartMapper.num_repeats, DeviceCityscapesPartMapper.min_parts, DeviceCityscapesPartMapper.filter_by_box,
            DeviceCityscapesPartMapper.part_class_key) == (20, 1, False, "part_category_id")


# ------------------------------------------------------------------------------------------------ refusals
def test_the_three_refusals():
    from partdistillation_amd.data import DeviceCityscapesPartMapper, DeviceVOCPartsMapper
    with pytest.raises(NotImplementedError, match="COLOR_AUG_SSD"):
        DeviceVOCPartsMapper.from_config(_cfg(["INPUT.COLOR_AUG_SSD", "True"]), is_train=True)
    with pytest.raises(NotImplementedError, match="polygon"):
        DeviceVOCPartsMapper(True, (64,), 100, device="cpu", mask_format="polygon")
    rng = np.random.RandomState(0)
    rec = G.record(*G.scene(rng, 24, 30, n_obj=1, n_parts=2), "voc", image=np.zeros((24, 30, 3), np.uint8))
    rec["part_annotations"][0][0]["segmentation"] = [[1.0, 1.0, 8.0, 1.0, 8.0, 8.0]]
    with pytest.raises(NotImplementedError, match="polygon"):                # before anything touches the device
        DeviceVOCPartsMapper(False, (32,), 100, device="cpu")(rec)
    with pytest.raises(NotImplementedError, match="panoptic_parts"):
        DeviceCityscapesPartMapper(False, (32,), 100, device="cpu")(({"file_name": "x.png"}, "x_gtFinePanopticParts.tif"))
    rec = G.record(*G.scene(rng, 24, 30, n_obj=1, n_parts=2), "voc", image=np.zeros((24, 30, 3), np.uint8))
    with pytest.raises(RuntimeError, match="GPU only"):                      # no CPU fallback
        DeviceVOCPartsMapper(False, (32,), 100, device="cpu")(rec)


# ------------------------------------------------------------------------------------------------ C-ABI
def test_sample_groups_rejects_bad_arguments_before_any_launch():
    """the argument checks of pd_rle_sample_groups_u8 come before the memsets and the launch, so they answer without a device"""
    import ctypes
    from partdistillation_amd import lib
    L = lib.load()
    limit = 1 << 20                                                        # PD_SAMPLE_GROUPS_MAX (include/pd_input.h)
    good = dict(n=3, H=33, W=70, out_h=12, out_w=9, n_groups=2)
    bad = {"negative n": dict(n=-1), "negative n_groups": dict(n_groups=-1), "n_groups above the limit": dict(n_groups=limit + 1),
           "H 0": dict(H=0), "W negative": dict(W=-5), "H * W over int32": dict(H=65536, W=32768), "out_h 0": dict(out_h=0),
           "out_w 0": dict(out_w=0), "out_h too large": dict(out_h=65536), "out_w too large": dict(out_w=65536), "null pointers": {},
           "null pointers without groups": dict(n_groups=0), "null pointers without members": dict(n=0)}
    for what, change in bad.items():
        a = dict(good, **change)
        rc = L.pd_rle_sample_groups_u8(None, None, a["n"], a["H"], a["W"], None, None, a["out_h"], a["out_w"], None, None, a["n_groups"],
                                       None, None, None, None)
        assert rc == -1 and "pd_rle_sample_groups_u8" in L.pd_last_error().decode(), what
        with pytest.raises(lib.PdHipError, match="null pointer" if what.startswith("null") else "bad sizes"):
            lib.check(rc)
    # each pointer on its own: everything else non-null (never dereferenced: the call returns before any launch)
    buf = (ctypes.c_int32 * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p).value
    names = ["starts", "offsets", "src_x", "src_y", "group_offsets", "group_members", "out", "member_area", "group_area"]
    for missing in names:
        v = {k: (None if k == missing else ptr) for k in names}
        rc = L.pd_rle_sample_groups_u8(v["starts"], v["offsets"], 3, 33, 70, v["src_x"], v["src_y"], 12, 9, v["group_offsets"],
                                       v["group_members"], 2, v["out"], v["member_area"], v["group_area"], None)
        assert rc == -1 and "null pointer" in L.pd_last_error().decode(), missing
    assert L.pd_rle_sample_groups_u8(None, None, 0, 33, 70, None, None, 12, 9, None, None, 0, None, None, None, None) == 0   # nothing to do
    assert lib.SIGNATURES["pd_rle_sample_groups_u8"][1][11] is ctypes.c_int and L.pd_cmd_fn_index(b"pd_rle_sample_groups_u8") >= 0


def test_wrapper_checks_the_member_range_before_upload():
    import torch
    from partdistillation_amd.functions.input_pipeline import rle_sample_groups
    z = torch.zeros(4, dtype=torch.int32)
    offsets = torch.tensor([0, 1, 2], dtype=torch.int32)                   # two members
    for members in ([0, 2], [-1, 0]):
        with pytest.raises(ValueError, match="member index"):
            rle_sample_groups(z, offsets, 4, 4, z, z, [0, 2], members)
    with pytest.raises(ValueError, match="CSR"):
        rle_sample_groups(z, offsets, 4, 4, z, z, [0, 3], [0, 1])
